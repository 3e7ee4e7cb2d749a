"""CPU-only tests of continuous per-frame action vectors: the C ABI additions (declared, exported, bound, struct layout as the compiler
sees it, argument errors before any HIP call), the built kernels' scratch, the config field, the state-dict keys, the zero warm start,
the dataset's states.bin, the collator's dropout draw and Guidance without a null_action."""
import ctypes
import importlib.util
import json
import os
import random

import numpy as np
import pytest

from conftest import REPO, pkg

torch = pytest.importorskip("torch")


def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def small_cfg(**kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


# ------------------------------------------------------------------ C ABI
NEW = ("genie_action_proj_layout", "genie_action_rows", "genie_action_rows_backward")


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    assert "#define GENIE_ABI_VERSION 3" in header and "typedef struct genie_action_proj" in header
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    assert lib_mod.SIGNATURES["genie_action_rows"][1][0] is ctypes.POINTER(lib_mod.ActionProj)
    assert f"#define GENIE_ACTION_MAX_DIM {lib_mod.ACTION_MAX_DIM}" in header


def test_action_proj_layout_matches_the_ctypes_struct():
    lib_mod, L = _lib()
    out = (ctypes.c_size_t * 6)()
    assert L.genie_action_proj_layout(out, 6) == 6
    P = lib_mod.ActionProj
    assert list(out) == [ctypes.sizeof(P)] + [getattr(P, n).offset for n, _ in P._fields_]
    assert [n for n, _ in P._fields_] == ["weight", "bias", "mean", "inv_std", "action_dim"]
    assert L.genie_action_proj_layout(None, 0) == 6


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """Every check below returns from host code: the fake device pointers are never dereferenced, nothing is launched."""
    lib_mod, L = _lib()
    fake = 1 << 20
    E = lib_mod.E_ARG
    P = lib_mod.ActionProj

    def fwd(p, vecs=fake, rows=fake, n=4, d=64):
        return L.genie_action_rows(p, vecs, rows, n, d, None)

    def bwd(p, vecs=fake, d_rows=fake, n=4, d=64, dW=fake, db=fake):
        return L.genie_action_rows_backward(p, vecs, d_rows, n, d, dW, db, 0, None)

    good = P(weight=fake, bias=None, mean=None, inv_std=None, action_dim=3)
    assert fwd(None) == E and bwd(None) == E
    assert fwd(P(weight=None, action_dim=3)) == E
    assert fwd(good, vecs=None) == E and fwd(good, rows=None) == E
    assert bwd(good, vecs=None) == E and bwd(good, d_rows=None) == E and bwd(good, dW=None) == E
    for bad_dim in (0, -1):
        assert fwd(P(weight=fake, action_dim=bad_dim)) == E and bwd(P(weight=fake, action_dim=bad_dim)) == E
    assert fwd(good, d=0) == E and bwd(good, d=0) == E
    assert fwd(good, n=-1) == E and bwd(good, n=-1) == E
    assert b"genie_action_rows" in L.genie_last_error()
    # sizes beyond what the kernels cover: a shape error, still before any launch
    assert fwd(P(weight=fake, action_dim=lib_mod.ACTION_MAX_DIM + 1)) == lib_mod.E_SHAPE
    assert fwd(good, d=1025) == lib_mod.E_SHAPE and bwd(good, d=1025) == lib_mod.E_SHAPE
    # n == 0 is a successful no-op
    assert fwd(good, n=0) == 0 and bwd(good, n=0) == 0


def test_action_kernels_use_no_scratch():
    """The built code object (tools/isa_audit.py, as the sampler's kernels are checked): no scratch, and LDS only for the staged z."""
    LLVM = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod, _ = _lib()
    rows = {r[0]: r for r in _tool("isa_audit").audit(lib_mod.LIB_PATH, all_kernels=True)}
    got = {k: v for k, v in rows.items() if "action_rows" in k}
    assert any("action_rows_kernel" in k for k in got) and any("action_rows_bwd_kernel" in k for k in got), list(got)
    for name, r in got.items():
        assert r[6] == 0, f"{name}: {r[6]} bytes of scratch per lane"


# ------------------------------------------------------------------ config, state dict, warm start
def test_config_round_trip_and_the_two_kinds_exclude_each_other(tmp_path):
    C = pkg("config")
    c = small_cfg(action_dim=5)
    p = tmp_path / "config.json"
    c.save_pretrained(p)
    raw = json.loads(p.read_text())
    assert raw["action_dim"] == 5 and "action_vocab_size" not in raw
    assert C.GenieConfig.from_pretrained(p) == c and c.shallow_copy() == c
    c0 = small_cfg()
    assert c0.action_dim == 0 and "action_dim" not in c0.to_json_dict() and "action_dim" not in vars(c0)
    assert c0.shallow_copy() == c0 and c0 != c
    with pytest.raises(ValueError):
        small_cfg(action_dim=5, action_vocab_size=3)
    with pytest.raises(ValueError):
        small_cfg(action_dim=-1)


def test_state_dict_keys_and_synthetic_weights():
    c = small_cfg(action_dim=5)
    m = pkg("st_mask_git").STMaskGIT(c)
    new = {"action_proj.weight": (32, 5), "action_proj.bias": (32,), "action_null": (32,), "action_mean": (5,), "action_std": (5,)}
    sd = m.state_dict()
    base = set(pkg("st_mask_git").STMaskGIT(small_cfg()).state_dict())
    assert set(sd) == base | set(new)
    for k, shp in new.items():
        assert tuple(sd[k].shape) == shp, k
    assert {n for n, _ in m.named_parameters()} - base == {"action_proj.weight", "action_proj.bias", "action_null"}
    assert bool((sd["action_mean"] == 0).all()) and bool((sd["action_std"] == 1).all())
    syn = pkg("synthetic").make_state_dict(c, seed=1)
    assert set(syn) == set(sd)
    assert np.all(syn["action_mean"] == 0) and np.all(syn["action_std"] == 1) and np.any(syn["action_proj.weight"] != 0)
    m.load_numpy_state_dict(syn)
    # the tensors every other config has are the ones it had before
    syn0 = pkg("synthetic").make_state_dict(small_cfg(), seed=1)
    assert all(np.array_equal(syn[k], syn0[k]) for k in syn0)
    # set_action_stats
    m.set_action_stats(np.arange(5), np.arange(1, 6))
    assert m.action_std.tolist() == [1, 2, 3, 4, 5] and m.action_mean.tolist() == [0, 1, 2, 3, 4]
    for bad in ([1, 1, 0, 1, 1], [1, 1, -1, 1, 1], [1, 1, float("nan"), 1, 1], [1, 1, 1]):
        with pytest.raises(ValueError):
            m.set_action_stats(np.zeros(5), bad)
    with pytest.raises(ValueError):
        pkg("st_mask_git").STMaskGIT(small_cfg()).set_action_stats([0], [1])
    # the trainer's grouping knows the three names: weight decays, bias and null row do not; all three are on the embedding side
    T = pkg("train")
    order = T.ready_order(c, [n for n, _ in m.named_parameters()])
    assert set(order[-3:]) | {"action_null"} <= set(order) and all(T._embedding_side(n) for n in new if not n.endswith(("mean", "std")))
    assert T.decays("action_proj.weight") and not T.decays("action_proj.bias") and not T.decays("action_null")


def test_zero_warm_start_from_an_unconditioned_checkpoint(tmp_path):
    M = pkg("st_mask_git").STMaskGIT
    c0 = small_cfg()
    sd0 = pkg("synthetic").make_state_dict(c0, seed=2)
    M(c0).load_numpy_state_dict(sd0).save_pretrained(tmp_path / "ckpt")
    m = M.from_pretrained(tmp_path / "ckpt", action_dim=3)
    assert m.config.action_dim == 3 and m.config.action_vocab_size == 0
    sd = m.state_dict()
    for k in ("action_proj.weight", "action_proj.bias", "action_null", "action_mean"):
        assert not bool(sd[k].any()), k
    assert bool((sd["action_std"] == 1).all())
    for k, v in sd0.items():
        assert np.array_equal(sd[k].numpy(), v), k
    # round trip of the conditioned checkpoint; asking for another kind or size is refused
    m.save_pretrained(tmp_path / "ckpt_a")
    assert M.from_pretrained(tmp_path / "ckpt_a").config.action_dim == 3
    with pytest.raises(ValueError):
        M.from_pretrained(tmp_path / "ckpt_a", action_dim=4)
    with pytest.raises(ValueError):
        M.from_pretrained(tmp_path / "ckpt_a", action_vocab_size=4)


# ------------------------------------------------------------------ data
def test_dataset_round_trips_states_bin(tmp_path):
    D = pkg("data")
    g = np.random.default_rng(0)
    n, A = 12, 3
    tokens = g.integers(0, 1000, (n, 4, 4))
    vecs = g.standard_normal((n, A)).astype(np.float32)
    meta = D.write_token_dataset(tmp_path / "d", tokens, segment_ids=np.zeros(n, np.int32), action_vectors=vecs)
    assert meta["state_dim"] == A and (tmp_path / "d" / "states.bin").stat().st_size == n * A * 4
    ds = D.RawTokenDataset(tmp_path / "d", window_size=4, stride=2)
    item = ds[1]
    assert item["action_vectors"].dtype == torch.float32 and tuple(item["action_vectors"].shape) == (4, A)
    assert np.array_equal(item["action_vectors"].numpy(), vecs[1:8:2]) and "action_ids" not in item
    assert tuple(ds.action_vector_batch([0, 2]).shape) == (2, 4, A)
    # A from the file size when the metadata lacks the key
    raw = json.loads((tmp_path / "d" / "metadata.json").read_text())
    raw.pop("state_dim")
    (tmp_path / "d" / "metadata.json").write_text(json.dumps(raw))
    assert np.array_equal(D.RawTokenDataset(tmp_path / "d", window_size=4, stride=2)[1]["action_vectors"].numpy(), vecs[1:8:2])
    # no file: no key, and the batch helper says so
    D.write_token_dataset(tmp_path / "e", tokens, segment_ids=np.zeros(n, np.int32))
    de = D.RawTokenDataset(tmp_path / "e", window_size=4)
    assert "action_vectors" not in de[0]
    with pytest.raises(FileNotFoundError):
        de.action_vector_batch([0])
    for bad in (vecs[:-1], vecs[:, 0], np.where(np.arange(A) == 1, np.nan, vecs)):
        with pytest.raises(ValueError):
            D.write_token_dataset(tmp_path / "f", tokens, action_vectors=bad)


class Recorder:
    """data.TorchDraws that keeps every draw in call order."""

    def __init__(self):
        self.inner = pkg("data").TorchDraws("cpu")
        self.log = []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def call(*a):
            self.log.append(fn(*a))
            return self.log[-1]
        return call


class Replay:
    def __init__(self, log):
        self.log = list(log)

    def __getattr__(self, name):
        return lambda *a: self.log.pop(0)


def test_collator_passes_vectors_through_and_draws_the_dropout_last():
    D = pkg("data")
    cfg = small_cfg(action_dim=3, num_prompt_frames=2)
    B = 8
    g = np.random.default_rng(3)
    ids = torch.from_numpy(g.integers(0, cfg.image_vocab_size, (B, cfg.T * cfg.S)))
    vecs = torch.from_numpy(g.standard_normal((B, cfg.T, 3)))          # float64 in: float32 out
    torch.manual_seed(11)
    random.seed(11)
    rec = Recorder()
    base = D.maskgit_collate(ids, cfg, rec, action_vectors=vecs)
    assert base["action_vectors"].dtype == torch.float32 and torch.equal(base["action_vectors"], vecs.float())
    assert "action_drop" not in base and "action_ids" not in base
    u = torch.tensor([0.9, 0.1, 0.3, 0.29999, 0.0, 0.5, 0.31, 0.999])
    out = D.maskgit_collate(ids, cfg, Replay(rec.log + [u]), action_vectors=vecs, action_dropout=0.3)
    assert torch.equal(out["input_ids"], base["input_ids"]) and torch.equal(out["labels"], base["labels"])
    assert out["action_drop"].dtype == torch.bool and out["action_drop"].tolist() == [b in (1, 3, 4) for b in range(B)]
    assert torch.equal(out["action_vectors"], base["action_vectors"])           # the vectors themselves are untouched
    # one (B,) uniform, after every other draw; none at p = 0 (same generator states afterwards)
    rec2 = Recorder()
    torch.manual_seed(11)
    random.seed(11)
    D.maskgit_collate(ids, cfg, rec2, action_vectors=vecs, action_dropout=0.3)
    assert len(rec2.log) == len(rec.log) + 1 and tuple(rec2.log[-1].shape) == (B,)
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(rec.log, rec2.log))
    states = []
    for kw in (dict(), dict(action_dropout=0.0)):
        torch.manual_seed(21)
        random.seed(21)
        D.maskgit_collate(ids, cfg, action_vectors=vecs, **kw)
        states.append((torch.get_rng_state(), random.getstate()))
    assert torch.equal(states[0][0], states[1][0]) and states[0][1] == states[1][1]
    # the collate_fn passes both through; ids and vectors together are refused
    feats = [{"input_ids": ids[b], "action_vectors": vecs[b].float()} for b in range(B)]
    got = D.get_maskgit_collator(cfg, action_dropout=1.0)(feats)
    assert bool(got["action_drop"].all()) and tuple(got["action_vectors"].shape) == (B, cfg.T, 3)
    with pytest.raises(ValueError):
        D.maskgit_collate(ids, cfg, action_vectors=vecs, action_ids=torch.zeros(B, cfg.T, dtype=torch.long))


# ------------------------------------------------------------------ host-side argument checks of the model (no GPU needed to reach them)
def test_guidance_without_null_action_and_host_side_errors():
    S = pkg("sampling")
    g = S.Guidance(3.0)
    assert g.null_action is S.MODEL_NULL
    st = S.guidance_struct(g, null_row=0)
    assert (st.scale, st.null_action) == (3.0, 0)
    assert S.guidance_struct(S.Guidance(1.0), null_row=0) is None
    assert S.guidance_struct(S.Guidance(3.0, 0), null_row=0).null_action == 0
    with pytest.raises(ValueError):
        S.guidance_struct(S.Guidance(3.0, 2), null_row=0)       # the null row's index is the model's
    with pytest.raises(ValueError):
        S.guidance_struct(g, 5)                                  # a model conditioned on ids needs null_action
    with pytest.raises(ValueError):
        g.to_struct()
    M = pkg("st_mask_git").STMaskGIT
    mv, mi = M(small_cfg(action_dim=3)), M(small_cfg(action_vocab_size=5))
    prompt = torch.zeros(1, 4, 4, 4, dtype=torch.long)
    ids, vec = torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 4, 3)
    for m, kw in ((mv, dict(action_ids=ids)), (mi, dict(action_vectors=vec)), (mv, dict(action_ids=ids, action_vectors=vec)), (mv, {})):
        with pytest.raises(ValueError):
            m._check_cond(kw.get("action_ids"), 1, kw.get("action_vectors"))
    with pytest.raises(RuntimeError):
        mv._check_cond(None, 1, torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError):
        mv._check_cond(None, 1, torch.zeros(1, 4, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        mv._check_cond(None, 1, torch.full((1, 4, 3), float("inf")))
    with pytest.raises(ValueError):
        mv.maskgit_generate(prompt, 1, action_vectors=vec, guidance=S.Guidance(3.0, 1))
    for tool, flag in (("train", "--action_dim"), ("bench_generate", "--action_dim")):
        assert flag in open(os.path.join(REPO, "tools", tool + ".py")).read(), tool
