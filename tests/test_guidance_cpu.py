"""CPU-only tests of classifier-free guidance: the C ABI additions (exported, bound, struct layout as the compiler sees it, the header
as C99, argument errors before any HIP call), the built guided kernels' scratch, Guidance validation, the CLI flags and the collator's
action dropout."""
import ctypes
import importlib.util
import os
import random
import shutil
import subprocess
from types import SimpleNamespace

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
NEW = ("genie_guidance_layout", "genie_sample_guided", "genie_guide_logits", "genie_maskgit_generate_guided",
       "genie_generate_cached_guided", "genie_generate_guided_workspace_bytes")


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    for base in ("genie_maskgit_generate", "genie_generate_cached"):   # the _ex signature plus a trailing genie_guidance*
        assert lib_mod.SIGNATURES[base + "_guided"][1][:-1] == lib_mod.SIGNATURES[base + "_ex"][1]
        assert lib_mod.SIGNATURES[base + "_guided"][1][-1] is ctypes.POINTER(lib_mod.Guidance)
    sg, se = lib_mod.SIGNATURES["genie_sample_guided"][1], lib_mod.SIGNATURES["genie_sample_ex"][1]
    assert sg == se[:2] + [lib_mod.c_ptr] + se[2:] + [ctypes.c_float]


def test_guidance_layout_matches_the_ctypes_struct():
    lib_mod, L = _lib()
    out = (ctypes.c_size_t * 3)()
    assert L.genie_guidance_layout(out, 3) == 3
    F = lib_mod.Guidance
    assert list(out) == [ctypes.sizeof(F), F.scale.offset, F.null_action.offset] == [8, 0, 4]
    assert L.genie_guidance_layout(None, 0) == 3


def test_header_with_the_guidance_additions_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    lib_mod, _ = _lib()
    src = tmp_path / "guid.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_guidance g = {3.0f, 2};\n"
                   "    int (*f)(const genie_cfg*, const float*, const float*, int, int, float, const float*, int64_t*, float*, void*,\n"
                   "             const genie_sampling*, float*, const float*, float, float) = genie_sample_guided;\n"
                   '    printf("%zu %zu %zu %d\\n", sizeof(genie_guidance), offsetof(genie_guidance, scale),\n'
                   "           offsetof(genie_guidance, null_action), (int)(g.null_action + (f != 0)));\n"
                   "    return 0;\n}\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), "-c", str(src),
                    "-o", str(tmp_path / "guid.o")], check=True)
    subprocess.run([gcc, str(tmp_path / "guid.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o",
                    str(tmp_path / "guid")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "guid")], capture_output=True, text=True, check=True).stdout.split()]
    F = lib_mod.Guidance
    assert out == [ctypes.sizeof(F), F.scale.offset, F.null_action.offset, 3]


def test_guided_workspace_covers_both_loops_at_twice_the_batch():
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())
    for B, P in ((1, 1), (3, 2), (4, 4)):
        n = L.genie_generate_guided_workspace_bytes(cfg, B, P)
        # (the passes run 2 B clips; the sample / confidence / flag scratch stays that of B)
        assert n > L.genie_generate_workspace_bytes(cfg, B, P) and n > L.genie_workspace_bytes(cfg, 2 * B)
    assert L.genie_generate_guided_workspace_bytes(cfg, 0, 1) == 0 and L.genie_generate_guided_workspace_bytes(cfg, 1, 5) == 0


def test_guided_entry_points_reject_bad_arguments_before_any_hip_call():
    """Guidance without a condition, null_action out of range, a non-finite scale: GENIE_E_ARG from host code (the fake device
    pointers are never dereferenced), also at a scale of 1 where the call would otherwise be the _ex entry point."""
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    fake = 1 << 20
    E = lib_mod.E_ARG
    nan, inf = float("nan"), float("inf")
    cond = lib_mod.FrameCond(table=fake, ids=fake, n_actions=5)
    uncond = lib_mod.FrameCond(table=0, ids=0, n_actions=0)

    def maskgit(c, g):
        return L.genie_maskgit_generate_guided(cfg, w, fake, 1, 1, 1, 0.0, 0, None, None, fake, None, 0, None, fake, 1 << 30, None, c,
                                               None, g)

    def cached(c, g):
        return L.genie_generate_cached_guided(cfg, w, fake, 1, 2, 1, 1, 0.0, 0, None, None, 0, 1, fake, None, fake, 1 << 30, fake,
                                              1 << 30, None, c, None, g)

    G = lib_mod.Guidance
    for call in (maskgit, cached):
        for c, g in ((None, G(3.0, 0)), (uncond, G(3.0, 0)), (cond, G(3.0, 5)), (cond, G(3.0, -1)), (cond, G(nan, 0)), (cond, G(inf, 0)),
                     (cond, G(-inf, 0)), (None, G(1.0, 0)), (cond, G(1.0, 9))):
            assert call(c, g) == E, (call.__name__, g.scale, g.null_action)
            assert b"guidance" in L.genie_last_error()
    for bad in (nan, inf):
        assert L.genie_sample_guided(cfg, fake, fake, 0, 1, 0.0, None, fake, fake, None, None, None, None, 0.0, bad) == E
        assert L.genie_guide_logits(fake, fake, fake, 16, bad, None) == E
    assert L.genie_sample_guided(cfg, fake, None, 0, 1, 0.0, None, fake, fake, None, None, None, None, 0.0, 3.0) == E


# ------------------------------------------------------------------ the built kernels
def test_guided_sample_kernels_use_no_scratch():
    """The guided Rows kernel combines its two 16-byte loads into the registers of the unguided one: no scratch, and within the
    register budget tests/test_sampling_cpu.py holds that one to; the strided one re-reads both rows per pass."""
    LLVM = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod, _ = _lib()
    rows = {r[0]: r for r in _tool("isa_audit").audit(lib_mod.LIB_PATH, all_kernels=True)}
    got = {k: v for k, v in rows.items() if "sample_guided" in k}
    assert any("sample_guided_rows_kernel<8>" in k for k in got) and any("sample_guided_kernel" in k for k in got), list(got)
    assert any("guide_logits_kernel" in k for k in rows)
    for name, r in got.items():
        assert r[6] == 0, f"{name}: {r[6]} bytes of scratch per lane"
        assert r[7] <= 128, f"{name}: {r[7]} registers (4 waves per SIMD need <= 128)"


# ------------------------------------------------------------------ Guidance and the CLI
def test_guidance_validation():
    S = pkg("sampling")
    g = S.Guidance(3.0, 2)
    st = g.to_struct()
    assert (st.scale, st.null_action) == (3.0, 2)
    for bad in ((float("nan"), 0), (float("inf"), 0), ("3", 0), (True, 0), (3.0, -1), (3.0, 1.5), (3.0, True), (3.0, None)):
        with pytest.raises(ValueError):
            S.Guidance(*bad)
    assert S.guidance_struct(None, 5) is None
    assert S.guidance_struct(S.Guidance(1.0, 2), 5) is None            # g = c: the unguided entry points
    assert S.guidance_struct(S.Guidance(0.0, 4), 5).null_action == 4
    with pytest.raises(IndexError):
        S.guidance_struct(S.Guidance(3.0, 5), 5)
    with pytest.raises(IndexError):
        S.guidance_struct(S.Guidance(1.0, 5), 5)
    with pytest.raises(ValueError):
        S.guidance_struct(S.Guidance(3.0, 0), 0)                        # a model without actions
    with pytest.raises(ValueError):
        S.guidance_struct((3.0, 0), 5)
    assert S.Guidance.from_args(SimpleNamespace(maskgit_steps=2)) is None
    assert S.Guidance.from_args(SimpleNamespace(guidance_scale=2.5, null_action=1)) == S.Guidance(2.5, 1)
    with pytest.raises(ValueError):
        S.Guidance.from_args(SimpleNamespace(guidance_scale=2.5, null_action=None))


def test_guidance_on_a_model_without_actions_raises():
    """Like action_ids today: checked on the host, before the device is touched."""
    S = pkg("sampling")
    m = pkg("st_mask_git").STMaskGIT(small_cfg())
    prompt = torch.zeros(1, 4, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        m.maskgit_generate(prompt, 1, guidance=S.Guidance(3.0, 0))
    with pytest.raises(ValueError):
        m.generate(prompt.view(1, -1)[:, :32], max_new_tokens=16, guidance=S.Guidance(3.0, 0))
    ma = pkg("st_mask_git").STMaskGIT(small_cfg(action_vocab_size=5))
    with pytest.raises(IndexError):
        ma.maskgit_generate(prompt, 1, guidance=S.Guidance(3.0, 5))
    with pytest.raises(ValueError):
        ma.maskgit_generate(prompt, 1, guidance=(3.0, 0))


def test_cli_flags_parse():
    S = pkg("sampling")
    ap = _tool("generate").build_parser()
    a = ap.parse_args(["--guidance_scale", "3", "--null_action", "0"])
    assert S.Guidance.from_args(a) == S.Guidance(3.0, 0)
    assert S.Guidance.from_args(ap.parse_args([])) is None
    for tool, flags in (("train", ("--action_dropout", "--null_action")), ("bench_generate", ("--guidance_scale",))):
        text = open(os.path.join(REPO, "tools", tool + ".py")).read()
        assert all(f in text for f in flags), tool


# ------------------------------------------------------------------ the collator's action dropout
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


def _clips(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.image_vocab_size, (B, cfg.T * cfg.S), generator=g)
    acts = torch.randint(0, cfg.action_vocab_size - 1, (B, cfg.T), generator=g)    # never the null action (the last row)
    return ids, acts


def test_action_dropout_with_replayed_draws():
    """The clips whose (replayed) uniform is below action_dropout, and only those, carry null_action at all T frames; tokens and labels
    are those of the run without dropout."""
    D = pkg("data")
    cfg = small_cfg(action_vocab_size=6, num_prompt_frames=2)
    B, null = 8, 5
    ids, acts = _clips(cfg, B, 3)
    torch.manual_seed(11)
    random.seed(11)
    rec = Recorder()
    base = D.maskgit_collate(ids, cfg, rec, action_ids=acts)
    u = torch.tensor([0.9, 0.1, 0.3, 0.29999, 0.0, 0.5, 0.31, 0.999])
    out = D.maskgit_collate(ids, cfg, Replay(rec.log + [u]), action_ids=acts, action_dropout=0.3, null_action=null)
    assert torch.equal(out["input_ids"], base["input_ids"]) and torch.equal(out["labels"], base["labels"])
    dropped = [1, 3, 4]
    for b in range(B):
        want = torch.full((cfg.T,), null) if b in dropped else acts[b]
        assert torch.equal(out["action_ids"][b], want), b
    # the draw is one (B,) uniform, taken after every other draw
    rec2 = Recorder()
    torch.manual_seed(11)
    random.seed(11)
    D.maskgit_collate(ids, cfg, rec2, action_ids=acts, action_dropout=0.3, null_action=null)
    assert len(rec2.log) == len(rec.log) + 1 and tuple(rec2.log[-1].shape) == (B,)
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(rec.log, rec2.log))
    # the collate_fn passes both options through
    feats = [{"input_ids": ids[b], "action_ids": acts[b]} for b in range(B)]
    got = D.get_maskgit_collator(cfg, action_dropout=1.0, null_action=null)(feats)
    assert (got["action_ids"] == null).all()
    for bad in (dict(action_dropout=0.5), dict(action_dropout=0.5, null_action=6), dict(action_dropout=1.5, null_action=0)):
        with pytest.raises(ValueError):
            D.maskgit_collate(ids, cfg, action_ids=acts, **bad)
    with pytest.raises(ValueError):
        D.maskgit_collate(ids, cfg, action_dropout=0.5, null_action=0)


def test_action_dropout_zero_draws_nothing():
    """action_dropout = 0: the same batch bit for bit and the same generator states afterwards as the call without the options."""
    D = pkg("data")
    cfg = small_cfg(action_vocab_size=6, num_prompt_frames=2)
    ids, acts = _clips(cfg, 4, 5)
    res = []
    for kw in (dict(), dict(action_dropout=0.0, null_action=5), dict(action_dropout=0.0)):
        torch.manual_seed(21)
        random.seed(21)
        out = D.maskgit_collate(ids, cfg, action_ids=acts, **kw)
        res.append((out, torch.get_rng_state(), random.getstate()))
    for out, ts, ps in res[1:]:
        assert out.keys() == res[0][0].keys()
        assert all(torch.equal(out[k], res[0][0][k]) for k in out)
        assert torch.equal(ts, res[0][1]) and ps == res[0][2]
    assert torch.equal(res[0][0]["action_ids"], acts)


def test_action_dropout_share_is_binomial():
    """4,096 clips at p = 0.25: the dropped share within 5 sigma of p (sigma = sqrt(p (1 - p) / N)); dropped clips are dropped whole."""
    D = pkg("data")
    cfg = small_cfg(action_vocab_size=6, num_prompt_frames=2)
    N, p, null = 4096, 0.25, 5
    ids, acts = _clips(cfg, N, 7)
    torch.manual_seed(31)
    random.seed(31)
    out = D.maskgit_collate(ids, cfg, action_ids=acts, action_dropout=p, null_action=null)["action_ids"]
    is_null = out == null
    assert (is_null.all(1) | ~is_null.any(1)).all()
    share = is_null.all(1).float().mean().item()
    sigma = np.sqrt(p * (1 - p) / N)
    print(f"dropped share {share:.4f} (p {p}, 5 sigma {5 * sigma:.4f})")
    assert abs(share - p) <= 5 * sigma, share
    assert torch.equal(out[~is_null.all(1)], acts[~is_null.all(1)])
