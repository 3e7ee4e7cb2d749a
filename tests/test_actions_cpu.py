"""CPU-only tests of per-frame action conditioning: config and checkpoint round trips, the dataset's actions.bin, the collator,
state-dict keys, the warm start from an unconditioned checkpoint, and the C ABI of the *_cond entry points (exported, struct
layout as the compiler sees it, argument errors before any HIP call)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import REPO, pkg

# the fields of the reference's GenieConfig dataclass: its from_pretrained is cls(**config), so a config.json may hold no other key
REFERENCE_CONFIG_FIELDS = {
    "num_layers", "num_heads", "d_model", "T", "S", "image_vocab_size", "use_mup", "num_factored_vocabs", "factored_vocab_size",
    "max_corrupt_rate", "non_mlm_ratio", "num_prompt_frames", "qkv_bias", "proj_bias", "attn_drop", "qk_norm", "mlp_ratio",
    "mlp_drop", "mlp_bias"}


def small_cfg(A=0, **kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False, action_vocab_size=A)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


def test_config_roundtrip_with_actions(tmp_path):
    C = pkg("config")
    c = small_cfg(A=7)
    p = tmp_path / "config.json"
    c.save_pretrained(p)
    assert json.loads(p.read_text())["action_vocab_size"] == 7
    assert C.GenieConfig.from_pretrained(p) == c
    assert c.shallow_copy() == c


def test_unconditioned_config_json_has_no_new_key(tmp_path):
    c = small_cfg(A=0)
    assert c.action_vocab_size == 0
    p = tmp_path / "config.json"
    c.save_pretrained(p)
    raw = json.loads(p.read_text())
    assert "action_vocab_size" not in raw
    assert set(raw) <= REFERENCE_CONFIG_FIELDS
    # byte-identical to what the field list without the new key dumps
    legacy = {k: v for k, v in vars(c).items() if k != "action_vocab_size"}
    assert p.read_text() == json.dumps(legacy)
    # the model's checkpoint writer too
    M = pkg("st_mask_git").STMaskGIT
    m = M(c).load_numpy_state_dict(pkg("synthetic").make_state_dict(c, seed=1))
    m.save_pretrained(tmp_path / "ckpt")
    raw = json.loads((tmp_path / "ckpt" / "config.json").read_text())
    assert set(raw) <= REFERENCE_CONFIG_FIELDS and "action_vocab_size" not in raw


def test_action_checkpoint_roundtrip(tmp_path):
    S = pkg("synthetic")
    M = pkg("st_mask_git").STMaskGIT
    c = small_cfg(A=5)
    m = M(c).load_numpy_state_dict(S.make_state_dict(c, seed=2))
    m.save_pretrained(tmp_path)
    m2 = M.from_pretrained(tmp_path)
    assert m2.config == c
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    with pytest.raises(ValueError):
        M.from_pretrained(tmp_path, action_vocab_size=6)


@pytest.mark.parametrize("A", [0, 9])
@pytest.mark.parametrize("qk_norm", [False, True])
def test_state_dict_keys_match_the_synthetic_spec(A, qk_norm):
    S = pkg("synthetic")
    c = small_cfg(A=A, qk_norm=qk_norm)
    m = pkg("st_mask_git").STMaskGIT(c)
    spec = S.state_dict_spec(c)
    assert list(m.state_dict()) == [k for k, _, _, _ in spec]
    assert all(tuple(m.state_dict()[k].shape) == tuple(s) for k, s, _, _ in spec)
    assert ("action_embed.weight" in m.state_dict()) == (A > 0)
    if A:
        assert tuple(m.state_dict()["action_embed.weight"].shape) == (A, c.d_model)
    # A == 0: the spec is today's (no action key anywhere)
    base = S.state_dict_spec(small_cfg(A=0, qk_norm=qk_norm))
    assert spec[:len(base)] == base


def test_init_weights_draws_the_action_table():
    torch.manual_seed(0)
    m = pkg("st_mask_git").STMaskGIT(small_cfg(A=4))
    m.action_embed.weight.data.zero_()
    m.init_weights()
    w = m.action_embed.weight
    assert float(w.abs().max()) > 0 and abs(float(w.std()) - 0.02) < 0.01


def test_warm_start_from_an_unconditioned_checkpoint(tmp_path):
    S = pkg("synthetic")
    M = pkg("st_mask_git").STMaskGIT
    c0 = small_cfg(A=0)
    m0 = M(c0).load_numpy_state_dict(S.make_state_dict(c0, seed=3))
    m0.save_pretrained(tmp_path)
    m = M.from_pretrained(tmp_path, action_vocab_size=6)
    assert m.config.action_vocab_size == 6
    sd, sd0 = m.state_dict(), m0.state_dict()
    assert set(sd) == set(sd0) | {"action_embed.weight"}
    assert torch.equal(sd["action_embed.weight"], torch.zeros(6, c0.d_model))
    assert all(torch.equal(sd0[k], sd[k]) for k in sd0)
    # every stored key stays strict: a checkpoint missing a tensor still fails
    from safetensors.torch import load_file, save_file
    broken = load_file(os.path.join(tmp_path, "model.safetensors"))
    broken.pop("out_x_proj.bias")
    save_file(broken, os.path.join(tmp_path, "model.safetensors"))
    with pytest.raises(RuntimeError):
        M.from_pretrained(tmp_path, action_vocab_size=6)


def test_action_argument_errors_on_the_host():
    """The checks of STMaskGIT._cond run on the host before anything else (no GPU needed to reach them)."""
    M = pkg("st_mask_git").STMaskGIT
    plain = M(small_cfg(A=0))
    with pytest.raises(ValueError):
        plain._cond(torch.zeros(1, 4, dtype=torch.long), 1)
    assert plain._cond(None, 1) is None
    m = M(small_cfg(A=3))
    with pytest.raises(ValueError):
        m._cond(None, 1)
    with pytest.raises(RuntimeError):
        m._cond(torch.zeros(1, 5, dtype=torch.long), 1)
    with pytest.raises(RuntimeError):
        m._cond(torch.zeros(2, 4, dtype=torch.long), 1)
    with pytest.raises(RuntimeError):
        m._cond(torch.zeros(1, 4), 1)
    with pytest.raises(IndexError):
        m._cond(torch.tensor([[0, 1, 3, 0]]), 1)
    with pytest.raises(IndexError):
        m._cond(torch.tensor([[0, -1, 0, 0]]), 1)


# ------------------------------------------------------------------ data
def _write(tmp_path, n=40, side=4, actions=True, seed=0):
    D = pkg("data")
    g = np.random.default_rng(seed)
    tokens = g.integers(0, 262144, size=(n, side, side))
    acts = g.integers(0, 65536, size=(n,)) if actions else None
    D.write_token_dataset(tmp_path, tokens, segment_ids=np.zeros(n, np.int32), actions=acts)
    return tokens, acts


@pytest.mark.parametrize("stride", [1, 3])
def test_dataset_reads_actions_aligned_with_frames(tmp_path, stride):
    D = pkg("data")
    tokens, acts = _write(tmp_path)
    assert (tmp_path / "actions.bin").stat().st_size == 2 * len(acts)
    ds = D.RawTokenDataset(tmp_path, window_size=4, stride=stride)
    assert len(ds) > 3
    for idx in (0, 1, len(ds) - 1):
        item = ds[idx]
        start = ds.valid_start_inds[idx]
        frames = list(range(start, start + 3 * stride + 1, stride))
        assert item["action_ids"].dtype == torch.int64 and item["action_ids"].shape == (4,)
        assert item["action_ids"].tolist() == [int(acts[f]) for f in frames]
        assert torch.equal(item["input_ids"], torch.from_numpy(tokens[frames].astype(np.int64)).flatten())


def test_dataset_without_actions_keeps_todays_keys(tmp_path):
    D = pkg("data")
    _write(tmp_path, actions=False)
    assert not (tmp_path / "actions.bin").exists()
    ds = D.RawTokenDataset(tmp_path, window_size=4)
    assert ds.actions is None
    assert sorted(ds[0]) == ["attention_mask", "input_ids", "labels"]


def test_write_token_dataset_rejects_bad_actions(tmp_path):
    D = pkg("data")
    with pytest.raises(ValueError):
        D.write_token_dataset(tmp_path, np.zeros((5, 2, 2)), actions=np.zeros(4))
    with pytest.raises(ValueError):
        D.write_token_dataset(tmp_path, np.zeros((5, 2, 2)), actions=np.full(5, 70000))


def test_collator_passes_actions_through_with_the_same_draws(tmp_path):
    D = pkg("data")
    c = small_cfg(A=11, non_mlm_ratio=0.5, num_prompt_frames=2)
    _write(tmp_path, n=60, side=4, seed=4)
    ds = D.RawTokenDataset(tmp_path, window_size=c.T, stride=2)
    feats = [ds[i] for i in range(6)]
    collate = D.get_maskgit_collator(c)
    for seed in range(6):   # both branches of the non-MLM draw
        torch.manual_seed(seed)
        random.seed(seed)
        with_a = collate(feats)
        torch.manual_seed(seed)
        random.seed(seed)
        without = collate([{k: v for k, v in f.items() if k != "action_ids"} for f in feats])
        assert sorted(without) == ["input_ids", "labels"]
        assert torch.equal(with_a["input_ids"], without["input_ids"])
        assert torch.equal(with_a["labels"], without["labels"])
        assert torch.equal(with_a["action_ids"], torch.stack([f["action_ids"] for f in feats]))
        assert with_a["action_ids"].dtype == torch.int64


# ------------------------------------------------------------------ C ABI
COND_NAMES = ["genie_embed_cond", "genie_compute_logits_cond", "genie_maskgit_generate_cond", "genie_clean_pass_cond",
              "genie_masked_frames_logits_cond", "genie_frame_pass_cond", "genie_frames_pass_cond", "genie_generate_cached_cond",
              "genie_train_forward_cond", "genie_train_backward_embed_cond"]


def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def test_cond_symbols_are_exported():
    lib_mod, L = _lib()
    for n in COND_NAMES:
        assert hasattr(L, n), n
        assert n in lib_mod.SIGNATURES, n
        base = n[: -len("_cond")]
        if base != "genie_train_backward_embed":
            # the plain argument list + one trailing genie_frame_cond*
            assert lib_mod.SIGNATURES[n][1][:-1] == lib_mod.SIGNATURES[base][1]
            assert lib_mod.SIGNATURES[n][1][-1] is ctypes.POINTER(lib_mod.FrameCond)
    assert L.genie_version() == 3


def test_frame_cond_layout_matches_the_compiler(tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib_mod, _ = _lib()
    src = tmp_path / "cond.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu\\n", sizeof(genie_frame_cond), offsetof(genie_frame_cond, table),\n'
                   "           offsetof(genie_frame_cond, ids), offsetof(genie_frame_cond, n_actions));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "cond"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F = lib_mod.FrameCond
    assert out == [ctypes.sizeof(F), F.table.offset, F.ids.offset, F.n_actions.offset]


def test_cond_entry_points_reject_bad_arguments_before_any_hip_call():
    """Every check below returns GENIE_E_ARG from host code: the fake device pointers are never dereferenced."""
    lib_mod, L = _lib()
    c = small_cfg(A=3)
    cfg = lib_mod.make_cfg(c)
    w = lib_mod.Weights()
    fake = 1 << 20   # never read
    bad = lib_mod.FrameCond(table=None, ids=fake, n_actions=3)
    neg = lib_mod.FrameCond(table=fake, ids=fake, n_actions=-1)
    E = lib_mod.E_ARG
    # NULL pointers
    assert L.genie_compute_logits_cond(cfg, w, None, 1, 0, 1, 0, None, None, 0, None, None) == E
    assert L.genie_embed_cond(cfg, w, None, 1, None, None, None) == E
    # a frame condition without a table, or with a negative count
    w.pos_embed = w.mask_embed = fake
    w.embed[0] = w.embed[1] = fake
    for fc in (bad, neg):
        assert L.genie_embed_cond(cfg, w, fake, 1, fake, None, fc) == E
        assert b"frame condition" in L.genie_last_error() or b"n_actions" in L.genie_last_error()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    assert L.genie_compute_logits_cond(cfg, w, fake, 1, 0, 1, 0, fake, fake, 1 << 30, None, bad) == E
    assert L.genie_maskgit_generate_cond(cfg, w, fake, 1, 1, 1, 0.0, 0, None, None, fake, None, 0, None, fake, 1 << 30, None,
                                         bad) == E
    assert L.genie_clean_pass_cond(cfg, w, fake, 1, 2, 2, fake, 1 << 30, fake, 1 << 30, None, bad) == E
    assert L.genie_masked_frames_logits_cond(cfg, w, fake, 1, 1, 2, fake, 1 << 30, fake, fake, 1 << 30, None, bad) == E
    assert L.genie_frames_pass_cond(cfg, w, fake, 1, 0, 1, fake, 1 << 30, None, fake, 1 << 30, None, bad) == E
    assert L.genie_frame_pass_cond(cfg, w, fake, 1, 0, fake, 1 << 30, None, fake, 1 << 30, None, bad) == E
    assert L.genie_generate_cached_cond(cfg, w, fake, 1, 2, 1, 1, 0.0, 0, None, None, 0, 1, fake, None, fake, 1 << 30, fake,
                                        1 << 30, None, bad) == E
    assert L.genie_train_forward_cond(cfg, w, fake, fake, 1, fake, 1 << 30, fake, None, bad) == E
    good = lib_mod.FrameCond(table=fake, ids=fake, n_actions=3)
    g = lib_mod.Weights()
    assert L.genie_train_backward_embed_cond(cfg, g, fake, 1, fake, 1 << 30, 0, None, fake, bad) == E
    # actions without a gradient buffer for the table
    assert L.genie_train_backward_embed_cond(cfg, g, fake, 1, fake, 1 << 30, 0, None, None, good) == E
    assert b"d_table" in L.genie_last_error()
