"""LoRA adapters, the part that runs anywhere (include/genie_hip.h, "LoRA adapters"; 1xgpt_amd/lora.py; GenieTrainer(lora=...)): the C ABI
and its host-side refusals, LoraConfig, target selection, the flat layout with adapter names, the adapter files, and the float64 model of
tests/lora_model.py against torch CPU autograd.  tests/test_hip_train_lora.py holds the GPU side."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lora_model as LM
from conftest import REPO, pkg
from test_train_frozen_cpu import cfg3, numels


def lib_and_mod():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod.load(), lib_mod


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_is_c99_and_exports_the_lora_symbols(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib, lib_mod = lib_and_mod()
    for name in ("genie_lora_layout", "genie_lora_merge", "genie_lora_project_scratch_bytes", "genie_lora_project"):
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
    assert lib.genie_version() == 3 == lib_mod.ABI_VERSION
    assert "LoRA adapters" in open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = tmp_path / "lora.c"
    src.write_text('#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_lora_item it[2]; size_t lay[12];\n"
                   "    memset(it, 0, sizeof it);\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3) return 1;\n"
                   "    if (genie_lora_layout(lay, 12) != 12 || lay[0] != sizeof(genie_lora_item)) return 2;\n"
                   "    if (genie_lora_merge(0, 1, 0) != GENIE_E_ARG) return 3;\n"
                   "    if (genie_lora_merge(it, 0, 0) != GENIE_E_ARG || genie_lora_merge(it, GENIE_LORA_MAX_ITEMS + 1, 0) != GENIE_E_ARG) return 4;\n"
                   "    if (genie_lora_project(it, 1, 0, 0, 0, 0) != GENIE_E_ARG) return 5;\n"
                   "    if (strstr(genie_last_error(), \"rank\") == 0) return 6;\n"
                   "    if (genie_lora_project_scratch_bytes(it, 1) != 0) return 7;\n"
                   "    return 0;\n}\n")
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "lora.o")], check=True)
    exe = tmp_path / "lora"
    subprocess.run([gcc, str(tmp_path / "lora.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_struct_layout_matches_ctypes():
    lib, lib_mod = lib_and_mod()
    lay = (C.c_size_t * 12)()
    assert lib.genie_lora_layout(lay, 12) == 12
    It = lib_mod.LoraItem
    assert list(lay) == [C.sizeof(It)] + [getattr(It, n).offset for n, _ in It._fields_]
    assert lib.genie_lora_layout(None, 12) == 12


# pointers that are never dereferenced: every refusal below happens on the host, before the device or the stream is touched
W, W0, A, B, DW, DA, DB, SCR = (0x10000000 * k for k in range(1, 9))


def good(**kw):
    lib_mod = pkg("_lib")
    f = dict(w=W, w0=W0, a=A, b=B, dw=DW, da=DA, db=DB, out=48, in_=32, rank=4, scale=2.0)
    f.update(kw)
    return lib_mod.LoraItem(**f)


def arr(*items):
    return (pkg("_lib").LoraItem * len(items))(*items), len(items)


REFUSALS = [
    ("rank 0", dict(rank=0), "rank 0 is not in 1 .. 64"),
    ("rank 65", dict(rank=65), "rank 65 is not in 1 .. 64"),
    ("in 24", dict(in_=24), "in = 24 is not a positive multiple of 16"),
    ("in 0", dict(in_=0), "in = 0 is not a positive multiple of 16"),
    ("out 0", dict(out=0), "out = 0"),
    ("inf scale", dict(scale=float("inf")), "scale is not finite"),
    ("nan scale", dict(scale=float("nan")), "scale is not finite"),
    ("NULL a", dict(a=None), "NULL a or b"),
    ("NULL b", dict(b=None), "NULL a or b"),
]


@pytest.mark.parametrize("what,change,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_both_calls_refuse(what, change, msg):
    lib, lib_mod = lib_and_mod()
    items, n = arr(good(), good(**change))   # the bad item is the second: every item is checked before anything is launched
    assert lib.genie_lora_merge(items, n, None) == lib_mod.E_ARG
    assert msg in lib.genie_last_error().decode() and "item 1" in lib.genie_last_error().decode()
    assert lib.genie_lora_project(items, n, 0, SCR, 1 << 30, None) == lib_mod.E_ARG
    assert msg in lib.genie_last_error().decode()
    assert lib.genie_lora_project_scratch_bytes(items, n) == 0


def test_merge_refusals():
    lib, lib_mod = lib_and_mod()
    E = lib_mod.E_ARG
    err = lambda: lib.genie_last_error().decode()   # noqa: E731
    assert lib.genie_lora_merge(None, 1, None) == E and "NULL items" in err()
    for n in (0, -1, 9):
        assert lib.genie_lora_merge(arr(*[good()] * 8)[0], n, None) == E and "is not in 1 .. 8" in err()
    for f in ("w", "w0"):
        assert lib.genie_lora_merge(*arr(good(**{f: None})), None) == E and "NULL w or w0" in err()
    assert lib.genie_lora_merge(*arr(good(w0=W0 + 4)), None) == E and "16-byte aligned" in err()
    assert lib.genie_lora_merge(*arr(good(w=W0 + 64)), None) == E and "overlaps w0 without being w0" in err()
    assert lib.genie_lora_merge(*arr(good(a=W + 4 * 48 * 32 - 16)), None) == E and "a or b overlaps the output w" in err()
    assert lib.genie_lora_merge(*arr(good(b=W)), None) == E and "a or b overlaps the output w" in err()
    assert lib.genie_lora_merge(*arr(good(w=W0, a=W0)), None) == E and "a or b overlaps the output w" in err()


def test_project_refusals_and_scratch_size():
    lib, lib_mod = lib_and_mod()
    E = lib_mod.E_ARG
    err = lambda: lib.genie_last_error().decode()   # noqa: E731
    items, n = arr(good(), good(out=130, in_=80, rank=5))
    # slabs: dA one (rank, in) per 64 rows, dB one (out, rank) per 64 columns, each run rounded up to 64 floats
    pad = lambda x: (x + 63) // 64 * 64   # noqa: E731
    want = 4 * (pad(1 * 4 * 32) + pad(1 * 48 * 4) + pad(3 * 5 * 80) + pad(2 * 130 * 5))
    need = lib.genie_lora_project_scratch_bytes(items, n)
    assert need == want
    assert lib.genie_lora_project(items, n, 0, SCR, need - 1, None) == E and f"{need} needed" in err()
    assert lib.genie_lora_project(items, n, 0, None, need, None) == E and "scratch" in err()
    assert lib.genie_lora_project(None, 1, 0, SCR, need, None) == E and "NULL items" in err()
    assert lib.genie_lora_project(items, 9, 0, SCR, need, None) == E and "is not in 1 .. 8" in err()
    for f in ("dw", "da", "db"):
        assert lib.genie_lora_project(*arr(good(**{f: None})), 0, SCR, need, None) == E and "NULL dw, da or db" in err()
    assert lib.genie_lora_project(*arr(good(da=A)), 0, SCR, need, None) == E and "a or b overlaps an output" in err()
    assert lib.genie_lora_project(*arr(good(db=B + 16)), 0, SCR, need, None) == E and "a or b overlaps an output" in err()
    assert lib.genie_lora_project(*arr(good(da=DW)), 0, SCR, need, None) == E and "dw, da and db overlap" in err()
    assert lib.genie_lora_project(*arr(good()), 0, DW, need, None) == E and "scratch overlaps" in err()
    assert lib.genie_lora_project(*arr(good(dw=DW + 4)), 0, SCR, need, None) == E and "16-byte aligned" in err()


# ---------------------------------------------------------------------------------------------- LoraConfig and the targets
def test_lora_config_validation():
    LC = pkg("train").LoraConfig
    c = LC(rank=4, alpha=8, targets="decoder.layers.0.*,out_x_proj.weight", seed=3)
    assert (c.rank, c.alpha, c.targets, c.seed, c.scale) == (4, 8.0, ["decoder.layers.0.*", "out_x_proj.weight"], 3, 2.0)
    assert LC().targets == ["decoder.layers.*"] and LC(targets=["a", "b"]).targets == ["a", "b"]
    for bad in (0, 65, -1, 2.5, True, "8"):
        with pytest.raises(ValueError, match="rank"):
            LC(rank=bad)
    for bad in (float("inf"), float("nan"), 1e40):   # (alpha / rank leaves f32)
        with pytest.raises(ValueError, match="alpha"):
            LC(alpha=bad)
    for bad in ("", [], None, [3]):
        with pytest.raises(ValueError, match="targets"):
            LC(targets=bad)


def test_target_selection():
    L = pkg("lora")
    cfg = cfg3()
    lin = pkg("train").linear_weight_names(cfg)
    assert len(lin) == 19 and lin == L.linear_weight_names(cfg)
    assert L.select_targets(cfg, ["decoder.layers.*"]) == lin[:-1]
    assert L.select_targets(cfg, ["out_x_proj.weight", "decoder.layers.1.mlp.*"]) == [
        "decoder.layers.1.mlp.fc1.weight", "decoder.layers.1.mlp.fc2.weight", "out_x_proj.weight"]
    assert L.select_targets(cfg, ["*"]) == lin
    for bad in ("decoder.layers.3.*", "out_x_proj.bias", "*.norm1.weight", "pos_embed_TSC"):   # biases, norms, embeddings: no targets
        with pytest.raises(ValueError, match="matches no Linear weight"):
            L.select_targets(cfg, ["decoder.layers.0.*", bad])
    assert L.adapter_names("decoder.layers.3.mlp.fc1.weight") == ("decoder.layers.3.mlp.fc1.lora_A", "decoder.layers.3.mlp.fc1.lora_B")


def test_initial_draw():
    L = pkg("lora")
    a = L.draw_a("decoder.layers.0.mlp.fc1.lora_A", (8, 64), 0)
    assert a.dtype == np.float32 and a.shape == (8, 64) and np.abs(a).max() <= 1 / 8 and np.abs(a).max() > 0.11 and abs(a.mean()) < 0.02
    assert np.array_equal(a, L.draw_a("decoder.layers.0.mlp.fc1.lora_A", (8, 64), 0))
    assert not np.array_equal(a, L.draw_a("decoder.layers.0.mlp.fc1.lora_A", (8, 64), 1))
    assert not np.array_equal(a, L.draw_a("decoder.layers.1.mlp.fc1.lora_A", (8, 64), 0))


# ---------------------------------------------------------------------------------------------- the flat layout with adapter names
def lora_layout(targets, rank=4, extra=None, cfg=None):
    T, L = pkg("train"), pkg("lora")
    cfg = cfg or cfg3()
    n = numels(cfg)
    shapes = {k: tuple(shape) for k, shape, *_ in pkg("synthetic").state_dict_spec(cfg)}
    names = L.select_targets(cfg, targets)
    ad = L.adapter_shapes(names, shapes, rank)
    allnum = dict(n, **{k: int(np.prod(s)) for k, s in ad.items()})
    chosen = set(ad) | (T.select_trainable(n, extra) if extra else set())
    return cfg, ad, allnum, T.FlatLayout(cfg, allnum, chosen)


def test_layout_with_adapters():
    cfg, ad, n, lay = lora_layout(["decoder.layers.[12].*"])
    pad = lambda x: (x + 63) // 64 * 64   # noqa: E731
    assert lay.trainable == set(ad) and len(ad) == 2 * 12 and not lay.all
    assert lay.n_train == sum(pad(n[k]) for k in ad)                        # adapter elements alone
    assert lay.order[:len(ad)] == [k for k in lay.order if k in ad]         # the trainable prefix
    assert [k for k, _, _ in lay.groups] == [2, 1] and lay.stop == 1 and not lay.embed
    assert lay.segments == [(lo, hi) for _, lo, hi in lay.groups] and lay.segments[-1][1] == lay.n_train
    assert len(lay.adam_runs) == 1 and lay.adam_runs[0][:3] == (0, lay.n_train, True)   # adapters decay as weights: one AdamW range
    assert all(k.startswith("decoder.layers.2.") for k in lay.order[:12]) and all(k.startswith("decoder.layers.1.") for k in lay.order[12:24])
    # every tensor has its place, 256-byte aligned, and the frozen base weights come behind the prefix
    assert all(lay.offsets[k][0] % 64 == 0 for k in n) and lay.offsets["decoder.layers.2.mlp.fc1.weight"][0] >= lay.n_train
    assert lay.n_flat == sum(pad(v) for v in n.values())


def test_layout_stop_and_groups_follow_the_lowest_adapted_layer():
    assert lora_layout(["out_x_proj.weight"])[3].stop == 3
    _, _, _, lay = lora_layout(["out_x_proj.weight"])
    assert [k for k, _, _ in lay.groups] == ["head"]
    _, _, _, lay = lora_layout(["decoder.layers.0.mlp.fc1.weight", "out_x_proj.weight"])
    assert lay.stop == 0 and [k for k, _, _ in lay.groups] == ["head", 0]
    # adapters beside fully trained action tensors: the embedding side is a group of its own and the backward runs to layer 0
    cfg, ad, n, lay = lora_layout(["decoder.layers.2.*"], extra="action_*", cfg=cfg3(action_dim=3))
    assert [k for k, _, _ in lay.groups] == [2, "embed"] and lay.stop == 0 and lay.embed
    assert lay.trainable == set(ad) | {"action_proj.weight", "action_proj.bias", "action_null"}
    assert len(lay.adam_runs) == 2   # the decaying run (adapters, action_proj.weight) and the bias-like tail


def test_lr_scale_patterns_reach_the_adapters():
    T = pkg("train")
    cfg, ad, n, _ = lora_layout(["decoder.layers.2.mlp.*"])
    lay = T.FlatLayout(cfg, n, set(ad), {"*.lora_B": 4.0})
    assert {r[3] for r in lay.adam_runs} == {1.0, 4.0} and lay.lr_factor["decoder.layers.2.mlp.fc1.lora_B"] == 4.0


def test_resource_counts_beside_the_full_fine_tune():
    """What DESIGN.md records: trainable elements, optimizer-state bytes, all-reduce bytes and AdamW launches, from the layout."""
    cfg, ad, n, lay = lora_layout(["decoder.layers.*"], rank=4)
    full = pkg("train").FlatLayout(cfg, numels(cfg))
    assert lay.n_train < full.n_train == full.n_flat < lay.n_flat   # (the flat buffer also holds the adapters; W0 is a buffer of its own)
    assert len(lay.adam_runs) == 1 and len(full.adam_runs) == 2 * (cfg.num_layers + 1) + 1
    assert len(lay.segments) == cfg.num_layers and len(full.segments) == cfg.num_layers + 2


# ---------------------------------------------------------------------------------------------- adapter files
def test_adapter_config_round_trip_and_mismatched_base(tmp_path):
    L = pkg("lora")
    cfg = cfg3()
    shapes = {k: tuple(shape) for k, shape, *_ in pkg("synthetic").state_dict_spec(cfg)}
    lc = L.LoraConfig(rank=3, alpha=6.0, targets="decoder.layers.1.*")
    targets = L.select_targets(cfg, lc.targets)
    tensors = {k: torch.randn(s) for k, s in L.adapter_shapes(targets, shapes, lc.rank).items()}
    ac = L.adapter_config(lc, targets, cfg)
    assert ac == {"rank": 3, "alpha": 6.0, "targets": targets, "base": {k: getattr(cfg, k) for k in L.BASE_FIELDS}}
    L.save_adapter(str(tmp_path / "ad"), ac, tensors)
    assert sorted(os.listdir(tmp_path / "ad")) == ["adapter.safetensors", "adapter_config.json"]
    assert json.load(open(tmp_path / "ad" / "adapter_config.json")) == ac
    got_cfg, got = L.load_adapter_files(str(tmp_path / "ad"))
    assert got_cfg == ac and set(got) == set(tensors) and all(torch.equal(got[k], tensors[k]) for k in got)
    assert L.check_adapter(got_cfg, got, cfg, shapes) == (3, 2.0, targets)
    # a base that differs in a shape field, a target the base lacks, a missing tensor, a wrong shape
    for other in (cfg3(d_model=128), cfg3(num_layers=2), cfg3(num_factored_vocabs=3)):
        with pytest.raises(ValueError, match="another base model"):
            L.check_adapter(got_cfg, got, other, {k: tuple(s) for k, s, *_ in pkg("synthetic").state_dict_spec(other)})
    with pytest.raises(ValueError, match="not Linear weights of this model"):
        L.check_adapter(dict(ac, targets=targets + ["decoder.layers.1.norm1.weight"]), got, cfg, shapes)
    with pytest.raises(ValueError, match="missing"):
        L.check_adapter(ac, {k: v for k, v in got.items() if not k.endswith("fc1.lora_B")}, cfg, shapes)
    with pytest.raises(ValueError, match="has shape"):
        L.check_adapter(ac, dict(got, **{"decoder.layers.1.mlp.fc1.lora_A": torch.zeros(4, 64)}), cfg, shapes)
    with pytest.raises(ValueError, match="incomplete"):
        L.check_adapter({"rank": 3}, got, cfg, shapes)
    with pytest.raises(FileNotFoundError):
        L.load_adapter_files(str(tmp_path / "nothing"))


# ---------------------------------------------------------------------------------------------- the float64 model against autograd
@pytest.mark.parametrize("out,in_,r", [(48, 16, 1), (16, 48, 3), (30, 64, 4), (130, 80, 5)])
def test_projection_identity_against_torch_autograd(out, in_, r):
    """dA = s B^T dW and dB = s dW A^T are the gradients of a loss of W0 + s B A with respect to A and B (torch CPU autograd, float64), to
    1e-12; and the model's merge is that W."""
    g = torch.Generator().manual_seed(out * 1000 + in_)
    w0, x = torch.randn(out, in_, generator=g, dtype=torch.float64), torch.randn(7, in_, generator=g, dtype=torch.float64)
    a = torch.randn(r, in_, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(out, r, generator=g, dtype=torch.float64, requires_grad=True)
    s = 16.0 / r
    w = (w0 + s * b @ a).detach().requires_grad_(True)
    loss_of = lambda w: torch.tanh(x @ w.T).square().sum()   # noqa: E731
    with torch.enable_grad():   # (importing the package's inference modules switches autograd off process-wide)
        loss_of(w).backward()
        loss_of(w0 + s * b @ a).backward()
    merged, _ = LM.merge(w0.numpy(), a.detach().numpy(), b.detach().numpy(), s)
    assert np.abs(merged - w.detach().numpy()).max() <= 1e-12
    da, db, _, _ = LM.project(w.grad.numpy(), a.detach().numpy(), b.detach().numpy(), s)
    assert np.abs(da - a.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(da).max())
    assert np.abs(db - b.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(db).max())
    old_a, old_b = np.ones_like(da), np.full_like(db, -2.0)
    da2, db2, _, _ = LM.project(w.grad.numpy(), a.detach().numpy(), b.detach().numpy(), s, old_a, old_b)
    assert np.allclose(da2, da + 1.0, rtol=0, atol=1e-12 * max(1.0, np.abs(da).max())) and np.allclose(db2, db - 2.0, rtol=0, atol=1e-12 * max(1.0, np.abs(db).max()))
