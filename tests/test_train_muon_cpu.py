"""Muon, the part that runs anywhere (include/genie_hip.h, "Muon"; 1xgpt_amd/muon.py; GenieTrainer(muon=...)): the float64 model of
tests/muon_model.py against the SVD form of the iteration and against torch.optim.Muon on the CPU, the C ABI and its host-side refusals,
MuonConfig, target selection, the q / k / v split and the flat layout with a Muon flag.  tests/test_hip_train_muon.py holds the GPU side."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import muon_model as MM
from conftest import REPO, pkg
from test_train_frozen_cpu import cfg3, check_layout, numels

SHAPES = [(16, 16), (64, 64), (32, 128), (128, 32), (48, 80)]
KINDS = ["gaussian", "lowrank"]


def matrix(shape, kind, seed=0):
    g = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    if kind == "gaussian":
        return g.standard_normal(shape)
    return g.standard_normal((shape[0], 4)) @ g.standard_normal((4, shape[1])) + 1e-3 * g.standard_normal(shape)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_iteration_is_the_polynomial_of_the_singular_values(shape, kind):
    """k steps of X <- a X + (b A + c A A) X map X = U S V^T to U p^k(S) V^T, p(s) = a s + b s^3 + c s^5: tall matrices included (the
    transposed form commutes with the SVD).  Bar 1e-10, relative Frobenius; 7e-16 .. 6e-14 measured."""
    a, b, c = MM.DEFAULT_COEFFICIENTS
    u = matrix(shape, kind)
    x = u / np.linalg.norm(u)
    U, S, Vt = np.linalg.svd(x, full_matrices=False)
    for k in (1, 5):
        s = S.copy()
        for _ in range(k):
            s = a * s + b * s ** 3 + c * s ** 5
        d = rel(MM.newton_schulz(u, steps=k), (U * s) @ Vt)
        print(f"polynomial identity {shape} {kind} k={k}: {d:.2e}")
        assert d <= 1e-10, (shape, kind, k, d)
    assert np.array_equal(MM.newton_schulz(u, steps=0), x)
    assert not MM.newton_schulz(np.zeros(shape), steps=5).any()   # 0 / max(0, eps)


def torch_muon_steps(w0, grads, lr, wd, nesterov, adjust, ns_steps):
    """[W after step k] of torch.optim.Muon on the CPU, f32 parameters."""
    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float32)))
    opt = torch.optim.Muon([p], lr=lr, weight_decay=wd, momentum=0.95, nesterov=nesterov, ns_steps=ns_steps, adjust_lr_fn=adjust)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.astype(np.float32))
        opt.step()
        out.append(p.detach().numpy().astype(np.float64).copy())
    return out


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("adjust", ["match_rms_adamw", "original"])
def test_two_steps_without_iterations_against_torch(adjust, nesterov, wd):
    """ns_steps = 0: torch differs only by its bf16 casts of u, of the norm and of the quotient.  Per element
    |dW_ours - dW_torch| <= 2^-7 lr adj |O|, plus the f32 rounding of W.  Pins the momentum form (torch keeps (1 - mu) B: the same
    direction after the normalisation), the decay order, the adjust rule and the step-2 state.  Measured: 0.66 .. 0.97 of the bound (one
    bf16 rounding is at most 2^-9 of the binade's top but 2^-8 of its bottom, so three of them can come close to 2^-7)."""
    lr = 0.02
    for shape in [(32, 48), (48, 32), (16, 16)]:
        g = np.random.default_rng(shape[0])
        w0 = g.standard_normal(shape).astype(np.float32).astype(np.float64)
        grads = [g.standard_normal(shape).astype(np.float32).astype(np.float64) for _ in range(2)]
        theirs = torch_muon_steps(w0, grads, lr, wd, nesterov, adjust, 0)
        w, buf, prev_t = w0, np.zeros(shape), w0
        for k in range(2):
            w_new, buf, o = MM.muon_matrix(w, grads[k], buf, lr, wd, nesterov=nesterov, steps=0, adjust_lr=adjust)
            adj = MM.adjust(adjust, *shape)
            mine, torchs = w_new - w * (1 - lr * wd), theirs[k] - prev_t * (1 - lr * wd)
            # torch's W took two f32 roundings: of W * (1 - lr wd), at most 2^-24 |W_old|, and of the sum, at most 2^-24 |W_new|
            bound = 2.0 ** -7 * lr * adj * np.abs(o) + 2.0 ** -24 * (np.abs(theirs[k]) + np.abs(prev_t))
            worst = float(np.max(np.abs(mine - torchs) / bound))
            print(f"no-iteration step {k + 1} {shape} {adjust} nesterov={nesterov} wd={wd}: worst / bound = {worst:.3f}")
            assert worst <= 1.0, (shape, k, worst)
            # the restatement goes on from its own weights; torch's are compared step by step
            w, prev_t = w_new, theirs[k]
            assert rel(w, theirs[k]) < 1e-3


@pytest.mark.parametrize("shape", [(64, 64), (32, 128), (128, 32)], ids=lambda s: "x".join(map(str, s)))
def test_full_iteration_against_torch_on_gaussian_gradients(shape):
    """ns_steps = 5, Gaussian gradients only (torch's bf16 iteration is 0.4 .. 0.8 from float64 on low-rank inputs): the relative
    Frobenius distance of the update is below 0.05 -- torch alone measures 0.011 .. 0.018 from float64 here; a wrong coefficient, a missing
    transpose or swapped products is O(1)."""
    lr, wd = 0.02, 0.1
    g = np.random.default_rng(7)
    w0 = g.standard_normal(shape).astype(np.float32).astype(np.float64)
    grads = [g.standard_normal(shape).astype(np.float32).astype(np.float64) for _ in range(2)]
    theirs = torch_muon_steps(w0, grads, lr, wd, True, "match_rms_adamw", 5)
    w, buf, prev_t = w0, np.zeros(shape), w0
    for k in range(2):
        w_new, buf, _ = MM.muon_matrix(w, grads[k], buf, lr, wd)
        d = rel(w_new - w * (1 - lr * wd), theirs[k] - prev_t * (1 - lr * wd))
        print(f"full iteration step {k + 1} {shape}: update distance {d:.4f}")
        assert d < 0.05, (shape, k, d)
        w, prev_t = w_new, theirs[k]


def test_float32_restatement_is_close_to_float64():
    """What the format alone costs (the GPU test's yardstick): 1e-6 on Gaussian, 1e-5 on low-rank inputs."""
    for kind, bar in (("gaussian", 1e-5), ("lowrank", 2e-4)):
        for shape in SHAPES:
            u = matrix(shape, kind).astype(np.float32)
            d = rel(MM.newton_schulz(u, dtype=np.float32), MM.newton_schulz(u.astype(np.float64)))
            assert d < bar, (shape, kind, d)


def test_mixed_optimizer_first_step_matches_its_parts():
    g = np.random.default_rng(3)
    p = {"decoder.layers.0.spatial_attn.qkv.weight": g.standard_normal((48, 16)), "decoder.layers.0.mlp.fc1.bias": g.standard_normal(64)}
    gr = {n: g.standard_normal(v.shape) for n, v in p.items()}
    opt = MM.MixedOptimizer(p, ["decoder.layers.0.spatial_attn.qkv.weight"], lr=1e-2, weight_decay=0.1, max_norm=1.0,
                            decays=lambda n: "bias" not in n, ema_omd=0.25)
    norm = opt.step(gr)
    ss = sum(float(np.sum(v * v)) for v in gr.values())
    assert norm == math.sqrt(ss)
    coef = MM.clip_coef(ss, 1.0, 1.0)
    assert coef < 1.0
    n = "decoder.layers.0.spatial_attn.qkv.weight"
    for i in range(3):   # q, k and v are orthogonalised separately
        sl = slice(16 * i, 16 * i + 16)
        want, b, _ = MM.muon_matrix(p[n][sl], gr[n][sl], np.zeros((16, 16)), 1e-2, 0.1, coef)
        assert np.array_equal(opt.p[n][sl], want) and np.array_equal(opt.m[n][sl], b)
    assert not opt.v[n].any()
    want, m, v = MM.adamw_tensor(p["decoder.layers.0.mlp.fc1.bias"], gr["decoder.layers.0.mlp.fc1.bias"], 0, 0, 1e-2, 0.0, 1, coef)
    assert np.array_equal(opt.p["decoder.layers.0.mlp.fc1.bias"], want)
    assert np.array_equal(opt.ema[n], p[n] - 0.25 * (p[n] - opt.p[n]))


# ---------------------------------------------------------------------------------------------- the C ABI
def lib_and_mod():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod.load(), lib_mod


def test_header_is_c99_and_exports_the_muon_symbols(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib, lib_mod = lib_and_mod()
    for name in ("genie_muon_layout", "genie_muon_workspace_bytes", "genie_muon_step", "genie_newton_schulz"):
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
    assert lib.genie_version() == 3 == lib_mod.ABI_VERSION
    src = tmp_path / "muon.c"
    src.write_text('#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_muon_item it[2]; genie_muon_settings s; size_t lay[23];\n"
                   "    memset(it, 0, sizeof it); memset(&s, 0, sizeof s);\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3 || GENIE_MUON_MAX_ITEMS < 16) return 1;\n"
                   "    if (genie_muon_layout(lay, 23) != 23 || lay[0] != sizeof(genie_muon_item) || lay[9] != sizeof(genie_muon_settings)) return 2;\n"
                   "    if (genie_muon_step(0, 1, &s, 0, 0, 0) != GENIE_E_ARG) return 3;\n"
                   "    if (genie_muon_step(it, 0, &s, 0, 0, 0) != GENIE_E_ARG || genie_muon_step(it, GENIE_MUON_MAX_ITEMS + 1, &s, 0, 0, 0) != GENIE_E_ARG) return 4;\n"
                   "    if (genie_muon_workspace_bytes(it, 1) != 0 || strstr(genie_last_error(), \"multiples of 16\") == 0) return 5;\n"
                   "    if (genie_newton_schulz(0, 0, 16, 16, 1, 5, 1.f, 1.f, 1.f, 1e-7f, 0, 0, 0) != GENIE_E_ARG) return 6;\n"
                   "    return 0;\n}\n")
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "muon.o")], check=True)
    exe = tmp_path / "muon"
    subprocess.run([gcc, str(tmp_path / "muon.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_struct_layout_matches_ctypes():
    lib, lib_mod = lib_and_mod()
    lay = (C.c_size_t * 23)()
    assert lib.genie_muon_layout(lay, 23) == 23
    want = [v for T in (lib_mod.MuonItem, lib_mod.MuonSettings) for v in [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]]
    assert list(lay) == want
    assert lib_mod.MUON_MAX_ITEMS >= 16


# pointers that are never dereferenced: every refusal below happens on the host, before the device or the stream is touched
P, G, B, E, WS = (0x10000000 * k for k in range(1, 6))


def good(**kw):
    f = dict(param=P, grad=G, momentum=B, ema=None, rows=32, cols=48, lr=1e-3, weight_decay=0.0)
    f.update(kw)
    return pkg("_lib").MuonItem(**f)


def arr(*items):
    return (pkg("_lib").MuonItem * len(items))(*items), len(items)


def good_settings(**kw):
    return pkg("muon").settings(pkg("muon").MuonConfig(), **kw)


ITEM_REFUSALS = [
    ("rows 24", dict(rows=24), "multiples of 16"),
    ("cols 0", dict(cols=0), "multiples of 16"),
    ("rows -16", dict(rows=-16), "multiples of 16"),
    ("NULL param", dict(param=None), "NULL param, grad or momentum"),
    ("NULL grad", dict(grad=None), "NULL param, grad or momentum"),
    ("NULL momentum", dict(momentum=None), "NULL param, grad or momentum"),
    ("misaligned param", dict(param=P + 4), "16-byte aligned"),
    ("misaligned ema", dict(ema=E + 8), "16-byte aligned"),
    ("nan lr", dict(lr=float("nan")), "lr or weight_decay is not finite"),
    ("inf weight decay", dict(weight_decay=float("inf")), "lr or weight_decay is not finite"),
]


@pytest.mark.parametrize("what,change,msg", ITEM_REFUSALS, ids=[r[0] for r in ITEM_REFUSALS])
def test_step_refuses_a_bad_item(what, change, msg):
    lib, lib_mod = lib_and_mod()
    items, n = arr(good(), good(**change))   # the bad item is the second: every item is checked before anything is launched
    assert lib.genie_muon_step(items, n, good_settings(), WS, 1 << 30, None) == lib_mod.E_ARG
    assert msg in lib.genie_last_error().decode() and "item 1" in lib.genie_last_error().decode()


def test_step_refuses_bad_tables_settings_and_workspaces():
    lib, lib_mod = lib_and_mod()
    E_ARG = lib_mod.E_ARG
    err = lambda: lib.genie_last_error().decode()   # noqa: E731
    items, n = arr(good(), good(rows=64, cols=16))
    need = lib.genie_muon_workspace_bytes(items, n)
    # 64 doubles per item, X0 and X1 of every item, A and P of the largest group (32 x 32), every part rounded to 64 floats
    assert need == 4 * (2 * 64 * 2 + 2 * (32 * 48 + 64 * 16) + 2 * 32 * 32)
    assert lib.genie_muon_step(None, 1, good_settings(), WS, need, None) == E_ARG and "NULL items" in err()
    assert lib.genie_muon_step(items, n, None, WS, need, None) == E_ARG and "NULL settings" in err()
    for k in (0, -1, lib_mod.MUON_MAX_ITEMS + 1):
        assert lib.genie_muon_step(items, k, good_settings(), WS, need, None) == E_ARG and "is not in 1 .." in err()
        assert lib.genie_muon_workspace_bytes(items, k) == 0
    assert lib.genie_muon_step(items, n, good_settings(), None, need, None) == E_ARG and "workspace" in err()
    assert lib.genie_muon_step(items, n, good_settings(), WS + 4, need, None) == E_ARG and "workspace" in err()
    assert lib.genie_muon_step(items, n, good_settings(), WS, need - 1, None) == E_ARG and "needed" in err()
    for field, value, msg in (("ns_steps", 100, "ns_steps"), ("ns_steps", -1, "ns_steps"), ("a", float("nan"), "not finite"),
                              ("eps", float("inf"), "not finite"), ("momentum", float("nan"), "not finite"),
                              ("grad_mult", float("inf"), "not finite"), ("adjust", 2, "adjust")):
        s = good_settings()
        setattr(s, field, value)
        assert lib.genie_muon_step(items, n, s, WS, need, None) == E_ARG and msg in err(), field
    s = good_settings(ema_one_minus_decay=1.5)
    assert lib.genie_muon_step(*arr(good(ema=E)), s, WS, need, None) == E_ARG and "ema_one_minus_decay" in err()


def test_newton_schulz_refusals():
    lib, lib_mod = lib_and_mod()
    E_ARG = lib_mod.E_ARG
    err = lambda: lib.genie_last_error().decode()   # noqa: E731
    ok = dict(in_=P, out=G, rows=32, cols=48, batch=2, steps=5, a=3.4445, b=-4.775, c=2.0315, eps=1e-7, ws=WS, ws_bytes=1 << 30)

    def call(**kw):
        f = dict(ok, **kw)
        return lib.genie_newton_schulz(f["in_"], f["out"], f["rows"], f["cols"], f["batch"], f["steps"], f["a"], f["b"], f["c"], f["eps"],
                                       f["ws"], f["ws_bytes"], None)
    for kw, msg in ((dict(rows=24), "multiples of 16"), (dict(cols=8), "multiples of 16"), (dict(in_=None), "NULL in or out"),
                    (dict(out=G + 4), "16-byte aligned"), (dict(batch=0), "batch = 0"), (dict(batch=lib_mod.MUON_MAX_ITEMS + 1), "batch ="),
                    (dict(steps=100), "ns_steps"), (dict(c=float("nan")), "not finite"), (dict(ws=None), "workspace"),
                    (dict(ws_bytes=1024), "needed"), (dict(out=P + 64), "overlaps out"), (dict(ws=P), "workspace overlaps")):
        assert call(**kw) == E_ARG and msg in err(), (kw, err())


# ---------------------------------------------------------------------------------------------- MuonConfig, targets, the split
def test_muon_config_validation():
    M = pkg("muon")
    c = M.MuonConfig()
    assert (c.momentum, c.nesterov, c.ns_steps, c.ns_coefficients, c.eps, c.adjust_lr, c.targets) == (
        0.95, True, 5, (3.4445, -4.7750, 2.0315), 1e-7, "match_rms_adamw", ["decoder.layers.*"])
    assert M.MuonConfig(targets="a,b").targets == ["a", "b"] and M.MuonConfig(targets=["x"]).targets == ["x"]
    for kw in (dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float("nan")), dict(ns_steps=100), dict(ns_steps=-1), dict(ns_steps=2.5),
               dict(ns_steps=True), dict(ns_coefficients=(1.0, 2.0)), dict(ns_coefficients=(1.0, 2.0, float("inf"))), dict(eps=0.0),
               dict(eps=float("nan")), dict(adjust_lr="rms"), dict(adjust_lr=None), dict(targets=""), dict(targets=[]), dict(targets=[3])):
        with pytest.raises(ValueError):
            M.MuonConfig(**kw)
    assert c.settings_dict() == dict(momentum=0.95, nesterov=True, ns_steps=5, ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7,
                                     adjust_lr="match_rms_adamw")
    s = M.settings(c, grad_mult=0.5, max_grad_norm=1.0, ema_one_minus_decay=0.25)
    assert (s.nesterov, s.ns_steps, s.adjust, s.grad_mult, s.max_grad_norm, s.ema_one_minus_decay) == (1, 5, 1, 0.5, 1.0, 0.25)
    assert M.adjust("match_rms_adamw", 64, 256) == 0.2 * 16 and M.adjust("original", 256, 64) == 2.0 and M.adjust("original", 64, 256) == 1.0


def test_target_selection_and_the_qkv_split():
    M, cfg = pkg("muon"), cfg3()
    names = set(numels(cfg))
    default = M.select_targets(cfg, ["decoder.layers.*"])
    assert len(default) == 6 * cfg.num_layers and "out_x_proj.weight" not in default and all(n.endswith(".weight") for n in default)
    assert M.select_targets(cfg, ["out_x_proj.weight"]) == ["out_x_proj.weight"]   # eligible, not in the default
    assert M.select_targets(cfg, ["*.mlp.*"]) == [f"decoder.layers.{i}.mlp.{f}.weight" for i in range(3) for f in ("fc1", "fc2")]
    with pytest.raises(ValueError, match="matches no Linear weight"):
        M.select_targets(cfg, ["decoder.layers.*.norm1.weight"])   # a norm is no target
    with pytest.raises(ValueError, match="matches no Linear weight"):
        M.select_targets(cfg, ["pos_embed_TSC"])
    assert M.muon_names(cfg, ["decoder.layers.*"], names) == default
    only = {"decoder.layers.1.mlp.fc1.weight", "pos_embed_TSC"}
    assert M.muon_names(cfg, ["decoder.layers.*"], only) == ["decoder.layers.1.mlp.fc1.weight"]   # a frozen target is skipped
    with pytest.raises(ValueError, match="no trainable tensor is left for Muon"):
        M.muon_names(cfg, ["decoder.layers.*"], {"pos_embed_TSC", "out_x_proj.weight"})
    d = cfg.d_model
    assert M.blocks("decoder.layers.0.spatial_attn.qkv.weight", (3 * d, d)) == [(0, d, d), (d, d, d), (2 * d, d, d)]
    assert M.blocks("decoder.layers.0.mlp.fc1.weight", (4 * d, d)) == [(0, 4 * d, d)]
    assert M.blocks("out_x_proj.weight", (1024, d)) == [(0, 1024, d)]


def test_chunks_sort_by_shape_and_bound_the_launch_count():
    M = pkg("muon")

    class It:
        def __init__(self, r, c):
            self.rows, self.cols = r, c
    for layers in (2, 32, 64):
        items = []
        for _ in range(layers):
            items += [It(512, 512)] * 8 + [It(2048, 512), It(512, 2048)]
        parts = M.chunks(items)
        assert sum(len(p) for p in parts) == len(items) and all(1 <= len(p) <= pkg("_lib").MUON_MAX_ITEMS for p in parts)
        assert len(parts) == math.ceil(len(items) / pkg("_lib").MUON_MAX_ITEMS)
        # per table: momentum, normalise, apply, and 15 products per shape in it; sorted by shape, every change of shape inside a table
        # adds one to the count of (table, shape) pairs: two changes for three shapes
        assert M.launches(items, 5) <= len(parts) * 3 + 15 * (len(parts) + 2)


# ---------------------------------------------------------------------------------------------- the flat layout
def test_layout_without_muon_is_the_layout_of_before():
    T, cfg = pkg("train"), cfg3()
    n = numels(cfg)
    a, b = T.FlatLayout(cfg, n), T.FlatLayout(cfg, n, None, None, None)
    check_layout(cfg, n, b)
    for k in ("order", "offsets", "n_flat", "n_train", "adam_runs", "groups", "segments", "stop", "embed"):
        assert getattr(a, k) == getattr(b, k), k
    assert b.muon == set()
    sel = T.select_trainable(n, "decoder.layers.1.*")
    assert T.FlatLayout(cfg, n, sel, {"*.bias": 2.0}, ()).adam_runs == T.FlatLayout(cfg, n, sel, {"*.bias": 2.0}).adam_runs


def test_layout_with_muon_keeps_offsets_and_takes_the_tensors_out_of_the_runs():
    T, M, cfg = pkg("train"), pkg("muon"), cfg3()
    n = numels(cfg)
    plain = T.FlatLayout(cfg, n)
    mu = M.muon_names(cfg, ["decoder.layers.*"], set(n))
    lay = T.FlatLayout(cfg, n, None, None, mu)
    for k in ("order", "offsets", "n_flat", "n_train", "groups", "segments", "stop", "embed"):
        assert getattr(plain, k) == getattr(lay, k), k
    assert lay.muon == set(mu)
    covered = lambda name: [r for r in lay.adam_runs if r[0] < lay.offsets[name][1] and lay.offsets[name][0] < r[1]]   # noqa: E731
    for name in lay.order:
        runs = covered(name)
        if name in lay.muon:
            assert runs == [], name
        else:
            (r,) = runs
            assert r[0] <= lay.offsets[name][0] and lay.offsets[name][1] <= r[1] and (r[2], r[3]) == (T.decays(name), 1.0)
    assert all(a[1] <= b[0] for a, b in zip(lay.adam_runs, lay.adam_runs[1:]))
    total = sum(hi - lo for lo, hi, _, _ in lay.adam_runs) + sum((n[x] + 63) // 64 * 64 for x in mu)
    assert total == lay.n_train
    with pytest.raises(ValueError, match="not trainable"):
        T.FlatLayout(cfg, n, T.select_trainable(n, "out_x_proj.*"), None, mu[:1])


def test_trainer_state_settings_round_trip_on_the_host():
    """What state_dict carries for Muon is MuonConfig.settings_dict() and the names: equal settings compare equal after a save / load
    through torch (tuples become lists), different ones do not."""
    import io
    M = pkg("muon")
    a = dict(M.MuonConfig().settings_dict(), names=["x"])
    buf = io.BytesIO()
    torch.save({"muon": a}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)["muon"]
    norm = lambda d: {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in d.items()}   # noqa: E731
    assert norm(back) == norm(a)
    assert norm(dict(M.MuonConfig(ns_steps=4).settings_dict(), names=["x"])) != norm(a)
    assert norm(dict(M.MuonConfig(nesterov=False).settings_dict(), names=["x"])) != norm(a)
