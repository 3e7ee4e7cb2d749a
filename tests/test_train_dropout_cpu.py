"""CPU-only: MLP dropout in the training step (include/genie_hip.h, "MLP dropout") -- the mask law restated in NumPy
(tests/dropout_model.py), the float64 model the GPU tests compare against, the reference's own Mlp through a fixture, the model
classes' acceptance of mlp_drop, and the host side of the new entry points.  tests/test_hip_train_dropout.py holds what needs a GPU.
"""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dropout_model as DM
from conftest import REPO, pkg
from oracle import genie_train_oracle as TO

NEW = ["genie_dropout_layout", "genie_dropout_mask", "genie_train_forward_drop", "genie_train_backward_layer_drop"]


def lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


# ---------------------------------------------------------------------------------------------- the law
@pytest.mark.parametrize("counter, key, out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, out):
    """The three Philox4x32-10 known-answer vectors of the Random123 distribution."""
    got = tuple(int(w) for w in DM.philox4x32_10(counter, key))
    assert got == out, [hex(w) for w in got]


def test_mask_is_a_function_of_its_counters():
    """Equal inputs give equal masks; changing any of seed, call, layer or site changes the mask; a prefix of a longer mask is the
    shorter mask (element e depends on e alone); a seed above 2^32 uses its high word."""
    base = dict(seed=7, call=3, layer=1, site=0, n=4099, p=0.5)
    m = DM.keep_mask(**base)
    assert m.dtype == np.uint8 and m.shape == (4099,) and set(np.unique(m)) == {0, 1}
    assert np.array_equal(m, DM.keep_mask(**base))
    for k, v in (("seed", 8), ("call", 4), ("layer", 2), ("site", 1), ("seed", 7 + 2 ** 32)):
        assert not np.array_equal(m, DM.keep_mask(**{**base, k: v})), k
    assert np.array_equal(m[:1001], DM.keep_mask(**{**base, "n": 1001}))
    # (layer, site) share one counter word: layer * 2 + site
    assert np.array_equal(DM.keep_mask(**{**base, "layer": 1, "site": 0}), DM.keep_mask(**{**base, "layer": 0, "site": 2}))
    assert DM.keep_mask(**{**base, "p": 0.0}).all()
    assert DM.threshold(0.5) == 2 ** 31 and DM.threshold(0.0) == 0
    assert DM.threshold(0.1) == int(math.floor(float(np.float32(0.1)) * 2.0 ** 32)) == 429496736


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(p):
    """The kept fraction of 2^20 elements is within 5 standard deviations of 1 - p (seed 0, call 0, layer 0, site 0: the draw is
    deterministic, so this checks that one seed, once)."""
    n = 1 << 20
    kept = int(DM.keep_mask(0, 0, 0, 0, n, p).sum())
    q = 1.0 - DM.threshold(p) / 2.0 ** 32
    sd = math.sqrt(n * q * (1 - q))
    print(f"p {p}: kept {kept} of {n}, expected {n * q:.1f}, {abs(kept - n * q) / sd:.2f} standard deviations")
    assert abs(kept - n * q) <= 5 * sd
    assert abs(q - (1 - p)) < 1e-7


# ---------------------------------------------------------------------------------------------- the float64 model
def tiny_case(qk_norm):
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=2, use_mup=False)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=31, law="conditioned")
    batch = TO.maskgit_collate(syn.make_clips(2, cfg, seed=905), cfg, TO.NumpyDraws(9))
    return cfg, sd, batch["input_ids"], batch["labels"]


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


@pytest.mark.parametrize("qk_norm", [False, True], ids=["ln", "qk"])
def test_model_with_all_ones_masks_is_the_training_oracle(qk_norm):
    """autograd_step with all-ones masks (and with no masks) equals TO.forward_backward(dtype=float64) to 1e-12: loss and every
    gradient tensor (largest error over the tensor's largest element)."""
    pytest.importorskip("torch")
    cfg, sd, ids, labels = tiny_case(qk_norm)
    loss_o, _, g_o = TO.forward_backward(ids, labels, sd, cfg, dtype=np.float64)
    for masks in (DM.ones_masks(cfg, ids.shape[0]), None):
        loss, g = DM.autograd_step(cfg, sd, ids, labels, masks, 0.0)
        assert abs(loss - loss_o) <= 1e-12 * abs(loss_o)
        assert set(g_o) <= set(g)
        worst = {k: rel_err(g[k], g_o[k]) for k in g_o}
        assert max(worst.values()) <= 1e-12, max(worst.items(), key=lambda kv: kv[1])


def test_model_masks_change_the_step():
    """Real masks move the loss and every layer's MLP gradients, and a dropped hidden unit's fc1 row sees only the tokens that kept it."""
    pytest.importorskip("torch")
    cfg, sd, ids, labels = tiny_case(False)
    base_loss, base = DM.autograd_step(cfg, sd, ids, labels)
    masks = DM.step_masks(cfg, ids.shape[0], seed=1, call=0, p=0.5)
    loss, g = DM.autograd_step(cfg, sd, ids, labels, masks, 0.5)
    assert loss != base_loss and np.isfinite(loss)
    for i in range(cfg.num_layers):
        for n in ("mlp.fc1.weight", "mlp.fc2.weight", "mlp.fc2.bias"):
            k = f"decoder.layers.{i}.{n}"
            assert not np.array_equal(g[k], base[k]), k
    m0 = masks[-1][0].copy()
    m0[:, 5] = 0                                     # hidden unit 5 of the last layer dropped at every token
    masks[-1] = (m0, masks[-1][1])
    _, g = DM.autograd_step(cfg, sd, ids, labels, masks, 0.5)
    last = f"decoder.layers.{cfg.num_layers - 1}."
    assert not g[last + "mlp.fc1.weight"][5].any() and not g[last + "mlp.fc2.weight"][:, 5].any()
    assert g[last + "mlp.fc1.weight"][6].any()


def test_reference_mlp_fixture():
    """tests/golden/mlp_dropout.npz (tools/make_goldens_dropout.py: the reference's Mlp in train mode, float64, masks recovered by a
    hook on its nn.Dropout): dropout_model.mlp reproduces the output and the gradients of the stored cotangent to 1e-12."""
    torch = pytest.importorskip("torch")
    g = np.load(os.path.join(REPO, "tests", "golden", "mlp_dropout.npz"))
    p = float(g["p"])
    assert 0 < p < 1 and 0 < g["m0"].mean() < 1 and 0 < g["m1"].mean() < 1
    with torch.enable_grad():
        t = {k: torch.from_numpy(g[k].astype(np.float64)).requires_grad_(True) for k in ("x", "fc1_w", "fc1_b", "fc2_w", "fc2_b")}
        m0, m1 = (torch.from_numpy(g[k].astype(np.float64)) for k in ("m0", "m1"))
        y = DM.mlp(t["x"], t["fc1_w"], t["fc1_b"], t["fc2_w"], t["fc2_b"], m0, m1, p)
        (y * torch.from_numpy(g["cot"])).sum().backward()
    assert rel_err(y.detach().numpy(), g["y"]) <= 1e-12
    for mine, ref in (("x", "dx"), ("fc1_w", "d_fc1_w"), ("fc1_b", "d_fc1_b"), ("fc2_w", "d_fc2_w"), ("fc2_b", "d_fc2_b")):
        assert rel_err(t[mine].grad.numpy(), g[ref]) <= 1e-12, ref
    # the order is pinned: with the masks swapped between the sites' roles (scaling before the bias) the output differs
    with torch.no_grad():
        h = torch.nn.functional.gelu(torch.nn.functional.linear(t["x"], t["fc1_w"], t["fc1_b"])) * m0 / (1 - p)
        wrong = torch.nn.functional.linear(h, t["fc2_w"]) * m1 / (1 - p) + t["fc2_b"]
    assert rel_err(wrong.numpy(), g["y"]) > 1e-3


# ---------------------------------------------------------------------------------------------- the model classes
def test_model_accepts_mlp_drop_and_the_config_round_trips(tmp_path):
    """STMaskGIT(GenieConfig(..., mlp_drop=0.1)) constructs (it raised NotImplementedError before), the value survives the JSON round trip,
    values outside [0, 1) are refused, and attn_drop -- which the reference constructs but never calls -- still raises."""
    pytest.importorskip("torch")
    C, M = pkg("config"), pkg("st_mask_git")
    kw = dict(num_layers=1, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False, num_prompt_frames=2)
    cfg = C.GenieConfig(**kw, mlp_drop=0.1)
    model = M.STMaskGIT(cfg)
    assert model.config.mlp_drop == 0.1 and model.decoder.layers[0].mlp.mlp_drop == 0.1
    path = tmp_path / "config.json"
    cfg.save_pretrained(str(path)) if hasattr(cfg, "save_pretrained") else path.write_text(json.dumps(vars(cfg)))
    text = json.loads(path.read_text())
    assert text["mlp_drop"] == 0.1
    again = C.GenieConfig.from_pretrained(str(path))
    assert again.mlp_drop == 0.1 and vars(again) == vars(cfg)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            M.STMaskGIT(C.GenieConfig(**kw, mlp_drop=bad))
    with pytest.raises(NotImplementedError):
        M.STMaskGIT(C.GenieConfig(**kw, attn_drop=0.1))


def test_cli_flags_exist():
    for tool, flags in (("train", ("--mlp_drop", "--dropout_seed")), ("bench_train", ("--mlp_drop",))):
        src = open(os.path.join(REPO, "tools", tool + ".py")).read()
        for f in flags:
            assert f'"{f}"' in src, (tool, f)


# ---------------------------------------------------------------------------------------------- ABI
def test_bindings_version_and_layouts():
    lib_mod, L = lib()
    src = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(genie_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in declared, f"{n} is not declared in genie_hip.h"
        assert n in lib_mod.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(L, n), f"{n} is not exported"
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    assert re.search(r"#define\s+GENIE_ABI_VERSION\s+3\b", src)
    assert L.genie_abi_layout(None, 0) == 12
    out = (ctypes.c_size_t * 4)()
    assert L.genie_dropout_layout(out, 4) == 4 and L.genie_dropout_layout(None, 0) == 4
    D = lib_mod.Dropout
    assert list(out) == [ctypes.sizeof(D), D.p.offset, D.call.offset, D.seed.offset] == [16, 0, 4, 8]
    S = lib_mod.SIGNATURES
    for fn in ("genie_train_forward", "genie_train_backward_layer"):
        assert S[fn + "_drop"][0] is S[fn + "_ex"][0] and S[fn + "_drop"][1] == S[fn + "_ex"][1] + [ctypes.POINTER(D)], fn


def test_bad_p_is_refused_before_anything_else():
    """p = -0.1, 1.0 and NaN: GENIE_E_ARG from the three entry points that take a genie_dropout, naming p, whatever else is wrong with the
    call (NULL pointers, never dereferenced; a bad recompute mode).  p = 0 and NULL go on to the checks of the *_ex forms."""
    lib_mod, L = lib()
    c = lib_mod.make_cfg(pkg("config").c35(), lib_mod.PREC_BF16)
    for p in (-0.1, 1.0, float("nan")):
        dr = lib_mod.Dropout(p=p, call=0, seed=0)
        for mode in (0, 1, 2):
            assert L.genie_train_forward_drop(c, None, 0, 0, 1, 0, 0, 0, 0, None, mode, dr) == lib_mod.E_ARG
            assert b"dropout p" in L.genie_last_error()
            assert L.genie_train_backward_layer_drop(c, None, None, None, 0, 1, 0, 0, 0, 0, 0, mode, dr) == lib_mod.E_ARG
            assert b"dropout p" in L.genie_last_error()
        assert L.genie_dropout_mask(dr, 0, 0, 16, 0, 0) == lib_mod.E_ARG
        assert b"dropout p" in L.genie_last_error()
    for dr in (None, lib_mod.Dropout(p=0.0, call=5, seed=9)):
        assert L.genie_train_forward_drop(c, None, 0, 0, 1, 0, 0, 0, 0, None, 2, dr) == lib_mod.E_ARG
        assert b"recompute" in L.genie_last_error()
        assert L.genie_train_forward_drop(c, None, 0, 0, 1, 0, 0, 0, 0, None, 1, dr) == lib_mod.E_ARG
        assert b"NULL" in L.genie_last_error()
        assert L.genie_train_backward_layer_drop(c, None, None, None, 0, 1, 0, 0, 0, 0, 0, 2, dr) == lib_mod.E_ARG
        assert b"recompute" in L.genie_last_error()
    ok = lib_mod.Dropout(p=0.5, call=0, seed=0)
    assert L.genie_dropout_mask(None, 0, 0, 16, 0, 0) == lib_mod.E_ARG
    for layer, site, n in ((-1, 0, 16), (0, 2, 16), (0, -1, 16), (0, 0, -1), (0, 0, 16)):   # the last: NULL keep with n > 0
        assert L.genie_dropout_mask(ok, layer, site, n, 0, 0) == lib_mod.E_ARG, (layer, site, n)
    assert L.genie_dropout_mask(ok, 0, 0, 0, 0, 0) == 0   # n = 0: nothing enqueued


def test_header_compiles_as_c99_and_c_reaches_the_new_entry_points(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib_mod, _ = lib()
    so = lib_mod.LIB_PATH
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_cfg c; genie_dropout dr; size_t lay[4];\n"
                   "    memset(&c, 0, sizeof c);\n"
                   "    c.num_layers = 2; c.num_heads = 8; c.head_dim = 64; c.d_model = 512; c.T = 16; c.S = 256; c.hidden = 2048;\n"
                   "    c.factored_vocab = 512; c.num_factored = 2; c.image_vocab_size = 262144; c.attn_scale = 0.125f; c.readout_mult = 1.0f;\n"
                   "    c.precision = GENIE_PREC_BF16;\n"
                   "    dr.p = 1.0f; dr.call = 0; dr.seed = 1;\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3) return 1;\n"
                   "    if (genie_dropout_layout(lay, 4) != 4 || lay[0] != sizeof(genie_dropout) || lay[1] != offsetof(genie_dropout, p)\n"
                   "        || lay[2] != offsetof(genie_dropout, call) || lay[3] != offsetof(genie_dropout, seed)) return 2;\n"
                   "    if (genie_train_forward_drop(&c, NULL, NULL, NULL, 2, NULL, 0, NULL, NULL, NULL, 0, &dr) != GENIE_E_ARG) return 3;\n"
                   "    if (genie_train_backward_layer_drop(&c, NULL, NULL, NULL, 0, 2, NULL, NULL, 0, 0, NULL, 0, &dr) != GENIE_E_ARG) return 4;\n"
                   "    if (genie_dropout_mask(&dr, 0, 0, 4, NULL, NULL) != GENIE_E_ARG) return 5;\n"
                   "    if (strstr(genie_last_error(), \"dropout p\") == NULL) return 6;\n"
                   "    return 0;\n}\n")
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "abi.o")],
                   check=True)
    subprocess.run([gcc, str(tmp_path / "abi.o"), so, f"-Wl,-rpath,{os.path.dirname(so)}", "-o", str(tmp_path / "abi")], check=True)
    r = subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
