"""CPU-only: the EMA of the weights (include/genie_hip.h, "EMA of the weights") -- the NumPy f32 restatement of tests/ema_model.py against
the arrays the reference's own LitEma wrote (tests/golden/ema_litema.npz, tools/make_goldens_ema.py), the trainer's schedule function,
and the host side of the three new entry points.  tests/test_hip_train_ema.py holds what needs a GPU.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ema_model as EM
from conftest import REPO, pkg

NEW = {"genie_adamw_ema_step": 17, "genie_ema_update": 5, "genie_swap_f32": 4}   # the header's arity
CONFIGS = {"d999": (0.999, False), "d999w": (0.999, True), "d9": (0.9, False), "d9w": (0.9, True)}
UPDATES, SIZES = 12, (5, 130, 1027)


def fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "ema_litema.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixture_is_what_the_tool_describes():
    g = fixture()
    for k, n in enumerate(SIZES):
        assert g[f"p{k}"].shape == (UPDATES + 1, n) and g[f"p{k}"].dtype == np.float32
        for tag in CONFIGS:
            assert g[f"{tag}_s{k}"].shape == (UPDATES, n) and g[f"{tag}_s{k}"].dtype == np.float32
    assert (g["p1"][:, :16] == 0).all() and (g["p1"][5:, 16:32] == 0).all() and (g["p1"][4, 16:32] != 0).any()
    assert (g["p0"] == g["p0"][0]).all()                                 # the tensor that does not move
    tiny = np.abs(g["p2"][1:, :64] - g["p2"][:-1, :64])
    assert 0 < tiny.max() < np.finfo(np.float32).tiny                    # denormal-range differences


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_restatement_is_litema_bit_for_bit(tag):
    """replay() over the recorded parameter states equals LitEma's shadow after every one of the 12 updates, on all three tensors."""
    g = fixture()
    decay, warm = CONFIGS[tag]
    for k in range(len(SIZES)):
        seq = g[f"p{k}"]
        got = EM.replay(seq[0], seq[1:], decay, warm)
        for u in range(UPDATES):
            want = g[f"{tag}_s{k}"][u]
            assert np.array_equal(bits(got[u]), bits(want)), (tag, k, u + 1, int((bits(got[u]) != bits(want)).sum()))
    assert not np.array_equal(g[f"{tag}_s2"][-1], g["p2"][-1])


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_schedule_is_the_fixtures(tag):
    """ema_decay_at / ema_one_minus_decay of 1xgpt_amd/train.py and the test model's schedule against the decay LitEma used at each update."""
    T = pkg("train")
    g = fixture()
    decay, warm = CONFIGS[tag]
    for n in range(1, UPDATES + 1):
        want = g[f"{tag}_d"][n - 1]
        assert np.float32(T.ema_decay_at(decay, n, warm)) == want == EM.decay_at(decay, n, warm), (tag, n)
        assert np.float32(T.ema_one_minus_decay(decay, n, warm)) == np.float32(1) - want == EM.one_minus_decay(decay, n, warm)
    if warm:
        assert g[f"{tag}_d"][0] == np.float32(2) / np.float32(11) and g[f"{tag}_d"][0] < np.float32(decay)
    else:
        assert (g[f"{tag}_d"] == np.float32(decay)).all()


def test_decay_validation():
    T = pkg("train")
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.ema_decay_at(bad, 1)
    with pytest.raises(ValueError):
        T.ema_decay_at(0.9, 0)
    assert T.ema_decay_at(0.0, 1) == 0.0 and T.ema_decay_at(1.0, 1) == 1.0
    assert T.ema_one_minus_decay(1.0, 3) == 0.0 and T.ema_one_minus_decay(0.0, 3) == 1.0
    import inspect
    sig = inspect.signature(T.GenieTrainer.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is False


def test_update_edge_values():
    """omd = 0 keeps the average, omd = 1 lands on the parameters up to the rounding of e - (e - p), equal values stay put."""
    e = np.array([0.0, 1.5, -2.25, 1e-38, 3e30], np.float32)
    p = np.array([1.0, 1.5, 4.0, 1.00001e-38, -1e30], np.float32)
    assert np.array_equal(EM.update(e, p, 0.0), e)
    assert np.array_equal(EM.update(e, p, 1.0), (e - (e - p).astype(np.float32)).astype(np.float32))
    assert np.array_equal(EM.update(e, e, 0.3), e)


def test_bindings_match_the_header():
    lib_mod = pkg("_lib")
    src = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in genie_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
        assert name in lib_mod.SIGNATURES, f"{name} has no ctypes signature"
        assert len(lib_mod.SIGNATURES[name][1]) == arity, name
    assert re.search(r"#define\s+GENIE_ABI_VERSION\s+3\b", src) and lib_mod.ABI_VERSION == 3
    a, e = lib_mod.SIGNATURES["genie_adamw_step"][1], lib_mod.SIGNATURES["genie_adamw_ema_step"][1]
    assert e[:4] + e[5:-2] + e[-1:] == a                                  # the AdamW arguments with ema and omd slotted in


def test_library_exports_and_refuses_on_the_host():
    """The refusals need no device: NULL with n > 0, step < 1, a bad one_minus_decay, overlapping ranges; n = 0 succeeds."""
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    L = lib_mod.load()
    E = lib_mod.E_ARG
    adam = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert L.genie_ema_update(None, 64, 4, 0.1, None) == E and L.genie_ema_update(64, None, 4, 0.1, None) == E
    for omd in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.genie_ema_update(64, 128, 4, omd, None) == E
        assert b"one_minus_decay" in L.genie_last_error()
        assert L.genie_adamw_ema_step(64, 128, 192, 256, 320, 4, *adam, 1, 1.0, None, 0.0, omd, None) == E
    assert L.genie_adamw_ema_step(64, 128, 192, 256, None, 4, *adam, 1, 1.0, None, 0.0, 0.1, None) == E
    assert L.genie_adamw_ema_step(64, 128, 192, 256, 320, 4, *adam, 0, 1.0, None, 0.0, 0.1, None) == E
    assert L.genie_swap_f32(None, 64, 4, None) == E and L.genie_swap_f32(64, None, 4, None) == E
    assert L.genie_swap_f32(64, 64 + 12, 4, None) == E and L.genie_swap_f32(64 + 12, 64, 4, None) == E and L.genie_swap_f32(64, 64, 1, None) == E
    assert b"overlap" in L.genie_last_error()
    assert L.genie_ema_update(None, None, 0, 0.1, None) == 0 and L.genie_swap_f32(None, None, 0, None) == 0
    assert L.genie_adamw_ema_step(None, None, None, None, None, 0, *adam, 1, 1.0, None, 0.0, 0.1, None) == 0


def test_cli_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--ema_decay", "--ema_warmup", "--eval_ema"):
        assert flag in out.stdout, flag
    assert '"--ema_decay"' in open(os.path.join(REPO, "tools", "bench_train.py")).read()
