"""CPU-only: the host side of the training step with activation recomputation (include/genie_hip.h, "Activation recomputation").
The size functions and the argument checks of the *_ex entry points need no GPU; tests/test_hip_train_recompute.py holds what does.

The grid of the size tests: c35() and c138() at T in {16, 32, 64}, B in {1, 3, 8}, the three precisions, both values of qk_norm.
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO, pkg

EX_NAMES = ["genie_train_activation_bytes_ex", "genie_train_workspace_bytes_ex", "genie_train_forward_ex",
            "genie_train_backward_head_ex", "genie_train_backward_layer_ex"]


def lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def grid():
    """(tag, GenieConfig, precision, B) over the whole grid."""
    lib_mod, C = pkg("_lib"), pkg("config")
    for name, make in (("c35", C.c35), ("c138", C.c138)):
        for T in (16, 32, 64):
            for qk_norm in (False, True):
                for prec in (lib_mod.PREC_EXACT, lib_mod.PREC_BF16, lib_mod.PREC_F16X3):
                    for B in (1, 3, 8):
                        cfg = make()
                        cfg.T, cfg.qk_norm = T, qk_norm
                        yield f"{name}/T{T}/qk{int(qk_norm)}/p{prec}/B{B}", cfg, prec, B


def test_mode_0_is_todays_size():
    lib_mod, L = lib()
    n = 0
    for tag, cfg, prec, B in grid():
        c = lib_mod.make_cfg(cfg, prec)
        assert L.genie_train_activation_bytes_ex(c, B, 0) == L.genie_train_activation_bytes(c, B) > 0, tag
        assert L.genie_train_workspace_bytes_ex(c, B, 0) == L.genie_train_workspace_bytes(c, B) > 0, tag
        n += 1
    assert n == 2 * 3 * 2 * 3 * 3


def test_recompute_size_bound():
    """bytes_ex(cfg, B, 1) <= A(cfg with num_layers = 1, B) + L * roundup256(M * d * 4), A today's size function: one layer's slots
    and the tail, plus the L checkpoints.  And smaller than mode 0 from three layers on (checked at L = 3 and at the config's own 32)."""
    lib_mod, L = lib()
    for tag, cfg, prec, B in grid():
        for layers in (cfg.num_layers, 3):
            cfg.num_layers = layers
            c = lib_mod.make_cfg(cfg, prec)
            cfg.num_layers = 1
            one = L.genie_train_activation_bytes(lib_mod.make_cfg(cfg, prec), B)
            M = B * cfg.T * cfg.S
            ckpt = (M * cfg.d_model * 4 + 255) // 256 * 256
            got = L.genie_train_activation_bytes_ex(c, B, 1)
            assert 0 < got <= one + layers * ckpt, (tag, layers, got, one, ckpt)
            assert got >= layers * ckpt, (tag, layers)                      # the checkpoints themselves
            assert got < L.genie_train_activation_bytes_ex(c, B, 0), (tag, layers)
            assert L.genie_train_workspace_bytes_ex(c, B, 1) > 0, tag


def test_bad_mode_is_refused_before_anything_else():
    """recompute in {-1, 2}: the size functions answer 0; the three launching entry points answer GENIE_E_ARG and name the argument,
    whatever else is wrong with the call -- here NULL pointers and, in the second config, a geometry the step refuses with
    GENIE_E_SHAPE (T * S = 288 in bf16), which mode 0 still reports as such."""
    lib_mod, L = lib()
    C = pkg("config")
    ok = lib_mod.make_cfg(C.c35(), lib_mod.PREC_BF16)
    odd = lib_mod.make_cfg(C.GenieConfig(num_layers=2, num_heads=2, d_model=128, T=2, S=144, num_factored_vocabs=2, qk_norm=False,
                                         num_prompt_frames=1, use_mup=False), lib_mod.PREC_BF16)
    assert L.genie_train_backward_head_ex(odd, None, None, None, 1, 0, 0, 0, 0, 0, 0) == lib_mod.E_SHAPE
    assert L.genie_train_backward_layer_ex(odd, None, None, None, 0, 1, 0, 0, 0, 0, 0, 1) == lib_mod.E_SHAPE
    for mode in (-1, 2):
        for c in (ok, odd):
            assert L.genie_train_activation_bytes_ex(c, 1, mode) == 0
            assert L.genie_train_workspace_bytes_ex(c, 1, mode) == 0
            calls = {"forward": (c, None, 0, 0, 1, 0, 0, 0, 0, None, mode),
                     "backward_head": (c, None, None, None, 1, 0, 0, 0, 0, 0, mode),
                     "backward_layer": (c, None, None, None, 0, 1, 0, 0, 0, 0, 0, mode)}
            for fn, args in calls.items():
                assert getattr(L, f"genie_train_{fn}_ex")(*args) == lib_mod.E_ARG, (mode, fn)
                msg = L.genie_last_error()
                assert b"recompute" in msg and str(mode).encode() in msg and f"genie_train_{fn}".encode() in msg, msg
    # the modes that exist still check the rest of the call
    assert L.genie_train_forward_ex(ok, None, 0, 0, 1, 0, 0, 0, 0, None, 1) == lib_mod.E_ARG
    assert b"NULL" in L.genie_last_error()


def test_bindings_and_version():
    lib_mod, L = lib()
    src = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(genie_[a-z0-9_]+)\s*\(", src))
    for n in EX_NAMES:
        assert n in declared, f"{n} is not declared in genie_hip.h"
        assert n in lib_mod.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(L, n), f"{n} is not exported"
    assert L.genie_version() == 3
    assert re.search(r"#define\s+GENIE_ABI_VERSION\s+3\b", src)
    # the trailing argument of each form is the int mode behind the arguments of the form it extends
    S = lib_mod.SIGNATURES
    import ctypes
    for ex, base in [("genie_train_activation_bytes_ex", "genie_train_activation_bytes"),
                     ("genie_train_workspace_bytes_ex", "genie_train_workspace_bytes"),
                     ("genie_train_forward_ex", "genie_train_forward_cond"),
                     ("genie_train_backward_head_ex", "genie_train_backward_head"),
                     ("genie_train_backward_layer_ex", "genie_train_backward_layer")]:
        assert S[ex][0] is S[base][0] and S[ex][1] == S[base][1] + [ctypes.c_int], ex


def test_header_compiles_as_c99_and_c_reaches_the_new_entry_points(tmp_path):
    """include/genie_hip.h stays plain C99 with the additions, and a C program linked against the library reads the two sizes and
    checks the bound itself (the pattern of tests/test_abi_and_host.py::test_header_is_plain_c_and_the_library_links_from_c)."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib_mod, _ = lib()
    so = lib_mod.LIB_PATH
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_cfg c; size_t a0, a1, one, ck;\n"
                   "    memset(&c, 0, sizeof c);\n"
                   "    c.num_layers = 32; c.num_heads = 8; c.head_dim = 64; c.d_model = 512; c.T = 16; c.S = 256; c.hidden = 2048;\n"
                   "    c.factored_vocab = 512; c.num_factored = 2; c.image_vocab_size = 262144; c.attn_scale = 0.125f; c.readout_mult = 1.0f;\n"
                   "    c.precision = GENIE_PREC_BF16;\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3) return 1;\n"
                   "    a0 = genie_train_activation_bytes_ex(&c, 2, 0); a1 = genie_train_activation_bytes_ex(&c, 2, 1);\n"
                   "    if (a0 == 0 || a0 != genie_train_activation_bytes(&c, 2)) return 2;\n"
                   "    if (genie_train_workspace_bytes_ex(&c, 2, 1) == 0 || genie_train_workspace_bytes_ex(&c, 2, 0) != genie_train_workspace_bytes(&c, 2)) return 3;\n"
                   "    ck = ((size_t)2 * 16 * 256 * 512 * 4 + 255) / 256 * 256;\n"
                   "    c.num_layers = 1; one = genie_train_activation_bytes(&c, 2); c.num_layers = 32;\n"
                   "    if (a1 == 0 || a1 > one + 32 * ck || a1 >= a0) return 4;\n"
                   "    if (genie_train_activation_bytes_ex(&c, 2, 2) != 0) return 5;\n"
                   "    if (genie_train_forward_ex(&c, NULL, NULL, NULL, 2, NULL, 0, NULL, NULL, NULL, 2) != GENIE_E_ARG) return 6;\n"
                   "    if (genie_train_backward_head_ex(&c, NULL, NULL, NULL, 2, NULL, NULL, 0, 0, NULL, -1) != GENIE_E_ARG) return 7;\n"
                   "    if (genie_train_backward_layer_ex(&c, NULL, NULL, NULL, 0, 2, NULL, NULL, 0, 0, NULL, -1) != GENIE_E_ARG) return 8;\n"
                   "    if (strstr(genie_last_error(), \"recompute\") == NULL) return 9;\n"
                   '    printf("%zu %zu\\n", a0, a1);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "abi"
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "abi.o")],
                   check=True)
    subprocess.run([gcc, str(tmp_path / "abi.o"), so, f"-Wl,-rpath,{os.path.dirname(so)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    a0, a1 = map(int, r.stdout.split())
    assert a0 > 10 * a1   # L 32: about a tenth

