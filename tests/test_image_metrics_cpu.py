"""CPU-only tests of the image-space metrics: the f64 NumPy model (tests/image_metrics_model.py) against scipy's Gaussian filter and against
closed forms, the C ABI additions (declared, exported, bound, the header as C99, argument errors before any HIP call), the built kernels'
scratch, and the Python refusals that need no device."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import image_metrics_model as M
from conftest import REPO, pkg

torch = pytest.importorskip("torch")

NEW = ("genie_frame_metrics_workspace_bytes", "genie_frame_metrics")
TILE_BYTES = 24   # one workspace record per (image, channel, 32 x 32 tile of window positions)


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


# ------------------------------------------------------------------ the model
def _scipy_ssim_mean(a, b):
    """The form skimage averages: scipy's Gaussian filter (sigma 1.5, truncate 3.5 = radius 5, reflect), cropped by 5."""
    ndi = pytest.importorskip("scipy.ndimage")

    def filt(v):
        return ndi.gaussian_filter(v, sigma=M.SIGMA, truncate=3.5, mode="reflect")[5:-5, 5:-5]

    x, y = a.astype(np.float64), b.astype(np.float64)
    mx, my = filt(x), filt(y)
    vx, vy, cxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    return (((2 * mx * my + M.C1) * (2 * cxy + M.C2)) / ((mx * mx + my * my + M.C1) * (vx + vy + M.C2))).mean()


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_equals_the_scipy_gaussian_filter_form(shape):
    worst = 0.0
    for content in M.CONTENTS:
        a, b = M.make_pair(content, 1, shape)
        mine = M.frame_metrics(a, b)["ssim"][0]
        ref = np.mean([_scipy_ssim_mean(a[0, c], b[0, c]) for c in range(shape[0])])
        worst = max(worst, abs(mine - ref))
        assert abs(mine - ref) < 1e-12, (content, mine, ref)
    print(f"model vs scipy {shape}: {worst:.2e}")


def test_taps_are_the_stated_window():
    g = M.taps()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-15 and abs(g[0] / g[5] - np.exp(-25 / 4.5)) < 1e-15
    assert abs(M.C1 - 6.5025) < 1e-12 and abs(M.C2 - 58.5225) < 1e-12


def test_model_closed_forms_and_symmetry():
    for shape in M.SHAPES[:4]:
        a, _ = M.make_pair("noise", 2, shape)
        sse, sae, ss, n_win = M.frame_sums(a, a)
        assert n_win == shape[0] * (shape[1] - 10) * (shape[2] - 10)
        assert np.all(sse == 0) and np.all(sae == 0) and np.allclose(ss / n_win, 1.0, rtol=0, atol=1e-12)
        assert np.all(np.isposinf(M.frame_metrics(a, a)["psnr"]))
        # black against white: both variances and the covariance vanish, mu_x = 0, mu_y = 255
        k, w = M.make_pair("black_white", 1, shape)
        closed = (M.C1 * M.C2) / ((255.0 ** 2 + M.C1) * M.C2)
        got = M.frame_metrics(k, w)
        assert abs(closed - 9.999e-5) < 1e-8 and abs(got["ssim"][0] - closed) < 1e-12
        assert got["mse"][0] == 255.0 ** 2 and got["mae"][0] == 255.0 and got["psnr"][0] == 0.0
        # symmetric in its arguments
        for content in ("noise", "smooth", "flat", "one_pixel"):
            a, b = M.make_pair(content, 2, shape)
            ab, ba = M.frame_sums(a, b), M.frame_sums(b, a)
            assert np.array_equal(ab[0], ba[0]) and np.array_equal(ab[1], ba[1]) and np.allclose(ab[2], ba[2], rtol=1e-14, atol=0)
    a, b = M.make_pair("one_pixel", 1, (3, 12, 37))
    assert M.frame_sums(a, b)[0][0] == 128 ** 2 and M.frame_sums(a, b)[1][0] == 128
    lead = M.frame_metrics(*(v.reshape(1, 1, 3, 12, 37) for v in (a, b)))
    assert lead["psnr"].shape == (1, 1) and abs(lead["psnr"][0, 0] - 10 * np.log10(255.0 ** 2 * 3 * 12 * 37 / 128 ** 2)) < 1e-12


# ------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    assert "#define GENIE_ABI_VERSION 3" in header
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    for stated in ("sigma 1.5", "exp(-r^2 / 4.5)", "(0.01 * 255)^2", "(0.03 * 255)^2", "C * (H - 10) * (W - 10)"):
        assert stated in header, stated
    assert "kernels_metrics.hip" in pkg("build").SOURCES


def test_workspace_bytes_and_refusals_before_any_hip_call():
    """Every check below returns from host code: the fake device pointers are never dereferenced, nothing is launched."""
    lib_mod, L = _lib()
    fake = 1 << 20
    wsb = L.genie_frame_metrics_workspace_bytes
    assert wsb(1, 1, 11, 11) == TILE_BYTES and wsb(5, 3, 12, 37) == 5 * 3 * TILE_BYTES
    assert wsb(1, 3, 75, 131) == 3 * 3 * 4 * TILE_BYTES and wsb(240, 3, 256, 256) == 240 * 3 * 64 * TILE_BYTES
    assert wsb(1, 1, 42, 43) == TILE_BYTES * 2 and wsb(0, 3, 64, 64) == 0
    assert wsb(-1, 3, 64, 64) == 0 and wsb(1, 0, 64, 64) == 0 and wsb(1, 3, 10, 64) == 0 and wsb(1, 3, 64, 10) == 0

    def call(a=fake, b=fake, n=2, C=3, H=64, W=80, out=fake, ws=fake, nbytes=None):
        return L.genie_frame_metrics(a, b, n, C, H, W, out, ws, wsb(max(n, 0), C, H, W) if nbytes is None else nbytes, None)

    E, S = lib_mod.E_ARG, lib_mod.E_SHAPE
    assert call(a=None) == E and call(b=None) == E and call(out=None) == E
    assert call(n=-1) == E and call(C=0) == E
    assert call(ws=None) == E and call(nbytes=wsb(2, 3, 64, 80) - 1) == E and call(ws=fake + 4) == E
    assert b"genie_frame_metrics" in L.genie_last_error()
    assert call(H=10) == S and call(W=10) == S and call(H=10, n=0) == S
    assert b"11 x 11" in L.genie_last_error()
    # one workgroup per (image, channel, tile): at most 2^31 - 1 of them in a call
    assert wsb((1 << 31) - 1, 1, 11, 11) == ((1 << 31) - 1) * TILE_BYTES and wsb(1 << 31, 1, 11, 11) == 0
    assert call(n=1 << 31, C=1, H=11, W=11, nbytes=0) == S and call(n=1 << 62, C=3, H=256, W=256, nbytes=0) == S
    assert call(n=0) == 0 and call(n=0, ws=None, nbytes=0) == 0      # n == 0: success, nothing needed


def test_header_compiles_as_c99_and_c_reaches_the_new_entry_points(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib_mod, _ = _lib()
    src = tmp_path / "fm.c"
    src.write_text('#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    static uint8_t px[4]; double out[4]; double ws[3];\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3) return 1;\n"
                   "    if (genie_frame_metrics_workspace_bytes(1, 1, 11, 11) != sizeof ws) return 2;\n"
                   "    if (genie_frame_metrics_workspace_bytes(1, 3, 10, 11) != 0) return 3;\n"
                   "    if (genie_frame_metrics(px, px, 1, 3, 10, 11, out, ws, sizeof ws, 0) != GENIE_E_SHAPE) return 4;\n"
                   "    if (strstr(genie_last_error(), \"11 x 11\") == 0) return 5;\n"
                   "    if (genie_frame_metrics(0, px, 1, 3, 11, 11, out, ws, sizeof ws, 0) != GENIE_E_ARG) return 6;\n"
                   "    if (genie_frame_metrics(px, px, 0, 3, 11, 11, out, 0, 0, 0) != GENIE_OK) return 7;\n"
                   "    return 0;\n}\n")
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "fm.o")], check=True)
    exe = tmp_path / "fm"
    subprocess.run([gcc, str(tmp_path / "fm.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_metrics_kernels_use_no_scratch():
    """The built code object (tools/isa_audit.py) and the compiler's own report of the source (tools/kernel_resources.py): 0 scratch bytes."""
    LLVM = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod, _ = _lib()
    rows = {r[0]: r for r in _tool("isa_audit").audit(lib_mod.LIB_PATH, all_kernels=True)}
    got = {k: v for k, v in rows.items() if "frame_metrics" in k}
    assert any("frame_metrics_tile_kernel" in k for k in got) and any("frame_metrics_finish_kernel" in k for k in got), list(got)
    for name, r in got.items():
        assert r[6] == 0, f"{name}: {r[6]} bytes of scratch per lane"
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        return
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"),
                          os.path.join(REPO, "1xgpt_amd", "csrc", "kernels_metrics.hip")], capture_output=True, text=True).stdout
    lines = [ln.split() for ln in out.splitlines() if "frame_metrics" in ln]
    assert len(lines) == 2, out
    for ln in lines:      # columns from the right: lds, occ, vspill, scratch
        assert int(ln[-4]) == 0 and int(ln[-3]) <= 0, ln


# ------------------------------------------------------------------ Python refusals that need no device
def test_python_refusals():
    IM = pkg("image_metrics")
    ok = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        IM.frame_metrics(ok.float(), ok)
    with pytest.raises(TypeError, match="uint8"):
        IM.frame_metrics(ok, ok.to(torch.int16))
    with pytest.raises(ValueError, match="differ in shape"):
        IM.frame_metrics(ok, ok[:1])
    with pytest.raises(ValueError, match="11 x 11"):
        IM.frame_metrics(ok[..., :10], ok[..., :10])
    with pytest.raises(ValueError, match="11 x 11"):
        IM.frame_metrics(ok[..., :10, :], ok[..., :10, :])
    with pytest.raises(ValueError, match=r"\(\.\.\., C, H, W\)"):
        IM.frame_metrics(ok[0, 0], ok[0, 0])
    # a well-formed CPU pair reaches the device check
    with pytest.raises(RuntimeError, match=r"runs on the GPU only \(no CPU fallback\)"):
        IM.frame_metrics(ok, ok)
    with pytest.raises(RuntimeError, match=r"runs on the GPU only \(no CPU fallback\)"):
        pkg("eval_utils").compute_image_metrics(ok[None], ok[None])
    assert IM.FrameMetrics._fields == ("mse", "mae", "psnr", "ssim") and IM.PSNR_CAP == 100.0


def test_evaluator_keywords_and_cli_flag_exist():
    import inspect
    E = pkg("evaluate")
    assert inspect.signature(E.evaluate_clips).parameters["image_metrics"].default is False
    assert inspect.signature(E.evaluate_clips).parameters["psnr_cap"].default == 100.0
    assert inspect.signature(E.run_reference_style_loop).parameters["decode_image_metrics"].default is False
    assert hasattr(pkg("magvit2").VQModel, "reconstruction_metrics")
    ap = _tool("evaluate").build_parser()
    assert ap.parse_args(["--synthetic", "2", "--image_metrics"]).image_metrics and not ap.parse_args([]).image_metrics

    class NoDecoder:
        decode_latents, device = None, "cpu"
        model = type("m", (), {"config": type("c", (), {"T": 4})})
    with pytest.raises(RuntimeError, match="decode_latents"):
        E.evaluate_clips(NoDecoder(), torch.zeros(1, 4), image_metrics=True)
