"""The spatial attention backward and the qk-norm pair of the training step, each implementation on its own through
genie_spatial_attention_backward / genie_qk_norm_forward / genie_qk_norm_backward, against the float64 NumPy restatements of
tests/spatial_bwd_model.py (pinned to float64 torch autograd, and the bars shown to reject a table of wrong variants on these very
inputs, by tests/test_spatial_bwd_cpu.py).  n_frames = 3, two heads; flat (q x 1) and sharp (q x 4) softmax rows; q | k read from qkv
itself (qk_ld = 3 d) or from a separate buffer with other values (2 d).

  fused         attn_spatial_bwd_fused_kernel<32 | 64>: S = 256
  materialised  five gemm_f32_gen launches around softmax_rows / softmax_bwd_rows: S = 16 (one partial tile, one softmax trip; head_dim
                16 .. 128), S = 144 (128 + 16 rows, three trips), and forced at S = 256 on a fused input per head_dim
  auto          what the exact and f16x3 training step runs; which kernel ran is read from the profile's kernel table
  bf16          attn_bwd16_q_kernel + attn_bwd16_kv_kernel<32 | 64>: S = 256
Every attention output is pre-filled with NaN between two guard regions, and so is the workspace: every element written, nothing
outside, nothing read that the call did not write; a second call gives the same bits.

f32 bars (attention blocks dq, dk, dv; qk-norm blocks qkn / d_qk, d_norm_w, d_norm_b): the largest error over the block's largest
element is at most KERNEL_FACTOR = 4 times that of the SAME restatement run in f32, the bar of the temporal kernels
(tests/test_hip_train_long_window.py).

Measured on an MI355X (profiles/spatial_bwd_kernels.txt has every figure), kernel error / the f32 restatement's / largest ratio:
  fused          4.7e-7 .. 1.9e-6 / 4.4e-7 .. 2.1e-6 / 1.51 (head_dim 64, qk_ld 3 d, q x 4, dk)
  materialised   1.6e-7 .. 1.7e-6 / 1.2e-7 .. 1.4e-6 / 3.36 (S 16, head_dim 128, q x 4, dv; the next is 2.02, dq of the same case)
  auto           2.2e-7 .. 3.2e-6 / 1.9e-7 .. 3.7e-6 / 1.44
  qk-norm fwd    3.8e-6 .. 1.1e-5 / 3.8e-6 .. 1.1e-5 / 1.00 (the near-constant rows set both)
  qk-norm bwd    7.5e-8 .. 1.7e-5 / 7.5e-8 .. 2.2e-5 / 1.42 (d_norm_w, head_dim 128, 37 rows)
No kernel was over the bar, sharp rows included, so none was changed.

bf16 bars, per block: (1) the largest-element error against float64 is at most 2 x that of the bf16 number model (the restatement
with the kernels' roundings, float64 accumulation); (2) the Frobenius distance from the number model is at most BF16_MODEL_SHARE of
the model's own Frobenius distance from float64.  Measured on an MI355X over the 8 cases x 3 blocks: (1) kernel 3.5e-3 .. 1.2e-2,
model 3.5e-3 .. 1.2e-2, ratio 1.00 in all 24; (2) ratios, sorted: 0.0001 0.0004 0.0006 0.0006 0.0009 0.0009 0.0010 0.0017 0.0019 0.0023
0.0024 0.0026 0.0027 0.0048 0.0055 0.0059 0.0063 0.0068 0.0069 0.0074 0.0082 0.0196 0.0201 0.0512 (the largest: head_dim 64, qk_ld 3 d,
q x 4, dk).  BF16_MODEL_SHARE = 3 x 0.0512 = 0.154, under the cap of 0.25.
"""
import ctypes

import numpy as np
import pytest

import spatial_bwd_model as M
from conftest import pkg, record_measure

GUARD = 4096  # floats on either side of every output and workspace
FUSED, GEN, PAIR = "attn_spatial_bwd_fused_kernel", "gemm_f32_gen_kernel", "attn_bwd16_q_kernel + attn_bwd16_kv_kernel"


def dev(a):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(np.array(a)).to("cuda")   # (a copy: the cached inputs are read-only)


def guarded(n, fill=float("nan")):
    """n floats filled with `fill` between two guard regions of -7; (buffer, pointer to the n floats)."""
    torch = pytest.importorskip("torch")
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    buf[:GUARD] = -7.0
    buf[GUARD + n:] = -7.0
    return buf, buf.data_ptr() + 4 * GUARD


def inside(buf, n, what):
    """The n floats of a guarded buffer on the host, after checking that the guards are intact."""
    out = buf.cpu().numpy()
    assert (out[:GUARD] == -7.0).all() and (out[GUARD + n:] == -7.0).all(), f"a kernel wrote outside {what}"
    return out[GUARD:GUARD + n]


def path_id(path):
    lib = pkg("_lib")
    return {"auto": lib.SPATIAL_BWD_AUTO, "fused": lib.SPATIAL_BWD_FUSED, "materialised": lib.SPATIAL_BWD_MATERIALISED,
            "bf16": lib.SPATIAL_BWD_BF16}[path]


def run_attn(inp, path):
    """d_qkv (n, S, 3d) from genie_spatial_attention_backward by `path`, output and workspace NaN-filled between guards."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    qkv, qk, dO, H, scale = inp
    n, S, d3 = qkv.shape
    d = d3 // 3
    t_qkv, t_do = dev(qkv), dev(dO)
    t_qk = t_qkv if qk is qkv else dev(qk)
    out, out_ptr = guarded(n * S * d3)
    ws_bytes = L.genie_spatial_attention_backward_workspace_bytes(path_id(path), n, S, H)
    assert ws_bytes % 4 == 0
    ws, ws_ptr = guarded(ws_bytes // 4)
    lib.check(L.genie_spatial_attention_backward(t_qkv.data_ptr(), t_qk.data_ptr(), qk.shape[-1], t_do.data_ptr(), out_ptr, n, S, d, H,
                                                 d // H, scale, path_id(path), ws_ptr if ws_bytes else 0, ws_bytes,
                                                 torch.cuda.current_stream().cuda_stream), "genie_spatial_attention_backward")
    torch.cuda.synchronize()
    inside(ws, ws_bytes // 4, "the workspace")
    res = inside(out, n * S * d3, "d_qkv").reshape(n, S, d3)
    assert not np.isnan(res).any(), f"{int(np.isnan(res).sum())} elements of d_qkv were not written"
    return res


def tag_of(kind, S, Dh, ld3, q_mul):
    return f"spatial_bwd/{kind}/S{S}_Dh{Dh}_{'ld3d' if ld3 else 'ld2d'}_q{int(q_mul)}"


def check_f32(kind, path, S, Dh, ld3, q_mul):
    inp, ref, f32 = M.attn_case(S, Dh, ld3, q_mul)
    out = run_attn(inp, path)
    assert np.array_equal(out, run_attn(inp, path)), "a second call gave other bits"
    seen, bad = M.accept_f32(M.split3(out), ref, f32)
    for name, (err, floor) in seen.items():
        tag = f"{tag_of(kind, S, Dh, ld3, q_mul)}/{name}"
        record_measure(tag, err)
        record_measure(tag + "_f32_restatement", floor)
        print(f"{tag}: kernel {err:.3e}, f32 restatement {floor:.3e}, ratio {err / floor:.2f}")
    assert not bad, bad


def launched_by(fn):
    """{kernel name: launches} of the GEMM and spatial-attention classes while fn() runs (the profile's kernel table, as
    tests/test_hip_train_geometry.py reads it)."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    launched = {}
    lib.check(L.genie_profile_enable((1 << lib.KC_GEMM) | (1 << lib.KC_ATTN_SPATIAL)), "profile_enable")
    L.genie_profile_reset()
    try:
        fn()
        torch.cuda.synchronize()
        for kc in (lib.KC_GEMM, lib.KC_ATTN_SPATIAL):
            kbuf = ctypes.create_string_buffer(16384)
            lib.check(L.genie_profile_kernels(kc, kbuf, len(kbuf)), "profile_kernels")
            launched.update({ln.split("\t")[0]: int(float(ln.split("\t")[1])) for ln in kbuf.value.decode().splitlines() if "\t" in ln})
    finally:
        L.genie_profile_enable(0)
    return launched


# ---------------------------------------------------------------------------------------------- f32 paths
@pytest.mark.gpu
@pytest.mark.parametrize("q_mul", [1.0, 4.0])
@pytest.mark.parametrize("ld3", [True, False], ids=["ld3d", "ld2d"])
@pytest.mark.parametrize("Dh", [32, 64])
def test_fused_vs_float64_restatement(Dh, ld3, q_mul):
    """attn_spatial_bwd_fused_kernel<Dh> at S = 256: dq, dk, dv within 4 x the f32 restatement's distance from the float64 one."""
    check_f32("fused", "fused", 256, Dh, ld3, q_mul)


MATERIALISED = [(16, 16, False, 4.0), (16, 32, True, 1.0), (16, 64, False, 1.0), (16, 128, True, 4.0),
                (144, 32, False, 4.0), (144, 32, True, 1.0), (144, 64, True, 4.0), (144, 64, False, 1.0),
                (256, 32, False, 4.0), (256, 64, True, 4.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,Dh,ld3,q_mul", MATERIALISED)
def test_materialised_vs_float64_restatement(S, Dh, ld3, q_mul):
    """The materialised path at the same bar: S = 16, S = 144, and forced at S = 256 on two sharp inputs of the fused cases, so
    that both f32 implementations are judged against one reference."""
    check_f32("materialised", "materialised", S, Dh, ld3, q_mul)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Dh,kernel", [(256, 32, FUSED), (256, 64, FUSED), (256, 128, GEN), (144, 64, GEN), (16, 16, GEN)])
def test_auto_takes_the_expected_kernel(S, Dh, kernel):
    """GENIE_SPATIAL_BWD_AUTO, the training step's f32 choice: one fused launch at S = 256 with head_dim 32 / 64, five gemm_f32_gen
    launches everywhere else (head_dim 128 at S = 256 included) and nothing of the other kind; the result at the f32 bar."""
    inp, ref, f32 = M.attn_case(S, Dh, False, 4.0)
    res = []
    launched = launched_by(lambda: res.append(run_attn(inp, "auto")))
    assert launched.get(kernel, 0) == (1 if kernel == FUSED else 5), launched
    assert not launched.get(GEN if kernel == FUSED else FUSED, 0) and not launched.get(PAIR, 0), launched
    seen, bad = M.accept_f32(M.split3(res[0]), ref, f32)
    for name, (err, floor) in seen.items():
        record_measure(f"{tag_of('auto', S, Dh, False, 4.0)}/{name}", err)
        record_measure(f"{tag_of('auto', S, Dh, False, 4.0)}/{name}_f32_restatement", floor)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- bf16 pair
@pytest.mark.gpu
@pytest.mark.parametrize("q_mul", [1.0, 4.0])
@pytest.mark.parametrize("ld3", [True, False], ids=["ld3d", "ld2d"])
@pytest.mark.parametrize("Dh", [32, 64])
def test_bf16_pair_vs_number_model(Dh, ld3, q_mul):
    """attn_bwd16_q_kernel + attn_bwd16_kv_kernel at S = 256: per block, within 2 x the number model's distance from float64, and
    within BF16_MODEL_SHARE of that distance (Frobenius) from the number model itself; the pair is what ran."""
    inp, ref, _ = M.attn_case(256, Dh, ld3, q_mul)
    model = M.bf16_model(256, Dh, ld3, q_mul)
    res = []
    launched = launched_by(lambda: res.append(run_attn(inp, "bf16")))
    assert launched.get(PAIR, 0) == 1 and not launched.get(FUSED, 0) and not launched.get(GEN, 0), launched
    assert np.array_equal(res[0], run_attn(inp, "bf16")), "a second call gave other bits"
    seen, bad = M.accept_bf16(M.split3(res[0]), ref, model)
    for name, (err, floor, ratio) in seen.items():
        tag = f"{tag_of('bf16', 256, Dh, ld3, q_mul)}/{name}"
        record_measure(tag, err)
        record_measure(tag + "_number_model", floor)
        record_measure(tag + "_model_share", ratio)
        print(f"{tag}: kernel {err:.3e}, number model {floor:.3e}, ratio {err / floor:.2f}; share of the model's distance {ratio:.4f}")
    assert not bad, (bad, M.BF16_MODEL_SHARE)


# ---------------------------------------------------------------------------------------------- qk-norm
def run_qk_norm_fwd(qkv, nw, nb, H):
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    rows, d3 = qkv.shape
    d = d3 // 3
    t_qkv, t_w, t_b = dev(qkv), dev(nw), dev(nb)
    out, out_ptr = guarded(rows * 2 * d)
    lib.check(L.genie_qk_norm_forward(t_qkv.data_ptr(), out_ptr, t_w.data_ptr(), t_b.data_ptr(), rows, H, d // H,
                                      torch.cuda.current_stream().cuda_stream), "genie_qk_norm_forward")
    torch.cuda.synchronize()
    res = inside(out, rows * 2 * d, "qkn").reshape(rows, 2 * d)
    assert not np.isnan(res).any(), f"{int(np.isnan(res).sum())} elements of qkn were not written"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("Dh,rows,H", M.QKNORM_CASES)
def test_qk_norm_forward(Dh, rows, H):
    """qk_norm_fwd_kernel<Dh>: qkn within 4 x the f32 restatement's distance from the float64 one, fully written, guards intact, the
    same bits on a second call."""
    (qkv, dy, nw, nb), ref, f32, _, _ = M.qk_norm_case(Dh, rows, H)
    out = run_qk_norm_fwd(qkv, nw, nb, H)
    assert np.array_equal(out, run_qk_norm_fwd(qkv, nw, nb, H))
    seen, bad = M.accept_blocks(("qkn",), (out,), (ref,), (f32,))
    err, floor = seen["qkn"]
    record_measure(f"spatial_bwd/qk_norm_fwd/Dh{Dh}_rows{rows}_H{H}/qkn", err)
    record_measure(f"spatial_bwd/qk_norm_fwd/Dh{Dh}_rows{rows}_H{H}/qkn_f32_restatement", floor)
    print(f"qk_norm_fwd Dh{Dh} rows{rows} H{H}: kernel {err:.3e}, f32 restatement {floor:.3e}, ratio {err / floor:.2f}")
    assert not bad, bad


def run_qk_norm_bwd(qkv, dy, nw, H, v_cols, want_w=True, want_b=True, pre=None, scratch=True):
    """(d_qkv (rows, 3d) after the call, d_norm_w or None, d_norm_b or None, scratch floats).  d_qkv holds dy | v_cols and sits
    between guards; d_norm_w / d_norm_b are NaN-filled (accumulate = 0) or hold `pre` = (w, b) (accumulate = 1); the scratch is
    filled with -7 throughout and returned."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    rows, d3 = qkv.shape
    d, Dh = d3 // 3, d3 // 3 // H
    t_qkv, t_w = dev(qkv), dev(nw)
    g, g_ptr = guarded(rows * d3)
    g[GUARD:GUARD + rows * d3] = dev(np.concatenate([dy, v_cols], axis=1).reshape(-1))
    params = []
    for k, want in enumerate((want_w, want_b)):
        buf, ptr = guarded(Dh)
        if pre is not None:
            buf[GUARD:GUARD + Dh] = dev(pre[k])
        params.append((buf, ptr if want else 0))
    sc_floats = L.genie_qk_norm_backward_scratch_bytes(Dh) // 4
    sc, sc_ptr = guarded(sc_floats, fill=-7.0)
    lib.check(L.genie_qk_norm_backward(t_qkv.data_ptr(), g_ptr, t_w.data_ptr(), params[0][1], params[1][1], rows, H, Dh,
                                       1 if pre is not None else 0, sc_ptr if scratch else 0, 4 * sc_floats if scratch else 0,
                                       torch.cuda.current_stream().cuda_stream), "genie_qk_norm_backward")
    torch.cuda.synchronize()
    res = inside(g, rows * d3, "d_qkv").reshape(rows, d3)
    return res, inside(params[0][0], Dh, "d_norm_w"), inside(params[1][0], Dh, "d_norm_b"), inside(sc, sc_floats, "the scratch")


@pytest.mark.gpu
@pytest.mark.parametrize("Dh,rows,H", M.QKNORM_CASES)
def test_qk_norm_backward(Dh, rows, H):
    """qk_norm_bwd_kernel<Dh, true> and the reductions behind it: d (raw q | k), d_norm_w, d_norm_b within 4 x the f32
    restatement's distance from the float64 one; NaN-filled gradients are overwritten with accumulate = 0 and pre-filled ones added
    to with accumulate = 1 (out = 1.0 * old + sum: exactly the f32 sum of the two); the v columns keep their bits; a second call
    gives the same bits."""
    (qkv, dy, nw, nb), _, _, ref, f32 = M.qk_norm_case(Dh, rows, H)
    d = H * Dh
    g = np.random.default_rng(Dh + rows)
    v_cols = g.standard_normal((rows, d)).astype(np.float32)
    v_cols[0, 0] = np.float32("nan")                      # neither read nor written: any bits survive
    out, dnw, dnb, _ = run_qk_norm_bwd(qkv, dy, nw, H, v_cols)
    assert np.array_equal(out[:, 2 * d:].view(np.uint32), v_cols.view(np.uint32)), "the v columns of d_qkv changed"
    assert not np.isnan(out[:, :2 * d]).any() and not np.isnan(dnw).any() and not np.isnan(dnb).any()
    out2, dnw2, dnb2, _ = run_qk_norm_bwd(qkv, dy, nw, H, v_cols)
    assert np.array_equal(out[:, :2 * d], out2[:, :2 * d]) and np.array_equal(dnw, dnw2) and np.array_equal(dnb, dnb2)
    names = ("d_qk", "d_norm_w", "d_norm_b")
    seen, bad = M.accept_blocks(names, (out[:, :2 * d], dnw, dnb), ref, f32)
    for name, (err, floor) in seen.items():
        tag = f"spatial_bwd/qk_norm_bwd/Dh{Dh}_rows{rows}_H{H}/{name}"
        record_measure(tag, err)
        record_measure(tag + "_f32_restatement", floor)
        print(f"{tag}: kernel {err:.3e}, f32 restatement {floor:.3e}, ratio {err / max(floor, 1e-30):.2f}")
    assert not bad, bad
    pre = (g.standard_normal(Dh).astype(np.float32), g.standard_normal(Dh).astype(np.float32))
    out3, dnw3, dnb3, _ = run_qk_norm_bwd(qkv, dy, nw, H, v_cols, pre=pre)
    assert np.array_equal(out3[:, :2 * d], out[:, :2 * d])
    assert np.array_equal(dnw3, pre[0] + dnw) and np.array_equal(dnb3, pre[1] + dnb)


@pytest.mark.gpu
@pytest.mark.parametrize("Dh,rows,H", M.QKNORM_CASES)
def test_qk_norm_backward_with_frozen_affine(Dh, rows, H):
    """d_norm_w NULL, d_norm_b NULL, both NULL: the same d (raw q | k) at the same bar (the same bits, in fact: one kernel body),
    the gradient that is asked for in the bits of the full call, the absent one's buffer untouched, and with both NULL
    (qk_norm_bwd_kernel<Dh, false>, no reduction) a scratch that is not written -- or not there at all."""
    (qkv, dy, nw, nb), _, _, ref, f32 = M.qk_norm_case(Dh, rows, H)
    d = H * Dh
    v_cols = np.zeros((rows, d), np.float32)
    full, dnw, dnb, _ = run_qk_norm_bwd(qkv, dy, nw, H, v_cols)
    for want_w, want_b in ((False, True), (True, False), (False, False)):
        out, w, b, sc = run_qk_norm_bwd(qkv, dy, nw, H, v_cols, want_w=want_w, want_b=want_b)
        assert not M.accept_blocks(("d_qk",), (out[:, :2 * d],), ref[:1], f32[:1])[1]
        assert np.array_equal(out, full)
        assert np.array_equal(w, dnw) if want_w else np.isnan(w).all()
        assert np.array_equal(b, dnb) if want_b else np.isnan(b).all()
        if not (want_w or want_b):
            assert (sc == -7.0).all(), "the parameter-free kernel wrote to the scratch"
            out, *_ = run_qk_norm_bwd(qkv, dy, nw, H, v_cols, want_w=False, want_b=False, scratch=False)
            assert np.array_equal(out, full)
