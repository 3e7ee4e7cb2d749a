"""NumPy references for the spatial attention backward and the qk-norm pair of the training step, each kernel on its own
(genie_spatial_attention_backward, genie_qk_norm_forward, genie_qk_norm_backward), and the acceptance functions of
tests/test_hip_spatial_bwd.py.  No GPU here: tests/test_spatial_bwd_cpu.py pins the references to float64 torch autograd and shows
that every acceptance function rejects a table of wrong variants (the `mutant` arguments below) on the inputs the GPU tests use.

attn_bwd_restated is the non-causal counterpart of the restatement in tests/test_hip_train_long_window.py.  With round=bf16 it is
the number model of csrc/kernels_attn_bwd16.hip, each rounding where the two kernels round:
  * Q, K, V, dO are rounded when they are staged (stage_256xDH, pack8 of the per-lane fragments): every product reads rounded operands;
  * the scores, the softmax (max, sum, 1 / sum) and dP = dO V^T are f32 and NOT rounded;
  * D_i = sum_j P_ij dP_ij is formed from the UNROUNDED P and dP (attn_bwd16_q_kernel sweep 2: fmaf over the f32 exponentials and the
    f32 dP tile, times 1 / sum) and handed to the second kernel as it is;
  * dS = P (dP - D) is formed from unrounded P, dP, D and rounded once, as the A operand of dQ = dS K and of dK = dS^T Q;
  * P is rounded once, as the A operand of dV = P^T dO;
  * the accumulators and the final `* scale` are f32.
"""
import functools

import numpy as np

KERNEL_FACTOR = 4.0          # f32 kernels: bar = KERNEL_FACTOR x |f32 restatement - float64 restatement| (the temporal kernels' bar)
BF16_FLOAT64_FACTOR = 2.0    # bf16 pair: largest-element error against float64 <= this x the number model's own distance
BF16_MODEL_SHARE_CAP = 0.25
# Frobenius distance of the bf16 pair from its number model as a share of the model's own distance from float64: 3 x the largest
# ratio measured on an MI355X over the 8 cases x 3 blocks of tests/test_hip_spatial_bwd.py (0.0512: head_dim 64, qk_ld 3 d, q x 4, dk;
# the other 23 are 0.0001 .. 0.0201 -- profiles/spatial_bwd_kernels.txt), never above the cap.  The 3 is for the roundings of P and dS
# that flip under another summation order: the CPU stand-in (f32 accumulation) varies 10x between seeds.
BF16_MODEL_SHARE = min(BF16_MODEL_SHARE_CAP, 3 * 0.0512)
N_FRAMES, HEADS = 3, 2       # an odd frame count; blockIdx.x / H with H > 1
EPS = 1e-5


# ---------------------------------------------------------------------------------------------- number formats
def bf16(a):
    """Round to the nearest bf16 (ties to even), result in a's dtype -- f32_to_bf16 of csrc/common.hpp for finite values."""
    a = np.asarray(a)
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(a.dtype)


def f16(a):
    a = np.asarray(a)
    return a.astype(np.float16).astype(a.dtype)


# ---------------------------------------------------------------------------------------------- measures
def rel_err(a, ref):
    """The largest error over the tensor's largest element."""
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


def fro(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def split3(a):
    d = a.shape[-1] // 3
    return a[..., :d], a[..., d:2 * d], a[..., 2 * d:]


# ---------------------------------------------------------------------------------------------- attention backward
def attn_bwd_restated(qkv, qk, dO, H, scale, dtype, round=None, mutant=None):
    """dq, dk, dv (n_frames, S, d) each of softmax(scale q k^T) v over the S tokens of a frame, every operation in `dtype`.
    qkv (n, S, 3d) gives v; q | k are the first 2d columns of qk ((n, S, 2d) or qkv itself).  round: None, or the function that
    rounds the operands of the products (see the top of this file).  mutant: one of the wrong variants of MUTANTS_*."""
    n, S, d3 = qkv.shape
    d = d3 // 3
    Dh = d // H
    if mutant == "qk_from_qkv":
        qk = qkv
    r = round if round is not None else (lambda a: a)
    f = lambda a: r(a.astype(dtype)).reshape(n, S, H, Dh).transpose(0, 2, 1, 3)  # noqa: E731   (n, H, S, Dh)
    t = lambda a: a.transpose(0, 1, 3, 2)  # noqa: E731
    q, k, v, do = f(qk[..., :d]), f(qk[..., d:2 * d]), f(qkv[..., 2 * d:]), f(dO)
    if mutant == "v_head0":
        v = np.broadcast_to(v[:, :1], v.shape)
    sc = dtype(scale)
    s = (q @ t(k)) * sc                                                  # (n, H, i, j)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    if mutant == "p_bf16_in_f32":
        p = bf16(p)
    dp = do @ t(v)
    pdp = p * dp
    D = (pdp[..., :S - 64] if mutant == "D_without_last_64_keys" else pdp).sum(-1, keepdims=True)
    ds = p * (dp - D)
    ds_a = ds if mutant == "ds_not_rounded" else r(ds)
    p_a = bf16(f16(p)) if mutant == "p_through_f16" else r(p)
    dq = (ds_a @ k) * sc
    iq = S - 32 if mutant == "dkdv_without_last_query_block" else S
    dk = (t(ds_a[:, :, :iq]) @ q[:, :, :iq]) * sc
    dv = t(p_a[:, :, :iq]) @ do[:, :, :iq]
    assert all(a.dtype == dtype for a in (dq, dk, dv))
    return tuple(np.ascontiguousarray(a.transpose(0, 2, 1, 3).reshape(n, S, d)) for a in (dq, dk, dv))


def row_max_probability(qk, H, scale):
    """(n, H, S): the largest probability of every softmax row, float64."""
    n, S, w = qk.shape
    d = w // 2 if w % 3 else w // 3
    q = qk[..., :d].astype(np.float64).reshape(n, S, H, d // H)
    k = qk[..., d:2 * d].astype(np.float64).reshape(n, S, H, d // H)
    s = np.einsum("nihc,njhc->nhij", q, k) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).max(-1)


def kernel_inputs(S, Dh, ld3, q_mul, seed=0, H=HEADS, n_frames=N_FRAMES):
    """Standard-normal qkv, q scaled by q_mul, dO scaled by 1e-3 (the inputs of tests/test_hip_train_long_window.py).  ld3: q | k are
    read from qkv itself; else from a separate (n, S, 2d) buffer with DIFFERENT values, so that reading the wrong source fails."""
    d = H * Dh
    g = np.random.default_rng(100000 * S + 10 * Dh + seed)
    qkv = g.standard_normal((n_frames, S, 3 * d)).astype(np.float32)
    qkv[..., :d] *= np.float32(q_mul)
    if ld3:
        qk = qkv
    else:
        qk = g.standard_normal((n_frames, S, 2 * d)).astype(np.float32)
        qk[..., :d] *= np.float32(q_mul)
    dO = (g.standard_normal((n_frames, S, d)) * 1e-3).astype(np.float32)
    return qkv, qk, dO, H, float(Dh) ** -0.5


@functools.lru_cache(maxsize=None)
def attn_case(S, Dh, ld3, q_mul, seed=0):
    """(inputs, float64 restatement, f32 restatement): computed once, shared, never written to."""
    inp = kernel_inputs(S, Dh, ld3, q_mul, seed)
    ref = attn_bwd_restated(*inp, np.float64)
    f32 = attn_bwd_restated(*inp, np.float32)
    for a in inp[:3] + ref + f32:
        a.setflags(write=False)
    return inp, ref, f32


@functools.lru_cache(maxsize=None)
def bf16_model(S, Dh, ld3, q_mul, seed=0):
    """The bf16 number model with float64 accumulation on attn_case's inputs."""
    out = attn_bwd_restated(*attn_case(S, Dh, ld3, q_mul, seed)[0], np.float64, round=bf16)
    for a in out:
        a.setflags(write=False)
    return out


def accept_f32(got, ref, f32, factor=KERNEL_FACTOR):
    """got, ref (float64), f32: tuples of blocks.  ({block: (error, floor)} for every block, {block: ...} for the blocks over the bar):
    largest error over the block's largest element <= factor x the f32 restatement's own."""
    names = ("dq", "dk", "dv") if len(got) == 3 else tuple(f"b{i}" for i in range(len(got)))
    seen = {nm: (rel_err(g, r64), rel_err(r32, r64)) for nm, g, r64, r32 in zip(names, got, ref, f32)}
    return seen, {nm: v for nm, v in seen.items() if not v[0] <= factor * v[1]}


def accept_bf16(got, ref, model, share=BF16_MODEL_SHARE):
    """The two assertions of the bf16 pair per block.  ({block: (error vs float64, model's error vs float64, Frobenius distance from
    the model / the model's Frobenius distance from float64)}, the blocks that fail either)."""
    seen, bad = {}, {}
    for nm, g, r64, m in zip(("dq", "dk", "dv"), got, ref, model):
        err, floor = rel_err(g, r64), rel_err(m, r64)
        ratio = fro(np.asarray(g, dtype=np.float64) - m) / fro(m - r64)
        seen[nm] = (err, floor, ratio)
        if not (err <= BF16_FLOAT64_FACTOR * floor and ratio <= share):
            bad[nm] = seen[nm]
    return seen, bad


MUTANTS_F32 = ("D_without_last_64_keys", "dkdv_without_last_query_block", "p_bf16_in_f32", "v_head0")
MUTANTS_BF16 = ("ds_not_rounded", "p_through_f16", "D_without_last_64_keys", "dkdv_without_last_query_block", "v_head0")
# (qk_from_qkv applies to either, on the qk_ld = 2 d inputs)


# ---------------------------------------------------------------------------------------------- qk-norm
def _heads(a, H):
    rows, w = a.shape
    return a.reshape(rows, 2, H, w // (2 * H))


def qk_norm_fwd_restated(qkv, nw, nb, H, dtype):
    """qkn (rows, 2d) = [LN(q) | LN(k)]: LayerNorm over head_dim of every q and k head row (attention.py: q_norm / k_norm share one
    nn.LayerNorm(head_dim), eps 1e-5), every operation in `dtype`."""
    rows, d3 = qkv.shape
    d = d3 // 3
    x = _heads(qkv[:, :2 * d].astype(dtype), H)
    xc = x - x.mean(-1, keepdims=True)
    rstd = dtype(1) / np.sqrt((xc * xc).mean(-1, keepdims=True) + dtype(EPS))
    return (xc * rstd * nw.astype(dtype) + nb.astype(dtype)).reshape(rows, 2 * d)


def qk_norm_bwd_restated(qkv, dy, nw, H, dtype, mutant=None):
    """d (raw q | k) (rows, 2d), d_norm_w, d_norm_b (head_dim) from dy (rows, 2d) = d loss / d (normalised q | k)."""
    rows, d3 = qkv.shape
    d = d3 // 3
    x, g = _heads(qkv[:, :2 * d].astype(dtype), H), _heads(dy.astype(dtype), H)
    xc = x - x.mean(-1, keepdims=True)
    rstd = dtype(1) / np.sqrt((xc * xc).mean(-1, keepdims=True) + dtype(EPS))
    xh = xc * rstd
    gy = g * nw.astype(dtype)
    s1, s2 = gy.mean(-1, keepdims=True), (gy * xh).mean(-1, keepdims=True)
    dx = (gy - s1 - (0 if mutant == "without_xh_s2" else xh * s2)) * rstd
    both = slice(0, 1) if mutant == "affine_over_q_only" else slice(0, 2)
    dnw = (g * xh)[:, both].sum((0, 1, 2))
    dnb = g[:, both].sum((0, 1, 2))
    return dx.reshape(rows, 2 * d), dnw, dnb


MUTANTS_QKNORM = ("without_xh_s2", "affine_over_q_only")

# (head_dim, rows, H): rows * 2 * H items against a block of 1024 / head_dim items and the backward's grid of 512 blocks --
# less than one block; no multiple of a block; one full grid (16384 / 8192 / 4096 items) and a little more, so that the backward's
# grid-stride loop takes a second trip
QKNORM_CASES = [
    (32, 3, 1), (32, 37, 3), (32, 4200, 2),
    (64, 3, 1), (64, 37, 3), (64, 2100, 2),
    (128, 3, 1), (128, 37, 3), (128, 1100, 2),
]


def qk_norm_inputs(Dh, rows, H, seed=0):
    """qkv (rows, 3d) standard normal with a handful of near-constant head rows (spread 1e-4 of their mean: eps dominates the
    variance), dy (rows, 2d) x 1e-3, random affine."""
    d = H * Dh
    g = np.random.default_rng(7000 * Dh + 10 * rows + H + seed)
    qkv = g.standard_normal((rows, 3 * d)).astype(np.float32)
    flat = [(r, w, h) for r in (0, rows // 2, rows - 1) for w in (0, 1) for h in (0, H - 1)][:5]
    for i, (r, w, h) in enumerate(flat):
        mean = (-1.0) ** i * (1.0 + 0.25 * i)
        c0 = w * d + h * Dh
        qkv[r, c0:c0 + Dh] = (mean * (1.0 + 1e-4 * g.standard_normal(Dh))).astype(np.float32)
    dy = (g.standard_normal((rows, 2 * d)) * 1e-3).astype(np.float32)
    nw = (1.0 + 0.5 * g.standard_normal(Dh)).astype(np.float32)
    nb = (0.5 * g.standard_normal(Dh)).astype(np.float32)
    return qkv, dy, nw, nb


@functools.lru_cache(maxsize=None)
def qk_norm_case(Dh, rows, H):
    """(inputs, float64 forward, f32 forward, float64 backward, f32 backward): computed once, never written to."""
    qkv, dy, nw, nb = inp = qk_norm_inputs(Dh, rows, H)
    out = (inp, qk_norm_fwd_restated(qkv, nw, nb, H, np.float64), qk_norm_fwd_restated(qkv, nw, nb, H, np.float32),
           qk_norm_bwd_restated(qkv, dy, nw, H, np.float64), qk_norm_bwd_restated(qkv, dy, nw, H, np.float32))
    for a in inp + (out[1], out[2]) + out[3] + out[4]:
        a.setflags(write=False)
    return out


def accept_blocks(names, got, ref, f32, factor=KERNEL_FACTOR):
    """accept_f32 with named blocks (qk-norm: qkn; d_qk, d_norm_w, d_norm_b)."""
    seen = {nm: (rel_err(g, r64), rel_err(r32, r64)) for nm, g, r64, r32 in zip(names, got, ref, f32)}
    return seen, {nm: v for nm, v in seen.items() if not v[0] <= factor * v[1]}
