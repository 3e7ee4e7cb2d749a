"""Plain references of the MAGVIT2 conv-stack operations of include/genie_hip.h ("MAGVIT2 decoder convolutions" section), with no
kernel code behind them.  Test infrastructure for tests/test_conv_reference_cpu.py (which pins them on the CPU) and
tests/test_hip_conv.py (which compares every conv-section entry point with them).

  torch, f64, on whatever device the operands live:  conv3x3 / conv1x1 / their magnitude companions / GroupNorm [+ swish]
  NumPy, bit-exact:                                   the four NHWC tokenizer ends, on uint16 bf16 bit patterns
  NumPy, f32 partials:                                the GroupNorm statistics in the separate statistics pass's summation order,
                                                      and the error bound that order implies (gn_stats_bound)

Layouts are the library's: activations NHWC bf16, packed weights (C_out, taps, C_in) bf16, bias / gamma / beta f32.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit roundoff of f32


# ---- bf16 bit patterns in NumPy -----------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 -> bf16 bit pattern (uint16), round to nearest even (+-inf pass through; no NaN)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit pattern (uint16) -> float32."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def pack_conv_weight(w):
    """(C_out, C_in, kh, kw) f32 torch layout -> (C_out, kh*kw, C_in) bf16 bit patterns (tap-major K): genie_pack_conv_weight."""
    w = np.asarray(w, np.float32)
    co, ci = w.shape[:2]
    return bf16_bits(w.reshape(co, ci, -1).transpose(0, 2, 1))


# ---- convolutions (torch, f64) ------------------------------------------------------------------------------------------------
def _weights_nchw(w_packed):
    """(C_out, 9, C_in) bf16 packed -> (C_out, C_in, 3, 3) f64: the weights the kernel actually multiplies."""
    co, taps, ci = w_packed.shape
    assert taps == 9
    return w_packed.view(co, 3, 3, ci).permute(0, 3, 1, 2).double()


def depth_to_space_dcr(y_nchw):
    """DCR: conv channel (i*2 + j)*C + c -> pixel (2y+i, 2x+j), channel c."""
    n, c4, h, w = y_nchw.shape
    c = c4 // 4
    return y_nchw.view(n, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 2 * h, 2 * w)


def _conv3x3(x, w, b, stride, d2s):
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=stride, padding=1)
    if d2s:
        y = depth_to_space_dcr(y)
    return y.permute(0, 2, 3, 1)


def conv3x3_ref(x, w_packed, bias=None, stride=1, d2s=False, residual=None):
    """x (n, H_in, W_in, C_in) bf16, w_packed (C_out, 9, C_in) bf16, bias f32 or None, residual (output shape) bf16 or None
    -> f64 NHWC: conv2d(3x3, padding 1, stride) on the bf16-rounded operands [-> DCR depth-to-space] [+ residual]."""
    y = _conv3x3(x.double(), _weights_nchw(w_packed), None if bias is None else bias.double(), stride, d2s)
    return y if residual is None else y + residual.double()


def conv3x3_mag(x, w_packed, bias=None, stride=1, d2s=False, residual=None):
    """conv2d(|x|, |w|) + |b| [+ |residual|]: the sum of the magnitudes of every term of conv3x3_ref, for error bounds."""
    y = _conv3x3(x.double().abs(), _weights_nchw(w_packed).abs(), None if bias is None else bias.double().abs(), stride, d2s)
    return y if residual is None else y + residual.double().abs()


def conv1x1_ref(x, w_packed, bias=None):
    """x (n_pix, C_in) bf16, w_packed (C_out, C_in) bf16 -> (n_pix, C_out) f64."""
    y = x.double() @ w_packed.double().t()
    return y if bias is None else y + bias.double()


def conv1x1_mag(x, w_packed, bias=None):
    y = x.double().abs() @ w_packed.double().abs().t()
    return y if bias is None else y + bias.double().abs()


# ---- GroupNorm (torch, f64) ---------------------------------------------------------------------------------------------------
def group_norm_ref(x, groups, gamma, beta, eps, swish):
    """x (n, HW, C) bf16 -> (y (n, HW, C) f64, mean (n, groups) f64, rstd (n, groups) f64, var (n, groups) f64):
    group_norm in f64 (biased variance), optionally followed by y * sigmoid(y)."""
    n, hw, c = x.shape
    xd = x.double()
    y = F.group_norm(xd.permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    if swish:
        y = y * torch.sigmoid(y)
    xg = xd.view(n, hw, groups, c // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    return y, mean, 1.0 / torch.sqrt(var + eps), var


def gn_block_pixels(HW):
    """Pixels per statistics block of genie_group_norm_swish_bf16 (the ragged last block has fewer)."""
    return 512 if HW >= 16384 else (128 if HW >= 1024 else (64 if HW >= 64 else HW))


def gn_chain_length(HW, C, groups):
    """n_acc: the longest chain of f32 additions any input element passes through in the separate statistics pass.
    A block is 256 threads over gn_block_pixels(HW) pixels; thread t owns the 8-channel chunk t % (C/8) and every (256 / (C/8))-th pixel,
    and adds per pixel and 4-channel half  s += a + b  twice (the same for a*a + b*b; the squares of bf16 values are exact in f32):
        1                               the pair a + b
      + 2 * ceil(ppb / (256 / (C/8)))   the thread's running sum
      + 512 / groups                    the reducer thread's sum over the (256 / (C/8)) * (C/groups) / 4 halves of its group.
    The blocks of an image are then added in f64."""
    ppb = gn_block_pixels(HW)
    pstep = 256 // (C // 8)
    return 1 + 2 * -(-ppb // pstep) + 512 // groups


def gn_stats_bound(HW, C, groups, mean, var):
    """(|d mean| bound, rel(rstd) bound) of f32 partial sums n_acc long against the exact statistics `mean`, `var` (f64 tensors).

    Recursive f32 summation of n terms errs by at most g = n*U*(sum of |terms|) (first order).  With m2 = mean^2 + var = E[x^2]:
        |d sum_x|  / cnt <= g * E|x|   <= g * sqrt(m2)
        |d sum_xx| / cnt <= g * m2
        var' = q/cnt - mean'^2  (f64):   |d var| <= g*m2 + 2*|mean|*g*sqrt(m2) <= 3*g*m2
        rstd = (var + eps)^-1/2:         rel(rstd) <= |d var| / (2*var) <= 1.5 * n_acc * U * (1 + (mean/std)^2)
    The final casts of mean and rstd to f32 add U each, and the first-order forms drop terms of relative size g*(1 + (mean/std)^2)
    (< 1 % for every case tested), so the bounds are stated with c = 2:
        rel(rstd) <= 2 * n_acc * 2^-24 * (1 + (mean/std)^2),        |d mean| <= 2 * n_acc * 2^-24 * sqrt(mean^2 + var)."""
    n_acc = gn_chain_length(HW, C, groups)
    m2 = mean * mean + var
    return 2 * n_acc * U * torch.sqrt(m2), 2 * n_acc * U * (m2 / var)


def gn_stats_f32_ordered(x_bits, groups, eps):
    """The statistics of x (n, HW, C) bf16 bit patterns with f32 partial sums added in the order of the separate statistics pass
    (see gn_chain_length), blocks added in f64.  Returns (mean, rstd) as float32 arrays (n, groups).  NumPy on the host: this is what
    confirms, without a GPU, that f32 partials in this order stay inside gn_stats_bound."""
    n, HW, C = x_bits.shape
    c8, cpg = C // 8, C // groups
    ppb = gn_block_pixels(HW)
    pstep = 256 // c8
    npt = -(-ppb // pstep)
    nblk = -(-HW // ppb)
    x = np.zeros((n, nblk * npt * pstep, C), np.float32)      # zero pixels behind the ragged end: adding 0.0f is exact
    xv = bf16_value(x_bits)
    for b in range(nblk):                                      # block b holds pixels b*ppb .. b*ppb + ppb - 1 (ppb <= npt * pstep)
        seg = xv[:, b * ppb:min((b + 1) * ppb, HW)]
        x[:, b * npt * pstep:b * npt * pstep + seg.shape[1]] = seg
    x = x.reshape(n, nblk, npt, pstep, c8, 2, 2, 2)            # [.., pixel step, pixel row, chunk, half, k, (a, b)]
    s = np.zeros((n, nblk, pstep, c8, 2), np.float32)
    q = np.zeros_like(s)
    for i in range(npt):
        for k in range(2):
            a, b = x[:, :, i, :, :, :, k, 0], x[:, :, i, :, :, :, k, 1]
            s = s + (a + b)
            q = q + (a * a + b * b)
    # reducer: thread t = prow * c8 + chunk, visited in t order; per thread first half then second half
    S = np.zeros((n, nblk, groups), np.float32)
    Q = np.zeros_like(S)
    for prow in range(pstep):
        for ch in range(c8):
            for half in range(2):
                g = (ch * 8 + 4 * half) // cpg
                S[:, :, g] = S[:, :, g] + s[:, :, prow, ch, half]
                Q[:, :, g] = Q[:, :, g] + q[:, :, prow, ch, half]
    cnt = float(np.float32(HW) * np.float32(cpg))
    mean = S.astype(np.float64).sum(1) / cnt
    var = np.maximum(Q.astype(np.float64).sum(1) / cnt - mean * mean, 0.0)
    return mean.astype(np.float32), (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32)


# ---- NHWC tokenizer ends (NumPy, bit-exact) -----------------------------------------------------------------------------------
def frames_to_nhwc(frames, cpad):
    """uint8 (n, c, HW) -> bf16 bit patterns (n, HW, cpad): bf16_rne(float32(b) / 127.5f - 1.0f), channels >= c zero."""
    f = np.asarray(frames, np.uint8)
    n, c, hw = f.shape
    v = f.astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    out = np.zeros((n, hw, cpad), np.uint16)
    out[:, :, :c] = bf16_bits(v).transpose(0, 2, 1)
    return out


def tokens_from_code_nhwc(h_bits, bits):
    """bf16 bit patterns (n_pix, cpad) -> int64 ids (n_pix,): bit c = [h_c > 0] for c < bits (a NaN, either zero: 0; a positive
    subnormal: 1); channels >= bits are ignored."""
    h = bf16_value(np.asarray(h_bits, np.uint16)[:, :bits])
    with np.errstate(invalid="ignore"):
        b = (h > 0).astype(np.int64)
    return (b << np.arange(bits, dtype=np.int64)[None, :]).sum(1)


def bits_from_tokens_nhwc(ids, bits, cpad):
    """int64 ids (n_pix,) -> bf16 bit patterns (n_pix, cpad): channel c < bits = +1.0 if bit c of the id is set else -1.0; channels >= bits
    zero, whatever higher bits the id has."""
    ids = np.asarray(ids, np.int64)
    b = (ids[:, None] >> np.arange(bits, dtype=np.int64)[None, :]) & 1
    out = np.zeros((ids.shape[0], cpad), np.uint16)
    out[:, :bits] = np.where(b == 1, np.uint16(0x3F80), np.uint16(0xBF80))
    return out


def rescale_u8_nhwc(x_bits, cout):
    """bf16 bit patterns (n, HW, cpad) -> uint8 (n, cout, HW): trunc(clamp(bf16(bf16(x + 1) * 127.5), 0, 255)) of the first cout channels.
    Finite or infinite inputs (a NaN has no defined byte)."""
    x = bf16_value(np.asarray(x_bits, np.uint16)[:, :, :cout])
    with np.errstate(over="ignore"):
        v = bf16_value(bf16_bits(x + np.float32(1.0)))
        v = bf16_value(bf16_bits(v * np.float32(127.5)))
    return np.clip(v, 0, 255).astype(np.uint8).transpose(0, 2, 1)

