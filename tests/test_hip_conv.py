"""GPU (-m gpu): every conv-section entry point of include/genie_hip.h against the plain references of tests/conv_reference.py (f64 torch
convolutions / GroupNorm, bit-exact NumPy tokenizer ends; pinned on the CPU by tests/test_conv_reference_cpu.py), at the shapes where
implicit-GEMM kernels go wrong: asymmetric stride-2 padding, odd sides, image seams inside a 256-pixel tile, rows wider than a tile, more
tiles than compute units (the persistent loop), ragged output-channel tiles, ragged statistics blocks, off-centre GroupNorm inputs.

Every output is pre-filled with NaN (0xFF bytes for integers) so an unwritten element fails; the worst observed error of each kernel goes
to record_measure.  Bars: bf16-output convolutions |err| <= 2^-7 |ref| + 2e-3 (the stride-1 bar of tests/test_hip_harness.py); the f32
output of genie_conv_direct_bf16 (9 C_in + 1) 2^-24 (conv2d(|x|, |w|) + |b|); GroupNorm 2^-7 |ref| + 1e-3 plus what the statistics bound
of conv_reference.gn_stats_bound allows; tokenizer ends and batch invariance: the same bytes."""
import ast

import numpy as np
import pytest

import conv_reference as R
from conftest import GOLDEN, pkg, record_measure

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BF16 = torch.bfloat16


def L():
    _lib = pkg("_lib")
    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=BF16, device="cuda")


def bits_to_dev(bits):
    """uint16 bf16 bit patterns -> bf16 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(BF16)


def zero_page():
    return torch.zeros(64, dtype=BF16, device="cuda")


def make_conv(g, n, Hi, Wi, cin, cout, taps=9, bias=True):
    """Operands of a convolution: x bf16 NHWC, packed bf16 weights through genie_pack_conv_weight (so the packer is checked too), f32 bias."""
    _lib, lib = L()
    x = torch.randn(n, Hi, Wi, cin, device="cuda", generator=g).to(BF16)
    w = (torch.randn(cout, cin, taps, device="cuda", generator=g) / (taps * cin) ** 0.5).contiguous()
    b = torch.randn(cout, device="cuda", generator=g) if bias else None
    wp = nan16(cout, taps, cin)
    _lib.check(lib.genie_pack_conv_weight(w.data_ptr(), wp.data_ptr(), cout, cin, taps, stream()), "pack")
    assert torch.equal(wp, w.permute(0, 2, 1).to(BF16))       # tap-major, round to nearest even
    return x, wp, b


def conv3(x, wp, b, n, H, W, cin, cout, stride=1, d2s=False, res=None, gn_groups=0):
    """One 3x3 launch into a NaN-filled output.  gn_groups > 0: the variant with fused GroupNorm partials; returns (rc, y, part)."""
    _lib, lib = L()
    y = nan16(n, 2 * H, 2 * W, cout // 4) if d2s else nan16(n, H, W, cout)
    z = zero_page()
    if gn_groups:
        part = torch.full((lib.genie_conv_gn_part_floats(n, H, W, cout),), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.genie_conv3x3_gn_bf16(x.data_ptr(), wp.data_ptr(), ptr(b), ptr(res), y.data_ptr(), z.data_ptr(), n, H, W, cin, cout,
                                       int(d2s), stride, part.data_ptr(), gn_groups, stream())
        torch.cuda.synchronize()
        return rc, y, part
    if stride == 2:
        rc = lib.genie_conv3x3_s2_bf16(x.data_ptr(), wp.data_ptr(), ptr(b), y.data_ptr(), z.data_ptr(), n, H, W, cin, cout, stream())
    else:
        rc = lib.genie_conv3x3_bf16(x.data_ptr(), wp.data_ptr(), ptr(b), ptr(res), y.data_ptr(), z.data_ptr(), n, H, W, cin, cout,
                                    int(d2s), stream())
    torch.cuda.synchronize()
    return rc, y, None


def worst(err, ref, rel, ab):
    """max of err / (rel |ref| + ab): <= 1 means every element is inside the bar."""
    return (err / (rel * ref.abs() + ab)).max().item()


def check_conv3(key, x, wp, b, y, stride=1, d2s=False, res=None):
    """y against the f64 convolution, one image at a time (bounded memory); returns the worst err / bar."""
    assert torch.isfinite(y.float()).all(), "unwritten or non-finite output"
    wr, we = 0.0, 0.0
    for i in range(x.shape[0]):
        ref = R.conv3x3_ref(x[i:i + 1], wp, b, stride, d2s, None if res is None else res[i:i + 1])
        err = (y[i:i + 1].double() - ref).abs()
        wr, we = max(wr, worst(err, ref, 2.0 ** -7, 2e-3)), max(we, err.max().item())
        del ref, err
    record_measure(key + "_maxerr", we)
    record_measure(key + "_err_over_bar", wr)
    print(f"{key}: max |err| {we:.3e}, worst err / bar {wr:.3f}")
    return wr


# ---- a. stride 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,cin,cout,bias", [(3, 5, 7, 64, 72, True),       # odd output sides, n*H*W = 105: one ragged tile, ragged columns
                                                 (5, 8, 8, 128, 128, False),    # five images in two 256-pixel tiles
                                                 (1, 4, 300, 64, 136, True),    # output rows wider than a tile, 128 + 8 columns
                                                 (2, 16, 24, 192, 512, True),   # three channel chunks, four column tiles, non power-of-two
                                                 (1, 9, 33, 192, 72, False),
                                                 (2, 16, 16, 128, 128, True)])  # the geometry the fused-statistics variant also covers
def test_conv3x3_s2_against_f64(n, H, W, cin, cout, bias):
    """genie_conv3x3_s2_bf16 (H, W: OUTPUT size; input (2H, 2W), padding 1: only the top row and left column of taps leave the image)
    against conv2d(stride 2, padding 1) in f64 on the same bf16 operands; the border rows and columns asserted on their own; and, as a
    different statement, genie_conv3x3_gn_bf16(stride 2) gives the same bytes where it is supported and writes nothing where it is not."""
    _lib, lib = L()
    x, wp, b = make_conv(gen(7 * n + H + cout), n, 2 * H, 2 * W, cin, cout, bias=bias)
    rc, y, _ = conv3(x, wp, b, n, H, W, cin, cout, stride=2)
    _lib.check(rc, "conv3x3_s2")
    assert torch.isfinite(y.float()).all()
    ref = R.conv3x3_ref(x, wp, b, stride=2)
    err = (y.double() - ref).abs()
    bar = 2.0 ** -7 * ref.abs() + 2e-3
    key = f"conv3x3_s2_n{n}_{H}x{W}_{cin}_{cout}"
    record_measure(key + "_maxerr", err.max().item())
    record_measure(key + "_err_over_bar", (err / bar).max().item())
    print(f"{key}: max |err| {err.max().item():.3e}, worst err / bar {(err / bar).max().item():.3f}")
    for name, e, br in (("top row", err[:, 0], bar[:, 0]), ("bottom row", err[:, -1], bar[:, -1]),
                        ("left column", err[:, :, 0], bar[:, :, 0]), ("right column", err[:, :, -1], bar[:, :, -1])):
        assert (e <= br).all(), (name, e.max().item())
    assert (err <= bar).all(), err.max().item()
    rc, yg, part = conv3(x, wp, b, n, H, W, cin, cout, stride=2, gn_groups=32)
    if (H * W) % 256 == 0 and cout % 128 == 0:
        _lib.check(rc, "conv3x3_gn")
        assert torch.equal(yg.view(torch.int16), y.view(torch.int16))
    else:
        assert rc == _lib.E_UNSUPPORTED
        assert torch.isnan(yg.float()).all() and torch.isnan(part).all()


# ---- b. stride 1: persistent loop, ragged columns, depth-to-space with residual -----------------------------------------------------
@pytest.mark.parametrize("n,H,W,cin,cout,d2s,res,bias", [
    (3, 96, 96, 64, 384, False, False, True),    # 108 x 3 = 324 tiles: more than the compute units, not a multiple of them
    (2, 192, 192, 64, 8, False, False, True),    # 32-column form, 288 row tiles
    (2, 12, 20, 64, 24, False, True, True),      # 32-column form, ragged columns
    (2, 12, 20, 64, 40, False, True, True),      # 128-column form, 40 of 128 columns
    (3, 24, 40, 128, 136, False, True, False),   # 128 + 8 columns, ragged last row tile, image seams inside tiles
    (5, 8, 8, 64, 24, False, False, False),      # several images per tile on the 32-column form
    (1, 20, 12, 64, 256, True, True, True),      # depth-to-space with a residual of the OUTPUT's (n, 2H, 2W, C/4) shape
    (2, 16, 16, 64, 160, True, True, False)])    # depth-to-space, ragged columns (160 = 128 + 32), two images per tile
def test_conv3x3_persistent_and_ragged_against_f64(n, H, W, cin, cout, d2s, res, bias):
    """genie_conv3x3_bf16 against conv2d in f64: workgroups that walk more than one tile, C_out that does not fill the last column tile on
    both forms, and the residual under depth-to-space (added at the permuted output position, as the header says)."""
    _lib, lib = L()
    g = gen(n * 100 + cout + W)
    x, wp, b = make_conv(g, n, H, W, cin, cout, bias=bias)
    oshape = (n, 2 * H, 2 * W, cout // 4) if d2s else (n, H, W, cout)
    r = torch.randn(oshape, device="cuda", generator=g).to(BF16) if res else None
    rc, y, _ = conv3(x, wp, b, n, H, W, cin, cout, d2s=d2s, res=r)
    _lib.check(rc, "conv3x3")
    wr = check_conv3(f"conv3x3_n{n}_{H}x{W}_{cin}_{cout}_d2s{int(d2s)}", x, wp, b, y, 1, d2s, r)
    assert wr <= 1.0, wr


# ---- c. 1x1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix,cin,cout,bias", [(300, 512, 20, True),   # the encoder's conv_out: 18 code bits padded to 20
                                                 (1, 512, 20, True), (255, 128, 256, False), (257, 256, 512, False),
                                                 (257, 512, 20, False), (255, 256, 512, True), (1, 128, 256, False), (1024, 128, 256, True)])
def test_conv1x1_against_f64(n_pix, cin, cout, bias):
    """genie_conv1x1_bf16 (the bf16-output GEMM: ResBlock shortcuts 128 -> 256, 256 -> 512, the encoder's 512 -> 20) against an f64 matmul."""
    _lib, lib = L()
    x, wp, b = make_conv(gen(n_pix + cout), 1, 1, n_pix, cin, cout, taps=1, bias=bias)
    x, wp = x.view(n_pix, cin), wp.view(cout, cin)
    y = nan16(n_pix, cout)
    _lib.check(lib.genie_conv1x1_bf16(x.data_ptr(), wp.data_ptr(), ptr(b), y.data_ptr(), n_pix, cin, cout, stream()), "conv1x1")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    ref = R.conv1x1_ref(x, wp, b)
    err = (y.double() - ref).abs()
    key = f"conv1x1_{n_pix}_{cin}_{cout}"
    record_measure(key + "_maxerr", err.max().item())
    record_measure(key + "_err_over_bar", worst(err, ref, 2.0 ** -7, 2e-3))
    print(f"{key}: max |err| {err.max().item():.3e}, worst err / bar {worst(err, ref, 2.0 ** -7, 2e-3):.3f}")
    assert (err <= 2.0 ** -7 * ref.abs() + 2e-3).all(), err.max().item()


# ---- d. direct ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_mode", [0, 1])
@pytest.mark.parametrize("n,H,W,cin,cout,bias", [(3, 5, 7, 18, 512, True), (3, 6, 10, 128, 3, True), (1, 9, 4, 18, 512, False)])
def test_conv_direct_against_f64(n, H, W, cin, cout, bias, out_mode):
    """genie_conv_direct_bf16 (the two edge layers it was written for, 18 -> 512 and 128 -> 3) against conv2d in f64.  out_mode 0: NHWC bf16,
    the bf16 bar.  out_mode 1: NCHW f32, no rounding of the result: a chain of 9 C_in fused multiply-adds behind the bias, so
    |err| <= (9 C_in + 1) 2^-24 (conv2d(|x|, |w|) + |b|)."""
    _lib, lib = L()
    x, wp, b = make_conv(gen(n + cin + cout), n, H, W, cin, cout, bias=bias)
    y = nan16(n, H, W, cout) if out_mode == 0 else torch.full((n, cout, H, W), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.genie_conv_direct_bf16(x.data_ptr(), wp.data_ptr(), ptr(b), y.data_ptr(), n, H, W, cin, cout, out_mode, stream()), "direct")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    ref = R.conv3x3_ref(x, wp, b)
    key = f"conv_direct_mode{out_mode}_{cin}_{cout}_n{n}"
    if out_mode == 0:
        err = (y.double() - ref).abs()
        bar = 2.0 ** -7 * ref.abs() + 2e-3
    else:
        err = (y.double().permute(0, 2, 3, 1) - ref).abs()
        bar = (9 * cin + 1) * 2.0 ** -24 * R.conv3x3_mag(x, wp, b)
    record_measure(key + "_maxerr", err.max().item())
    record_measure(key + "_err_over_bar", (err / bar).max().item())
    print(f"{key}: max |err| {err.max().item():.3e}, worst err / bar {(err / bar).max().item():.3f}")
    assert (err <= bar).all(), (err.max().item(), (err / bar).max().item())


# ---- e. GroupNorm ---------------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(2, 50, 128, 32), (2, 200, 256, 32), (2, 1000, 64, 16), (2, 20000, 128, 32), (2, 64, 2048, 32), (3, 37, 8, 2),
             (1, 65536, 128, 32)]


def gn_input(g, n, HW, C, groups, ratio):
    scale = 0.5 + 1.5 * torch.rand(n, 1, groups, 1, device="cuda", generator=g)
    x = (torch.randn(n, HW, groups, C // groups, device="cuda", generator=g) + ratio) * scale
    return x.view(n, HW, C).to(BF16)


def group_norm(x, gamma, beta, groups, swish, eps=1e-6):
    """One genie_group_norm_swish_bf16 call into NaN-filled output and scratch; returns (rc, y, scratch)."""
    _lib, lib = L()
    n, HW, C = x.shape
    y = nan16(n, HW, C)
    nws = max(int(lib.genie_group_norm_scratch_floats(n, HW, groups)), 2 * n * groups)
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.genie_group_norm_swish_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), ws.data_ptr(), n, HW, C, groups,
                                         eps, int(swish), stream())
    torch.cuda.synchronize()
    return rc, y, ws


@pytest.mark.parametrize("ratio", [0, 4, 16])
@pytest.mark.parametrize("n,HW,C,groups", GN_SHAPES)
def test_group_norm_swish_against_f64(n, HW, C, groups, ratio):
    """genie_group_norm_swish_bf16, apply_swish 0 and 1, against group_norm in f64: ragged and tiny statistics blocks, one pixel per pass
    (C = 2048), C = 8, groups != 32, and inputs whose group mean is `ratio` standard deviations from zero.  The kernel keeps f32 sums of x
    and x^2 and forms q/cnt - mean^2 at the end, so its statistics are held to the bound its summation chain implies
    (conv_reference.gn_stats_bound):  rel(rstd) <= 2 n_acc 2^-24 (1 + (mean/std)^2),  |d mean| <= 2 n_acc 2^-24 sqrt(mean^2 + var),
    and the output to 2^-7 |ref| + 1e-3 plus the change those two allow."""
    _lib, lib = L()
    g = gen(HW + C + ratio)
    x = gn_input(g, n, HW, C, groups, ratio)
    gamma = (1 + 0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()
    beta = (0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()
    cpg = C // groups
    for swish in (0, 1):
        rc, y, ws = group_norm(x, gamma, beta, groups, swish)
        _lib.check(rc, "group_norm")
        assert torch.isfinite(y.float()).all()
        ref, mean, rstd, var = R.group_norm_ref(x, groups, gamma, beta, 1e-6, bool(swish))
        dm, rr = R.gn_stats_bound(HW, C, groups, mean, var)
        st = ws[:2 * n * groups].view(n, groups, 2).double()
        assert torch.isfinite(st).all()
        em, er = (st[..., 0] - mean).abs(), (st[..., 1] / rstd - 1).abs()
        key = f"group_norm_hw{HW}_c{C}_g{groups}_r{ratio}_swish{swish}"
        record_measure(key + "_mean_err_over_bound", (em / dm).max().item())
        record_measure(key + "_rstd_relerr", er.max().item())
        record_measure(key + "_rstd_err_over_bound", (er / rr).max().item())
        assert (em <= dm).all(), ((em / dm).max().item(), R.gn_chain_length(HW, C, groups))
        assert (er <= rr).all(), ((er / rr).max().item(), R.gn_chain_length(HW, C, groups))
        # d y <= |gamma| rstd (|x - mean| rel(rstd) + |d mean|), through a swish of slope <= 1.1
        per_c = lambda t: t.repeat_interleave(cpg, dim=1)[:, None, :]   # (n, groups) -> (n, 1, C)
        slack = 1.1 * gamma.double().abs() * per_c(rstd) * ((x.double() - per_c(mean)).abs() * per_c(rr) + per_c(dm))
        err = (y.double() - ref).abs()
        bar = 2.0 ** -7 * ref.abs() + 1e-3 + slack
        record_measure(key + "_maxerr", err.max().item())
        record_measure(key + "_err_over_bar", (err / bar).max().item())
        print(f"{key}: rstd rel err {er.max().item():.3e} ({(er / rr).max().item():.3f} of the bound), out err / bar {(err / bar).max().item():.3f}")
        assert (err <= bar).all(), (err.max().item(), (err / bar).max().item())
        rc, y2, ws2 = group_norm(x, gamma, beta, groups, swish)      # order-fixed reduction: the same bytes again
        _lib.check(rc, "group_norm")
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16))
        assert torch.equal(ws2[:2 * n * groups], ws[:2 * n * groups])


@pytest.mark.parametrize("C,groups", [(192, 16), (256, 128)])
def test_group_norm_unsupported_geometry_is_an_error(C, groups):
    """C/8 that does not divide the 256-thread block, more than 64 groups: GENIE_E_SHAPE, and neither the output nor the scratch is touched."""
    _lib, lib = L()
    x = gn_input(gen(C), 2, 64, C, groups, 0)
    rc, y, ws = group_norm(x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), groups, 1)
    assert rc == _lib.E_SHAPE
    assert torch.isnan(y.float()).all() and torch.isnan(ws).all()


# ---- f. NHWC tokenizer ends: the same bits as the NumPy references --------------------------------------------------------------------
@pytest.mark.parametrize("cpad", [3, 4, 64])
def test_frames_to_nhwc_bit_exact(cpad):
    _lib, lib = L()
    n, cin, HW = 2, 3, 200
    f = (np.arange(n * cin * HW, dtype=np.int64) * 37 % 256).astype(np.uint8).reshape(n, cin, HW)
    assert all(len(np.unique(f[:, c])) == 256 for c in range(cin))          # every byte value in every channel
    fd = torch.from_numpy(f).cuda()
    x = torch.full((n, HW, cpad), -1, dtype=torch.int16, device="cuda")     # 0xFFFF
    _lib.check(lib.genie_frames_to_nhwc_bf16(fd.data_ptr(), x.data_ptr(), n, HW, cin, cpad, stream()), "frames_to_nhwc")
    got = x.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, R.frames_to_nhwc(f, cpad))
    assert not got[:, :, cin:].any()                                        # padding channels exactly zero


@pytest.mark.parametrize("cpad", [18, 20, 64])
def test_tokens_from_code_nhwc_bit_exact(cpad):
    _lib, lib = L()
    bits, n_pix = 18, 1000
    rng = np.random.default_rng(cpad)
    h = R.bf16_bits(rng.standard_normal((n_pix, cpad)).astype(np.float32))
    special = np.array([0x0000, 0x8000, 0x0001, 0x7FC0, 0x8001, 0xFFC0, 0x7F80, 0xFF80, 0x007F, 0x0080], np.uint16)
    h[rng.integers(0, n_pix, 4000), rng.integers(0, cpad, 4000)] = special[rng.integers(0, len(special), 4000)]
    h[:len(special), 0] = special                                           # each special value at least once in bit 0 ...
    h[:len(special), 1:bits] = 0xBF80                                       # ... alone in its id
    h[:, bits:] = 0x3F80                                                    # +1.0 in the padding channels: ignored
    hd = bits_to_dev(h)
    ids = torch.full((n_pix,), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.genie_tokens_from_code_nhwc_bf16(hd.data_ptr(), ids.data_ptr(), n_pix, bits, cpad, stream()), "tokens_from_code")
    got = ids.cpu().numpy()
    # +0, -0, NaN, negative values: bit 0; the smallest positive subnormal: bit 1
    assert got[:len(special)].tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 1, 1]
    assert np.array_equal(got, R.tokens_from_code_nhwc(h, bits))


@pytest.mark.parametrize("cpad", [18, 20, 64])
def test_bits_from_tokens_nhwc_bit_exact(cpad):
    _lib, lib = L()
    bits, n_pix = 18, 1000
    rng = np.random.default_rng(cpad)
    ids = rng.integers(0, 1 << bits, n_pix, dtype=np.int64)
    ids[::3] |= np.int64(1) << bits                                          # bits above `bits` set
    ids[1::5] |= (np.int64(1) << 40) | (np.int64(1) << 19)
    ids[7], ids[8], ids[9] = -1, 0, (1 << bits) - 1
    z = torch.full((n_pix, cpad), -1, dtype=torch.int16, device="cuda")
    idd = torch.from_numpy(ids).cuda()
    _lib.check(lib.genie_bits_from_tokens_nhwc_bf16(idd.data_ptr(), z.data_ptr(), n_pix, bits, cpad, stream()), "bits_nhwc")
    got = z.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, R.bits_from_tokens_nhwc(ids, bits, cpad))
    assert not got[:, bits:].any()                                          # padding channels exactly zero
    # and the round trip through the other end
    out = torch.full((n_pix,), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.genie_tokens_from_code_nhwc_bf16(z.data_ptr(), out.data_ptr(), n_pix, bits, cpad, stream()), "tokens_from_code")
    assert np.array_equal(out.cpu().numpy(), ids & ((1 << bits) - 1))


@pytest.mark.parametrize("cpad,cout", [(4, 3), (8, 3), (3, 3), (64, 1)])
def test_rescale_u8_nhwc_bit_exact(cpad, cout):
    """Every non-NaN bf16 bit pattern (both clamp edges, infinities and every tie of the two bf16 roundings among them) in every used
    channel."""
    _lib, lib = L()
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    allb = allb[~np.isnan(R.bf16_value(allb))]
    n, HW = 3, 21900
    assert n * HW >= len(allb) + cpad
    x = np.resize(allb, n * HW + cpad)
    x = np.stack([x[c:c + n * HW] for c in range(cpad)], axis=1).reshape(n, HW, cpad)   # channel c sees the sequence shifted by c
    xd = bits_to_dev(x)
    out = torch.full((n, cout, HW), 0xFF, dtype=torch.uint8, device="cuda")
    want = R.rescale_u8_nhwc(x, cout)
    assert (want != 0xFF).any() and len(np.unique(want)) == 256
    _lib.check(lib.genie_rescale_u8_nhwc_bf16(xd.data_ptr(), out.data_ptr(), n, HW, cpad, cout, stream()), "rescale_nhwc")
    assert np.array_equal(out.cpu().numpy(), want)


# ---- g. batch invariance: an image's bytes do not depend on what else is in the batch -------------------------------------------------
GEOM = [(8, 8), (15, 20), (16, 16)]   # H*W = 64 and 300: 256-pixel tiles straddle images; 256: they do not


def assert_batch_invariant(run, n, what):
    """run(slice of the batch) -> tuple of outputs with the batch as first axis: image j alone == image j of the batch, j = 0, 1, last."""
    full = run(slice(0, n))
    for j in (0, 1, n - 1):
        alone = run(slice(j, j + 1))
        for a, f in zip(alone, full):
            assert a.dtype == f.dtype and a.shape[1:] == f.shape[1:]
            av, fv = (a, f[j:j + 1]) if a.dtype != BF16 else (a.view(torch.int16), f[j:j + 1].contiguous().view(torch.int16))
            if a.dtype == torch.float32:
                av, fv = a.view(torch.int32), f[j:j + 1].contiguous().view(torch.int32)
            assert torch.equal(av, fv), (what, j)


@pytest.mark.parametrize("H,W", GEOM)
@pytest.mark.parametrize("kind", ["s1_128", "s1_32", "s1_d2s", "s2", "gn_s1", "gn_s2", "gn_d2s"])
def test_conv3x3_batch_invariance(kind, H, W):
    """Stride-1 convolution on both forms (with residual), depth-to-space, stride 2, and the fused-statistics variants (with the
    GroupNorm + swish they feed) where the geometry supports them (elsewhere they must refuse and write nothing)."""
    _lib, lib = L()
    n, cin = 4, 64
    stride = 2 if kind.endswith("s2") else 1
    d2s = kind.endswith("d2s")
    cout = {"s1_128": 136, "s1_32": 24, "s1_d2s": 160, "s2": 136, "gn_s1": 128, "gn_s2": 128, "gn_d2s": 512}[kind]
    g = gen(H * W + cout)
    x, wp, b = make_conv(g, n, H * stride, W * stride, cin, cout)
    oshape = (n, 2 * H, 2 * W, cout // 4) if d2s else (n, H, W, cout)
    res = torch.randn(oshape, device="cuda", generator=g).to(BF16) if stride == 1 else None
    if not kind.startswith("gn"):
        def run(sl):
            xb = x[sl].contiguous()
            r = None if res is None else res[sl].contiguous()
            rc, y, _ = conv3(xb, wp, b, xb.shape[0], H, W, cin, cout, stride=stride, d2s=d2s, res=r)
            _lib.check(rc, kind)
            assert torch.isfinite(y.float()).all()
            return (y,)
        assert_batch_invariant(run, n, kind)
        return
    C = cout // 4 if d2s else cout
    gamma = (1 + 0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()
    beta = (0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()
    if (H * W) % 256:
        rc, y, part = conv3(x, wp, b, n, H, W, cin, cout, stride=stride, d2s=d2s, res=res, gn_groups=32)
        assert rc == _lib.E_UNSUPPORTED and torch.isnan(y.float()).all() and torch.isnan(part).all()
        return

    def run_gn(sl):
        xb = x[sl].contiguous()
        nb = xb.shape[0]
        r = None if res is None else res[sl].contiguous()
        rc, y, part = conv3(xb, wp, b, nb, H, W, cin, cout, stride=stride, d2s=d2s, res=r, gn_groups=32)
        _lib.check(rc, kind)
        z = nan16(*y.shape)
        ws = torch.full((nb * 64,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.genie_group_norm_swish_fused_bf16(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), z.data_ptr(), part.data_ptr(),
                                                         ws.data_ptr(), nb, H, W, cout, int(d2s), 32, 1e-6, 1, stream()), "gn_fused")
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all() and torch.isfinite(z.float()).all()
        return y, z, ws.view(nb, 64)
    assert_batch_invariant(run_gn, n, kind)


@pytest.mark.parametrize("H,W", GEOM)
def test_conv1x1_direct_groupnorm_batch_invariance(H, W):
    _lib, lib = L()
    n = 4
    g = gen(H * W)
    # 1x1: an "image" is H*W rows of the GEMM
    x, wp, b = make_conv(g, n, H, W, 128, 256, taps=1)

    def run1(sl):
        xb = x[sl].contiguous()
        npx = xb.shape[0] * H * W
        y = nan16(xb.shape[0], H, W, 256)
        _lib.check(lib.genie_conv1x1_bf16(xb.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), npx, 128, 256, stream()), "conv1x1")
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all()
        return (y,)
    assert_batch_invariant(run1, n, "conv1x1")
    xe, wpe, be = make_conv(g, n, H, W, 512, 20, taps=1)

    def run1e(sl):
        xb = xe[sl].contiguous()
        y = nan16(xb.shape[0], H, W, 20)
        _lib.check(lib.genie_conv1x1_bf16(xb.data_ptr(), wpe.data_ptr(), be.data_ptr(), y.data_ptr(), xb.shape[0] * H * W, 512, 20, stream()),
                   "conv1x1")
        torch.cuda.synchronize()
        return (y,)
    assert_batch_invariant(run1e, n, "conv1x1 512->20")
    # direct, both output layouts
    xd, wpd, bd = make_conv(g, n, H, W, 18, 32)
    for mode in (0, 1):
        def rund(sl):
            xb = xd[sl].contiguous()
            nb = xb.shape[0]
            y = nan16(nb, H, W, 32) if mode == 0 else torch.full((nb, 32, H, W), float("nan"), dtype=torch.float32, device="cuda")
            _lib.check(lib.genie_conv_direct_bf16(xb.data_ptr(), wpd.data_ptr(), bd.data_ptr(), y.data_ptr(), nb, H, W, 18, 32, mode, stream()),
                       "direct")
            torch.cuda.synchronize()
            assert torch.isfinite(y.float()).all()
            return (y,)
        assert_batch_invariant(rund, n, f"direct mode {mode}")
    # separate GroupNorm, output and statistics
    C = 128
    xg = gn_input(g, n, H * W, C, 32, 4)
    gamma = (1 + 0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()
    beta = (0.1 * torch.randn(C, device="cuda", generator=g)).contiguous()

    def rung(sl):
        xb = xg[sl].contiguous()
        rc, y, ws = group_norm(xb, gamma, beta, 32, 1)
        _lib.check(rc, "group_norm")
        return y, ws[:xb.shape[0] * 64].view(xb.shape[0], 64)
    assert_batch_invariant(rung, n, "group_norm")


def test_encoder_batch_invariance():
    """HipEncoder.encode_tokens on the golden frames: a batch of 3 == one frame at a time (tiles of the deeper levels straddle images)."""
    mv = pkg("magvit2")
    z = np.load(f"{GOLDEN}/magvit_mid.npz")
    m = mv.VQModel(mv.VQConfig(**ast.literal_eval(str(z["cfg"]))))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in mv.make_vq_state_dict(m, int(z["weight_seed"])).items()})
    he = mv.HipEncoder(m.to("cuda").encoder)
    frames = torch.from_numpy(z["enc_frames"]).cuda()
    full = he.encode_tokens(frames)
    assert full.shape[0] == 3
    for j in range(3):
        assert torch.equal(he.encode_tokens(frames[j:j + 1]), full[j:j + 1]), j
    rev = he.encode_tokens(frames.flip(0))
    assert torch.equal(rev.flip(0), full)
