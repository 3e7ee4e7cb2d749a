"""CPU: pins tests/conv_reference.py (the references tests/test_hip_conv.py holds the conv-stack kernels to) so that it cannot drift with the
kernels: the NHWC tokenizer ends against the oracle functions already pinned to the reference's goldens, the stride-2 convolution against
oracle/magvit2_oracle.py's downsample, and the GroupNorm statistics bound against f32 partials added in the kernel's order."""
import ast

import numpy as np
import pytest

import conv_reference as R
from conftest import GOLDEN, pkg
from oracle import genie_oracle as O

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def magvit():
    return np.load(f"{GOLDEN}/magvit_small.npz")


def test_bf16_bits_round_trip_and_rounding():
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = R.bf16_value(allb)
    fin = np.isfinite(v)
    assert np.array_equal(R.bf16_bits(v[fin]), allb[fin])                      # every finite bf16 is a fixed point
    a = np.random.default_rng(0).standard_normal(100000).astype(np.float32) * np.float32(3.0)
    assert np.array_equal(R.bf16_value(R.bf16_bits(a)), O.round_bf16(a))
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x3F807FFF, 0x3F808001], np.uint32).view(np.float32)
    assert R.bf16_bits(ties).tolist() == [0x3F80, 0x3F82, 0xBF80, 0x3F80, 0x3F81]  # ties to even, either side of a tie
    w = np.random.default_rng(1).standard_normal((5, 7, 3, 3)).astype(np.float32)
    p = R.bf16_value(R.pack_conv_weight(w)).reshape(5, 3, 3, 7)
    assert np.array_equal(p.transpose(0, 3, 1, 2), O.round_bf16(w))


@pytest.mark.parametrize("cpad", [18, 20, 64])
def test_bits_and_tokens_nhwc_are_layout_permutations_of_the_oracle(magvit, cpad):
    ids = magvit["bits_ids"]                                                   # (3, 4, 4)
    z = R.bits_from_tokens_nhwc(ids.reshape(-1), 18, cpad)
    assert z.dtype == np.uint16 and z.shape == (48, cpad)
    zf = R.bf16_value(z).reshape(3, 4, 4, cpad)
    assert np.array_equal(zf[..., :18].transpose(0, 3, 1, 2), O.bits_from_tokens(ids)) and np.array_equal(zf[..., :18].transpose(0, 3, 1, 2), magvit["bits_z"])
    assert not z[:, 18:].any()
    # ids with bits above `bits` set give the same planes
    assert np.array_equal(R.bits_from_tokens_nhwc(ids.reshape(-1) | (1 << 18) | (1 << 40), 18, cpad), z)
    # and back: the golden bit planes and the reference encoder's code, channels >= bits ignored
    for h in (magvit["bits_z"], O.round_bf16(magvit["enc_h"])):
        n, c, hh, ww = h.shape
        code = np.full((n * hh * ww, cpad), 0x3F80, np.uint16)                 # +1.0 in the padding: must not leak into the id
        code[:, :18] = R.bf16_bits(h.transpose(0, 2, 3, 1).reshape(-1, 18))
        assert np.array_equal(R.tokens_from_code_nhwc(code, 18).reshape(n, hh, ww), O.tokens_from_bits(h))
    assert np.array_equal(R.tokens_from_code_nhwc(z, 18).reshape(ids.shape), ids)
    # +0, -0, NaN, -subnormal, -inf: 0;  smallest positive subnormal, +inf: 1
    sp = np.array([[0x0000, 0x8000, 0x7FC0, 0x8001, 0xFF80, 0x0001, 0x7F80]], np.uint16)
    assert R.tokens_from_code_nhwc(sp, 7).tolist() == [0b1100000]


def test_rescale_nhwc_is_a_layout_permutation_of_the_oracle(magvit):
    x = magvit["rescale_in_bf16_as_f32"]                                       # 4096 bf16 values
    bits = R.bf16_bits(x)
    assert np.array_equal(R.bf16_value(bits), x)
    assert np.array_equal(R.rescale_u8_nhwc(bits.reshape(1, 4096, 1), 1).reshape(-1), magvit["rescale_out"])
    nhwc = bits.reshape(2, 512, 4)                                             # cpad 4, 3 channels used
    want = O.rescale_u8_bf16(x.reshape(2, 512, 4)[:, :, :3]).transpose(0, 2, 1)
    assert np.array_equal(R.rescale_u8_nhwc(nhwc, 3), want)
    d = magvit["dec_out_bf16_as_f32"]                                          # (2, 3, 8, 8) NCHW
    nhwc = np.zeros((2, 64, 8), np.uint16)
    nhwc[:, :, :3] = R.bf16_bits(d.reshape(2, 3, 64).transpose(0, 2, 1))
    assert np.array_equal(R.rescale_u8_nhwc(nhwc, 3).reshape(2, 3, 8, 8), magvit["dec_u8_bf16"])
    # every finite or infinite bf16: the oracle's bytes
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    allb = allb[~np.isnan(R.bf16_value(allb))]
    with np.errstate(over="ignore"):
        assert np.array_equal(R.rescale_u8_nhwc(allb.reshape(1, -1, 1), 1).reshape(-1), O.rescale_u8_bf16(R.bf16_value(allb)))
    edge = R.bf16_bits(np.array([-3.0, -1.0, -0.99609375, 0.0, 0.9921875, 1.0, 5.0], np.float32))
    assert R.rescale_u8_nhwc(edge.reshape(1, -1, 1), 1).reshape(-1).tolist() == [0, 0, 0, 127, 254, 255, 255]


@pytest.mark.parametrize("cpad", [3, 4, 64])
def test_frames_to_nhwc_all_bytes(cpad):
    f = np.arange(2 * 3 * 128, dtype=np.int64).reshape(2, 3, 128).astype(np.uint8)        # every byte value, in every channel
    assert len(np.unique(f[:, 0])) == 256
    x = R.frames_to_nhwc(f, cpad)
    assert x.shape == (2, 128, cpad) and x.dtype == np.uint16
    want = O.round_bf16(f.astype(np.float32) / np.float32(127.5) - np.float32(1.0))       # bf16(x / 127.5 - 1)
    assert np.array_equal(R.bf16_value(x[:, :, :3]).transpose(0, 2, 1), want)
    assert not x[:, :, 3:].any()
    assert R.bf16_value(R.frames_to_nhwc(np.array([[[0, 255]]], np.uint8), 1)).reshape(-1).tolist() == [-1.0, 1.0]


@pytest.mark.parametrize("name", ["magvit_small", "magvit_mid"])
def test_stride2_reference_agrees_with_the_oracle_downsample(name):
    """conv3x3_ref(stride=2) on packed NHWC operands == oracle/magvit2_oracle.py's downsample (Conv2d(3x3, stride 2, padding 1) of the
    reference's Encoder) on the activations the golden frames produce at that layer; the stride-1 and 1x1 forms likewise on a ResBlock's
    conv1 / the encoder's conv_out."""
    from oracle import magvit2_oracle as MO
    mv = pkg("magvit2")
    z = np.load(f"{GOLDEN}/{name}.npz")
    m = mv.VQModel(mv.VQConfig(**ast.literal_eval(str(z["cfg"]))))
    sd = mv.make_vq_state_dict(m, int(z["weight_seed"]))
    m.load_state_dict({k: torch.from_numpy(O.round_bf16(v)) for k, v in sd.items()})     # bf16-representable parameters
    m = m.double()
    enc = m.encoder
    with torch.no_grad():
        x = torch.from_numpy(z["enc_frames"]).double() / 127.5 - 1.0
        x = MO._conv(x, enc.conv_in)
        for blk in enc.down[0].block:
            x = MO.res_block(blk, x)
        x = torch.from_numpy(O.round_bf16(x.float().numpy())).to(torch.bfloat16)          # (n, C, H, W) bf16 activations
        ds = enc.down[0].downsample
        assert tuple(ds.stride) == (2, 2) and tuple(ds.padding) == (1, 1)
        want = MO._conv(x.double(), ds)
        wp = torch.from_numpy(R.pack_conv_weight(ds.weight.float().numpy()).view(np.int16)).view(torch.bfloat16)
        got = R.conv3x3_ref(x.permute(0, 2, 3, 1).contiguous(), wp, ds.bias.float(), stride=2)
        assert got.shape == (x.shape[0], x.shape[2] // 2, x.shape[3] // 2, ds.weight.shape[0])
        assert (got.permute(0, 3, 1, 2) - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())
        mag = R.conv3x3_mag(x.permute(0, 2, 3, 1).contiguous(), wp, ds.bias.float(), stride=2)
        assert (mag >= got.abs() * (1 - 1e-12)).all()
        c1 = enc.down[1].block[0].conv1                                                   # stride 1, no bias, channel change
        xs = torch.from_numpy(O.round_bf16(want.float().numpy())).to(torch.bfloat16)
        wp1 = torch.from_numpy(R.pack_conv_weight(c1.weight.float().numpy()).view(np.int16)).view(torch.bfloat16)
        got1 = R.conv3x3_ref(xs.permute(0, 2, 3, 1).contiguous(), wp1)
        want1 = MO._conv(xs.double(), c1)
        assert (got1.permute(0, 3, 1, 2) - want1).abs().max().item() < 1e-12 * max(1.0, want1.abs().max().item())
        # depth-to-space is the oracle's
        assert torch.equal(R.depth_to_space_dcr(want1[:, :want1.shape[1] // 4 * 4]), MO.depth_to_space(want1[:, :want1.shape[1] // 4 * 4], 2))
        co = enc.conv_out                                                                 # 1x1 with bias
        xo = torch.from_numpy(O.round_bf16(want1.float().numpy())).to(torch.bfloat16)
        wpo = torch.from_numpy(R.pack_conv_weight(co.weight.float().numpy()).view(np.int16)).view(torch.bfloat16)
        goto = R.conv1x1_ref(xo.permute(0, 2, 3, 1).reshape(-1, xo.shape[1]), wpo.view(wpo.shape[0], -1), co.bias.float())
        wanto = MO._conv(xo.double(), co).permute(0, 2, 3, 1).reshape(-1, co.weight.shape[0])
        assert (goto - wanto).abs().max().item() < 1e-12 * max(1.0, wanto.abs().max().item())


GN_SHAPES = [(50, 128, 32), (200, 256, 32), (1000, 64, 16), (20000, 128, 32), (64, 2048, 32), (37, 8, 2), (65536, 128, 32)]


def gn_input(n, HW, C, groups, ratio, seed):
    """(n, HW, C) bf16 bit patterns whose groups have mean / std ~ `ratio` and a scale that differs per group."""
    g = np.random.default_rng(seed)
    scale = g.uniform(0.5, 2.0, size=(n, 1, groups, 1)).astype(np.float32)
    x = (g.standard_normal((n, HW, groups, C // groups), dtype=np.float32) + np.float32(ratio)) * scale
    return R.bf16_bits(x.reshape(n, HW, C))


def test_gn_chain_lengths():
    assert [R.gn_chain_length(*s) for s in GN_SHAPES] == [1 + 2 * 4 + 16, 1 + 2 * 8 + 16, 1 + 2 * 2 + 32, 1 + 2 * 32 + 16, 1 + 2 * 64 + 16,
                                                          1 + 2 * 1 + 256, 1 + 2 * 32 + 16]


@pytest.mark.parametrize("ratio", [0, 4, 16])
@pytest.mark.parametrize("HW,C,groups", GN_SHAPES)
def test_gn_statistics_bound_holds_for_f32_partials_in_kernel_order(HW, C, groups, ratio):
    """The f64 statistics against f32 partial sums added in the separate statistics pass's order: inside
    rel(rstd) <= 2 * n_acc * 2^-24 * (1 + (mean/std)^2) and |d mean| <= 2 * n_acc * 2^-24 * sqrt(mean^2 + var) -- the bound
    tests/test_hip_conv.py then holds the kernel to."""
    n = 1 if HW >= 20000 else 2
    xb = gn_input(n, HW, C, groups, ratio, seed=HW + C + ratio)
    x = torch.from_numpy(xb.view(np.int16)).view(torch.bfloat16)
    one, zero = torch.ones(C), torch.zeros(C)
    _, mean, rstd, var = R.group_norm_ref(x, groups, one, zero, 1e-6, False)
    m32, r32 = R.gn_stats_f32_ordered(xb, groups, 1e-6)
    dm, rr = R.gn_stats_bound(HW, C, groups, mean, var)
    em = (torch.from_numpy(m32).double() - mean).abs()
    er = (torch.from_numpy(r32).double() / rstd - 1).abs()
    assert (em <= dm).all() and (er <= rr).all(), ((em / dm).max().item(), (er / rr).max().item())
    if ratio:  # the inputs are what they claim
        assert ((mean / var.sqrt()) > 0.8 * ratio).all() and ((mean / var.sqrt()) < 1.25 * ratio).all()
