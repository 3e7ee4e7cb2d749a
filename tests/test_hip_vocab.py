"""GPU (-m gpu): vocabularies other than the shipped 2 x 512.  genie_check_config admits 1 to 4 factored vocabularies of any size;
the kernels keep a 2 x 512 fast path (register CE, sample_rows_kernel<8>) and a generic one.  Here the generic paths, the 1 / 3 / 4
embedding tables, the ragged and narrow readout widths and the V < d workspace are held to the f64 / f32 oracle and to the
reference's own outputs (tests/golden/vocab_*.npz, tools/make_goldens.py vocab)."""
import ctypes
import math

import numpy as np
import pytest

from conftest import load_golden, pkg
from oracle import genie_oracle as O
from oracle import genie_train_oracle as TO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECISIONS = ["exact", "f16x3", "bf16"]
FIXTURES = ["vocab_v4096_n1", "vocab_v64_n3_qknorm", "vocab_v16_n4", "vocab_v100_n2"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_cfg(image_vocab_size, nv, d=64, heads=2, layers=2, T=4, S=16, qk_norm=False):
    return pkg("config").GenieConfig(num_layers=layers, num_heads=heads, d_model=d, T=T, S=S, image_vocab_size=image_vocab_size,
                                     num_factored_vocabs=nv, qk_norm=qk_norm, use_mup=False)


# name -> (cfg, state dict, B, ids, golden or None)
def _case(name):
    if name in FIXTURES:
        z, cfg, sd = load_golden(name)
        return cfg, sd, z["ids"].shape[0], z["ids"], z
    geo = {
        # V = 192 < d = 256 on the generic spatial (S = 64) and temporal (T = 4 / T = 32) attention paths
        "v192_d256_t4": dict(image_vocab_size=262144, nv=3, d=256, heads=4, layers=2, T=4, S=64),
        "v192_d256_t32": dict(image_vocab_size=262144, nv=3, d=256, heads=4, layers=1, T=32, S=16),
        # the shipped 2 x 512 vocabulary at d = 1536 (V = 1024 < d), heads of 64
        "v1024_d1536": dict(image_vocab_size=262144, nv=2, d=1536, heads=24, layers=1, T=4, S=16),
        # the reference's dataclass default: one vocabulary of 262,144 logits per token
        "v262144_n1": dict(image_vocab_size=262144, nv=1, d=64, heads=2, layers=1, T=4, S=16),
    }[name]
    cfg = make_cfg(**geo)
    sd = pkg("synthetic").make_state_dict(cfg, seed=31 + cfg.d_model + cfg.T, law="conditioned")
    B = 1 if name == "v262144_n1" else 2
    ids = pkg("synthetic").make_clips(B, cfg, seed=17 + cfg.S)
    return cfg, sd, B, ids, None


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _case(name)
    return _CASES[name]


def model(cfg, sd, precision):
    return pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")


def nm_of(precision):
    return {"exact": O.F32, "f16x3": O.F32, "bf16": O.BF16_MFMA}[precision]


def check_logits(lg, ref, precision, what):
    scale = max(1.0, float(np.abs(ref).max()) / 8)
    err = np.abs(lg - ref)
    if precision == "bf16":
        assert np.median(err) < 4e-3 * scale and err.max() < 0.1 * scale, (what, np.median(err), err.max())
    else:
        assert err.max() < 5e-5 * scale, (what, err.max())
    return float(err.max() / scale)


def ids_bar(precision):
    return 0.98 if precision != "bf16" else 0.9


MODEL_CASES = FIXTURES + ["v192_d256_t4", "v192_d256_t32", "v1024_d1536", "v262144_n1"]


@pytest.mark.parametrize("name", MODEL_CASES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_vocab_model_vs_oracle(name, precision):
    """compute_logits in both layouts, forward loss / acc, genie_factored_ce on the logits, MaskGIT at temperature 0 and > 0 in
    both unmask modes, and genie_generate_cached -- against the oracle (and the reference's own goldens where they exist)."""
    cfg, sd, B, ids, z = case(name)
    V = cfg.factored_vocab_size * cfg.num_factored_vocabs
    nv, vf = cfg.num_factored_vocabs, cfg.factored_vocab_size
    T, S = cfg.T, cfg.S
    H = W = math.isqrt(S)
    m = model(cfg, sd, precision)
    nm = nm_of(precision)
    x = ids.reshape(B, T, H, W).copy()
    x[:, T // 2:] = cfg.image_vocab_size
    # logits, both layouts, of the half-masked clip
    ref = O.compute_logits(x, sd, cfg, nm)
    lg = m.compute_logits(dev(x)).cpu().numpy()
    assert lg.shape == ref.shape == (B, V, T, H, W)
    check_logits(lg, ref, precision, "bcthw")
    tok = m.compute_logits_frames(dev(x), 0, T, "token").cpu().numpy()
    assert tok.shape == (B, T, S, V)
    assert np.array_equal(tok, lg.reshape(B, V, T, S).transpose(0, 2, 3, 1))   # the same numbers in the other layout
    if z is not None and precision != "bf16":   # the reference's own logits of the unmasked clip
        full = m.compute_logits(dev(ids.reshape(B, T, H, W))).cpu().numpy()
        if "probe_t" in z.files:
            full = np.stack([full[:, :, t, s // W, s % W] for t, s in zip(z["probe_t"], z["probe_s"])], 1)
            check_logits(full, z["probe_logits"], precision, "golden probes")
        else:
            check_logits(full, z["logits"], precision, "golden")
    # forward loss / acc (masked mean over frames >= 1) and the standalone CE kernel on the returned logits
    loss_bar = 1e-4 if precision != "bf16" else 3e-3
    fin = z["fwd_input"] if z is not None else x.reshape(B, -1)
    out = m(dev(fin), dev(ids))
    loss_o, acc_o, _ = O.forward_loss_acc(fin, ids, sd, cfg, nm)
    assert abs(out.loss.item() - loss_o) < loss_bar, (out.loss.item(), loss_o)
    assert abs(out.acc.item() - acc_o) < 1e-6 or precision == "bf16", (out.acc.item(), acc_o)
    if z is not None and precision != "bf16":
        assert abs(out.loss.item() - float(z["fwd_loss"])) < loss_bar
        assert abs(out.acc.item() - float(z["fwd_acc"])) < 1e-6
    lib = pkg("_lib")
    L = lib.load()
    c = lib.make_cfg(cfg, lib.PREC_EXACT)
    lgt = out.logits[:, :, 1:].contiguous()
    tgt = dev(ids)
    fin_d = dev(fin)
    for layout, arr in ((lib.LAYOUT_BCTHW, lgt), (lib.LAYOUT_TOKEN_MAJOR, lgt.permute(0, 2, 3, 4, 1).contiguous())):
        sums = torch.zeros(3, dtype=torch.float64, device="cuda")
        lib.check(L.genie_factored_ce(c, arr.data_ptr(), layout, tgt.data_ptr(), fin_d.data_ptr(), B, 1, T, sums.data_ptr(),
                                      stream()), "genie_factored_ce")
        ce_ref, hit_ref = O._factored_ce_and_hit(O._to_factored(out.logits.cpu().numpy()[:, :, 1:].astype(np.float64), cfg),
                                                 ids.reshape(B, T, H, W)[:, 1:], cfg)
        wmask = fin.reshape(B, T, H, W)[:, 1:] == cfg.image_vocab_size
        s = sums.cpu().numpy()
        assert s[2] == wmask.sum()
        assert abs(s[0] - ce_ref[wmask].sum()) < 1e-5 * max(1.0, abs(ce_ref[wmask].sum())), (layout, s[0], ce_ref[wmask].sum())
        assert s[1] == hit_ref[wmask].sum()
    # temperature > 0, one step: the ids are the f64 inverse-CDF picks on the decode's own step-0 logits for every draw further than
    # 1e-6 (of the sum) from a CDF step -- independent of how far the logits are from the oracle's
    t0 = T // 2
    u1 = pkg("synthetic").make_noise((1, nv, B, S), seed=3)
    s1, fl1 = m.maskgit_generate(dev(x), t0, maskgit_steps=1, temperature=1.0, uniforms=dev(u1))
    s1, fl1 = s1.cpu().numpy().reshape(B, S), fl1.cpu().numpy().astype(np.float64).reshape(B, vf, nv, S)
    want, ambiguous = np.zeros((B, S), np.int64), np.zeros((B, S), bool)
    for k, f in enumerate(range(nv - 1, -1, -1)):   # the most significant vocabulary first (st_mask_git.py:179)
        e = np.exp(fl1[:, :, f] - fl1[:, :, f].max(1, keepdims=True))
        tot, cdf = e.sum(1), np.cumsum(e, 1)
        target = u1[0, k].astype(np.float64) * tot
        want = want * vf + np.minimum((cdf < target[:, None]).sum(1), vf - 1)
        ambiguous |= (np.abs(cdf - target[:, None]).min(1) / tot) < 1e-6
    assert (~ambiguous).any()
    assert np.array_equal(s1[~ambiguous], want[~ambiguous]), int((s1[~ambiguous] != want[~ambiguous]).sum())
    # MaskGIT on the first masked frame: temperature 0 (both unmask modes) and > 0 with caller uniforms
    noise = pkg("synthetic").make_noise((1, B, S), seed=5)
    for mode in ("random", "greedy"):
        for temp in (0.0, 1.0):
            u = pkg("synthetic").make_noise((2, nv, B, S), seed=9) if temp else None
            p_dev = dev(x)
            s_dev, fl = m.maskgit_generate(p_dev, t0, maskgit_steps=2, temperature=temp, unmask_mode=mode, noise=dev(noise),
                                           uniforms=None if u is None else dev(u))
            s_o, fl_o = O.maskgit_generate(x.copy(), t0, sd, cfg, 2, temp, mode, noise=noise,
                                           uniforms=None if u is None else u.reshape(2, nv, B, H, W), nm=nm)
            s_dev = s_dev.cpu().numpy()
            assert s_dev.min() >= 0 and s_dev.max() < cfg.image_vocab_size
            assert fl.shape == (B, vf, nv, H, W)
            check_logits(fl.cpu().numpy(), fl_o, precision, "step-0 logits")
            same = (s_dev == s_o).mean()
            if temp == 0:
                assert same > ids_bar(precision), (mode, same)
            elif precision != "bf16" and vf <= 4096:
                # (an inverse-CDF pick moves with any logit difference above the CDF step spacing: ~1 / vf of the sum for the
                # flat logits of 262,144 classes, and bf16's 0.1 moves steps everywhere -- those are held by the check above)
                assert same > 0.95, (mode, same)
            assert np.array_equal(p_dev[:, t0].cpu().numpy(), s_dev)
    if z is not None and precision != "bf16":   # the reference's own decodes (every tracked top-2 gap > 2e-4)
        for steps in (1, 3, 8):
            for mode in ("random", "greedy"):
                k = f"mg_s{steps}_{mode}"
                p = z["ids"].reshape(B, T, H, W).copy()
                p[:, 2:] = cfg.image_vocab_size
                nz = z[k + "_noise"]
                s_dev, _ = m.maskgit_generate(dev(p), 2, maskgit_steps=steps, unmask_mode=mode,
                                              noise=dev(nz) if nz.size else None)
                assert np.array_equal(s_dev.cpu().numpy(), z[k + "_samples"]), (k, int((s_dev.cpu().numpy() != z[k + "_samples"]).sum()))
    # generate: T - 2 prompt frames -> the last 2 frames of the clip on the temporal KV cache (genie_generate_cached)
    P = T - 2
    n_new = 2
    gnoise = pkg("synthetic").make_noise((n_new, 1, B, S), seed=77)
    g_dev = m.generate(dev(ids[:, :P * S]), max_new_tokens=n_new * S, maskgit_steps=2, noise=dev(gnoise)).cpu().numpy()
    g_o = O.generate(ids[:, :P * S], n_new * S, sd, cfg, maskgit_steps=2, noise=gnoise, nm=nm)
    assert g_dev.shape == g_o.shape
    assert np.array_equal(g_dev[:, :P * S], ids[:, :P * S])
    assert (g_dev[:, P * S:] == g_o[:, P * S:]).mean() > ids_bar(precision)
    if z is not None and precision != "bf16":
        g_ref = m.generate(dev(z["ids"][:, :P * S]), max_new_tokens=2 * S, maskgit_steps=2, noise=dev(z["gen_noise"])).cpu().numpy()
        assert np.array_equal(g_ref, z["gen_out"])


def test_fragment_order_frame_readout_at_v192():
    """The f16x3 one-frame passes read out with the fragment-order GEMM (readout_frame_f16x3, V % 64 == 0); at V = 192 the width is
    not a multiple of 128, so the readout takes launch_fr_w instead of the mid-size kernel.  d 256, S 256, T 16."""
    cfg = make_cfg(262144, 3, d=256, heads=4, layers=2, T=16, S=256)
    sd = pkg("synthetic").make_state_dict(cfg, seed=5, law="conditioned")
    B, P = 1, 2
    ids = pkg("synthetic").make_clips(B, cfg, seed=6)
    m = model(cfg, sd, "f16x3")
    assert m._weights()[1].out_frame_w16, "no fragment-order readout stream was packed"
    lib = pkg("_lib")
    L = lib.load()
    noise = pkg("synthetic").make_noise((1, 1, B, cfg.S), seed=8)
    lib.check(L.genie_profile_enable(1 << lib.KC_GEMM), "profile_enable")
    L.genie_profile_reset()
    try:
        g_dev, lg = m.generate(dev(ids[:, :P * cfg.S]), max_new_tokens=cfg.S, maskgit_steps=2, noise=dev(noise), return_logits=True)
        torch.cuda.synchronize()
        kbuf = ctypes.create_string_buffer(8192)
        lib.check(L.genie_profile_kernels(lib.KC_GEMM, kbuf, len(kbuf)), "profile_kernels")
    finally:
        L.genie_profile_enable(0)
    launched = {ln.split("\t")[0]: int(float(ln.split("\t")[1])) for ln in kbuf.value.decode().splitlines() if "\t" in ln}
    assert launched.get("gemm16_fr(m)_kernel (readout)", 0) >= 2, launched   # one readout per MaskGIT step
    p = ids.reshape(B, cfg.T, 16, 16).copy()
    p[:, P:] = cfg.image_vocab_size
    s_o, fl_o = O.maskgit_generate(p, P, sd, cfg, 2, 0.0, "random", noise=noise[0])
    check_logits(lg[:, :, :, 0].cpu().numpy(), fl_o, "f16x3", "frame readout")
    assert (g_dev.cpu().numpy()[:, P * cfg.S:].reshape(B, 16, 16) == s_o).mean() > 0.98


SAMPLE_VOCABS = [(16, 4), (64, 3), (100, 2), (512, 2), (4096, 2), (262144, 1)]


@pytest.mark.parametrize("vf,nv", SAMPLE_VOCABS)
def test_sample_kernel_vs_f64_softmax(vf, nv):
    """genie_sample on given logits, both layouts: argmax ids exact, confidence within 1e-6 of the f64 softmax, inverse-CDF picks
    exact for every draw further than 2e-6 (of the sum) from a CDF step, and the two layouts bit-identical."""
    lib = pkg("_lib")
    L = lib.load()
    S = 64 if vf <= 512 else 16
    R = 8 if vf <= 512 else 4 if vf <= 4096 else 2
    cfg = make_cfg(vf ** nv, nv, T=4, S=S)
    c = lib.make_cfg(cfg, lib.PREC_EXACT)
    g = np.random.default_rng(vf + nv)
    V = vf * nv
    scale = 2.5 if vf <= 4096 else 8.0   # a peaked law for 262,144 classes: CDF steps of ~1/V would leave few draws clear of a step
    logits = (g.standard_normal((R, S, V)) * scale).astype(np.float32)
    logits[0, 0, :vf] = 1.0                                         # an all-equal factor: first max wins
    uni = g.random((nv, R, S), dtype=np.float32)
    tm, bc = dev(logits), dev(logits.transpose(0, 2, 1))
    u_d = dev(uni)
    res = {}
    for temp in (0.0, 0.7):
        for layout, arr in ((lib.LAYOUT_TOKEN_MAJOR, tm), (lib.LAYOUT_BCTHW, bc)):
            samples = torch.full((R, S), -1, dtype=torch.int64, device="cuda")
            conf = torch.full((R, S), -1.0, dtype=torch.float32, device="cuda")
            lib.check(L.genie_sample(c, arr.data_ptr(), layout, R, temp, u_d.data_ptr() if temp else 0, samples.data_ptr(),
                                     conf.data_ptr(), stream()), "genie_sample")
            res[temp, layout] = (samples.cpu().numpy(), conf.cpu().numpy())
        a, b = res[temp, lib.LAYOUT_TOKEN_MAJOR], res[temp, lib.LAYOUT_BCTHW]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), temp
    picks0, picks1, ambiguous = [], [], np.zeros((R, S), bool)
    conf0, conf1 = np.ones((R, S)), np.ones((R, S))
    for k, f in enumerate(range(nv - 1, -1, -1)):   # the most significant vocabulary first (st_mask_git.py:179)
        l = logits[:, :, f * vf:(f + 1) * vf].astype(np.float64)
        e = np.exp(l - l.max(-1, keepdims=True))
        tot = e.sum(-1)
        am = l.argmax(-1)
        picks0.append(am)
        conf0 *= 1.0 / tot
        cdf = np.cumsum(e, -1)
        target = uni[k].astype(np.float64) * tot
        pick = np.minimum((cdf < target[..., None]).sum(-1), vf - 1)
        ambiguous |= (np.abs(cdf - target[..., None]).min(-1) / tot) < 2e-6
        picks1.append(pick)
        conf1 *= np.take_along_axis(e, pick[..., None], -1)[..., 0] / tot
    pw = vf ** np.arange(nv - 1, -1, -1, dtype=np.int64)
    want0 = sum(p * w for p, w in zip(picks0, pw))
    want1 = sum(p * w for p, w in zip(picks1, pw))
    s0, c0 = res[0.0, lib.LAYOUT_TOKEN_MAJOR]
    s1, c1 = res[0.7, lib.LAYOUT_TOKEN_MAJOR]
    assert np.array_equal(s0, want0), int((s0 != want0).sum())
    assert s0.max() < vf ** nv and s1.max() < vf ** nv and s1.min() >= 0
    np.testing.assert_allclose(c0, conf0, rtol=1e-6)
    assert ambiguous.mean() < 0.05, ambiguous.mean()
    clear = ~ambiguous
    assert np.array_equal(s1[clear], want1[clear]), int((s1[clear] != want1[clear]).sum())
    np.testing.assert_allclose(c1[clear], conf1[clear], rtol=1e-6)


TRAIN_CASES = [
    # image_vocab_size, nv, precision
    (262144, 3, "exact"), (262144, 3, "bf16"),     # 3 tables of 64
    (64, 1, "exact"), (64, 1, "bf16"),             # one table of 64
    (65536, 4, "exact"), (65536, 4, "bf16"),       # 4 tables of 16
]


@pytest.mark.parametrize("iv,nv,precision", TRAIN_CASES)
def test_train_gradients_vs_oracle(iv, nv, precision):
    """One forward / backward of the training step against oracle/genie_train_oracle.py: ce_fwd_bwd_kernel at the new vf, and
    embed_bwd_tables_kernel with 1, 3 and 4 tables.  exact: loss 1e-5 relative, every gradient within 1e-4 of its largest element;
    bf16: 3 % Frobenius, loss 1e-2 (tests/test_hip_train.py's bars)."""
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, image_vocab_size=iv, num_factored_vocabs=nv,
                                    qk_norm=False, use_mup=False, num_prompt_frames=2)
    sd = pkg("synthetic").make_state_dict(cfg, seed=21 + nv, law="conditioned")
    batch = TO.maskgit_collate(pkg("synthetic").make_clips(2, cfg, seed=22), cfg, TO.NumpyDraws(23))
    loss_o, acc_o, g_o = TO.forward_backward(batch["input_ids"], batch["labels"], sd, cfg)
    tr = pkg("train").GenieTrainer(model(cfg, sd, precision))
    loss, acc = tr.forward_backward(dev(batch["input_ids"]), dev(batch["labels"]))
    grads = tr.gradients()
    assert sorted(grads) == sorted(g_o)
    assert sum(k.startswith("token_embed.factored_embeds.") for k in grads) == nv
    if precision == "exact":
        assert abs(float(loss) - loss_o) < 1e-5 * abs(loss_o), (float(loss), loss_o)
        assert abs(float(acc) - acc_o) < 1e-7
        bad = {k: e for k, g in grads.items()
               if (e := float(np.abs(g.cpu().numpy() - g_o[k]).max() / (np.abs(g_o[k]).max() + 1e-30))) > 1e-4}
    else:
        assert abs(float(loss) - loss_o) < 1e-2, (float(loss), loss_o)
        bad = {}
        for k, g in grads.items():
            a, r = g.cpu().numpy().astype(np.float64), g_o[k].astype(np.float64)
            e = float(np.sqrt(((a - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + 1e-30))
            if e > 3e-2:
                bad[k] = e
    assert not bad, bad


def test_train_refuses_a_readout_width_off_the_16_grid():
    """V = 100: the training step's head backward GEMM contracts over V in steps of 16 -- it must refuse, not compute."""
    cfg = pkg("config").GenieConfig(num_layers=1, num_heads=2, d_model=64, T=4, S=16, image_vocab_size=100, num_factored_vocabs=1,
                                    qk_norm=False, use_mup=False, num_prompt_frames=2)
    sd = pkg("synthetic").make_state_dict(cfg, seed=5, law="conditioned")
    batch = TO.maskgit_collate(pkg("synthetic").make_clips(2, cfg, seed=6), cfg, TO.NumpyDraws(7))
    tr = pkg("train").GenieTrainer(model(cfg, sd, "exact"))
    with pytest.raises(pkg("_lib").GenieHipError, match="multiple of 16"):
        tr.forward_backward(dev(batch["input_ids"]), dev(batch["labels"]))
