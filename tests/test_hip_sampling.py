"""The sampling law on the GPU (csrc/kernels_sample.hip through genie_sample_ex and the *_ex generate entry points): neutral law =
the kernels of before bit for bit, draw by draw against the f64 model of tests/sampling_model.py, row kernel = strided kernel,
the drawn distribution, tempering, the "confidence" unmasking keys, and the module-level paths against each other.
Needs a real MI355X: run with ``-m gpu``."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import sampling_model as SM
from conftest import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VF = 512
OFF = (1.0, 0, 1.0)
# (tau, top_k, top_p) of the draw-by-draw test
CONFIGS = [(0.7, 0, 1.0), (1.3, 50, 1.0), (1.0, 0, 0.9), (0.7, 8, 0.5), (1.3, 50, 0.95), (1.0, 1, 1.0), (2.0, 0, 0.3)]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def stream():
    return torch.cuda.current_stream().cuda_stream


def sample_cfg(S=256, image_vocab_size=262144, nv=2):
    lib = pkg("_lib")
    cfg = pkg("config").GenieConfig(num_layers=1, num_heads=2, d_model=64, T=4, S=S, image_vocab_size=image_vocab_size,
                                    num_factored_vocabs=nv, qk_norm=False, use_mup=False)
    return lib.make_cfg(cfg, lib.PREC_EXACT)


def law_of(tau, k, p, c=4.5):
    return pkg("_lib").Sampling(tau, k, p, c)


def run_ex(c, logits, layout, R, S, temperature, uni, law, noise=None, anneal=0.0):
    """genie_sample_ex -> (samples, conf, keys or None) as numpy."""
    lib = pkg("_lib")
    L = lib.load()
    samples = torch.full((R, S), -1, dtype=torch.int64, device="cuda")
    conf = torch.full((R, S), -1.0, dtype=torch.float32, device="cuda")
    keys = torch.full((R, S), -7.0, dtype=torch.float32, device="cuda") if noise is not None else None
    lib.check(L.genie_sample_ex(c, logits.data_ptr(), layout, R, temperature, 0 if uni is None else uni.data_ptr(), samples.data_ptr(),
                                conf.data_ptr(), stream(), law, 0 if keys is None else keys.data_ptr(),
                                0 if noise is None else noise.data_ptr(), anneal), "genie_sample_ex")
    return samples.cpu().numpy(), conf.cpu().numpy(), None if keys is None else keys.cpu().numpy()


def run_old(c, logits, layout, R, S, temperature, uni):
    lib = pkg("_lib")
    L = lib.load()
    samples = torch.full((R, S), -1, dtype=torch.int64, device="cuda")
    conf = torch.full((R, S), -1.0, dtype=torch.float32, device="cuda")
    lib.check(L.genie_sample(c, logits.data_ptr(), layout, R, temperature, 0 if uni is None else uni.data_ptr(), samples.data_ptr(),
                             conf.data_ptr(), stream()), "genie_sample")
    return samples.cpu().numpy(), conf.cpu().numpy()


def tie_inputs(seed=23, R=9, S=256):
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((R, S, 2 * VF)) * 2.5).astype(np.float32)
    logits[0, :, 100] = logits[0, :, 300] = 20.0       # ties: the first maximum wins
    logits[1, :, VF + 7] = logits[1, :, VF + 8] = 19.0
    logits[2, :, 10:40] = 3.0                          # a plateau that a top-k / top-p boundary cuts through
    logits[2, :, VF + 200:VF + 260] = 2.0
    uni = g.random((2, R, S), dtype=np.float32)
    return logits, uni


# ------------------------------------------------------------------------------------------ neutral = the kernels of before
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_neutral_law_equals_genie_sample_bit_for_bit(temperature):
    """Every field off (tau 1; top_k 0 or >= 512; top_p >= 1 or <= 0), and no law at all: the samples and the bits of conf of
    genie_sample, both layouts, ties included.  With keys_out the filtered kernel itself runs the neutral law: same bits again."""
    lib = pkg("_lib")
    R, S = 9, 256
    c = sample_cfg(S)
    logits, uni = tie_inputs()
    d_tok, d_uni = dev(logits), dev(uni)
    d_bvs = d_tok.permute(0, 2, 1).contiguous()
    noise = torch.rand(R, S, device="cuda")
    for buf, layout in ((d_tok, lib.LAYOUT_TOKEN_MAJOR), (d_bvs, lib.LAYOUT_BCTHW)):
        s0, c0 = run_old(c, buf, layout, R, S, temperature, d_uni)
        for law in (None, law_of(*OFF), law_of(1.0, VF, 1.0), law_of(1.0, 100000, 7.0), law_of(1.0, 0, 0.0), law_of(1.0, 0, -1.0)):
            s1, c1, _ = run_ex(c, buf, layout, R, S, temperature, d_uni, law)
            assert np.array_equal(s0, s1) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32)), (layout, law)
        s2, c2, k2 = run_ex(c, buf, layout, R, S, temperature, d_uni, law_of(*OFF), noise=noise, anneal=0.5)
        assert np.array_equal(s0, s2) and np.array_equal(c0.view(np.uint32), c2.view(np.uint32)), layout
        assert np.isfinite(k2[c0 > 0]).all()


# ------------------------------------------------------------------------------------------ draw by draw against the f64 model
@pytest.fixture(scope="module")
def margin_inputs():
    """The inputs of test_hip_parity.py::test_sample_temperature_exact_outside_cdf_margins."""
    g = np.random.default_rng(17)
    R, S = 24, 256
    logits = (g.standard_normal((R, S, 2 * VF)) * 2.5).astype(np.float32)
    uni = g.random((2, R, S), dtype=np.float32)
    return logits, uni, dev(logits), dev(uni)


def check_against_model(got_ids, got_conf, logits, uni, vf, tau, k, p, cap):
    nv = logits.shape[-1] // vf
    want = SM.sample(logits, uni, vf, tau, k, p)
    share = want["ambiguous"].mean()
    print(f"law (tau={tau}, top_k={k}, top_p={p}) vf={vf}: ambiguous share {share:.4f}")
    assert share < cap, share
    clear = ~want["ambiguous"]
    assert np.array_equal(got_ids[clear], want["ids"][clear]), int((got_ids[clear] != want["ids"][clear]).sum())
    np.testing.assert_allclose(got_conf[clear], want["conf"][clear], rtol=2e-5)
    # every token, ambiguous or not: the pick lies inside the f64 kept set widened by the boundary entry
    rest = got_ids.copy()
    for j in range(nv - 1, -1, -1):               # least significant digit first = the last factor drawn
        pick = rest % vf
        rest = rest // vf
        inside = np.take_along_axis(SM.widened_kept(want["laws"][j], p), pick[..., None], -1)[..., 0]
        assert inside.all(), (j, int((~inside).sum()))
    return want, clear


@pytest.mark.parametrize("tau,k,p", CONFIGS)
def test_filtered_draws_equal_the_f64_model_outside_the_margins(margin_inputs, tau, k, p):
    """On the same logits and uniforms the kernel's pick equals the f64 model's for every token that is not ambiguous: inverse-CDF
    target further than 2e-6 (of the total) from a CDF step of the kept entries and, with top-p on, no surviving rank >= 1 whose
    mass-before lies within 2e-6 of top_p.  Top-k needs no margin (exact on f32 values).  Ambiguous tokens are < 1 % per law;
    confidence = the tempered unfiltered softmax at rtol 2e-5; and NO token, ambiguous or not, is a filtered-out id."""
    lib = pkg("_lib")
    logits, uni, d_logits, d_uni = margin_inputs
    R, S = uni.shape[1:]
    ids, conf, _ = run_ex(sample_cfg(S), d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(tau, k, p))
    check_against_model(ids, conf, logits, uni, VF, tau, k, p, cap=0.01)


def test_top_p_of_one_or_more_is_off(margin_inputs):
    """Near the tail every prefix mass is within 2e-6 of 1: top_p >= 1 must not filter at all (genie_sample's own picks)."""
    lib = pkg("_lib")
    logits, uni, d_logits, d_uni = margin_inputs
    R, S = uni.shape[1:]
    c = sample_cfg(S)
    s0, _ = run_old(c, d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni)
    for p in (1.0, 1.5):
        s1, _, _ = run_ex(c, d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(1.0, 0, p))
        assert np.array_equal(s0, s1)
        s2, _, _ = run_ex(c, d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(0.7, 0, p))    # (tempered: the new kernel)
        want = SM.sample(logits, uni, VF, 0.7, 0, p)
        assert np.array_equal(s2[~want["ambiguous"]], want["ids"][~want["ambiguous"]])


def test_argmax_under_a_law_keeps_the_pick_and_tempers_the_confidence(margin_inputs):
    """temperature <= 1e-8: the arg-max, whatever the filters; conf = the tempered unfiltered softmax of it."""
    lib = pkg("_lib")
    logits, uni, d_logits, _ = margin_inputs
    R, S = uni.shape[1:]
    c = sample_cfg(S)
    s0, _ = run_old(c, d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.0, None)
    s1, c1, _ = run_ex(c, d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.0, None, law_of(0.7, 5, 0.2))
    want = SM.sample(logits, uni, VF, 0.7, 5, 0.2, temperature=0.0)
    assert np.array_equal(s0, s1) and np.array_equal(s1, want["ids"])
    np.testing.assert_allclose(c1, want["conf"], rtol=2e-5)


# ------------------------------------------------------------------------------------------ the two kernel flavours
@pytest.mark.parametrize("temperature,tau,k,p", [(0.8, 0.7, 50, 0.9), (0.8, 1.0, 25, 1.0), (0.8, 1.3, 0, 0.6), (0.0, 0.7, 50, 0.9)])
def test_filtered_row_kernel_equals_strided_kernel(temperature, tau, k, p):
    """Token-major 2 x 512 logits take the register kernel, the same logits in the (B, V, S) layout the strided one: the same
    operations in the same order, so samples, confidences and keys are bit-identical; ties and plateaus across the top-k / top-p
    boundaries included."""
    lib = pkg("_lib")
    R, S = 9, 256
    c = sample_cfg(S)
    logits, uni = tie_inputs()
    d_tok, d_uni = dev(logits), dev(uni)
    d_bvs = d_tok.permute(0, 2, 1).contiguous()
    noise = torch.rand(R, S, device="cuda")
    a = run_ex(c, d_tok, lib.LAYOUT_TOKEN_MAJOR, R, S, temperature, d_uni, law_of(tau, k, p), noise=noise, anneal=0.5)
    b = run_ex(c, d_bvs, lib.LAYOUT_BCTHW, R, S, temperature, d_uni, law_of(tau, k, p), noise=noise, anneal=0.5)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    if temperature > 0:     # and the plateaus are cut where the f64 model cuts them (top-k: exact)
        want = SM.sample(logits, uni, VF, tau, k, p)
        clear = ~want["ambiguous"]
        assert np.array_equal(a[0][clear], want["ids"][clear])


@pytest.mark.parametrize("vf,nv,tau,k,p", [(100, 2, 1.3, 20, 0.9), (64, 3, 0.7, 8, 0.8)])
def test_other_vocabularies_against_the_f64_model(vf, nv, tau, k, p):
    """Vocabularies other than 2 x 512 (geometries of tests/test_hip_vocab.py) take the strided kernel in both layouts."""
    lib = pkg("_lib")
    R, S = 8, 64
    c = sample_cfg(S, image_vocab_size=vf ** nv, nv=nv)
    g = np.random.default_rng(vf + nv)
    logits = (g.standard_normal((R, S, vf * nv)) * 2.5).astype(np.float32)
    logits[0, 0, :vf] = 1.0                                         # an all-equal factor
    uni = g.random((nv, R, S), dtype=np.float32)
    d_tok, d_uni = dev(logits), dev(uni)
    a = run_ex(c, d_tok, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(tau, k, p))
    b = run_ex(c, d_tok.permute(0, 2, 1).contiguous(), lib.LAYOUT_BCTHW, R, S, 0.8, d_uni, law_of(tau, k, p))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[0].min() >= 0 and a[0].max() < vf ** nv
    check_against_model(a[0], a[1], logits, uni, vf, tau, k, p, cap=0.05)    # (the cap of test_sample_kernel_vs_f64_softmax)


# ------------------------------------------------------------------------------------------ distribution and tempering
def one_row_draws(row, tau, k, p, seed, R=256, S=256):
    lib = pkg("_lib")
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = row.expand(R, S, 2 * VF).contiguous()
    uni = torch.rand(2, R, S, device="cuda", generator=g)
    s, conf, _ = run_ex(sample_cfg(S), logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 1.0, uni, law_of(tau, k, p))
    s = s.reshape(-1)
    return s % VF, s // VF, conf.reshape(-1)


def test_filtered_distribution():
    """65,536 draws from ONE logits row at (tau 0.7, top_k 50, top_p 0.9): per-class frequencies within 5 sigma of the f64
    filtered-tempered distribution, for both vocabularies, and no draw at all outside the kept set."""
    g = torch.Generator(device="cuda").manual_seed(11)
    row = torch.randn(2 * VF, device="cuda", generator=g) * 2.0
    lo, hi, conf = one_row_draws(row, 0.7, 50, 0.9, seed=12)
    N = lo.size
    rown = row.cpu().numpy()
    for name, draws, l in (("lo", lo, rown[:VF]), ("hi", hi, rown[VF:])):
        p, kept = SM.filtered_probs(l, 0.7, 50, 0.9)
        f = np.bincount(draws, minlength=VF) / N
        assert f[~kept].sum() == 0, (name, f[~kept].sum())
        sigma = np.sqrt(p * (1 - p) / N)
        assert (np.abs(f - p) <= 5 * sigma + 1e-9).all(), (name, (np.abs(f - p) / np.maximum(sigma, 1e-12)).max())
        assert 1 <= kept.sum() <= 50
    # confidence: the tempered UNFILTERED probabilities of the picks
    z = SM.temper(rown, 0.7).astype(np.float64)
    p_lo = np.exp(z[:VF] - z[:VF].max()); p_lo /= p_lo.sum()
    p_hi = np.exp(z[VF:] - z[VF:].max()); p_hi /= p_hi.sum()
    np.testing.assert_allclose(conf, p_hi[hi] * p_lo[lo], rtol=2e-5)


def test_tempering_is_live():
    """The user-visible gap this feature closes: `temperature` alone switches arg-max to sampling and tempers nothing, so the
    draws at 0.5, 1 and 2 used to follow one law.  With logit_temperature the empirical entropy of 65,536 draws from one row
    grows with tau."""
    g = torch.Generator(device="cuda").manual_seed(5)
    row = torch.randn(2 * VF, device="cuda", generator=g) * 2.0
    ent = []
    for tau in (0.5, 1.0, 2.0):
        lo, hi, _ = one_row_draws(row, tau, 0, 1.0, seed=6)
        h = 0.0
        for draws in (lo, hi):
            f = np.bincount(draws, minlength=VF) / draws.size
            h -= (f[f > 0] * np.log(f[f > 0])).sum()
        ent.append(h)
    print("empirical entropies (nats, both vocabularies) at tau 0.5 / 1 / 2:", ent)
    assert ent[0] < ent[1] < ent[2], ent
    assert ent[1] - ent[0] > 0.5 and ent[2] - ent[1] > 0.5, ent      # (f64 entropies of this row: a gap of > 1 nat each way)


# ------------------------------------------------------------------------------------------ "confidence" unmasking
KEY_BAR = 1.4e-5   # 10 x 1.351e-06, the largest deviation measured on an MI355X over the four cases of the test below


def test_confidence_keys_against_the_f64_formula(margin_inputs):
    """keys_out = log(conf) + c * anneal * g(noise) against the f64 formula on the f64 model's confidence, tokens whose pick is
    not ambiguous, |difference| / max(1, |key|).  Draws of exactly 0 and 1 - 2^-24 are in the input (the clamp).
    Measured on an MI355X: largest deviation 1.351e-06; the bar is 10 x that, 1.4e-05."""
    lib = pkg("_lib")
    logits, uni, d_logits, d_uni = margin_inputs
    R, S = uni.shape[1:]
    g = np.random.default_rng(29)
    noise = g.random((R, S), dtype=np.float32)
    noise[0, :8] = 0.0
    noise[0, 8:16] = np.float32(1.0 - 2.0 ** -24)
    worst = 0.0
    for (tau, k, p), c, step, steps in (((0.7, 50, 0.9), 4.5, 0, 2), ((1.0, 0, 1.0), 4.5, 0, 8), ((1.3, 8, 1.0), 1.0, 2, 4),
                                        ((1.0, 0, 1.0), 0.0, 0, 2)):
        anneal = 1.0 - (step + 1) / steps
        ids, conf, keys = run_ex(sample_cfg(S), d_logits, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(tau, k, p, c),
                                 noise=dev(noise), anneal=anneal)
        want = SM.sample(logits, uni, VF, tau, k, p)
        ok = ~want["ambiguous"] & (ids == want["ids"])
        ref = SM.confidence_keys(want["conf"], noise, c, step, steps)
        err = np.abs(keys.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err[ok].max()))
        if c == 0.0:      # the greedy order, up to the monotone log
            assert (np.diff(keys.reshape(-1)[np.argsort(conf.reshape(-1), kind="stable")]) >= 0).all()
    print(f"confidence keys: largest deviation from the f64 formula {worst:.3e} (bar {KEY_BAR:.1e})")
    assert worst < KEY_BAR, worst


def tiny_model(precision, A=0, seed=5):
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=8, S=16, num_factored_vocabs=2, qk_norm=False,
                                    use_mup=False, action_vocab_size=A)
    sd = pkg("synthetic").make_state_dict(cfg, seed=seed, law="conditioned")
    if A:
        g = np.random.default_rng(seed + 1)
        sd["action_embed.weight"] = (0.5 * g.standard_normal(sd["action_embed.weight"].shape)).astype(np.float32)
    m = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    B = 3
    ex = dev(pkg("synthetic").make_clips(B, cfg, seed=seed + 2)).view(B, cfg.T, 4, 4)
    acts = torch.randint(0, A, (B, cfg.T), device="cuda") if A else None
    return cfg, m, ex, acts


def test_choice_temperature_zero_is_the_greedy_decode():
    """c = 0: the keys are log(conf), a monotone image of the greedy keys: the same ids, exactly."""
    SC = pkg("sampling").SamplingConfig
    cfg, m, ex, _ = tiny_model("exact")
    for temperature in (0.0, 1.0):
        uni = torch.rand(3, 2, 3, cfg.S, device="cuda")
        noise = torch.rand(2, 3, cfg.S, device="cuda")
        out = []
        for mode, law in (("greedy", None), ("confidence", SC(choice_temperature=0.0)), ("greedy", SC(0.7, 20, 0.9)),
                          ("confidence", SC(0.7, 20, 0.9, 0.0))):
            p = ex.clone()
            p[:, 2:] = cfg.image_vocab_size
            s, _ = m.maskgit_generate(p, 2, maskgit_steps=3, temperature=temperature, unmask_mode=mode, noise=noise, uniforms=uni,
                                      sampling=law)
            assert int((s == cfg.image_vocab_size).sum()) == 0
            out.append(s)
        assert torch.equal(out[0], out[1]) and torch.equal(out[2], out[3])


@pytest.mark.parametrize("A", [0, 5])
@pytest.mark.parametrize("precision", ["exact", "bf16", "f16x3"])
def test_whole_loop_equals_host_loop(precision, A):
    """genie_generate_cached_ex (one library call) against the same loop driven from Python with genie_sample_ex + genie_mask_step
    (generate_frames_cached(host_loop=True)) on replayed draws: identical ids, in the "confidence" mode under a filtered law and
    under none, with and without actions.  The neutral law through the _ex entry point = the entry point of before."""
    G = pkg("generate")
    SC = pkg("sampling").SamplingConfig
    cfg, m, ex, acts = tiny_model(precision, A)
    P, steps, B = 2, 3, ex.shape[0]
    n_new = cfg.T - P
    noise = torch.rand(n_new, steps - 1, B, cfg.S, device="cuda")
    uni = torch.rand(n_new, steps, 2, B, cfg.S, device="cuda")
    for mode, law in (("confidence", SC(0.7, 20, 0.9, 4.5)), ("confidence", None), ("random", SC(1.3, 8, 1.0)), ("greedy", SC(top_p=0.8))):
        a = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, unmask_mode=mode, action_ids=acts, sampling=law, uniforms=uni)
        b = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, unmask_mode=mode, action_ids=acts, sampling=law, uniforms=uni,
                                     host_loop=True)
        assert torch.equal(a, b), (mode, law, int((a != b).sum()))
        assert int((a == cfg.image_vocab_size).sum()) == 0
    for mode in ("random", "greedy"):
        a = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, unmask_mode=mode, action_ids=acts, uniforms=uni)
        b = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, unmask_mode=mode, action_ids=acts, uniforms=uni, sampling=SC())
        assert torch.equal(a, b), mode
    # a law changes what is drawn (the filters are live in the whole loop)
    a = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, action_ids=acts, uniforms=uni)
    b = G.generate_frames_cached(m, ex, P, steps, 1.0, noise=noise, action_ids=acts, uniforms=uni, sampling=SC(top_k=1))
    c = G.generate_frames_cached(m, ex, P, steps, 0.0, noise=noise, action_ids=acts)
    assert not torch.equal(a, b) and torch.equal(b, c)          # top_k = 1 is the arg-max decode


# ------------------------------------------------------------------------------------------ module level
def test_module_paths_agree_under_a_law():
    """maskgit_generate / generate (KV cache on and off) / generate_frames / generate_frames_cached / the evaluator (both
    schedules) under one SamplingConfig with replayed draws.  Paths that run the same passes agree exactly; KV cache against full
    forward with the comparison of tests/test_hip_frame.py (first new frame > 0.995, all frames > 0.97)."""
    G = pkg("generate")
    SC = pkg("sampling").SamplingConfig
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    sd = pkg("synthetic").make_state_dict(cfg, seed=11, law="conditioned")
    m = pkg("st_mask_git").STMaskGIT(cfg, precision="f16x3").load_numpy_state_dict(sd).to("cuda")
    B, P, n_new, steps, S = 2, 14, 2, 2, cfg.S      # P + n_new = T: the full-forward schedule takes whole canvases only
    law = SC(0.7, 8, 0.9)
    clips = dev(pkg("synthetic").make_clips(B, cfg, seed=62)).view(B, cfg.T, 16, 16)
    ids = clips[:, :P].reshape(B, P * S)
    noise = torch.rand(cfg.T - P, steps - 1, B, S, device="cuda")
    uni = torch.rand(cfg.T - P, steps, 2, B, S, device="cuda")
    kw = dict(maskgit_steps=steps, temperature=1.0, sampling=law, unmask_mode="confidence")
    a = m.generate(ids, None, max_new_tokens=n_new * S, noise=noise[:n_new], uniforms=uni[:n_new], kv_cache=True, **kw)
    b = m.generate(ids, None, max_new_tokens=n_new * S, noise=noise[:n_new], uniforms=uni[:n_new], kv_cache=False, **kw)
    first = a[:, P * S:(P + 1) * S] == b[:, P * S:(P + 1) * S]
    assert first.float().mean().item() > 0.995
    assert (a == b).float().mean().item() > 0.97
    # the harness functions: cached whole loop = generate(kv_cache=True); full forward = generate(kv_cache=False), frame by frame
    fc = G.generate_frames_cached(m, clips, P, steps, 1.0, noise=noise, unmask_mode="confidence", sampling=law, uniforms=uni)
    ff = G.generate_frames(m, clips, P, steps, 1.0, noise=noise, unmask_mode="confidence", sampling=law, uniforms=uni)
    assert torch.equal(fc[:, :P + n_new].reshape(B, -1), a)
    assert torch.equal(ff[:, :P + n_new].reshape(B, -1), b)
    # maskgit_generate on the canvas = the first new frame of the full-forward schedule
    canvas = clips.clone()
    canvas[:, P:] = cfg.image_vocab_size
    s, _ = m.maskgit_generate(canvas, P, maskgit_steps=steps, temperature=1.0, unmask_mode="confidence", noise=noise[0], uniforms=uni[0],
                              sampling=law)
    assert torch.equal(s.reshape(B, S), b[:, P * S:(P + 1) * S])
    # the evaluator reads the law from its args; arg-max decode so that the two schedules need no shared uniforms
    E = pkg("evaluate")
    args = SimpleNamespace(maskgit_steps=steps, temperature=0.0, latent_h=16, latent_w=16, logit_temperature=0.7, top_k=8, top_p=0.9,
                           unmask_mode="confidence", choice_temperature=4.5)
    ev = E.GenieEvaluator(args, None, "cuda", model=m)
    en = torch.rand(cfg.T - 1, steps - 1, B, S, device="cuda")
    s_full, _ = ev.predict_zframe_logits(clips.view(B, -1), noise=en, return_logits=False)
    s_reuse, _ = ev.predict_zframe_logits_reuse(clips.view(B, -1), noise=en, return_logits=False)
    assert (s_full == s_reuse).float().mean().item() > 0.97
    plain = E.GenieEvaluator(SimpleNamespace(maskgit_steps=steps, temperature=0.0, latent_h=16, latent_w=16), None, "cuda", model=m)
    s_plain, _ = plain.predict_zframe_logits_reuse(clips.view(B, -1), noise=en, return_logits=False)
    assert not torch.equal(s_plain, s_reuse)                      # (confidence keys re-mask other tokens than random draws)
    # with sampling: the evaluator's reuse path on replayed uniforms = maskgit_generate frame by frame at the first timeline
    args.temperature = 1.0
    eu = torch.rand(steps, 2, B * (cfg.T - 1), S, device="cuda")
    s_r, _ = ev.predict_zframe_logits_reuse(clips.view(B, -1), noise=en, return_logits=False, uniforms=eu)
    tl = clips.clone()
    tl[:, 1:] = cfg.image_vocab_size
    u1 = eu.view(steps, 2, B, cfg.T - 1, S)[:, :, :, 0].contiguous()
    s_1, _ = m.maskgit_generate(tl, 1, maskgit_steps=steps, temperature=1.0, unmask_mode="confidence", noise=en[0], uniforms=u1,
                                sampling=law, check=False)
    assert (s_r[:, 0] == s_1).float().mean().item() > 0.97
