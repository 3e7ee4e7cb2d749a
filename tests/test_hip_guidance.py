"""Classifier-free guidance on the GPU (genie_guidance: csrc/kernels_sample.hip through genie_sample_guided / genie_guide_logits, the
*_guided generate entry points and the guidance= keyword of the module): the identities at scale 1 and 0, the guided kernels draw by
draw against the f64 model on logits combined in NumPy f32, the whole loop against the host loop, the null stream against an unguided
run on the hand-built doubled batch, the step-0 logits against two forwards combined in torch, the module paths against each other,
argument errors, and the training side of the null action.  Needs a real MI355X: run with ``-m gpu``."""
import numpy as np
import pytest

import sampling_model as SM
from conftest import pkg
from test_hip_sampling import (OFF, VF, check_against_model, dev, law_of, run_ex, sample_cfg, stream, tie_inputs, tiny_model)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NULL = 4    # the null action of the tiny action models (A = 5)
# logits of one clip differ between a batch of B and a batch of 2 B by at most this (f32 paths):
# tests/test_hip_actions.py::test_batch_of_clips_with_their_own_actions, BATCH_TOL["exact"]
BATCH_TOL_EXACT = 2e-5


def guide_np(c, u, w):
    """g = (w * c) + ((1.0f - w) * u): three separately rounded f32 operations."""
    w32 = np.float32(w)
    omw = np.float32(1.0) - w32
    return ((w32 * c).astype(np.float32) + (omw * u).astype(np.float32)).astype(np.float32)


def run_guided(c, lc, lu, layout, R, S, temperature, uni, law, scale, noise=None, anneal=0.0):
    """genie_sample_guided -> (samples, conf, keys or None) as numpy."""
    lib = pkg("_lib")
    L = lib.load()
    samples = torch.full((R, S), -1, dtype=torch.int64, device="cuda")
    conf = torch.full((R, S), -1.0, dtype=torch.float32, device="cuda")
    keys = torch.full((R, S), -7.0, dtype=torch.float32, device="cuda") if noise is not None else None
    lib.check(L.genie_sample_guided(c, lc.data_ptr(), lu.data_ptr(), layout, R, temperature, 0 if uni is None else uni.data_ptr(),
                                    samples.data_ptr(), conf.data_ptr(), stream(), law, 0 if keys is None else keys.data_ptr(),
                                    0 if noise is None else noise.data_ptr(), anneal, scale), "genie_sample_guided")
    return samples.cpu().numpy(), conf.cpu().numpy(), None if keys is None else keys.cpu().numpy()


def same_bits(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert (a[2] is None) == (b[2] is None)
    if a[2] is not None:
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


# ------------------------------------------------------------------------------------------ 1. kernel identities
@pytest.mark.parametrize("temperature", [0.0, 0.8])
@pytest.mark.parametrize("law", [OFF, (0.7, 50, 0.9)])
def test_scale_one_is_the_conditional_and_scale_zero_the_null_stream(law, temperature):
    """genie_sample_guided at scale 1 = genie_sample_ex on the conditional logits, at scale 0 = genie_sample_ex on the null logits:
    samples, bits of conf and of the keys; 2 x 512, S = 256, 9 rows with tie blocks in both tensors; with the keys (the filtered
    kernels under every law) and without them under no law at all (genie_sample's kernels), token-major and (B, V, S)."""
    lib = pkg("_lib")
    R, S = 9, 256
    c = sample_cfg(S)
    lc, uni = tie_inputs()
    lu, _ = tie_inputs(seed=24)
    lu[3, :, 50:90] = 1.5      # a tie block of the null logits alone
    noise = torch.rand(R, S, device="cuda")
    d_uni = dev(uni)
    for layout, dc, du in ((lib.LAYOUT_TOKEN_MAJOR, dev(lc), dev(lu)),
                           (lib.LAYOUT_BCTHW, dev(lc).permute(0, 2, 1).contiguous(), dev(lu).permute(0, 2, 1).contiguous())):
        for sp, nz in ((law_of(*law), noise), (law_of(*law), None), (None, None)):
            for scale, ref in ((1.0, dc), (0.0, du)):
                got = run_guided(c, dc, du, layout, R, S, temperature, d_uni, sp, scale, noise=nz, anneal=0.5)
                want = run_ex(c, ref, layout, R, S, temperature, d_uni, sp, noise=nz, anneal=0.5)
                same_bits(got, want)


# ------------------------------------------------------------------------------------------ 2. against the f64 model
LAW = (0.7, 50, 0.9)


@pytest.fixture(scope="module")
def guided_margin_inputs():
    """Conditional and null logits drawn like margin_inputs of tests/test_hip_sampling.py (8 rows: the model is f64 over 1,024 entries)."""
    g = np.random.default_rng(17)
    R, S = 8, 256
    lc = (g.standard_normal((R, S, 2 * VF)) * 2.5).astype(np.float32)
    lu = (g.standard_normal((R, S, 2 * VF)) * 2.5).astype(np.float32)
    uni = g.random((2, R, S), dtype=np.float32)
    return lc, lu, uni, dev(lc), dev(lu), dev(uni)


@pytest.mark.parametrize("w", [3.0, -0.5, 0.25])
def test_guided_draws_equal_the_f64_model_on_numpy_guided_logits(guided_margin_inputs, w):
    """g formed in NumPy f32 with the three roundings, handed to the f64 model: picks equal outside the ambiguous set (< 1 %), no
    filtered-out id anywhere, confidence at rtol 2e-5 -- check_against_model of tests/test_hip_sampling.py -- and the strided kernel
    on the (B, V, S) layout gives the row kernel's bits."""
    lib = pkg("_lib")
    lc, lu, uni, d_lc, d_lu, d_uni = guided_margin_inputs
    R, S = uni.shape[1:]
    g = guide_np(lc, lu, w)
    c = sample_cfg(S)
    noise = torch.rand(R, S, device="cuda")
    a = run_guided(c, d_lc, d_lu, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(*LAW), w, noise=noise, anneal=0.5)
    check_against_model(a[0], a[1], g, uni, VF, *LAW, cap=0.01)
    b = run_guided(c, d_lc.permute(0, 2, 1).contiguous(), d_lu.permute(0, 2, 1).contiguous(), lib.LAYOUT_BCTHW, R, S, 0.8, d_uni,
                   law_of(*LAW), w, noise=noise, anneal=0.5)
    same_bits(a, b)
    # arg-max decode: exactly the arg-max of the NumPy guided logits, first maximum wins
    s0, c0, _ = run_guided(c, d_lc, d_lu, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.0, None, law_of(*LAW), w)
    want = SM.sample(g, uni, VF, *LAW, temperature=0.0)
    assert np.array_equal(s0, want["ids"])
    np.testing.assert_allclose(c0, want["conf"], rtol=2e-5)


@pytest.mark.parametrize("vf,nv,tau,k,p", [(100, 2, 1.3, 20, 0.9), (64, 3, 0.7, 8, 0.8)])
@pytest.mark.parametrize("w", [3.0, -0.5, 0.25])
def test_other_vocabularies_take_the_strided_guided_kernel(vf, nv, tau, k, p, w):
    """Vocabularies other than 2 x 512 in the (B, V, S) layout: the strided flavour, against the f64 model (the cap of
    test_other_vocabularies_against_the_f64_model), and equal to the token-major run of the same kernel."""
    lib = pkg("_lib")
    R, S = 8, 64
    c = sample_cfg(S, image_vocab_size=vf ** nv, nv=nv)
    g = np.random.default_rng(vf + nv)
    lc = (g.standard_normal((R, S, vf * nv)) * 2.5).astype(np.float32)
    lu = (g.standard_normal((R, S, vf * nv)) * 2.5).astype(np.float32)
    lc[0, 0, :vf] = 1.0
    lu[0, 0, :vf] = -2.0                                           # an all-equal guided factor
    uni = g.random((nv, R, S), dtype=np.float32)
    d_lc, d_lu, d_uni = dev(lc), dev(lu), dev(uni)
    b = run_guided(c, d_lc.permute(0, 2, 1).contiguous(), d_lu.permute(0, 2, 1).contiguous(), lib.LAYOUT_BCTHW, R, S, 0.8, d_uni,
                   law_of(tau, k, p), w)
    a = run_guided(c, d_lc, d_lu, lib.LAYOUT_TOKEN_MAJOR, R, S, 0.8, d_uni, law_of(tau, k, p), w)
    same_bits(a, b)
    assert b[0].min() >= 0 and b[0].max() < vf ** nv
    check_against_model(b[0], b[1], guide_np(lc, lu, w), uni, vf, tau, k, p, cap=0.05)


# ------------------------------------------------------------------------------------------ 3. genie_guide_logits
@pytest.mark.parametrize("w", [3.0, -0.5, 0.25, 1.0, 0.0])
def test_guide_logits_equals_the_numpy_formula_bit_for_bit(w):
    lib = pkg("_lib")
    L = lib.load()
    n = 70001          # not a multiple of the block (256); more than one block
    g = np.random.default_rng(3)
    c = (g.standard_normal(n) * 4).astype(np.float32)
    u = (g.standard_normal(n) * 4).astype(np.float32)
    c[:4] = [0.0, -0.0, 1e-38, -3e38]
    d_c, d_u = dev(c), dev(u)
    out = torch.full((n + 8,), 123.0, device="cuda")
    lib.check(L.genie_guide_logits(d_c.data_ptr(), d_u.data_ptr(), out.data_ptr(), n, w, stream()), "genie_guide_logits")
    got = out.cpu().numpy()
    with np.errstate(over="ignore"):
        want = guide_np(c, u, w)
    assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32))
    assert (got[n:] == 123.0).all()


# ------------------------------------------------------------------------------------------ 4. whole loop = host loop
@pytest.mark.parametrize("precision", ["exact", "bf16", "f16x3"])
def test_guided_whole_loop_equals_the_host_loop(precision):
    """genie_generate_cached_guided (one library call: the library doubles tokens and actions itself) against the loop driven from
    Python at 2 B (genie_frame_pass_cond, genie_sample_guided, genie_mask_step, the mirror): identical ids.  B = 3, P = 2, two new
    frames, 3 steps, w = 3; merge_commit on and off; random and confidence unmasking on replayed draws; teacher forcing in time."""
    G = pkg("generate")
    S_ = pkg("sampling")
    cfg, m, ex, acts = tiny_model(precision, A=5)
    P, n_new, steps, B = 2, 2, 3, ex.shape[0]
    clip, a = ex[:, :P + n_new].contiguous(), acts[:, :P + n_new].contiguous()
    noise = torch.rand(n_new, steps - 1, B, cfg.S, device="cuda")
    uni = torch.rand(n_new, steps, 2, B, cfg.S, device="cuda")
    guide = S_.Guidance(3.0, NULL)
    for mode, law in (("random", None), ("confidence", S_.SamplingConfig(0.7, 20, 0.9, 4.5)), ("confidence", None)):
        for merge in (True, False):
            for tf in (False, True):
                kw = dict(noise=noise, unmask_mode=mode, action_ids=a, sampling=law, uniforms=uni, guidance=guide, merge_commit=merge,
                          teacher_force_time=tf)
                one = G.generate_frames_cached(m, clip, P, steps, 1.0, **kw)
                host = G.generate_frames_cached(m, clip, P, steps, 1.0, host_loop=True, **kw)
                assert torch.equal(one, host), (mode, law, merge, tf, int((one != host).sum()))
                assert int((one == cfg.image_vocab_size).sum()) == 0


# ------------------------------------------------------------------------------------------ 5. the null stream
@pytest.mark.parametrize("precision", ["exact", "bf16", "f16x3"])
def test_scale_zero_is_the_null_half_of_the_doubled_batch(precision):
    """scale 0 decodes from the null stream alone.  An UNGUIDED run on the hand-built doubled batch (tokens twice, actions
    [a ; null], noise and uniforms twice) runs the same kernels at the same batch size on the same rows [B, 2B): the guided output
    equals those rows bit for bit."""
    G = pkg("generate")
    cfg, m, ex, acts = tiny_model(precision, A=5)
    P, n_new, steps, B = 2, 2, 3, ex.shape[0]
    clip, a = ex[:, :P + n_new].contiguous(), acts[:, :P + n_new].contiguous()
    noise = torch.rand(n_new, steps - 1, B, cfg.S, device="cuda")
    uni = torch.rand(n_new, steps, 2, B, cfg.S, device="cuda")
    for temperature in (0.0, 1.0):
        for host in (False, True):
            got = G.generate_frames_cached(m, clip, P, steps, temperature, noise=noise, action_ids=a, uniforms=uni, host_loop=host,
                                           guidance=pkg("sampling").Guidance(0.0, NULL))
            ref = G.generate_frames_cached(m, torch.cat([clip, clip]), P, steps, temperature, noise=torch.cat([noise, noise], dim=2),
                                           action_ids=torch.cat([a, torch.full_like(a, NULL)]), uniforms=torch.cat([uni, uni], dim=3),
                                           host_loop=host)
            assert torch.equal(got, ref[B:]), (temperature, host, int((got != ref[B:]).sum()))


# ------------------------------------------------------------------------------------------ 6. an independent composition
@pytest.mark.parametrize("w", [3.0, -0.5])
def test_step0_logits_against_two_forwards_combined_in_torch(w):
    """maskgit_generate(guidance) in `exact`, one step, arg-max: the returned step-0 logits against compute_logits_frames called twice
    at batch B (the clip's actions; all-null actions) and combined in torch with three separate operations.  The forwards of the
    guided call run at batch 2 B; a clip's logits may differ between batch sizes by the bound of
    tests/test_hip_actions.py::test_batch_of_clips_with_their_own_actions (2e-5 in `exact`), so the guided logits by
    (|w| + |1 - w|) times that.  Sampled ids are equal wherever the top-2 gap of the composed logits exceeds that bound."""
    cfg, m, ex, acts = tiny_model("exact", A=5)
    B, t = ex.shape[0], 3
    p = ex.clone()
    p[:, t:] = cfg.image_vocab_size
    lc = m.compute_logits_frames(p, t, t + 1, "bcthw", action_ids=acts)[:, :, 0]            # (B, V, H, W)
    lu = m.compute_logits_frames(p, t, t + 1, "bcthw", action_ids=torch.full_like(acts, NULL))[:, :, 0]
    wt = torch.tensor(w, dtype=torch.float32, device="cuda")
    a = wt * lc
    b = (1.0 - wt) * lu
    want = (a + b).view(B, 2, VF, 4, 4).permute(0, 2, 1, 3, 4)                                # (B, vf, nv, H, W)
    s, got = m.maskgit_generate(p, t, maskgit_steps=1, temperature=0.0, action_ids=acts, guidance=pkg("sampling").Guidance(w, NULL))
    bound = (abs(w) + abs(1.0 - w)) * BATCH_TOL_EXACT
    err = float((got - want).abs().max())
    print(f"w = {w}: guided step-0 logits vs the composition: max |diff| {err:.3e} (bound {bound:.1e})")
    assert err <= bound, err
    top2 = want.topk(2, dim=1).values                                                         # (B, 2, nv, H, W)
    clear = ((top2[:, 0] - top2[:, 1]) > bound).all(1)                                        # both factors
    ids = want.argmax(1)                                                                      # (B, nv, H, W): [lo, hi]
    want_ids = ids[:, 1] * VF + ids[:, 0]
    assert clear.float().mean().item() > 0.9
    assert torch.equal(s[clear], want_ids[clear])
    assert torch.equal(p[:, t], s)                                                            # written in place, as without guidance


# ------------------------------------------------------------------------------------------ 7. live, and the module paths
def test_guidance_is_live_and_the_module_paths_agree():
    """w = 3 and w = 1 decode different ids on a model whose action table matters; under guidance generate (KV cache on / off),
    generate_frames and generate_frames_cached agree by the criteria of test_module_paths_agree_under_a_law: paths that run the same
    passes exactly, KV cache against full forward first new frame > 0.995, all frames > 0.97."""
    G = pkg("generate")
    S_ = pkg("sampling")
    A = 5
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False,
                                    use_mup=False, action_vocab_size=A)
    sd = pkg("synthetic").make_state_dict(cfg, seed=11, law="conditioned")
    sd["action_embed.weight"] = (0.5 * np.random.default_rng(12).standard_normal((A, cfg.d_model))).astype(np.float32)
    m = pkg("st_mask_git").STMaskGIT(cfg, precision="f16x3").load_numpy_state_dict(sd).to("cuda")
    B, P, n_new, steps, S = 2, 14, 2, 2, cfg.S
    clips = dev(pkg("synthetic").make_clips(B, cfg, seed=62)).view(B, cfg.T, 16, 16)
    acts = torch.randint(0, NULL, (B, cfg.T), device="cuda")
    ids = clips[:, :P].reshape(B, P * S)
    noise = torch.rand(n_new, steps - 1, B, S, device="cuda")
    uni = torch.rand(n_new, steps, 2, B, S, device="cuda")
    guide = S_.Guidance(3.0, NULL)
    kw = dict(maskgit_steps=steps, temperature=1.0, sampling=S_.SamplingConfig(0.7, 8, 0.9), unmask_mode="confidence", action_ids=acts,
              noise=noise, uniforms=uni)
    a = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=True, guidance=guide, **kw)
    b = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=False, guidance=guide, **kw)
    first = a[:, P * S:(P + 1) * S] == b[:, P * S:(P + 1) * S]
    assert first.float().mean().item() > 0.995
    assert (a == b).float().mean().item() > 0.97
    hk = dict(kw)
    del hk["maskgit_steps"], hk["temperature"]
    fc = G.generate_frames_cached(m, clips, P, steps, 1.0, guidance=guide, **hk)
    ff = G.generate_frames(m, clips, P, steps, 1.0, guidance=guide, **hk)
    assert torch.equal(fc[:, :P + n_new].reshape(B, -1), a)
    assert torch.equal(ff[:, :P + n_new].reshape(B, -1), b)
    # scale 1 is the unguided call, and guidance changes what is decoded
    plain = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=True, **kw)
    one = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=True, guidance=S_.Guidance(1.0, NULL), **kw)
    assert torch.equal(plain, one)
    assert not torch.equal(plain, a)
    # ... with return_logits: the guided step-0 logits, (B, vf, nv, n_new, H, W)
    _, lg = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=True, guidance=guide, return_logits=True, **kw)
    _, lp = m.generate(ids, None, max_new_tokens=n_new * S, kv_cache=True, return_logits=True, **kw)
    assert lg.shape == lp.shape and not torch.equal(lg, lp)


# ------------------------------------------------------------------------------------------ 8. errors
def test_errors_before_anything_is_enqueued():
    lib = pkg("_lib")
    L = lib.load()
    G = pkg("generate")
    S_ = pkg("sampling")
    cfg, m, ex, acts = tiny_model("exact", A=5)
    _, m0, _, _ = tiny_model("exact", A=0)
    with pytest.raises(ValueError):
        S_.Guidance(float("nan"), NULL)
    with pytest.raises(ValueError):
        G.generate_frames_cached(m0, ex, 2, 2, guidance=S_.Guidance(3.0, 0))             # a model without actions
    with pytest.raises(IndexError):
        G.generate_frames_cached(m, ex, 2, 2, action_ids=acts, guidance=S_.Guidance(3.0, 5))
    with pytest.raises(ValueError):
        G.generate_frames_cached(m, ex, 2, 2, guidance=S_.Guidance(3.0, NULL))           # guidance without the actions
    p = ex.clone()
    p[:, 2:] = cfg.image_vocab_size
    before = p.clone()
    with pytest.raises(IndexError):
        m.maskgit_generate(p, 2, action_ids=acts, guidance=S_.Guidance(3.0, 7))
    assert torch.equal(p, before)
    # the C entry point itself, on real buffers: GENIE_E_ARG and the outputs untouched
    c, w = m._weights()[:2]
    B, P, n_new = ex.shape[0], 2, 2
    ids = ex.view(B, cfg.T, cfg.S)[:, :P + n_new].contiguous()
    gen = torch.full((B, n_new, cfg.S), -1, dtype=torch.int64, device="cuda")
    nb = L.genie_prefix_cache_bytes(c, 2 * B)
    cache = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.genie_generate_guided_workspace_bytes(c, B, P), dtype=torch.uint8, device="cuda")
    cond = m._cond(acts, B)
    for cd, g in ((None, lib.Guidance(3.0, NULL)), (cond, lib.Guidance(3.0, 5)), (cond, lib.Guidance(float("nan"), NULL))):
        rc = L.genie_generate_cached_guided(c, w, ids.data_ptr(), B, P, n_new, 1, 0.0, lib.UNMASK_RANDOM, None, None, 0, 1,
                                            gen.data_ptr(), None, cache.data_ptr(), nb, ws.data_ptr(), ws.numel(), stream(), cd, None, g)
        assert rc == lib.E_ARG and b"guidance" in L.genie_last_error()
    torch.cuda.synchronize()
    assert bool((gen == -1).all())
    # a workspace sized for the unguided loop is refused, not overrun
    small = torch.empty(L.genie_generate_workspace_bytes(c, B, P), dtype=torch.uint8, device="cuda")
    rc = L.genie_generate_cached_guided(c, w, ids.data_ptr(), B, P, n_new, 1, 0.0, lib.UNMASK_RANDOM, None, None, 0, 1, gen.data_ptr(),
                                        None, cache.data_ptr(), nb, small.data_ptr(), small.numel(), stream(), cond, None,
                                        lib.Guidance(3.0, NULL))
    assert rc == lib.E_ARG and b"workspace" in L.genie_last_error()


# ------------------------------------------------------------------------------------------ 9. training the null action
def test_action_dropout_trains_the_null_row_alone():
    """One GenieTrainer.train_step in `exact`, weight_decay 0, on a batch collated with action_dropout = 1: only row null_action of
    the action table changes, and its gradient is that of the same batch with the ids replaced by hand.  All B T frames carry one
    action: they land on one workgroup of action_bwd_kernel (its longest sum)."""
    import random
    D = pkg("data")
    A = 5
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False,
                                    use_mup=False, num_prompt_frames=2, action_vocab_size=A)
    sd = pkg("synthetic").make_state_dict(cfg, seed=31)
    sd["action_embed.weight"] = (0.5 * np.random.default_rng(9).standard_normal((A, cfg.d_model))).astype(np.float32)
    B = 6
    clips = dev(pkg("synthetic").make_clips(B, cfg, seed=32))
    acts = torch.randint(0, A, (B, cfg.T), device="cuda")
    torch.manual_seed(3)
    random.seed(3)
    batch = D.maskgit_collate(clips, cfg, action_ids=acts, action_dropout=1.0, null_action=NULL)
    assert bool((batch["action_ids"] == NULL).all())

    def trainer():
        m = pkg("st_mask_git").STMaskGIT(cfg, precision="exact").load_numpy_state_dict(sd).to("cuda")
        return pkg("train").GenieTrainer(m, lr=1e-2, weight_decay=0.0)

    tr = trainer()
    table0 = torch.from_numpy(sd["action_embed.weight"]).cuda()
    tr.train_step(batch)
    g = tr.gradients()["action_embed.weight"].clone()
    table1 = tr.model.action_embed.weight.detach()
    others = [k for k in range(A) if k != NULL]
    assert torch.equal(table1[others], table0[others])
    assert not torch.equal(table1[NULL], table0[NULL])
    assert bool((g[others] == 0).all()) and float(g[NULL].abs().max()) > 0
    by_hand = trainer()
    by_hand.forward_backward(batch["input_ids"], batch["labels"], action_ids=torch.full((B, cfg.T), NULL, device="cuda"))
    assert torch.equal(by_hand.gradients()["action_embed.weight"], g)
