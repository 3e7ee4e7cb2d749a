"""GPU tests of the rollout past the context window (genie_rollout_cached, generate.rollout_frames, generate.Rollout).

The oracle of every test is a composition of calls that exist without the rollout: a rollout of N frames equals, in token ids, bit for
bit, chaining generate_frames_cached (the whole-loop library call) window by window -- first the P prompt frames and min(T - P, N) new
ones, then the last `keep` frames as the prompt of min(hop, remaining) new ones --, each call with its window's slice of actions,
noise and uniforms (include/genie_hip.h, "rollout past the context window").  All draws are fixed tensors."""
import functools

import pytest

from conftest import pkg
from test_hip_sampling import dev, tiny_model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 2


@functools.lru_cache(maxsize=None)
def model(precision, A=0):
    return tiny_model(precision, A)          # cfg, model, clips (3, 8, 4, 4), actions: L 2, H 2, d 64, T 8, S 16, B 3


@functools.lru_cache(maxsize=None)
def fragment_model():
    """The d_model 128 f16x3 model of test_hip_sampling.test_module_paths_agree_under_a_law: the fragment-order kernels cover it."""
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    sd = pkg("synthetic").make_state_dict(cfg, seed=11, law="conditioned")
    m = pkg("st_mask_git").STMaskGIT(cfg, precision="f16x3").load_numpy_state_dict(sd).to("cuda")
    clips = dev(pkg("synthetic").make_clips(2, cfg, seed=62)).view(2, cfg.T, 16, 16)
    return cfg, m, clips


def draws(cfg, N, B, steps=STEPS, seed=3):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(N, steps - 1, B, cfg.S, generator=g).cuda()
    uni = torch.rand(N, steps, cfg.num_factored_vocabs, B, cfg.S, generator=g).cuda()
    return noise, uni


def chain(m, prompt, N, keep, noise, uni, temperature, steps=STEPS, actions=None, **kw):
    """The oracle: today's whole-loop call, window by window, written without the schedule helper of the code under test."""
    G = pkg("generate")
    T, B, P = m.config.T, prompt.shape[0], prompt.shape[1]
    hop = T - keep
    frames = prompt.clone()
    done = 0
    while done < N:
        ctx = P if done == 0 else keep
        n = min(T - P if done == 0 else hop, N - done)
        have = frames.shape[1]
        ex = torch.cat([frames[:, have - ctx:], torch.full((B, n) + tuple(prompt.shape[2:]), m.mask_token_id, dtype=torch.int64, device="cuda")], 1)
        out = G.generate_frames_cached(m, ex, ctx, steps, temperature, noise=noise[done:done + n], uniforms=uni[done:done + n].contiguous(),
                                       action_ids=None if actions is None else actions[:, have - ctx:have + n].contiguous(), **kw)
        frames = torch.cat([frames, out[:, ctx:ctx + n]], 1)
        done += n
    return frames


def check(a, b, cfg):
    assert a.shape == b.shape
    assert int((a == cfg.image_vocab_size).sum()) == 0 and int((a < 0).sum()) == 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} ids differ, first frame {int((a != b).flatten(2).any(2).any(0).nonzero()[0])}"


def mode_kw(mode):
    return dict(unmask_mode=mode, sampling=pkg("sampling").SamplingConfig(0.7, 8, 0.9) if mode == "confidence" else None)


# ------------------------------------------------------------------ 1-3: rollout = chained windows
@pytest.mark.parametrize("mode", ["random", "greedy", "confidence"])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_rollout_equals_chained_windows(precision, temperature, mode):
    """P = 3, keep = 2, N = 15 on T = 8: windows of 5, 6 and 4 frames, the last one partial."""
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    P, keep, N = 3, 2, 15
    noise, uni = draws(cfg, N, ex.shape[0])
    got = G.rollout_frames(m, ex[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=temperature, noise=noise, uniforms=uni, **mode_kw(mode))
    assert got.shape == (3, P + N, 4, 4) and torch.equal(got[:, :P], ex[:, :P])
    check(got, chain(m, ex[:, :P], N, keep, noise, uni, temperature, **mode_kw(mode)), cfg)


@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_hop_of_one_and_the_model_method(precision):
    """keep = 7, N = 4 behind 7 prompt frames: every frame is its own window (the true sliding window)."""
    cfg, m, ex, _ = model(precision)
    P, keep, N = 7, 7, 4
    noise, uni = draws(cfg, N, ex.shape[0], seed=4)
    got = m.rollout(ex[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni)
    check(got, chain(m, ex[:, :P], N, keep, noise, uni, 1.0), cfg)
    # three MaskGIT steps, keep by default = P, merge_commit off
    noise, uni = draws(cfg, 9, ex.shape[0], steps=3, seed=5)
    got = m.rollout(ex[:, :3], 9, maskgit_steps=3, temperature=1.0, noise=noise, uniforms=uni, merge_commit=False)
    check(got, chain(m, ex[:, :3], 9, 3, noise, uni, 1.0, steps=3, merge_commit=False), cfg)


@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_in_window_rollout_is_generate_frames_cached(precision):
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    P = 3
    N = cfg.T - P
    noise, uni = draws(cfg, N, ex.shape[0], seed=6)
    got = G.rollout_frames(m, ex[:, :P], N, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni)
    want = G.generate_frames_cached(m, ex, P, STEPS, 1.0, noise=noise, uniforms=uni)[:, :cfg.T]
    check(got, want, cfg)


# ------------------------------------------------------------------ 4: the fragment-order kernels
def test_fragment_order_path_equals_chained_windows():
    """d_model 128, T 16, S 256, B 2 in f16x3; P = 14, keep = 13, N = 7: windows of 2, 3 and 2 frames.  B * keep * S = 6,656 rows, under
    the 16,384-row cut: the context runs as one multi-frame pass and the commits are merged with the next frame's step 0."""
    G = pkg("generate")
    cfg, m, clips = fragment_model()
    P, keep, N = 14, 13, 7
    noise, uni = draws(cfg, N, 2, seed=7)
    kw = dict(unmask_mode="confidence", sampling=pkg("sampling").SamplingConfig(0.7, 8, 0.9))
    got = G.rollout_frames(m, clips[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni, **kw)
    check(got, chain(m, clips[:, :P], N, keep, noise, uni, 1.0, **kw), cfg)
    r = G.Rollout(m, clips[:, :P], keep=keep, maskgit_steps=STEPS, temperature=1.0, **kw)
    for k in (1, 2, 1, 3):                       # resumed calls: the merged commit of the pending frame opens frames 15, 17 and 18
        r.extend(k, noise=noise[r.n - P:r.n - P + k], uniforms=uni[r.n - P:r.n - P + k])
    check(r.frames, got, cfg)


# ------------------------------------------------------------------ 5: actions and guidance
@pytest.mark.parametrize("guided", [False, True])
def test_actions_of_the_absolute_frames_and_guidance(guided):
    G = pkg("generate")
    cfg, m, ex, _ = model("exact", 5)
    P, keep, N, B = 3, 2, 15, ex.shape[0]
    acts = torch.randint(0, 4, (B, P + N), generator=torch.Generator().manual_seed(9)).cuda()
    noise, uni = draws(cfg, N, B, seed=8)
    kw = dict(guidance=pkg("sampling").Guidance(3.0, 4)) if guided else {}
    got = G.rollout_frames(m, ex[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni, action_ids=acts, **kw)
    check(got, chain(m, ex[:, :P], N, keep, noise, uni, 1.0, actions=acts, **kw), cfg)
    # the actions of frames >= T reach no frame < T, and do reach later ones
    other = acts.clone()
    other[:, cfg.T:] = acts[:, cfg.T:].flip(1)            # a permutation of the actions of frames >= T
    assert not torch.equal(other, acts)
    got2 = G.rollout_frames(m, ex[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni, action_ids=other, **kw)
    assert torch.equal(got2[:, :cfg.T], got[:, :cfg.T])
    assert not torch.equal(got2[:, cfg.T:], got[:, cfg.T:])
    # the step API takes the same actions frame by frame
    r = G.Rollout(m, ex[:, :P], keep=keep, prompt_actions=acts[:, :P], maskgit_steps=STEPS, temperature=1.0, **kw)
    for k in range(N):
        r.step(acts[:, P + k], noise=noise[k], uniforms=uni[k])
    check(r.frames, got, cfg)


# ------------------------------------------------------------------ 6: resumable
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_split_calls_resume_one_cache(precision):
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    P, keep, N, B = 3, 2, 15, ex.shape[0]
    noise, uni = draws(cfg, N, B, seed=10)
    kw = dict(maskgit_steps=STEPS, temperature=1.0)
    one = G.rollout_frames(m, ex[:, :P], N, keep=keep, noise=noise, uniforms=uni, **kw)
    # raw calls of 1, 1, 4, 2 and 7 frames with resume = 1 on one cache (two of them cross a window boundary)
    dec = G._Decode(m, STEPS, 1.0, "random", None, None, True)
    frames = torch.full((B, P + N, cfg.S), cfg.image_vocab_size, dtype=torch.int64, device="cuda")
    frames[:, :P] = ex[:, :P].reshape(B, P, cfg.S)
    cache = G._rollout_cache(m, B, dec, "cuda")
    f = P
    for n in (1, 1, 4, 2, 7):
        G.rollout_call(m, frames, None, P, keep, f, f + n, int(f > P), cache, dec, noise[f - P:f - P + n].contiguous(),
                       uni[f - P:f - P + n].contiguous())
        f += n
    check(frames.view_as(one), one, cfg)
    # the step API: 15 steps, and one extend of 15
    r = G.Rollout(m, ex[:, :P], keep=keep, **kw)
    for k in range(N):
        fr = r.step(noise=noise[k], uniforms=uni[k])
        assert fr.shape == (B, 4, 4) and r.frames.shape[1] == P + k + 1
    check(r.frames, one, cfg)
    r = G.Rollout(m, ex[:, :P], keep=keep, **kw)
    new = r.extend(N, noise=noise, uniforms=uni)
    check(new, one[:, P:], cfg)
    check(r.frames, one, cfg)


def test_fresh_call_in_mid_window_is_generate_on_that_window():
    """resume = 0 at f0 = 10 (window 1 starts at frame 6, slot 4): the context [6, 10) is run from the buffer, as generate_frames_cached
    does with four prompt frames."""
    G = pkg("generate")
    cfg, m, ex, _ = model("exact")
    P, keep, N, B = 3, 2, 15, ex.shape[0]
    noise, uni = draws(cfg, N, B, seed=11)
    one = G.rollout_frames(m, ex[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni)
    f0, f1, start = 10, 14, 6
    assert G.frame_window(f0, P, keep, cfg.T) == (1, start, 4)
    dec = G._Decode(m, STEPS, 1.0, "random", None, None, True)
    frames = one.reshape(B, P + N, cfg.S).clone()
    frames[:, f0:] = -1
    G.rollout_call(m, frames, None, P, keep, f0, f1, 0, G._rollout_cache(m, B, dec, "cuda"), dec, noise[f0 - P:f1 - P].contiguous(),
                   uni[f0 - P:f1 - P].contiguous())
    want = G.generate_frames_cached(m, one[:, start:f1], f0 - start, STEPS, 1.0, noise=noise[f0 - P:f1 - P], uniforms=uni[f0 - P:f1 - P].contiguous())
    check(frames[:, f0:f1].view(B, f1 - f0, 4, 4), want[:, f0 - start:f1 - start], cfg)
    assert int((frames[:, f1:] != -1).sum()) == 0 and torch.equal(frames[:, :f0], one.reshape(B, P + N, cfg.S)[:, :f0])


# ------------------------------------------------------------------ 7: buffers
def test_only_the_generated_frames_are_written_and_the_buffers_grow():
    G = pkg("generate")
    cfg, m, ex, _ = model("exact", 5)
    P, keep, N, B, cap = 3, 2, 15, ex.shape[0], 25
    acts = torch.randint(0, 5, (B, cap), generator=torch.Generator().manual_seed(12)).cuda()
    noise, uni = draws(cfg, N, B, seed=13)
    kw = dict(maskgit_steps=STEPS, temperature=1.0)
    one = G.rollout_frames(m, ex[:, :P], N, keep=keep, noise=noise, uniforms=uni, action_ids=acts[:, :P + N].contiguous(), **kw)
    dec = G._Decode(m, STEPS, 1.0, "random", None, None, True)
    frames = torch.full((B, cap, cfg.S), -1, dtype=torch.int64, device="cuda")
    frames[:, :P] = ex[:, :P].reshape(B, P, cfg.S)
    G.rollout_call(m, frames, acts, P, keep, P, P + N, 0, G._rollout_cache(m, B, dec, "cuda"), dec, noise, uni)
    assert int((frames[:, P + N:] != -1).sum()) == 0
    check(frames[:, :P + N].view_as(one), one, cfg)
    # a Rollout that starts with room for one more frame doubles its buffers in mid-window (4 -> 8 -> 16 -> 32 frames)
    r = G.Rollout(m, ex[:, :P], keep=keep, prompt_actions=acts[:, :P], capacity=4, **kw)
    caps = set()
    for k in range(N):
        r.step(acts[:, P + k], noise=noise[k], uniforms=uni[k])
        caps.add(r._frames.shape[1])
    assert caps == {4, 8, 16, 32}
    check(r.frames, one, cfg)
