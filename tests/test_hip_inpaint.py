"""GPU tests of decoding with known tokens (inpainting) through every MaskGIT decode loop (include/genie_hip.h, "known tokens").

Every oracle is bit equality on token ids or cache bytes:
  * the two kernels against the NumPy model (tests/inpaint_model.py);
  * `known` all-mask against `known` absent, in all four loops;
  * the loops against a composition written HERE from calls that exist without the feature: genie_frame_pass / genie_frames_pass (or
    genie_compute_logits), genie_sample_ex / genie_sample_guided and the EXISTING genie_mask_step called once per clip with that clip's
    own count from inpaint_model.counts, the start state laid with torch ops, and two-frame commits whose second frame holds the next
    slot's known tokens.
All draws are fixed tensors."""
import functools

import numpy as np
import pytest

import inpaint_model as M
import stale_memory
from conftest import pkg
from test_hip_fanout import branch_actions, check, draws, mode_kw, shaped_model, slots
from test_hip_sampling import dev, tiny_model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def model(precision, A=0):
    return tiny_model(precision, A)          # cfg, model, clips (3, 8, 4, 4), actions: L 2, H 2, d 64, T 8, S 16, B 3


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_known(cfg, rows, frames, seed, truth=None):
    """(rows, frames, S) int64 known tokens on the GPU with mixed counts per clip and per frame: K = 0, 1, S / 2, S - 1 (one unknown token)
    and S (a fully known frame) in rotation, at random positions; "generate" is the mask id, -1 or a value past the vocabulary.
    truth: (rows, frames, S) tokens to keep (a counterfactual edit keeps observed tokens), else random ones."""
    S, mask = cfg.S, cfg.image_vocab_size
    rng = np.random.default_rng(seed)
    Ks = [S // 2, 0, S - 1, S, 1]
    kn = rng.choice([mask, -1, mask + 7], size=(rows, frames, S)).astype(np.int64)
    for r in range(rows):
        for f in range(frames):
            pos = rng.permutation(S)[:Ks[(r + 2 * f) % len(Ks)]]
            kn[r, f, pos] = rng.integers(0, mask, len(pos)) if truth is None else truth[r, f, pos]
    return dev(kn)


def valid(kn, mask):
    return (kn >= 0) & (kn < mask)


def check_keeps(out, known, cfg):
    """the output holds `known` wherever it is a token, and no mask id"""
    v = valid(known, cfg.image_vocab_size)
    assert torch.equal(out[v], known[v])
    assert int((out == cfg.image_vocab_size).sum()) == 0 and int((out < 0).sum()) == 0


# ------------------------------------------------------------------ 1: the kernels against the NumPy model
@pytest.mark.parametrize("S", [1, 16, 100, 256, 400, 1024])
def test_kernels_against_the_numpy_model(S):
    """B = 5 with K_b = 0, 1, S / 2, S - 1, S; keys with ties and -inf; the frame embedded in a (B, T, S) prompt; two non-final steps in a
    row (the second meets tokens unmasked by the first), then the final one; copies 1 and 2; known == NULL."""
    L = pkg("_lib")
    lib = L.load()
    B, T, t, mask, steps = 5, 3, 1, 1000, 3
    rng = np.random.default_rng(S)
    kn = np.full((B, 2, S), mask, dtype=np.int64)   # known rows live in a (B, 2, S) tensor: clip stride 2 S
    for b, K in enumerate([0, 1, S // 2, S - 1, S]):
        pos = rng.permutation(S)[:K]
        kn[b, 1, pos] = rng.integers(0, mask, len(pos))
    kn[:, 1][(kn[:, 1] == mask) & (rng.random((B, S)) < 0.3)] = -3     # another way to say "generate"
    kn[:, 1][(kn[:, 1] == mask) & (rng.random((B, S)) < 0.3)] = mask + 1
    d_kn = dev(kn)
    want_tok, want_um = M.start_state(kn[:, 1], mask)
    for copies in (1, 2):
        frame = torch.full((copies * B, T, S), -7, dtype=torch.int64, device="cuda")
        um = torch.full((B, S), 9, dtype=torch.uint8, device="cuda")
        L.check(lib.genie_known_begin(d_kn[:, 1].data_ptr(), 2 * S, mask, frame[:, t].data_ptr(), T * S, um.data_ptr(), B, S, copies, stream()),
                "genie_known_begin")
        got = frame.cpu().numpy()
        assert np.array_equal(got[:, t], np.concatenate([want_tok] * copies)) and (got[:, [0, 2]] == -7).all()
        assert np.array_equal(um.cpu().numpy().astype(bool), want_um)
        L.check(lib.genie_known_begin(d_kn[:, 1].data_ptr(), 2 * S, mask, frame[:, 2].data_ptr(), T * S, None, B, S, copies, stream()),
                "genie_known_begin")          # without the flags
        assert np.array_equal(frame.cpu().numpy()[:, 2], got[:, t])

    for known in (kn[:, 1], None):
        tok, um = M.start_state(kn[:, 1] if known is not None else np.full((B, S), mask), mask)
        prompt = np.full((B, T, S), -7, dtype=np.int64)
        prompt[:, t] = tok
        d_prompt, d_um = dev(prompt), dev(um.astype(np.uint8))
        for step in range(steps):
            last = step == steps - 1
            keys = (rng.integers(0, 4, (B, S)) / 4).astype(np.float32)     # ties everywhere
            keys[rng.random((B, S)) < 0.1] = -np.inf
            samples = rng.integers(0, mask, (B, S)).astype(np.int64)
            d_keys, d_s = dev(keys), dev(samples)
            L.check(lib.genie_mask_step_known(0 if last else d_keys.data_ptr(), 0.0 if last else lib.genie_mask_fraction(step, steps), int(last),
                                              mask, 0 if known is None else d_kn[:, 1].data_ptr(), 2 * S, d_um.data_ptr(), d_s.data_ptr(),
                                              d_prompt[:, t].data_ptr(), T * S, B, S, stream()), "genie_mask_step_known")
            M.mask_step(samples, keys, um, known, step, steps, mask, tok)
            got = d_prompt.cpu().numpy()
            assert np.array_equal(got[:, t], tok) and (got[:, [0, 2]] == -7).all(), (step, known is None)
            assert np.array_equal(d_s.cpu().numpy(), samples) and np.array_equal(d_um.cpu().numpy().astype(bool), um)
            if not last:
                K = M.is_known(kn[:, 1], mask).sum(1) if known is not None else np.zeros(B, dtype=int)
                assert [(tok[b] == mask).sum() for b in range(B)] == [M.counts(steps, S - int(K[b]))[step] for b in range(B)]
        k = M.is_known(kn[:, 1], mask)
        assert not (tok == mask).any() and (known is None or np.array_equal(tok[k], kn[:, 1][k]))


# ------------------------------------------------------------------ the calls under test, at the C level
def decode_of(m, steps, temperature, mode, guidance=None, merge_commit=True):
    return pkg("generate")._Decode(m, steps, temperature, mode, mode_kw(mode)["sampling"], guidance, merge_commit)


def run_cached(m, ex, P, dec, noise, uni, known=None, tf=False, acts=None, want_logits=False):
    """genie_generate_cached (known None: through the entry points of before) -> (gen (B, n_new, S), cache bytes, step-0 logits or None)"""
    L = pkg("_lib")
    lib = L.load()
    cfg, w = m._weights()[:2]
    c = m.config
    B, n_new, S = ex.shape[0], ex.shape[1] - P, c.S
    ids = ex.reshape(B, P + n_new, S).contiguous()
    NB = B if dec.guide is None else 2 * B
    cond = m._cond(acts, B, n_frames=P + n_new)
    cache = torch.full((lib.genie_prefix_cache_bytes(cfg, NB),), 0x55, dtype=torch.uint8, device="cuda")
    ws = m._workspace(B, generate_prompt_frames=P, guided=dec.guide is not None)
    nz, un = dec.draws(m, n_new, B, noise, uni, ex.device)
    gen = torch.empty(B, n_new, S, dtype=torch.int64, device="cuda")
    lg = torch.empty(B, n_new, S, c.factored_vocab_size * c.num_factored_vocabs, device="cuda") if want_logits else None
    L.check(L.call_known(lib, "genie_generate_cached", cond, dec.law, dec.guide, L.make_known(known, n_new, S), cfg, w, ids.data_ptr(), B, P,
                         n_new, dec.steps, dec.temperature, dec.mode, 0 if nz is None else nz.data_ptr(), 0 if un is None else un.data_ptr(),
                         int(tf), int(dec.merge_commit), gen.data_ptr(), 0 if lg is None else lg.data_ptr(), cache.data_ptr(), cache.numel(),
                         ws.data_ptr(), ws.numel(), stream()), "genie_generate_cached")
    return gen, cache, lg


def run_fanout(m, prompt, K, n_new, dec, noise, uni, known=None, acts=None, pacts=None):
    """genie_generate_fanout -> (gen (B, K, n_new, S), trunk, branch, (B K, T) action ids or None)"""
    G, L = pkg("generate"), pkg("_lib")
    lib = L.load()
    cfg = m._weights()[0]
    B, P, K, pa, ba, pv, bv = G._fanout_inputs(m, prompt, n_new, K, acts, None, pacts, None)
    NB = B * (1 if dec.guide is None else 2)
    cond = G.fanout_cond(m, B, P, K, n_new, pa, ba, pv, bv, prompt.device)
    trunk = torch.full((lib.genie_prefix_cache_bytes(cfg, NB),), 0x7F, dtype=torch.uint8, device="cuda")
    branch = torch.full((lib.genie_fanout_branch_bytes(cfg, NB, K, n_new),), 0x7F, dtype=torch.uint8, device="cuda")
    nz, un = dec.draws(m, n_new, B * K, noise, uni, prompt.device)
    gen = G.fanout_call(m, prompt.reshape(B, P, -1).contiguous(), K, n_new, cond, dec, nz, un, trunk=trunk, branch=branch, known=known)
    return gen, trunk, branch, None if cond is None else cond.keep.view(B * K, -1)


def run_rollout(m, prompt, n_new, keep, dec, noise, uni, known=None):
    """genie_rollout_cached from the prompt -> (frames (B, P + n_new, S), cache)"""
    G = pkg("generate")
    B, P, S = prompt.shape[0], prompt.shape[1], m.config.S
    frames = torch.full((B, P + n_new, S), m.mask_token_id, dtype=torch.int64, device="cuda")
    frames[:, :P] = prompt.reshape(B, P, S)
    cache = G._rollout_cache(m, B, dec, prompt.device)
    cache.fill_(0x55)
    nz, un = dec.draws(m, n_new, B, noise, uni, prompt.device)
    G.rollout_call(m, frames, None, P, keep, P, P + n_new, 0, cache, dec, nz, un, known=known)
    return frames, cache


# ------------------------------------------------------------------ the composition oracle
def compose(m, B, P, n_new, dec, noise, uni, known, ids=None, tf=False, act_ids=None, seed=None):
    """The decode loop of B clips with known tokens (B, n_new, S), from calls that exist without them -> (tokens (B, n_new, S), cache,
    did the merged commits run).  ids (B, P + n_new, S): the clips (prompt, and the ground truth when teacher-forcing).  seed: (trunk,
    clips of the trunk, K) of a fan-out call -- the cache starts from the trunk's slots [0, P), each parent K times, instead of running
    the prompt.  act_ids: (B, T) actions."""
    L = pkg("_lib")
    lib = L.load()
    c = m.config
    cfg, w = m._weights()[:2]
    S, T, V, steps, mask = c.S, c.T, c.factored_vocab_size * c.num_factored_vocabs, dec.steps, c.image_vocab_size
    guided = dec.guide is not None
    NB = 2 * B if guided else B
    cache = torch.full((lib.genie_prefix_cache_bytes(cfg, NB),), 0x55, dtype=torch.uint8, device="cuda")
    cond = None
    if act_ids is not None:
        a = torch.cat([act_ids, torch.full_like(act_ids, dec.guide.null_action)]) if guided else act_ids
        cond = m._frame_cond(a.contiguous())
    ws = torch.empty(max(lib.genie_generate_workspace_bytes(cfg, NB, P), lib.genie_workspace_bytes(cfg, NB)), dtype=torch.uint8, device="cuda")
    st = stream()
    both = (lambda x: torch.cat([x, x]).contiguous()) if guided else (lambda x: x.contiguous())

    def frames_pass(tokens, t, nf, lg):
        return L.call_cond(lib, "genie_frames_pass", cond, cfg, w, tokens.data_ptr(), NB, t, nf, cache.data_ptr(), cache.numel(),
                           0 if lg is None else lg.data_ptr(), ws.data_ptr(), ws.numel(), st)

    def frame_pass(tokens, t, lg):
        L.check(L.call_cond(lib, "genie_frame_pass", cond, cfg, w, tokens.data_ptr(), NB, t, cache.data_ptr(), cache.numel(),
                            0 if lg is None else lg.data_ptr(), ws.data_ptr(), ws.numel(), st), "genie_frame_pass")

    if seed is not None:
        trunk, nb_trunk, K = seed
        slots(cache, m, NB, T)[:, :, :P] = slots(trunk, m, nb_trunk, T)[:, :, :P].repeat_interleave(K, dim=1)
    else:   # the prompt, by the sequence of the loops: one P-frame pass, else the clean pass, else frame by frame
        pr = both(ids[:, :P])
        rc = L.E_UNSUPPORTED
        if P > 1:
            rc = frames_pass(pr, 0, P, None)
            if rc == L.E_UNSUPPORTED:
                rc = L.call_cond(lib, "genie_clean_pass", cond, cfg, w, pr.data_ptr(), NB, P, T, cache.data_ptr(), cache.numel(), ws.data_ptr(),
                                 ws.numel(), st)
        if rc == L.E_UNSUPPORTED:
            for t in range(P):
                frame_pass(pr[:, t].contiguous(), t, None)
        else:
            L.check(rc, "prompt")
    logits = torch.empty(NB, S, V, dtype=torch.float32, device="cuda")
    samples = torch.empty(B, S, dtype=torch.int64, device="cuda")
    conf = torch.empty(B, S, dtype=torch.float32, device="cuda")
    by_conf = dec.mode == L.UNMASK_CONFIDENCE
    left = (S - valid(known, mask).sum(-1)).cpu().numpy()           # M_b of every (clip, frame)
    start = torch.where(valid(known, mask), known, torch.full_like(known, mask))
    out, opened, merge, merged = [], False, dec.merge_commit, False
    for k in range(n_new):
        t = P + k
        cur = both(start[:, k])
        unmasked = valid(known[:, k], mask).to(torch.uint8).contiguous()
        for step in range(steps):
            if not (step == 0 and opened):
                frame_pass(cur, t, logits)
            last = step == steps - 1
            u = uni[k, step].contiguous() if dec.temperature > 1e-8 else None
            nz = None if (last or dec.unmask_mode == "greedy") else noise[k, step].contiguous()
            keys_out = conf if (by_conf and not last) else None
            tail = (dec.law, 0 if keys_out is None else keys_out.data_ptr(), 0 if nz is None else nz.data_ptr(), 1.0 - (step + 1) / steps)
            if guided:
                L.check(lib.genie_sample_guided(cfg, logits[:B].data_ptr(), logits[B:].data_ptr(), L.LAYOUT_TOKEN_MAJOR, B, dec.temperature,
                                                0 if u is None else u.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, *tail,
                                                dec.guide.scale), "genie_sample_guided")
            else:
                L.check(lib.genie_sample_ex(cfg, logits.data_ptr(), L.LAYOUT_TOKEN_MAJOR, B, dec.temperature, 0 if u is None else u.data_ptr(),
                                            samples.data_ptr(), conf.data_ptr(), st, *tail), "genie_sample_ex")
            keys = None if last else (nz if dec.unmask_mode == "random" else conf)
            for b in range(B):   # the existing mask step, one clip at a time, with that clip's own count
                n = 0 if last else M.counts(steps, int(left[b, k]))[step]
                L.check(lib.genie_mask_step(0 if keys is None else keys.data_ptr() + 4 * b * S, n, int(last), mask, unmasked.data_ptr() + b * S,
                                            samples.data_ptr() + 8 * b * S, cur.data_ptr() + 8 * b * S, S, 1, S, st), "genie_mask_step")
            if guided:
                cur[B:] = cur[:B]
        out.append(cur[:B].clone())
        opened = False
        if k + 1 < n_new:
            final = both(ids[:, t]) if tf else cur
            if merge:
                two = torch.stack([final, both(start[:, k + 1])], dim=1).contiguous()
                rc = frames_pass(two, t, 2, logits)
                if rc == L.E_UNSUPPORTED:
                    merge = False
                else:
                    L.check(rc, "genie_frames_pass")
                    opened = merged = True
            if not opened:
                frame_pass(final, t, None)
    return torch.stack(out, dim=1), cache, merged


def cached_vs_composition(m, ex, P, steps, temperature, mode, known, tf=False, merge_commit=True, acts=None, guidance=None, seed=3):
    c = m.config
    B, n_new = ex.shape[0], ex.shape[1] - P
    noise, uni = draws(c, n_new, B, steps=steps, seed=seed)
    dec = decode_of(m, steps, temperature, mode, guidance, merge_commit)
    gen, cache, _ = run_cached(m, ex, P, dec, noise, uni, known, tf, acts)
    want, ref, merged = compose(m, B, P, n_new, dec, noise, uni, known, ids=ex.reshape(B, P + n_new, -1), tf=tf, act_ids=acts)
    check(gen, want, c)
    check_keeps(gen, known, c)
    NB = B if dec.guide is None else 2 * B
    a, b = slots(cache, m, NB, c.T)[:, :, :P + n_new - 1], slots(ref, m, NB, c.T)[:, :, :P + n_new - 1]     # the prompt and every committed slot
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} cache values differ"
    return gen, merged


# ------------------------------------------------------------------ 2: known all-mask == known absent
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_all_mask_known_is_no_known_in_all_four_loops(precision, temperature):
    cfg, m, ex, _ = model(precision)
    B, S, P, steps = ex.shape[0], cfg.S, 3, 2
    n_new = cfg.T - P
    dec = decode_of(m, steps, temperature, "random")

    def nothing(rows, frames):
        return torch.full((rows, frames, S), cfg.image_vocab_size, dtype=torch.int64, device="cuda")

    noise, uni = draws(cfg, n_new, B, seed=21)
    a, b = run_cached(m, ex, P, dec, noise, uni, None, want_logits=True), run_cached(m, ex, P, dec, noise, uni, nothing(B, n_new), want_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = run_rollout(m, ex[:, :P], 9, 3, dec, *draws(cfg, 9, B, seed=22)), run_rollout(m, ex[:, :P], 9, 3, dec, *draws(cfg, 9, B, seed=22),
                                                                                        known=nothing(B, 9))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    noise, uni = draws(cfg, n_new, 2 * 3, seed=23)
    a, b = run_fanout(m, ex[:2, :P], 3, n_new, dec, noise, uni)[:3], run_fanout(m, ex[:2, :P], 3, n_new, dec, noise, uni, nothing(6, n_new))[:3]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the full-forward loop: samples, the prompt frame and the step-0 logits
    outs = []
    for known in (None, nothing(B, 1).view(B, 4, 4)):
        p = ex.clone()
        p[:, P:] = cfg.image_vocab_size
        s, lg = m.maskgit_generate(p, P, maskgit_steps=steps, temperature=temperature, noise=noise[0, :, :B].contiguous(),
                                   uniforms=uni[0, :, :, :B].contiguous(), known=known)
        outs.append((s, lg.contiguous(), p))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


# ------------------------------------------------------------------ 3: the cached loop against the composition
@pytest.mark.parametrize("mode", ["random", "greedy", "confidence"])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("steps", [1, 2, 4])
def test_cached_loop_equals_the_composition(steps, temperature, mode):
    """B = 3, P = 3, 5 new frames whose known counts are mixed per clip and per frame (a fully known frame and a frame with one unknown
    token among them); merge_commit on and off, teacher forcing on and off."""
    cfg, m, ex, _ = model("exact")
    known = make_known(cfg, 3, 5, seed=steps)
    for merge_commit in (True, False):
        for tf in (False, True):
            cached_vs_composition(m, ex, 3, steps, temperature, mode, known, tf, merge_commit)


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_cached_loop_equals_the_composition_in_16_bit(precision):
    cfg, m, ex, _ = model(precision)
    truth = ex[:, 3:].reshape(3, 5, -1).cpu().numpy()
    for tf in (False, True):       # the edit: observed tokens kept, the context teacher-forced
        cached_vs_composition(m, ex, 3, 2, 1.0, "random", make_known(cfg, 3, 5, seed=31, truth=truth), tf)


@pytest.mark.parametrize("merge_commit", [True, False])
def test_cached_loop_equals_the_composition_under_guidance(merge_commit):
    """both halves of every pass see the same tokens, known ones included; the second frame of a merged commit too"""
    cfg, m, ex, _ = model("exact", 5)
    acts = torch.randint(0, 4, (3, cfg.T), generator=torch.Generator().manual_seed(9)).cuda()
    gd = pkg("sampling").Guidance(3.0, 4)
    for mode in ("random", "confidence"):
        cached_vs_composition(m, ex, 3, 2, 1.0, mode, make_known(cfg, 3, 5, seed=41), merge_commit=merge_commit, acts=acts, guidance=gd)


def test_cached_loop_on_the_fragment_order_kernels():
    """S = 256, d = 128, 2 heads, f16x3: the merged two-frame commit is taken, and its second frame carries the next slot's known tokens."""
    cfg, m, clips = shaped_model("f16x3", heads=2, d=128, T=16, S=256)
    known = make_known(cfg, 2, 3, seed=51)
    _, merged = cached_vs_composition(m, clips[:, :8], 5, 2, 1.0, "random", known)
    assert merged, "the merged two-frame passes did not run: the fragment-order kernels do not cover this model"


# ------------------------------------------------------------------ 4: merge_commit on == off
def test_merged_commits_equal_plain_commits_with_known_tokens():
    """the conditions of test_hip_frame.test_merged_commit_schedule_equals_plain_kv_cache_schedule (d 256, heads of 64, T 16, S 256,
    f16x3, 8 prompt frames), with known tokens: both loop forms, merged or not, teacher-forced or not"""
    from test_hip_frame import _model
    G = pkg("generate")
    cfg, m = _model(256, 4, layers=3)
    steps, B = 2, 2
    ex = dev(pkg("synthetic").make_clips(B, cfg, seed=42)).view(B, 16, 16, 16)
    noise = torch.rand(8, steps - 1, B, cfg.S, generator=torch.Generator().manual_seed(1)).cuda()
    known = make_known(cfg, B, 8, seed=61).view(B, 8, 16, 16)
    for tf in (False, True):
        plain = G.generate_frames_cached(m, ex, 8, steps, 0.0, tf, noise=noise, merge_commit=False, host_loop=True, known=known)
        for mc, host in ((True, True), (False, False), (True, False)):
            got = G.generate_frames_cached(m, ex, 8, steps, 0.0, tf, noise=noise, merge_commit=mc, host_loop=host, known=known)
            assert torch.equal(got, plain), (tf, mc, host)
        check_keeps(plain[:, 8:16], known, cfg)


# ------------------------------------------------------------------ 5: the full-forward loop
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("mode,temperature,steps", [("random", 0.0, 1), ("random", 1.0, 2), ("greedy", 0.0, 4), ("confidence", 1.0, 4)])
def test_full_forward_loop_equals_the_composition(mode, temperature, steps, guided):
    """genie_maskgit_generate_known against genie_compute_logits, the sample launch and the per-clip genie_mask_step on a prompt whose
    frame starts from the known tokens; samples_out equals the prompt frame; the step-0 logits are those of that start."""
    L = pkg("_lib")
    lib = L.load()
    cfg, m, ex, _ = model("exact", 5 if guided else 0)
    c, w = m._weights()[:2]
    B, S, T, t, mask = ex.shape[0], cfg.S, cfg.T, 4, cfg.image_vocab_size
    V = cfg.factored_vocab_size * cfg.num_factored_vocabs
    acts = torch.randint(0, 4, (B, T), generator=torch.Generator().manual_seed(9)).cuda() if guided else None
    gd = pkg("sampling").Guidance(3.0, 4) if guided else None
    dec = decode_of(m, steps, temperature, mode, gd)
    known = make_known(cfg, B, 1, seed=70 + steps)[:, 0].contiguous()
    noise, uni = draws(cfg, 1, B, steps=steps, seed=71)
    noise, uni = noise[0], uni[0]
    p = ex.clone()
    p[:, t:] = mask
    got, lg0 = m.maskgit_generate(p, t, maskgit_steps=steps, temperature=temperature, unmask_mode=mode, sampling=mode_kw(mode)["sampling"],
                                  noise=noise if steps > 1 else None, uniforms=uni, action_ids=acts, guidance=gd, known=known.view(B, 4, 4))
    assert torch.equal(got, p[:, t])          # samples_out is the prompt frame
    check_keeps(got.view(B, S), known, cfg)
    # the composition
    NB = 2 * B if guided else B
    q = ex.clone().view(B, T, S)
    q[:, t:] = mask
    q[:, t] = torch.where(valid(known, mask), known, torch.full_like(known, mask))
    unmasked = valid(known, mask).to(torch.uint8).contiguous()
    left = (S - valid(known, mask).sum(-1)).cpu().numpy()
    cond = None
    if guided:
        cond = m._frame_cond(torch.cat([acts, torch.full_like(acts, gd.null_action)]).contiguous())
    ws = torch.empty(lib.genie_workspace_bytes(c, NB), dtype=torch.uint8, device="cuda")
    logits = torch.empty(NB, S, V, device="cuda")
    samples = torch.empty(B, S, dtype=torch.int64, device="cuda")
    conf = torch.empty(B, S, device="cuda")
    by_conf = dec.mode == L.UNMASK_CONFIDENCE
    st = stream()
    for step in range(steps):
        tokens = torch.cat([q, q]).contiguous() if guided else q
        L.check(L.call_cond(lib, "genie_compute_logits", cond, c, w, tokens.data_ptr(), NB, t, t + 1, L.LAYOUT_TOKEN_MAJOR, logits.data_ptr(),
                            ws.data_ptr(), ws.numel(), st), "genie_compute_logits")
        if step == 0:
            first = logits.clone()
        last = step == steps - 1
        u = uni[step].contiguous() if temperature > 1e-8 else None
        nz = None if (last or mode == "greedy") else noise[step].contiguous()
        keys_out = conf if (by_conf and not last) else None
        tail = (dec.law, 0 if keys_out is None else keys_out.data_ptr(), 0 if nz is None else nz.data_ptr(), 1.0 - (step + 1) / steps)
        if guided:
            L.check(lib.genie_sample_guided(c, logits[:B].data_ptr(), logits[B:].data_ptr(), L.LAYOUT_TOKEN_MAJOR, B, dec.temperature,
                                            0 if u is None else u.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, *tail, dec.guide.scale),
                    "genie_sample_guided")
        else:
            L.check(lib.genie_sample_ex(c, logits.data_ptr(), L.LAYOUT_TOKEN_MAJOR, B, dec.temperature, 0 if u is None else u.data_ptr(),
                                        samples.data_ptr(), conf.data_ptr(), st, *tail), "genie_sample_ex")
        keys = None if last else (nz if mode == "random" else conf)
        for b in range(B):
            n = 0 if last else M.counts(steps, int(left[b]))[step]
            L.check(lib.genie_mask_step(0 if keys is None else keys.data_ptr() + 4 * b * S, n, int(last), mask, unmasked.data_ptr() + b * S,
                                        samples.data_ptr() + 8 * b * S, q[b, t].data_ptr(), T * S, 1, S, st), "genie_mask_step")
    check(got.view(B, S), q[:, t], cfg)
    assert torch.equal(samples, q[:, t])
    # step-0 logits: the model's logits on the start tokens, known positions included (guided: the guided ones)
    if guided:
        L.check(lib.genie_guide_logits(first[:B].data_ptr(), first[B:].data_ptr(), first.data_ptr(), B * S * V, gd.scale, st), "genie_guide_logits")
    want0 = first[:B].view(B, 4, 4, cfg.num_factored_vocabs, cfg.factored_vocab_size).permute(0, 4, 3, 1, 2)
    assert torch.equal(lg0, want0)


# ------------------------------------------------------------------ 6: fan-out and rollout
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_fanout_of_one_branch_is_the_cached_call(precision):
    cfg, m, ex, _ = model(precision)
    B, P = ex.shape[0], 3
    n_new = cfg.T - P
    dec = decode_of(m, 2, 1.0, "random")
    noise, uni = draws(cfg, n_new, B, seed=81)
    known = make_known(cfg, B, n_new, seed=82)
    gen = run_fanout(m, ex[:, :P], 1, n_new, dec, noise, uni, known)[0]
    want = run_cached(m, ex, P, dec, noise, uni, known)[0]
    check(gen[:, 0], want, cfg)
    check_keeps(want, known, cfg)


@pytest.mark.parametrize("guided", [False, True])
def test_fanout_of_three_branches_equals_the_replicated_composition(guided):
    """B = 2, K = 3, P = 3, 4 new frames, per-branch actions and per-branch known tokens: the composition on a full cache of B K clips
    seeded from the trunk; tokens and the committed branch slots"""
    cfg, m, ex, _ = model("exact", 5)
    B, K, P, n_new = 2, 3, 3, 4
    acts, pacts = branch_actions(B, K, P, n_new, 4, seed=10)
    dec = decode_of(m, 2, 1.0, "random", pkg("sampling").Guidance(3.0, 4) if guided else None)
    noise, uni = draws(cfg, n_new, B * K, seed=83)
    known = make_known(cfg, B * K, n_new, seed=84)
    gen, trunk, branch, act_ids = run_fanout(m, ex[:B, :P], K, n_new, dec, noise, uni, known, acts, pacts)
    copies = 2 if guided else 1
    want, cache, _ = compose(m, B * K, P, n_new, dec, noise, uni, known, act_ids=act_ids, seed=(trunk, B * copies, K))
    check(gen.view(B * K, n_new, -1), want, cfg)
    check_keeps(gen.view(B * K, n_new, -1), known, cfg)
    NBK = B * K * copies
    got, ref = slots(branch, m, NBK, n_new)[:, :, :n_new - 1], slots(cache, m, NBK, cfg.T)[:, :, P:P + n_new - 1]
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {got.numel()} cache values differ"


@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_rollout_over_two_windows(precision):
    """T = 8, P = 3, keep = 3, 9 new frames: window 0 decodes 5 frames, window 1 the other 4.  One call == a Rollout.step(known=...) chain
    (every step resumes the cache: the merged commit of the pending frame opens the next one with ITS known tokens); inside the first
    window == the cached call."""
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    B, P, keep, N = ex.shape[0], 3, 3, 9
    noise, uni = draws(cfg, N, B, seed=91)
    known = make_known(cfg, B, N, seed=92).view(B, N, 4, 4)
    kw = dict(keep=keep, maskgit_steps=2, temperature=1.0)
    got = G.rollout_frames(m, ex[:, :P], N, noise=noise, uniforms=uni, known=known, **kw)
    check_keeps(got[:, P:], known, cfg)
    r = G.Rollout(m, ex[:, :P], **kw)
    for k in range(N):
        fr = r.step(noise=noise[k], uniforms=uni[k], known=known[:, k].contiguous())
        assert torch.equal(fr, got[:, P + k]), k
    check(r.frames, got, cfg)
    n0 = cfg.T - P
    dec = decode_of(m, 2, 1.0, "random")
    want = run_cached(m, ex, P, dec, noise[:n0], uni[:n0].contiguous(), known[:, :n0].reshape(B, n0, -1).contiguous())[0]
    check(got[:, P:cfg.T].reshape(B, n0, -1), want, cfg)


# ------------------------------------------------------------------ 7: the Python surface
def test_python_surface():
    G = pkg("generate")
    cfg, m, ex, _ = model("exact")
    B, P, S, mask = ex.shape[0], 3, cfg.S, cfg.image_vocab_size
    n_new = cfg.T - P
    dec = decode_of(m, 2, 1.0, "random")
    noise, uni = draws(cfg, n_new, B, seed=101)
    keep = torch.zeros(4, 4, dtype=torch.bool, device="cuda")
    keep[1:3, 0:3] = True                                   # a box in token coordinates
    known = G.known_tokens(ex[:, P:], keep, m.mask_token_id)
    assert known.shape == (B, n_new, 4, 4) and torch.equal(known[..., 1:3, 0:3], ex[:, P:, 1:3, 0:3]) and int((known == mask).sum()) == B * n_new * 10
    full = G.known_tokens(ex[:, P:], keep.expand(B, n_new, 4, 4), m.mask_token_id)
    assert torch.equal(full, known)
    kflat = known.view(B, n_new, S)
    kw = dict(maskgit_steps=2, temperature=1.0, noise=noise, uniforms=uni, known=known)
    want = run_cached(m, ex, P, dec, noise, uni, kflat)[0].view(B, n_new, 4, 4)
    assert torch.equal(want[..., 1:3, 0:3], ex[:, P:, 1:3, 0:3])
    # the cached loop in both forms, and the full-forward harness (same arithmetic per row in exact)
    one = G.generate_frames_cached(m, ex, P, **kw)
    assert torch.equal(one[:, P:cfg.T], want) and torch.equal(one[:, :P], ex[:, :P]) and torch.equal(one[:, cfg.T:], ex[:, P:])
    assert torch.equal(G.generate_frames_cached(m, ex, P, host_loop=True, **kw), one)
    for tf in (False, True):
        a = G.generate_frames_cached(m, ex, P, teacher_force_time=tf, **kw)
        assert torch.equal(G.generate_frames_cached(m, ex, P, teacher_force_time=tf, host_loop=True, **kw), a)
        f = G.generate_frames(m, ex, P, teacher_force_time=tf, **kw)
        check_keeps(f[:, P:cfg.T], known, cfg)
        assert f.shape == a.shape
    # rollout, Rollout.extend, fan-out, and the model's methods
    r = G.rollout_frames(m, ex[:, :P], n_new, **kw)
    assert torch.equal(r[:, P:], want) and torch.equal(m.rollout(ex[:, :P], n_new, **kw), r)
    ro = G.Rollout(m, ex[:, :P], maskgit_steps=2, temperature=1.0)
    a = ro.extend(2, noise=noise[:2], uniforms=uni[:2], known=known[:, :2].contiguous())
    b = ro.extend(n_new - 2, noise=noise[2:], uniforms=uni[2:], known=known[:, 2:].contiguous())
    assert torch.equal(torch.cat([a, b], 1), want)
    fo = G.fanout_frames(m, ex[:, :P], n_new, K=1, **kw)                                    # (B, n_new, H, W) for all K
    assert torch.equal(fo[:, 0], want)
    assert torch.equal(m.fanout(ex[:, :P], n_new, K=1, **dict(kw, known=known[:, None].contiguous())), fo)
    nz3, un3 = draws(cfg, n_new, B * 2, seed=102)
    f2 = G.fanout_frames(m, ex[:, :P], n_new, K=2, **dict(kw, noise=nz3, uniforms=un3))
    check_keeps(f2, known[:, None].expand(B, 2, n_new, 4, 4), cfg)
    # maskgit_generate of the model
    p = ex.clone()
    p[:, P:] = mask
    s, _ = m.maskgit_generate(p, P, maskgit_steps=2, temperature=1.0, noise=noise[0], uniforms=uni[0], known=known[:, 0].contiguous())
    check_keeps(s, known[:, 0], cfg)
    assert torch.equal(s, p[:, P])
    # a wrong shape, dtype or device raises before any launch
    for bad in (known[:, :2], known.to(torch.int32), known.cpu(), known.view(B, n_new, S)):
        for call in (lambda k: G.generate_frames_cached(m, ex, P, **dict(kw, known=k)), lambda k: G.generate_frames(m, ex, P, **dict(kw, known=k)),
                     lambda k: G.rollout_frames(m, ex[:, :P], n_new, **dict(kw, known=k)),
                     lambda k: G.fanout_frames(m, ex[:, :P], n_new, K=1, **dict(kw, known=k))):
            with pytest.raises(RuntimeError, match="known"):
                call(bad)
    with pytest.raises(RuntimeError, match="known"):
        m.maskgit_generate(p, P, known=known)
    with pytest.raises(RuntimeError, match="known"):
        G.Rollout(m, ex[:, :P]).step(known=known[:, 0].view(B, S))
    with pytest.raises(RuntimeError, match="keep"):
        G.known_tokens(ex[:, P:], keep.to(torch.uint8), mask)


# ------------------------------------------------------------------ 8: stale memory
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_known_tokens_under_stale_memory(precision):
    """a known-token cached generate, a fan-out and a rollout past the window: the ids of the clean run under both poisons"""
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    B, P = ex.shape[0], 3
    n_new = cfg.T - P
    noise, uni = draws(cfg, 9, B, seed=111)
    nz2, un2 = draws(cfg, n_new, B * 2, seed=112)
    known = make_known(cfg, B, 9, seed=113).view(B, 9, 4, 4)
    kw = dict(maskgit_steps=2, temperature=1.0)

    def run(byte=None):
        if byte is not None:     # the model keeps its workspace across calls: poison it too
            stale_memory.poison_tensor(m._ws, byte)
        return (G.generate_frames_cached(m, ex, P, noise=noise[:n_new], uniforms=uni[:n_new].contiguous(), known=known[:, :n_new].contiguous(), **kw),
                G.fanout_frames(m, ex[:, :P], n_new, K=2, noise=nz2, uniforms=un2, known=known[:, :n_new].contiguous(), **kw),
                G.rollout_frames(m, ex[:, :P], 9, keep=3, noise=noise, uniforms=uni, known=known, **kw))
    clean = run()
    for byte in stale_memory.PATTERNS:
        with stale_memory.poisoned(byte, sentinel=cfg.image_vocab_size):
            got = run(byte)
        for a, b in zip(got, clean):
            assert torch.equal(a, b), (byte, int((a != b).sum()))
