"""GPU tests of fan-out generation (genie_generate_fanout, generate.fanout_frames): K futures per clip over one shared context cache.

Every oracle is bit equality on token ids or cache contents, and a composition of calls that exist without the feature:
  * K = 1 is generate_frames_cached (the whole-loop library call) -- the same launches at other addresses;
  * K > 1 is the K-times replicated batch: a full (L, NB K, T, S, 3d) cache whose slots [0, P) are the trunk's, each parent's clip
    repeated K times, decoded by a host loop written HERE from genie_frame_pass / genie_frames_pass, genie_sample_ex (or
    genie_sample_guided) and genie_mask_step with per-branch actions and the same draws.  Its tokens and the slots it commits must equal
    the call's tokens and branch cache.
All draws are fixed tensors."""
import functools
import math

import numpy as np
import pytest

from conftest import pkg
from test_hip_action_vectors import AD, proj_weights, projected_table
from test_hip_sampling import dev, tiny_model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 2


@functools.lru_cache(maxsize=None)
def model(precision, A=0):
    return tiny_model(precision, A)          # cfg, model, clips (3, 8, 4, 4), actions: L 2, H 2, d 64, T 8, S 16, B 3


@functools.lru_cache(maxsize=None)
def shaped_model(precision, heads=2, d=64, T=8, S=16, qk_norm=False, seed=11):
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=heads, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm, use_mup=False)
    sd = pkg("synthetic").make_state_dict(cfg, seed=seed, law="conditioned")
    m = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    side = int(math.isqrt(S))
    clips = dev(pkg("synthetic").make_clips(2, cfg, seed=seed + 51)).view(2, T, side, side)
    return cfg, m, clips


def draws(cfg, N, rows, steps=STEPS, seed=3):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(N, steps - 1, rows, cfg.S, generator=g).cuda()
    uni = torch.rand(N, steps, cfg.num_factored_vocabs, rows, cfg.S, generator=g).cuda()
    return noise, uni


def mode_kw(mode):
    return dict(unmask_mode=mode, sampling=pkg("sampling").SamplingConfig(0.7, 8, 0.9) if mode == "confidence" else None)


def check(a, b, cfg):
    assert a.shape == b.shape
    assert int((a == cfg.image_vocab_size).sum()) == 0 and int((a < 0).sum()) == 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} ids differ"


def cache16(m):
    """Does this model keep its temporal KV cache in 16 bits (the first half of each layer's slice)?"""
    c = m.config
    return m.precision == "bf16" and c.T <= 16 and c.d_model // c.num_heads in (32, 64)


def slots(buf, m, clips, frames):
    """(L, clips, frames, S * 3d) view of a cache buffer's values: f32, or the 16-bit halves of the layer slices."""
    c = m.config
    n = clips * frames * c.S * 3 * c.d_model
    if cache16(m):
        return buf.view(torch.int16).view(c.num_layers, 2, n)[:, 0].view(c.num_layers, clips, frames, -1)
    return buf.view(torch.int32).view(c.num_layers, clips, frames, -1)


# ------------------------------------------------------------------ the call, and the replicated-cache oracle
def run_fanout(m, prompt, K, n_new, temperature, noise, uni, steps=STEPS, acts=None, pacts=None, guidance=None, merge_commit=True, mode="random",
               sampling=None):
    """-> (tokens (B, K, n_new, S), trunk, branch, (B K, T) action ids or None, the _Decode options)."""
    G, L = pkg("generate"), pkg("_lib")
    lib = L.load()
    cfg = m._weights()[0]
    B, P = prompt.shape[:2]
    B, P, K, pa, ba, pv, bv = G._fanout_inputs(m, prompt, n_new, K, acts, None, pacts, None)
    dec = G._Decode(m, steps, temperature, mode, sampling, guidance, merge_commit)
    NB = B * (1 if dec.guide is None else 2)
    cond = G.fanout_cond(m, B, P, K, n_new, pa, ba, pv, bv, prompt.device)
    trunk = torch.full((lib.genie_prefix_cache_bytes(cfg, NB),), 0x7F, dtype=torch.uint8, device="cuda")
    branch = torch.full((lib.genie_fanout_branch_bytes(cfg, NB, K, n_new),), 0x7F, dtype=torch.uint8, device="cuda")
    nz, un = dec.draws(m, n_new, B * K, noise, uni, prompt.device)
    gen = G.fanout_call(m, prompt.reshape(B, P, -1).contiguous(), K, n_new, cond, dec, nz, un, trunk=trunk, branch=branch)
    return gen, trunk, branch, None if cond is None else cond.keep.view(B * K, -1), dec


def replicated_oracle(m, trunk, B, K, P, n_new, temperature, noise, uni, dec, act_ids=None):
    """The K-times replicated batch on a full cache seeded from the trunk: -> (tokens (B, K, n_new, S), the cache)."""
    L = pkg("_lib")
    lib = L.load()
    c = m.config
    cfg, w = m._weights()[:2]
    S, T, V, steps = c.S, c.T, c.factored_vocab_size * c.num_factored_vocabs, dec.steps
    guided = dec.guide is not None
    BK = B * K
    NB, NBK = (2 * B, 2 * BK) if guided else (B, BK)
    cache = torch.full((lib.genie_prefix_cache_bytes(cfg, NBK),), 0x55, dtype=torch.uint8, device="cuda")
    slots(cache, m, NBK, T)[:, :, :P] = slots(trunk, m, NB, T)[:, :, :P].repeat_interleave(K, dim=1)
    cond = None
    if act_ids is not None:
        ids = torch.cat([act_ids, torch.full_like(act_ids, dec.guide.null_action)]) if guided else act_ids
        cond = m._frame_cond(ids.contiguous())
    ws = torch.empty(lib.genie_workspace_bytes(cfg, NBK), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    logits = torch.empty(NBK, S, V, dtype=torch.float32, device="cuda")
    samples = torch.empty(BK, S, dtype=torch.int64, device="cuda")
    conf = torch.empty(BK, S, dtype=torch.float32, device="cuda")
    by_conf = dec.mode == L.UNMASK_CONFIDENCE

    def frames_pass(tokens, t, nf, lg):
        return L.call_cond(lib, "genie_frames_pass", cond, cfg, w, tokens.data_ptr(), NBK, t, nf, cache.data_ptr(), cache.numel(),
                           0 if lg is None else lg.data_ptr(), ws.data_ptr(), ws.numel(), st)

    def frame_pass(tokens, t, lg):
        L.check(L.call_cond(lib, "genie_frame_pass", cond, cfg, w, tokens.data_ptr(), NBK, t, cache.data_ptr(), cache.numel(),
                            0 if lg is None else lg.data_ptr(), ws.data_ptr(), ws.numel(), st), "genie_frame_pass")

    out, opened, merge = [], False, dec.merge_commit
    for k in range(n_new):
        t = P + k
        cur = torch.full((NBK, S), c.image_vocab_size, dtype=torch.int64, device="cuda")
        unmasked = torch.zeros(BK, S, dtype=torch.uint8, device="cuda")
        for step in range(steps):
            if not (step == 0 and opened):
                frame_pass(cur, t, logits)
            last = step == steps - 1
            u = uni[k, step].contiguous() if temperature > 1e-8 else None
            nz = None if (last or dec.unmask_mode == "greedy") else noise[k, step].contiguous()
            keys_out = conf if (by_conf and not last) else None
            anneal = 1.0 - (step + 1) / steps
            tail = (dec.law, 0 if keys_out is None else keys_out.data_ptr(), 0 if nz is None else nz.data_ptr(), anneal)
            if guided:
                L.check(lib.genie_sample_guided(cfg, logits[:BK].data_ptr(), logits[BK:].data_ptr(), L.LAYOUT_TOKEN_MAJOR, BK, float(temperature),
                                                0 if u is None else u.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, *tail,
                                                dec.guide.scale), "genie_sample_guided")
            else:
                L.check(lib.genie_sample_ex(cfg, logits.data_ptr(), L.LAYOUT_TOKEN_MAJOR, BK, float(temperature), 0 if u is None else u.data_ptr(),
                                            samples.data_ptr(), conf.data_ptr(), st, *tail), "genie_sample_ex")
            keys = None if last else (nz if dec.unmask_mode == "random" else conf)
            n = 0 if last else math.ceil(math.cos((step + 1) / steps * math.pi / 2) * S)
            L.check(lib.genie_mask_step(0 if keys is None else keys.data_ptr(), n, int(last), c.image_vocab_size, unmasked.data_ptr(),
                                        samples.data_ptr(), cur.data_ptr(), S, BK, S, st), "genie_mask_step")
            if guided:
                cur[BK:] = cur[:BK]
        out.append(cur[:BK].clone())
        opened = False
        if k + 1 < n_new:
            if merge:
                two = torch.stack([cur, torch.full_like(cur, c.image_vocab_size)], dim=1).contiguous()
                rc = frames_pass(two, t, 2, logits)
                if rc == L.E_UNSUPPORTED:
                    merge = False
                else:
                    L.check(rc, "genie_frames_pass")
                    opened = True
            if not opened:
                frame_pass(cur, t, None)
    return torch.stack(out, dim=1).view(B, K, n_new, S), cache, merge


def fanout_vs_replicated(m, prompt, K, n_new, temperature=1.0, steps=STEPS, acts=None, pacts=None, guidance=None, merge_commit=True, mode="random",
                         seed=3):
    cfg = m.config
    B, P = prompt.shape[:2]
    noise, uni = draws(cfg, n_new, B * K, steps=steps, seed=seed)
    gen, trunk, branch, act_ids, dec = run_fanout(m, prompt, K, n_new, temperature, noise, uni, steps, acts, pacts, guidance, merge_commit, mode,
                                                  mode_kw(mode)["sampling"])
    want, cache, merged = replicated_oracle(m, trunk, B, K, P, n_new, temperature, noise, uni, dec, act_ids)
    check(gen, want, cfg)
    NBK = B * K * (1 if dec.guide is None else 2)
    if n_new > 1:      # the slots the loop commits (the last slot is never committed)
        got, ref = slots(branch, m, NBK, n_new)[:, :, :n_new - 1], slots(cache, m, NBK, cfg.T)[:, :, P:P + n_new - 1]
        assert torch.equal(got, ref), f"{int((got != ref).sum())} of {got.numel()} cache values differ"
    assert len({tuple(gen[b, k].flatten().tolist()) for b in range(B) for k in range(K)}) > B or temperature == 0.0   # branches do differ
    return gen, merged


# ------------------------------------------------------------------ 1: K = 1 is today's call
@pytest.mark.parametrize("mode", ["random", "greedy", "confidence"])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_one_branch_is_generate_frames_cached(precision, temperature, mode):
    G = pkg("generate")
    cfg, m, ex, _ = model(precision)
    P = 3
    N = cfg.T - P
    noise, uni = draws(cfg, N, ex.shape[0], seed=6)
    got = G.fanout_frames(m, ex[:, :P], N, K=1, maskgit_steps=STEPS, temperature=temperature, noise=noise, uniforms=uni, **mode_kw(mode))
    assert got.shape == (3, 1, N, 4, 4)
    want = G.generate_frames_cached(m, ex, P, STEPS, temperature, noise=noise, uniforms=uni, **mode_kw(mode))[:, P:cfg.T]
    check(got[:, 0], want, cfg)


def test_one_branch_under_guidance_with_actions():
    G = pkg("generate")
    cfg, m, ex, _ = model("exact", 5)
    P, B = 3, ex.shape[0]
    N = cfg.T - P
    acts = torch.randint(0, 4, (B, cfg.T), generator=torch.Generator().manual_seed(9)).cuda()
    noise, uni = draws(cfg, N, B, seed=8)
    gd = pkg("sampling").Guidance(3.0, 4)
    got = m.fanout(ex[:, :P], N, action_ids=acts[:, P:].reshape(B, 1, N), prompt_actions=acts[:, :P], maskgit_steps=STEPS, temperature=1.0,
                   noise=noise, uniforms=uni, guidance=gd)
    want = G.generate_frames_cached(m, ex, P, STEPS, 1.0, noise=noise, uniforms=uni, action_ids=acts, guidance=gd)[:, P:cfg.T]
    check(got[:, 0], want, cfg)


# ------------------------------------------------------------------ 2: K = 3 against the replicated cache
def branch_actions(B, K, P, n_new, A, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, A, (B, K, n_new), generator=g).cuda(), torch.randint(0, A, (B, P), generator=g).cuda()


@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_three_branches_equal_the_replicated_batch(precision):
    """B = 2, P = 3, n_new = 4 on the T = 8 model, per-branch actions."""
    cfg, m, ex, _ = model(precision, 5)
    acts, pacts = branch_actions(2, 3, 3, 4, 5)
    gen, _ = fanout_vs_replicated(m, ex[:2, :3], 3, 4, acts=acts, pacts=pacts)
    # the actions of a branch reach that branch alone
    other = acts.clone()
    other[:, 1] = (acts[:, 1] + 1) % 5
    noise, uni = draws(cfg, 4, 6)
    gen2 = run_fanout(m, ex[:2, :3], 3, 4, 1.0, noise, uni, acts=other, pacts=pacts)[0]
    assert torch.equal(gen2[:, 0], gen[:, 0]) and torch.equal(gen2[:, 2], gen[:, 2]) and not torch.equal(gen2[:, 1], gen[:, 1])


def test_three_branches_with_qk_norm():
    """qk-norm: the general path of the `single` kernel (no one-pass scores), trunk and branch slots normalised on read."""
    cfg, m, clips = shaped_model("exact", qk_norm=True)
    fanout_vs_replicated(m, clips[:, :3], 3, 4)


def test_three_branches_under_guidance():
    """Trunk [cond ; null] of 2 B clips, branches [cond B K ; null B K]: parent i / K in both halves."""
    cfg, m, ex, _ = model("exact", 5)
    acts, pacts = branch_actions(2, 3, 3, 4, 4, seed=10)
    fanout_vs_replicated(m, ex[:2, :3], 3, 4, acts=acts, pacts=pacts, guidance=pkg("sampling").Guidance(3.0, 4))


# ------------------------------------------------------------------ 3: edges
EDGES = {"P1": dict(P=1, n_new=4), "last_slot": dict(P=7, n_new=1), "short": dict(P=3, n_new=2), "no_merge": dict(P=3, n_new=4, merge_commit=False),
         "three_steps": dict(P=3, n_new=3, steps=3)}


@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(edge, precision):
    cfg, m, ex, _ = model(precision)
    kw = dict(EDGES[edge])
    P, n_new = kw.pop("P"), kw.pop("n_new")
    fanout_vs_replicated(m, ex[:2, :P], 2, n_new, seed=12, **kw)


# ------------------------------------------------------------------ 4: the fragment-order kernels
@pytest.mark.parametrize("heads", [2, 4])
def test_fragment_order_path(heads):
    """d 128, T 16, S 256 in f16x3, heads of 64 and of 32; B = 1, K = 3, P = 5: the trunk / branch boundary falls inside a 4-frame and an
    8-frame load group of attn_temporal_fr_kernel.  1,536 rows per merged pass: the two-frame passes run."""
    cfg, m, clips = shaped_model("f16x3", heads=heads, d=128, T=16, S=256)
    _, merged = fanout_vs_replicated(m, clips[:1, :5], 3, 3, seed=7)
    assert merged, "the merged two-frame passes did not run: the fragment-order kernels do not cover this model"


# ------------------------------------------------------------------ 5: T = 32
def test_long_window_general_path():
    """T = 32 in exact, P = 18, n_new = 2: t >= 16, the general path of the `single` kernel, over a trunk longer than 16 slots -- without
    qk-norm, and with it (trunk and branch slots normalised on read).  The replicated oracle runs the ordinary flavour of the kernel, the
    fan-out call the other."""
    for qk_norm in (False, True):
        cfg, m, clips = shaped_model("exact", T=32, qk_norm=qk_norm)
        fanout_vs_replicated(m, clips[:, :18], 3, 2, seed=13)


# ------------------------------------------------------------------ 6: the kernel alone
@pytest.mark.parametrize("in16", [0, 1])
@pytest.mark.parametrize("Dh", [8, 16, 32, 64])
def test_decode_attention_kernel_alone(Dh, in16):
    """genie_temporal_attention_decode_fanout on random trunk / branch slices == the same entry point on the dense replicated cache
    (K = 1, P0 = 0, Tb = T), bit for bit: K = 1 and 4, P0 = 0, inside the window and = t, t < 16 with and without qk-norm (one-pass and
    general path), t >= 16.  H = 3 heads and S = 5 positions: the last workgroup is partly idle."""
    L = pkg("_lib")
    lib = L.load()
    H, S, NB = 3, 5, 2
    d = H * Dh
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(100 + Dh + in16)

    def rand(*shape):
        x = torch.randn(*shape, generator=g).cuda()
        return x.to(torch.bfloat16).view(torch.int16) if in16 else x

    for T, t, qk_norm in ((8, 5, False), (8, 5, True), (32, 20, False), (32, 31, True)):
        cfg = L.GenieCfg(num_layers=1, num_heads=H, head_dim=Dh, d_model=d, T=T, S=S, qk_norm=int(qk_norm), attn_scale=Dh ** -0.5)
        nw, nb = (1.0 + 0.1 * torch.randn(Dh, generator=g)).cuda(), (0.1 * torch.randn(Dh, generator=g)).cuda()
        aw = L.AttnWeights(norm_w=nw.data_ptr(), norm_b=nb.data_ptr())
        for K in (1, 4):
            for P0 in (0, 3, t):
                Tb = t - P0 + 1
                NBK = NB * K
                trunk, branch = rand(NB, T, S, 3 * d), rand(NBK, Tb, S, 3 * d)
                dense = rand(NBK, T, S, 3 * d)
                dense[:, :P0] = trunk[:, :P0].repeat_interleave(K, dim=0)
                dense[:, P0:t + 1] = branch
                out = torch.full((2, NBK, S, d), float("nan"), device="cuda")
                L.check(lib.genie_temporal_attention_decode_fanout(cfg, aw, trunk.data_ptr(), branch.data_ptr(), out[0].data_ptr(), NBK, K, P0, Tb, t,
                                                                   in16, st), "genie_temporal_attention_decode_fanout")
                L.check(lib.genie_temporal_attention_decode_fanout(cfg, aw, None, dense.data_ptr(), out[1].data_ptr(), NBK, 1, 0, T, t, in16, st),
                        "genie_temporal_attention_decode_fanout (dense)")
                assert bool(torch.isfinite(out).all()), (T, t, qk_norm, K, P0)
                assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), (T, t, qk_norm, K, P0)
                if K == 4 and P0 == t and not in16:   # softmax-weighted values, against torch in f64 (a loose sanity bound: no bit oracle here)
                    x = dense.double().view(NBK, T, S, 3, H, Dh)[:, :t + 1]
                    q, k, v = x[:, t, :, 0], x[:, :, :, 1], x[:, :, :, 2]
                    if qk_norm:
                        ln = lambda a: torch.nn.functional.layer_norm(a, (Dh,), nw.double(), nb.double(), 1e-5)   # noqa: E731
                        q, k = ln(q), ln(k)
                    p = torch.softmax(torch.einsum("bshd,btshd->bsht", q, k) * Dh ** -0.5, dim=-1)
                    ref = torch.einsum("bsht,btshd->bshd", p, v).reshape(NBK, S, d)
                    assert float((out[0].double() - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ 7: action vectors
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
def test_action_vectors_equal_ids_on_the_projected_table(precision):
    """action_vectors (B, K, n_new, A) and prompt_action_vectors (B, P, A) == the discrete model whose table is [null row ; NumPy
    projection of the prompt's vectors ; ... of the branches'] on the ids that address it."""
    G = pkg("generate")
    B, K, P, n_new = 2, 3, 3, 4
    args = dict(num_layers=2, num_heads=2, d_model=64, T=8, S=16, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    C = pkg("config").GenieConfig
    c0, ci, cv = C(**args), C(**args, action_vocab_size=1 + B * P + B * K * n_new), C(**args, action_dim=AD)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=31, law="conditioned")
    pw = proj_weights(c0.d_model)
    rng = np.random.default_rng(32)
    pv, bv = rng.standard_normal((B, P, AD)).astype(np.float32), rng.standard_normal((B, K, n_new, AD)).astype(np.float32)
    table = projected_table(pw, np.concatenate([pv.reshape(-1, AD), bv.reshape(-1, AD)]))
    M = pkg("st_mask_git").STMaskGIT
    mi = M(ci, precision=precision).load_numpy_state_dict(dict(sd0, **{"action_embed.weight": table})).to("cuda")
    mv = M(cv, precision=precision).load_numpy_state_dict(dict(sd0, **pw)).to("cuda")
    prompt = dev(pkg("synthetic").make_clips(B, c0, seed=33)).view(B, c0.T, 4, 4)[:, :P]
    noise, uni = draws(c0, n_new, B * K, seed=14)
    kw = dict(maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni)
    got = G.fanout_frames(mv, prompt, n_new, action_vectors=dev(bv), prompt_action_vectors=dev(pv), **kw)
    want = G.fanout_frames(mi, prompt, n_new, action_ids=dev(1 + B * P + np.arange(B * K * n_new).reshape(B, K, n_new)),
                           prompt_actions=dev(1 + np.arange(B * P).reshape(B, P)), **kw)
    check(got, want, c0)
    m0 = M(c0, precision=precision).load_numpy_state_dict(sd0).to("cuda")
    assert not torch.equal(got, G.fanout_frames(m0, prompt, n_new, K=K, **kw))      # and the vectors matter
