"""GPU tests of scoring observed futures (genie_score_logits, genie_score_fanout, generate.score_frames): per-(clip, branch, frame) NLL
over the fan-out cache.

  1. the kernel alone against the NumPy restatement (tests/score_model.py): token NLL within 4 x the f32 restatement's own distance
     from float64 on the same rows, hits exact, the row sum exact, two launches bit-identical;
  2. K = 1 is genie_score_logits of the step-0 logits of the teacher-forced cached loop, bit for bit;
  3. K = 3 is the K = 1 score of the K-times replicated batch, bit for bit;
  4. in `exact`, every frame's NLL against the CPU oracle on the clip masked from that frame on;
  5. every argument error leaves the output buffers untouched."""
import functools
import os

import numpy as np
import pytest

import score_model as SM
from conftest import REPO, pkg
from test_hip_action_vectors import AD, proj_weights, projected_table
from test_hip_fanout import branch_actions, model, shaped_model
from test_hip_sampling import dev, sample_cfg, stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PRECISIONS = ["exact", "f16x3", "bf16"]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} values differ"


def score_logits(cfg, logits_NSV, targets_CS, K, per_token=True):
    """genie_score_logits on contiguous rows (N, S, V) against clip targets (N / K, S) -> (nll (N,), hits (N,), token_nll (N, S))."""
    L = pkg("_lib")
    N, S = logits_NSV.shape[:2]
    assert logits_NSV.is_contiguous() and targets_CS.is_contiguous() and targets_CS.shape == (N // K, S)
    nll = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    hits = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    tok = torch.full((N, S), float("nan"), dtype=torch.float32, device="cuda") if per_token else None
    L.check(L.load().genie_score_logits(cfg, logits_NSV.data_ptr(), targets_CS.data_ptr(), S, K, N, nll.data_ptr(), 1, hits.data_ptr(),
                                        0 if tok is None else tok.data_ptr(), S, stream()), "genie_score_logits")
    return nll, hits, tok


# ------------------------------------------------------------------ 1: the kernel alone
KINDS = ("moderate", "sharp", "argmax")          # clip 0, 1, 2: rows 2 b and 2 b + 1 read clip b's targets


def kernel_rows(vf, nfac, S=16, seed=0):
    """(logits (6, S, V) f32, targets (3, S)): N(0, 2) logits; sharp ones (|logit| ~ 16); N(0, 2) with the target raised above the row's maximum."""
    g = np.random.default_rng(seed + 7 * vf + nfac)
    tg = g.integers(0, vf ** nfac, (3, S))
    lg = 2.0 * g.standard_normal((6, S, nfac * vf))
    lg[2:4] *= 8.0
    tf = SM.factor_targets(tg[2], vf, nfac)
    for r in (4, 5):
        for f in range(nfac):
            lg[r, np.arange(S), f * vf + tf[:, f]] = lg[r, :, f * vf:(f + 1) * vf].max(-1) + 1.0
    return lg.astype(np.float32), tg


@pytest.mark.parametrize("vocab", [(262144, 2), (4096, 2), (262144, 3)], ids=["2x512", "2x64", "3x64"])
def test_kernel_against_the_restatement(vocab):
    cfg = sample_cfg(S=16, image_vocab_size=vocab[0], nv=vocab[1])
    vf, nfac = cfg.factored_vocab, cfg.num_factored
    lg, tg = kernel_rows(vf, nfac)
    nll, hits, tok = score_logits(cfg, dev(lg), dev(tg), 2)
    nll2, hits2, tok2 = score_logits(cfg, dev(lg), dev(tg), 2)
    for a, b, what in ((nll, nll2, "nll"), (hits, hits2, "hits"), (tok, tok2, "token_nll")):
        same_bits(a, b, what + " of two launches")
    n64, h64, t64 = SM.row_scores(lg, tg, 2, vf, nfac, np.float64)
    _, _, t32 = SM.row_scores(lg, tg, 2, vf, nfac, np.float32)
    got = tok.cpu().numpy().astype(np.float64)
    for c, kind in enumerate(KINDS):
        r = slice(2 * c, 2 * c + 2)
        d_kernel, d_f32 = float(np.abs(got[r] - t64[r]).max()), float(np.abs(t32[r].astype(np.float64) - t64[r]).max())
        print(f"{vf}^{nfac} {kind}: kernel {d_kernel:.3e}, f32 restatement {d_f32:.3e} from float64 (token NLL up to {t64[r].max():.1f})")
        assert d_kernel <= 4 * d_f32, (kind, d_kernel, d_f32)
    assert np.array_equal(hits.cpu().numpy(), h64)                       # continuous random logits: no ties
    assert h64[4] == 16 and h64[5] == 16 and h64[:4].max() < 16
    # without token_nll and hits the row sums are the same bits
    L = pkg("_lib")
    alone = torch.empty(6, dtype=torch.float64, device="cuda")
    x, t = dev(lg), dev(tg)
    L.check(L.load().genie_score_logits(cfg, x.data_ptr(), t.data_ptr(), 16, 2, 6, alone.data_ptr(), 1, None, None, 0, stream()), "genie_score_logits")
    same_bits(alone, nll, "nll alone")
    # the row sum: every token NLL of the moderate rows lies in [2^-6, 2^6], so an f64 sum of at most 256 such f32 values is exact in any order
    mod = tok[:2].cpu()
    assert float(mod.min()) >= 2.0 ** -6 and float(mod.max()) <= 2.0 ** 6
    assert torch.equal(nll[:2].cpu(), mod.double().sum(-1))


def test_kernel_strides_and_many_tokens():
    """S = 256 (16 waves of 16 tokens) and S = 5 (one wave), K = 3, strided outputs: nll (N, 2)[:, 1], token_nll rows of S + 3."""
    L = pkg("_lib")
    for S in (256, 5):
        cfg = sample_cfg(S=S)
        g = np.random.default_rng(S)
        lg, tg = (2.0 * g.standard_normal((6, S, 1024))).astype(np.float32), g.integers(0, 262144, (2, S + 9))
        x, t = dev(lg), dev(tg)
        nll = torch.full((6, 2), -1.0, dtype=torch.float64, device="cuda")
        hits = torch.full((6, 2), -1.0, dtype=torch.float64, device="cuda")
        tok = torch.full((6, S + 3), -1.0, dtype=torch.float32, device="cuda")
        L.check(L.load().genie_score_logits(cfg, x.data_ptr(), t.data_ptr(), S + 9, 3, 6, nll[:, 1:].data_ptr(), 2, hits[:, 1:].data_ptr(),
                                            tok.data_ptr(), S + 3, stream()), "genie_score_logits")
        n64, h64, t64 = SM.row_scores(lg, tg[:, :S], 3, 512, 2)
        _, _, t32 = SM.row_scores(lg, tg[:, :S], 3, 512, 2, np.float32)
        assert float((nll[:, 0] + 1).abs().max()) == 0 and float((tok[:, S:] + 1).abs().max()) == 0 and float((hits[:, 0] + 1).abs().max()) == 0
        d_kernel = float(np.abs(tok[:, :S].cpu().numpy().astype(np.float64) - t64).max())
        assert d_kernel <= 4 * float(np.abs(t32.astype(np.float64) - t64).max())
        assert torch.equal(nll[:, 1].cpu(), tok[:, :S].cpu().double().sum(-1)) and np.array_equal(hits[:, 1].cpu().numpy(), h64)


# ------------------------------------------------------------------ the calls
def run_score(m, clip, P, K, acts=None, pacts=None, vecs=None, pvecs=None, merge_commit=True, per_token=True):
    """score_call on sentinel-filled caches -> (nll (B, K, n), hits, token_nll (B, K, n, S))."""
    G = pkg("generate")
    B, P, n, K, pa, ba, pv, bv = G._score_inputs(m, clip, P, K, acts, vecs, pacts, pvecs)
    cfg = m._weights()[0]
    lib = pkg("_lib").load()
    ids = clip.reshape(B, P + n, -1).contiguous()
    cond = G.fanout_cond(m, B, P, K, n, pa, ba, pv, bv, ids.device)
    trunk = torch.full((lib.genie_prefix_cache_bytes(cfg, B),), 0x7F, dtype=torch.uint8, device="cuda")
    branch = torch.full((lib.genie_fanout_branch_bytes(cfg, B, K, n),), 0x7F, dtype=torch.uint8, device="cuda")
    return G.score_call(m, ids, P, K, cond, merge_commit=merge_commit, per_token=per_token, trunk=trunk, branch=branch)


def teacher_forced_logits0(m, clip, P, acts=None, merge_commit=True):
    """logits0_out (B, n, S, V) of genie_generate_cached_ex(steps = 1, temperature = 0, teacher_force_time = 1) on clip (B, P + n, H, W)."""
    L = pkg("_lib")
    lib = L.load()
    c = m.config
    cfg, w = m._weights()[:2]
    B, Tc = clip.shape[:2]
    n, S, V = Tc - P, c.S, c.factored_vocab_size * c.num_factored_vocabs
    ids = clip.reshape(B, Tc, S).contiguous()
    cond = m._cond(acts, B, n_frames=Tc)
    ws = m._workspace(B, generate_prompt_frames=P)
    nbytes = lib.genie_prefix_cache_bytes(cfg, B)
    cache = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gen = torch.empty(B, n, S, dtype=torch.int64, device="cuda")
    lg = torch.full((B, n, S, V), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.call_guided(lib, "genie_generate_cached", cond, None, None, cfg, w, ids.data_ptr(), B, P, n, 1, 0.0, L.UNMASK_GREEDY, 0, 0, 1,
                          int(merge_commit), gen.data_ptr(), lg.data_ptr(), cache.data_ptr(), nbytes, ws.data_ptr(), ws.numel(), stream()),
            "genie_generate_cached")
    return lg


# ------------------------------------------------------------------ 2: K = 1 is the teacher-forced cached loop
@pytest.mark.parametrize("with_actions", [False, True], ids=["plain", "actions"])
@pytest.mark.parametrize("merge_commit", [True, False], ids=["merged", "unmerged"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_branch_is_the_teacher_forced_cached_loop(precision, merge_commit, with_actions):
    cfg, m, ex, _ = model(precision, 5 if with_actions else 0)
    B, P = ex.shape[0], 3
    n = cfg.T - P
    acts = torch.randint(0, 5, (B, cfg.T), generator=torch.Generator().manual_seed(9)).cuda() if with_actions else None
    kw = dict(acts=acts[:, P:].reshape(B, 1, n), pacts=acts[:, :P]) if with_actions else {}
    nll, hits, tok = run_score(m, ex, P, 1, merge_commit=merge_commit, **kw)
    lg = teacher_forced_logits0(m, ex, P, acts, merge_commit)
    assert bool(torch.isfinite(lg).all())
    c = m._weights()[0]
    ids = ex.reshape(B, cfg.T, cfg.S)
    for j in range(n):
        want = score_logits(c, lg[:, j].contiguous(), ids[:, P + j].contiguous(), 1)
        for got, w, what in zip((nll, hits, tok), want, ("nll", "hits", "token_nll")):
            same_bits(got[:, 0, j], w, f"{what} of frame {j}")
    assert float(nll.min()) > 0 and 0 <= float(hits.min()) and float(hits.max()) <= cfg.S
    if with_actions:          # and the actions matter
        other = run_score(m, ex, P, 1, acts=(acts[:, P:].reshape(B, 1, n) + 1) % 5, pacts=acts[:, :P], merge_commit=merge_commit)[0]
        assert not torch.equal(other, nll)


def test_score_frames_surface():
    """score_frames / STMaskGIT.score / infer_actions return what score_call computes, in the documented shapes."""
    G = pkg("generate")
    cfg, m, ex, _ = model("exact", 5)
    acts, pacts = branch_actions(2, 3, 3, 4, 5)
    nll, hits, tok = run_score(m, ex[:2, :7], 3, None, acts=acts, pacts=pacts)
    sc = m.score(ex[:2, :7], 3, action_ids=acts, prompt_actions=pacts, per_token=True)
    assert sc.nll.shape == (2, 3, 4) and sc.nll.dtype == torch.float64 and sc.token_nll.shape == (2, 3, 4, 4, 4)
    same_bits(sc.nll, nll, "nll")
    same_bits(sc.hits, hits, "hits")
    same_bits(sc.token_nll.reshape(tok.shape), tok, "token_nll")
    assert G.score_frames(m, ex[:2, :7], 3, action_ids=acts, prompt_actions=pacts).token_nll is None
    best, nll2 = G.infer_actions(m, ex[:2, :7], 3, action_ids=acts, prompt_actions=pacts)
    same_bits(nll2, nll, "infer_actions' nll")
    assert torch.equal(best, nll.sum(-1).argmin(dim=1)) and best.shape == (2,)


# ------------------------------------------------------------------ 3: K = 3 is the replicated batch
def score_vs_replicated(m, clip, P, K, acts=None, pacts=None, merge_commit=True):
    """K branches per clip == the K = 1 score of clip b run as row b * K + k of a B K batch under branch k's actions."""
    B, n = clip.shape[0], clip.shape[1] - P
    got = run_score(m, clip, P, K, acts=acts, pacts=pacts, merge_commit=merge_commit)
    rep = clip.repeat_interleave(K, dim=0).contiguous()
    kw = {} if acts is None else dict(acts=acts.reshape(B * K, 1, n), pacts=pacts.repeat_interleave(K, dim=0).contiguous())
    want = run_score(m, rep, P, 1, merge_commit=merge_commit, **kw)
    for g, w, what in zip(got, want, ("nll", "hits", "token_nll")):
        same_bits(g, w.view(g.shape), what)
    return got


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_branches_equal_the_replicated_batch(precision):
    """B = 2, P = 3, n = 4 on the T = 8 model, per-branch actions; a branch's actions reach that branch alone."""
    cfg, m, ex, _ = model(precision, 5)
    acts, pacts = branch_actions(2, 3, 3, 4, 5)
    nll = score_vs_replicated(m, ex[:2, :7], 3, 3, acts, pacts)[0]
    other = acts.clone()
    other[:, 1] = (acts[:, 1] + 1) % 5
    nll2 = run_score(m, ex[:2, :7], 3, 3, acts=other, pacts=pacts)[0]
    assert torch.equal(nll2[:, 0], nll[:, 0]) and torch.equal(nll2[:, 2], nll[:, 2]) and not torch.equal(nll2[:, 1], nll[:, 1])


def test_three_branches_with_qk_norm():
    cfg, m, clips = shaped_model("exact", qk_norm=True)
    score_vs_replicated(m, clips[:, :7], 3, 3)


EDGES = {"P1": dict(P=1, n=4), "last_slot": dict(P=7, n=1), "short": dict(P=3, n=2), "no_merge": dict(P=3, n=4, merge_commit=False)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(edge, precision):
    """P = 1; P = T - 1 (n = 1: nothing is committed); n < T - P; the unmerged loop."""
    cfg, m, ex, _ = model(precision)
    kw = dict(EDGES[edge])
    P, n = kw.pop("P"), kw.pop("n")
    score_vs_replicated(m, ex[:2, :P + n], P, 2, **kw)


@pytest.mark.parametrize("heads", [2, 4])
def test_fragment_order_path(heads):
    """d 128, T 16, S 256 in f16x3, heads of 64 and of 32, K = 3, P = 5: the trunk / branch boundary falls inside a 4-frame and an 8-frame
    load group of the fragment-order decode attention, and the merged two-frame passes run.
    B = 4: the library picks the GEMM kernels of a pass by its row count (register-direct below 2,048 rows, LDS-tiled from there, the
    out-projections from 4,096), and the two families differ in accumulation order.  The context of B clips runs 1,280 B rows, that of the
    replicated batch 3,840 B: only B = 4 (5,120 and 15,360 rows, under the 16,384-row cut) puts both on the same kernels, which is what
    bit equality with the replicated batch needs.  (At B = 1 -- 1,280 against 3,840 rows -- the two differ by 1e-6 in an NLL of 3,600.)"""
    cfg, m, _ = shaped_model("f16x3", heads=heads, d=128, T=16, S=256)
    clips = dev(pkg("synthetic").make_clips(4, cfg, seed=77)).view(4, cfg.T, 16, 16)
    merged = score_vs_replicated(m, clips[:, :8], 5, 3)
    assert float(merged[0].min()) > 0 and merged[0].shape == (4, 3, 3)
    # B = 1, the geometry of the fan-out test: one branch is the teacher-forced loop there too, and equal hypotheses score equal bits
    one = run_score(m, clips[:1, :8], 5, 1)
    lg = teacher_forced_logits0(m, clips[:1, :8], 5)
    ids = clips[:1, :8].reshape(1, 8, cfg.S)
    for j in range(3):
        want = score_logits(m._weights()[0], lg[:, j].contiguous(), ids[:, 5 + j].contiguous(), 1)
        for got, w, what in zip(one, want, ("nll", "hits", "token_nll")):
            same_bits(got[:, 0, j], w, f"{what} of frame {j}")
    three = run_score(m, clips[:1, :8], 5, 3)
    for g in three:
        assert torch.equal(bits(g[:, 0]), bits(g[:, 1])) and torch.equal(bits(g[:, 0]), bits(g[:, 2]))


def test_long_window_general_path():
    """T = 32 in exact, P = 18, n = 2: t >= 16, the general path of the decode attention over a trunk longer than 16 slots."""
    cfg, m, clips = shaped_model("exact", T=32)
    score_vs_replicated(m, clips[:, :20], 18, 3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_action_vectors_equal_ids_on_the_projected_table(precision):
    """action_vectors (B, K, n, A) and prompt_action_vectors (B, P, A) == the discrete model whose table is [null row ; NumPy projection
    of the prompt's vectors ; ... of the branches'] on the ids that address it."""
    B, K, P, n = 2, 3, 3, 4
    args = dict(num_layers=2, num_heads=2, d_model=64, T=8, S=16, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    C = pkg("config").GenieConfig
    c0, ci, cv = C(**args), C(**args, action_vocab_size=1 + B * P + B * K * n), C(**args, action_dim=AD)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=31, law="conditioned")
    pw = proj_weights(c0.d_model)
    rng = np.random.default_rng(32)
    pv, bv = rng.standard_normal((B, P, AD)).astype(np.float32), rng.standard_normal((B, K, n, AD)).astype(np.float32)
    table = projected_table(pw, np.concatenate([pv.reshape(-1, AD), bv.reshape(-1, AD)]))
    M = pkg("st_mask_git").STMaskGIT
    mi = M(ci, precision=precision).load_numpy_state_dict(dict(sd0, **{"action_embed.weight": table})).to("cuda")
    mv = M(cv, precision=precision).load_numpy_state_dict(dict(sd0, **pw)).to("cuda")
    clip = dev(pkg("synthetic").make_clips(B, c0, seed=33)).view(B, c0.T, 4, 4)[:, :P + n]
    got = run_score(mv, clip, P, None, vecs=dev(bv), pvecs=dev(pv))
    want = run_score(mi, clip, P, None, acts=dev(1 + B * P + np.arange(B * K * n).reshape(B, K, n)), pacts=dev(1 + np.arange(B * P).reshape(B, P)))
    for g, w, what in zip(got, want, ("nll", "hits", "token_nll")):
        same_bits(g, w, what)
    m0 = M(c0, precision=precision).load_numpy_state_dict(sd0).to("cuda")
    assert not torch.equal(got[0], run_score(m0, clip, P, K)[0])            # and the vectors matter


# ------------------------------------------------------------------ 4: against the oracle, in exact
def parity_logit_tolerance(ref_logits):
    """The absolute logit tolerance tests/test_hip_parity.py applies in `exact` (test_compute_logits_golden): 5e-5 * max(1, max |ref| / 8),
    read from that file."""
    src = open(os.path.join(REPO, "tests", "test_hip_parity.py")).read()
    assert 'scale = max(1.0, float(np.abs(z["logits"]).max()) / 8)' in src and 'assert np.abs(lg - z["logits"]).max() < 5e-5 * scale' in src
    return 5e-5 * max(1.0, float(np.abs(ref_logits).max()) / 8)


@functools.lru_cache(maxsize=None)
def oracle_case():
    """B = 2, K = 2, P = 3, n = 3 on the tiny action-conditioned model: -> (nll, hits, token_nll) of the call and the oracle's float64
    (nll (B, K, n), its logit tolerance per (b, k, j))."""
    from oracle import genie_oracle as O
    from test_hip_actions import fold
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=8, S=16, num_factored_vocabs=2, qk_norm=False, use_mup=False,
                                    action_vocab_size=5)
    sd = pkg("synthetic").make_state_dict(cfg, seed=41, law="conditioned")
    sd["action_embed.weight"] = (0.5 * np.random.default_rng(42).standard_normal(sd["action_embed.weight"].shape)).astype(np.float32)
    m = pkg("st_mask_git").STMaskGIT(cfg, precision="exact").load_numpy_state_dict(sd).to("cuda")
    ex = dev(pkg("synthetic").make_clips(2, cfg, seed=43)).view(2, cfg.T, 4, 4)
    B, K, P, n = 2, 2, 3, 3
    acts, pacts = branch_actions(B, K, P, n, 5, seed=21)
    got = run_score(m, ex[:B, :P + n], P, None, acts=acts, pacts=pacts)
    clip = ex[:B].cpu().numpy()
    vf, nfac = cfg.factored_vocab_size, cfg.num_factored_vocabs
    ref, tol = np.zeros((B, K, n)), np.zeros((B, K, n))
    for b in range(B):
        for k in range(K):
            a = np.zeros(cfg.T, np.int64)
            a[:P], a[P:P + n] = pacts[b].cpu().numpy(), acts[b, k].cpu().numpy()
            sdk = fold(sd, sd["action_embed.weight"], a)
            for j in range(n):
                x = clip[b:b + 1].copy()
                x[:, P + j:] = cfg.image_vocab_size
                lg = O.compute_logits(x, sdk, cfg)[0, :, P + j].reshape(-1, cfg.S).T          # (S, V) of slot P + j
                ref[b, k, j] = SM.token_nll(lg, clip[b, P + j].reshape(-1), vf, nfac).sum()
                tol[b, k, j] = parity_logit_tolerance(lg)
    return cfg, got, ref, tol


def test_against_the_oracle():
    """Per frame |nll - oracle| <= 2 S a, a = the absolute logit tolerance of tests/test_hip_parity.py in `exact`: log-sum-exp and the
    target term are each 1-Lipschitz in the max norm of a token's logits, per token (the factors split one token's logits)."""
    cfg, got, ref, tol = oracle_case()
    err = np.abs(got[0].cpu().numpy() - ref)
    print(f"score vs oracle: max |d nll| {err.max():.3e} per frame against a bound of {(2 * cfg.S * tol).min():.3e}; nll {ref.min():.2f} .. {ref.max():.2f}")
    assert (err <= 2 * cfg.S * tol).all(), (err.max(), tol)
    assert len({round(v, 6) for v in ref[:, :, -1].flatten()}) == ref[:, :, -1].size       # the hypotheses do differ


# ------------------------------------------------------------------ 5: refusals
def test_refusals_leave_the_outputs_untouched():
    """The refusals tests/test_score_cpu.py lists (checked there on the host alone), replayed on real device buffers filled with a
    sentinel: GENIE_E_ARG, and nothing was written."""
    from test_score_cpu import REFUSALS, refused_call
    L = pkg("_lib")
    lib = L.load()
    cfg_py, m, ex, _ = model("exact")
    cfg, w = m._weights()[:2]
    B, K, P, n, S = 2, 3, 3, 4, cfg_py.S
    assert cfg_py.T == 8
    ids = ex[:B, :P + n].reshape(B, P + n, S).contiguous()
    nll = torch.full((B, K, n), -7.0, dtype=torch.float64, device="cuda")
    hits = torch.full((B, K, n), -7.0, dtype=torch.float64, device="cuda")
    tok = torch.full((B, K, n, S), -7.0, dtype=torch.float32, device="cuda")
    sizes = dict(trunk=lib.genie_prefix_cache_bytes(cfg, B), branch=lib.genie_fanout_branch_bytes(cfg, B, K, n),
                 ws=lib.genie_score_workspace_bytes(cfg, B, K, P))
    bufs = {k: torch.full((v,), 0x7F, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    table = torch.zeros(5, cfg_py.d_model, device="cuda")
    ptrs = dict(w=w, ids=ids.data_ptr(), nll=nll.data_ptr(), hits=hits.data_ptr(), tok=tok.data_ptr(), table=table.data_ptr(),
                **{k: b.data_ptr() for k, b in bufs.items()})
    for case, word in REFUSALS:
        assert refused_call(L, lib, cfg, ptrs, case, stream()) == L.E_ARG, (case, lib.genie_last_error())
        assert word in lib.genie_last_error(), (case, lib.genie_last_error())
    cfg1 = sample_cfg(S=S)
    x = torch.zeros(6, S, 1024, device="cuda")
    for kw in (dict(K=0), dict(N=0), dict(nstride=0), dict(tstride=-1), dict(kstride=S - 1), dict(off=4)):
        rc = lib.genie_score_logits(cfg1, x.data_ptr() + kw.get("off", 0), ids.data_ptr(), kw.get("tstride", S), kw.get("K", 2), kw.get("N", 6),
                                    nll.data_ptr(), kw.get("nstride", 1), hits.data_ptr(), tok.data_ptr(), kw.get("kstride", S), stream())
        assert rc == L.E_ARG, (kw, lib.genie_last_error())
    torch.cuda.synchronize()
    assert float((nll + 7).abs().max()) == 0 and float((hits + 7).abs().max()) == 0 and float((tok + 7).abs().max()) == 0
    for k, b in bufs.items():
        assert bool((b == 0x7F).all()), k
    # ... and the same buffers do take the good call
    L.check(refused_call(L, lib, cfg, ptrs, {}, stream()), "genie_score_fanout")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nll).all()) and float(nll.min()) > 0
