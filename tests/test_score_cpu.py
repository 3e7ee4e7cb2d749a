"""CPU-only tests of scoring observed futures (genie_score_fanout, generate.score_frames): the NumPy restatement of the per-token
arithmetic (tests/score_model.py) against float64 torch cross-entropy, the Python input checks, infer_actions' argmin, the ctypes
declarations against the header, and the host-side argument errors of the C ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import score_model as SM
from conftest import REPO, pkg

torch = pytest.importorskip("torch")

NEW = ("genie_score_logits", "genie_score_workspace_bytes", "genie_score_fanout")


def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def small_cfg(**kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=8, S=16, num_factored_vocabs=2, qk_norm=False)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


# ------------------------------------------------------------------ the restatement
def rows(kind, vf, nfac, n=40, seed=0):
    """(logits (n, nfac * vf) f32, targets (n,)): random N(0, 2), sharp (|logit| ~ 16) or near-one-hot on the target."""
    g = np.random.default_rng(seed + vf + nfac)
    tg = g.integers(0, vf ** nfac, n)
    if kind == "random":
        lg = 2.0 * g.standard_normal((n, nfac * vf))
    elif kind == "sharp":
        lg = 16.0 * g.standard_normal((n, nfac * vf))
    else:
        lg = g.standard_normal((n, nfac * vf))
        tf = SM.factor_targets(tg, vf, nfac)
        for f in range(nfac):
            lg[np.arange(n), f * vf + tf[:, f]] += 40.0
    return lg.astype(np.float32), tg


@pytest.mark.parametrize("vf,nfac", [(512, 2), (64, 2), (64, 3), (100, 2)])
@pytest.mark.parametrize("kind", ["random", "sharp", "one_hot"])
def test_restatement_is_float64_cross_entropy(kind, vf, nfac):
    lg, tg = rows(kind, vf, nfac)
    tf = SM.factor_targets(tg, vf, nfac)
    want = sum(torch.nn.functional.cross_entropy(torch.from_numpy(lg[:, f * vf:(f + 1) * vf]).double(), torch.from_numpy(tf[:, f]),
                                                 reduction="none") for f in range(nfac)).numpy()
    got64 = SM.token_nll(lg, tg, vf, nfac, np.float64)
    assert got64.dtype == np.float64
    mag = max(1.0, float(np.abs(lg).max()))
    assert np.abs(got64 - want).max() <= 64 * np.finfo(np.float64).eps * mag * nfac       # two f64 evaluations of one formula
    got32 = SM.token_nll(lg, tg, vf, nfac, np.float32)
    assert got32.dtype == np.float32
    # f32: a handful of roundings at the magnitude of the largest logit per factor
    assert np.abs(got32.astype(np.float64) - want).max() <= 8 * np.finfo(np.float32).eps * mag * nfac
    want_hit = np.stack([torch.from_numpy(lg[:, f * vf:(f + 1) * vf]).argmax(-1).numpy() == tf[:, f] for f in range(nfac)]).all(0)
    assert np.array_equal(SM.token_hits(lg, tg, vf, nfac), want_hit)
    if kind == "one_hot":
        assert want_hit.all() and float(got64.max()) < 1e-10
    clips = tg[:20].reshape(4, 5)                  # rows 2 b and 2 b + 1 read clip b's targets
    nll, hits, tok = SM.row_scores(lg.reshape(8, 5, -1), clips, 2, vf, nfac)
    assert np.array_equal(nll, tok.sum(-1)) and np.array_equal(tok[3], SM.token_nll(lg.reshape(8, 5, -1)[3], clips[1], vf, nfac))
    assert hits.shape == (8,)


def test_first_max_wins():
    lg = np.zeros((1, 128), np.float32)
    lg[0, [3, 9]] = 1.0            # factor 0 ties at 3 and 9
    lg[0, 64 + 5] = 2.0
    assert SM.token_hits(lg, np.array([3 + 64 * 5]), 64, 2)[0] and not SM.token_hits(lg, np.array([9 + 64 * 5]), 64, 2)[0]


# ------------------------------------------------------------------ the ABI
def test_new_symbols_are_exported_and_declared_with_the_headers_arity():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    assert "GENIE_ABI_VERSION 3" in header
    for n in NEW:
        decl = re.search(r"^(?:int|size_t) " + n + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl, n
        assert hasattr(L, n) and len(lib_mod.SIGNATURES[n][1]) == decl.group(1).count(",") + 1, n
    G = pkg("generate")
    for n in ("score_frames", "score_call", "infer_actions", "_score_inputs", "Score"):
        assert hasattr(G, n), n
    assert hasattr(pkg("st_mask_git").STMaskGIT, "score")


# Every way genie_score_fanout is refused, as overrides of a good call at B = 2, K = 3, P = 3, n = 4 on a T = 8 model: integers by name,
# "null": the pointer to pass as NULL, "short": the buffer whose size is given one byte too small, "bad_cond": an action condition
# without ids.  tests/test_hip_score.py replays the same list on real device buffers.
REFUSALS = ((dict(K=0), b"K=0"), (dict(K=-1), b"K=-1"), (dict(B=0), b"B=0"), (dict(P=0), b"prompt"), (dict(n=0), b"scored frames"),
            (dict(P=5, n=4), b"of at most 8"), (dict(P=8, n=1), b"of at most 8"), (dict(B=1 << 20, K=1 << 20), b"too many"),
            (dict(null="ids"), b"NULL pointer"), (dict(null="nll"), b"NULL pointer"), (dict(null="trunk"), b"NULL pointer"),
            (dict(null="branch"), b"NULL pointer"), (dict(null="ws"), b"NULL pointer"), (dict(null="w"), b"NULL pointer"),
            (dict(short="trunk"), b"trunk cache too small"), (dict(short="branch"), b"branch cache too small"),
            (dict(short="ws"), b"workspace too small"), (dict(bad_cond=True), b"score_fanout"))


def refused_call(lib_mod, L, cfg, ptrs, case, stream=None):
    """genie_score_fanout under one entry of REFUSALS.  ptrs: cfg-independent addresses by name (w, ids, nll, hits, tok, trunk, branch, ws,
    table); the buffer sizes are the library's own for the good call's shape."""
    assert not set(case) - {"B", "K", "P", "n", "null", "short", "bad_cond"}, case
    B, K, P, n = 2, 3, 3, 4
    size = dict(trunk=L.genie_prefix_cache_bytes(cfg, B), branch=L.genie_fanout_branch_bytes(cfg, B, K, n),
                ws=L.genie_score_workspace_bytes(cfg, B, K, P))
    assert min(size.values()) > 0
    if "short" in case:
        size[case["short"]] -= 1
    p = dict(ptrs)
    if "null" in case:
        p[case["null"]] = None
    cond = lib_mod.FrameCond(table=p["table"], ids=None, n_actions=5) if case.get("bad_cond") else None
    return L.genie_score_fanout(cfg, p["w"], p["ids"], case.get("B", B), case.get("K", K), case.get("P", P), case.get("n", n), 1, p["nll"],
                                p["hits"], p["tok"], p["trunk"], size["trunk"], p["branch"], size["branch"], p["ws"], size["ws"], stream, cond)


def test_score_entry_points_reject_bad_arguments_before_any_hip_call():
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())           # T = 8, S = 16
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    E, fake = lib_mod.E_ARG, 1 << 20
    ptrs = dict(w=w, ids=fake, nll=fake, hits=fake, tok=fake, trunk=fake, branch=fake, ws=fake, table=fake)
    for case, word in REFUSALS:
        assert refused_call(lib_mod, L, cfg, ptrs, case) == E, (case, L.genie_last_error())
        assert word in L.genie_last_error(), (case, L.genie_last_error())
    assert L.genie_score_fanout(None, w, fake, 2, 3, 3, 4, 1, fake, fake, fake, fake, 1 << 40, fake, 1 << 40, fake, 1 << 40, None, None) != 0

    def one(K=2, N=6, logits=fake, targets=fake, tstride=16, nll=fake, nstride=1, tok=None, kstride=16):
        return L.genie_score_logits(cfg, logits, targets, tstride, K, N, nll, nstride, None, tok, kstride, None)

    for kw in (dict(K=0), dict(N=0), dict(N=1 << 31), dict(logits=None), dict(targets=None), dict(nll=None), dict(tstride=-1), dict(nstride=0),
               dict(tok=fake, kstride=15), dict(logits=fake + 4)):
        assert one(**kw) == E, (kw, L.genie_last_error())
    # the workspace: that of the fan-out loop on the same shape, 0 on bad arguments
    assert L.genie_score_workspace_bytes(cfg, 2, 3, 3) == L.genie_fanout_workspace_bytes(cfg, 2, 3, 3, 0) > 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 8), (1 << 20, 1 << 20, 1)):
        assert L.genie_score_workspace_bytes(cfg, *bad) == 0, bad
    assert L.genie_score_workspace_bytes(None, 1, 1, 1) == 0


# ------------------------------------------------------------------ the Python surface
def test_score_inputs(monkeypatch):
    G = pkg("generate")
    M = pkg("st_mask_git").STMaskGIT
    monkeypatch.setattr(M, "_device", lambda self: torch.device("cpu"))
    m = M(small_cfg())
    clip = torch.zeros(2, 7, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        G.score_frames(m, clip, 3)                                               # an unconditioned model takes K explicitly
    for P in (0, 7, 8, -1):
        with pytest.raises(ValueError):
            G.score_frames(m, clip, P, K=1)                                      # no prompt / nothing to score
    with pytest.raises(ValueError):
        G.score_frames(m, torch.zeros(2, 9, 4, 4, dtype=torch.long), 3, K=1)     # P + n > T
    for K in (0, -2):
        with pytest.raises(ValueError):
            G.score_frames(m, clip, 3, K=K)
    with pytest.raises(RuntimeError):
        G.score_frames(m, torch.zeros(2, 7, 16, dtype=torch.long), 3, K=1)       # not (B, P + n, H, W)
    with pytest.raises(RuntimeError):
        G.score_frames(m, clip.float(), 3, K=1)
    for bad in (-1, m.config.image_vocab_size):                                   # an observed clip holds no mask token
        with pytest.raises(IndexError):
            G.score_frames(m, torch.full((2, 7, 4, 4), bad), 3, K=1)
    with pytest.raises(ValueError):
        m.score(clip, 3, action_ids=torch.zeros(2, 3, 4, dtype=torch.long))      # a model without actions
    ma = M(small_cfg(action_vocab_size=5))
    good, pa = torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        ma.score(clip, 3, K=3)                                                   # actions missing
    with pytest.raises(ValueError):
        ma.score(clip, 3, action_ids=good)                                       # prompt_actions missing
    with pytest.raises(ValueError):
        ma.score(clip, 3, K=2, action_ids=good, prompt_actions=pa)               # K disagrees with the actions
    for bad in (torch.zeros(2, 3, 5, dtype=torch.long), torch.zeros(3, 3, 4, dtype=torch.long), torch.zeros(2, 12, dtype=torch.long)):
        with pytest.raises(RuntimeError):
            ma.score(clip, 3, action_ids=bad, prompt_actions=pa)
    with pytest.raises(IndexError):
        ma.score(clip, 3, action_ids=torch.full((2, 3, 4), 5), prompt_actions=pa)
    with pytest.raises(ValueError):
        ma.score(clip, 3, action_ids=good, prompt_actions=pa, action_vectors=torch.zeros(2, 3, 4, 6))
    mv = M(small_cfg(action_dim=6))
    vec, pv = torch.zeros(2, 3, 4, 6), torch.zeros(2, 3, 6)
    with pytest.raises(ValueError):
        mv.score(clip, 3, action_ids=good, prompt_actions=pa)                    # ids given to a model of action vectors
    with pytest.raises(ValueError):
        mv.score(clip, 3, action_vectors=vec)                                    # prompt_action_vectors missing
    with pytest.raises(RuntimeError):
        mv.score(clip, 3, action_vectors=torch.zeros(2, 3, 5, 6), prompt_action_vectors=pv)
    # what the checks hand on: n from the clip, K from the actions, branch-major rows
    B, P, n, K, a_p, a_b, v_p, v_b = G._score_inputs(ma, clip, 3, None, torch.arange(24).view(2, 3, 4) % 5, None, pa, None)
    assert (B, P, n, K) == (2, 3, 4, 3) and a_b.shape == (6, 4) and a_p.shape == (2, 3) and v_p is None and v_b is None
    assert a_b[4].tolist() == [(16 + j) % 5 for j in range(4)]
    B, P, n, K, a_p, a_b, v_p, v_b = G._score_inputs(mv, clip, 3, None, None, vec, None, pv)
    assert (B, P, n, K) == (2, 3, 4, 3) and a_b is None and v_b.shape == (6, 4, 6) and v_p.shape == (2, 3, 6)
    assert G._score_inputs(m, clip[:, :4], 3, 5, None, None, None, None)[:4] == (2, 3, 1, 5)


def test_infer_actions_takes_the_argmin_of_the_summed_nll(monkeypatch):
    G = pkg("generate")
    nll = torch.tensor([[[1.0, 5.0], [2.0, 2.5], [0.5, 6.0]],
                        [[9.0, 1.0], [3.0, 3.0], [4.0, 4.0]]], dtype=torch.float64)            # sums: [6, 4.5, 6.5], [10, 6, 8]
    seen = {}

    def stub(model, clip, P, **kw):
        seen.update(kw, P=P)
        return G.Score(nll, torch.zeros_like(nll))

    monkeypatch.setattr(G, "score_frames", stub)
    best, got = G.infer_actions(None, None, 3, K=3, merge_commit=False)
    assert best.tolist() == [1, 1] and got is nll and seen == dict(K=3, merge_commit=False, P=3)


def test_tools_list_the_score_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "generate.py"), "--help"], capture_output=True, text=True, check=True)
    assert "--score" in out.stdout
    assert "--score" in open(os.path.join(REPO, "tools", "bench_generate.py")).read()
