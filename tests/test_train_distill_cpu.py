"""Distillation (include/genie_hip.h, "Distillation"), the part that needs no GPU: the yardsticks of tests/distill_model.py against
float64 torch autograd and against each other, the validity condition of the GPU step cases of tests/test_hip_train_distill.py, the
library's refusals (they precede every device call), the struct's layout and the entry points' arity, the trainer's validation, the
CLI's flags, and the compiled kernel's resources.
"""
import ctypes
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distill_model as DS
import objective_model as OM
from conftest import REPO, pkg

GRAD_TOL, LOSS_TOL = 1e-4, 1e-5          # the bars of tests/test_hip_train_geometry.py, restated
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("genie_distill_layout", "genie_train_forward_distill", "genie_ce_distill")

# (n_clips, T, S, vf, nfac): the shapes of the loss-launch test on the GPU; the CPU test takes the same rows
# (the last one: 9,216 tokens, more than the 2,048 four-token groups one launch has workgroups for: some walk a second group)
WINDOW_SHAPES = [(3, 3, 5, 512, 2), (2, 4, 16, 100, 2), (2, 4, 16, 16, 4), (1, 2, 16, 4096, 1), (2, 4, 16, 64, 3), (9, 4, 256, 16, 2)]
# tag -> (alpha, tau, eps, zeta, weighted)
WINDOW_SETTINGS = {"a1t1": (1.0, 1.0, 0.0, 0.0, False), "a05t2": (0.5, 2.0, 0.0, 0.0, False), "a03t05": (0.3, 0.5, 0.0, 0.0, False),
                   "a05t2+obj": (0.5, 2.0, 0.1, 1e-2, True)}


def window_weights(T):
    return tuple((1.0, 0.5, 0.0, 2.0)[t % 4] for t in range(T))


@functools.lru_cache(maxsize=None)
def window_inputs(shape, scale):
    """(student logits f32 (N, nfac * vf), teacher logits f32, ids, labels, mask_id).  About half the ids are the mask id, frame 0
    included.  Rows by index mod 9: 1 one-hot teacher (+80 on each factor's target) against a one-hot student (+80 on ANOTHER class);
    3 uniform (student 0.25, teacher -0.5); 5 both shifted by +1000; 7 the teacher equals the student; the rest random at `scale`,
    student and teacher drawn apart."""
    n_clips, T, S, vf, nfac = shape
    g = np.random.default_rng(2000 * vf + 10 * nfac + int(scale))
    N, mask_id = n_clips * T * S, vf ** nfac
    labels = g.integers(0, mask_id, N)
    ids = np.where(g.random(N) < 0.5, mask_id, g.integers(0, mask_id, N))
    assert (ids.reshape(n_clips, T, S)[:, 0] == mask_id).any() and OM.counted_mask(ids, T, S, mask_id).sum(axis=(0, 2))[1:].all()
    z = (scale * g.standard_normal((N, nfac, vf))).astype(np.float32)
    u = (scale * g.standard_normal((N, nfac, vf))).astype(np.float32)
    row = np.arange(N)
    y = np.stack([(labels // vf ** f) % vf for f in range(nfac)], 1)
    hot = row % 9 == 1
    z[hot] = (0.1 * g.standard_normal((int(hot.sum()), nfac, vf))).astype(np.float32)
    u[hot] = (0.1 * g.standard_normal((int(hot.sum()), nfac, vf))).astype(np.float32)
    for f in range(nfac):
        u[row[hot], f, y[hot, f]] += np.float32(80.0)
        z[row[hot], f, (y[hot, f] + 1) % vf] += np.float32(80.0)
    z[row % 9 == 3] = np.float32(0.25)
    u[row % 9 == 3] = np.float32(-0.5)
    z[row % 9 == 5] += np.float32(1000.0)
    u[row % 9 == 5] += np.float32(1000.0)
    u[row % 9 == 7] = z[row % 9 == 7]
    for a in (z, u, ids, labels):
        a.setflags(write=False)
    return z.reshape(N, nfac * vf), u.reshape(N, nfac * vf), ids, labels, mask_id


def window_args(shape, key):
    alpha, tau, eps, zeta, weighted = WINDOW_SETTINGS[key]
    return dict(alpha=alpha, tau=tau, eps=eps, zeta=zeta, weights=window_weights(shape[1]) if weighted else None)


# ---------------------------------------------------------------------------------------------- 1. the yardsticks
def autograd_window(shape, scale, alpha, tau, eps, zeta, weights):
    """(loss, d logits, kd per token, teacher ce per token) of the window by float64 torch autograd of F.kl_div, F.cross_entropy, logsumexp."""
    import torch
    F = torch.nn.functional
    n_clips, T, S, vf, nfac = shape
    logits, teacher, ids, labels, mask_id = window_inputs(shape, scale)
    N = logits.shape[0]
    a32, t32, e32, z32 = (float(np.float32(v)) for v in (alpha, tau, eps, zeta))
    with torch.enable_grad():
        z = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
        flat = z.reshape(N * nfac, vf)
        uf = torch.from_numpy(teacher.astype(np.float64)).reshape(N * nfac, vf)
        y = torch.from_numpy(np.stack([(labels // vf ** f) % vf for f in range(nfac)], 1).reshape(-1))
        kd = F.kl_div(F.log_softmax(flat / t32, -1), F.softmax(uf / t32, -1), reduction="none").sum(-1) * t32 ** 2
        per = ((1.0 - a32) * F.cross_entropy(flat, y, label_smoothing=e32, reduction="none") + a32 * kd
               + z32 * torch.logsumexp(flat, -1) ** 2).reshape(N, nfac).sum(-1)
        counted = torch.from_numpy(OM.counted_mask(ids, T, S, mask_id).reshape(N))
        w = torch.from_numpy(np.broadcast_to(OM.frame_weights(weights, T)[None, :, None], (n_clips, T, S)).reshape(N).copy())
        loss = (per * w * counted).sum() / (w * counted).sum()
        loss.backward()
        nc = float(counted.sum())
        kd_tok = float((kd.detach().reshape(N, nfac).sum(-1) * counted).sum()) / nc
        tce = float((F.cross_entropy(uf, y, reduction="none").reshape(N, nfac).sum(-1) * counted).sum()) / nc
    return float(loss.detach()), z.grad.numpy(), kd_tok, tce


@pytest.mark.parametrize("key", list(WINDOW_SETTINGS))
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatements_agree_with_autograd(shape, scale, key):
    """ce_distill (float64 closed forms) against float64 torch autograd: loss, kd, teacher_ce and d logits to 1e-12 (of the largest
    element).  ce_distill_f32 (the kernel's order in float32) against ce_distill: d logits to 1e-5 of the largest element (the floor bar
    of tests/test_hip_train_objective.py), the sums to LOSS_TOL, hits, W and n exactly.  No NaN anywhere, the one-hot rows at tau = 0.5
    included (their r_k underflows to 0); on the rows where the teacher equals the student the soft gradient vanishes and kd is 0."""
    n_clips, T, S, vf, nfac = shape
    logits, teacher, ids, labels, mask_id = window_inputs(shape, scale)
    kw = window_args(shape, key)
    d, s = DS.ce_distill(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, **kw)
    loss, ref, kd_tok, tce = autograd_window(shape, scale, kw["alpha"], kw["tau"], kw["eps"], kw["zeta"], kw["weights"])
    assert np.isfinite(d).all() and np.isfinite(s).all() and np.isfinite(ref).all()
    assert abs(s[0] / s[2] - loss) <= 1e-12 * abs(loss)
    assert abs(s[5] / s[4] - kd_tok) <= 1e-12 * abs(kd_tok) and abs(s[6] / s[4] - tce) <= 1e-12 * abs(tce)
    assert np.abs(d - ref).max() <= 1e-12 * np.abs(ref).max()
    d32, s32 = DS.ce_distill_f32(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, **kw)
    assert d32.dtype == np.float32 and np.isfinite(d32).all() and np.isfinite(s32).all()
    err = float(np.abs(d32 - d).max() / np.abs(d).max())
    rel = [abs(a - b) / max(abs(b), 1e-300) for a, b in zip(s32, s)]
    print(f"train_distill/restatement/{'x'.join(map(str, shape))}/s{scale}/{key}: d logits {err:.3e}, sums " + " ".join(f"{r:.1e}" for r in rel))
    assert err < 1e-5 and max(rel) <= LOSS_TOL
    assert s32[1] == s[1] and s32[2] == s[2] and s32[4] == s[4]
    counted = OM.counted_mask(ids, T, S, mask_id).reshape(-1)
    dead = ~counted
    if kw["weights"] is not None:
        dead = dead | (np.broadcast_to(np.asarray(kw["weights"])[None, :, None], (n_clips, T, S)).reshape(-1) == 0.0)
    assert dead.any() and not d[dead].any() and not d32[dead].any()
    # teacher == student: no soft gradient, no kd -- at alpha = 1 without the knobs the whole row vanishes
    same = (np.arange(len(counted)) % 9 == 7) & ~dead
    assert same.any() or len(counted) < 64, "no live row with teacher == student"
    if key == "a1t1" and same.any():
        assert np.abs(d[same]).max() <= 1e-15 and not d32[same].any()
        k = int(same.sum())   # those rows alone, each as frame 1 of a two-frame clip of one token
        two = lambda a: np.repeat(a[same], 2, axis=0)   # noqa: E731
        _, s_same = DS.ce_distill(two(logits), two(teacher), np.full(2 * k, mask_id), two(labels), 2, 1, vf, nfac, mask_id, **kw)
        assert s_same[4] == k and s_same[5] == 0.0


def test_neutral_restatement_is_the_objectives():
    """At alpha = 0 ce_distill is objective_model.ce_objective term for term (d logits and the first five sums to 1e-13)."""
    shape = WINDOW_SHAPES[1]
    n_clips, T, S, vf, nfac = shape
    logits, teacher, ids, labels, mask_id = window_inputs(shape, 1)
    for tau in (1.0, 2.0):
        d, s = DS.ce_distill(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, 0.0, tau, 0.1, 1e-2, window_weights(T))
        d0, s0 = OM.ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id, 0.1, 1e-2, window_weights(T))
        assert np.abs(d - d0).max() <= 1e-13 * np.abs(d0).max() and np.allclose(s[:5], s0, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------- 2. validity of the GPU step cases
def make_case(name):
    import test_hip_train_dropout as TD
    return TD.make_case(name, OM.STEP_CASES[name][0])


@functools.lru_cache(maxsize=None)
def teacher_case(name):
    """(teacher cfg, teacher state dict, its float64-forward logits on the case's input ids rounded to f32 (B, T, S, V))."""
    cfg, _, ids, _ = make_case(name)
    H, d, layers, qk_norm = DS.TEACHERS[name]
    cfg_t = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=cfg.T, S=cfg.S, num_factored_vocabs=2, qk_norm=qk_norm,
                                      num_prompt_frames=cfg.T // 2, use_mup=False)
    sd_t = pkg("synthetic").make_state_dict(cfg_t, seed=177 + d, law="conditioned")
    tl = DS.forward_logits(cfg_t, sd_t, ids).astype(np.float32)
    tl.setflags(write=False)
    return cfg_t, sd_t, tl


@functools.lru_cache(maxsize=None)
def model_step(name, tag, p=0.0, seed=3):
    """The float64 model's step at a setting of DS.STEP_SETTINGS ("none": alpha = 0).  Computed once, shared, never written to."""
    import dropout_model as DM
    cfg, sd, ids, labels = make_case(name)
    alpha, tau, eps, zeta, weights = (0.0, 1.0, 0.0, 0.0, None) if tag == "none" else DS.step_setting(name, tag)
    masks = DM.step_masks(cfg, ids.shape[0], seed, 0, p) if p else None
    return DS.autograd_step(cfg, sd, ids, labels, teacher_case(name)[2], alpha, tau, eps, zeta, weights, masks, float(np.float32(p)))


@pytest.mark.parametrize("tag", list(DS.STEP_SETTINGS))
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_gpu_cases_can_tell_distillation_from_none(name, tag):
    """The validity condition of the step tests of tests/test_hip_train_distill.py: at every setting they use, the float64 model's loss
    differs from the alpha = 0 model's by more than 100 x LOSS_TOL (relative) and EVERY gradient tensor by more than 100 x GRAD_TOL
    (worst element over the alpha = 0 tensor's largest): a step that ignored the teacher would miss the bars by two orders of magnitude.
    At alpha = 0 the model is objective_model.autograd_step's (1e-13)."""
    cfg, sd, ids, labels = make_case(name)
    loss0, grads0, ce0, acc0, kd0, tce0 = model_step(name, "none")
    lo, go_, ceo, acco = OM.autograd_step(cfg, sd, ids, labels)
    assert abs(loss0 - lo) <= 1e-13 * abs(lo) and all(np.abs(grads0[k] - g).max() <= 1e-13 * np.abs(g).max() for k, g in go_.items())
    loss, grads, ce, acc, kd, tce = model_step(name, tag)
    dl = abs(loss - loss0) / abs(loss0)
    moved = {k: float(np.abs(g - grads0[k]).max() / np.abs(grads0[k]).max()) for k, g in grads.items()}
    low = min(moved.items(), key=lambda kv: kv[1])
    print(f"train_distill/validity/{name}/{tag}: loss moves by {dl:.3e}, the least moved tensor {low[0]} by {low[1]:.3e}; kd {kd:.4f}, "
          f"teacher_ce {tce:.4f}, ce {ce:.4f}")
    assert set(grads) == set(grads0)
    assert abs(ce - ce0) <= 1e-13 * ce0 and abs(tce - tce0) <= 1e-13 * tce0 and acc == acc0, "plain CE, teacher CE and acc do not depend on the mix"
    assert kd > 0 and dl > 100 * LOSS_TOL
    assert low[1] > 100 * GRAD_TOL, low


# ---------------------------------------------------------------------------------------------- 3. host side
def test_distill_layout_and_arity():
    """genie_distill as the compiler lays it out against the ctypes declaration (16 bytes, the pointer at 8); the three new entry points
    are exported and declared in _lib.py with the header's arity; the ABI version stays 3."""
    lib = pkg("_lib")
    L = lib.load()
    out = (ctypes.c_size_t * 4)()
    assert L.genie_distill_layout(out, 4) == 4
    D = lib.Distill
    assert list(out) == [ctypes.sizeof(D), D.alpha.offset, D.temperature.offset, D.teacher_logits.offset] == [16, 0, 4, 8]
    short = (ctypes.c_size_t * 2)(7, 7)
    assert L.genie_distill_layout(short, 1) == 4 and list(short) == [16, 7]
    assert L.genie_version() == 3 and lib.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    assert "GENIE_ABI_VERSION 3" in header
    for n in NEW:
        decl = re.search(r"^(?:int|size_t) " + n + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl, n
        assert hasattr(L, n) and len(lib.SIGNATURES[n][1]) == decl.group(1).count(",") + 1, n


def refusals():
    """(what, alpha, temperature, with a teacher pointer) for every GENIE_E_ARG the distillation adds."""
    nan, inf = float("nan"), float("inf")
    return [("alpha < 0", -0.01, 1.0, True), ("alpha > 1", 1.01, 1.0, True), ("alpha nan", nan, 1.0, True),
            ("tau 0", 0.5, 0.0, True), ("tau < 0", 0.5, -1.0, True), ("tau inf", 0.5, inf, True), ("tau nan", 0.5, nan, True),
            ("tau 0 at alpha 0", 0.0, 0.0, True), ("no teacher", 0.5, 1.0, False)]


def test_library_refuses_bad_distillation_before_anything_else():
    """Every refusal is GENIE_E_ARG from genie_ce_distill and genie_train_forward_distill before any other check: here with every other
    pointer NULL, which a later check reports under another message -- no device is needed.  Behind them come the objective's own
    refusals, then the NULL pointers; overlapping buffers are refused with the pointers in place."""
    import test_train_objective_cpu as OC
    lib = pkg("_lib")
    L = lib.load()
    T = 4
    cfg = lib.GenieCfg(T=T)
    one = (ctypes.c_double * 16)()
    p = ctypes.addressof(one)   # never dereferenced: the argument checks come first
    for what, alpha, tau, with_teacher in refusals():
        ds = lib.Distill(alpha=alpha, temperature=tau, teacher_logits=p if with_teacher else None)
        assert L.genie_ce_distill(None, p if with_teacher else None, None, None, 2, T, 16, 512, 2, 262144, None, ds, None, None) == lib.E_ARG, what
        assert b"genie_ce_distill" in L.genie_last_error() and b"NULL" not in L.genie_last_error(), (what, L.genie_last_error())
        assert L.genie_train_forward_distill(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, None, ds) == lib.E_ARG, what
        assert b"genie_train_forward_distill" in L.genie_last_error(), (what, L.genie_last_error())
    good = lib.Distill(alpha=0.5, temperature=2.0, teacher_logits=p)
    for what, ob in OC.refusals(T):
        assert L.genie_ce_distill(None, p, None, None, 2, T, 16, 512, 2, 262144, ob, good, None, None) == lib.E_ARG, what
        assert b"genie_ce_distill" in L.genie_last_error() and b"NULL" not in L.genie_last_error(), (what, L.genie_last_error())
        assert L.genie_train_forward_distill(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, ob, good) == lib.E_ARG, what
        assert b"genie_train_forward_distill" in L.genie_last_error(), (what, L.genie_last_error())
    assert L.genie_ce_distill(None, p, None, None, 2, T, 16, 512, 2, 262144, None, good, None, None) == lib.E_ARG
    assert b"NULL" in L.genie_last_error()
    for n_clips, Tq, S, vf, nfac in ((0, 4, 16, 512, 2), (2, 0, 16, 512, 2), (2, 4, 0, 512, 2), (2, 4, 16, 0, 2), (2, 4, 16, 512, 0),
                                     (2, 4, 16, 512, 5)):
        assert L.genie_ce_distill(p, p + 64, p, p, n_clips, Tq, S, vf, nfac, 1, None, good, p, None) == lib.E_ARG, (n_clips, Tq, S, vf, nfac)
    # overlap: 1 x 1 x 1 tokens of 1 x 4 logits = 16 bytes of logits, 56 bytes of sums
    for what, logits, teacher, sums in (("teacher == logits", p, p, p + 64), ("teacher inside logits", p, p + 8, p + 64),
                                        ("teacher ends in logits", p + 8, p, p + 64), ("teacher in sums", p, p + 64 + 48, p + 64),
                                        ("teacher reaches sums", p, p + 56, p + 64)):
        assert L.genie_ce_distill(logits, teacher, p, p, 1, 1, 1, 4, 1, 4, None, good, sums, None) == lib.E_ARG, what
        assert b"overlap" in L.genie_last_error(), (what, L.genie_last_error())


def test_neutral_struct_is_the_objective_call():
    """ds == NULL and alpha == 0 (with any teacher pointer) hand the arguments to genie_train_forward_obj / genie_ce_objective: with NULL
    buffers the answer is those entry points' own refusal, word for word."""
    lib = pkg("_lib")
    L = lib.load()
    cfg = lib.GenieCfg(T=4)
    ob = lib.Objective(label_smoothing=0.1)
    assert L.genie_train_forward_obj(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, ob) == lib.E_ARG
    want = L.genie_last_error()
    assert L.genie_ce_objective(None, None, None, 2, 4, 16, 512, 2, 262144, ob, None, None) == lib.E_ARG
    want_ce = L.genie_last_error()
    assert b"genie_ce_objective: NULL" in want_ce
    for ds in (None, lib.Distill(alpha=0.0, temperature=1.0, teacher_logits=None), lib.Distill(alpha=0.0, temperature=2.0, teacher_logits=12345)):
        assert L.genie_train_forward_distill(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, ob, ds) == lib.E_ARG
        assert L.genie_last_error() == want
        assert L.genie_ce_distill(None, 12345, None, None, 2, 4, 16, 512, 2, 262144, ob, ds, None, None) == lib.E_ARG
        assert L.genie_last_error() == want_ce
    bad = lib.Objective(label_smoothing=1.0)   # the objective's refusal is the _obj call's own
    assert L.genie_train_forward_distill(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, bad, None) == lib.E_ARG
    assert b"genie_train_forward_obj" in L.genie_last_error()


def test_trainer_validation():
    """distill_settings and check_teacher: alpha outside [0, 1], a temperature that is not finite and > 0, a teacher with another T, S
    or vocabulary, and a teacher conditioned otherwise than the student are ValueErrors; depth, width, heads and norms are free."""
    T = pkg("train")
    assert T.distill_settings() == (0.0, 1.0) and T.distill_settings(0.5, 2) == (0.5, 2.0) and T.distill_settings(1, 0.5) == (1.0, 0.5)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(distill_alpha=-0.1), dict(distill_alpha=1.1), dict(distill_alpha=nan), dict(distill_temperature=0.0),
                dict(distill_temperature=-1.0), dict(distill_temperature=inf), dict(distill_temperature=nan)):
        with pytest.raises(ValueError):
            T.distill_settings(**bad)
    G = pkg("config").GenieConfig
    base = dict(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2)
    student = G(**base)
    T.check_teacher(student, G(**{**base, "num_layers": 5, "num_heads": 4, "d_model": 256, "qk_norm": True}))
    for other in (dict(T=8), dict(S=64), dict(num_factored_vocabs=1), dict(image_vocab_size=4096, num_factored_vocabs=2)):
        with pytest.raises(ValueError):
            T.check_teacher(student, G(**{**base, **other}))
    with pytest.raises(ValueError):
        T.check_teacher(student, G(**base, action_vocab_size=3))
    with pytest.raises(ValueError):
        T.check_teacher(G(**base, action_vocab_size=3), G(**base, action_vocab_size=4))
    with pytest.raises(ValueError):
        T.check_teacher(G(**base, action_vocab_size=3), G(**base, action_dim=3))
    T.check_teacher(G(**base, action_vocab_size=3), G(**base, action_vocab_size=3))
    T.check_teacher(G(**base, action_vocab_size=3), G(**base))   # an unconditioned teacher serves any student
    T.check_teacher(G(**base, action_dim=5), G(**base, action_dim=5))


def test_train_cli_lists_the_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-800:]
    for flag in ("--teacher_path", "--teacher_precision", "--distill_alpha", "--distill_temperature"):
        assert flag in out.stdout, flag


def test_train_cli_refuses_bad_distillation_flags(tmp_path):
    """tools/train.py ends with a `train.py:` message, before it builds anything, on an alpha above 1, a temperature of 0, and an
    alpha > 0 without --teacher_path -- each with the trainer's own message, not argparse's for a flag it does not know."""
    runs = {"alpha": ["--distill_alpha", "1.5", "--teacher_path", str(tmp_path)], "tau": ["--distill_alpha", "0.5", "--distill_temperature", "0",
                                                                                          "--teacher_path", str(tmp_path)],
            "none": ["--distill_alpha", "0.5"]}
    procs = {tag: subprocess.Popen([sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "16", "--model", "tiny",
                                    "--max_train_steps", "1", "--output_dir", str(tmp_path / tag)] + flags,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for tag, flags in runs.items()}
    for tag, pr in procs.items():
        out, err = pr.communicate(timeout=600)
        assert pr.returncode not in (0, None) and pr.returncode > 0, (tag, pr.returncode, err[-500:])
        last = err.strip().splitlines()[-1]
        assert last.startswith("train.py: ") and "--distill" in last and "unrecognized" not in err, (tag, err[-800:])
        want = {"alpha": "distill_alpha must be in [0, 1]", "tau": "distill_temperature must be finite and > 0", "none": "needs --teacher_path"}[tag]
        assert want in last, (tag, last)
        assert not (tmp_path / tag).exists(), f"{tag}: the run got as far as its output directory"


# ---------------------------------------------------------------------------------------------- 4. the compiled kernel
def test_compiled_distill_kernel_has_no_scratch():
    """The four instantiations of ce_distill_kernel (registers / streaming x tau == 1 / any tau) in the built library: no scratch, and
    at most 128 VGPRs -- four waves per SIMD, one workgroup's worth: the kernel is memory-bound and hides latency with the sixteen
    requests each lane keeps in flight times the resident waves.  Read from the code objects' metadata (tools/isa_audit.py)."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(REPO, "tools", "isa_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = {r[0]: r for r in mod.audit(lib_mod.LIB_PATH, all_kernels=True) if "ce_distill_kernel<" in r[0]}
    assert len(rows) == 4, sorted(rows)
    for name, r in rows.items():
        scratch, vgpr = r[6], r[7]
        print(name, "scratch", scratch, "vgpr", vgpr)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert 0 < vgpr <= 128, (name, vgpr)
