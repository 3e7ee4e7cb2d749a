"""The training objective (label smoothing, z-loss, per-frame loss weights; include/genie_hip.h, "Training objective"), the part that
needs no GPU: the two yardsticks of tests/objective_model.py against each other and against the step's existing model, the trainer's
validation, the struct's layout, the refusals of the library (they precede every device call), the CLI's refusals, and the validity
condition of the GPU cases of tests/test_hip_train_objective.py.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dropout_model as DM
import objective_model as OM
from conftest import REPO, pkg

GRAD_TOL, LOSS_TOL = 1e-4, 1e-5          # the bars of tests/test_hip_train_geometry.py, restated


def make_case(name, data_seed):
    import test_hip_train_dropout as TD   # its make_case is the construction the issue names (cached, read-only)
    return TD.make_case(name, data_seed)


# ---------------------------------------------------------------------------------------------- the two yardsticks
@pytest.mark.parametrize("vf,nfac", [(16, 4), (100, 2), (512, 1)])
@pytest.mark.parametrize("eps,zeta,weighted", [(0.0, 0.0, False), (0.1, 0.0, False), (0.0, 1e-2, False), (0.0, 0.0, True), (0.1, 1e-2, True)])
def test_ce_objective_agrees_with_autograd(vf, nfac, eps, zeta, weighted):
    """ce_objective's d logits and loss (its formulas) against torch autograd of F.cross_entropy(label_smoothing) + zeta logsumexp^2
    with per-frame weights, in float64 on random logits: 1e-12 of the largest element."""
    import torch
    F = torch.nn.functional
    g = np.random.default_rng(vf + nfac)
    n_clips, T, S = 2, 4, 6
    N, mask_id = n_clips * T * S, vf ** nfac
    weights = (1.0, 0.5, 0.0, 2.0) if weighted else None
    logits = (3.0 * g.standard_normal((N, nfac * vf))).astype(np.float32)
    labels = g.integers(0, mask_id, N)
    ids = np.where(g.random(N) < 0.5, mask_id, labels)
    d, sums = OM.ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id, eps, zeta, weights)
    e32, z32 = float(np.float32(eps)), float(np.float32(zeta))
    with torch.enable_grad():
        z = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
        flat = z.reshape(N * nfac, vf)
        y = torch.from_numpy(np.stack([(labels // vf ** f) % vf for f in range(nfac)], 1).reshape(-1))
        per = (F.cross_entropy(flat, y, label_smoothing=e32, reduction="none") + z32 * torch.logsumexp(flat, -1) ** 2).reshape(N, nfac).sum(-1)
        counted = torch.from_numpy(OM.counted_mask(ids, T, S, mask_id).reshape(N))
        w = torch.from_numpy(np.broadcast_to(OM.frame_weights(weights, T)[None, :, None], (n_clips, T, S)).reshape(N).copy())
        loss = (per * w * counted).sum() / (w * counted).sum()
        loss.backward()
    assert counted.sum() > 0 and sums[4] == float(counted.sum()) and sums[2] == float((w * counted).sum())
    loss = float(loss.detach())
    assert abs(sums[0] / sums[2] - loss) <= 1e-12 * abs(loss)
    ref = z.grad.numpy()
    assert np.abs(d - ref).max() <= 1e-12 * np.abs(ref).max()
    dead = ~(counted.numpy() & (w.numpy() > 0))
    assert dead.any() and not d[dead].any()
    if eps == 0.0 and zeta == 0.0:   # the plain CE is the neutral objective
        plain = sums[3] / sums[4]
        if not weighted:
            assert abs(plain - sums[0] / sums[2]) <= 1e-14 * plain


def test_ce_objective_zero_weight_sum():
    """W = 0 with counted tokens: every row zero, s0 = 0 and s2 = 0 (the loss is their 0 / 0), hits, plain nll and n as without weights."""
    g = np.random.default_rng(5)
    T, S, vf, nfac = 3, 4, 8, 2
    N, mask_id = 2 * T * S, vf ** nfac
    logits = g.standard_normal((N, nfac * vf)).astype(np.float32)
    labels = g.integers(0, mask_id, N)
    ids = labels.copy().reshape(2, T, S)
    ids[:, 2] = mask_id
    d, sums = OM.ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id, 0.1, 1e-2, (1.0, 1.0, 0.0))
    _, plain = OM.ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id)
    assert not d.any() and sums[0] == 0.0 and sums[2] == 0.0
    assert sums[4] == 2 * S and sums[1] == plain[1] and sums[3] == plain[3] and sums[4] == plain[4]


@functools.lru_cache(maxsize=None)
def neutral_step(name):
    cfg, sd, ids, labels = make_case(name, OM.STEP_CASES[name][0])
    return OM.autograd_step(cfg, sd, ids, labels)


@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_neutral_autograd_step_is_the_dropout_models(name):
    """At eps = zeta = 0 and no weights objective_model.autograd_step is dropout_model.autograd_step (loss and every gradient to 1e-13),
    its plain CE is its loss, and an all-ones weight vector changes nothing; the cases count the tokens per frame that the GPU tests rely on."""
    seed, _, per_frame = OM.STEP_CASES[name]
    cfg, sd, ids, labels = make_case(name, seed)
    assert OM.counted_mask(ids, cfg.T, cfg.S, cfg.image_vocab_size).sum(axis=(0, 2)).tolist() == per_frame
    loss, grads, ce, acc = neutral_step(name)
    loss_d, grads_d = DM.autograd_step(cfg, sd, ids, labels)
    assert abs(loss - loss_d) <= 1e-13 * abs(loss_d) and abs(ce - loss) <= 1e-13 * abs(loss) and 0.0 <= acc <= 1.0
    assert set(grads) == set(grads_d)
    for k, g in grads.items():
        assert np.abs(g - grads_d[k]).max() <= 1e-13 * np.abs(grads_d[k]).max(), k
    loss_1, grads_1, _, _ = OM.autograd_step(cfg, sd, ids, labels, weights=(1.0,) * cfg.T)
    assert abs(loss_1 - loss) <= 1e-13 * abs(loss) and all(np.abs(grads_1[k] - g).max() <= 1e-13 * np.abs(g).max() for k, g in grads.items())


@pytest.mark.parametrize("tag", ["eps", "zeta", "weights", "all"])
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_gpu_cases_can_tell_the_objective_from_none(name, tag):
    """The validity condition of the step tests of tests/test_hip_train_objective.py: at every knob setting they use the model's loss
    differs from the neutral model's by more than 100 x LOSS_TOL (relative) and EVERY gradient tensor by more than 100 x GRAD_TOL
    (worst element over the neutral tensor's largest) -- a step that ignored the knob would miss the bars by two orders of magnitude.
    Smallest changes over the settings: loss 1.27e-3 (eps = 0.1), tensor 2.8e-2.  (At zeta = 1e-4 the gradients move by 5.6e-4 only,
    which is why the step tests take zeta = 1e-2.)"""
    cfg, sd, ids, labels = make_case(name, OM.STEP_CASES[name][0])
    loss0, grads0, _, _ = neutral_step(name)
    eps, zeta, weights = OM.settings(name)[tag]
    loss, grads, ce, _ = OM.autograd_step(cfg, sd, ids, labels, eps, zeta, weights)
    dl = abs(loss - loss0) / abs(loss0)
    moved = {k: float(np.abs(g - grads0[k]).max() / np.abs(grads0[k]).max()) for k, g in grads.items()}
    low = min(moved.items(), key=lambda kv: kv[1])
    print(f"train_objective/validity/{name}/{tag}: loss moves by {dl:.3e}, the least moved tensor {low[0]} by {low[1]:.3e}")
    assert set(grads) == set(grads0)
    assert abs(ce - loss0) <= 1e-13 * loss0, "the plain CE does not depend on the objective"
    assert dl > 100 * LOSS_TOL
    assert low[1] > 100 * GRAD_TOL, low


# ---------------------------------------------------------------------------------------------- the trainer's validation
def test_objective_settings_validation():
    T = pkg("train")
    f = T.objective_settings
    assert f() == (0.0, 0.0, None) and f(0.1, 1e-4, None, 4) == (0.1, 1e-4, None)
    assert f(0.0, 0.0, [1, 1, 1, 1], 4) == (0.0, 0.0, None), "all-ones weights are no weights"
    assert f(0.0, 0.0, (1, 0, 0.5, 2), 4) == (0.0, 0.0, (1.0, 0.0, 0.5, 2.0))
    assert f(0.0, 0.0, np.array([0.0, 0.0, 0.0, 3.0], np.float32), 4)[2] == (0.0, 0.0, 0.0, 3.0)
    for bad in (dict(label_smoothing=-0.1), dict(label_smoothing=1.0), dict(label_smoothing=float("nan")),
                dict(z_loss=-1e-4), dict(z_loss=float("inf")), dict(z_loss=float("nan")),
                dict(frame_weights=(1, 1, 1)), dict(frame_weights=(1, 1, 1, 1, 1)), dict(frame_weights=(1, -1, 1, 1)),
                dict(frame_weights=(1, float("inf"), 1, 1)), dict(frame_weights=(1, float("nan"), 1, 1)),
                dict(frame_weights=(1, 0, 0, 0)), dict(frame_weights=(0, 0, 0, 0))):
        with pytest.raises(ValueError):
            f(**{"T": 4, **bad})


def test_neutral_settings_make_no_struct():
    """The neutral-struct rule on the Python side: eps = zeta = 0 without weights (all-ones included, and values that are 0 as floats)
    gives None -- the trainer then calls the entry points of before; anything else a genie_objective with n_frames 0 or T."""
    T, lib = pkg("train"), pkg("_lib")
    assert T.make_objective(*T.objective_settings()) is None
    assert T.make_objective(*T.objective_settings(0.0, 0.0, (1.0,) * 8, 8)) is None
    assert T.make_objective(1e-60, 1e-60, None) is None
    ob = T.make_objective(*T.objective_settings(0.1, 0.0, None, 4))
    assert isinstance(ob, lib.Objective) and ob.n_frames == 0 and ob.reserved == 0 and ob.label_smoothing == np.float32(0.1)
    ob = T.make_objective(*T.objective_settings(0.0, 0.0, (1, 0, 0.5, 2), 4))
    assert ob.n_frames == 4 and list(ob.frame_weight)[:5] == [1.0, 0.0, 0.5, 2.0, 0.0] and ob.z_loss == 0.0


# ---------------------------------------------------------------------------------------------- the library, without a device
def test_objective_layout():
    """genie_objective as the compiler lays it out against the ctypes declaration: 272 bytes, the weights at 16."""
    lib = pkg("_lib")
    L = lib.load()
    out = (ctypes.c_size_t * 6)()
    assert L.genie_objective_layout(out, 6) == 6
    O = lib.Objective
    assert list(out) == [ctypes.sizeof(O), O.label_smoothing.offset, O.z_loss.offset, O.n_frames.offset, O.reserved.offset,
                         O.frame_weight.offset] == [272, 0, 4, 8, 12, 16]
    short = (ctypes.c_size_t * 2)(7, 7)
    assert L.genie_objective_layout(short, 1) == 6 and list(short) == [272, 7]
    assert L.genie_version() == 3


def refusals(T):
    """(what, genie_objective) for every GENIE_E_ARG of the contract, for a call over T frames."""
    O = pkg("_lib").Objective
    nan, inf = float("nan"), float("inf")

    def ob(eps=0.0, zeta=0.0, n=0, w=()):
        o = O(label_smoothing=eps, z_loss=zeta, n_frames=n)
        for t, v in enumerate(w):
            o.frame_weight[t] = v
        return o
    ones = [1.0] * T
    return [("eps < 0", ob(eps=-0.01)), ("eps = 1", ob(eps=1.0)), ("eps > 1", ob(eps=1.5)), ("eps nan", ob(eps=nan)),
            ("zeta < 0", ob(zeta=-1e-4)), ("zeta inf", ob(zeta=inf)), ("zeta nan", ob(zeta=nan)),
            ("n_frames T - 1", ob(n=T - 1, w=ones)), ("n_frames T + 1", ob(n=T + 1, w=ones + [1.0])), ("n_frames < 0", ob(n=-1)),
            ("w < 0", ob(n=T, w=ones[:-1] + [-1.0])), ("w inf", ob(n=T, w=[inf] + ones[1:])), ("w nan", ob(n=T, w=ones[:1] + [nan] + ones[2:]))]


def test_library_refuses_bad_objectives_before_anything_else():
    """Every refusal of the contract is GENIE_E_ARG from genie_ce_objective and genie_train_forward_obj BEFORE any other check: here
    with every pointer NULL, which a later check would report under another message -- and no device is needed."""
    lib = pkg("_lib")
    L = lib.load()
    T = 4
    cfg = lib.GenieCfg(T=T)
    for what, ob in refusals(T):
        assert L.genie_ce_objective(None, None, None, 2, T, 16, 512, 2, 262144, ob, None, None) == lib.E_ARG, what
        assert b"genie_ce_objective" in L.genie_last_error() and b"NULL" not in L.genie_last_error(), (what, L.genie_last_error())
        assert L.genie_train_forward_obj(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, ob) == lib.E_ARG, what
        assert b"genie_train_forward_obj" in L.genie_last_error(), (what, L.genie_last_error())
    # a weight behind n_frames is not read: garbage there is not refused (the next check, the NULL pointers, is what answers)
    ok = lib.Objective(label_smoothing=0.1, n_frames=0)
    ok.frame_weight[0] = -1.0
    assert L.genie_ce_objective(None, None, None, 2, T, 16, 512, 2, 262144, ok, None, None) == lib.E_ARG
    assert b"NULL" in L.genie_last_error()
    # the loss launch alone: geometry it cannot take
    one = ctypes.c_double()
    p = ctypes.addressof(one)   # never dereferenced: the argument checks come first
    for n_clips, Tq, S, vf, nfac in ((0, 4, 16, 512, 2), (2, 0, 16, 512, 2), (2, 4, 0, 512, 2), (2, 4, 16, 0, 2), (2, 4, 16, 512, 0),
                                     (2, 4, 16, 512, 5)):
        assert L.genie_ce_objective(p, p, p, n_clips, Tq, S, vf, nfac, 1, None, p, None) == lib.E_ARG, (n_clips, Tq, S, vf, nfac)
    assert L.genie_ce_objective(p, p, p, 2, 4, 16, 512, 2, 2 ** 40, None, p, None) == lib.E_ARG   # the neutral kernels' mask id is an int


def test_neutral_struct_is_the_drop_call():
    """obj == NULL and a neutral struct hand genie_train_forward_obj's arguments to genie_train_forward_drop: with a NULL model the answer
    is that entry point's own refusal, word for word; a struct that is not neutral gets there too once it has passed its own checks."""
    lib = pkg("_lib")
    L = lib.load()
    cfg = lib.GenieCfg(T=4)
    assert L.genie_train_forward_drop(cfg, None, None, None, 2, None, 0, None, None, None, 0, None) == lib.E_ARG
    want = L.genie_last_error()
    assert b"genie_train_forward: NULL argument" in want
    for ob in (None, lib.Objective(), lib.Objective(label_smoothing=0.1)):
        assert L.genie_train_forward_obj(cfg, None, None, None, 2, None, 0, None, None, None, 0, None, ob) == lib.E_ARG
        assert L.genie_last_error() == want
    # recompute and dropout arguments are checked as the _drop call checks them
    assert L.genie_train_forward_obj(cfg, None, None, None, 2, None, 0, None, None, None, 2, None, lib.Objective()) == lib.E_ARG
    assert b"recompute" in L.genie_last_error()


# ---------------------------------------------------------------------------------------------- the CLI
def test_train_cli_refuses_bad_objective_flags(tmp_path):
    """tools/train.py ends with a `train.py:` message, before it builds anything, on a label smoothing of 1, a negative z-loss, weights
    that are no numbers, a negative weight, and weights that leave nothing behind frame 0.  (A weight count that is not the window's
    is refused once the window is known: tests/test_hip_train_objective.py.)"""
    runs = {"eps": ["--label_smoothing", "1.0"], "zeta": ["--z_loss=-1e-4"], "text": ["--frame_loss_weights", "1,x,2,2"],
            "neg": ["--frame_loss_weights", "1,-1,2,2"], "none": ["--frame_loss_weights", "1,0,0,0"]}
    procs = {tag: subprocess.Popen([sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "16", "--model", "tiny",
                                    "--max_train_steps", "1", "--output_dir", str(tmp_path / tag)] + flags,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for tag, flags in runs.items()}
    for tag, pr in procs.items():
        out, err = pr.communicate(timeout=600)
        assert pr.returncode not in (0, None) and pr.returncode > 0, (tag, pr.returncode, err[-500:])
        last = err.strip().splitlines()[-1]
        assert last.startswith("train.py: "), (tag, err[-800:])
        assert ("--frame_loss_weights" in last) if tag in ("text", "neg", "none") else ("--label_smoothing" in last), (tag, last)
        assert not (tmp_path / tag).exists(), f"{tag}: the run got as far as its output directory"
