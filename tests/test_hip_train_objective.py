"""Training with label smoothing, z-loss and per-frame loss weights (include/genie_hip.h, "Training objective"; ce_objective_kernel in
csrc/kernels_loss.hip): the loss launch alone against the float64 contract with the neutral step's kernel as the floor, trainer steps
against the float64 autograd model of tests/objective_model.py in the three precisions, composition with recomputation, dropout and
gradient accumulation, the neutral trainer against the trainer of before, W = 0, refusals, resume and the CLI.

Step cases (tests/objective_model.py::STEP_CASES; built by tests/test_hip_train_dropout.py::make_case):
  ln3   H 2, d 64, T 4, S 16, B 2, LayerNorm, 3 layers; data seed 0, weights (1, 0, 0.5, 2), counted per frame [0, 20, 19, 24]
  qk3   H 2, d 128, T 8, S 16, B 3, Identity norms, 3 layers; data seed 2, weights (1, 0.5, 1, 1.5, 2, 0, 3, 0.25),
        counted per frame [0, 35, 32, 13, 30, 38, 29, 17]
Settings: eps = 0.1 alone, zeta = 1e-2 alone, the weights alone, all three (tests/test_train_objective_cpu.py shows that each moves the
loss by more than 100 x LOSS_TOL and every gradient tensor by more than 100 x GRAD_TOL).

The GPU tests need an MI355X (``-m gpu``); tests/test_train_objective_cpu.py holds what runs anywhere.
"""
import functools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import dropout_model as DM
import objective_model as OM
import test_hip_train_dropout as TD
from conftest import REPO, pkg, record_measure
from oracle import genie_train_oracle as TO

GRAD_TOL, LOSS_TOL = 1e-4, 1e-5          # the bars of tests/test_hip_train_geometry.py, restated
PRECISIONS = ["exact", "f16x3", "bf16"]
TAGS = ["eps", "zeta", "weights", "all"]
SEED = 3   # dropout_seed of the step with dropout

# bf16 bars (median / max / Frobenius / loss / global norm; tests/test_hip_train_bf16.py::errors and check_vs_oracle), the constants of
# tests/test_hip_train_dropout.py::BF16_BARS restated: 3 x the worst error, over data seeds 0 .. 23 of make_case, of the PARENT's bf16
# step -- no objective, no dropout -- against the float64 model (printed on an MI355X, profiles/train_dropout.txt).  The objective
# changes the loss kernel only, which is f32 in every precision: the bf16 error of a step is that of its Linear products, as before.
BF16_BARS = {
    "ln3": (3 * 2.32e-3, 3 * 1.46e-2, 3 * 9.42e-3, 3 * 2.42e-3, 3 * 1.14e-3),
    "qk3": (3 * 3.66e-3, 3 * 2.29e-2, 3 * 1.26e-2, 3 * 1.85e-3, 3 * 1.37e-3),
}


def torch_():
    return pytest.importorskip("torch")


def case(name, data_seed=None):
    return TD.make_case(name, OM.STEP_CASES[name][0] if data_seed is None else data_seed)


@functools.lru_cache(maxsize=None)
def model_step(name, tag, p=0.0, data_seed=None):
    """(loss, grads, plain CE, acc) of the float64 model at a setting of OM.settings ("none": neutral); p: with the dropout masks of
    (SEED, call 0).  Computed once, shared, never written to."""
    cfg, sd, ids, labels = case(name, data_seed)
    eps, zeta, weights = (0.0, 0.0, None) if tag == "none" else OM.settings(name)[tag]
    masks = DM.step_masks(cfg, ids.shape[0], SEED, 0, p) if p else None
    return OM.autograd_step(cfg, sd, ids, labels, eps, zeta, weights, masks, TD.f32p(p))


def trainer(name, precision, tag, p=0.0, data_seed=None, **kw):
    cfg, sd, _, _ = case(name, data_seed)
    if tag != "none":
        eps, zeta, weights = OM.settings(name)[tag]
        kw = dict(label_smoothing=eps, z_loss=zeta, frame_weights=weights, **kw)
    return TD.make_trainer(cfg, sd, precision, p, **kw)


def one_step(name, precision, tag, p=0.0, data_seed=None, **kw):
    """One forward_backward -> (loss, acc, {tensor: gradient}, trainer)."""
    _, _, ids, labels = case(name, data_seed)
    tr = trainer(name, precision, tag, p, data_seed, **kw)
    loss, acc = tr.forward_backward(TD.dev(ids), TD.dev(labels))
    return float(loss), float(acc), {k: v.cpu().numpy() for k, v in tr.gradients().items()}, tr


# ---------------------------------------------------------------------------------------------- 1. the loss launch alone
WINDOW_SHAPES = [   # (n_clips, T, S, vf, nfac)
    (3, 3, 5, 512, 2),      # 45 tokens: the last workgroup has one live wave
    (2, 4, 16, 100, 2),     # vf no multiple of 64
    (2, 4, 16, 16, 4),      # vf < 64, four factors
    (1, 2, 16, 4096, 1),    # above 512: the streaming path
    (2, 4, 16, 64, 3),
    (4, 4, 80, 512, 2),     # 1,280 tokens: more than one pass of the count block
]
WINDOW_SETTINGS = {"eps": (0.1, 0.0, False), "zeta": (0.0, 1e-2, False), "zeta1e-4": (0.0, 1e-4, False), "weights": (0.0, 0.0, True),
                   "all": (0.1, 1e-2, True)}


def window_weights(T):
    """One weight per frame with a zero-weight frame as soon as T >= 3 and a positive one behind frame 0."""
    return tuple((1.0, 0.5, 0.0, 2.0)[t % 4] for t in range(T))


@functools.lru_cache(maxsize=None)
def window_inputs(shape, scale):
    """(logits f32 (N, nfac * vf), ids, labels, mask_id): about half the ids are the mask id, frame 0 included; rows are random at
    `scale`, with one-hot rows (+80 on each factor's target), uniform rows and rows shifted by +1000 mixed in."""
    n_clips, T, S, vf, nfac = shape
    g = np.random.default_rng(1000 * vf + 10 * nfac + int(scale))
    N, mask_id = n_clips * T * S, vf ** nfac
    labels = g.integers(0, mask_id, N)
    ids = np.where(g.random(N) < 0.5, mask_id, g.integers(0, mask_id, N))
    assert (ids.reshape(n_clips, T, S)[:, 0] == mask_id).any() and OM.counted_mask(ids, T, S, mask_id).sum(axis=(0, 2))[1:].all()
    z = (scale * g.standard_normal((N, nfac, vf))).astype(np.float32)
    row = np.arange(N)
    y = np.stack([(labels // vf ** f) % vf for f in range(nfac)], 1)
    hot = row % 7 == 1
    z[hot] = (0.1 * g.standard_normal((int(hot.sum()), nfac, vf))).astype(np.float32)
    for f in range(nfac):
        z[row[hot], f, y[hot, f]] += np.float32(80.0)
    z[row % 7 == 3] = np.float32(0.25)
    z[row % 7 == 5] += np.float32(1000.0)
    for a in (z, ids, labels):
        a.setflags(write=False)
    return z.reshape(N, nfac * vf), ids, labels, mask_id


class Window:
    """One shape's device buffers: the logits between guard regions (tests/test_hip_train_ema.py::Guarded), ids, labels, and eight
    doubles of sums pre-filled with a sentinel."""

    def __init__(self, shape, scale):
        import test_hip_train_ema as TE
        torch = torch_()
        self.shape = shape
        self.logits, self.ids, self.labels, self.mask_id = window_inputs(shape, scale)
        self.buf = TE.Guarded(self.logits.reshape(-1).copy())
        self.d_ids, self.d_labels = TD.dev(self.ids.copy()), TD.dev(self.labels.copy())   # (the cached inputs are read-only)
        self.sums = torch.empty(8, dtype=torch.float64, device="cuda")
        self.lib = pkg("_lib")
        self.L = self.lib.load()

    def run(self, obj):
        """genie_ce_objective on a fresh copy of the logits -> (d logits f32 (N, V), sums (8,)); the guards are checked by read()."""
        torch = torch_()
        n_clips, T, S, vf, nfac = self.shape
        self.buf.f[self.buf.lo:self.buf.lo + self.buf.n].copy_(torch.from_numpy(self.logits.reshape(-1).copy()))
        self.sums.fill_(-7.0)
        self.lib.check(self.L.genie_ce_objective(self.buf.ptr, self.d_ids.data_ptr(), self.d_labels.data_ptr(), n_clips, T, S, vf, nfac,
                                                 self.mask_id, obj, self.sums.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "genie_ce_objective")
        torch.cuda.synchronize()
        return self.buf.read().reshape(self.logits.shape), self.sums.cpu().numpy()

    def objective(self, eps=0.0, zeta=0.0, weights=None):
        ob = self.lib.Objective(label_smoothing=eps, z_loss=zeta, n_frames=0 if weights is None else len(weights))
        for t, v in enumerate(weights or ()):
            ob.frame_weight[t] = v
        return ob

    def model(self, eps=0.0, zeta=0.0, weights=None):
        n_clips, T, S, vf, nfac = self.shape
        return OM.ce_objective(self.logits, self.ids, self.labels, T, S, vf, nfac, self.mask_id, eps, zeta, weights)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_launch_against_the_contract(shape, scale):
    """genie_ce_objective on guarded logits.  obj = NULL (the neutral step's kernel) against the float64 contract gives this shape's
    floor: the largest error of d logits over the model's largest element.  The general kernel at neutral values (n_frames 0, and
    n_frames T with all ones) gives the floor kernel's d logits BIT FOR BIT and its sums to 1e-12 (s3 = s0, s4 = s2).  At eps = 0.1,
    zeta = 1e-2, zeta = 1e-4, the weights, and all three, d logits is within 4 x the floor of the model (the element takes two more
    f32 roundings, the factor 1 + 2 zeta lse and the smoothed target, on top of the shared exp / normalise error) and the five sums
    within LOSS_TOL; a second launch gives the same bits; rows of uncounted and zero-weight tokens are exactly zero; guards untouched.
    Measured on an MI355X: the floor is 7.0e-8 to 2.1e-7 over the twelve cases; the knob settings reach 0.28 to 1.76 x the floor (the
    largest at 2x4x16x64x3, scale 1, eps = 0.1: 1.57e-7 against 8.9e-8; no ratio exceeds 2); the sums are within 4.4e-7."""
    n_clips, T, S, vf, nfac = shape
    tag = "x".join(map(str, shape)) + f"/s{scale}"
    w = Window(shape, scale)
    counted = OM.counted_mask(w.ids, T, S, w.mask_id).reshape(-1)
    # the floor
    d_par, s_par = w.run(None)
    d_m, s_m = w.model()
    floor = float(np.abs(d_par - d_m).max() / np.abs(d_m).max())
    record_measure(f"train_objective/window/{tag}/parent", floor)
    print(f"train_objective/window/{tag}: parent {floor:.3e}")
    assert 0 < floor < 1e-5 and (s_par[3:] == -7.0).all(), (floor, s_par)
    assert s_par[1] == s_m[1] and s_par[2] == s_m[2] == s_m[4] and abs(s_par[0] - s_m[3]) <= LOSS_TOL * s_m[3]
    assert not d_par[~counted].any()
    # neutral values: the floor kernel's bits
    for ob in (w.objective(), w.objective(weights=(1.0,) * T)):
        d, s = w.run(ob)
        assert np.array_equal(bits(d), bits(d_par)), f"{int((bits(d) != bits(d_par)).sum())} words differ from the neutral kernel's"
        assert abs(s[0] - s_par[0]) <= 1e-12 * s_par[0] and abs(s[1] - s_par[1]) <= 1e-12 * s_par[1]
        assert abs(s[3] - s[0]) <= 1e-12 * s[0] and abs(s[4] - s[2]) <= 1e-12 * s[2] and s[2] == s_par[2]
        assert (s[5:] == -7.0).all()
    # the knobs
    ww = window_weights(T)
    wn = np.broadcast_to(np.asarray(ww)[None, :, None], (n_clips, T, S)).reshape(-1)
    for key, (eps, zeta, weighted) in WINDOW_SETTINGS.items():
        weights = ww if weighted else None
        ob = w.objective(eps, zeta, weights)
        d, s = w.run(ob)
        d_m, s_m = w.model(eps, zeta, weights)
        err = float(np.abs(d - d_m).max() / np.abs(d_m).max())
        record_measure(f"train_objective/window/{tag}/{key}", err)
        print(f"train_objective/window/{tag}: {key} {err:.3e} = {err / floor:.2f} x parent; sums "
              + " ".join(f"{abs(a - b) / max(abs(b), 1e-300):.1e}" for a, b in zip(s[:5], s_m)))
        assert err <= 4 * floor, (key, err, floor)
        assert all(abs(a - b) <= LOSS_TOL * abs(b) for a, b in zip(s[:5], s_m)), (key, s[:5], s_m)
        assert s[2] == s_m[2] and s[4] == s_m[4] and s[1] == s_m[1], "counts and hits are integers"
        dead = ~counted | (wn == 0.0) if weighted else ~counted
        assert dead.any() and not d[dead].any() and d[~dead].any(axis=1).all()
        d2, s2 = w.run(ob)
        assert np.array_equal(bits(d2), bits(d)), "a second launch from the same inputs gave other bits"
        assert (s[5:] == -7.0).all()


# ---------------------------------------------------------------------------------------------- 2. the step, exact and f16x3
@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_vs_float64_model(name, precision, tag):
    """Loss (LOSS_TOL, relative) and every gradient tensor (GRAD_TOL, worst element over the tensor's largest) of one step against
    the float64 autograd model at the same setting; last_ce against the model's plain CE (LOSS_TOL) and acc against its accuracy
    (1e-7, the bar of tests/test_hip_train.py).  Measured on an MI355X, worst tensor over the four settings: exact ln3 9.7e-07, qk3
    1.8e-06; f16x3 ln3 5.4e-07, qk3 8.1e-07; loss 4.3e-08 and plain CE 1.7e-08 at most."""
    loss_o, g_o, ce_o, acc_o = model_step(name, tag)
    loss, acc, grads, tr = one_step(name, precision, tag)
    worst = {k: TD.rel_err(g, g_o[k]) for k, g in grads.items()}
    assert set(worst) <= set(g_o)
    top = max(worst.items(), key=lambda kv: kv[1])
    dl, dce = abs(loss - loss_o) / abs(loss_o), abs(float(tr.last_ce) - ce_o) / ce_o
    record_measure(f"train_objective/{precision}/{name}/{tag}", top[1])
    print(f"train_objective/{precision}/{name}/{tag}: loss {loss:.8f} (model {loss_o:.8f}, rel {dl:.2e}), ce rel {dce:.2e}, "
          f"worst tensor {top[0]} {top[1]:.3e}")
    assert tr.sums.numel() == 5 and tr.last_ce.is_cuda and tr.last_ce.dim() == 0
    assert dl < LOSS_TOL and dce < LOSS_TOL and abs(acc - acc_o) < 1e-7
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 3. bf16
@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_bf16_vs_float64_model(name, tag):
    """The five statistics of tests/test_hip_train_bf16.py::check_vs_oracle for one bf16 step with the objective against the float64
    model at the same setting, at BF16_BARS (see there).  Measured on an MI355X, the largest over the four settings (median / max /
    Frobenius / loss / norm): ln3 1.70e-03 / 1.02e-02 / 7.29e-03 / 4.37e-04 / 1.46e-03; qk3 2.71e-03 / 1.28e-02 / 1.15e-02 / 1.47e-03 /
    9.56e-04 -- every one inside the parent's own spread over data seeds (profiles/train_dropout.txt, section 4)."""
    torch = torch_()
    import test_hip_train_bf16 as B16
    loss_o, g_o, _, _ = model_step(name, tag)
    loss, _, grads, tr = one_step(name, "bf16", tag)
    worst = np.zeros(3)
    for k, g in grads.items():
        worst = np.maximum(worst, np.array(B16.errors(g, g_o[k])))
    gn, gn_o = float(torch.sqrt(tr.grad_sumsq()[0])), TO.grad_norm({k: g_o[k] for k in grads})
    stats = (float(worst[0]), float(worst[1]), float(worst[2]), abs(loss - loss_o), abs(gn - gn_o) / gn_o)
    keys = ("median", "max", "fro", "loss", "norm")
    for key, v, bar in zip(keys, stats, BF16_BARS[name]):
        record_measure(f"train_objective/bf16/{name}/{tag}/{key}", v)
        print(f"train_objective/bf16/{name}/{tag}/{key}: {v:.3e} (bar {bar:.3e})")
    bad = {key: (v, bar) for key, v, bar in zip(keys, stats, BF16_BARS[name]) if not v < bar}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 4. composition
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_recompute_same_bits(name, precision):
    """All three knobs on: recompute=True gives the flat gradient bits and the loss of recompute=False (the backward reads d logits from
    the logits slot in both layouts and knows nothing of the objective)."""
    torch = torch_()
    _, _, ids, labels = case(name)
    ids, labels = TD.dev(ids), TD.dev(labels)
    saved, rec = trainer(name, precision, "all"), trainer(name, precision, "all", recompute=True)
    l0, a0 = saved.forward_backward(ids, labels)
    l1, a1 = rec.forward_backward(ids, labels)
    assert bool(torch.isfinite(saved.grads).all()) and float(saved.grads.abs().max()) > 0
    assert torch.equal(rec.grads, saved.grads), f"{int((rec.grads != saved.grads).sum())} gradient words differ between the modes"
    assert abs(float(l0) - float(l1)) <= 1e-12 * abs(float(l0)) and float(a0) == float(a1)
    assert abs(float(saved.last_ce) - float(rec.last_ce)) <= 1e-12 * float(saved.last_ce)
    assert rec._acts.numel() < saved._acts.numel()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_with_dropout_vs_float64_model(name):
    """mlp_drop = 0.1 and all three knobs, exact: against the model that applies both (the masks of dropout_model.step_masks).
    Measured on an MI355X, worst tensor: ln3 8.0e-07, qk3 1.6e-06 (loss 3.3e-08 at most)."""
    loss_o, g_o, ce_o, _ = model_step(name, "all", 0.1)
    loss, _, grads, tr = one_step(name, "exact", "all", 0.1, dropout_seed=SEED)
    worst = {k: TD.rel_err(g, g_o[k]) for k, g in grads.items()}
    top = max(worst.items(), key=lambda kv: kv[1])
    dl = abs(loss - loss_o) / abs(loss_o)
    record_measure(f"train_objective/exact/{name}/all+drop", top[1])
    print(f"train_objective/exact/{name}/all+drop: loss rel {dl:.2e}, worst tensor {top[0]} {top[1]:.3e}")
    assert dl < LOSS_TOL and abs(float(tr.last_ce) - ce_o) < LOSS_TOL * ce_o
    assert abs(loss_o - model_step(name, "all")[0]) > 100 * LOSS_TOL * loss_o, "the masks changed nothing: the case tests no dropout"
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_gradient_accumulation(precision):
    """gradient_accumulation_steps = 2 over two different micro-batches: train_step twice equals forward_backward, forward_backward
    with accumulate, optimizer_step -- gradients and updated parameters bit for bit; train_step reports "ce" with the objective on."""
    torch = torch_()
    batches = []
    for seed in (0, 3):
        _, _, ids, labels = case("ln3", seed)
        batches.append({"input_ids": TD.dev(ids), "labels": TD.dev(labels)})
    kw = dict(gradient_accumulation_steps=2, lr=1e-3)
    a, b = trainer("ln3", precision, "all", **kw), trainer("ln3", precision, "all", **kw)
    out0 = a.train_step(batches[0])
    assert set(out0) == {"loss", "acc", "ce"}
    out1 = a.train_step(batches[1])
    assert set(out1) == {"loss", "acc", "ce", "grad_norm", "lr"} and float(out1["ce"]) == float(a.last_ce)
    l0, _ = b.forward_backward(batches[0]["input_ids"], batches[0]["labels"])
    first = b.grads.clone()
    l1, _ = b.forward_backward(batches[1]["input_ids"], batches[1]["labels"], accumulate=True)
    assert float(l0) == float(out0["loss"]) and float(l1) == float(out1["loss"]) and float(l0) != float(l1)
    assert not torch.equal(b.grads, first) and torch.equal(a.grads, b.grads)
    b.optimizer_step()
    assert torch.equal(a.params, b.params) and a.completed_steps == b.completed_steps == 1


# ---------------------------------------------------------------------------------------------- 5. neutral is the step of before
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_neutral_is_the_step_of_before(name, precision):
    """A trainer given label_smoothing=0, z_loss=0, frame_weights=None and one given all-ones weights against a trainer built without
    the arguments: no objective struct, a three-double sums buffer, torch.equal flat gradients, the same loss and the same kernel table
    (genie_profile_kernels), in which no objective kernel appears; a trainer with the knobs on launches each of the two once."""
    torch = torch_()
    cfg, sd, ids, labels = case(name)
    ids, labels = TD.dev(ids), TD.dev(labels)
    plain = TD.make_trainer(cfg, sd, precision)
    g0, t0 = TD.profiled(plain, ids, labels)
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0 and sum(t0.values()) > 0
    assert not any("objective" in k or "count_frames" in k for k in t0), t0
    for kw in (dict(label_smoothing=0.0, z_loss=0.0, frame_weights=None), dict(frame_weights=[1.0] * cfg.T)):
        tr = TD.make_trainer(cfg, sd, precision, **kw)
        assert tr._objective is None and tr.sums.numel() == 3 and tr.frame_weights is None
        g1, t1 = TD.profiled(tr, ids, labels)
        assert torch.equal(g0, g1)
        assert t0 == t1, {k: (t0.get(k), t1.get(k)) for k in set(t0) | set(t1) if t0.get(k) != t1.get(k)}
        assert float(tr.last_ce) == float(plain.last_ce) and torch.equal(tr.sums, plain.sums)
    on = trainer(name, precision, "all")
    g2, t2 = TD.profiled(on, ids, labels)
    assert not torch.equal(g2, g0)
    assert set(t0) <= set(t2)
    extra = {k.split(":")[1]: v for k, v in t2.items() if t0.get(k) != v}
    assert extra == {"ce_objective_kernel": 1, "count_frames_kernel": 1}, extra


# ---------------------------------------------------------------------------------------------- 6. W = 0
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_zero_weight_sum(precision):
    """ln3 with data seed 1 counts tokens in the last frame only ([0, 0, 0, 24]); weights (1, 1, 1, 0) give W = 0: the loss is NaN,
    last_ce and acc are finite and the neutral step's, every gradient is exactly zero."""
    torch = torch_()
    cfg, sd, ids, labels = case("ln3", 1)
    assert OM.counted_mask(ids, cfg.T, cfg.S, cfg.image_vocab_size).sum(axis=(0, 2)).tolist() == [0, 0, 0, 24]
    ids, labels = TD.dev(ids), TD.dev(labels)
    neutral = TD.make_trainer(cfg, sd, precision)
    l0, a0 = neutral.forward_backward(ids, labels)
    tr = TD.make_trainer(cfg, sd, precision, label_smoothing=0.1, z_loss=1e-2, frame_weights=(1, 1, 1, 0))
    tr.grads.fill_(1.0)   # stale values: the backward has to overwrite every tensor with zeros
    loss, acc = tr.forward_backward(ids, labels)
    assert np.isnan(float(loss))
    assert np.isfinite(float(l0)) and abs(float(tr.last_ce) - float(l0)) <= 1e-12 * float(l0) and float(acc) == float(a0)
    assert float(tr.sums[2]) == 0.0 and float(tr.sums[4]) == 24.0
    nonzero = [k for k, g in tr.gradients().items() if bool(g.any())]
    assert not nonzero, nonzero


# ---------------------------------------------------------------------------------------------- 7. refusals and resume
@pytest.mark.gpu
def test_refusals():
    """Every GENIE_E_ARG of the contract through genie_ce_objective on real buffers: refused, logits and sums as they were; and the
    ValueErrors of the trainer."""
    import test_train_objective_cpu as CPU
    lib = pkg("_lib")
    shape = WINDOW_SHAPES[1]
    n_clips, T, S, vf, nfac = shape
    w = Window(shape, 1)
    for what, ob in CPU.refusals(T):
        with pytest.raises(lib.GenieHipError) as e:
            w.run(ob)
        assert e.value.code == lib.E_ARG, what
        assert np.array_equal(bits(w.buf.read().reshape(w.logits.shape)), bits(w.logits)), what
        assert (w.sums.cpu().numpy() == -7.0).all(), what
    d, s = w.run(w.objective(0.1, 1e-4, window_weights(T)))   # the same buffers still serve a good call
    assert np.isfinite(d).all() and s[2] > 0
    cfg, sd, _, _ = case("ln3")
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(z_loss=-1e-4),
               dict(z_loss=float("inf")), dict(frame_weights=(1, 1, 1)), dict(frame_weights=(1, 1, 1, 1, 1)),
               dict(frame_weights=(1, -1, 1, 1)), dict(frame_weights=(1, float("nan"), 1, 1)), dict(frame_weights=(1, 0, 0, 0))):
        with pytest.raises(ValueError):
            TD.make_trainer(cfg, sd, "exact", **kw)


@pytest.mark.gpu
def test_resume():
    """Two train_steps with the objective are bit-equal to one step, state_dict, a fresh trainer with the same settings on the stepped
    weights with load_state_dict, one step.  state_dict()["hyper"] carries the three settings; loading it into a trainer with another
    label_smoothing (or other weights) names them in the "different hyper-parameters" warning."""
    torch = torch_()
    cfg, sd, ids, labels = case("ln3")
    eps, zeta, weights = OM.settings("ln3")["all"]
    batch = {"input_ids": TD.dev(ids), "labels": TD.dev(labels)}
    kw = dict(lr=1e-3, weight_decay=0.01, label_smoothing=eps, z_loss=zeta, frame_weights=weights)
    two = TD.make_trainer(cfg, sd, "exact", **kw)
    two.train_step(batch)
    state = two.state_dict()
    assert state["hyper"]["label_smoothing"] == eps and state["hyper"]["z_loss"] == zeta and state["hyper"]["frame_weights"] == weights
    sd1 = {k: v.detach().cpu().numpy().copy() for k, v in two.model.state_dict().items()}
    two.train_step(batch)
    resumed = TD.make_trainer(cfg, sd1, "exact", **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        resumed.load_state_dict(state)
    resumed.train_step(batch)
    assert torch.equal(resumed.params, two.params)
    assert torch.equal(resumed.exp_avg, two.exp_avg) and torch.equal(resumed.exp_avg_sq, two.exp_avg_sq)
    other = TD.make_trainer(cfg, sd1, "exact", **{**kw, "label_smoothing": 0.2, "frame_weights": None})
    with pytest.warns(UserWarning, match=r"different hyper-parameters.*label_smoothing=0\.1->0\.2.*frame_weights=\(1\.0, 0\.0, 0\.5, 2\.0\)->None"):
        other.load_state_dict(state)
    assert TD.make_trainer(cfg, sd, "exact").state_dict()["hyper"]["frame_weights"] is None


# ---------------------------------------------------------------------------------------------- 8. the CLI
@pytest.mark.gpu
def test_train_cli_objective(tmp_path):
    """tools/train.py --synthetic 16 --model tiny --label_smoothing 0.1 --z_loss 1e-4 --frame_loss_weights 1,1,2,2 --max_train_steps 2
    in a fresh child process: the step lines print `ce` next to train_loss, both finite and different; trainer_state.pt in the
    checkpoint holds the settings.  Beside it, a run whose weight count is not the window's ends with a `train.py:` message."""
    torch = torch_()
    base = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "16", "--model", "tiny", "--max_train_steps", "2",
            "--seed", "1", "--precision", "exact", "--per_device_eval_batch_size", "2"]
    good = subprocess.Popen(base + ["--label_smoothing", "0.1", "--z_loss", "1e-4", "--frame_loss_weights", "1,1,2,2",
                                    "--output_dir", str(tmp_path / "on")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    count = subprocess.Popen(base + ["--frame_loss_weights", "1,1,2", "--output_dir", str(tmp_path / "count")], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
    out, err = good.communicate(timeout=600)
    assert good.returncode == 0, out[-2000:] + err[-2000:]
    steps = [ln for ln in out.splitlines() if re.match(r"step \d+: train_loss", ln)]
    assert len(steps) == 2, out[-2000:]
    for ln in steps:
        m = re.match(r"step \d+: train_loss ([0-9.]+) ce ([0-9.]+) ppl", ln)
        assert m, ln
        assert np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2))) and m.group(1) != m.group(2), ln
    hyper = torch.load(tmp_path / "on" / "final_checkpt" / "trainer_state.pt", map_location="cpu")["hyper"]
    assert hyper["label_smoothing"] == 0.1 and hyper["z_loss"] == 1e-4 and tuple(hyper["frame_weights"]) == (1.0, 1.0, 2.0, 2.0)
    _, err = count.communicate(timeout=600)
    assert count.returncode not in (0, None) and err.strip().splitlines()[-1].startswith("train.py: --frame_loss_weights has 3 entries"), err[-800:]
