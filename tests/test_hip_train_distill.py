"""Distilling a teacher into a student (include/genie_hip.h, "Distillation"; ce_distill_kernel in csrc/kernels_loss.hip): the loss
launch alone against the float64 contract, neutral calls against the calls of before, trainer steps against the float64 autograd model
of tests/distill_model.py in the three precisions with precomputed teacher logits and with a live teacher, composition with
recomputation, accumulation, frozen tensors, dropout and stale memory, a short training run, refusals and the CLI.

Step cases: ln3 and qk3 of tests/objective_model.py::STEP_CASES; teachers of another width and depth (tests/distill_model.py::TEACHERS:
H 2, d 128, 2 layers, LayerNorm for ln3; H 2, d 64, 2 layers, LayerNorm for qk3), their logits from the float64 forward rounded to f32.
Settings (tests/distill_model.py::STEP_SETTINGS): alpha 1 tau 1; alpha 0.5 tau 2; alpha 0.5 tau 2 with eps 0.1, zeta 1e-2 and the
case's frame weights -- tests/test_train_distill_cpu.py shows that each moves the loss and every gradient tensor by far more than the bars.

The GPU tests need an MI355X (``-m gpu``); tests/test_train_distill_cpu.py holds what runs anywhere.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distill_model as DS
import objective_model as OM
import test_hip_train_dropout as TD
import test_hip_train_objective as TOBJ
import test_train_distill_cpu as CPU
from conftest import REPO, pkg, record_measure
from oracle import genie_train_oracle as TO

GRAD_TOL, LOSS_TOL = 1e-4, 1e-5          # the bars of tests/test_hip_train_geometry.py, restated
BF16_BARS = TOBJ.BF16_BARS               # stated in tests/test_hip_train_objective.py: the loss kernel is f32 in every precision
TAGS = list(DS.STEP_SETTINGS)
SEED = 3


def torch_():
    return pytest.importorskip("torch")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def close(a, b):
    """Sums and losses of two runs: the double atomics of the loss kernels add the workgroups' partial sums in any order."""
    a, b = (np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float64) for v in (a, b))
    return bool(np.allclose(a, b, rtol=1e-12, atol=0))


def case(name):
    return CPU.make_case(name)


def teacher_logits(name):
    return TD.dev(CPU.teacher_case(name)[2].copy())


def trainer(name, precision, tag, p=0.0, **kw):
    cfg, sd, _, _ = case(name)
    if tag != "none":
        alpha, tau, eps, zeta, weights = DS.step_setting(name, tag)
        kw = dict(distill_alpha=alpha, distill_temperature=tau, label_smoothing=eps, z_loss=zeta, frame_weights=weights, **kw)
    return TD.make_trainer(cfg, sd, precision, p, **kw)


def teacher_model(name, precision):
    cfg_t, sd_t, _ = CPU.teacher_case(name)
    return pkg("st_mask_git").STMaskGIT(cfg_t, precision=precision).load_numpy_state_dict(sd_t).to("cuda")


def grads_of(tr):
    return {k: v.cpu().numpy() for k, v in tr.gradients().items()}


def check_f32_step(what, name, tag, tr, loss, acc, model, p=0.0):
    """Loss, last_ce, last_kd, last_teacher_ce at LOSS_TOL (relative), acc at 1e-7, every gradient tensor at GRAD_TOL."""
    loss_o, g_o, ce_o, acc_o, kd_o, tce_o = model
    worst = {k: TD.rel_err(g, g_o[k]) for k, g in grads_of(tr).items()}
    assert set(worst) <= set(g_o)
    top = max(worst.items(), key=lambda kv: kv[1])
    rel = {"loss": abs(float(loss) - loss_o) / abs(loss_o), "ce": abs(float(tr.last_ce) - ce_o) / ce_o,
           "kd": abs(float(tr.last_kd) - kd_o) / kd_o, "teacher_ce": abs(float(tr.last_teacher_ce) - tce_o) / tce_o}
    record_measure(f"train_distill/{what}/{name}/{tag}", top[1])
    print(f"train_distill/{what}/{name}/{tag}: " + ", ".join(f"{k} rel {v:.2e}" for k, v in rel.items()) + f", worst tensor {top[0]} {top[1]:.3e}")
    assert tr.sums.numel() == 7 and all(t.is_cuda and t.dim() == 0 for t in (tr.last_ce, tr.last_kd, tr.last_teacher_ce))
    assert all(v < LOSS_TOL for v in rel.values()), rel
    assert abs(float(acc) - acc_o) < 1e-7
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 1. the loss launch alone
class Window:
    """One shape's device buffers: student and teacher logits each between guard regions (tests/test_hip_train_ema.py::Guarded), ids,
    labels, and ten doubles of sums pre-filled with a sentinel."""

    def __init__(self, shape, scale):
        import test_hip_train_ema as TE
        torch = torch_()
        self.shape = shape
        self.logits, self.teacher, self.ids, self.labels, self.mask_id = CPU.window_inputs(shape, scale)
        self.buf = TE.Guarded(self.logits.reshape(-1).copy())
        self.tbuf = TE.Guarded(self.teacher.reshape(-1).copy())
        self.d_ids, self.d_labels = TD.dev(self.ids.copy()), TD.dev(self.labels.copy())
        self.sums = torch.empty(10, dtype=torch.float64, device="cuda")
        self.lib = pkg("_lib")
        self.L = self.lib.load()

    def reset(self):
        torch = torch_()
        self.buf.f[self.buf.lo:self.buf.lo + self.buf.n].copy_(torch.from_numpy(self.logits.reshape(-1).copy()))
        self.sums.fill_(-7.0)

    def objective(self, eps=0.0, zeta=0.0, weights=None):
        if eps == 0.0 and zeta == 0.0 and weights is None:
            return None
        ob = self.lib.Objective(label_smoothing=eps, z_loss=zeta, n_frames=0 if weights is None else len(weights))
        for t, v in enumerate(weights or ()):
            ob.frame_weight[t] = v
        return ob

    def call(self, ob, ds, teacher_ptr):
        torch = torch_()
        n_clips, T, S, vf, nfac = self.shape
        return self.L.genie_ce_distill(self.buf.ptr, teacher_ptr, self.d_ids.data_ptr(), self.d_labels.data_ptr(), n_clips, T, S, vf, nfac,
                                       self.mask_id, ob, ds, self.sums.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def run(self, alpha, tau, eps=0.0, zeta=0.0, weights=None):
        """genie_ce_distill on a fresh copy of the student logits -> (d logits f32 (N, V), sums (10,)); read() checks the guards."""
        self.reset()
        ds = self.lib.Distill(alpha=alpha, temperature=tau, teacher_logits=None)   # the call's own argument carries the rows
        self.lib.check(self.call(self.objective(eps, zeta, weights), ds, self.tbuf.ptr), "genie_ce_distill")
        torch_().cuda.synchronize()
        return self.buf.read().reshape(self.logits.shape), self.sums.cpu().numpy()

    def run_parent(self, ob):
        torch = torch_()
        n_clips, T, S, vf, nfac = self.shape
        self.reset()
        self.lib.check(self.L.genie_ce_objective(self.buf.ptr, self.d_ids.data_ptr(), self.d_labels.data_ptr(), n_clips, T, S, vf, nfac,
                                                 self.mask_id, ob, self.sums.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "genie_ce_objective")
        torch.cuda.synchronize()
        return self.buf.read().reshape(self.logits.shape), self.sums.cpu().numpy()

    def model(self, f32=False, **kw):
        n_clips, T, S, vf, nfac = self.shape
        f = DS.ce_distill_f32 if f32 else DS.ce_distill
        return f(self.logits, self.teacher, self.ids, self.labels, T, S, vf, nfac, self.mask_id, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("shape", CPU.WINDOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_launch_against_the_contract(shape, scale):
    """genie_ce_distill on guarded buffers, the row mixture of tests/test_train_distill_cpu.py::window_inputs.  The floor of a shape is
    genie_ce_objective(obj = NULL) against float64 on the same student logits (worst element of d logits over the model's largest).  At
    alpha 1 tau 1, alpha 0.5 tau 2, alpha 0.3 tau 0.5, and alpha 0.5 tau 2 with eps 0.1, zeta 1e-2 and frame weights (1, 0.5, 0, 2)[t % 4],
    d logits is within 4 x the larger of that floor and the f32 restatement's own distance from float64 at the same setting; the seven
    sums are within LOSS_TOL (hits, W, n exact); rows of uncounted and zero-weight tokens are exactly zero; the teacher buffer keeps its
    bits and its guards; a second launch gives the same bits; sums beyond the seventh keep their sentinel.
    Measured on an MI355X over the 48 figures: the floor is 6.2e-8 to 2.0e-7, the kernel's error 3.0e-8 to 2.3e-7, the ratio of the error
    to max(floor, restatement) 0.26 to 1.21 (the largest at 3x3x5x512x2, scale 1, alpha 0.5 tau 2: 1.12e-7 against 9.2e-8); the sums are
    within 5e-7 (profiles/train_distill.txt)."""
    n_clips, T, S, vf, nfac = shape
    tag = "x".join(map(str, shape)) + f"/s{scale}"
    w = Window(shape, scale)
    counted = OM.counted_mask(w.ids, T, S, w.mask_id).reshape(-1)
    d_par, s_par = w.run_parent(None)
    d_m, _ = OM.ce_objective(w.logits, w.ids, w.labels, T, S, vf, nfac, w.mask_id)
    floor = float(np.abs(d_par - d_m).max() / np.abs(d_m).max())
    print(f"train_distill/window/{tag}: parent floor {floor:.3e}")
    assert 0 < floor < 1e-5
    ww = CPU.window_weights(T)
    wn = np.broadcast_to(np.asarray(ww)[None, :, None], (n_clips, T, S)).reshape(-1)
    for key in CPU.WINDOW_SETTINGS:
        kw = CPU.window_args(shape, key)
        d, s = w.run(**kw)
        d_m, s_m = w.model(**kw)
        d_r, _ = w.model(f32=True, **kw)
        big = np.abs(d_m).max()
        err, own = float(np.abs(d - d_m).max() / big), float(np.abs(d_r - d_m).max() / big)
        base = max(floor, own)
        record_measure(f"train_distill/window/{tag}/{key}", err)
        print(f"train_distill/window/{tag}: {key} {err:.3e} = {err / base:.2f} x max(floor {floor:.3e}, restatement {own:.3e}); sums "
              + " ".join(f"{abs(a - b) / max(abs(b), 1e-300):.1e}" for a, b in zip(s[:7], s_m)))
        assert np.isfinite(d).all() and np.isfinite(s).all()
        assert err <= 4 * base, (key, err, floor, own)
        assert all(abs(a - b) <= LOSS_TOL * abs(b) for a, b in zip(s[:7], s_m)), (key, s[:7], s_m)
        assert s[2] == s_m[2] and s[4] == s_m[4] and s[1] == s_m[1], "counts and hits are integers"
        dead = ~counted | (wn == 0.0) if kw["weights"] is not None else ~counted
        assert dead.any() and not d[dead].any()
        assert np.array_equal(bits(w.tbuf.read()), bits(w.teacher.reshape(-1))), "the teacher logits were written"
        d2, s2 = w.run(**kw)
        assert np.array_equal(bits(d2), bits(d)), "a second launch from the same inputs gave other bits"
        assert (s[7:] == -7.0).all() and (s2[7:] == -7.0).all()


# ---------------------------------------------------------------------------------------------- 2. neutral is today's call
@pytest.mark.gpu
def test_neutral_loss_launch_is_the_objective_call():
    """genie_ce_distill with ds = NULL, and with alpha = 0 and a teacher pointer into a small poisoned buffer (far too short for the rows:
    it must never be read), gives genie_ce_objective's bits and its number of sums, without and with an objective."""
    torch = torch_()
    shape = CPU.WINDOW_SHAPES[1]
    T = shape[1]
    w = Window(shape, 1)
    poison = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    for ob, n_sums in ((None, 3), (w.objective(0.1, 1e-2, CPU.window_weights(T)), 5)):
        d0, s0 = w.run_parent(ob)
        for ds, ptr in ((None, None), (None, poison.data_ptr()), (w.lib.Distill(alpha=0.0, temperature=2.0, teacher_logits=poison.data_ptr()),
                                                                poison.data_ptr())):
            w.reset()
            w.lib.check(w.call(ob, ds, ptr), "genie_ce_distill")
            torch.cuda.synchronize()
            d, s = w.buf.read().reshape(w.logits.shape), w.sums.cpu().numpy()
            assert np.array_equal(bits(d), bits(d0))
            assert close(s[:n_sums], s0[:n_sums])
            assert (s[n_sums:] == -7.0).all()
    assert bool(torch.isnan(poison).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_neutral_trainer_is_the_trainer_of_before(precision):
    """A trainer given teacher=None, distill_alpha=0 against one built without the arguments: three sums (five with an objective), no
    teacher buffer, torch.equal flat gradients and the same loss.  Then the entry points themselves on the trainer's buffers, the
    activation buffer pre-filled with 0xFF bytes before every call: genie_train_forward_distill with ds = NULL, and with alpha = 0 and a
    poisoned teacher pointer, leaves the whole activation buffer -- every saved activation and, in its logits slot, d loss / d logits --
    torch.equal to what genie_train_forward_obj leaves there, and writes its number of sums."""
    torch = torch_()
    cfg, sd, ids, labels = case("ln3")
    ids, labels = TD.dev(ids), TD.dev(labels)
    for kw, n_sums in ((dict(), 3), (dict(label_smoothing=0.1), 5)):
        plain = TD.make_trainer(cfg, sd, precision, **kw)
        l0, _ = plain.forward_backward(ids, labels)
        tr = TD.make_trainer(cfg, sd, precision, teacher=None, distill_alpha=0.0, distill_temperature=2.0, **kw)
        assert tr.sums.numel() == n_sums and tr._teacher_logits is None and not tr._distilling
        l1, _ = tr.forward_backward(ids, labels)
        assert torch.equal(tr.grads, plain.grads) and close(l0, l1) and close(tr.sums, plain.sums)
        assert tr.last_kd is None and tr.last_teacher_ce is None
        # the entry point itself, through the trainer's own buffers
        lib, L = pkg("_lib"), tr.lib
        poison = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
        acts, _ = tr._buffers(ids.shape[0])
        head = (tr.cfg, tr.w_table, ids.data_ptr(), labels.data_ptr(), ids.shape[0], acts.data_ptr(), acts.numel())
        sums = torch.full((10,), -7.0, dtype=torch.float64, device="cuda")
        acts.fill_(0xFF)
        lib.check(L.genie_train_forward_obj(*head, sums.data_ptr(), tr._stream(), None, tr.recompute, None, tr._objective), "genie_train_forward_obj")
        acts_obj = acts.clone()
        assert close(sums[:n_sums], plain.sums) and not bool((acts_obj == 0xFF).all())
        for ds in (None, lib.Distill(alpha=0.0, temperature=1.0, teacher_logits=poison.data_ptr())):
            sums.fill_(-7.0)
            acts.fill_(0xFF)
            lib.check(L.genie_train_forward_distill(*head, sums.data_ptr(), tr._stream(), None, tr.recompute, None, tr._objective, ds),
                      "genie_train_forward_distill")
            assert torch.equal(acts, acts_obj), f"{int((acts != acts_obj).sum())} bytes of the activation buffer differ from the _obj call's"
            assert close(sums[:n_sums], plain.sums) and bool((sums[n_sums:] == -7.0).all())


# ---------------------------------------------------------------------------------------------- 3. the step against float64
@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_vs_float64_model(name, precision, tag):
    """One step with the teacher's logits handed in through teacher_logits= against the float64 autograd model: loss, last_ce, last_kd,
    last_teacher_ce at LOSS_TOL, every gradient tensor at GRAD_TOL."""
    _, _, ids, labels = case(name)
    tr = trainer(name, precision, tag)
    loss, acc = tr.forward_backward(TD.dev(ids), TD.dev(labels), teacher_logits=teacher_logits(name))
    check_f32_step(precision, name, tag, tr, loss, acc, CPU.model_step(name, tag))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_bf16_vs_float64_model(name, tag):
    """The five statistics of tests/test_hip_train_bf16.py::check_vs_oracle for one bf16 step against the float64 model at the same
    setting, at the BF16_BARS of tests/test_hip_train_objective.py."""
    torch = torch_()
    import test_hip_train_bf16 as B16
    loss_o, g_o = CPU.model_step(name, tag)[:2]
    _, _, ids, labels = case(name)
    tr = trainer(name, "bf16", tag)
    loss, _ = tr.forward_backward(TD.dev(ids), TD.dev(labels), teacher_logits=teacher_logits(name))
    grads = grads_of(tr)
    worst = np.zeros(3)
    for k, g in grads.items():
        worst = np.maximum(worst, np.array(B16.errors(g, g_o[k])))
    gn, gn_o = float(torch.sqrt(tr.grad_sumsq()[0])), TO.grad_norm({k: g_o[k] for k in grads})
    stats = (float(worst[0]), float(worst[1]), float(worst[2]), abs(float(loss) - loss_o), abs(gn - gn_o) / gn_o)
    keys = ("median", "max", "fro", "loss", "norm")
    for key, v, bar in zip(keys, stats, BF16_BARS[name]):
        record_measure(f"train_distill/bf16/{name}/{tag}/{key}", v)
        print(f"train_distill/bf16/{name}/{tag}/{key}: {v:.3e} (bar {bar:.3e})")
    bad = {key: (v, bar) for key, v, bar in zip(keys, stats, BF16_BARS[name]) if not v < bar}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 4. the live teacher
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_live_teacher_vs_float64_model(name):
    """teacher= an `exact` HIP model with the teacher's weights instead of precomputed logits: the same bars (its logits are within the
    parity tolerance of the float64 forward's).  Two optimizer steps leave every teacher parameter torch.equal to its value before, and
    the teacher appears nowhere in the trainer's flat buffers or state; state_dict()["hyper"] carries alpha and tau, and loading it into a
    trainer with other values names them in the "different hyper-parameters" warning."""
    torch = torch_()
    tag = "a05t2+obj"
    _, _, ids, labels = case(name)
    teacher = teacher_model(name, "exact")
    before = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    tr = trainer(name, "exact", tag, teacher=teacher, lr=1e-3)
    n_flat = tr.params.numel()
    loss, acc = tr.forward_backward(TD.dev(ids), TD.dev(labels))
    check_f32_step("live", name, tag, tr, loss, acc, CPU.model_step(name, tag))
    assert tr._teacher_logits is not None and tr._teacher_logits.shape == (ids.shape[0], tr.config.T, tr.config.S, 2 * tr.config.factored_vocab_size)
    for _ in range(2):
        tr.train_step({"input_ids": TD.dev(ids), "labels": TD.dev(labels)})
    assert tr.completed_steps == 2 and tr.params.numel() == n_flat
    for k, v in teacher.state_dict().items():
        assert torch.equal(v, before[k]), k
    state = tr.state_dict()
    assert not any("teacher" in k for k in state["state"]) and state["hyper"]["distill_alpha"] == 0.5 and state["hyper"]["distill_temperature"] == 2.0
    other = trainer(name, "exact", "a1t1")
    with pytest.warns(UserWarning, match=r"different hyper-parameters.*distill_alpha=0\.5->1\.0.*distill_temperature=2\.0->1\.0"):
        other.load_state_dict(state)


@pytest.mark.gpu
def test_bf16_teacher_under_an_exact_student():
    """The teacher in bf16 under an exact student: it runs, the student's plain CE is unaffected (LOSS_TOL) and teacher_ce is within
    the bf16 loss bar of the float64 model's."""
    name, tag = "ln3", "a05t2"
    _, _, ids, labels = case(name)
    tr = trainer(name, "exact", tag, teacher=teacher_model(name, "bf16"))
    loss, _ = tr.forward_backward(TD.dev(ids), TD.dev(labels))
    _, _, ce_o, _, kd_o, tce_o = CPU.model_step(name, tag)
    print(f"train_distill/bf16-teacher/{name}: teacher_ce {float(tr.last_teacher_ce):.6f} (model {tce_o:.6f}), kd {float(tr.last_kd):.6f} (model {kd_o:.6f})")
    assert np.isfinite(float(loss)) and abs(float(tr.last_ce) - ce_o) < LOSS_TOL * ce_o
    assert abs(float(tr.last_teacher_ce) - tce_o) < BF16_BARS[name][3]


def conditioned_case(kind):
    """(student cfg, sd, teacher sd, batch, forward_backward keywords) of 2-layer models conditioned on action ids (action_vocab_size 3)
    or on action vectors (action_dim 3, with action_drop on one clip); the teacher has the student's shape and other weights."""
    import test_hip_train_frozen as TF
    cfg_v, sd_v, batch, kw_v = TF.action_case("vectors")
    g = np.random.default_rng(41)
    if kind == "vectors":
        cfg, sd, kw = cfg_v, sd_v, kw_v
    else:
        base = {k: v for k, v in vars(cfg_v).items() if k != "action_dim"}
        cfg = pkg("config").GenieConfig(**{**base, "action_vocab_size": 3})
        sd = {k: v for k, v in sd_v.items() if not k.startswith("action_")}
        sd["action_embed.weight"] = (0.5 * g.standard_normal((3, cfg.d_model))).astype(np.float32)
        kw = dict(action_ids=TD.dev(g.integers(0, 3, (2, cfg.T))))
    sd_t = {k: (v if k.startswith("action_") and "weight" not in k else (v * np.float32(0.75)).astype(v.dtype)) for k, v in sd.items()}
    return cfg, sd, sd_t, batch, kw


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ids", "vectors"])
def test_conditioned_teacher_equals_the_logits_route(kind):
    """An action-conditioned student and teacher (action ids with action_vocab_size = 3; action vectors with action_drop set on one
    clip -- the trainer takes action_drop with vectors only): the live teacher gets the student's actions and drop flags, and the step
    equals, bit for bit, the teacher_logits= route fed with the teacher's own logits under the same condition.  Without the condition the
    teacher's logits differ, so the test can tell."""
    torch = torch_()
    cfg, sd, sd_t, batch, kw = conditioned_case(kind)
    ids, lab = TD.dev(batch["input_ids"]), TD.dev(batch["labels"])
    B = ids.shape[0]
    teacher = pkg("st_mask_git").STMaskGIT(cfg, precision="exact").load_numpy_state_dict(sd_t).to("cuda")
    live = TD.make_trainer(cfg, sd, "exact", teacher=teacher, distill_alpha=0.5, distill_temperature=2.0)
    l0, _ = live.forward_backward(ids, lab, **kw)
    # the same condition, built by hand
    if kind == "ids":
        cond = teacher._cond(kw["action_ids"], B)
        other = teacher._cond((kw["action_ids"] + 1) % 3, B)
    else:
        cond = live._frame_cond(teacher, None, kw["action_vectors"], kw["action_drop"], B)
        other = live._frame_cond(teacher, None, kw["action_vectors"], None, B)
    tl = teacher.compute_logits_frames(ids, 0, cfg.T, "token", cond=cond).clone()
    tl_other = teacher.compute_logits_frames(ids, 0, cfg.T, "token", cond=other).clone()
    assert torch.equal(tl, live._teacher_logits) and not torch.equal(tl, tl_other)
    fed = TD.make_trainer(cfg, sd, "exact", distill_alpha=0.5, distill_temperature=2.0)
    l1, _ = fed.forward_backward(ids, lab, teacher_logits=tl, **kw)
    assert close(l0, l1) and torch.equal(live.grads, fed.grads) and close(live.sums, fed.sums)
    assert float(live.grads.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- 5. composition
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_recompute_accumulation_and_frozen_subset_same_bits(precision):
    """alpha 0.5 tau 2 with all objective knobs on ln3.  recompute=True gives the flat gradient bits of recompute=False.  Two accumulated
    micro-batches equal the same two calls made separately and summed in the documented order (first + second, f32).  trainable="*.mlp.*"
    gives the full step's bits on what it trains."""
    torch = torch_()
    name, tag = "ln3", "a05t2+obj"
    _, _, ids, labels = case(name)
    ids, labels, tl = TD.dev(ids), TD.dev(labels), teacher_logits(name)
    full = trainer(name, precision, tag)
    l0, _ = full.forward_backward(ids, labels, teacher_logits=tl)
    assert bool(torch.isfinite(full.grads).all()) and float(full.grads.abs().max()) > 0
    rec = trainer(name, precision, tag, recompute=True)
    l1, _ = rec.forward_backward(ids, labels, teacher_logits=tl)
    assert torch.equal(rec.grads, full.grads) and close(l0, l1) and close(rec.sums, full.sums)
    frozen = trainer(name, precision, tag, trainable="*.mlp.*")
    frozen.forward_backward(ids, labels, teacher_logits=tl)
    g_full = full.gradients()
    assert frozen.gradients() and all(torch.equal(g, g_full[k]) for k, g in frozen.gradients().items())
    # accumulation: the second micro-batch is the first with the clips exchanged (other tokens per clip slot, the same teacher rows exchanged)
    ids2, labels2, tl2 = ids.flip(0).contiguous(), labels.flip(0).contiguous(), tl.flip(0).contiguous()
    a = trainer(name, precision, tag)
    a.forward_backward(ids, labels, teacher_logits=tl)
    a.forward_backward(ids2, labels2, accumulate=True, teacher_logits=tl2)
    b = trainer(name, precision, tag)
    b.forward_backward(ids2, labels2, teacher_logits=tl2)
    second = b.grads.clone()
    assert not torch.equal(second, full.grads)
    if precision == "exact":   # the 16-bit products accumulate inside the GEMM (beta = 1): there the order is not first + second in f32
        assert torch.equal(a.grads, full.grads + second)
    else:
        assert float((a.grads - (full.grads + second)).abs().max()) <= 1e-5 * float(a.grads.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OM.STEP_CASES))
def test_step_with_dropout_vs_float64_model(name):
    """mlp_drop = 0.1 with alpha 0.5 tau 2 and the objective knobs, exact: against the float64 model with the same masks, at the bars of
    the step test."""
    tag = "a05t2+obj"
    _, _, ids, labels = case(name)
    tr = trainer(name, "exact", tag, 0.1, dropout_seed=SEED)
    loss, acc = tr.forward_backward(TD.dev(ids), TD.dev(labels), teacher_logits=teacher_logits(name))
    model = CPU.model_step(name, tag, 0.1, SEED)
    assert abs(model[0] - CPU.model_step(name, tag)[0]) > 100 * LOSS_TOL * model[0], "the masks changed nothing: the case tests no dropout"
    check_f32_step("exact+drop", name, tag, tr, loss, acc, model)


@pytest.mark.gpu
@pytest.mark.parametrize("recompute", [False, True])
def test_stale_memory(recompute):
    """The activation buffer, the workspace, the teacher logits buffer and the teacher's workspace pre-filled with 0xFF bytes
    (tests/stale_memory.py) give the bits of a run on zeroed buffers."""
    import stale_memory as SM
    torch = torch_()
    name, tag = "ln3", "a05t2+obj"
    _, _, ids, labels = case(name)
    ids, labels = TD.dev(ids), TD.dev(labels)
    out = []
    for byte in (0x00, 0xFF):
        teacher = teacher_model(name, "exact")
        tr = trainer(name, "exact", tag, teacher=teacher, recompute=recompute)
        with SM.poisoned(byte, sentinel=tr.config.image_vocab_size):
            tr._buffers(ids.shape[0])
        for t in (tr._acts, tr._ws, tr._teacher_logits, teacher._ws):
            assert t is not None
            SM.poison_tensor(t, byte)
        loss, _ = tr.forward_backward(ids, labels)
        out.append((float(loss), tr.grads.clone(), tr.sums.clone()))
    assert np.isfinite(out[0][0]) and close(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1]) and close(out[0][2], out[1][2])


# ---------------------------------------------------------------------------------------------- 6. it trains
@pytest.mark.gpu
def test_it_trains():
    """ln3, alpha = 1, one fixed batch, lr 1e-3, 20 optimizer steps: last_kd after the last step is lower than after the first."""
    name = "ln3"
    cfg, sd, ids, labels = case(name)
    tr = TD.make_trainer(cfg, sd, "exact", distill_alpha=1.0, lr=1e-3)
    batch = {"input_ids": TD.dev(ids), "labels": TD.dev(labels), "teacher_logits": teacher_logits(name)}
    kd = []
    for _ in range(20):
        out = tr.train_step(batch)
        kd.append(out["kd"])
    assert set(out) == {"loss", "acc", "ce", "kd", "teacher_ce", "grad_norm", "lr"}
    first, last = float(kd[0]), float(kd[-1])
    print(f"train_distill/trains: kd {first:.4f} -> {last:.4f}")
    assert np.isfinite(last) and last < first


# ---------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.gpu
def test_refusals():
    """Every GENIE_E_ARG of the contract through genie_ce_distill on real buffers: refused, and the sentinel-filled logits, sums and
    teacher buffer are as they were; the trainer's ValueErrors."""
    import test_train_objective_cpu as OC
    torch = torch_()
    lib = pkg("_lib")
    shape = CPU.WINDOW_SHAPES[1]
    n_clips, T, S, vf, nfac = shape
    w = Window(shape, 1)

    def refused(what, ob, ds, ptr):
        w.reset()
        assert w.call(ob, ds, ptr) == lib.E_ARG, what
        torch.cuda.synchronize()
        assert np.array_equal(bits(w.buf.read().reshape(w.logits.shape)), bits(w.logits)), what
        assert np.array_equal(bits(w.tbuf.read()), bits(w.teacher.reshape(-1))), what
        assert (w.sums.cpu().numpy() == -7.0).all(), what
    for what, alpha, tau, with_teacher in CPU.refusals():
        refused(what, None, lib.Distill(alpha=alpha, temperature=tau), w.tbuf.ptr if with_teacher else None)
    good = lib.Distill(alpha=0.5, temperature=2.0)
    for what, ob in OC.refusals(T):
        refused(what, ob, good, w.tbuf.ptr)
    refused("teacher == logits", None, good, w.buf.ptr)
    refused("teacher ends inside logits", None, good, w.buf.ptr - 4 * 16)
    refused("teacher overlaps the sums", None, good, w.sums.data_ptr() - 4 * (w.buf.n - 2))
    d, s = w.run(0.5, 2.0)   # the same buffers still serve a good call
    assert np.isfinite(d).all() and s[4] > 0 and s[5] > 0
    cfg, sd, ids, labels = case("ln3")
    for kw in (dict(distill_alpha=-0.1), dict(distill_alpha=1.5), dict(distill_alpha=float("nan")), dict(distill_temperature=0.0),
               dict(distill_alpha=0.5, distill_temperature=float("inf"))):
        with pytest.raises(ValueError):
            TD.make_trainer(cfg, sd, "exact", **kw)
    cfg_t = pkg("config").GenieConfig(**{**vars(CPU.teacher_case("ln3")[0]), "T": 8})
    other_t = pkg("st_mask_git").STMaskGIT(cfg_t, precision="exact").to("cuda")
    with pytest.raises(ValueError):
        TD.make_trainer(cfg, sd, "exact", teacher=other_t, distill_alpha=0.5)
    tr = TD.make_trainer(cfg, sd, "exact", distill_alpha=0.5)
    with pytest.raises(ValueError):   # alpha > 0 with neither a teacher nor per-call logits
        tr.forward_backward(TD.dev(ids), TD.dev(labels))
    with pytest.raises(ValueError):   # logits for a trainer that does not distil
        TD.make_trainer(cfg, sd, "exact").forward_backward(TD.dev(ids), TD.dev(labels), teacher_logits=teacher_logits("ln3"))


# ---------------------------------------------------------------------------------------------- 8. the CLI
@pytest.mark.gpu
def test_train_cli_distill(tmp_path):
    """tools/train.py --synthetic 8 --max_train_steps 2 --teacher_path <a directory saved here> --distill_alpha 0.5 --distill_temperature 2
    in a fresh child process: it exits 0, the step lines print kd and teacher_ce, and the checkpoint loads with from_pretrained."""
    STMaskGIT = pkg("st_mask_git").STMaskGIT
    cfg_t = pkg("config").GenieConfig(num_layers=3, num_heads=2, d_model=128, T=4, S=16, num_factored_vocabs=2, qk_norm=False, num_prompt_frames=2)
    sd_t = pkg("synthetic").make_state_dict(cfg_t, seed=5, law="conditioned")
    STMaskGIT(cfg_t, precision="exact").load_numpy_state_dict(sd_t).save_pretrained(str(tmp_path / "teacher"))
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--model", "tiny",
                          "--max_train_steps", "2", "--seed", "1", "--precision", "exact", "--per_device_train_batch_size", "2",
                          "--per_device_eval_batch_size", "1", "--teacher_path", str(tmp_path / "teacher"), "--distill_alpha", "0.5",
                          "--distill_temperature", "2", "--output_dir", str(tmp_path / "out")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    steps = [ln for ln in run.stdout.splitlines() if re.match(r"step \d+: train_loss", ln)]
    assert len(steps) == 2, run.stdout[-2000:]
    for ln in steps:
        m = re.match(r"step \d+: train_loss ([0-9.]+) ce ([0-9.]+) kd ([0-9.]+) teacher_ce ([0-9.]+) ppl", ln)
        assert m, ln
        assert all(np.isfinite(float(v)) for v in m.groups()) and float(m.group(3)) > 0, ln
    model = STMaskGIT.from_pretrained(str(tmp_path / "out" / "final_checkpt"), precision="exact")
    assert model.config.d_model == 64 and model.config.num_layers == 2 and not any(k.startswith("teacher") for k in model.state_dict())
