"""Training with MLP dropout (config.mlp_drop > 0; include/genie_hip.h, "MLP dropout"; csrc/kernels_dropout.hip): the mask kernel
against the NumPy law, trainer steps against the float64 model of tests/dropout_model.py driven with the SAME masks, p = 0 against
the step without dropout, recomputation, determinism and resume, stale memory, inference, and the CLI.

(H, d, T, S, B, qk_norm, use_mup, layers), tokens, what the case reaches (the cases of tests/test_hip_train_recompute.py, built the same way):
  ln3     (2, 64, 4, 16, 2, F, F, 3)     128   LayerNorm blocks
  qk3     (2, 128, 8, 16, 3, T, F, 3)    384   Identity norms, odd batch: the site 1 pass writes the next layer's operand
  qk2k    (4, 256, 8, 64, 5, T, F, 2)    2560  recomputation only: fc2 above the limits of the small-problem GEMM kernel

The GPU tests need an MI355X (``-m gpu``); tests/test_train_dropout_cpu.py holds what runs anywhere.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dropout_model as DM
from conftest import REPO, pkg, record_measure
from oracle import genie_train_oracle as TO

GRAD_TOL, LOSS_TOL = 1e-4, 1e-5          # the bars of tests/test_hip_train_geometry.py, restated
CASES = {
    "ln3": (2, 64, 4, 16, 2, False, False, 3),
    "qk3": (2, 128, 8, 16, 3, True, False, 3),
    "qk2k": (4, 256, 8, 64, 5, True, False, 2),
}
STEP_CASES = ["ln3", "qk3"]
P_VALUES = [0.1, 0.5]
PRECISIONS = ["exact", "f16x3", "bf16"]
SEED = 3   # dropout_seed of the steps compared with the model

# bf16 bars (median / max / Frobenius / loss / global norm; tests/test_hip_train_bf16.py::errors and check_vs_oracle): the project's
# 3x rule -- 3x the maximum, over 24 data seeds, of the error of the p = 0 bf16 step against the float64 model (all-ones masks), the
# same yardstick the dropped steps are held to.  p = 0 is the step without dropout bit for bit (test_p0_is_the_step_without_dropout).
# Data seed k draws other clips and other collator draws (make_case(name, k), k = 0 .. 23; the weights stay).  Printed on an MI355X by
# bf16_stats(name, 0.0, k) over those seeds (p50 / p95 / max; profiles/train_dropout.txt):
#   ln3   median 1.64e-03 / 2.24e-03 / 2.32e-03   max 8.17e-03 / 1.19e-02 / 1.46e-02   fro 7.36e-03 / 8.28e-03 / 9.42e-03
#         loss 1.05e-03 / 2.09e-03 / 2.42e-03     norm 3.94e-04 / 9.30e-04 / 1.14e-03
#   qk3   median 2.32e-03 / 2.87e-03 / 3.66e-03   max 1.14e-02 / 1.65e-02 / 2.29e-02   fro 9.10e-03 / 1.17e-02 / 1.26e-02
#         loss 5.80e-04 / 1.66e-03 / 1.85e-03     norm 6.68e-04 / 1.26e-03 / 1.37e-03
BF16_BARS = {
    "ln3": (3 * 2.32e-3, 3 * 1.46e-2, 3 * 9.42e-3, 3 * 2.42e-3, 3 * 1.14e-3),
    "qk3": (3 * 3.66e-3, 3 * 2.29e-2, 3 * 1.26e-2, 3 * 1.85e-3, 3 * 1.37e-3),
}


@functools.lru_cache(maxsize=None)
def make_case(name, data_seed=0):
    """(cfg, sd, input_ids, labels) as NumPy with the seeds of tests/test_hip_train_recompute.py::make_case; data_seed > 0 draws other
    clips and other collator draws (the bf16 floor).  Computed once, shared, never written to."""
    H, d, T, S, B, qk_norm, use_mup, layers = CASES[name]
    cfg = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=T // 2, use_mup=use_mup)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=77 + H, law="conditioned")
    batch = TO.maskgit_collate(syn.make_clips(B, cfg, seed=900 + d + 1000 * data_seed), cfg, TO.NumpyDraws(5 + B + 1000 * data_seed))
    return cfg, sd, batch["input_ids"], batch["labels"]


def f32p(p):
    return float(np.float32(p))   # the library's p is a float


@functools.lru_cache(maxsize=None)
def model_step(name, p, data_seed=0):
    """(loss, grads) of the float64 model with the masks of (SEED, call 0) at p; p = 0: no dropout."""
    cfg, sd, ids, labels = make_case(name, data_seed)
    masks = DM.step_masks(cfg, ids.shape[0], SEED, 0, p) if p else None
    return DM.autograd_step(cfg, sd, ids, labels, masks, f32p(p))


def dev(a):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_trainer(cfg, sd, precision, p=0.0, **kw):
    cfg = cfg.shallow_copy()
    cfg.mlp_drop = p
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    return pkg("train").GenieTrainer(model, **kw)


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


# ---------------------------------------------------------------------------------------------- the mask kernel
GUARD = 4096


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5, 4097, 2 * 64 * 256 + 2])
def test_mask_kernel_is_the_numpy_law(n):
    """genie_dropout_mask against keep_mask, bit-exact, for lengths that are no multiple of four and span more than one workgroup, at
    several (p, seed, call, layer, site) -- a seed above 2^32 and a call near 2^32 among them.  The output is pre-filled with 0xFF and
    sits between two guard regions: every byte written, nothing outside."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for p, seed, call, layer, site in ((0.1, 0, 0, 0, 0), (0.5, 1, 0, 0, 1), (0.1, 2 ** 40 + 12345, 7, 31, 1), (0.9, 5, 2 ** 32 - 1, 2, 0),
                                       (0.0, 9, 1, 0, 0)):
        buf = torch.full((n + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[:GUARD] = 0x5A
        buf[GUARD + n:] = 0x5A
        dr = lib.Dropout(p=p, call=call, seed=seed)
        lib.check(L.genie_dropout_mask(dr, layer, site, n, buf.data_ptr() + GUARD, st), "genie_dropout_mask")
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:GUARD] == 0x5A).all() and (out[GUARD + n:] == 0x5A).all(), "the kernel wrote outside keep"
        got = out[GUARD:GUARD + n]
        assert not (got == 0xFF).any(), "bytes of keep were not written"
        want = DM.keep_mask(seed, call, layer, site, n, p)
        assert np.array_equal(got, want), (p, seed, call, layer, site, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------- the step against the float64 model
def step_errors(name, precision, p, data_seed=0, **kw):
    """One forward_backward (dropout_seed SEED, call 0) -> (loss, {tensor: gradient}, trainer)."""
    cfg, sd, ids, labels = make_case(name, data_seed)
    tr = make_trainer(cfg, sd, precision, p, dropout_seed=SEED, **kw)
    loss, _ = tr.forward_backward(dev(ids), dev(labels))
    return float(loss), {k: v.cpu().numpy() for k, v in tr.gradients().items()}, tr


def check_f32_class(name, precision, p, margin):
    loss_o, g_o = model_step(name, p)
    loss, grads, _ = step_errors(name, precision, p)
    worst = {k: rel_err(g, g_o[k]) for k, g in grads.items()}
    assert set(worst) <= set(g_o)
    top = max(worst.items(), key=lambda kv: kv[1])
    dl = abs(loss - loss_o) / abs(loss_o)
    record_measure(f"train_dropout/{precision}/{name}/p{p}", top[1])
    print(f"train_dropout/{precision}/{name}/p{p}: loss {loss:.8f} (model {loss_o:.8f}, rel {dl:.2e}), worst tensor {top[0]} {top[1]:.3e}")
    assert dl < margin * LOSS_TOL
    bad = {k: v for k, v in worst.items() if v >= margin * GRAD_TOL}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_cases_leave_half_the_bar_without_dropout(name, precision):
    """The validity condition of the cases below: at p = 0 the step is within HALF of GRAD_TOL / LOSS_TOL of the float64 model.
    Measured on an MI355X, worst tensor: exact ln3 9.2e-07, qk3 1.7e-06; f16x3 ln3 5.3e-07, qk3 9.3e-07 (loss: 1.7e-08 at most)."""
    check_f32_class(name, precision, 0.0, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("p", P_VALUES)
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_step_vs_float64_model(name, precision, p):
    """Loss (LOSS_TOL, relative) and every gradient tensor (GRAD_TOL, largest error over the tensor's largest element) of one step with
    dropout against the float64 model with the helper's masks.  One wrong mask bit at either site of any layer moves a gradient by far
    more than the bar.  Measured on an MI355X, worst tensor: exact ln3 8.1e-07 / 1.3e-06 (p 0.1 / 0.5), qk3 1.8e-06 / 1.4e-06;
    f16x3 ln3 5.0e-07 / 7.7e-07, qk3 8.6e-07 / 7.5e-07 (loss: 4.4e-08 at most)."""
    check_f32_class(name, precision, p, 1.0)


def bf16_stats(name, p, data_seed=0):
    """The five statistics of tests/test_hip_train_bf16.py::check_vs_oracle for one bf16 step against the float64 model."""
    torch = pytest.importorskip("torch")
    import test_hip_train_bf16 as B16
    loss_o, g_o = model_step(name, p, data_seed)
    loss, grads, tr = step_errors(name, "bf16", p, data_seed)
    worst = np.zeros(3)
    for k, g in grads.items():
        worst = np.maximum(worst, np.array(B16.errors(g, g_o[k])))
    gn, gn_o = float(torch.sqrt(tr.grad_sumsq()[0])), TO.grad_norm({k: g_o[k] for k in grads})
    return float(worst[0]), float(worst[1]), float(worst[2]), abs(loss - loss_o), abs(gn - gn_o) / gn_o


@pytest.mark.gpu
@pytest.mark.parametrize("p", P_VALUES)
@pytest.mark.parametrize("name", STEP_CASES)
def test_step_bf16_vs_float64_model(name, p):
    """The bf16 step with dropout against the float64 model at BF16_BARS (see there).  Measured on an MI355X (median / max / Frobenius /
    loss / norm): ln3 p 0.1 1.81e-03 / 1.04e-02 / 7.43e-03 / 1.50e-04 / 4.87e-04, p 0.5 2.02e-03 / 1.25e-02 / 1.03e-02 / 1.68e-03 / 1.74e-04;
    qk3 p 0.1 2.70e-03 / 1.09e-02 / 1.00e-02 / 1.38e-04 / 3.93e-04, p 0.5 2.80e-03 / 1.40e-02 / 1.14e-02 / 4.64e-03 / 1.20e-03."""
    stats = bf16_stats(name, p)
    for key, v, bar in zip(("median", "max", "fro", "loss", "norm"), stats, BF16_BARS[name]):
        record_measure(f"train_dropout/bf16/{name}/p{p}/{key}", v)
        print(f"train_dropout/bf16/{name}/p{p}/{key}: {v:.3e} (bar {bar:.3e})")
    bad = {key: (v, bar) for key, v, bar in zip(("median", "max", "fro", "loss", "norm"), stats, BF16_BARS[name]) if not v < bar}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- p = 0 is the step without dropout
def profiled(tr, ids, labels):
    """The flat gradients of one forward_backward and the {class:kernel name -> launches} table of the whole step."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    table = {}
    lib.check(L.genie_profile_enable(0x3F), "profile_enable")
    L.genie_profile_reset()
    try:
        tr.forward_backward(ids, labels)
        torch.cuda.synchronize()
        for kc in range(6):
            kbuf = ctypes.create_string_buffer(16384)
            lib.check(L.genie_profile_kernels(kc, kbuf, len(kbuf)), "profile_kernels")
            table.update({f"{kc}:{ln.split(chr(9))[0]}": int(float(ln.split("\t")[1])) for ln in kbuf.value.decode().splitlines() if "\t" in ln})
    finally:
        L.genie_profile_enable(0)
    return tr.grads.clone(), table


@pytest.mark.gpu
@pytest.mark.parametrize("recompute", [False, True], ids=["save", "recompute"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", STEP_CASES)
def test_p0_is_the_step_without_dropout(name, precision, recompute):
    """A trainer on mlp_drop = 0 (which calls the entry points of before) and one driven through genie_train_forward_drop /
    genie_train_backward_layer_drop with a genie_dropout of p = 0: torch.equal flat gradients and identical kernel tables, none of
    whose names is a dropout kernel; a step at p = 0.1 launches the dropout kernels (per layer: both sites in the forward, both in the backward, and site 0 again when
    the layer is recomputed)."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    cfg, sd, ids, labels = make_case(name)
    ids, labels = dev(ids), dev(labels)
    plain = make_trainer(cfg, sd, precision, recompute=recompute)
    via = make_trainer(cfg, sd, precision, recompute=recompute)
    calls = []
    via._dropout = lambda: calls.append(1) or lib.Dropout(p=0.0, call=len(calls), seed=11)
    g0, t0 = profiled(plain, ids, labels)
    g1, t1 = profiled(via, ids, labels)
    assert len(calls) == 1 and plain._dropout() is None
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(g0, g1)
    assert t0 == t1 and sum(t0.values()) > 0, {k: (t0.get(k), t1.get(k)) for k in set(t0) | set(t1) if t0.get(k) != t1.get(k)}
    assert not any("drop" in k for k in t0), t0
    dropped = make_trainer(cfg, sd, precision, 0.1, recompute=recompute)
    g2, t2 = profiled(dropped, ids, labels)
    assert not torch.equal(g2, g0)
    n_drop = sum(v for k, v in t2.items() if "drop" in k)
    assert n_drop == (5 if recompute else 4) * cfg.num_layers, t2


# ---------------------------------------------------------------------------------------------- recomputation
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_recompute_same_bits(name, precision):
    """recompute=True against False at p = 0.1: torch.equal on the whole flat gradient buffer.  The recomputation draws the site 0 mask
    again, and with Identity norms in the 16-bit precisions rebuilds each layer's operand in the bits the site 1 pass gave it; qk2k is
    the geometry of tests/test_hip_train_recompute.py::test_same_bits_with_fc2_on_a_throughput_kernel."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case(name)
    ids, labels = dev(ids), dev(labels)
    saved = make_trainer(cfg, sd, precision, 0.1, dropout_seed=SEED)
    rec = make_trainer(cfg, sd, precision, 0.1, dropout_seed=SEED, recompute=True)
    l0, _ = saved.forward_backward(ids, labels)
    l1, _ = rec.forward_backward(ids, labels)
    g0 = saved.grads
    diff = int((rec.grads.view(torch.int32) != g0.view(torch.int32)).sum())
    print(f"train_dropout/recompute/{precision}/{name}: loss {float(l0):.12f} / {float(l1):.12f}, {diff} of {g0.numel()} gradient words differ")
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(rec.grads, g0), f"{diff} gradient words differ between the modes"
    assert abs(float(l0) - float(l1)) <= 1e-12 * abs(float(l0))
    assert rec._acts.numel() < saved._acts.numel() and rec._ws.numel() == saved._ws.numel()


# ---------------------------------------------------------------------------------------------- determinism and resume
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_masks_follow_seed_and_counter(precision):
    """Same seed twice: equal bits.  dropout_seed 0 against 1: different gradients.  Two consecutive micro-batches of identical data:
    different gradients (the counter advanced), and the second equals the first of a trainer whose counter starts at 1."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("ln3")
    ids, labels = dev(ids), dev(labels)
    a, b, c = (make_trainer(cfg, sd, precision, 0.1, dropout_seed=s) for s in (0, 0, 1))
    for tr in (a, b, c):
        tr.forward_backward(ids, labels)
    assert torch.equal(a.grads, b.grads)
    assert not torch.equal(a.grads, c.grads)
    first = a.grads.clone()
    a.forward_backward(ids, labels)
    assert not torch.equal(a.grads, first)
    d = make_trainer(cfg, sd, precision, 0.1, dropout_seed=0)
    d._drop_call = 1
    d.forward_backward(ids, labels)
    assert torch.equal(d.grads, a.grads)


@pytest.mark.gpu
def test_resume_draws_the_masks_it_would_have_drawn():
    """Two train_steps are bit-equal to: one step, state_dict, a fresh trainer on the stepped weights with load_state_dict, one step
    (parameters and both moments).  A fresh trainer that does not load the state draws mask 0 again and ends elsewhere."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("ln3")
    batch = {"input_ids": dev(ids), "labels": dev(labels)}
    kw = dict(lr=1e-3, weight_decay=0.01, dropout_seed=5)
    two = make_trainer(cfg, sd, "exact", 0.1, **kw)
    two.train_step(batch)
    state = two.state_dict()
    assert state["dropout"] == {"seed": 5, "call": 1}
    sd1 = {k: v.detach().cpu().numpy().copy() for k, v in two.model.state_dict().items()}
    two.train_step(batch)
    outcomes = []
    for load in (True, False):
        tr = make_trainer(cfg, sd1, "exact", 0.1, **{**kw, "dropout_seed": 5 if not load else 99})
        if load:
            tr.load_state_dict(state)
            assert tr.dropout_seed == 5 and tr._drop_call == 1
        else:   # moments and step counter, but not the dropout state
            tr.load_state_dict({k: v for k, v in state.items() if k != "dropout"})
        tr.train_step(batch)
        outcomes.append(tr)
    resumed, fresh = outcomes
    assert torch.equal(resumed.params, two.params)
    assert torch.equal(resumed.exp_avg, two.exp_avg) and torch.equal(resumed.exp_avg_sq, two.exp_avg_sq)
    assert not torch.equal(fresh.params, two.params)


# ---------------------------------------------------------------------------------------------- stale memory
@pytest.mark.gpu
@pytest.mark.parametrize("recompute", [False, True], ids=["save", "recompute"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_stale_memory(name, recompute):
    """bf16, p = 0.1: every byte of the activation buffer and of the workspace is 0xFF (NaN in f32, bf16 and f16) before the step; the
    gradients are finite and the bits of a step on fresh buffers -- the two passes' scratch (the output slot, w.d1) is written before
    it is read."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case(name)
    ids, labels = dev(ids), dev(labels)
    B = ids.shape[0]
    clean = make_trainer(cfg, sd, "bf16", 0.1, dropout_seed=SEED, recompute=recompute)
    clean.forward_backward(ids, labels)
    stale = make_trainer(cfg, sd, "bf16", 0.1, dropout_seed=SEED, recompute=recompute)
    for buf in stale._buffers(B):
        buf.fill_(0xFF)
    stale.forward_backward(ids, labels)
    assert bool(torch.isfinite(stale.grads).all())
    assert torch.equal(stale.grads, clean.grads)


# ---------------------------------------------------------------------------------------------- inference
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_inference_ignores_mlp_drop(precision):
    """compute_logits of a model with mlp_drop = 0.3 is torch.equal to the same weights with 0, and so is the drop-in Mlp.forward."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, _ = make_case("ln3")
    x = dev(ids).view(-1, cfg.T, 4, 4)
    outs, mlps = [], []
    for p in (0.0, 0.3):
        c = cfg.shallow_copy()
        c.mlp_drop = p
        model = pkg("st_mask_git").STMaskGIT(c, precision=precision).load_numpy_state_dict(sd).to("cuda")
        outs.append(model.compute_logits(x))
        mlps.append(model.decoder.layers[0].mlp(torch.linspace(-2, 2, 8 * cfg.d_model, device="cuda").view(8, cfg.d_model)))
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    assert torch.equal(mlps[0], mlps[1])


# ---------------------------------------------------------------------------------------------- the CLI
@pytest.mark.gpu
def test_train_cli_mlp_drop(tmp_path):
    """tools/train.py --synthetic 8 --max_train_steps 2 --mlp_drop 0.1 in fresh child processes (a 2-layer d 64 config, an eval batch of
    1 for the one eval clip that 8 synthetic clips leave): the loss is finite, the same with the same seeds, another with
    --dropout_seed 1 and another with --mlp_drop 0; the saved config carries mlp_drop."""
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False,
                                    num_prompt_frames=2, use_mup=False)
    cfg.save_pretrained(tmp_path / "config.json")
    runs = {"a": ["--mlp_drop", "0.1"], "b": ["--mlp_drop", "0.1"], "seed1": ["--mlp_drop", "0.1", "--dropout_seed", "1"],
            "off": ["--mlp_drop", "0"]}
    procs = {}
    for tag, flags in runs.items():   # four independent child processes, side by side
        cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--max_train_steps", "2", "--seed", "1",
               "--genie_config", str(tmp_path / "config.json"), "--per_device_eval_batch_size", "1", "--precision", "exact",
               "--output_dir", str(tmp_path / tag)] + flags
        procs[tag] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = {}
    for tag, pr in procs.items():
        out, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, out[-2000:] + err[-2000:]
        step2 = [ln for ln in out.splitlines() if ln.startswith("step 2: train_loss")]
        assert len(step2) == 1, out[-2000:]
        lines[tag] = re.sub(r"\s+[0-9.]+ examples/s.*$", "", step2[0])
        assert np.isfinite(float(re.search(r"train_loss ([0-9.eE+-]+|nan|inf)", lines[tag]).group(1))), lines[tag]
    assert lines["a"] == lines["b"], lines
    assert lines["a"] != lines["off"] and lines["a"] != lines["seed1"], lines
    saved = pkg("config").GenieConfig.from_pretrained(str(tmp_path / "a" / "final_checkpt" / "config.json"))
    assert saved.mlp_drop == 0.1
