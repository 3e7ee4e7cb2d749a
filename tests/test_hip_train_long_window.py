"""Training at T = 32 and 64 frames: the tiled MFMA temporal attention backward (csrc/kernels_attn_bwd.hip
attn_temporal_bwd_tiled_kernel<head_dim, T / 16>) alone through genie_temporal_attention_backward, and whole trainer steps behind it.

The kernel alone is compared with a float64 NumPy restatement of the formulas above attn_temporal_bwd_kernel on the same f32 inputs;
the bar, per output block (dq, dk, dv), is KERNEL_FACTOR times the distance of the SAME restatement run in f32 from the float64
one, which the test computes itself.  T = 16 reaches the existing attn_temporal_bwd_mfma_kernel and is the calibration leg of the bar.

The step is compared with the float64 training oracle at the bars and seeds of tests/test_hip_train_geometry.py.
(H, d, T, S, B, qk_norm, use_mup, layers), tokens, precisions, what the case reaches:
  t32       (2, 64, 32, 16, 1, F, F, 2)    512   exact, f16x3   head_dim 32, two tile rows, LayerNorm blocks
  t64qk     (2, 128, 64, 16, 1, T, F, 1)   1024  exact, f16x3   head_dim 64, four tile rows, qk_ld = 2 d and the qk-norm backward behind it
  t64b3     (2, 64, 64, 16, 3, F, F, 1)    3072  exact, f16x3   head_dim 32 at T = 64, odd batch
  t32s64qk  (1, 64, 32, 64, 1, T, F, 2)    2048  exact, bf16    one head of 64, S = 64
t32s64qk is not run in f16x3: its number model (F16X3_TRAIN) is 6.1e-5 from the float64 oracle, above half the bar
(tests/test_train_long_window_cpu.py asserts the condition for the three that are).

The GPU tests need an MI355X (``-m gpu``); tests/test_train_long_window_cpu.py holds what runs anywhere.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, pkg, record_measure
from oracle import genie_train_oracle as TO

# the bars of tests/test_hip_train_geometry.py, restated
GRAD_TOL, LOSS_TOL, ACC_TOL = 1e-4, 1e-5, 1e-7

# id: (H, d, T, S, B, qk_norm, use_mup, layers)
CASES = {
    "t32": (2, 64, 32, 16, 1, False, False, 2),
    "t64qk": (2, 128, 64, 16, 1, True, False, 1),
    "t64b3": (2, 64, 64, 16, 3, False, False, 1),
    "t32s64qk": (1, 64, 32, 64, 1, True, False, 2),
}
TOKENS = {"t32": 512, "t64qk": 1024, "t64b3": 3072, "t32s64qk": 2048}
F16X3_CASES = ["t32", "t64qk", "t64b3"]

# bf16 bars of t32s64qk (median / max / Frobenius / loss / global norm): 3x the max over 100 seeds of
#   python tools/train_bf16_floor.py --seeds 100 t32s64qk
# which printed (p50 / p95 / max):
#   median  2.31e-04 / 3.49e-04 / 5.18e-04
#   max     3.29e-03 / 4.14e-03 / 5.23e-03
#   fro     2.42e-03 / 2.51e-03 / 2.58e-03
#   loss    9.95e-05 / 2.12e-04 / 2.89e-04
#   norm    2.77e-05 / 6.75e-05 / 8.73e-05
T32S64QK_BF16_BARS = (3 * 5.18e-4, 3 * 5.23e-3, 3 * 2.58e-3, 3 * 2.89e-4, 3 * 8.73e-5)

# kernel alone: bar = KERNEL_FACTOR x |f32 restatement - f64 restatement| (a different but fixed summation order)
KERNEL_FACTOR = 4.0


def make_case(name):
    """(cfg, sd, input_ids, labels) with the seeds of tests/test_hip_train_geometry.py; tools/train_bf16_floor.py reads this too."""
    H, d, T, S, B, qk_norm, use_mup, layers = CASES[name]
    cfg = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=T // 2, use_mup=use_mup)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=77 + H, law="conditioned")
    batch = TO.maskgit_collate(syn.make_clips(B, cfg, seed=900 + d), cfg, TO.NumpyDraws(5 + B))
    return cfg, sd, batch["input_ids"], batch["labels"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, sd, input_ids, labels, loss, acc, grads) with the float64 oracle's results: computed once, shared, never written to."""
    cfg, sd, ids, labels = make_case(name)
    loss, acc, grads = TO.forward_backward(ids, labels, sd, cfg, dtype=np.float64)
    return cfg, sd, ids, labels, loss, acc, grads


def rel_err(a, ref):
    """The largest error over the tensor's largest element."""
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


def dev(a):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_trainer(cfg, sd, precision, **kw):
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    return pkg("train").GenieTrainer(model, **kw)


# ---------------------------------------------------------------------------------------------- the kernel alone
def attn_bwd_restated(qkv, qk, dO, H, scale, dtype):
    """dq, dk, dv (B, T, S, d) each, by the formulas above attn_temporal_bwd_kernel, every operation in `dtype`."""
    B, T, S, d3 = qkv.shape
    d = d3 // 3
    Dh = d // H
    f = lambda a: a.astype(dtype).reshape(B, T, S, H, Dh)  # noqa: E731
    q, k, v, do = f(qk[..., :d]), f(qk[..., d:2 * d]), f(qkv[..., 2 * d:]), f(dO)
    sc = dtype(scale)
    s = np.einsum("bishc,bjshc->bshij", q, k) * sc
    s = np.where(np.tril(np.ones((T, T), bool)), s, dtype(-np.inf))
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    dp = np.einsum("bishc,bjshc->bshij", do, v)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    dq = np.einsum("bshij,bjshc->bishc", ds, k) * sc
    dk = np.einsum("bshij,bishc->bjshc", ds, q) * sc
    dv = np.einsum("bshij,bishc->bjshc", p, do)
    return tuple(a.reshape(B, T, S, d) for a in (dq, dk, dv))


def kernel_inputs(T, Dh, ld3, q_mul, seed=0, H=2, S=3, B=2):
    """Standard-normal qkv and q | k source (the q | k columns of qkv itself when ld3), q scaled by q_mul, dO scaled by 1e-3."""
    d = H * Dh
    g = np.random.default_rng(1000 * T + 10 * Dh + seed)
    qkv = g.standard_normal((B, T, S, 3 * d)).astype(np.float32)
    qkv[..., :d] *= np.float32(q_mul)
    if ld3:
        qk = qkv
    else:
        qk = g.standard_normal((B, T, S, 2 * d)).astype(np.float32)
        qk[..., :d] *= np.float32(q_mul)
    dO = (g.standard_normal((B, T, S, d)) * 1e-3).astype(np.float32)
    return qkv, qk, dO, H, float(Dh) ** -0.5


GUARD = 4096  # floats on either side of d_qkv


def run_kernel(qkv, qk, dO, H, scale):
    """d_qkv (B, T, S, 3d) from genie_temporal_attention_backward.  The output is pre-filled with NaN and sits between two guard
    regions: every element must have been written, and nothing outside."""
    torch = pytest.importorskip("torch")
    lib = pkg("_lib")
    L = lib.load()
    B, T, S, d3 = qkv.shape
    d = d3 // 3
    t_qkv, t_do = dev(qkv), dev(dO)
    t_qk = t_qkv if qk is qkv else dev(qk)
    n = B * T * S * d3
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:GUARD] = -7.0
    buf[GUARD + n:] = -7.0
    lib.check(L.genie_temporal_attention_backward(t_qkv.data_ptr(), t_qk.data_ptr(), qk.shape[-1], t_do.data_ptr(),
                                                  buf.data_ptr() + 4 * GUARD, B, T, S, d, H, d // H, scale,
                                                  torch.cuda.current_stream().cuda_stream), "genie_temporal_attention_backward")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == -7.0).all() and (out[GUARD + n:] == -7.0).all(), "the kernel wrote outside d_qkv"
    out = out[GUARD:GUARD + n].reshape(B, T, S, d3)
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} elements of d_qkv were not written"
    return out


def split3(a):
    d = a.shape[-1] // 3
    return a[..., :d], a[..., d:2 * d], a[..., 2 * d:]


@pytest.mark.gpu
@pytest.mark.parametrize("q_mul", [1.0, 4.0])
@pytest.mark.parametrize("ld3", [True, False], ids=["ld3d", "ld2d"])
@pytest.mark.parametrize("Dh", [32, 64])
@pytest.mark.parametrize("T", [16, 32, 64])
def test_kernel_vs_float64_restatement(T, Dh, ld3, q_mul):
    """dq, dk, dv of the kernel within KERNEL_FACTOR = 4 times the f32 restatement's own distance from the float64 one (largest
    error over the block's largest element), with flat (q x 1) and sharp (q x 4) softmax rows; the output fully written, nothing
    outside it, and a second call gives the same bits.  T = 16 is the calibration leg: the existing attn_temporal_bwd_mfma_kernel.

    Measured on an MI355X over the 8 cases x 3 blocks of one T (the f32 restatement itself is 1.2e-7 .. 1.5e-6 from the float64 one):
    kernel error 1.0e-7 .. 8.0e-7 at T = 16, 1.5e-7 .. 6.4e-7 at T = 32, 1.5e-7 .. 6.5e-7 at T = 64; largest ratio to the f32
    restatement's distance 2.16 (T = 16, the existing kernel), 1.56 (T = 32), 1.46 (T = 64).
    The tiled kernel sums each score product in two accumulator chains: with sharp rows (|s| ~ 16) the rounding of one
    head_dim / 4-long f32 chain in the scores is the largest error of the backward, and a single chain exceeds this bar (5.49 at
    T = 32, head_dim 64, qk_ld = 2 d, q x 4; profiles/train_long_window.txt)."""
    qkv, qk, dO, H, scale = kernel_inputs(T, Dh, ld3, q_mul)
    ref = attn_bwd_restated(qkv, qk, dO, H, scale, np.float64)
    f32 = attn_bwd_restated(qkv, qk, dO, H, scale, np.float32)
    out = run_kernel(qkv, qk, dO, H, scale)
    again = run_kernel(qkv, qk, dO, H, scale)
    assert np.array_equal(out, again)
    bad = {}
    for name, got, r64, r32 in zip(("dq", "dk", "dv"), split3(out), ref, f32):
        err, floor = rel_err(got, r64), rel_err(r32, r64)
        tag = f"train_long_window/kernel/T{T}_Dh{Dh}_{'ld3d' if ld3 else 'ld2d'}_q{int(q_mul)}/{name}"
        record_measure(tag, err)
        record_measure(tag + "_f32_restatement", floor)
        print(f"{tag}: kernel {err:.3e}, f32 restatement {floor:.3e}, ratio {err / floor:.2f}")
        if not err <= KERNEL_FACTOR * floor:
            bad[name] = (err, floor)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("Dh", [32, 64])
@pytest.mark.parametrize("T", [32, 64])
def test_kernel_causality(T, Dh):
    """dq of the frames < f does not change by a bit when q, k, v and dO of the frames >= f do (f = 16: a tile edge; 17: inside the
    diagonal tile; T - 1), and dk, dv of the last frame depend on the last query row alone: they keep their bits when q and dO of
    every earlier frame change."""
    qkv, qk, dO, H, scale = kernel_inputs(T, Dh, False, 1.0)
    d = H * Dh
    base = run_kernel(qkv, qk, dO, H, scale)
    g = np.random.default_rng(5)
    for f in (16, 17, T - 1):
        qkv2, qk2, dO2 = qkv.copy(), qk.copy(), dO.copy()
        qkv2[:, f:] = g.standard_normal(qkv2[:, f:].shape).astype(np.float32)
        qk2[:, f:] = g.standard_normal(qk2[:, f:].shape).astype(np.float32)
        dO2[:, f:] = (g.standard_normal(dO2[:, f:].shape) * 1e-3).astype(np.float32)
        out = run_kernel(qkv2, qk2, dO2, H, scale)
        assert np.array_equal(out[:, :f, :, :d], base[:, :f, :, :d]), f
        assert not np.array_equal(out[:, f:, :, :d], base[:, f:, :, :d])
    qk2, dO2 = qk.copy(), dO.copy()
    qk2[:, :T - 1, :, :d] = g.standard_normal(qk2[:, :T - 1, :, :d].shape).astype(np.float32)
    dO2[:, :T - 1] = (g.standard_normal(dO2[:, :T - 1].shape) * 1e-3).astype(np.float32)
    out = run_kernel(qkv, qk2, dO2, H, scale)
    assert np.array_equal(out[:, T - 1, :, d:], base[:, T - 1, :, d:])
    assert not np.array_equal(out[:, :T - 1, :, d:], base[:, :T - 1, :, d:])


# ---------------------------------------------------------------------------------------------- the step
def step_vs_oracle(name, precision):
    cfg, sd, ids, labels, loss_o, acc_o, g_o = case(name)
    tr = make_trainer(cfg, sd, precision)
    loss, acc = tr.forward_backward(dev(ids), dev(labels))
    worst = {k: rel_err(g.cpu().numpy(), g_o[k]) for k, g in tr.gradients().items()}
    assert set(worst) == set(g_o)
    top = max(worst.items(), key=lambda kv: kv[1])
    record_measure(f"train_long_window/{precision}/{name}", top[1])
    print(f"train_long_window/{precision}/{name}: loss {float(loss):.8f} (oracle {loss_o:.8f}), acc {float(acc):.6f} ({acc_o:.6f}), "
          f"worst tensor {top[0]} {top[1]:.3e}")
    assert abs(float(loss) - loss_o) < LOSS_TOL * abs(loss_o)
    assert abs(float(acc) - acc_o) < ACC_TOL
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_step_exact(name):
    """One exact trainer step against the float64 oracle.  Measured on an MI355X, worst tensor per case: t32 7.5e-7, t64qk 6.8e-7,
    t64b3 7.4e-7, t32s64qk 6.4e-7 (pos_embed_TSC each time)."""
    step_vs_oracle(name, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("name", F16X3_CASES)
def test_step_f16x3(name):
    """The same bar in f16x3 (generic temporal forward + launch_cast16 in front of the 16-bit projection).  Measured on an MI355X,
    worst tensor per case: t32 3.7e-7, t64qk 3.9e-7, t64b3 4.8e-7."""
    step_vs_oracle(name, "f16x3")


@pytest.mark.gpu
def test_step_bf16_vs_bf16_oracle():
    """t32s64qk in bf16 against BF16_TRAIN at the five bars of tests/test_hip_train_bf16.py (its check_vs_oracle), computed by that
    file's rule: see T32S64QK_BF16_BARS.  Measured on an MI355X, median / max / Frobenius (loss, norm): 1.9e-4 / 3.0e-3 / 2.4e-3
    (7.5e-5, 2.0e-5) -- inside the floor's spread."""
    import test_hip_train_bf16 as B16
    cfg, sd, ids, labels = make_case("t32s64qk")
    B16.check_vs_oracle("t32s64qk", cfg, sd, ids, labels, T32S64QK_BF16_BARS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_step_is_bit_reproducible(name):
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case(name)
    tr = make_trainer(cfg, sd, "exact")
    ids, labels = dev(ids), dev(labels)
    tr.forward_backward(ids, labels)
    g1 = tr.grads.clone()
    tr.forward_backward(ids, labels)
    assert torch.equal(g1, tr.grads)


@pytest.mark.gpu
def test_accumulation_t32():
    """accumulate=True adds (tests/test_hip_train.py::test_bit_reproducible_and_accumulation), at t32 in exact."""
    cfg, sd, a_ids, a_lab = make_case("t32")
    b = TO.maskgit_collate(pkg("synthetic").make_clips(1, cfg, seed=5), cfg, TO.NumpyDraws(6))
    tr = make_trainer(cfg, sd, "exact")
    a_ids, a_lab, b_ids, b_lab = dev(a_ids), dev(a_lab), dev(b["input_ids"]), dev(b["labels"])
    tr.forward_backward(a_ids, a_lab)
    g1 = tr.grads.clone()
    tr.forward_backward(b_ids, b_lab)
    g2 = tr.grads.clone()
    tr.forward_backward(a_ids, a_lab)
    tr.forward_backward(b_ids, b_lab, accumulate=True)
    assert float((tr.grads - (g1 + g2)).abs().max()) <= 1e-6 * float(g1.abs().max())


@pytest.mark.gpu
def test_one_clipped_adamw_step_t32():
    """One train_step (clip_grad_norm_ at 1.0, AdamW with decay) at t32 in exact against oracle adamw_step / clip_coef on the float64
    oracle's gradients, at the bars of tests/test_hip_train.py::test_two_optimizer_steps_vs_reference: loss and gradient norm 2e-5
    relative, parameter error mean 2e-6 and max 2e-3 per tensor (Adam's first update is lr * sign(g) = 1e-3 wherever it applies)."""
    cfg, sd, ids, labels, loss_o, _, g_o = case("t32")
    lr, wd, clip = 1e-3, 0.01, 1.0
    tr = make_trainer(cfg, sd, "exact", lr=lr, weight_decay=wd, max_grad_norm=clip)
    out = tr.train_step({"input_ids": dev(ids), "labels": dev(labels)})
    gn_o = TO.grad_norm(g_o)
    assert gn_o > clip                                  # the clip is live
    assert abs(float(out["loss"]) - loss_o) < 2e-5 * abs(loss_o)
    assert abs(float(out["grad_norm"]) - gn_o) < 2e-5 * gn_o
    params = {k: np.array(sd[k], dtype=np.float32) for k in g_o}
    TO.adamw_step(params, g_o, {}, 1, lr, weight_decay=wd, grad_scale=TO.clip_coef(gn_o, clip))
    state = tr.model.state_dict()
    for k, p in params.items():
        err = np.abs(state[k].cpu().numpy().astype(np.float64) - p)
        assert err.mean() < 2e-6, (k, err.mean())
        assert err.max() < 2e-3, (k, err.max())
        assert np.abs(p - sd[k]).max() > 0              # the step moved the tensor


@pytest.mark.gpu
def test_train_cli_at_window_32(tmp_path):
    """tools/train.py --synthetic 8 --window_size 32 --max_train_steps 2 in a fresh child process (the default c35 shape in bf16 at
    32 frames; 8 synthetic clips leave one eval window, hence the eval batch of 1)."""
    cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--window_size", "32", "--max_train_steps",
           "2", "--per_device_eval_batch_size", "1", "--output_dir", str(tmp_path / "out")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "step 2: train_loss" in res.stdout, res.stdout[-2000:]
