"""The training step at the geometries between the S = 16 and S = 256 fixtures of test_hip_train.py: one trainer step per case
(GenieTrainer.forward_backward) against the float64 restatement of the step (oracle.genie_train_oracle.forward_backward with
dtype=np.float64; the f32 restatement sits 6e-7 .. 1.4e-6 from it on these cases).  The bars are the file-level bars of
tests/test_hip_train.py (loss 1e-5 relative, accuracy 1e-7, every gradient tensor within GRAD_TOL = 1e-4 of its largest
element), restated here, in exact AND in f16x3 ("f32-class gradients").

What each case reaches (csrc/train_api.hip, csrc/kernels_train.hip, csrc/kernels_attn_bwd.hip); (H, d, T, S, B, qk_norm, use_mup, layers):
  s144       (1, 64, 2, 144, 1, F, F, 2)   Dh 64; spatial backward through materialised scores (every S != 256): five batched
                                           gemm_f32_gen_kernel launches (P and dP row-major x row-major, dV and dK k-major x
                                           k-major, dQ row-major x k-major) whose 128 x 128 tiles cover 128 + 16 rows, columns and
                                           k-major float4 groups, softmax rows of 3 trips of 64 lanes; M = 288
  s144qk     (2, 128, 4, 144, 1, T, F, 2)  the same from the normalised q / k copies (qk_ld = 2 d); M = 576 = 9 * 64: in f16x3 every
                                           wgrad16 has ns = 1 (its slab loop needs Mtok % 128 == 0), at widths 128 .. 1024
  s400qk     (2, 64, 2, 400, 1, T, F, 1)   Dh 32; 3 x 128 + 16: four tiles per side, softmax rows of 7 trips
  s576       (2, 64, 2, 576, 1, F, F, 1)   the largest square frame head_dim 32 admits (S * head_dim * 8 <= 160 KiB); 4 x 128 + 64.
                                           Without muP: with it the readout saturates (loss 32) and the gradients say nothing
  t8s64qk    (2, 64, 8, 64, 1, T, F, 2)    T = 8: attn_temporal_bwd_kernel (16 threads per group, 8 active) behind the short-window
                                           MFMA temporal forward (16-bit epilogue in f16x3); S = 64: half a tile, at the exact bar
  t8b3       (2, 128, 8, 16, 3, F, F, 2)   T = 8, odd batch, M = 384
  t8s256     (2, 128, 8, 256, 1, F, F, 1)  T = 8 with the S = 256 kernels: MFMA spatial forward, fused spatial backward, short-window
                                           temporal forward, generic temporal backward
  m32        (2, 64, 2, 16, 1, F, F, 2)    M = 32, below the 64-row chunks of the column sums / slab reduction
  m96        (2, 64, 2, 16, 3, F, F, 2)    M = 96

f16x3 runs a case only where (a) the 16-bit step admits it -- train_check needs T * S % 64 == 0, which rules out s144 (288), s400qk
(800), m32 and m96 (32): test_16_bit_step_refuses_token_counts_off_64 checks that they are refused up front -- and (b) the number
model itself (oracle F16X3_TRAIN: where the split-f16 step rounds) is at most 5e-5 -- half the bar -- from the float64 oracle, so
that the number format alone cannot fail the test; test_f16x3_number_model_leaves_half_the_bar asserts that on the CPU.  Distances:
s144qk 4.1e-5, s576 1.2e-5, t8s64qk 1.6e-5, t8b3 1.0e-5 (and, for the record, s144 9.1e-6 and s400qk 1.3e-5, which (a) excludes).
t8s256 is at 6.9e-5 with the seeds of this file, and at 8.2e-5 .. 1.2e-4 with eight other weight (80 .. 83) or clip (1029 .. 1032)
seeds: no seed tried meets the condition, the 2048-token contractions of that geometry sit above it.  So t8s256 is left to exact here
and to bf16 (tests/test_hip_train_bf16.py, case d128t8s256); it is NOT run in f16x3.

The GPU tests need an MI355X (``-m gpu``); the unmarked ones run anywhere.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import pkg, record_measure
from oracle import genie_train_oracle as TO
# the file-level bars of tests/test_hip_train.py (GRAD_TOL there; loss and accuracy as in its gradients_vs_oracle), restated
GRAD_TOL, LOSS_TOL, ACC_TOL = 1e-4, 1e-5, 1e-7
F16X3_MODEL_TOL = 0.5 * GRAD_TOL

# id: (H, d, T, S, B, qk_norm, use_mup, layers)
CASES = {
    "s144": (1, 64, 2, 144, 1, False, False, 2),
    "s144qk": (2, 128, 4, 144, 1, True, False, 2),
    "s400qk": (2, 64, 2, 400, 1, True, False, 1),
    "s576": (2, 64, 2, 576, 1, False, False, 1),
    "t8s64qk": (2, 64, 8, 64, 1, True, False, 2),
    "t8b3": (2, 128, 8, 16, 3, False, False, 2),
    "t8s256": (2, 128, 8, 256, 1, False, False, 1),
    "m32": (2, 64, 2, 16, 1, False, False, 2),
    "m96": (2, 64, 2, 16, 3, False, False, 2),
}
OFF_64 = ["s144", "s400qk", "m32", "m96"]               # T * S % 64 != 0: exact only, the 16-bit step refuses them
F16X3_CASES = ["s144qk", "s576", "t8s64qk", "t8b3"]     # the rest, without t8s256 (see above)
TOKENS = {"s144": 288, "s144qk": 576, "s400qk": 800, "s576": 1152, "t8s64qk": 512, "t8b3": 384, "t8s256": 2048, "m32": 32,
          "m96": 96}

FUSED, GEN = "attn_spatial_bwd_fused_kernel", "gemm_f32_gen_kernel"


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, sd, input_ids, labels, loss, acc, grads) with the float64 oracle's results: computed once, shared, never written to."""
    H, d, T, S, B, qk_norm, use_mup, layers = CASES[name]
    cfg = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=max(1, T // 2), use_mup=use_mup)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=77 + H, law="conditioned")
    ids = syn.make_clips(B, cfg, seed=900 + d)
    batch = TO.maskgit_collate(ids, cfg, TO.NumpyDraws(5 + B))
    loss, acc, grads = TO.forward_backward(batch["input_ids"], batch["labels"], sd, cfg, dtype=np.float64)
    return cfg, sd, batch["input_ids"], batch["labels"], loss, acc, grads


def rel_err(a, ref):
    """test_hip_train.py::rel_err: the largest error over the tensor's largest element."""
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


def dev(a):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_trainer(cfg, sd, precision):
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    return pkg("train").GenieTrainer(model)


# ---------------------------------------------------------------------------------------------- anywhere (no GPU)
@pytest.mark.parametrize("name", list(CASES))
def test_cases_have_the_geometry_they_claim(name):
    cfg, _, ids, labels, loss, _, grads = case(name)
    H, d, T, S, B, *_ = CASES[name]
    assert ids.shape == labels.shape == (B, T * S) and B * T * S == TOKENS[name]
    assert cfg.head_dim == d // H and cfg.head_dim in (32, 64)
    assert S % 16 == 0 and S * cfg.head_dim * 8 <= 160 * 1024      # what check_cfg / train_check admit
    masked = int((ids.reshape(B, T, S)[:, 1:] == cfg.image_vocab_size).sum())
    assert masked >= 8, masked                                      # the loss counts tokens; 8 (m32) .. 1293 (t8s256)
    assert np.isfinite(loss) and 13.0 < loss < 16.0                 # an unsaturated readout (2 ln 512 = 12.5 for a uniform one)
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in grads.values())
    assert ((T * S) % 64 != 0) == (name in OFF_64)                  # the 16-bit step's own requirement


@pytest.mark.parametrize("name", F16X3_CASES)
def test_f16x3_number_model_leaves_half_the_bar(name):
    """The condition under which a case runs in f16x3: F16X3_TRAIN (f32 arithmetic, split-f16 operands at the rounding points of the
    16-bit step) is within GRAD_TOL / 2 of the float64 oracle on every gradient tensor, and the loss within a tenth of its bar."""
    cfg, sd, ids, labels, loss, _, grads = case(name)
    loss_m, _, g_m = TO.forward_backward(ids, labels, sd, cfg, nm=TO.F16X3_TRAIN)
    worst = {k: rel_err(g_m[k], grads[k]) for k in grads}
    assert max(worst.values()) <= F16X3_MODEL_TOL, max(worst.items(), key=lambda kv: kv[1])
    assert abs(loss_m - loss) < 0.1 * LOSS_TOL * abs(loss)


# ---------------------------------------------------------------------------------------------- MI355X
def step_vs_oracle(name, precision):
    cfg, sd, ids, labels, loss_o, acc_o, g_o = case(name)
    tr = make_trainer(cfg, sd, precision)
    loss, acc = tr.forward_backward(dev(ids), dev(labels))
    worst = {k: rel_err(g.cpu().numpy(), g_o[k]) for k, g in tr.gradients().items()}
    assert set(worst) == set(g_o)
    top = max(worst.items(), key=lambda kv: kv[1])
    record_measure(f"train_geometry/{precision}/{name}", top[1])
    print(f"train_geometry/{precision}/{name}: loss {float(loss):.8f} (oracle {loss_o:.8f}), acc {float(acc):.6f} ({acc_o:.6f}), "
          f"worst tensor {top[0]} {top[1]:.3e}")
    assert abs(float(loss) - loss_o) < LOSS_TOL * abs(loss_o)
    assert abs(float(acc) - acc_o) < ACC_TOL
    bad = {k: v for k, v in worst.items() if v >= GRAD_TOL}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_geometry_exact(name):
    """Measured on an MI355X, worst tensor per case: s144 7.7e-7, s144qk 1.1e-6, s400qk 6.6e-7, s576 7.8e-7, t8s64qk 1.6e-6,
    t8b3 1.5e-6, t8s256 9.0e-7, m32 1.0e-6, m96 7.6e-7 (the f32 restatement is 6e-7 .. 1.4e-6 from the float64 one)."""
    step_vs_oracle(name, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("name", F16X3_CASES)
def test_geometry_f16x3(name):
    """The same bar as exact.  Measured on an MI355X, worst tensor per case: s144qk 6.5e-7, s576 5.7e-7, t8s64qk 6.1e-7, t8b3 5.7e-7.

    s144qk found a defect: before the gradient operands were scaled ahead of their split (csrc/kernels.hpp GRAD_SCALE16) these
    read s144qk 1.10e-4 (token_embed.factored_embeds.1.weight: over the bar), s576 4.3e-5, t8s64qk 3.0e-5, t8b3 1.7e-5.  A
    gradient below 2^-14 had its f16 hi half flushed, lived in lo alone, and the three-product GEMM (no lo.lo term) then
    multiplied it with the hi half of the weight or activation only; restating exactly that on the CPU (F16X3_TRAIN with the
    three products) gave 1.09e-4 on the same tensor, and 1.3e-6 with the operands scaled by 2^12.
    t8s256, not asserted here (see the module docstring): 2.2e-4 before (decoder.layers.0.norm1.bias), 3.6e-7 after."""
    step_vs_oracle(name, "f16x3")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
@pytest.mark.parametrize("name", OFF_64)
def test_16_bit_step_refuses_token_counts_off_64(name, precision):
    """T * S % 64 != 0: the 16-bit step (64 x 64 transposition tiles, K-steps of 64 tokens in the weight gradients) refuses in
    train_check, before anything is launched, with a message that names T*S."""
    cfg, sd, ids, labels, *_ = case(name)
    with pytest.raises(pkg("_lib").GenieHipError, match=r"T\*S"):
        make_trainer(cfg, sd, precision).forward_backward(dev(ids), dev(labels))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_spatial_backward_dispatch_exact(name):
    """Which spatial attention backward one exact step launched.  In exact every Linear product is a gemm_f32_gen_kernel launch too, so
    the name alone says nothing and the COUNT is asserted: per step 6 L + 1 forward Linears, the readout's wgrad + dgrad, and 6 wgrads
    + 6 dgrads per layer = 18 L + 3 (launch_wgrad_f32 is one launch whatever its split); the materialised spatial backward
    (spatial_attn_bwd: P, dV, dP, dQ, dK -- five batched launches) adds 5 per layer, the fused one none.
    Not launch-checked: the temporal backward -- its ProfScope carries no kernel name.  By launch_attn_temporal_bwd, T == 16 with
    head_dim 32 / 64 takes attn_temporal_bwd_mfma_kernel and every other T (here 2, 4, 8) attn_temporal_bwd_kernel<head_dim>; the
    training forward at T = 8 takes launch_attn_temporal_f32_mfma (temporal_attn_fwd tries it first, it covers T = 8 and 16)."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels, *_ = case(name)
    tr = make_trainer(cfg, sd, "exact")
    lib = pkg("_lib")
    L = lib.load()
    launched = {}
    lib.check(L.genie_profile_enable((1 << lib.KC_GEMM) | (1 << lib.KC_ATTN_SPATIAL)), "profile_enable")
    L.genie_profile_reset()
    try:
        tr.forward_backward(dev(ids), dev(labels))
        torch.cuda.synchronize()
        for kc in (lib.KC_GEMM, lib.KC_ATTN_SPATIAL):
            kbuf = ctypes.create_string_buffer(16384)
            lib.check(L.genie_profile_kernels(kc, kbuf, len(kbuf)), "profile_kernels")
            launched.update({ln.split("\t")[0]: int(float(ln.split("\t")[1]))
                             for ln in kbuf.value.decode().splitlines() if "\t" in ln})
    finally:
        L.genie_profile_enable(0)
    linears = 18 * cfg.num_layers + 3
    if cfg.S != 256:
        assert launched.get(GEN, 0) == linears + 5 * cfg.num_layers, launched
        assert not launched.get(FUSED, 0), launched
    else:
        assert launched.get(FUSED, 0) == cfg.num_layers, launched
        assert launched.get(GEN, 0) == linears, launched      # no gemm_f32_gen_kernel launch for attention


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "f16x3", "bf16"])
@pytest.mark.parametrize("qk_norm", [False, True])
def test_head_dim_16_training_is_refused_up_front(qk_norm, precision):
    """head_dim = 16 has no temporal attention backward and no qk-norm backward kernel: train_check refuses the step in
    genie_train_forward, with a message that names head_dim, before anything is launched -- and inference is unaffected."""
    torch = pytest.importorskip("torch")
    cfg = pkg("config").GenieConfig(num_layers=1, num_heads=4, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=2)
    assert cfg.head_dim == 16
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=3, law="conditioned")
    clips = syn.make_clips(1, cfg, seed=4)
    batch = TO.maskgit_collate(clips, cfg, TO.NumpyDraws(5))
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    ids, labels = dev(batch["input_ids"]), dev(batch["labels"])
    with pytest.raises(pkg("_lib").GenieHipError, match="head_dim"):
        pkg("train").GenieTrainer(model).forward_backward(ids, labels)
    torch.cuda.synchronize()
    if precision == "exact":
        from oracle import genie_oracle
        loss_o, _, _ = genie_oracle.forward_loss_acc(batch["input_ids"], batch["labels"], sd, cfg)
        assert abs(float(model(ids, labels).loss) - loss_o) < 1e-4
