"""Pin the training-step oracle (oracle/genie_train_oracle.py) against the reference's own collator outputs,
autograd gradients, clip_grad_norm_ and AdamW results (tests/golden/train_*.npz, made by
tools/make_goldens_train.py from the imported reference).  CPU only."""
import numpy as np
import pytest

from conftest import pkg
from oracle import genie_train_oracle as TO

FULL = ["train_tiny_ln", "train_tiny_qknorm"]
GRAD_TOL = 2e-5  # max |g - g_ref| / max |g_ref| per tensor, fp32 reference autograd vs fp32 oracle


def replay(z, step):
    kinds = z[f"s{step}_draw_kinds"]
    return TO.ReplayDraws(kinds, [z[f"s{step}_draw_{i}"] for i in range(len(kinds))])


@pytest.mark.parametrize("name", FULL + ["train_shape_dh64"])
@pytest.mark.parametrize("step", [0, 1])
def test_collator_bit_exact(golden, name, step):
    z, cfg, _ = golden(name)
    batch = TO.maskgit_collate(z[f"s{step}_ids"], cfg, replay(z, step))
    assert np.array_equal(batch["input_ids"], z[f"s{step}_input_ids"])
    assert np.array_equal(batch["labels"], z[f"s{step}_labels"])
    assert (batch["input_ids"] == cfg.image_vocab_size).any()


def test_collator_covers_both_branches(golden):
    z, _, _ = golden("train_tiny_ln")
    assert {str(z["s0_branch"]), str(z["s1_branch"])} == {"mlm", "nonmlm"}


@pytest.mark.parametrize("name", FULL)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_loss_and_every_gradient(golden, name, dtype):
    z, cfg, sd = golden(name)
    loss, acc, grads = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg, dtype=dtype)
    assert abs(loss - float(z["s0_loss"])) < 1e-5 * abs(float(z["s0_loss"]))
    assert abs(acc - float(z["s0_acc"])) < 1e-7
    assert set(grads) == set(sd)
    for k in sd:
        ref = z[f"s0_grad/{k}"]
        assert grads[k].shape == ref.shape, k
        assert np.abs(grads[k] - ref).max() <= GRAD_TOL * np.abs(ref).max() + 1e-12, k
    assert abs(TO.grad_norm(grads) - float(z["s0_grad_norm"])) < 1e-5 * float(z["s0_grad_norm"])


def test_gradient_samples_real_geometry(golden):
    z, cfg, sd = golden("train_shape_dh64")
    loss, _, grads = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg)
    assert abs(loss - float(z["s0_loss"])) < 1e-5 * abs(float(z["s0_loss"]))
    for k in sd:
        g = grads[k]
        n_ref = float(z[f"s0_gradnorm/{k}"])
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - n_ref) <= 1e-4 * n_ref + 1e-12, k
        samp = g.reshape(-1)[:: max(1, g.size // 64)][:64]
        assert np.abs(samp - z[f"s0_gradsample/{k}"]).max() <= 1e-4 * np.abs(g).max() + 1e-12, k


@pytest.mark.parametrize("name", FULL)
def test_two_optimizer_steps(golden, name):
    """collate -> forward/backward -> clip -> AdamW (decay grouping of train.py:426-437) -> scheduler, twice."""
    z, cfg, sd = golden(name)
    params = {k: v.astype(np.float32).copy() for k, v in sd.items()}
    state = {}
    for step in range(2):
        batch = TO.maskgit_collate(z[f"s{step}_ids"], cfg, replay(z, step))
        loss, _, grads = TO.forward_backward(batch["input_ids"], batch["labels"], params, cfg)
        assert abs(loss - float(z[f"s{step}_loss"])) < 2e-5 * abs(float(z[f"s{step}_loss"]))
        tn = TO.grad_norm(grads)
        assert abs(tn - float(z[f"s{step}_grad_norm"])) < 1e-5 * tn
        lr = float(z["lr"]) * TO.lr_factor_custom_cosine(step, 1, 4)
        assert abs(lr - float(z[f"s{step}_lr"])) < 1e-12
        TO.adamw_step(params, grads, state, step + 1, lr, float(z["beta1"]), float(z["beta2"]), float(z["eps"]),
                      float(z["weight_decay"]), grad_scale=TO.clip_coef(tn, float(z["max_grad_norm"])))
    for k in sd:
        # two steps of lr ~1e-3 with |m/sqrt(v)| ~ 1: the update is ~2e-3, parity to 1 % of that
        assert np.abs(params[k] - z[f"final_param/{k}"]).max() < 2.5e-5, k


def test_decay_grouping_quirk():
    # train.py:427: the "layer_norm.weight" pattern matches no GENIE parameter, so norm weights decay; biases do not
    assert TO.decays("decoder.layers.0.norm1.weight")
    assert TO.decays("pos_embed_TSC") and TO.decays("decoder.layers.3.mlp.fc1.weight")
    assert not TO.decays("decoder.layers.0.norm1.bias") and not TO.decays("out_x_proj.bias")


def test_lr_factors():
    assert TO.lr_factor_custom_cosine(0, 2, 10) == 0.5 and TO.lr_factor_custom_cosine(1, 2, 10) == 1.0
    assert abs(TO.lr_factor_custom_cosine(10, 2, 10) - 0.1) < 1e-12
    assert TO.lr_factor_linear(0, 0, 10) == 1.0 and TO.lr_factor_linear(5, 0, 10) == 0.5


# ---- number models of the 16-bit training step (TO.BF16_TRAIN, TO.F16X3_TRAIN)
def fro(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / ((ref ** 2).sum() + 1e-60)))


@pytest.mark.parametrize("name", FULL + ["train_shape_dh64"])
def test_contract_with_every_point_off_is_the_f32_oracle(golden, name):
    """The nm= code path with no rounding point switched on computes exactly what the default (f32) path computes, bit for bit:
    the rounding points are the only difference between the two paths.  Two paths of the same module, so this does not pin the
    default path itself; test_loss_and_every_gradient / test_gradient_samples_real_geometry pin that against the reference's
    autograd (to f32 tolerance: a bit-level fingerprint would depend on the BLAS build).  Holds with muP off, as in these
    fixtures: with muP on, the 16-bit path scales the readout's f32 accumulator ((x @ Wo^T) * readout_mult, as the kernel's
    alpha does) where the default path scales x first ((x * readout_mult) @ Wo^T), which rounds differently."""
    z, cfg, sd = golden(name)
    loss, acc, g = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg)
    off = TO.TrainNumerics("none", TO.go.round_bf16, ())
    loss2, acc2, g2 = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg, nm=off)
    assert (loss, acc) == (loss2, acc2)
    assert all(np.array_equal(g[k], g2[k]) for k in g)


@pytest.mark.parametrize("name", FULL)
def test_bf16_contract_vs_reference_autograd(golden, name):
    """BF16_TRAIN models what bf16 operands cost, not a different computation: against the reference's f32 autograd it stays
    within the bars the bf16 trainer is held to there (test_hip_train.py::test_bf16_gradients_close_to_reference)."""
    z, cfg, sd = golden(name)
    loss, _, g = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg, nm=TO.BF16_TRAIN)
    assert abs(loss - float(z["s0_loss"])) < 1e-2
    bad = {k: fro(g[k], z[f"s0_grad/{k}"]) for k in sd}
    assert max(bad.values()) > 1e-3  # it does round (measured 6e-3 .. 9e-3 worst tensor)
    bad = {k: v for k, v in bad.items() if v > 3e-2}
    assert not bad, bad
    assert abs(TO.grad_norm(g) - float(z["s0_grad_norm"])) < 1e-2 * float(z["s0_grad_norm"])


def test_bf16_contract_real_geometry(golden):
    """T 16, S 256, Dh 64 (the bf16 spatial backward rounding points are live): test_hip_train.py::test_real_geometry_bf16's bars."""
    z, cfg, sd = golden("train_shape_dh64")
    loss, _, g = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg, nm=TO.BF16_TRAIN)
    assert abs(loss - float(z["s0_loss"])) < 1e-2
    for k in sd:
        n_ref = float(z[f"s0_gradnorm/{k}"])
        assert abs(np.sqrt((g[k].astype(np.float64) ** 2).sum()) - n_ref) <= 2e-2 * n_ref + 1e-12, k
        samp = g[k].reshape(-1)[:: max(1, g[k].size // 64)][:64]
        assert np.abs(samp - z[f"s0_gradsample/{k}"]).max() <= 3e-2 * np.abs(g[k]).max() + 1e-12, k


@pytest.mark.parametrize("name", FULL)
def test_f16x3_contract_is_f32_class(golden, name):
    """Split-f16 operands (22 bits) at every Linear point: indistinguishable from the f32 oracle at its own bar against the
    reference autograd (measured 8.2e-6 / 8.6e-6 against GRAD_TOL 2e-5)."""
    z, cfg, sd = golden(name)
    loss, _, g = TO.forward_backward(z["s0_input_ids"], z["s0_labels"], sd, cfg, nm=TO.F16X3_TRAIN)
    assert abs(loss - float(z["s0_loss"])) < 1e-5 * abs(float(z["s0_loss"]))
    for k in sd:
        ref = z[f"s0_grad/{k}"]
        assert np.abs(g[k] - ref).max() <= GRAD_TOL * np.abs(ref).max() + 1e-12, k


@pytest.fixture(scope="module")
def live_case():
    """S = 256 and head_dim 32, so that the spatial-backward points of BF16_TRAIN apply; one layer, 512 tokens."""
    cfg = pkg("config").GenieConfig(num_layers=1, num_heads=2, d_model=64, T=2, S=256, num_factored_vocabs=2, qk_norm=False,
                                    num_prompt_frames=1)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=3, law="conditioned")
    b = TO.maskgit_collate(syn.make_clips(1, cfg, seed=4), cfg, TO.NumpyDraws(5))
    return cfg, sd, b["input_ids"], b["labels"]


@pytest.mark.parametrize("nm,floor", [(TO.BF16_TRAIN, 1e-4), (TO.F16X3_TRAIN, 1e-6)], ids=["bf16", "f16x3"])
def test_every_rounding_point_is_live(live_case, nm, floor):
    """Switching off any single rounding point moves some gradient tensor by more than f32 noise (relative to the tensor's
    largest element; measured: bf16 5e-4 .. 8e-3, f16x3 3e-6 .. 1e-5), so no point is silently never applied."""
    cfg, sd, ids, labels = live_case
    _, _, g = TO.forward_backward(ids, labels, sd, cfg, nm=nm)
    dead = {}
    for pt in sorted(nm.points):
        _, _, g2 = TO.forward_backward(ids, labels, sd, cfg, nm=nm.without(pt))
        moved = max(float(np.abs(g2[k] - g[k]).max() / np.abs(g[k]).max()) for k in g)
        if moved <= floor:
            dead[pt] = moved
    assert not dead, dead
    assert nm is not TO.BF16_TRAIN or set(nm.points) == set(TO.TrainNumerics.POINTS)


def test_bf16_spatial_backward_follows_the_kernel_dispatch():
    """launch_attn_spatial_bwd_bf16 takes S = 256 with head_dim 32 / 64 only: elsewhere the bf16 trainer's spatial backward is
    f32, and so is the contract's (its bwd_* points are then no-ops)."""
    syn = pkg("synthetic")
    for S, H in ((64, 2), (256, 4)):   # S != 256; head_dim 16
        cfg = pkg("config").GenieConfig(num_layers=1, num_heads=H, d_model=64, T=2, S=S, num_factored_vocabs=2, qk_norm=False,
                                        num_prompt_frames=1)
        sd = syn.make_state_dict(cfg, seed=3, law="conditioned")
        b = TO.maskgit_collate(syn.make_clips(1, cfg, seed=4), cfg, TO.NumpyDraws(5))
        _, _, g = TO.forward_backward(b["input_ids"], b["labels"], sd, cfg, nm=TO.BF16_TRAIN)
        _, _, g2 = TO.forward_backward(b["input_ids"], b["labels"], sd, cfg,
                                       nm=TO.TrainNumerics("no-bwd16", TO.go.round_bf16, TO.TrainNumerics.POINTS))
        assert all(np.array_equal(g[k], g2[k]) for k in g), (S, H)
