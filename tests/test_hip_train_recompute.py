"""Training with activation recomputation (GenieTrainer(recompute=True); include/genie_hip.h, "Activation recomputation"): the
recomputing step must give the SAME BITS as the saving step -- the forward kernels are bit-reproducible, and the recomputation is the
forward's own layer statement launched again from the layer's checkpoint.

(H, d, T, S, B, qk_norm, use_mup, layers), tokens, what the case reaches; three layers so that a first, a middle and a last checkpoint
exist; all in exact, f16x3 and bf16 (T * S % 64 == 0 everywhere, as the 16-bit step requires):
  ln3     (2, 64, 4, 16, 2, F, F, 3)     128   LayerNorm blocks: u1 and u2 from `norm`
  qk3     (2, 128, 8, 16, 3, T, F, 3)    384   Identity norms: operands from GEMM epilogues and casts, the fc2 hazard (its epilogue would
                                               write the next layer's operand over the shared u1), odd batch, head_dim 64
  t32     (2, 64, 32, 16, 1, F, F, 2)    512   generic temporal forward and its f32 scratch in the 16-bit precisions; tiled temporal backward
  s256qk  (2, 128, 2, 256, 1, T, F, 2)   512   the S = 256 MFMA spatial forward and the fused spatial backward on recomputed qkv_s

Cases are built as tests/test_hip_train_long_window.py::make_case builds them (seeds 77 + H for the weights, 900 + d for the clips,
5 + B for the collator's draws).  The GPU tests need an MI355X (``-m gpu``); tests/test_train_recompute_cpu.py holds what runs anywhere.
"""
import functools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import REPO, pkg
from oracle import genie_train_oracle as TO

# id: (H, d, T, S, B, qk_norm, use_mup, layers)
CASES = {
    "ln3": (2, 64, 4, 16, 2, False, False, 3),
    "qk3": (2, 128, 8, 16, 3, True, False, 3),
    "t32": (2, 64, 32, 16, 1, False, False, 2),
    "s256qk": (2, 128, 2, 256, 1, True, False, 2),
}
# Not among the four: Identity norms with an fc2 (M 2560, N 256, K 1024) ABOVE the limits of the small-problem GEMM kernel (K > 512 and
# M * N = 655,360 > 2^19 outputs), so that in f16x3 layer 1's u1 comes from a throughput kernel's epilogue, as at the GENIE shapes, and the
# recomputation must take the other route of launch_cast16_like_gemm than at qk3 and s256qk (fc2 at 384 and 512 rows, K = 512).
BIG_FC2 = {"qk2k": (4, 256, 8, 64, 5, True, False, 2)}
PRECISIONS = ["exact", "f16x3", "bf16"]
REL = 1e-12   # loss and accuracy: the same forward and CE in both modes; their sums are f64 atomics whose order is free


@functools.lru_cache(maxsize=None)
def make_case(name, **extra):
    """(cfg, sd, input_ids, labels) as NumPy, with the seeds of tests/test_hip_train_long_window.py::make_case; `extra` goes into the
    config (action_vocab_size, action_dim).  Computed once, shared, never written to."""
    H, d, T, S, B, qk_norm, use_mup, layers = {**CASES, **BIG_FC2}[name]
    cfg = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=T // 2, use_mup=use_mup, **extra)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=77 + H, law="conditioned")
    batch = TO.maskgit_collate(syn.make_clips(B, cfg, seed=900 + d), cfg, TO.NumpyDraws(5 + B))
    return cfg, sd, batch["input_ids"], batch["labels"]


def dev(a):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_trainer(cfg, sd, precision, **kw):
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")
    return pkg("train").GenieTrainer(model, **kw)


def pair(cfg, sd, precision, **kw):
    """(saving trainer, recomputing trainer) from the same state dict."""
    return make_trainer(cfg, sd, precision, **kw), make_trainer(cfg, sd, precision, recompute=True, **kw)


def close(a, b):
    a, b = float(a), float(b)
    return a == b or abs(a - b) <= REL * abs(a)


def same_bits(name, precision, stale=False):
    """Two saving runs are torch.equal (the case is deterministic on this box), then the recomputing trainer's whole flat gradient
    buffer is torch.equal to theirs; loss and accuracy agree to REL.  stale: every byte of both activation buffers is 0xFF first, so
    that a slot read before it is (re)written shows up as NaN."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case(name)
    ids, labels = dev(ids), dev(labels)
    B = ids.shape[0]
    saved, rec = pair(cfg, sd, precision)
    if stale:
        for tr in (saved, rec):
            tr._buffers(B)[0].fill_(0xFF)
    l0, a0 = saved.forward_backward(ids, labels)
    g0 = saved.grads.clone()
    if stale:
        saved._buffers(B)[0].fill_(0xFF)
    l0b, a0b = saved.forward_backward(ids, labels)
    assert torch.equal(g0, saved.grads), "the saving step is not deterministic here: nothing can be said about recomputation"
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    l1, a1 = rec.forward_backward(ids, labels)
    diff = int((rec.grads.view(torch.int32) != g0.view(torch.int32)).sum())
    print(f"train_recompute/{precision}/{name}{'/stale' if stale else ''}: loss {float(l0):.12f} / {float(l1):.12f}, "
          f"{diff} of {g0.numel()} gradient words differ, acts {saved._acts.numel()} -> {rec._acts.numel()} bytes")
    assert torch.equal(rec.grads, g0), f"{diff} gradient words differ between the modes"
    assert close(l0, l0b) and close(a0, a0b)
    assert close(l0, l1) and close(a0, a1), (float(l0), float(l1), float(a0), float(a1))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(name, precision):
    same_bits(name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_same_bits_with_fc2_on_a_throughput_kernel(precision):
    """qk2k (2,560 tokens, d 256, hidden 1024, two layers): see BIG_FC2."""
    same_bits("qk2k", precision)


@pytest.mark.gpu
def test_accumulation_same_bits():
    """Two different micro-batches on qk3 in f16x3, the second with accumulate=True: bit-equal gradients between the modes."""
    torch = pytest.importorskip("torch")
    cfg, sd, a_ids, a_lab = make_case("qk3")
    B = a_ids.shape[0]
    b = TO.maskgit_collate(pkg("synthetic").make_clips(B, cfg, seed=5), cfg, TO.NumpyDraws(6))
    assert not np.array_equal(b["input_ids"], a_ids)
    a_ids, a_lab, b_ids, b_lab = dev(a_ids), dev(a_lab), dev(b["input_ids"]), dev(b["labels"])
    saved, rec = pair(cfg, sd, "f16x3")
    for tr in (saved, rec):
        tr.forward_backward(a_ids, a_lab)
    g1 = saved.grads.clone()
    assert torch.equal(rec.grads, g1)
    for tr in (saved, rec):
        tr.forward_backward(b_ids, b_lab, accumulate=True)
    assert not torch.equal(saved.grads, g1)
    assert torch.equal(rec.grads, saved.grads)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ln3", "qk3"])
def test_stale_memory(name):
    """bf16, both activation buffers filled with 0xFF bytes (NaN in f32, bf16 and f16) before every step."""
    same_bits(name, "bf16", stale=True)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "exact"])
def test_two_optimizer_steps(precision):
    """Two train_steps on ln3 (clip at 1.0, AdamW with decay): parameters and both moments bit-equal between the modes after step 2,
    whose recomputation reads the re-packed 16-bit weights."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("ln3")
    batch = {"input_ids": dev(ids), "labels": dev(labels)}
    saved, rec = pair(cfg, sd, precision, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    p0 = saved.params.clone()
    for _ in range(2):
        o0, o1 = saved.train_step(batch), rec.train_step(batch)
        assert close(o0["loss"], o1["loss"]) and float(o0["grad_norm"]) == float(o1["grad_norm"])
    assert saved.completed_steps == rec.completed_steps == 2
    assert not torch.equal(saved.params, p0)
    assert torch.equal(rec.params, saved.params)
    assert torch.equal(rec.exp_avg, saved.exp_avg)
    assert torch.equal(rec.exp_avg_sq, saved.exp_avg_sq)


@pytest.mark.gpu
def test_conditioning_action_ids():
    """ln3 with an action table of 5 rows and random per-frame action ids, exact: every gradient, the table's included."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("ln3", action_vocab_size=5)
    B = ids.shape[0]
    acts = dev(np.random.default_rng(11).integers(0, 5, (B, cfg.T)).astype(np.int64))
    saved, rec = pair(cfg, sd, "exact")
    l0, _ = saved.forward_backward(dev(ids), dev(labels), action_ids=acts)
    l1, _ = rec.forward_backward(dev(ids), dev(labels), action_ids=acts)
    assert close(l0, l1)
    assert float(saved.gradients()["action_embed.weight"].abs().max()) > 0
    assert torch.equal(rec.grads, saved.grads)


@pytest.mark.gpu
def test_conditioning_action_vectors_and_dropout():
    """qk3 with action vectors of 3 values and an action_drop mask, bf16: every gradient, the projection's and the null row's included."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("qk3", action_dim=3)
    B = ids.shape[0]
    vec = dev(np.random.default_rng(12).standard_normal((B, cfg.T, 3)).astype(np.float32))
    drop = dev(np.array([False, True, False]))
    saved, rec = pair(cfg, sd, "bf16")
    l0, _ = saved.forward_backward(dev(ids), dev(labels), action_vectors=vec, action_drop=drop)
    l1, _ = rec.forward_backward(dev(ids), dev(labels), action_vectors=vec, action_drop=drop)
    assert close(l0, l1)
    for k in ("action_proj.weight", "action_proj.bias", "action_null"):
        assert float(saved.gradients()[k].abs().max()) > 0, k
        assert torch.equal(rec.gradients()[k], saved.gradients()[k]), k
    assert torch.equal(rec.grads, saved.grads)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_sizes_in_use(precision):
    """The recomputing trainer allocates genie_train_activation_bytes_ex(cfg, B, 1), less than the saving trainer; a forward given one
    byte less is refused with GENIE_E_ARG and the error names both sizes."""
    torch = pytest.importorskip("torch")
    lib_mod = pkg("_lib")
    cfg, sd, ids, labels = make_case("ln3")
    ids, labels = dev(ids), dev(labels)
    B = ids.shape[0]
    saved, rec = pair(cfg, sd, precision)
    L = rec.lib
    saved.forward_backward(ids, labels)
    rec.forward_backward(ids, labels)
    n1 = L.genie_train_activation_bytes_ex(rec.cfg, B, 1)
    assert rec._acts.numel() == n1 > 0
    assert saved._acts.numel() == L.genie_train_activation_bytes_ex(rec.cfg, B, 0) == L.genie_train_activation_bytes(rec.cfg, B)
    assert n1 < saved._acts.numel()
    assert rec._ws.numel() == L.genie_train_workspace_bytes_ex(rec.cfg, B, 1)
    g = rec.grads.clone()
    st = torch.cuda.current_stream().cuda_stream
    rc = L.genie_train_forward_ex(rec.cfg, rec.w_table, ids.data_ptr(), labels.data_ptr(), B, rec._acts.data_ptr(), n1 - 1,
                                  rec.sums.data_ptr(), st, None, 1)
    assert rc == lib_mod.E_ARG
    msg = L.genie_last_error().decode()
    assert str(n1 - 1) in msg and re.search(rf"\b{n1}\b", msg), msg
    # ... and a buffer sized for mode 1 is too small for mode 0
    rc = L.genie_train_forward_ex(rec.cfg, rec.w_table, ids.data_ptr(), labels.data_ptr(), B, rec._acts.data_ptr(), n1,
                                  rec.sums.data_ptr(), st, None, 0)
    assert rc == lib_mod.E_ARG
    torch.cuda.synchronize()
    assert torch.equal(rec.grads, g)


@pytest.mark.gpu
def test_resume_across_modes_is_silent():
    """state_dict()["hyper"] records the mode; loading it into a trainer of the other mode does not warn (the mode changes no number),
    and the resumed trainer continues to the same bits."""
    torch = pytest.importorskip("torch")
    cfg, sd, ids, labels = make_case("ln3")
    batch = {"input_ids": dev(ids), "labels": dev(labels)}
    saved, rec = pair(cfg, sd, "exact", lr=1e-3)
    saved.train_step(batch)
    state = saved.state_dict()
    assert state["hyper"]["recompute"] is False and rec.state_dict()["hyper"]["recompute"] is True
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rec.load_state_dict(state)
    rec.params.copy_(saved.params)
    rec.sync_external_weights()
    saved.train_step(batch)
    rec.train_step(batch)
    assert torch.equal(rec.params, saved.params) and torch.equal(rec.exp_avg_sq, saved.exp_avg_sq)


@pytest.mark.gpu
def test_train_cli_recompute_activations(tmp_path):
    """tools/train.py --synthetic 8 --max_train_steps 2 --seed 1 --genie_config <2 layers, d 64> in fresh child processes, with and
    without --recompute_activations (plus what the tool needs to start: an --output_dir, and an eval batch of 1 for the one eval clip
    that 8 synthetic clips leave): both return 0 and print the same `step 2: train_loss` line, up to its last field, the measured
    examples/s, which is wall-clock time."""
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False,
                                    num_prompt_frames=2, use_mup=False)
    cfg.save_pretrained(tmp_path / "config.json")
    lines = []
    for flag in ([], ["--recompute_activations"]):
        cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--max_train_steps", "2", "--seed", "1",
               "--genie_config", str(tmp_path / "config.json"), "--per_device_eval_batch_size", "1", "--output_dir",
               str(tmp_path / ("out" + str(len(flag))))] + flag
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        step2 = [ln for ln in res.stdout.splitlines() if ln.startswith("step 2: train_loss")]
        assert len(step2) == 1, res.stdout[-2000:]
        lines.append(re.sub(r"\s+[0-9.]+ examples/s.*$", "", step2[0]))
    assert "train_loss" in lines[0] and "|g|" in lines[0]
    assert lines[0] == lines[1], lines
