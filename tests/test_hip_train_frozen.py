"""Training a subset of the weights on the HIP path (include/genie_hip.h, "Frozen tensors"; GenieTrainer(trainable=..., lr_scale=...)).

The yardsticks are not the code under test: the reference's autograd gradients (tests/golden/train_tiny_*.npz), the FULL training step
(trainable=None: pinned to the oracles by the existing training tests) for bit identity, oracle.genie_train_oracle.adamw_step, the NumPy
EMA restatement (tests/ema_model.py), a fresh trainer built from the saved weights, and the library's own launch profile.

Shapes (the smallest that reach each path): the two committed fixtures (2 layers, d 64, LayerNorm / qk-norm); ln3 and qk3 of
tests/test_hip_train_ema.py (3 layers; generic ln_bwd, head_dim 32 and 64, an odd batch); d256s64 of tests/test_hip_train_bf16.py (TN
weight gradients and cast_rows16 in bf16, ln_bwd_fast_kernel<4>, and in f16x3 the rows-only cast_transpose with token slabs).
Selections: a = the readout; b = the last layer and the readout; c = every bias and every norm weight (db without dw in every Linear);
d = one MLP weight of layer 1, one qkv weight of layer 0 and pos_embed (parameter-free LayerNorm / qk-norm backward everywhere, embedding
backward with dpos alone); e = the token embeddings; f = the action tensors of an action-vector and of an action-id model.
Needs an MI355X: ``-m gpu``; tests/test_train_frozen_cpu.py holds what runs anywhere."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import ema_model as EM
import test_hip_action_vectors as TA
import test_hip_train_bf16 as TB
import test_hip_train_ema as TE
from conftest import load_golden, pkg
from oracle import genie_train_oracle as TO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECISIONS = ["exact", "f16x3", "bf16"]
FIXTURES = ["train_tiny_ln", "train_tiny_qknorm"]
SHAPES = FIXTURES + ["ln3", "qk3", "d256s64"]
TAGS = ["a", "b", "c", "d", "e"]
GRAD_TOL = 1e-4           # tests/test_hip_train.py: exact and f16x3, of the tensor's largest element; bf16: 3 % Frobenius
STEP_KW = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=None)
D_NAMES = "decoder.layers.1.mlp.fc1.weight,decoder.layers.0.spatial_attn.qkv.weight,pos_embed_TSC"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "of", g.size, "words differ")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, sd, input_ids, labels), NumPy, computed once and never written to."""
    if name in FIXTURES:
        z, cfg, sd = load_golden(name)
        return cfg, sd, z["s0_input_ids"], z["s0_labels"]
    return TE.make_case(name) if name in TE.CASES else TB.make_case(name)


def selection(tag, cfg):
    last = cfg.num_layers - 1
    return {"a": "out_x_proj.*", "b": f"decoder.layers.{last}.*,out_x_proj.*", "c": "*.bias,*norm*.weight", "d": D_NAMES,
            "e": "token_embed.*"}[tag]


def make_trainer(cfg, sd, precision, mlp_drop=0.0, **kw):
    c = cfg.shallow_copy()
    c.mlp_drop = mlp_drop
    model = pkg("st_mask_git").STMaskGIT(c, precision=precision).load_numpy_state_dict(sd).to("cuda")
    return pkg("train").GenieTrainer(model, **kw)


def twin_from(tr, precision, **kw):
    """A fresh model of tr's config loaded from tr.model.state_dict() (clones), and a trainer on it (it packs every 16-bit copy)."""
    state = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    model = pkg("st_mask_git").STMaskGIT(tr.model.config.shallow_copy(), precision=precision).to("cuda")
    model.load_state_dict(state)
    return pkg("train").GenieTrainer(model, **kw)


def batch_of(name):
    _, _, ids, labels = case(name)
    return {"input_ids": dev(ids), "labels": dev(labels)}


def params_of(tr):
    return {n: p.detach().cpu().numpy().copy() for n, p in tr.model.named_parameters()}


def grads_of(tr):
    return {n: g.cpu().numpy().copy() for n, g in tr.gradients().items()}


@functools.lru_cache(maxsize=None)
def step_run(shape, tag, precision):
    """One train_step (no clip, weight decay 0.01) of a trainer with selection `tag` (None: everything): parameters before and after,
    the gradients it holds, the loss."""
    cfg, sd, _, _ = case(shape)
    tr = make_trainer(cfg, sd, precision, trainable=None if tag is None else selection(tag, cfg), **STEP_KW)
    before = params_of(tr)
    out = tr.train_step(batch_of(shape))
    return dict(before=before, after=params_of(tr), grads=grads_of(tr), loss=float(out["loss"]), acc=float(out["acc"]),
                grad_norm=float(out["grad_norm"]), names=set(tr.trainable), n_train=tr.n_train, n_flat=tr.n_flat)


# ---------------------------------------------------------------------------------------------- 2, 4: the full step's bits
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_and_step_are_the_full_steps_bits(shape, tag, precision):
    """Every trainable gradient is, bit for bit, the same tensor's gradient of a trainer with trainable=None on the same batch (a
    condition, not a tolerance: the same kernels in the same order); no gradient is kept for a frozen tensor; after one optimizer step
    without a clip the trainable parameters are the full trainer's bits and every frozen parameter has not moved."""
    cfg, _, _, _ = case(shape)
    full, sel = step_run(shape, None, precision), step_run(shape, tag, precision)
    want = pkg("train").select_trainable(full["before"], selection(tag, cfg))
    assert sel["names"] == set(sel["grads"]) == want and 0 < len(want) < len(full["grads"])
    assert sel["n_train"] < sel["n_flat"] == full["n_flat"] == full["n_train"]
    assert sel["loss"] == full["loss"] and sel["acc"] == full["acc"] and np.isfinite(sel["loss"])
    for n in sorted(want):
        assert np.any(full["grads"][n] != 0), n
        same_bits(sel["grads"][n], full["grads"][n], f"gradient of {n}")
    for n, p0 in sel["before"].items():
        same_bits(p0, full["before"][n], f"{n} before the step")
        if n in want:
            same_bits(sel["after"][n], full["after"][n], f"{n} after the step")
            assert not np.array_equal(sel["after"][n], p0), n
        else:
            same_bits(sel["after"][n], p0, f"frozen {n}")


# ---------------------------------------------------------------------------------------------- 1: the reference's autograd
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("shape", FIXTURES)
def test_trainable_gradients_vs_reference_autograd(shape, tag, precision):
    """The bars of tests/test_hip_train.py, unchanged: exact and f16x3 within 1e-4 of the tensor's largest element and the loss within
    1e-5 relative; bf16 within 3 % Frobenius and the loss within 1e-2."""
    z, _, _ = load_golden(shape)
    sel = step_run(shape, tag, precision)
    bad = {}
    for n, g in sel["grads"].items():
        ref = z[f"s0_grad/{n}"]
        if precision == "bf16":
            e = float(np.sqrt(((g.astype(np.float64) - ref) ** 2).sum()) / (np.sqrt((ref.astype(np.float64) ** 2).sum()) + 1e-30))
            if e > 3e-2:
                bad[n] = e
        else:
            e = float(np.abs(g - ref).max() / (np.abs(ref).max() + 1e-30))
            if e > GRAD_TOL:
                bad[n] = e
    assert not bad, bad
    if precision == "bf16":
        assert abs(sel["loss"] - float(z["s0_loss"])) < 1e-2
    else:
        assert abs(sel["loss"] - float(z["s0_loss"])) < 1e-5 * float(z["s0_loss"])


# ---------------------------------------------------------------------------------------------- 2: accumulation, recomputation + dropout
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["c", "d"])
def test_accumulated_gradients_are_the_full_steps_bits(tag, precision):
    """accumulate=True over two micro-batches (beta = 1 in every reduction that is still run)."""
    cfg, sd, ids, labels = case("ln3")
    a = (dev(ids), dev(labels))
    b = (dev(ids[::-1]), dev(labels[::-1]))
    got = []
    for sel in (None, selection(tag, cfg)):
        tr = make_trainer(cfg, sd, precision, trainable=sel)
        tr.forward_backward(*a)
        one = grads_of(tr)
        tr.forward_backward(*b, accumulate=True)
        got.append((one, grads_of(tr)))
    (full1, full2), (sel1, sel2) = got
    assert set(sel2) == pkg("train").select_trainable(full2, selection(tag, cfg))
    for n in sel2:
        same_bits(sel2[n], full2[n], f"accumulated gradient of {n}")
        assert not np.array_equal(sel2[n], sel1[n]), n


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,tag", [("ln3", "b"), ("qk3", "d")])
def test_recompute_with_dropout_is_the_full_steps_bits(shape, tag, precision):
    """recompute=True and mlp_drop=0.1: the layers that are still run are rebuilt and masked as in the full step."""
    cfg, sd, _, _ = case(shape)
    batch = batch_of(shape)
    got = []
    for sel in (None, selection(tag, cfg)):
        tr = make_trainer(cfg, sd, precision, mlp_drop=0.1, recompute=True, dropout_seed=7, trainable=sel)
        loss, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
        got.append((float(loss), grads_of(tr)))
    (lf, full), (ls, sel) = got
    assert lf == ls and 0 < len(sel) < len(full)
    for n in sel:
        same_bits(sel[n], full[n], f"gradient of {n}")


# ---------------------------------------------------------------------------------------------- 3: the skipped work is skipped
def profiled(fn):
    """{class: {kernel name: launches}} of fn() (tests/test_hip_train_bf16.py reads the same table)."""
    lib = pkg("_lib")
    L = lib.load()
    classes = (lib.KC_GEMM, lib.KC_ATTN_TEMPORAL, lib.KC_OTHER)
    lib.check(L.genie_profile_enable(sum(1 << k for k in classes)), "profile_enable")
    L.genie_profile_reset()
    out = {}
    try:
        fn()
        torch.cuda.synchronize()
        for kc in classes:
            kbuf = ctypes.create_string_buffer(16384)
            lib.check(L.genie_profile_kernels(kc, kbuf, len(kbuf)), "profile_kernels")
            out[kc] = {ln.split("\t")[0]: int(float(ln.split("\t")[1])) for ln in kbuf.value.decode().splitlines() if "\t" in ln}
    finally:
        L.genie_profile_enable(0)
    return out


@functools.lru_cache(maxsize=None)
def launches(shape, tag, precision, recompute=False):
    """Launch counts of one forward_backward: GEMM-class launches, temporal attention backward launches (one per layer whose backward
    runs), temporal attention forward launches (one set per layer forward, rebuilt ones included), reductions behind a norm backward,
    TN weight-gradient launches."""
    lib = pkg("_lib")
    cfg, sd, _, _ = case(shape)
    tr = make_trainer(cfg, sd, precision, recompute=recompute, trainable=None if tag is None else selection(tag, cfg))
    batch = batch_of(shape)
    tr.forward_backward(batch["input_ids"], batch["labels"])   # buffers exist, nothing lazy is left to time
    p = profiled(lambda: tr.forward_backward(batch["input_ids"], batch["labels"]))
    t = p[lib.KC_ATTN_TEMPORAL]
    bwd = t.get("attn_temporal_bwd", 0)
    return dict(gemm=sum(p[lib.KC_GEMM].values()), t_bwd=bwd, t_fwd=sum(t.values()) - bwd,
                norm_reduce=p[lib.KC_OTHER].get("slab_reduce_norm", 0), tn=p[lib.KC_GEMM].get(TB.TN, 0))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", ["ln3", "qk3"])
def test_skipped_work_is_not_launched(shape, precision):
    cfg, _, _, _ = case(shape)
    L = cfg.num_layers
    full, a, b, d = (launches(shape, tag, precision) for tag in (None, "a", "b", "d"))
    assert full["t_bwd"] == L and full["norm_reduce"] > 0 and full["t_fwd"] % L == 0
    # a: no per-layer backward kernel; b: none below the last layer -- and what one layer's backward launches is what it always did
    assert a["t_bwd"] == 0 and a["norm_reduce"] == 0 and a["t_fwd"] == full["t_fwd"]
    assert b["t_bwd"] == 1 and b["t_fwd"] == full["t_fwd"]
    per_layer = b["gemm"] - a["gemm"]
    assert per_layer > 0 and full["gemm"] - a["gemm"] == L * per_layer
    assert L * b["norm_reduce"] == full["norm_reduce"]
    # d: every layer's backward runs; of the 6 L + 1 Linear weight gradients exactly two are launched; no reduction behind a norm
    assert d["t_bwd"] == L and full["gemm"] - d["gemm"] == 6 * L + 1 - 2 and d["norm_reduce"] == 0
    # recompute: b rebuilds the last layer alone
    per_fwd = full["t_fwd"] // L
    rec_full, rec_b = launches(shape, None, precision, True), launches(shape, "b", precision, True)
    assert rec_full["t_fwd"] == 2 * full["t_fwd"] and rec_full["t_bwd"] == L
    assert rec_b["t_fwd"] == full["t_fwd"] + per_fwd and rec_b["t_bwd"] == 1


def test_bf16_tn_weight_gradients_of_a_selection():
    """d256s64 in bf16 puts all 13 weight gradients on the TN kernel; selection d launches it twice, selection c never."""
    assert launches("d256s64", None, "bf16")["tn"] == 13
    assert launches("d256s64", "d", "bf16")["tn"] == 2 and launches("d256s64", "c", "bf16")["tn"] == 0
    assert launches("d256s64", "d", "bf16")["norm_reduce"] == 0 < launches("d256s64", "c", "bf16")["norm_reduce"]


# ---------------------------------------------------------------------------------------------- 5: the clip
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["b", "d"])
def test_grad_norm_is_over_the_trainable_gradients(tag, precision):
    """torch's semantics (clip_grad_norm_ over the parameters that have a gradient): out["grad_norm"] within 1e-6 relative of the float64
    norm of the downloaded trainable gradients, and well below the full step's."""
    cfg, sd, _, _ = case("ln3")
    tr = make_trainer(cfg, sd, precision, trainable=selection(tag, cfg), lr=1e-3, max_grad_norm=1.0)
    out = tr.train_step(batch_of("ln3"))
    want = TO.grad_norm(grads_of(tr))
    got = float(out["grad_norm"])
    assert abs(got - want) <= 1e-6 * want, (got, want)
    assert got < 0.999 * step_run("ln3", None, precision)["grad_norm"]


# ---------------------------------------------------------------------------------------------- 6: lr_scale
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lr_scale_against_the_oracles_adamw(precision):
    """One step with lr_scale: every trainable tensor is oracle.adamw_step applied to it with lr * its factor, from the trainer's own
    downloaded gradient, inside the parameter bars of tests/test_hip_train.py::test_two_optimizer_steps_vs_reference; frozen tensors do
    not move; the factors reach different tensors."""
    cfg, sd, _, _ = case("ln3")
    scale = {"out_x_proj.bias": 0.5, "out_x_proj.*": 4.0, "decoder.layers.2.mlp.*": 2.0}
    tr = make_trainer(cfg, sd, precision, trainable=selection("b", cfg), lr_scale=scale, **STEP_KW)
    assert {r[3] for r in tr.adam_runs} == {0.5, 4.0, 2.0, 1.0}
    before = params_of(tr)
    tr.train_step(batch_of("ln3"))
    grads, after = grads_of(tr), params_of(tr)
    factor = pkg("train").lr_factors(before, scale)
    moved = {}
    for n, p0 in before.items():
        if n not in grads:
            same_bits(after[n], p0, f"frozen {n}")
            continue
        want = {n: p0.copy()}
        TO.adamw_step(want, {n: grads[n]}, {}, 1, STEP_KW["lr"] * factor[n], weight_decay=STEP_KW["weight_decay"])
        err = np.abs(after[n] - want[n])
        assert err.mean() < 2e-6 and (err > 2.5e-5).mean() <= 1e-3 and err.max() < 2e-3, (n, err.mean(), err.max())
        moved[n] = float(np.abs(after[n] - p0).mean())
    # Adam's first update is ~ lr * factor per element: the factors are visible in how far each tensor moved
    assert moved["out_x_proj.weight"] > 3 * moved["decoder.layers.2.spatial_attn.qkv.weight"]
    assert moved["decoder.layers.2.mlp.fc1.weight"] > 1.5 * moved["decoder.layers.2.spatial_attn.qkv.weight"]
    assert moved["out_x_proj.bias"] < 0.2 * moved["out_x_proj.weight"]


# ---------------------------------------------------------------------------------------------- 7: selective repack
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,tag", [("ln3", "a"), ("ln3", "b"), ("d256s64", "d")])
def test_selective_repack_leaves_current_copies(shape, tag, precision):
    """After a step that repacked only the trainable Linears, the next forward's loss is bit-equal to that of a fresh trainer (which packs
    everything) built from the model's updated state_dict()."""
    cfg, sd, _, _ = case(shape)
    batch = batch_of(shape)
    tr = make_trainer(cfg, sd, precision, trainable=selection(tag, cfg), **STEP_KW)
    first = float(tr.train_step(batch)["loss"])
    nxt, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
    fresh = twin_from(tr, precision)
    want, _ = fresh.forward_backward(batch["input_ids"], batch["labels"])
    assert float(nxt) == float(want) and float(nxt) != first


# ---------------------------------------------------------------------------------------------- 8: resume
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_resume_with_the_same_and_with_another_selection(precision):
    cfg, sd, _, _ = case("ln3")
    batch = batch_of("ln3")
    kw = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9)
    a = make_trainer(cfg, sd, precision, trainable=selection("b", cfg), **kw)
    a.train_step(batch)
    a.train_step(batch)
    b = twin_from(a, precision, trainable=selection("b", cfg), **kw)
    c = twin_from(a, precision, trainable="decoder.layers.[12].*", **kw)
    state = a.state_dict()
    assert state["trainable"] == sorted(a.trainable) and set(state["state"]) == set(a.trainable) == set(a.gradients())
    assert set(state["ema"]["state"]) == set(a.trainable)
    a.train_step(batch)
    want = params_of(a)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b.load_state_dict(state)
    b.train_step(batch)
    for n, p in params_of(b).items():
        same_bits(p, want[n], f"{n} after the resumed step")
    assert torch.equal(b.ema, a.ema) and torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    # another selection: the names on both sides are restored, the others start from zero moments; it warns and runs
    with pytest.warns(UserWarning, match="different selection of trainable tensors"):
        c.load_state_dict(state)
    lo, hi = c.offsets["decoder.layers.1.mlp.fc1.weight"]
    assert not bool(c.exp_avg[lo:hi].any()) and torch.equal(c.ema[lo:hi], c.params[lo:hi])
    lo, hi = c.offsets["decoder.layers.2.mlp.fc1.weight"]
    assert torch.equal(c.exp_avg[lo:hi].cpu(), state["state"]["decoder.layers.2.mlp.fc1.weight"]["exp_avg"].reshape(-1).cpu())
    assert c.completed_steps == 2
    out = c.train_step(batch)
    assert np.isfinite(float(out["loss"])) and c.completed_steps == 3


# ---------------------------------------------------------------------------------------------- 9: EMA with a selection
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ema_with_a_selection(precision):
    """Inside ema_scope() a frozen tensor is the parameter, a trainable one the NumPy replay (tests/ema_model.py) over the parameters
    captured after each step; on exit the parameters are back bit for bit; ema_state_dict() lists every tensor."""
    cfg, sd, _, _ = case("ln3")
    batch = batch_of("ln3")
    tr = make_trainer(cfg, sd, precision, trainable=selection("b", cfg), ema_decay=0.9, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    assert tr.ema.numel() == tr.n_train < tr.n_flat
    start, seq = params_of(tr), []
    for _ in range(3):
        tr.train_step(batch)
        seq.append(params_of(tr))
    raw = seq[-1]
    avg_sd = tr.ema_state_dict()
    assert set(avg_sd) == set(raw)
    with tr.ema_scope() as model:
        inside = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
        with pytest.raises(RuntimeError):
            tr.train_step(batch)
    for n in raw:
        if n in tr.gradients():
            want = EM.replay(start[n], [s[n] for s in seq], 0.9)[-1]
            same_bits(inside[n], want, f"average of {n}")
            assert not np.array_equal(inside[n], raw[n]), n
        else:
            same_bits(inside[n], raw[n], f"frozen {n} inside the scope")
            same_bits(raw[n], start[n], f"frozen {n}")
        same_bits(avg_sd[n].cpu().numpy(), inside[n], f"ema_state_dict of {n}")
    for n, p in params_of(tr).items():
        same_bits(p, raw[n], f"{n} after the scope")


# ---------------------------------------------------------------------------------------------- f: the action tensors
def action_case(kind):
    """(cfg, sd, keyword arguments of forward_backward) of a 2-layer model conditioned on action vectors (action_dim 3) or action ids."""
    B, A = 2, 3
    c0, ci, cv = TA.cfgs(1 + B * 4, ad=A, num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_prompt_frames=2)
    syn = pkg("synthetic")
    sd0 = syn.make_state_dict(c0, seed=31)
    batch = TO.maskgit_collate(syn.make_clips(B, c0, seed=32), c0, TO.NumpyDraws(33))
    g = np.random.default_rng(34)
    if kind == "vectors":
        return cv, dict(sd0, **TA.proj_weights(c0.d_model, ad=A, seed=9)), batch, dict(
            action_vectors=dev(g.standard_normal((B, c0.T, A)).astype(np.float32)), action_drop=dev(np.array([False, True])))
    table = (0.5 * g.standard_normal((1 + B * 4, c0.d_model))).astype(np.float32)
    return ci, dict(sd0, **{"action_embed.weight": table}), batch, dict(action_ids=dev(1 + np.arange(B * c0.T).reshape(B, c0.T)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["vectors", "ids"])
def test_action_tensors_alone(kind, precision):
    """trainable="action_*" on both kinds of conditioned model: the action gradients are the full step's bits, nothing else has a
    gradient, every layer's backward still runs (the tensors sit below layer 0), and one step moves them alone."""
    cfg, sd, batch, kw = action_case(kind)
    ids, lab = dev(batch["input_ids"]), dev(batch["labels"])
    new = {"action_proj.weight", "action_proj.bias", "action_null"} if kind == "vectors" else {"action_embed.weight"}
    full = make_trainer(cfg, sd, precision, **STEP_KW)
    full.forward_backward(ids, lab, **kw)
    tr = make_trainer(cfg, sd, precision, trainable="action_*", **STEP_KW)
    assert set(tr.gradients()) == new and tr.layout.stop == 0 and tr.layout.embed
    tr.forward_backward(ids, lab, **kw)
    want = grads_of(full)
    for n, g in grads_of(tr).items():
        assert np.any(want[n] != 0), n
        same_bits(g, want[n], f"gradient of {n}")
    before = params_of(tr)
    tr.train_step({"input_ids": ids, "labels": lab, **kw})
    for n, p in params_of(tr).items():
        assert np.array_equal(p, before[n]) == (n not in new), n


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["action_proj.weight", "action_proj.bias", "action_null"])
def test_each_action_projection_tensor_on_its_own(name, precision):
    """The three tensors of an action-vector model are selected one by one; a frozen one's gradient is not kept."""
    cfg, sd, batch, kw = action_case("vectors")
    ids, lab = dev(batch["input_ids"]), dev(batch["labels"])
    full = make_trainer(cfg, sd, precision)
    full.forward_backward(ids, lab, **kw)
    tr = make_trainer(cfg, sd, precision, trainable=[name, "pos_embed_TSC"])
    tr.forward_backward(ids, lab, **kw)
    got, want = grads_of(tr), grads_of(full)
    assert set(got) == {name, "pos_embed_TSC"}
    for n in got:
        same_bits(got[n], want[n], f"gradient of {n}")
    tr.forward_backward(ids, lab, accumulate=True, **kw)   # twice the sum, exactly: x + x
    same_bits(grads_of(tr)[name], want[name] + want[name], f"accumulated gradient of {name}")


# ---------------------------------------------------------------------------------------------- 10: the library's contract, directly
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_all_null_gradient_table_still_propagates_dx(precision):
    """A grads table with every member NULL and no actions: head and layer calls succeed and leave, in the workspace, the d loss / d x the
    full backward leaves there, bit for bit; the embedding call succeeds and writes nothing."""
    lib = pkg("_lib")
    T = pkg("train")
    cfg, sd, ids, labels = case("qk3" if precision == "exact" else "ln3")
    tr = make_trainer(cfg, sd, precision)
    x, y = dev(ids).to(torch.int64).contiguous(), dev(labels).to(torch.int64).contiguous()
    tr.forward_backward(x, y)
    n_dx = x.numel() * cfg.d_model
    want = tr._ws[:4 * n_dx].clone()            # w.dx is the first slot of the workspace: (M, d) floats
    held = tr.grads.clone()
    L, st = tr.lib, tr._stream()
    none, keep = T.weights_table(cfg, {})
    B = x.shape[0]
    lib.check(L.genie_train_forward(tr.cfg, tr.w_table, x.data_ptr(), y.data_ptr(), B, tr._acts.data_ptr(), tr._acts.numel(),
                                    tr.sums.data_ptr(), st), "genie_train_forward")
    tr._ws.zero_()
    lib.check(L.genie_train_backward_head(tr.cfg, tr.w_table, tr.wT_table, none, B, tr._acts.data_ptr(), tr._ws.data_ptr(),
                                          tr._ws.numel(), 0, st), "genie_train_backward_head")
    for layer in reversed(range(cfg.num_layers)):
        lib.check(L.genie_train_backward_layer(tr.cfg, tr.w_table, tr.wT_table, none, layer, B, tr._acts.data_ptr(), tr._ws.data_ptr(),
                                               tr._ws.numel(), 0, st), "genie_train_backward_layer")
    lib.check(L.genie_train_backward_embed(tr.cfg, none, x.data_ptr(), B, tr._ws.data_ptr(), tr._ws.numel(), 0, st),
              "genie_train_backward_embed")
    torch.cuda.synchronize()
    assert torch.equal(tr._ws[:4 * n_dx], want) and bool(want.any())
    assert torch.equal(tr.grads, held)
    del keep


def test_pack_weights_some_refuses_the_exact_precision():
    lib = pkg("_lib")
    cfg, sd, _, _ = case("ln3")
    tr = make_trainer(cfg, sd, "exact")
    st = tr._stream()
    assert tr.lib.genie_train_pack_weights_some(tr.cfg, tr.w_table, tr.w_table, tr.w_table, None, st) == lib.E_ARG
    assert tr.lib.genie_train_pack_weights(tr.cfg, tr.w_table, tr.w_table, tr.w_table, st) == lib.E_ARG
    assert b"exact" in tr.lib.genie_last_error()


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_pack_weights_some_packs_the_selected_linears_only(precision):
    """Poison every 16-bit copy, repack with a selection: the selected Linears' copies are genie_train_pack_weights' bits again, the
    others still hold the poison; select = NULL packs everything."""
    cfg, sd, _, _ = case("ln3")
    tr = make_trainer(cfg, sd, precision, trainable=selection("d", cfg))
    good = {n: (tr.w16[n].clone(), tr.w16T[n].clone()) for n in tr.w16}
    chosen = {n for n in tr.w16 if n in tr.gradients()}
    assert chosen == {"decoder.layers.1.mlp.fc1.weight", "decoder.layers.0.spatial_attn.qkv.weight"}

    def poison():
        for n in tr.w16:
            tr.w16[n].fill_(0x5A5A)
            tr.w16T[n].fill_(0x5A5A)
    poison()
    tr._pack_trained()
    torch.cuda.synchronize()
    for n in tr.w16:
        if n in chosen:
            assert torch.equal(tr.w16[n], good[n][0]) and torch.equal(tr.w16T[n], good[n][1]), n
        else:
            assert bool((tr.w16[n] == 0x5A5A).all()) and bool((tr.w16T[n] == 0x5A5A).all()), n
    poison()
    pkg("_lib").check(tr.lib.genie_train_pack_weights_some(tr.cfg, tr.w_table, tr.w_table, tr.wT_table, None, tr._stream()), "pack")
    torch.cuda.synchronize()
    assert all(torch.equal(tr.w16[n], good[n][0]) and torch.equal(tr.w16T[n], good[n][1]) for n in tr.w16)


def test_trainer_refuses_bad_selections():
    cfg, sd, _, _ = case("ln3")
    for kw in (dict(trainable="decoder.layers.9.*"), dict(trainable=lambda n: False), dict(lr_scale={"*.bias": 0.0}),
               dict(lr_scale={"nope": 2.0})):
        with pytest.raises(ValueError):
            make_trainer(cfg, sd, "exact", **kw)
    tr = make_trainer(cfg, sd, "exact", trainable=lambda n: n.startswith("out_x_proj."))
    assert set(tr.gradients()) == {"out_x_proj.weight", "out_x_proj.bias"} and tr.layout.stop == cfg.num_layers


# ---------------------------------------------------------------------------------------------- the CLI
def test_train_cli_fine_tunes_a_selection(tmp_path):
    """tools/train.py --train_only / --freeze / --lr_scale in fresh child processes under a time limit: two steps that move the selected
    tensors alone (the saved trainer state lists them), and a pattern that matches nothing ends in sys.exit with the trainer's message."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--model", "tiny",
            "--precision", "bf16", "--max_train_steps", "2", "--checkpointing_steps", "2", "--seed", "1", "--per_device_eval_batch_size", "1"]
    r = subprocess.run(base + ["--output_dir", str(tmp_path / "out"), "--train_only", "decoder.layers.*,out_x_proj.*", "--freeze",
                               "decoder.layers.0.*", "--lr_scale", "out_x_proj.*=10,*.bias=0.5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "training " in r.stdout and "the backward stops at layer 1" in r.stdout, r.stdout[-2000:]
    state = torch.load(tmp_path / "out" / "final_checkpt" / "trainer_state.pt", map_location="cpu")
    assert state["trainable"] == sorted(state["state"]) and "out_x_proj.weight" in state["trainable"]
    assert all(n.startswith(("out_x_proj.", "decoder.layers.")) and not n.startswith("decoder.layers.0.") for n in state["trainable"])
    assert state["hyper"]["lr_scale"] == {"out_x_proj.*": 10.0, "*.bias": 0.5}
    for flags, msg in ((["--train_only", "decoder.layer.*"], "matches no parameter name"), (["--lr_scale", "bias"], "PATTERN=FACTOR")):
        bad = subprocess.run(base + ["--output_dir", str(tmp_path / "bad")] + flags, capture_output=True, text=True)
        assert bad.returncode == 1 and "train.py: --train_only / --freeze / --lr_scale:" in bad.stderr and msg in bad.stderr, bad.stderr[-2000:]
        assert "Traceback" not in bad.stderr
