"""LoRA adapters on the HIP path (include/genie_hip.h, "LoRA adapters"; csrc/kernels_lora.hip; GenieTrainer(lora=LoraConfig(...));
STMaskGIT.load_adapter).

The yardsticks are not the code under test: the float64 model of tests/lora_model.py with its derived bound, (n + 2) * 2^-24 * sum |terms|;
the FULL training step on the merged model (a twin trainer: pinned to the oracles by the existing training tests) whose dW the projection
must be of; oracle.genie_train_oracle.forward_backward and adamw_step; a direct genie_lora_merge call; a fresh model.
Shapes: the tiny fixtures and d256s64 that tests/test_hip_train_frozen.py uses.  Needs an MI355X: ``-m gpu``; tests/test_train_lora_cpu.py
holds what runs anywhere."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lora_model as LM
import test_hip_train_frozen as TF
from conftest import REPO, pkg
from oracle import genie_train_oracle as TO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECISIONS = TF.PRECISIONS
GUARD = 64   # floats on either side of every buffer
MARK = np.float32(-7.25)
LC = dict(rank=4, alpha=8.0, targets="decoder.layers.*", seed=0)


def lora_cfg(**kw):
    return pkg("train").LoraConfig(**dict(LC, **kw))


# ---------------------------------------------------------------------------------------------- 1: the kernels on guarded buffers
class Guarded:
    """A device buffer holding `a` between two runs of GUARD marker floats."""

    def __init__(self, a):
        a = np.ascontiguousarray(a, np.float32)
        self.shape = a.shape
        full = np.concatenate([np.full(GUARD, MARK), a.reshape(-1), np.full(GUARD, MARK)])
        self.full = TF.dev(full)
        self.ptr = self.full.data_ptr() + 4 * GUARD

    def get(self):
        h = self.full.cpu().numpy()
        assert np.all(h[:GUARD] == MARK) and np.all(h[-GUARD:] == MARK), "a guard was written"
        return h[GUARD:-GUARD].reshape(self.shape).copy()


CASES = [(48, 16, 1), (16, 48, 3), (30, 64, 4), (2048, 512, 64), (512, 2048, 16)]
MIXED = CASES[:3] + [(64, 64, 8), (65, 16, 2), (1, 32, 64), (130, 80, 5), (256, 128, 16)]   # eight items, one launch


@functools.lru_cache(maxsize=None)
def operands(out, in_, r):
    g = np.random.default_rng(out * 7 + in_ * 3 + r)
    f = lambda *s: g.standard_normal(s).astype(np.float32)   # noqa: E731
    return dict(w0=f(out, in_), a=f(r, in_), b=f(out, r), dw=f(out, in_), da0=f(r, in_), db0=f(out, r), s=np.float32(16.0 / r))


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_merge(shapes, in_place=False):
    """One genie_lora_merge launch over `shapes`; returns [(W as computed, operands)]."""
    L, lib_mod = pkg("lora"), pkg("_lib")
    lib = lib_mod.load()
    bufs, items = [], []
    for shp in shapes:
        o = operands(*shp)
        w0, a, b = Guarded(o["w0"]), Guarded(o["a"]), Guarded(o["b"])
        w = w0 if in_place else Guarded(np.full_like(o["w0"], np.nan))
        bufs.append((w, w0, a, b))
        items.append(L.item(float(o["s"]), shp[0], shp[1], shp[2], a.ptr, b.ptr, w=w.ptr, w0=w0.ptr))
    arr, n = L.table(items)
    lib_mod.check(lib.genie_lora_merge(arr, n, stream()), "genie_lora_merge")
    torch.cuda.synchronize()
    out = []
    for (w, w0, a, b), shp in zip(bufs, shapes):
        o = operands(*shp)
        if not in_place:
            assert np.array_equal(w0.get(), o["w0"])
        assert np.array_equal(a.get(), o["a"]) and np.array_equal(b.get(), o["b"])
        out.append((w.get(), o))
    return out


def run_project(shapes, accumulate=0, poison=None):
    """One genie_lora_project call over `shapes`; returns [(dA, dB, operands)].  poison: byte the scratch is filled with first."""
    L, lib_mod = pkg("lora"), pkg("_lib")
    lib = lib_mod.load()
    bufs, items = [], []
    for shp in shapes:
        o = operands(*shp)
        a, b, dw, da, db = (Guarded(o[k]) for k in ("a", "b", "dw", "da0", "db0"))
        bufs.append((a, b, dw, da, db))
        items.append(L.item(float(o["s"]), shp[0], shp[1], shp[2], a.ptr, b.ptr, dw=dw.ptr, da=da.ptr, db=db.ptr))
    arr, n = L.table(items)
    need = lib.genie_lora_project_scratch_bytes(arr, n)
    assert need > 0
    scratch = torch.full((need + 4 * 2 * GUARD,), 0 if poison is None else poison, dtype=torch.uint8, device="cuda")
    scratch[:4 * GUARD] = 0x5A
    scratch[-4 * GUARD:] = 0x5A
    lib_mod.check(lib.genie_lora_project(arr, n, accumulate, scratch.data_ptr() + 4 * GUARD, need, stream()), "genie_lora_project")
    torch.cuda.synchronize()
    assert bool((scratch[:4 * GUARD] == 0x5A).all()) and bool((scratch[-4 * GUARD:] == 0x5A).all()), "the scratch's guards were written"
    out = []
    for (a, b, dw, da, db), shp in zip(bufs, shapes):
        o = operands(*shp)
        assert np.array_equal(a.get(), o["a"]) and np.array_equal(b.get(), o["b"]) and np.array_equal(dw.get(), o["dw"])
        out.append((da.get(), db.get(), o))
    return out


def check_merge(got, o, what):
    want, bound = LM.merge(o["w0"], o["a"], o["b"], float(o["s"]))
    LM.within(got, want, bound, what)


def check_project(da, db, o, accumulate, what):
    wa, wb, ba, bb = LM.project(o["dw"], o["a"], o["b"], float(o["s"]), o["da0"] if accumulate else None, o["db0"] if accumulate else None)
    LM.within(da, wa, ba, what + " dA")
    LM.within(db, wb, bb, what + " dB")


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_merge_kernel(shape):
    (w, o), = run_merge([shape])
    check_merge(w, o, f"merge {shape}")
    (w2, _), = run_merge([shape], in_place=True)
    TF.same_bits(w2, w, f"in-place merge {shape}")
    assert not np.array_equal(w, o["w0"])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_project_kernel(shape, accumulate):
    (da, db, o), = run_project([shape], accumulate)
    check_project(da, db, o, accumulate, f"project {shape} accumulate={accumulate}")
    # the same call again, and with poisoned scratch: the same bits
    (da2, db2, _), = run_project([shape], accumulate)
    (da3, db3, _), = run_project([shape], accumulate, poison=0xFF)
    for x, y, what in ((da2, da, "dA again"), (db2, db, "dB again"), (da3, da, "dA, poisoned scratch"), (db3, db, "dB, poisoned scratch")):
        TF.same_bits(x, y, what)


def test_eight_mixed_items_in_one_launch():
    for (w, o), shp in zip(run_merge(MIXED), MIXED):
        check_merge(w, o, f"merge {shp} of 8")
    for (w, o), shp in zip(run_merge(MIXED, in_place=True), MIXED):
        check_merge(w, o, f"in-place merge {shp} of 8")
    for acc in (0, 1):
        res = run_project(MIXED, acc)
        for (da, db, o), shp in zip(res, MIXED):
            check_project(da, db, o, acc, f"project {shp} of 8, accumulate={acc}")
        for (da, db, _), (da2, db2, _) in zip(res, run_project(MIXED, acc, poison=0xFF)):
            TF.same_bits(da2, da, "dA")
            TF.same_bits(db2, db, "dB")


def test_a_refusal_leaves_the_outputs_as_they_were():
    """A good first item and a refused second: nothing is launched, for any of the refusals that need real buffers to show it."""
    L, lib_mod = pkg("lora"), pkg("_lib")
    lib = lib_mod.load()
    o = operands(30, 64, 4)
    w, w0, a, b, dw, da, db = (Guarded(o[k]) for k in ("w0", "w0", "a", "b", "dw", "da0", "db0"))
    ok = dict(w=w.ptr, w0=w0.ptr, dw=dw.ptr, da=da.ptr, db=db.ptr)
    good = L.item(2.0, 30, 64, 4, a.ptr, b.ptr, **ok)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    bads = [L.item(2.0, 30, 64, 65, a.ptr, b.ptr, **ok), L.item(2.0, 30, 24, 4, a.ptr, b.ptr, **ok), L.item(float("nan"), 30, 64, 4, a.ptr, b.ptr, **ok),
            L.item(2.0, 30, 64, 4, None, b.ptr, **ok), L.item(2.0, 30, 64, 4, w.ptr, b.ptr, **dict(ok, da=w.ptr))]   # (a over w, and over da)
    for bad in bads:
        arr, n = L.table([good, bad])
        assert lib.genie_lora_merge(arr, n, stream()) == lib_mod.E_ARG
        assert lib.genie_lora_project(arr, n, 0, scratch.data_ptr(), scratch.numel(), stream()) == lib_mod.E_ARG
    arr, n = L.table([good])
    assert lib.genie_lora_project(arr, n, 0, scratch.data_ptr(), 64, stream()) == lib_mod.E_ARG        # too little scratch
    assert lib.genie_lora_project(arr, 9, 0, scratch.data_ptr(), scratch.numel(), stream()) == lib_mod.E_ARG
    torch.cuda.synchronize()
    for buf, k in ((w, "w0"), (da, "da0"), (db, "db0")):
        TF.same_bits(buf.get(), o[k], k)


# ---------------------------------------------------------------------------------------------- trainer helpers
def lora_trainer(shape, precision, lora=None, **kw):
    cfg, sd, _, _ = TF.case(shape)
    return TF.make_trainer(cfg, sd, precision, lora=lora or lora_cfg(), **kw)


def random_adapters(tr, seed=5):
    """A as drawn, B ~ N(0, 0.02), through load_adapter_state_dict.  Returns the NumPy tensors."""
    g = np.random.default_rng(seed)
    sd = {n: t.cpu().numpy() for n, t in tr.adapter_state_dict().items()}
    for n in sd:
        if n.endswith(".lora_B"):
            sd[n] = (0.02 * g.standard_normal(sd[n].shape)).astype(np.float32)
    tr.load_adapter_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    return sd


def check_adapter_grads(tr, dws, adapters, what, old=None):
    """Every adapter gradient of `tr` is the float64 projection of `dws` (the twin's dW by weight name) within the kernels' bound."""
    L = pkg("lora")
    grads = TF.grads_of(tr)
    for n in tr.lora_targets:
        na, nb = L.adapter_names(n)
        wa, wb, ba, bb = LM.project(dws[n], adapters[na], adapters[nb], tr.lora.scale, None if old is None else old[na],
                                    None if old is None else old[nb])
        LM.within(grads[na], wa, ba, f"{what}: {na}")
        LM.within(grads[nb], wb, bb, f"{what}: {nb}")
        assert np.any(grads[na] != 0) and np.any(grads[nb] != 0), n
    return grads


# ---------------------------------------------------------------------------------------------- 2: B = 0 is the base model
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", TF.FIXTURES)
def test_a_fresh_adapter_is_the_base_model(shape, precision):
    cfg, sd, _, _ = TF.case(shape)
    base = TF.make_trainer(cfg, sd, precision)
    tr = lora_trainer(shape, precision)
    want = TF.params_of(base)
    for n, p in TF.params_of(tr).items():
        assert np.array_equal(p, want[n]), n
    batch = TF.batch_of(shape)
    l0, a0 = base.forward_backward(batch["input_ids"], batch["labels"])
    l1, a1 = tr.forward_backward(batch["input_ids"], batch["labels"])
    assert float(l0) == float(l1) and float(a0) == float(a1) and np.isfinite(float(l1))
    grads = TF.grads_of(tr)
    assert set(grads) == {n for t in tr.lora_targets for n in pkg("lora").adapter_names(t)} and len(grads) == 2 * 6 * cfg.num_layers
    assert tr.n_train < base.n_train // 4 and tr.layout.stop == 0 and tr.ema is None
    for n, g in grads.items():
        if n.endswith(".lora_A"):
            assert not np.any(g), n          # dA = s B^T dW with B = 0
    assert any(np.any(g) for n, g in grads.items() if n.endswith(".lora_B"))
    assert all(np.any(g) for n, g in grads.items() if n.endswith(".lora_B")), [n for n, g in grads.items() if n.endswith("B") and not np.any(g)]


def test_constructor_refusals_and_the_neutral_trainer():
    cfg, sd, _, _ = TF.case("train_tiny_ln")
    with pytest.raises(ValueError, match="matches no Linear weight"):
        TF.make_trainer(cfg, sd, "exact", lora=lora_cfg(targets="decoder.layers.7.*"))
    with pytest.raises(ValueError, match="adapted by `lora` and named by `trainable`"):
        TF.make_trainer(cfg, sd, "exact", lora=lora_cfg(), trainable="decoder.layers.1.mlp.*")
    with pytest.raises(TypeError):
        TF.make_trainer(cfg, sd, "exact", lora=dict(LC))
    plain = TF.make_trainer(cfg, sd, "exact")
    assert plain.lora is None and not hasattr(plain, "w0") and not hasattr(plain, "_lora_scratch")
    with pytest.raises(RuntimeError, match="needs a trainer built with lora="):
        plain.adapter_state_dict()


# ---------------------------------------------------------------------------------------------- 3: the projection reads the step's own dW
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", ["train_tiny_qknorm", "d256s64"])
def test_adapter_gradients_are_the_projection_of_the_full_steps_dw(shape, precision):
    tr = lora_trainer(shape, precision, lora=lora_cfg(targets="decoder.layers.*,out_x_proj.weight"))
    w0 = {n: t.cpu().numpy() for n, t in tr.w0.items()}
    ad = random_adapters(tr)
    n0 = "decoder.layers.0.mlp.fc1.weight"
    moved = np.abs(TF.params_of(tr)[n0] - w0[n0]).max()
    assert moved > 100 * (4 + 2) * LM.U * np.abs(w0[n0]).max()      # W_eff is far from W0 on the scale of the bars below
    batch = TF.batch_of(shape)
    twin = TF.twin_from(tr, precision)
    lt, _ = twin.forward_backward(batch["input_ids"], batch["labels"])
    l, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
    assert float(l) == float(lt)
    check_adapter_grads(tr, TF.grads_of(twin), ad, f"{shape} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_accumulated_adapter_gradients(precision):
    """Two micro-batches with accumulate: the second call adds the projection of ITS dW (the reused scratch starts from zero: no other
    layer's or micro-batch's dW leaks in) to what the first left."""
    cfg, sd, ids, labels = TF.case("ln3")
    a, b = (TF.dev(ids), TF.dev(labels)), (TF.dev(ids[::-1]), TF.dev(labels[::-1]))
    tr = lora_trainer("ln3", precision, lora=lora_cfg(targets="decoder.layers.*,out_x_proj.weight"))
    ad = random_adapters(tr)
    twin = TF.twin_from(tr, precision)
    tr.forward_backward(*a)
    twin.forward_backward(*a)
    first = check_adapter_grads(tr, TF.grads_of(twin), ad, f"first micro-batch {precision}")
    tr.forward_backward(*b, accumulate=True)
    twin.forward_backward(*b)
    second = check_adapter_grads(tr, TF.grads_of(twin), ad, f"second micro-batch {precision}", old=first)
    assert all(not np.array_equal(second[n], first[n]) for n in first)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_recompute_with_dropout(precision):
    kw = dict(mlp_drop=0.1, recompute=True, dropout_seed=7)
    tr = lora_trainer("qk3", precision, **kw)
    ad = random_adapters(tr)
    batch = TF.batch_of("qk3")
    twin = TF.twin_from(tr, precision, recompute=True, dropout_seed=7)
    lt, _ = twin.forward_backward(batch["input_ids"], batch["labels"])
    l, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
    assert float(l) == float(lt)
    check_adapter_grads(tr, TF.grads_of(twin), ad, f"recompute + dropout {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_adapters_beside_trained_action_tensors(precision):
    """trainable="action_*" beside the adapters on a model conditioned on action vectors: the action gradients are the full step's bits."""
    cfg, sd, batch, kw = TF.action_case("vectors")
    ids, lab = TF.dev(batch["input_ids"]), TF.dev(batch["labels"])
    tr = TF.make_trainer(cfg, sd, precision, lora=lora_cfg(), trainable="action_*")
    new = {"action_proj.weight", "action_proj.bias", "action_null"}
    assert set(tr.trainable) == new | {n for t in tr.lora_targets for n in pkg("lora").adapter_names(t)}
    ad = random_adapters(tr)
    twin = TF.twin_from(tr, precision)
    tr.forward_backward(ids, lab, **kw)
    twin.forward_backward(ids, lab, **kw)
    full = TF.grads_of(twin)
    got = check_adapter_grads(tr, full, ad, f"action model {precision}")
    for n in sorted(new):
        TF.same_bits(got[n], full[n], f"gradient of {n}")
        assert np.any(got[n]), n


# ---------------------------------------------------------------------------------------------- 4: against the oracle
@functools.lru_cache(maxsize=None)
def oracle_case(shape):
    """Random adapters merged in float64 into the fixture's weights, and the oracle's float64 gradients on the merged model."""
    cfg, sd, ids, labels = TF.case(shape)
    L = pkg("lora")
    shapes = {n: v.shape for n, v in sd.items()}
    targets = L.select_targets(cfg, ["decoder.layers.*", "out_x_proj.weight"])
    g = np.random.default_rng(11)
    ad = {}
    for n, shp in L.adapter_shapes(targets, shapes, LC["rank"]).items():
        ad[n] = L.draw_a(n, shp, 0) if n.endswith(".lora_A") else (0.02 * g.standard_normal(shp)).astype(np.float32)
    _, _, grads = TO.forward_backward(ids, labels, merged_sd(sd, ad, targets), cfg, dtype=np.float64)
    return ad, targets, grads


def merged_sd(sd, ad, targets):
    L = pkg("lora")
    out = dict(sd)
    for n in targets:
        na, nb = L.adapter_names(n)
        out[n] = LM.merge(sd[n], ad[na], ad[nb], LC["alpha"] / LC["rank"])[0].astype(np.float32)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", TF.FIXTURES)
def test_adapter_gradients_against_the_oracle(shape, precision):
    """The project's bars (tests/test_hip_train.py: 1e-4 of the tensor's largest element in exact and f16x3, 3 % Frobenius in bf16) carried
    through the projection: an error e in dW moves dA[k, :] by at most s ||B[:, k]||_1 max|e| (and ||delta dA||_F <= s ||B||_2 ||e||_F)."""
    L = pkg("lora")
    ad, targets, ref = oracle_case(shape)
    tr = lora_trainer(shape, precision, lora=lora_cfg(targets="decoder.layers.*,out_x_proj.weight"))
    tr.load_adapter_state_dict({n: torch.from_numpy(v) for n, v in ad.items()})
    batch = TF.batch_of(shape)
    tr.forward_backward(batch["input_ids"], batch["labels"])
    grads, s = TF.grads_of(tr), tr.lora.scale
    for n in targets:
        na, nb = L.adapter_names(n)
        A, B, dw = ad[na].astype(np.float64), ad[nb].astype(np.float64), ref[n].astype(np.float64)
        wa, wb, ba, bb = LM.project(dw, A, B, s)
        ea, eb = grads[na] - wa, grads[nb] - wb
        if precision == "bf16":
            fro = np.sqrt((dw ** 2).sum())
            assert np.sqrt((ea ** 2).sum()) <= s * np.linalg.norm(B, 2) * 0.03 * fro, na
            assert np.sqrt((eb ** 2).sum()) <= s * np.linalg.norm(A, 2) * 0.03 * fro, nb
        else:
            top = TF.GRAD_TOL * np.abs(dw).max()
            LM.within(grads[na], wa, s * np.abs(B).sum(0)[:, None] * top + ba, f"{na} vs the oracle")
            LM.within(grads[nb], wb, s * np.abs(A).sum(1)[None, :] * top + bb, f"{nb} vs the oracle")


# ---------------------------------------------------------------------------------------------- 5: one optimizer step
def direct_merge(w0, a, b, s):
    """genie_lora_merge on copies: (out, in) NumPy."""
    L, lib_mod = pkg("lora"), pkg("_lib")
    w0d, ad, bd = TF.dev(w0), TF.dev(a), TF.dev(b)
    w = torch.empty_like(w0d)
    arr, n = L.table([L.item(s, w0.shape[0], w0.shape[1], a.shape[0], ad.data_ptr(), bd.data_ptr(), w=w.data_ptr(), w0=w0d.data_ptr())])
    lib_mod.check(lib_mod.load().genie_lora_merge(arr, n, stream()), "genie_lora_merge")
    return w.cpu().numpy()


def check_merged(tr, params, adapters, what):
    L = pkg("lora")
    for n in tr.lora_targets:
        na, nb = L.adapter_names(n)
        TF.same_bits(params[n], direct_merge(tr.w0[n].cpu().numpy(), adapters[na], adapters[nb], tr.lora.scale), f"{what}: {n}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", ["ln3", "d256s64"])
def test_one_optimizer_step(shape, precision):
    tr = lora_trainer(shape, precision, **TF.STEP_KW)
    ad = random_adapters(tr)
    before, w0 = TF.params_of(tr), {n: t.cpu().numpy() for n, t in tr.w0.items()}
    batch = TF.batch_of(shape)
    first = float(tr.train_step(batch)["loss"])
    grads, after = TF.grads_of(tr), TF.params_of(tr)
    new = {n: t.cpu().numpy() for n, t in tr.adapter_state_dict().items()}
    for n in ad:   # the bars of tests/test_hip_train_frozen.py::test_lr_scale_against_the_oracles_adamw
        want = {n: ad[n].copy()}
        TO.adamw_step(want, {n: grads[n]}, {}, 1, TF.STEP_KW["lr"], weight_decay=TF.STEP_KW["weight_decay"])
        err = np.abs(new[n] - want[n])
        assert err.mean() < 2e-6 and (err > 2.5e-5).mean() <= 1e-3 and err.max() < 2e-3, (n, err.mean(), err.max())
        assert not np.array_equal(new[n], ad[n]), n
    check_merged(tr, after, new, "after the step")
    for n, p in after.items():
        if n in w0:
            TF.same_bits(tr.w0[n].cpu().numpy(), w0[n], f"W0 of {n}")
            assert not np.array_equal(p, before[n]), n
        else:
            TF.same_bits(p, before[n], f"frozen {n}")
    # the 16-bit copies of the adapted Linears are current (tests/test_hip_train_frozen.py::test_selective_repack_leaves_current_copies)
    nxt, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
    want, _ = TF.twin_from(tr, precision).forward_backward(batch["input_ids"], batch["labels"])
    assert float(nxt) == float(want) and float(nxt) != first


# ---------------------------------------------------------------------------------------------- 6: several steps
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_twenty_steps_lower_the_loss(precision):
    tr = lora_trainer("train_tiny_ln", precision, lr=1e-2, max_grad_norm=1.0)
    batch = TF.batch_of("train_tiny_ln")
    losses = [float(tr.train_step(batch)["loss"]) for _ in range(20)]
    assert losses[-1] < losses[0] - 0.05, (losses[0], losses[-1])
    out = tr.model(batch["input_ids"], batch["labels"])   # the module's inference entry point sees the adapted weights
    assert float(out.loss) < losses[0] - 0.05


@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_resume_reproduces_the_adapter_bits(precision):
    kw = dict(lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    batch = TF.batch_of("ln3")
    a = lora_trainer("ln3", precision, **kw)
    for _ in range(2):
        a.train_step(batch)
    state, adapters = a.state_dict(), a.adapter_state_dict()
    assert set(state["state"]) == set(adapters) == set(state["ema"]["state"])
    for _ in range(2):
        a.train_step(batch)
    b = lora_trainer("ln3", precision, **kw)   # on the base model: W0 comes from it, the adapters and their moments from the saved state
    b.load_adapter_state_dict(adapters)
    b.load_state_dict(state)
    for _ in range(2):
        b.train_step(batch)
    got, want = b.adapter_state_dict(), a.adapter_state_dict()
    for n in want:
        TF.same_bits(got[n].cpu().numpy(), want[n].cpu().numpy(), n)
    TF.same_bits(b.ema.cpu().numpy(), a.ema.cpu().numpy(), "the averaged adapters")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ema_scope_runs_on_the_merged_average(precision):
    tr = lora_trainer("ln3", precision, lr=1e-2, ema_decay=0.5)
    batch = TF.batch_of("ln3")
    for _ in range(3):
        tr.train_step(batch)
    raw, raw_ad = TF.params_of(tr), {n: t.cpu().numpy() for n, t in tr.adapter_state_dict().items()}
    raw_loss = float(tr.model(batch["input_ids"], batch["labels"]).loss)
    with tr.ema_scope() as m:
        avg_ad = {n: t.cpu().numpy() for n, t in tr.adapter_state_dict().items()}
        assert any(not np.array_equal(avg_ad[n], raw_ad[n]) for n in raw_ad)
        check_merged(tr, TF.params_of(tr), avg_ad, "inside the scope")
        avg_loss = float(m(batch["input_ids"], batch["labels"]).loss)
        fresh = pkg("st_mask_git").STMaskGIT(m.config.shallow_copy(), precision=precision).to("cuda")
        fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
        assert float(fresh(batch["input_ids"], batch["labels"]).loss) == avg_loss != raw_loss
    for n, p in TF.params_of(tr).items():
        TF.same_bits(p, raw[n], f"{n} after the scope")
    assert float(tr.model(batch["input_ids"], batch["labels"]).loss) == raw_loss


# ---------------------------------------------------------------------------------------------- 7: serving
@pytest.mark.parametrize("precision", PRECISIONS)
def test_serving_an_adapter(tmp_path, precision):
    cfg, sd, ids, _ = TF.case("train_tiny_qknorm")
    M = pkg("st_mask_git").STMaskGIT
    M(cfg.shallow_copy(), precision=precision).load_numpy_state_dict(sd).save_pretrained(str(tmp_path / "base"))
    tr = lora_trainer("train_tiny_qknorm", precision, lora=lora_cfg(targets="decoder.layers.*,out_x_proj.weight"), lr=1e-2)
    batch = TF.batch_of("train_tiny_qknorm")
    for _ in range(3):
        tr.train_step(batch)
    tr.save_adapter(str(tmp_path / "adapter"))
    x = TF.dev(ids)
    trained = tr.model.compute_logits(x).cpu().numpy()
    served = M.from_pretrained(str(tmp_path / "base"), precision=precision).to("cuda")
    base = served.compute_logits(x).cpu().numpy()
    assert served.load_adapter(str(tmp_path / "adapter")) is served
    TF.same_bits(served.compute_logits(x).cpu().numpy(), trained, "logits with the adapter")
    assert not np.array_equal(trained, base)
    served.load_adapter(str(tmp_path / "adapter"))        # a second load unloads the first: not applied twice
    TF.same_bits(served.compute_logits(x).cpu().numpy(), trained, "logits after a second load")
    # a wrong-shaped and a wrong-base adapter raise and leave the model as it is
    acfg, tensors = pkg("lora").load_adapter_files(str(tmp_path / "adapter"))
    bad = dict(tensors, **{"out_x_proj.lora_A": torch.zeros(4, 32)})
    for adapter, msg in (((acfg, bad), "has shape"), ((dict(acfg, base=dict(acfg["base"], d_model=128)), tensors), "another base model"),
                         ((dict(acfg, targets=acfg["targets"] + ["decoder.layers.9.mlp.fc1.weight"]), tensors), "not Linear weights")):
        with pytest.raises(ValueError, match=msg):
            served.load_adapter(adapter)
        TF.same_bits(served.compute_logits(x).cpu().numpy(), trained, "logits after a refused load")
    served.unload_adapter()
    TF.same_bits(served.compute_logits(x).cpu().numpy(), base, "logits after unload_adapter")
    for n, p in served.state_dict().items():
        TF.same_bits(p.cpu().numpy(), sd[n], f"{n} after unload_adapter")
    # the merged checkpoint of the trained model stands alone
    tr.model.save_pretrained(str(tmp_path / "merged"))
    merged = M.from_pretrained(str(tmp_path / "merged"), precision=precision).to("cuda")
    TF.same_bits(merged.compute_logits(x).cpu().numpy(), trained, "logits of the merged checkpoint")


def test_cli_trains_an_adapter_and_the_evaluator_loads_it(tmp_path):
    """tools/train.py --lora_rank 4 in a fresh child process under a time limit writes adapter/ beside the merged checkpoint;
    tools/evaluate.py --adapter serves it on the base model."""
    data, cfgm = pkg("data"), pkg("config")
    g = np.random.default_rng(0)
    for split in ("train", "val"):
        data.write_token_dataset(tmp_path / split, g.integers(0, 262144, (1000, 4, 4)), np.zeros(1000, np.int32), hz=30)
    cfg = cfgm.GenieConfig(num_layers=1, num_heads=2, d_model=64, T=16, S=16, num_factored_vocabs=2, qk_norm=False, num_prompt_frames=8)
    base = pkg("st_mask_git").STMaskGIT(cfg, precision="exact").load_numpy_state_dict(pkg("synthetic").make_state_dict(cfg, seed=3))
    base.save_pretrained(str(tmp_path / "base"))
    cfg.save_pretrained(tmp_path / "cfg.json")
    out = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tools", "train.py"), "--genie_config", str(tmp_path / "cfg.json"),
           "--train_data_dir", str(tmp_path / "train"), "--val_data_dir", str(tmp_path / "val"), "--window_size", "16", "--stride", "15",
           "--warmstart_path", str(tmp_path / "base"), "--output_dir", str(out), "--per_device_train_batch_size", "2",
           "--per_device_eval_batch_size", "2", "--max_train_steps", "2", "--eval_every_n_steps", "2", "--seed", "1", "--precision", "exact",
           "--lora_rank", "4", "--learning_rate", "1e-2"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "step 2: train_loss" in res.stdout and "training 12 of" in res.stdout
    ck = out / "final_checkpt"
    assert sorted(os.listdir(ck / "adapter")) == ["adapter.safetensors", "adapter_config.json"]
    ac = json.load(open(ck / "adapter" / "adapter_config.json"))
    assert ac["rank"] == 4 and ac["alpha"] == 8.0 and len(ac["targets"]) == 6 and ac["base"]["d_model"] == 64
    assert os.path.exists(ck / "model.safetensors") and os.path.exists(ck / "trainer_state.pt")
    ev = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tools", "evaluate.py"), "--checkpoint_dir", str(tmp_path / "base"),
          "--val_data_dir", str(tmp_path / "val"), "--adapter", str(ck / "adapter"), "--batch_size", "2", "--max_examples", "2", "--precision", "exact"]
    res = subprocess.run(ev, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "adapter" in res.stdout and "merged" in res.stdout
    res = subprocess.run(ev[:ev.index("--adapter")] + ["--adapter", str(tmp_path / "train")] + ev[ev.index("--adapter") + 2:], capture_output=True,
                         text=True)
    assert res.returncode != 0 and "evaluate.py: --adapter" in res.stderr
