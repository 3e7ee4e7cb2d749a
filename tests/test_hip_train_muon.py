"""Muon on the HIP path (include/genie_hip.h, "Muon"; csrc/kernels_muon.hip; GenieTrainer(muon=MuonConfig(...))).

The yardstick is not the code under test: the float64 restatement of tests/muon_model.py.  The bar of a kernel whose summation order
differs from NumPy's: its relative Frobenius distance from float64 is at most 4 x the float32 restatement's own distance on the same input,
and under 1e-3 in every case.  The AdamW side of a Muon trainer is compared bit for bit with a trainer without Muon.  Needs an MI355X:
``-m gpu``; tests/test_train_muon_cpu.py holds what runs anywhere."""
import functools
import warnings

import numpy as np
import pytest

import muon_model as MM
import test_hip_train_frozen as TF
from conftest import pkg, record_measure
from stale_memory import poison_tensor

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS_SHAPES = [(16, 16), (16, 48), (48, 16), (64, 64), (80, 48), (32, 128), (144, 144)]   # the last: past one tile, no tile multiple
KINDS = ["gaussian", "lowrank"]
COEF = MM.DEFAULT_COEFFICIENTS


def stream():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def ns_input(shape, kind):
    """(3, rows, cols) f32: two matrices of `kind` around an all-zero one.  Computed once, never written to."""
    g = np.random.default_rng(977 * shape[0] + shape[1] + (0 if kind == "gaussian" else 5))
    def one():
        if kind == "gaussian":
            return g.standard_normal(shape)
        return g.standard_normal((shape[0], 4)) @ g.standard_normal((4, shape[1])) + 1e-3 * g.standard_normal(shape)
    x = np.stack([one(), np.zeros(shape), one()]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ns_reference(shape, kind):
    """[(float64 result, the float32 restatement's distance from it)] per matrix of ns_input."""
    out = []
    for m in ns_input(shape, kind):
        want = MM.newton_schulz(m.astype(np.float64), 5, COEF, 1e-7)
        d32 = rel(MM.newton_schulz(m, 5, COEF, 1e-7, dtype=np.float32), want) if m.any() else 0.0
        out.append((want, d32))
    return out


def newton_schulz(x, steps=5, poison=None, in_place=False, eps=1e-7):
    """genie_newton_schulz on a (batch, rows, cols) f32 array; the workspace starts as zeros or as `poison` bytes."""
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    batch, rows, cols = x.shape
    items = (lib_mod.MuonItem * batch)(*[lib_mod.MuonItem(rows=rows, cols=cols) for _ in range(batch)])
    need = lib.genie_muon_workspace_bytes(items, batch)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    if poison is not None:
        poison_tensor(ws, poison)
    src = TF.dev(x)
    dst = src if in_place else TF.dev(np.full_like(x, np.nan))
    lib_mod.check(lib.genie_newton_schulz(src.data_ptr(), dst.data_ptr(), rows, cols, batch, steps, *COEF, eps, ws.data_ptr(), need, stream()),
                  "genie_newton_schulz")
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), x), "the input was written"
    return dst.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1: the iteration against float64
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", NS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_newton_schulz_against_float64(shape, kind):
    got = newton_schulz(ns_input(shape, kind))
    assert not got[1].any(), "an all-zero matrix must come out all zero"
    for i in (0, 2):
        want, d32 = ns_reference(shape, kind)[i]
        d = rel(got[i], want)
        print(f"newton_schulz {shape} {kind} [{i}]: {d:.3e} from float64, the float32 restatement {d32:.3e}, ratio {d / d32:.2f}")
        record_measure(f"muon_ns_ratio_{shape[0]}x{shape[1]}_{kind}_{i}", d / d32)
        assert d <= 4 * d32 and d < 1e-3, (shape, kind, i, d, d32)


def test_newton_schulz_zero_steps_is_the_normalisation_and_in_place_works():
    x = ns_input((80, 48), "gaussian")
    got = newton_schulz(x, steps=0)
    for i in (0, 2):
        want = x[i].astype(np.float64) / np.linalg.norm(x[i].astype(np.float64))
        assert np.max(np.abs(got[i] - want)) <= 2.0 ** -22 * np.max(np.abs(want))   # the f32 norm and one f32 division
    assert not got[1].any()
    TF.same_bits(newton_schulz(x, in_place=True), newton_schulz(x), "in == out")
    TF.same_bits(newton_schulz(x, steps=0, in_place=True), got, "in == out, no steps")


# ---------------------------------------------------------------------------------------------- 2: determinism and isolation
@pytest.mark.parametrize("shape", [(48, 16), (144, 144), (32, 128)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_run_to_run_alone_or_in_a_full_table_and_over_a_poisoned_workspace(shape):
    x = ns_input(shape, "lowrank")
    first = newton_schulz(x)
    TF.same_bits(newton_schulz(x), first, "second call")
    for byte in (0xFF, 0x3C):
        TF.same_bits(newton_schulz(x, poison=byte), first, f"workspace poisoned with {byte:#x}")
    TF.same_bits(newton_schulz(x[2:3]), first[2:3], "the item alone")
    n = pkg("_lib").MUON_MAX_ITEMS
    g = np.random.default_rng(5)
    full = g.standard_normal((n,) + shape).astype(np.float32)
    full[n - 2] = x[2]
    TF.same_bits(newton_schulz(full, poison=0xFF)[n - 2], first[2], "the item inside a full table")


# ---------------------------------------------------------------------------------------------- the step on caller buffers
class Table:
    """Device buffers of a genie_muon_step call over `shapes` [(rows, cols)] and the call itself."""

    def __init__(self, shapes, lr=0.01, wd=0.1, ema=False, zero_grad=(), seed=0):
        M, self.lib_mod = pkg("muon"), pkg("_lib")
        self.lib = self.lib_mod.load()
        g = np.random.default_rng(seed)
        f = lambda s: g.standard_normal(s).astype(np.float32)   # noqa: E731
        self.host = [dict(w=f(s), g=np.zeros(s, np.float32) if i in zero_grad else f(s), b=np.zeros(s, np.float32) if i in zero_grad else f(s),
                          e=f(s)) for i, s in enumerate(shapes)]
        self.devs = [{k: TF.dev(v) for k, v in h.items()} for h in self.host]
        self.items = [M.item(s[0], s[1], d["w"].data_ptr(), d["g"].data_ptr(), d["b"].data_ptr(), d["e"].data_ptr() if ema else None, lr, wd)
                      for s, d in zip(shapes, self.devs)]
        self.arr, self.n = M.table(self.items)
        self.need = self.lib.genie_muon_workspace_bytes(self.arr, self.n)
        assert self.need > 0
        self.ws = torch.full((self.need,), 0x5A, dtype=torch.uint8, device="cuda")

    def step(self, settings, arr=None, n=None, ws_ptr=None, ws_bytes=None):
        rc = self.lib.genie_muon_step(self.arr if arr is None else arr, self.n if n is None else n, settings,
                                      self.ws.data_ptr() if ws_ptr is None else ws_ptr, self.need if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        return [{k: v.cpu().numpy() for k, v in d.items()} for d in self.devs]

    def untouched(self):
        return (all(np.array_equal(now[k], h[k]) for now, h in zip(self.read(), self.host) for k in h)
                and bool((self.ws == 0x5A).all()))


MIXED = [(32, 48), (64, 64), (48, 32), (64, 64), (144, 144), (32, 48), (16, 16)]


def check_table(tb, cfg, omd=None, coef=1.0, what=""):
    """Every item of a stepped table against the float64 restatement, by the kernel bar on O; B by its three f32 operations."""
    for i, (h, now) in enumerate(zip(tb.host, tb.read())):
        it = tb.items[i]
        kw = dict(mu=cfg.momentum, nesterov=cfg.nesterov, steps=cfg.ns_steps, coefficients=cfg.ns_coefficients, eps=cfg.eps,
                  adjust_lr=cfg.adjust_lr)
        want, b, o = MM.muon_matrix(h["w"], h["g"], h["b"], it.lr, it.weight_decay, coef, **kw)
        _, _, o32 = MM.muon_matrix(h["w"], h["g"], h["b"], it.lr, it.weight_decay, coef, dtype=np.float32, **kw)
        assert np.array_equal(now["g"], h["g"])
        assert np.max(np.abs(now["b"] - b)) <= 3 * 2.0 ** -24 * np.max(np.abs(b)) + 1e-30, (what, i)
        check_update(now["w"], h["w"], o, o32, it.lr, it.weight_decay, cfg.adjust_lr, f"{what} item {i}")
        if omd is not None:
            e = MM.ema_line(h["e"], now["w"], np.float32(omd), dtype=np.float32)   # the line itself is exact f32: from the W the kernel wrote
            TF.same_bits(now["e"], e, f"{what} item {i} ema")


def check_update(w_new, w_old, o, o32, lr, wd, adjust_lr, what):
    """The kernel bar scaled by lr * adj: with s = lr adj, ||W_old (1 - lr wd) - W_new - s O||_F <= 4 d32 ||s O||_F, d32 the float32
    restatement's own relative distance, plus the f32 roundings of W itself (of W_old * decay, of s * O and of the difference: 2^-24 of
    each in norm).  Under 1e-3 ||s O|| in every case."""
    rows, cols = o.shape
    s = lr * MM.adjust(adjust_lr, rows, cols)
    upd = np.asarray(w_old, np.float64) * (1.0 - lr * wd) - np.asarray(w_new, np.float64)
    nso = np.linalg.norm(s * o)
    if nso == 0.0:
        TF.same_bits(w_new, (w_old * np.float32(1.0 - lr * wd)).astype(np.float32), what + " (zero update)")
        return
    d32 = rel(o32, o)
    rounding = 2.0 ** -24 * (np.linalg.norm(w_old) + np.linalg.norm(w_new) + nso)
    err = np.linalg.norm(upd - s * o)
    print(f"{what}: update error {err / nso:.3e} of ||s O||, the float32 restatement {d32:.3e}, W's own rounding {rounding / nso:.3e}")
    assert err <= 4 * d32 * nso + rounding and err < 1e-3 * nso + rounding, (what, err / nso, d32, rounding / nso)


@pytest.mark.parametrize("adjust,nesterov,steps", [("match_rms_adamw", True, 5), ("original", False, 4), ("match_rms_adamw", True, 0)])
def test_step_on_a_mixed_table(adjust, nesterov, steps):
    """Seven items of five shapes in one call (wide, tall, square, repeated shapes apart from each other), with an EMA."""
    M = pkg("muon")
    cfg = M.MuonConfig(adjust_lr=adjust, nesterov=nesterov, ns_steps=steps)
    tb = Table(MIXED, ema=True)
    assert tb.step(M.settings(cfg, ema_one_minus_decay=0.25)) == 0
    check_table(tb, cfg, omd=0.25, what=f"mixed {adjust}")
    # an item alone gives the bits it gives inside the table
    alone = Table(MIXED, ema=True)
    arr, n = M.table(alone.items[3:4])
    assert alone.step(M.settings(cfg, ema_one_minus_decay=0.25), arr=arr, n=n) == 0
    for k in ("w", "b", "e"):
        TF.same_bits(alone.read()[3][k], tb.read()[3][k], f"item 3 alone, {k}")


def test_step_applies_the_global_clip_coefficient():
    M = pkg("muon")
    cfg = M.MuonConfig()
    tb = Table([(32, 48), (48, 32)])
    ss = torch.tensor([400.0], dtype=torch.float64, device="cuda")   # norm 20 * grad_mult 0.5 = 10 against max_norm 1: coef = 0.5 * 0.1
    assert tb.step(M.settings(cfg, grad_mult=0.5, grad_sumsq=ss.data_ptr(), max_grad_norm=1.0)) == 0
    check_table(tb, cfg, coef=float(MM.clip_coef(400.0, 0.5, 1.0, np.float32)), what="clipped")


def test_zero_gradient_leaves_only_the_decay():
    M = pkg("muon")
    tb = Table([(32, 48), (64, 64), (48, 32)], lr=0.01, wd=0.1, zero_grad=(1,))
    assert tb.step(M.settings(M.MuonConfig())) == 0
    now = tb.read()[1]
    TF.same_bits(now["w"], tb.host[1]["w"] * np.float32(1.0 - 0.01 * 0.1), "zero gradient: W * (1 - lr wd)")
    assert not now["b"].any()
    assert not np.array_equal(tb.read()[0]["w"], tb.host[0]["w"])


# ---------------------------------------------------------------------------------------------- 3: refusals
def test_a_refused_table_leaves_every_buffer_untouched():
    M, lib_mod = pkg("muon"), pkg("_lib")
    tb = Table([(32, 48), (64, 64)], ema=True)
    s = M.settings(M.MuonConfig(), ema_one_minus_decay=0.1)
    E = lib_mod.E_ARG
    bad_rows = M.table([tb.items[0], M.item(24, 64, *(getattr(tb.items[1], k) for k in ("param", "grad", "momentum", "ema")), 0.01, 0.1)])
    assert tb.step(s, *bad_rows) == E and tb.untouched()
    off = M.table([tb.items[0], M.item(64, 64, tb.items[1].param + 4, tb.items[1].grad, tb.items[1].momentum, tb.items[1].ema, 0.01, 0.1)])
    assert tb.step(s, *off) == E and tb.untouched()
    assert tb.step(s, n=0) == E and tb.untouched()
    big = (lib_mod.MuonItem * (lib_mod.MUON_MAX_ITEMS + 1))(*([tb.items[0]] * (lib_mod.MUON_MAX_ITEMS + 1)))
    assert tb.step(s, arr=big, n=lib_mod.MUON_MAX_ITEMS + 1) == E and tb.untouched()
    assert tb.step(s, ws_bytes=tb.need - 16) == E and tb.untouched()
    assert tb.step(s, ws_ptr=tb.ws.data_ptr() + 4) == E and tb.untouched()
    assert tb.step(s) == 0 and not tb.untouched()   # and the table itself runs


# ---------------------------------------------------------------------------------------------- 4: the trainer's step
KW = dict(lr=3e-3, weight_decay=0.01, max_grad_norm=1.0)


def muon_trainer(shape, precision, muon=None, **kw):
    cfg, sd, _, _ = TF.case(shape)
    M = pkg("muon")
    return TF.make_trainer(cfg, sd, precision, muon=M.MuonConfig() if muon is None else muon, **dict(KW, **kw))


class Restated(MM.MixedOptimizer):
    """MixedOptimizer that also keeps each step's O per Muon tensor (from the state it has before the step)."""

    def step(self, grads, grad_mult=1.0):
        sumsq = float(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in grads.values()))
        coef = MM.clip_coef(sumsq, grad_mult, self.max_norm or 0.0, self.t)
        self.last_o = {}
        for n in self.muon_names:
            o = np.zeros(self.p[n].shape, self.t)
            for r0, rows in MM.blocks(n, o.shape):
                sl = slice(r0, r0 + rows)
                u, _ = MM.momentum_update(grads[n][sl], self.m[n][sl], coef, self.kw["mu"], self.kw["nesterov"], self.t)
                o[sl] = MM.newton_schulz(u, self.kw["steps"], self.kw["coefficients"], self.kw["eps"], self.t)
            self.last_o[n] = o
        return super().step(grads, grad_mult)


def restatement(tr, before, dtype):
    """The trainer's optimizer restated over its weights `before`."""
    m = tr.muon
    return Restated(before, tr.muon_names, tr.base_lr, tr.weight_decay, tr.max_grad_norm, pkg("train").decays, tr.layout.lr_factor,
                    m.momentum, m.nesterov, m.ns_steps, m.ns_coefficients, m.eps, m.adjust_lr, dtype=dtype)


def check_muon_tensors(tr, opt64, opt32, before, after, what):
    """Every Muon matrix of the trainer against the restatement's O of this step (the restatements were stepped already)."""
    T = pkg("train")
    for n in tr.muon_names:
        lr, wd = tr.base_lr * tr.layout.lr_factor[n], tr.weight_decay if T.decays(n) else 0.0
        for r0, rows in MM.blocks(n, before[n].shape):
            sl = slice(r0, r0 + rows)
            check_update(after[n][sl], before[n][sl], opt64.last_o[n][sl], opt32.last_o[n][sl], lr, wd, tr.muon.adjust_lr, f"{what} {n}[{r0}:]")


@pytest.mark.parametrize("precision", ["exact", "bf16"])
@pytest.mark.parametrize("shape", TF.FIXTURES)
def test_trainer_steps_against_the_restatement_and_the_adamw_trainer(shape, precision):
    """d_model 64, 2 layers, S 16, T 4, LN and qk-norm: two steps, each from one forward_backward whose gradients go to the host before
    optimizer_step.  Muon tensors by the kernel bar scaled by lr * adj; after step 1 every other tensor holds the bits of a trainer without
    Muon (same initial weights, same batch); after step 2 they follow the float64 AdamW of the restatement, which carries its own
    momentum and moments and takes the trainer's weights at the start of each step (so no drift between the two is accumulated)."""
    cfg, sd, _, _ = TF.case(shape)
    batch = TF.batch_of(shape)
    tr = muon_trainer(shape, precision)
    assert len(tr.muon_names) == 6 * cfg.num_layers and len(tr.muon_items) == 10 * cfg.num_layers
    assert tr.muon_launches() == 3 + 15 * len({(it.rows, it.cols) for it in tr.muon_items})
    plain = TF.make_trainer(cfg, sd, precision, **KW)
    before = TF.params_of(tr)
    opt64, opt32 = restatement(tr, before, np.float64), restatement(tr, before, np.float32)
    for step in (1, 2):
        tr.forward_backward(batch["input_ids"], batch["labels"])
        grads = TF.grads_of(tr)
        norm, _ = tr.optimizer_step()
        after = TF.params_of(tr)
        want_norm = opt64.step(grads)
        opt32.step(grads)
        assert abs(float(norm) - want_norm) <= 1e-6 * want_norm
        check_muon_tensors(tr, opt64, opt32, before, after, f"{shape} {precision} step {step}")
        if step == 1:
            plain.train_step(batch)
            theirs = TF.params_of(plain)
        for n in after:
            if n in tr.muon_names:
                continue
            if step == 1:
                TF.same_bits(after[n], theirs[n], f"{n}: the AdamW side of a Muon trainer")
            # AdamW's few f32 operations on W and on an update of at most a few lr
            assert np.max(np.abs(after[n] - opt64.p[n])) <= 2.0 ** -22 * (np.abs(after[n]).max() + 4 * tr.base_lr), (n, step)
        # the momentum lives in exp_avg, exp_avg_sq stays zero
        for n in tr.muon_names:
            lo, hi = tr.offsets[n]
            assert not bool(tr.exp_avg_sq[lo:hi].any())
            mom = tr.exp_avg[lo:hi].cpu().numpy().reshape(before[n].shape)
            assert np.max(np.abs(mom - opt64.m[n])) <= 8 * 2.0 ** -24 * np.max(np.abs(opt64.m[n])), n
        before = after
        for o in (opt64, opt32):
            o.p = {n: np.asarray(v, o.t).copy() for n, v in after.items()}


# ---------------------------------------------------------------------------------------------- 5: trainer features
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_ema_of_muon_tensors_is_the_restated_line(precision):
    T = pkg("train")
    tr = muon_trainer("train_tiny_ln", precision, ema_decay=0.9)
    batch = TF.batch_of("train_tiny_ln")
    ema0 = {n: tr.ema[lo:hi].cpu().numpy() for n, (lo, hi) in tr.offsets.items() if n in tr.g_views}
    tr.train_step(batch)
    omd = np.float32(T.ema_one_minus_decay(0.9, 1))
    after = TF.params_of(tr)
    for n in tr.trainable:
        lo, hi = tr.offsets[n]
        want = MM.ema_line(ema0[n], after[n].reshape(-1), omd, dtype=np.float32)
        TF.same_bits(tr.ema[lo:hi].cpu().numpy(), want, f"ema of {n}")
        assert n not in tr.muon_names or not np.array_equal(want, ema0[n]), n


def test_a_frozen_target_is_untouched_and_costs_no_state():
    cfg, sd, _, _ = TF.case("train_tiny_ln")
    sel = "decoder.layers.1.*,out_x_proj.*"
    tr = muon_trainer("train_tiny_ln", "exact", trainable=sel)
    plain = TF.make_trainer(cfg, sd, "exact", trainable=sel, **KW)
    assert tr.n_train == plain.n_train and tr.exp_avg.numel() == plain.exp_avg.numel() and tr.offsets == plain.offsets
    assert tr.muon_names == [n for n in pkg("muon").select_targets(cfg, ["decoder.layers.*"]) if n.startswith("decoder.layers.1.")]
    before = TF.params_of(tr)
    tr.train_step(TF.batch_of("train_tiny_ln"))
    after = TF.params_of(tr)
    for n in after:
        if n.startswith("decoder.layers.0."):
            TF.same_bits(after[n], before[n], f"frozen {n}")
    assert all(not np.array_equal(after[n], before[n]) for n in tr.muon_names)


def test_lr_scale_multiplies_the_muon_learning_rate():
    """Two trainers on the same weights and batch, one with lr_scale 2 on the MLP weights and no decay: its update of those tensors is
    twice the other's (s = float(lr * factor * adj); W - s O in f32), the other Muon tensors hold the same bits."""
    a = muon_trainer("train_tiny_ln", "exact", weight_decay=0.0)
    b = muon_trainer("train_tiny_ln", "exact", weight_decay=0.0, lr_scale={"*.mlp.fc?.weight": 2.0})
    before = TF.params_of(a)
    batch = TF.batch_of("train_tiny_ln")
    a.train_step(batch)
    b.train_step(batch)
    pa, pb = TF.params_of(a), TF.params_of(b)
    for n in a.muon_names:
        if ".mlp." in n:
            da, db = pa[n].astype(np.float64) - before[n], pb[n].astype(np.float64) - before[n]
            assert np.max(np.abs(db - 2 * da)) <= 3 * 2.0 ** -24 * np.max(np.abs(before[n])), n
            assert np.linalg.norm(da) > 0
        else:
            TF.same_bits(pa[n], pb[n], n)


def test_lora_on_spatial_attention_and_muon_on_the_rest():
    T = pkg("train")
    cfg, sd, _, _ = TF.case("train_tiny_ln")
    tr = muon_trainer("train_tiny_ln", "exact", lora=T.LoraConfig(rank=4, alpha=8.0, targets="*.spatial_attn.*"),
                      trainable="*.temporal_attn.*.weight,*.mlp.fc?.weight")
    assert all(".spatial_attn." not in n for n in tr.muon_names) and len(tr.muon_names) == 4 * cfg.num_layers
    w0 = {n: v.clone() for n, v in tr.w0.items()}
    before = TF.params_of(tr)
    ad0 = {n: v.clone() for n, v in tr.adapter_state_dict().items()}
    batch = TF.batch_of("train_tiny_ln")
    tr.train_step(batch)
    tr.train_step(batch)   # B starts at zero: dA is zero in the first step
    after = TF.params_of(tr)
    assert all(torch.equal(tr.w0[n], w0[n]) for n in w0)
    assert all(not np.array_equal(after[n], before[n]) for n in tr.muon_names)
    assert all(not torch.equal(v, ad0[n]) for n, v in tr.adapter_state_dict().items())
    assert all(not np.array_equal(after[n], before[n]) for n in w0)   # the merged weights follow the adapters


def test_muon_targets_that_select_nothing_trainable_raise():
    M = pkg("muon")
    with pytest.raises(ValueError, match="no trainable tensor is left for Muon"):
        muon_trainer("train_tiny_ln", "exact", trainable="*.bias,out_x_proj.*")
    with pytest.raises(ValueError, match="no trainable tensor is left for Muon"):
        muon_trainer("train_tiny_ln", "exact", muon=M.MuonConfig(targets="out_x_proj.weight"), trainable="decoder.layers.*")
    with pytest.raises(ValueError, match="matches no Linear weight"):
        muon_trainer("train_tiny_ln", "exact", muon=M.MuonConfig(targets="decoder.layers.9.*"))
    with pytest.raises(TypeError):
        muon_trainer("train_tiny_ln", "exact", muon=dict(momentum=0.9))
    tr = muon_trainer("train_tiny_ln", "exact", muon=M.MuonConfig(targets="out_x_proj.weight,*.mlp.*"))   # the readout is eligible
    assert "out_x_proj.weight" in tr.muon_names and len(tr.muon_names) == 1 + 2 * tr.config.num_layers
    tr.train_step(TF.batch_of("train_tiny_ln"))


# ---------------------------------------------------------------------------------------------- 6: resume, overfit
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_resume_is_bit_equal_and_the_other_optimizers_state_is_refused(precision):
    M = pkg("muon")
    cfg, sd, _, _ = TF.case("train_tiny_qknorm")
    batch = TF.batch_of("train_tiny_qknorm")
    a = muon_trainer("train_tiny_qknorm", precision, ema_decay=0.9)
    a.train_step(batch)
    state = a.state_dict()
    assert state["muon"] == dict(M.MuonConfig().settings_dict(), names=a.muon_names)
    b = TF.twin_from(a, precision, muon=M.MuonConfig(), ema_decay=0.9, **KW)
    a.train_step(batch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b.load_state_dict(state)
    b.train_step(batch)
    want = TF.params_of(a)
    for n, p in TF.params_of(b).items():
        TF.same_bits(p, want[n], f"{n} after the resumed step")
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq) and torch.equal(b.ema, a.ema)
    plain = TF.twin_from(a, precision, **KW)
    with pytest.raises(ValueError, match="AdamW alone"):
        b.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="Muon settings"):
        plain.load_state_dict(state)
    other = TF.twin_from(a, precision, muon=M.MuonConfig(ns_steps=4), **KW)
    with pytest.raises(ValueError, match="Muon settings"):
        other.load_state_dict(state)
    assert "muon" not in plain.state_dict()


def test_twenty_steps_on_one_batch_lower_the_loss():
    """A sanity condition, not a convergence claim."""
    tr = muon_trainer("train_tiny_ln", "exact", lr=1e-3)
    batch = TF.batch_of("train_tiny_ln")
    losses = [float(tr.train_step(batch)["loss"]) for _ in range(20)]
    after, _ = tr.forward_backward(batch["input_ids"], batch["labels"])
    print(f"overfit: loss {losses[0]:.4f} -> {float(after):.4f}")
    assert np.all(np.isfinite(losses)) and float(after) < losses[0]
