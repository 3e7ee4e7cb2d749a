"""Training with an EMA of the weights (include/genie_hip.h, "EMA of the weights"; csrc/kernels_train.hip): genie_ema_update against the
NumPy f32 restatement (tests/ema_model.py) and against what the reference's LitEma wrote (tests/golden/ema_litema.npz); the fused
genie_adamw_ema_step against genie_adamw_step (parameters, moments) and genie_ema_update (average); genie_swap_f32; the refusals; and
GenieTrainer -- the average does not perturb training, is the contract's, ema_scope(), resume, and the CLI.

No test holds the fused step to itself: the yardsticks are genie_adamw_step, the NumPy restatement and the reference-written fixture.

(H, d, T, S, B, qk_norm, use_mup, layers) of the trainer cases, built as in tests/test_hip_train_dropout.py:
  ln3     (2, 64, 4, 16, 2, F, F, 3)     LayerNorm blocks
  qk3     (2, 128, 8, 16, 3, T, F, 3)    Identity norms, odd batch
  qk32    (2, 64, 4, 16, 2, T, F, 2)     qk-norm weights of 32 floats: the only case whose flat buffers have padding (the first two have none)

The GPU tests need an MI355X (``-m gpu``); tests/test_train_ema_cpu.py holds what runs anywhere.
"""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import ema_model as EM
from conftest import REPO, pkg
from oracle import genie_train_oracle as TO

CASES = {
    "ln3": (2, 64, 4, 16, 2, False, False, 3),
    "qk3": (2, 128, 8, 16, 3, True, False, 3),
    "qk32": (2, 64, 4, 16, 2, True, False, 2),
}
STEP_CASES = ["ln3", "qk3"]
PRECISIONS = ["exact", "f16x3", "bf16"]
# not multiples of four, more than one workgroup; the last is past one pass of the capped grid (2048 workgroups x 256 threads x 4 floats),
# so the grid-stride loops run a second time
SIZES = [1, 3, 5, 64, 1027, 4097, 2 * 64 * 256 + 2, 2048 * 256 * 4 + 1027]
OFFSETS = [0, 1]          # floats between a 256-byte aligned address and each base pointer: 1 = the one-element path for the whole range
GUARD = 1024              # guard floats on either side
CONFIGS = {"d999": (0.999, False), "d999w": (0.999, True), "d9": (0.9, False), "d9w": (0.9, True)}
STEPS = 4
TRAIN_KW = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)


def torch_():
    return pytest.importorskip("torch")


def libs():
    lib = pkg("_lib")
    return lib, lib.load()


def stream():
    return torch_().cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "of", g.size, "words differ; first at", int(np.argmax(g != w)))


class Guarded:
    """A device copy of `values` `off` floats past a 256-byte aligned address, between two guard regions of 0x5A bytes."""

    def __init__(self, values, off=0):
        torch = torch_()
        values = np.ascontiguousarray(values, np.float32)
        self.n, self.off = values.size, off
        self.buf = torch.full((4 * (2 * GUARD + self.n + off),), 0x5A, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.f = self.buf.view(torch.float32)
        self.lo = GUARD + off
        self.f[self.lo:self.lo + self.n].copy_(torch.from_numpy(values))
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def read(self):
        """The values, after checking that both guard regions still hold 0x5A."""
        raw = self.buf.cpu().numpy()
        lo, hi = 4 * self.lo, 4 * (self.lo + self.n)
        assert (raw[:lo] == 0x5A).all() and (raw[hi:] == 0x5A).all(), "the kernel wrote outside its range"
        return raw[lo:hi].view(np.float32).copy()


def values(n, seed, scale=1.0):
    """f32 values with zeros, values near 1e-38 (differences and products in the denormal range) and large ones among them."""
    g = np.random.default_rng(seed)
    x = (scale * g.standard_normal(n)).astype(np.float32)
    k = np.arange(n)
    x[k % 11 == 3] = 0.0
    x[k % 13 == 5] = (1e-38 * (1 + g.random(n))).astype(np.float32)[k % 13 == 5]
    x[k % 17 == 7] *= np.float32(1e20)
    return x


# ---------------------------------------------------------------------------------------------- genie_ema_update
@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_is_the_restatement(n, off):
    """genie_ema_update against ema_model.update, bit for bit, at omd 0.001, 0, 1 and a warm-up value; guards untouched; a second launch
    from the same inputs gives the same bits.  off = 1 misaligns both pointers; at n = 1027 a case with only `params` misaligned rides along."""
    torch = torch_()
    lib, L = libs()
    e0, p = values(n, 1 + n), values(n, 2 + n)
    p[::7] = e0[::7]                      # elements that do not move
    for omd in (np.float32(0.001), np.float32(0), np.float32(1), EM.one_minus_decay(0.999, 2, True)):
        for off_e, off_p in {(off, off), (0, off)} if n == 1027 else {(off, off)}:
            outs = []
            for _ in range(2):
                e, pp = Guarded(e0, off_e), Guarded(p, off_p)
                lib.check(L.genie_ema_update(e.ptr, pp.ptr, n, float(omd), stream()), "genie_ema_update")
                torch.cuda.synchronize()
                outs.append(e.read())
                assert_bits(pp.read(), p, "params are read only")
            assert_bits(outs[0], EM.update(e0, p, omd), f"ema n={n} omd={omd} off=({off_e},{off_p})")
            assert_bits(outs[1], outs[0], "two launches")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_ema_update_is_litema(tag):
    """The kernel fed the fixture's parameter sequence lands on LitEma's shadow after every one of the 12 updates, on all three tensors
    (5, 130 and 1027 elements; zeros, denormal-range differences, a tensor that does not move), with omd from the trainer's schedule."""
    torch = torch_()
    lib, L = libs()
    T = pkg("train")
    g = np.load(os.path.join(REPO, "tests", "golden", "ema_litema.npz"))
    decay, warm = CONFIGS[tag]
    for k in range(3):
        seq = g[f"p{k}"]
        e = Guarded(seq[0])
        for u in range(1, seq.shape[0]):
            p = Guarded(seq[u])
            lib.check(L.genie_ema_update(e.ptr, p.ptr, e.n, T.ema_one_minus_decay(decay, u, warm), stream()), "genie_ema_update")
            torch.cuda.synchronize()
            assert_bits(e.read(), g[f"{tag}_s{k}"][u - 1], f"{tag} tensor {k} update {u}")


# ---------------------------------------------------------------------------------------------- genie_adamw_ema_step
# (step, weight_decay, clip: None = no grad_sumsq / "above" / "below" max_grad_norm, grad_mult, omd)
SETTINGS = [(1, 0.0, None, 1.0, 0.001), (1000, 0.01, "above", 1.0, 0.001), (1, 0.01, "below", 1.0 / 6, 1.0), (1000, 0.0, "above", 1.0 / 6, 0.0),
            (1000, 0.01, None, 1.0 / 6, 0.001)]


@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_adamw_ema_step_is_adamw_then_ema(n, off):
    """p, m, v of the fused step are the bits genie_adamw_step writes from copies of the same inputs, and `ema` is genie_ema_update -- and
    the restatement -- applied to that new p: over step 1 / 1000, weight decay 0 / 0.01, clipping off / norm above / norm below
    max_grad_norm, grad_mult 1 / 1/6, omd 0 / 1 / 0.001.  Guards untouched; the gradient is read only."""
    torch = torch_()
    lib, L = libs()
    rng = np.random.default_rng(n)
    p0, g0, e0 = values(n, 3 + n, 0.1), (0.01 * rng.standard_normal(n)).astype(np.float32), values(n, 4 + n, 0.1)
    m0 = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v0 = (1e-4 * rng.random(n)).astype(np.float32)
    g0[::9] = 0.0
    adam = (1e-3, 0.9, 0.999, 1e-8)
    st = stream()
    for step, wd, clip, mult, omd in SETTINGS:
        max_norm = 1.0 if clip else 0.0
        norm = {None: 1.0, "above": 40.0, "below": 0.5}[clip] / mult          # the norm after grad_mult is 40 or 0.5 against 1.0
        ss = torch.tensor([norm * norm], dtype=torch.float64, device="cuda")
        tail = (*adam, wd, step, mult, ss.data_ptr() if clip else None, max_norm)
        ref = [Guarded(a, off) for a in (p0, g0, m0, v0)]
        lib.check(L.genie_adamw_step(*(r.ptr for r in ref), n, *tail, st), "genie_adamw_step")
        e_ref = Guarded(e0, off)
        lib.check(L.genie_ema_update(e_ref.ptr, ref[0].ptr, n, omd, st), "genie_ema_update")
        fused = [Guarded(a, off) for a in (p0, g0, m0, v0, e0)]
        lib.check(L.genie_adamw_ema_step(*(f.ptr for f in fused[:4]), fused[4].ptr, n, *tail, omd, st), "genie_adamw_ema_step")
        torch.cuda.synchronize()
        p1, g1, m1, v1 = (r.read() for r in ref)
        what = f"n={n} off={off} step={step} wd={wd} clip={clip} mult={mult:.3f} omd={omd}"
        assert not np.array_equal(p1, p0) and np.isfinite(p1).all(), what
        for name, got, want in zip("pgmv", (f.read() for f in fused[:4]), (p1, g1, m1, v1)):
            assert_bits(got, want, f"{name}: {what}")
        assert_bits(g1, g0, "the gradient is read only")
        ema = fused[4].read()
        assert_bits(ema, e_ref.read(), f"ema against genie_ema_update: {what}")
        assert_bits(ema, EM.update(e0, p1, omd), f"ema against the restatement: {what}")


@pytest.mark.gpu
def test_adamw_ema_step_settings_are_distinct():
    """The setting axes of the test above change the update (a yardstick that ignored one would let the fused kernel ignore it too)."""
    torch = torch_()
    lib, L = libs()
    n = 1027
    p0, g0 = values(n, 21, 0.1), (0.01 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    outs = []
    for step, wd, clip, mult, _ in SETTINGS:
        bufs = [Guarded(a) for a in (p0, g0, np.zeros(n, np.float32), np.zeros(n, np.float32))]
        norm = {None: 1.0, "above": 40.0, "below": 0.5}[clip] / mult
        ss = torch.tensor([norm * norm], dtype=torch.float64, device="cuda")
        lib.check(L.genie_adamw_step(*(b.ptr for b in bufs), n, 1e-3, 0.9, 0.999, 1e-8, wd, step, mult, ss.data_ptr() if clip else None,
                                     1.0 if clip else 0.0, stream()), "genie_adamw_step")
        torch.cuda.synchronize()
        outs.append(bufs[0].read())
    for i in range(len(outs)):
        for j in range(i):
            assert not np.array_equal(outs[i], outs[j]), (SETTINGS[i], SETTINGS[j])


# ---------------------------------------------------------------------------------------------- genie_swap_f32
@pytest.mark.gpu
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_exactly(n, off):
    """a and b change places bit for bit (NaN payloads and denormals included), nothing outside is written, two swaps are the identity."""
    torch = torch_()
    lib, L = libs()
    a0, b0 = values(n, 5 + n), values(n, 6 + n)
    a0.view(np.uint32)[::5] = 0x7FC12345      # a NaN with a payload: an exchange moves bytes, it does not compute
    a, b = Guarded(a0, off), Guarded(b0, off)
    lib.check(L.genie_swap_f32(a.ptr, b.ptr, n, stream()), "genie_swap_f32")
    torch.cuda.synchronize()
    assert_bits(a.read(), b0, "a <- b")
    assert_bits(b.read(), a0, "b <- a")
    lib.check(L.genie_swap_f32(a.ptr, b.ptr, n, stream()), "genie_swap_f32")
    torch.cuda.synchronize()
    assert_bits(a.read(), a0, "two swaps: a")
    assert_bits(b.read(), b0, "two swaps: b")


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_leave_the_outputs():
    """Every refusal returns GENIE_E_ARG and leaves sentinel-filled buffers as they were; n = 0 succeeds and writes nothing."""
    torch = torch_()
    lib, L = libs()
    n = 64
    sent = np.full(n, 12345.0, np.float32)
    p, g, m, v, e = (Guarded(sent) for _ in range(5))
    st = stream()
    adam = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    ok = (1, 1.0, None, 0.0, 0.1)
    E = lib.E_ARG
    ptrs = [p.ptr, g.ptr, m.ptr, v.ptr, e.ptr]
    for hole in range(5):
        args = list(ptrs)
        args[hole] = None
        assert L.genie_adamw_ema_step(*args, n, *adam, *ok, st) == E, hole
    assert L.genie_adamw_ema_step(*ptrs, n, *adam, 0, 1.0, None, 0.0, 0.1, st) == E
    assert L.genie_adamw_ema_step(*ptrs, n, *adam, -3, 1.0, None, 0.0, 0.1, st) == E
    for omd in (-1e-3, 1.001, float("nan"), float("inf"), float("-inf")):
        assert L.genie_adamw_ema_step(*ptrs, n, *adam, 1, 1.0, None, 0.0, omd, st) == E, omd
        assert L.genie_ema_update(e.ptr, p.ptr, n, omd, st) == E, omd
    assert L.genie_ema_update(None, p.ptr, n, 0.1, st) == E and L.genie_ema_update(e.ptr, None, n, 0.1, st) == E
    assert L.genie_swap_f32(None, p.ptr, n, st) == E and L.genie_swap_f32(p.ptr, None, n, st) == E
    assert L.genie_swap_f32(p.ptr, p.ptr, n, st) == E and L.genie_swap_f32(p.ptr, p.ptr + 4 * (n - 1), n, st) == E
    assert L.genie_swap_f32(p.ptr + 4 * (n - 1), p.ptr, n, st) == E
    assert L.genie_adamw_ema_step(*ptrs, 0, *adam, *ok, st) == 0 and L.genie_ema_update(e.ptr, p.ptr, 0, 0.1, st) == 0
    assert L.genie_swap_f32(p.ptr, e.ptr, 0, st) == 0
    torch.cuda.synchronize()
    for buf in (p, g, m, v, e):
        assert_bits(buf.read(), sent, "a refused call wrote")


# ---------------------------------------------------------------------------------------------- the trainer
@functools.lru_cache(maxsize=None)
def make_case(name):
    """(cfg, sd, input_ids, labels) as NumPy with the seeds of tests/test_hip_train_dropout.py::make_case.  Computed once, never written to."""
    H, d, T, S, B, qk_norm, use_mup, layers = CASES[name]
    cfg = pkg("config").GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                                    num_prompt_frames=T // 2, use_mup=use_mup)
    syn = pkg("synthetic")
    sd = syn.make_state_dict(cfg, seed=77 + H, law="conditioned")
    batch = TO.maskgit_collate(syn.make_clips(B, cfg, seed=900 + d), cfg, TO.NumpyDraws(5 + B))
    return cfg, sd, batch["input_ids"], batch["labels"]


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_trainer(name, precision, sd=None, **kw):
    cfg, sd0, _, _ = make_case(name)
    model = pkg("st_mask_git").STMaskGIT(cfg.shallow_copy(), precision=precision).load_numpy_state_dict(sd0 if sd is None else sd).to("cuda")
    return pkg("train").GenieTrainer(model, **{**TRAIN_KW, **kw})


def batch_of(name):
    _, _, ids, labels = make_case(name)
    return {"input_ids": dev(ids), "labels": dev(labels)}


def snapshot(tr, out):
    rec = {k: tr.__dict__[k].cpu().numpy().copy() for k in ("params", "exp_avg", "exp_avg_sq")}
    rec.update(loss=float(out["loss"]), acc=float(out["acc"]), grad_norm=float(out["grad_norm"]) if "grad_norm" in out else None,
               ema=None if tr.ema is None else tr.ema.cpu().numpy().copy(), ema_updates=tr.ema_updates)
    return rec


@functools.lru_cache(maxsize=None)
def run(name, precision, ema_decay, warm=False, accum=1):
    """STEPS train_steps on one batch -> (flat parameters before the first step, [snapshot after each step], padding mask)."""
    tr = make_trainer(name, precision, ema_decay=ema_decay, ema_warmup=warm, gradient_accumulation_steps=accum)
    start = tr.params.cpu().numpy().copy()
    if tr.ema is not None:
        assert_bits(tr.ema.cpu().numpy(), start, "the average starts as a copy of the parameters")
    batch = batch_of(name)
    recs = [snapshot(tr, tr.train_step(batch)) for _ in range(STEPS)]
    pad = np.ones(tr.n_flat, bool)
    for lo, hi in tr.offsets.values():
        pad[lo:hi] = False
    return start, recs, pad


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", STEP_CASES)
def test_ema_does_not_perturb_training(name, precision):
    """Four train_steps (weight decay 0.01, clipping at 1.0) with ema_decay = 0.9 and without: loss, acc, grad norm, parameters and both
    moments are bit-identical after every step -- the fused launch writes what genie_adamw_step writes."""
    _, with_ema, _ = run(name, precision, 0.9)
    start, without, _ = run(name, precision, None)
    assert without[0]["ema"] is None and without[-1]["ema_updates"] == 0
    for k, (a, b) in enumerate(zip(with_ema, without), 1):
        for key in ("loss", "acc", "grad_norm"):
            assert a[key] == b[key] and np.isfinite(a[key]), (k, key, a[key], b[key])
        for key in ("params", "exp_avg", "exp_avg_sq"):
            assert_bits(a[key], b[key], f"{key} after step {k}")
    assert not np.array_equal(without[-1]["params"], start) and not np.array_equal(without[-1]["params"], without[0]["params"])


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_trainer_average_is_the_contracts(name, precision, warm):
    """trainer.ema after each step is the NumPy replay over the parameters captured after each step, bit for bit; its padding is zero;
    ema_updates counts the steps."""
    start, recs, pad = run(name, precision, 0.9, warm)
    want = EM.replay(start, [r["params"] for r in recs], 0.9, warm)
    assert pad.any() == (name == "qk32")
    for k, (r, w) in enumerate(zip(recs, want), 1):
        assert r["ema_updates"] == k
        assert_bits(r["ema"], w, f"ema after step {k}")
        assert not r["ema"][pad].any() and not r["params"][pad].any()
    assert recs[-1]["ema_updates"] == STEPS == 4
    assert not np.array_equal(recs[-1]["ema"], recs[-1]["params"]) and not np.array_equal(recs[-1]["ema"], start)
    if warm:   # the two schedules differ from the first update on (2 / 11 against 0.9)
        assert not np.array_equal(recs[0]["ema"], run(name, precision, 0.9, False)[1][0]["ema"])


@pytest.mark.gpu
def test_average_moves_once_per_optimizer_step():
    """gradient_accumulation_steps = 2: four micro-batches give two updates, after the second and the fourth."""
    start, recs, _ = run("ln3", "exact", 0.9, False, 2)
    assert [r["ema_updates"] for r in recs] == [0, 1, 1, 2]
    assert_bits(recs[0]["ema"], start, "no update on a micro-batch without an optimizer step")
    want = EM.replay(start, [recs[1]["params"], recs[3]["params"]], 0.9)
    assert_bits(recs[1]["ema"], want[0], "first update")
    assert_bits(recs[2]["ema"], want[0], "third micro-batch")
    assert_bits(recs[3]["ema"], want[1], "second update")


# ---------------------------------------------------------------------------------------------- ema_scope
@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ema_scope(precision):
    """Inside the scope model(input_ids, labels) is, bit for bit, a fresh STMaskGIT of the same precision loaded from ema_state_dict() (the
    16-bit operand copies were repacked from the average); afterwards params and ema are what they were and the next train_step is that
    of a twin that never entered a scope; a raising body restores too; training calls inside raise RuntimeError."""
    torch = torch_()
    cfg, _, _, _ = make_case("ln3")
    batch = batch_of("ln3")
    tr, twin = (make_trainer("ln3", precision, ema_decay=0.9) for _ in range(2))
    for t in (tr, twin):
        for _ in range(2):
            t.train_step(batch)
    p0, e0 = tr.params.clone(), tr.ema.clone()
    assert not torch.equal(p0, e0)
    raw = tr.model(batch["input_ids"], batch["labels"])
    raw_loss, raw_logits = raw.loss.clone(), raw.logits.clone()
    avg_sd = tr.ema_state_dict()
    assert set(avg_sd) == set(dict(tr.model.named_parameters())) and all(avg_sd[k].shape == v.shape for k, v in tr.model.named_parameters())
    fresh = pkg("st_mask_git").STMaskGIT(cfg.shallow_copy(), precision=precision).to("cuda")
    fresh.load_state_dict(avg_sd, strict=True)
    want = fresh(batch["input_ids"], batch["labels"])
    want_loss, want_logits = want.loss.clone(), want.logits.clone()
    with tr.ema_scope() as model:
        assert model is tr.model
        got = model(batch["input_ids"], batch["labels"])
        assert torch.equal(got.loss, want_loss) and torch.equal(got.logits, want_logits) and bool(torch.isfinite(got.logits).all())
        assert not torch.equal(got.logits, raw_logits)
        assert torch.equal(tr.params, e0) and torch.equal(tr.ema, p0)
        inside = tr.ema_state_dict()
        assert all(torch.equal(inside[k], avg_sd[k]) for k in avg_sd)
        for call in (lambda: tr.train_step(batch), lambda: tr.forward_backward(batch["input_ids"], batch["labels"]), tr.optimizer_step,
                     tr.state_dict, lambda: tr.ema_scope().__enter__()):
            with pytest.raises(RuntimeError):
                call()
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0)
    again = tr.model(batch["input_ids"], batch["labels"])
    assert torch.equal(again.loss, raw_loss) and torch.equal(again.logits, raw_logits)      # the raw weights' 16-bit copies are back
    with pytest.raises(KeyError):
        with tr.ema_scope():
            raise KeyError("the body raises")
    assert torch.equal(tr.params, p0) and torch.equal(tr.ema, e0) and not tr._in_ema_scope
    a, b = tr.train_step(batch), twin.train_step(batch)
    assert float(a["loss"]) == float(b["loss"]) and float(a["grad_norm"]) == float(b["grad_norm"])
    for key in ("params", "ema", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr, key), getattr(twin, key)), key
    with pytest.raises(RuntimeError):
        with make_trainer("ln3", precision).ema_scope():
            pass


# ---------------------------------------------------------------------------------------------- resume
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_resume_restores_the_average(precision):
    """Two steps, state_dict() and model.state_dict() into a new model and trainer, two more: the average (and parameters, moments) are the
    bits of four uninterrupted steps.  A state without "ema" restarts the average from the parameters, a saved average is ignored by a
    trainer without EMA, a different decay joins the hyper-parameter warning -- each with a warning."""
    torch = torch_()
    batch = batch_of("ln3")
    _, recs, _ = run("ln3", precision, 0.9, True)
    first = make_trainer("ln3", precision, ema_decay=0.9, ema_warmup=True)
    for _ in range(2):
        first.train_step(batch)
    state = first.state_dict()
    assert state["ema"]["updates"] == 2 and state["ema"]["decay"] == 0.9 and state["ema"]["warmup"] is True
    assert set(state["ema"]["state"]) == set(state["state"])
    sd = {k: v.detach().cpu().numpy().copy() for k, v in first.model.state_dict().items()}
    resumed = make_trainer("ln3", precision, sd=sd, ema_decay=0.9, ema_warmup=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        resumed.load_state_dict(state)
    assert resumed.ema_updates == 2
    assert_bits(resumed.ema.cpu().numpy(), recs[1]["ema"], "the restored average")
    for k in (2, 3):
        resumed.train_step(batch)
        for key in ("params", "ema", "exp_avg", "exp_avg_sq"):
            assert_bits(getattr(resumed, key).cpu().numpy(), recs[k][key], f"{key} after step {k + 1}")
    assert resumed.ema_updates == 4

    no_ema_state = {k: v for k, v in state.items() if k != "ema"}
    restart = make_trainer("ln3", precision, sd=sd, ema_decay=0.9)
    restart.ema.fill_(7.0)
    with pytest.warns(UserWarning, match="restarts from the current parameters"):
        restart.load_state_dict(no_ema_state)
    assert restart.ema_updates == 0 and torch.equal(restart.ema, restart.params)
    plain = make_trainer("ln3", precision, sd=sd)
    with pytest.warns(UserWarning, match="ignored"):
        plain.load_state_dict(state)
    assert plain.ema is None and plain.completed_steps == 2 and "ema" not in plain.state_dict()
    other = make_trainer("ln3", precision, sd=sd, ema_decay=0.99, ema_warmup=False)
    with pytest.warns(UserWarning, match=r"different hyper-parameters.*ema_decay=0\.9->0\.99.*ema_warmup=True->False"):
        other.load_state_dict(state)
    assert other.ema_updates == 2 and torch.equal(other.ema, resumed.ema) is False
    assert_bits(other.ema.cpu().numpy(), recs[1]["ema"], "the saved average loads whatever the decay")


# ---------------------------------------------------------------------------------------------- the CLI
@pytest.mark.gpu
def test_train_cli_writes_the_average(tmp_path):
    """tools/train.py with --ema_decay 0.9 --eval_ema in one fresh child process under a time limit: the final checkpoint has an ema/
    directory that from_pretrained loads, whose weights differ from the raw checkpoint's and are trainer_state.pt's "ema" entries bit for
    bit (three updates); both evaluation losses are logged."""
    torch = torch_()
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "8", "--model", "tiny",
           "--precision", "exact", "--ema_decay", "0.9", "--max_train_steps", "3", "--checkpointing_steps", "3", "--eval_ema", "--seed", "1",
           "--per_device_eval_batch_size", "1", "--output_dir", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "step 3: eval_loss" in r.stdout and "step 3: ema_eval_loss" in r.stdout, r.stdout[-2000:]
    ck = tmp_path / "out" / "final_checkpt"
    assert (ck / "ema" / "config.json").exists() and (ck / "ema" / "model.safetensors").exists()
    M = pkg("st_mask_git").STMaskGIT
    raw, avg = M.from_pretrained(str(ck)), M.from_pretrained(str(ck / "ema"))
    assert vars(raw.config) == vars(avg.config)
    state = torch.load(str(ck / "trainer_state.pt"), map_location="cpu")
    assert state["ema"]["updates"] == 3 and state["ema"]["decay"] == 0.9 and state["ema"]["warmup"] is False
    raw_sd, avg_sd = raw.state_dict(), avg.state_dict()
    assert set(state["ema"]["state"]) == set(dict(avg.named_parameters()))
    moved = 0
    for k, v in state["ema"]["state"].items():
        assert torch.equal(avg_sd[k].cpu(), v.cpu()), k
        moved += int(not torch.equal(avg_sd[k].cpu(), raw_sd[k].cpu()))
    assert moved >= len(state["ema"]["state"]) // 2, moved
