"""Training step on the HIP path -- counterpart of the reference's train.py:426-441 (optimizer + grouping),
:468-492 (learning-rate schedules) and :600-633 (forward, backward, clip, step), with the data-parallel gradient
exchange accelerate/DDP does for it.

    trainer = GenieTrainer(model, lr=1e-4, weight_decay=0.0, max_grad_norm=1.0)
    out = trainer.train_step(collate_fn(features))        # dict(loss, acc, grad_norm, lr)

Design (MI355X-first):
  * parameters, gradients and both Adam moments live in four flat f32 buffers laid out in the order gradients become
    READY during the backward (readout, layers L-1..0, embeddings); the model's nn.Parameters are re-pointed at views
    of the parameter buffer, so `model.state_dict()` / `save_pretrained` keep working;
  * every activation the backward needs is kept (288 GB of HBM; nothing is recomputed except the spatial softmax);
  * multi-GPU: one process per GPU, clips sharded, gradients summed with one RCCL all-reduce per bucket of layers,
    launched as soon as that bucket's backward has been enqueued so the exchange overlaps the remaining backward;
    1/world_size and the clip coefficient are folded into the AdamW kernel (no host sync in the step);
  * precisions: the model's (`exact` f32 MFMA; `f16x3` split-f16 MFMA with f32-class gradients; `bf16` = what
    accelerate's bf16 autocast computes); parameters, gradients and Adam moments are f32 in all of them;
  * GPU only: there is no CPU fallback for the model math (the collator in data.py is device-agnostic data prep).
  * EMA of the weights (`ema_decay`; the reference's mechanism is magvit2/modules/ema.py, LitEma): one more flat f32 buffer that the AdamW
    launch itself updates (genie_adamw_ema_step: one more read and write per element, no second pass); `ema_scope()` swaps it
    with the parameters in place to evaluate, sample or save with the averaged weights.
  * distillation (`teacher`, `distill_alpha`, `distill_temperature`): soft targets from a teacher model's logits, mixed into the same fused
    loss kernel (genie_train_forward_distill), which reads the teacher's row beside the student's; the teacher's forward is the inference path.
  * Muon (`muon=MuonConfig(...)`): momentum and a Newton-Schulz orthogonalisation of the update of the hidden weight matrices, f32 on the
    matrix cores in every precision (genie_muon_step: batched over the same-shape matrices of all layers); everything else stays on AdamW.
  * training objective (`label_smoothing`, `z_loss`, `frame_weights`): label smoothing, z-loss and per-frame loss weights inside the
    fused loss kernel (genie_train_forward_obj); the backward reads its d logits as it reads the plain loss's; evaluation ignores it.
MuAdamW (--mu_transfer, train.py:439; third-party mup fork) is not built.
"""
import contextlib
import ctypes as C
import fnmatch
import math
import warnings

import numpy as np

import torch
import torch.distributed as dist

from . import _lib
from . import lora as _lora
from . import muon as _muon
from .lora import LINEAR_WEIGHTS, LoraConfig, linear_weight_names   # noqa: F401  (public here as well)
from .muon import MuonConfig   # noqa: F401


# ------------------------------------------------------------------ schedules (train.py:468-492)
def lr_factor_custom_cosine(warmup_steps, max_steps, end_ratio=0.1):
    """train.py:468-477: linear warm-up to 1, cosine decay to `end_ratio`."""
    def f(step):
        if step < warmup_steps:
            return (step + 1) / warmup_steps
        remaining = max_steps - warmup_steps
        return ((1 + math.cos(math.pi * (step - warmup_steps) / remaining)) / 2) * (1 - end_ratio) + end_ratio
    return f


def lr_factor_linear(warmup_steps, max_steps):
    """transformers.get_scheduler("linear", ...) -- the default --lr_scheduler_type (train.py:483-492)."""
    def f(step):
        if step < warmup_steps:
            return step / max(1, warmup_steps)
        return max(0.0, (max_steps - step) / max(1, max_steps - warmup_steps))
    return f


def decays(name: str) -> bool:
    """train.py:427-437: names containing "bias" or "layer_norm.weight" are excluded from weight decay.  No GENIE
    parameter is called layer_norm.* (they are norm1/norm2/norm), so LayerNorm weights DO decay, as in the reference.
    The learned null row of a model conditioned on action vectors (no reference counterpart) is a bias-like row and does not decay."""
    return not ("bias" in name or "layer_norm.weight" in name or name == "action_null")


# ------------------------------------------------------------------ EMA schedule (magvit2/modules/ema.py, LitEma.forward)
def ema_decay_at(decay, n, warmup=False):
    """d_n, the f32 decay of EMA update n = 1, 2, ... (include/genie_hip.h, "EMA of the weights"): float32(decay), or with `warmup`
    (LitEma's use_num_upates) min(float32(decay), float32((1 + n) / (10 + n))).  Raises ValueError unless 0 <= decay <= 1."""
    if not 0.0 <= decay <= 1.0:   # (False for NaN)
        raise ValueError(f"ema_decay must be in [0, 1], got {decay!r}")
    if n < 1:
        raise ValueError(f"EMA updates count from 1, got {n!r}")
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + n) / np.float32(10 + n))
    return float(d)


def ema_one_minus_decay(decay, n, warmup=False):
    """omd = float32(1) - d_n, the scalar the kernels take."""
    return float(np.float32(1) - np.float32(ema_decay_at(decay, n, warmup)))


# ------------------------------------------------------------------ training objective (include/genie_hip.h, "Training objective")
def objective_settings(label_smoothing=0.0, z_loss=0.0, frame_weights=None, T=None):
    """(eps, zeta, weights) as the trainer keeps them: floats, and a tuple of T floats or None.  All-ones weights are None.  Raises
    ValueError for eps outside [0, 1), a negative or non-finite zeta, a wrong number of weights, a negative or non-finite weight, or no
    positive weight behind frame 0 (frame 0 is never counted: nothing would be left to train on)."""
    eps, zeta = float(label_smoothing), float(z_loss)
    if not 0.0 <= eps < 1.0:   # (False for NaN)
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
    if not (zeta >= 0.0 and math.isfinite(zeta)):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss!r}")
    if frame_weights is None:
        return eps, zeta, None
    w = tuple(float(v) for v in frame_weights)
    if T is not None and len(w) != T:
        raise ValueError(f"frame_weights needs one weight per frame: {len(w)} given, T = {T}")
    if len(w) > 64:
        raise ValueError(f"frame_weights holds at most 64 frames, got {len(w)}")
    if not all(v >= 0.0 and math.isfinite(v) for v in w):
        raise ValueError(f"frame_weights must be finite and >= 0, got {w!r}")
    if not any(v > 0.0 for v in w[1:]):
        raise ValueError(f"frame_weights needs a positive weight behind frame 0 (frame 0 is never counted), got {w!r}")
    return eps, zeta, (None if all(v == 1.0 for v in w) else w)


def make_objective(eps, zeta, weights):
    """The genie_objective of objective_settings' values; None when they are neutral (the entry points of before)."""
    if np.float32(eps) == 0.0 and np.float32(zeta) == 0.0 and weights is None:   # the library's values are floats
        return None
    ob = _lib.Objective(label_smoothing=eps, z_loss=zeta, n_frames=0 if weights is None else len(weights), reserved=0)
    for t, v in enumerate(weights or ()):
        ob.frame_weight[t] = v
    return ob


# ------------------------------------------------------------------ distillation (include/genie_hip.h, "Distillation")
def distill_settings(distill_alpha=0.0, distill_temperature=1.0):
    """(alpha, tau) as floats.  Raises ValueError for alpha outside [0, 1] and for a temperature that is not finite and > 0."""
    alpha, tau = float(distill_alpha), float(distill_temperature)
    if not 0.0 <= alpha <= 1.0:   # (False for NaN)
        raise ValueError(f"distill_alpha must be in [0, 1], got {distill_alpha!r}")
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError(f"distill_temperature must be finite and > 0, got {distill_temperature!r}")
    return alpha, tau


def check_teacher(config, teacher_config):
    """A teacher may differ from the student in depth, width, heads and norms; it must share the clip geometry and the vocabulary, and
    be unconditioned or conditioned exactly as the student is.  Raises ValueError otherwise."""
    for k in ("T", "S", "image_vocab_size", "num_factored_vocabs"):
        if getattr(config, k) != getattr(teacher_config, k):
            raise ValueError(f"the teacher's {k} = {getattr(teacher_config, k)} differs from the student's {getattr(config, k)}")
    t_cond = (teacher_config.action_vocab_size, teacher_config.action_dim)
    if t_cond != (0, 0) and t_cond != (config.action_vocab_size, config.action_dim):
        raise ValueError(f"the teacher is conditioned on (action_vocab_size, action_dim) = {t_cond}, the student on "
                         f"{(config.action_vocab_size, config.action_dim)}: a teacher is unconditioned or conditioned as the student is")


# ------------------------------------------------------------------ pointer tables
def _ptr(t):
    return None if t is None else t.data_ptr()


# (LINEAR_WEIGHTS and linear_weight_names -- the nn.Linear weights that have 16-bit operand copies in the bf16 / f16x3 precisions, and
# that an adapter may target -- live in lora.py)


def weights_table(config, tensors, w16=None):
    """genie_weights table over state-dict-named tensors (parameters or gradients); `w16` (optional) maps Linear weight
    names to their 16-bit copies (*_w16 members).  Returns (table, keepalive)."""
    L = config.num_layers
    layers = (_lib.LayerWeights * L)()
    g = tensors.get
    h = (w16 or {}).get
    for i in range(L):
        p = f"decoder.layers.{i}."
        lw = layers[i]
        lw.norm1_w, lw.norm1_b = _ptr(g(p + "norm1.weight")), _ptr(g(p + "norm1.bias"))
        lw.norm2_w, lw.norm2_b = _ptr(g(p + "norm2.weight")), _ptr(g(p + "norm2.bias"))
        for name, aw in (("spatial_attn.", lw.spatial), ("temporal_attn.", lw.temporal)):
            aw.qkv_w, aw.qkv_b = _ptr(g(p + name + "qkv.weight")), _ptr(g(p + name + "qkv.bias"))
            aw.proj_w, aw.proj_b = _ptr(g(p + name + "proj.weight")), _ptr(g(p + name + "proj.bias"))
            aw.norm_w, aw.norm_b = _ptr(g(p + name + "norm.weight")), _ptr(g(p + name + "norm.bias"))
            aw.qkv_w16, aw.proj_w16 = _ptr(h(p + name + "qkv.weight")), _ptr(h(p + name + "proj.weight"))
        lw.fc1_w, lw.fc1_b = _ptr(g(p + "mlp.fc1.weight")), _ptr(g(p + "mlp.fc1.bias"))
        lw.fc2_w, lw.fc2_b = _ptr(g(p + "mlp.fc2.weight")), _ptr(g(p + "mlp.fc2.bias"))
        lw.fc1_w16, lw.fc2_w16 = _ptr(h(p + "mlp.fc1.weight")), _ptr(h(p + "mlp.fc2.weight"))
    w = _lib.Weights()
    w.pos_embed = _ptr(g("pos_embed_TSC"))
    w.mask_embed = _ptr(g("token_embed.mask_token_embed"))
    for j in range(config.num_factored_vocabs):
        w.embed[j] = _ptr(g(f"token_embed.factored_embeds.{j}.weight"))
    w.out_w, w.out_b = _ptr(g("out_x_proj.weight")), _ptr(g("out_x_proj.bias"))
    w.out_w16 = _ptr(h("out_x_proj.weight"))
    w.layers_host = layers
    return w, layers


def _embedding_side(name):
    return name.startswith("token_embed.") or name in ("pos_embed_TSC", "action_embed.weight", "action_proj.weight", "action_proj.bias",
                                                        "action_null")


def ready_order(config, names):
    """Parameter names in the order their gradients are final during the backward: readout, layers L-1..0 (within a
    layer: decaying tensors first, so each layer is two AdamW ranges), then the embedding side (with the action table of an
    action-conditioned model last -- or the projection weight, bias and null row of one conditioned on action vectors)."""
    names = list(names)
    head = [n for n in names if n.startswith("out_x_proj.")]
    emb = [n for n in names if _embedding_side(n)]
    out = sorted(head, key=lambda n: not decays(n))
    for i in reversed(range(config.num_layers)):
        p = f"decoder.layers.{i}."
        lay = [n for n in names if n.startswith(p)]
        out += sorted(lay, key=lambda n: not decays(n))
    out += emb
    assert sorted(out) == sorted(names), "unexpected parameter names"
    return out


# ------------------------------------------------------------------ training a subset of the weights
def _patterns(p):
    """None, one comma-separated string or an iterable of fnmatch patterns -> list of patterns (None stays None)."""
    if p is None:
        return None
    return [q for q in p.split(",") if q] if isinstance(p, str) else list(p)


def select_trainable(names, train_only=None, freeze=None):
    """The set of trainable state-dict names: those matching a `train_only` pattern (None: every name) and no `freeze` pattern.
    Patterns are fnmatch patterns, case-sensitive, over the whole name ("action_*", "decoder.layers.3[01].*", "*.bias"); each argument
    is a list of them or one comma-separated string.  Raises ValueError for a pattern that matches no name (a typo would otherwise
    freeze or train silently) and for an empty result."""
    names = list(names)
    chosen = set(names)
    for what, pats in (("train_only", _patterns(train_only)), ("freeze", _patterns(freeze))):
        if pats is None:
            continue
        hit = set()
        for p in pats:
            m = [n for n in names if fnmatch.fnmatchcase(n, p)]
            if not m:
                raise ValueError(f"{what} pattern {p!r} matches no parameter name")
            hit.update(m)
        chosen = chosen & hit if what == "train_only" else chosen - hit
    if not chosen:
        raise ValueError("no trainable parameter is left: train_only / freeze select nothing")
    return chosen


def lr_factors(names, lr_scale=None):
    """{name: factor} of `lr_scale` = {pattern: factor}: the factor of the first pattern (in the mapping's order) that matches the name,
    1.0 when none does.  Raises ValueError for a factor that is not finite and > 0, and for a pattern that matches no name."""
    names = list(names)
    out = {n: 1.0 for n in names}
    if not lr_scale:
        return out
    seen = set()
    for p, f in lr_scale.items():
        f = float(f)
        if not (f > 0.0 and math.isfinite(f)):
            raise ValueError(f"lr_scale[{p!r}] = {f!r} must be finite and > 0")
        m = [n for n in names if fnmatch.fnmatchcase(n, p)]
        if not m:
            raise ValueError(f"lr_scale pattern {p!r} matches no parameter name")
        for n in m:
            if n not in seen:
                out[n] = f
                seen.add(n)
    return out


def _pad64(n):
    return (n + 63) // 64 * 64   # 256-byte aligned tensors (float4 / MFMA staging loads)


def _layer_of(name):
    return int(name.split(".")[2]) if name.startswith("decoder.layers.") else None


class FlatLayout:
    """Where every tensor lives in the flat buffers, for a set of trainable names (None: all of them).

    order     trainable names in ready order, then the frozen ones in ready order
    offsets   {name: (lo, hi)} into the parameter buffer (tensors 256-byte aligned)
    n_flat    elements of the parameter buffer; n_train: of its trainable prefix = of the gradient, moment and EMA buffers
    trainable the set of trainable names; all: every name is trainable
    adam_runs [(lo, hi, decays, lr factor)]: maximal runs of consecutive trainable AdamW tensors with equal (decay flag, lr factor)
    muon      the trainable names the Muon step updates (`muon=`; empty by default): they break the runs and belong to none
    groups    [(key, lo, hi)] over the prefix, key "head", a layer index (L-1 .. 0) or "embed": one all-reduce segment per group that
              holds a trainable tensor, in ready order (segments = the (lo, hi) alone)
    stop      the backward runs layers L-1 .. stop: the lowest layer holding a trainable tensor, 0 when an embedding-side tensor
              (action tensors included) trains, num_layers when only the readout does
    embed     something on the embedding side trains: the embedding backward is called"""

    def __init__(self, config, numels, trainable=None, lr_scale=None, muon=None):
        names = list(numels)
        ro = ready_order(config, names)
        self.trainable = set(names) if trainable is None else set(trainable)
        unknown = self.trainable - set(names)
        if unknown or not self.trainable:
            raise ValueError(f"trainable names {sorted(unknown)} are not parameters" if unknown else "no trainable parameter")
        self.all = len(self.trainable) == len(names)
        self.order = [n for n in ro if n in self.trainable] + [n for n in ro if n not in self.trainable]
        self.lr_factor = lr_factors(names, lr_scale)
        self.offsets, o = {}, 0
        for n in self.order:
            self.offsets[n] = (o, o + numels[n])
            o += _pad64(numels[n])
        self.n_flat = o
        prefix = self.order[:len(self.trainable)]
        self.n_train = self.offsets[prefix[-1]][0] + _pad64(numels[prefix[-1]])
        self.muon = set(muon or ())
        if self.muon - self.trainable:
            raise ValueError(f"Muon names {sorted(self.muon - self.trainable)[:4]} are not trainable parameters")
        # AdamW ranges (padding between tensors is zero and stays zero: zero gradient, zero moments); a Muon tensor ends the run before it
        runs = []
        for n in prefix:
            lo = self.offsets[n][0]
            key = (decays(n), self.lr_factor[n], n in self.muon)
            if runs and tuple(runs[-1][2:]) == key:
                runs[-1][1] = lo + _pad64(numels[n])
            else:
                runs.append([lo, lo + _pad64(numels[n]), *key])
        self.adam_runs = [tuple(r[:4]) for r in runs if not r[4]]
        # all-reduce segments: one per group with a trainable tensor
        def group(n):
            return "head" if n.startswith("out_x_proj.") else ("embed" if _embedding_side(n) else _layer_of(n))
        self.groups = []
        for n in prefix:
            lo = self.offsets[n][0]
            if self.groups and self.groups[-1][0] == group(n):
                self.groups[-1][2] = lo + _pad64(numels[n])
            else:
                self.groups.append([group(n), lo, lo + _pad64(numels[n])])
        self.groups = [tuple(g) for g in self.groups]
        self.segments = [(lo, hi) for _, lo, hi in self.groups]
        self.embed = any(_embedding_side(n) for n in prefix)
        layers = [k for k, _, _ in self.groups if isinstance(k, int)]
        self.stop = 0 if self.embed else (min(layers) if layers else config.num_layers)


class BucketReducer:
    """Sum-all-reduce of contiguous slices of one flat gradient buffer, one slice per bucket, asynchronously.

    `ready(hi)` says "gradients [0, hi) are final (their kernels are enqueued on the current stream)"; every bucket
    that is now complete is handed to the process group at once (RCCL orders itself after the current stream), so
    the exchange of late layers runs under the backward of early ones.  `finish()` makes the current stream wait for
    all of them.  Works on any backend (gloo in the CPU tests)."""

    def __init__(self, flat, bounds, group=None, always=False):
        # always: hand the buckets to the process group even at world size 1 (a one-GPU box exercising RCCL itself)
        self.flat, self.bounds, self.group, self.always = flat, list(bounds), group, always
        self.reset()

    def reset(self):
        self.next, self.works = 0, []

    @property
    def world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def ready(self, hi):
        if self.world == 1 and not (self.always and dist.is_available() and dist.is_initialized()):
            return
        while self.next < len(self.bounds) and self.bounds[self.next][1] <= hi:
            lo, up = self.bounds[self.next]
            self.works.append(dist.all_reduce(self.flat[lo:up], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            self.next += 1

    def finish(self):
        self.ready(self.flat.numel())
        for w in self.works:
            w.wait()
        self.reset()


def bucket_bounds(segments, target_elems):
    """Greedy contiguous buckets over [(lo, hi)] segments (in ready order) of at least `target_elems` elements."""
    out, start, end = [], None, None
    for lo, hi in segments:
        if start is None:
            start = lo
        end = hi
        if end - start >= target_elems:
            out.append((start, end))
            start = None
    if start is not None:
        out.append((start, end))
    return out


class GenieTrainer:
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0,
                 gradient_accumulation_steps=1, lr_lambda=None, bucket_mb=64, group=None, recompute=False, dropout_seed=0,
                 ema_decay=None, ema_warmup=False, label_smoothing=0.0, z_loss=0.0, frame_weights=None, trainable=None, lr_scale=None,
                 teacher=None, distill_alpha=0.0, distill_temperature=1.0, lora=None, muon=None):
        """muon: a MuonConfig: the trainable tensors among the Linear weights its `targets` select (muon.py; include/genie_hip.h, "Muon") are
        updated by Muon -- momentum, then a Newton-Schulz orthogonalisation of the update, f32 on the matrix cores in all three precisions --
        and everything else (embeddings, positions, norms, biases, action tensors, LoRA adapters, an untargeted readout) by AdamW with the
        bits it has today.  A fused qkv weight is three matrices (q, k, v rows), orthogonalised separately.  A frozen target is skipped (the
        base weight of a LoRA-adapted Linear included); ValueError when no target trains.  The momentum lives in the tensor's `exp_avg`
        range, its `exp_avg_sq` range stays zero; `lr_scale`, `decays(name)`, the schedule, the global clip and the EMA apply as for AdamW.
        The matrices of all layers are sorted by shape and cut into tables of GENIE_MUON_MAX_ITEMS: one genie_muon_step call per table,
        into one workspace sized for the largest.  `state_dict` carries the settings; `load_state_dict` raises ValueError for a state saved
        under other settings or under the other optimizer.  None: the layout, launches and bits of before.
        lora: a LoraConfig: train low-rank adapters on the Linears its `targets` select (lora.py; include/genie_hip.h, "LoRA adapters").
        Each adapted <linear>.weight keeps its base W0 in a trainer-owned f32 buffer (`self.w0`) and gains <linear>.lora_A (rank, in) and
        <linear>.lora_B (out, rank): not module parameters, but tensors of the flat buffers like any trainable one (ready order inside
        their layer's group, decaying; AdamW ranges, all-reduce segments, the norm, the clip, the EMA and `lr_scale` patterns cover them by
        name).  The module's parameter holds W = W0 + (alpha / rank) B A, so the untouched step, `forward`, `generate` and
        `save_pretrained` (a merged stand-alone checkpoint) see the adapted model in every precision.  The backward writes dW of an
        adapted Linear into a scratch (one layer's worth, reused by every layer; the readout has its own) and genie_lora_project turns it
        into dA, dB in `grads` right behind each head / layer call; after an optimizer step or an EMA exchange the weights are merged
        again and the adapted Linears repacked.  The weight-gradient products of adapted Linears still run: the step is not faster than
        a full fine-tune, it is smaller (state, all-reduce bytes, what is shipped).  With `lora`, `trainable=None` means "the adapters
        alone" and `trainable=` names ADDITIONAL fully trained tensors ("action_*"); an adapted weight named by it raises ValueError.  A
        starts as U(-1/sqrt(in), 1/sqrt(in)) from (seed, name), B as zero: the fresh trainer computes the base model.
        `adapter_state_dict`, `load_adapter_state_dict`, `save_adapter`.  None: no new buffer and the library calls of before.
        teacher, distill_alpha, distill_temperature: distillation (include/genie_hip.h, "Distillation"): the loss becomes
        (1 - alpha) * the objective's hard loss + alpha * tau^2 KL(softmax(teacher / tau) || softmax(student / tau)) + the z-loss, still
        inside the fused loss kernel, which reads the teacher's logits beside the student's.  `teacher` is an STMaskGIT on the same
        device, in any precision, depth, width and norm of its own, with the student's T, S and vocabulary, unconditioned or conditioned as
        the student is (ValueError otherwise).  Every `forward_backward` runs its `compute_logits` on the ids the student sees (and the
        student's actions and action_drop flags when it is conditioned), on the trainer's stream, into a trainer-owned (B, T, S, V) f32
        buffer: no host synchronisation.  Without a teacher, `forward_backward(teacher_logits=)` takes precomputed logits.  `last_kd` (the
        unweighted tau^2 KL per counted token) and `last_teacher_ce` (the teacher's own cross-entropy on the same tokens: it tells a
        mis-wired teacher at once) sit beside `last_ce`.  The teacher is never trained, saved, averaged, all-reduced or repacked; under
        data parallelism every rank holds its own.  With teacher None and distill_alpha 0: no new buffer and the entry points of before.
        trainable: train a subset of the weights (fine-tuning; the reference: requires_grad = False on the rest, which torch.optim.AdamW
        and clip_grad_norm_ then skip).  None: everything.  Else fnmatch patterns over state-dict names (a list, or one comma-separated
        string; `select_trainable` also takes a freeze list and returns names, which are patterns too), or a callable name -> bool.  A
        frozen tensor costs nothing: no gradient (a NULL in the gradient table: include/genie_hip.h, "Frozen tensors"), no moments, no
        average, no all-reduce bytes, no 16-bit repack; the backward stops at the lowest layer that holds a trainable tensor (`layout.stop`)
        and, with `recompute`, rebuilds nothing below it.  The flat parameter buffer keeps the trainable tensors first (ready order), then
        the frozen ones; `grads`, `exp_avg`, `exp_avg_sq` and `ema` cover that prefix (`n_train` elements).  The gradients that are
        computed are the bits of the full step; grad norm and clip run over them alone, which is torch's semantics.
        lr_scale: {pattern: factor}: a tensor's learning rate is lr * factor of the first pattern that matches it (1 when none does).
        With both None: the buffers and the library calls of before.
        label_smoothing, z_loss, frame_weights: the training objective (include/genie_hip.h, "Training objective"): per factor
        F.cross_entropy(label_smoothing=eps) + z_loss * logsumexp^2, each counted token weighted by its frame's entry of `frame_weights`
        (T floats >= 0; frame 0 is never counted) and the sum divided by the summed weights of the counted tokens.  All in the fused loss
        kernel, which still reads and writes the logits once; the backward is untouched.  `forward_backward` returns this objective as
        its loss -- the quantity the gradients are of -- and `last_ce` holds the plain masked cross-entropy of the same micro-batch, which
        is what the evaluators report.  At the defaults (all-ones weights count as None): no new buffer and the entry points of before.
        ema_decay: keep an exponential moving average of the weights in `self.ema`, a flat f32 buffer with the layout of `self.params`
        that starts as a copy of it (after the rank-0 broadcast: replicas hold identical averages, nothing is communicated).  Every
        optimizer step -- not every micro-batch -- moves it by ema = ema - omd * (ema - p_new) inside the AdamW launch, with
        omd = 1 - ema_decay_at(ema_decay, ema_updates + 1, ema_warmup); ema_warmup is LitEma's use_num_upates, min(decay, (1 + n) / (10 + n)).
        `ema_scope()` runs the model on the averaged weights, `ema_state_dict()` / `save_ema_pretrained(dir)` export them, `state_dict()`
        carries them.  None (the default): no buffer, and exactly the launches of a trainer without the feature.
        dropout_seed: with config.mlp_drop > 0 the step trains with the reference's MLP dropout (st_transformer.py:22-25).  The masks
        are a pure function of (dropout_seed + rank, micro-batch counter, layer, site, element) (include/genie_hip.h, "MLP dropout"): nothing
        is stored, and a run resumed from `state_dict` draws the masks it would have drawn.  mlp_drop = 0 is the step without dropout.
        recompute: keep only each layer's input from the forward and rebuild the layer's other activations in front of its
        backward (include/genie_hip.h, "Activation recomputation"): the same loss and gradient bits from an activation buffer of
        about one layer plus L checkpoints, for about one more layer forward per layer of time."""
        self.model, self.config = model, model.config
        self.recompute = 1 if recompute else 0
        dev = model._device()  # raises on CPU: no fallback
        self.lib = _lib.load()
        self.precision = model.precision
        self.cfg = _lib.make_cfg(self.config, model._prec)
        self.base_lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.accum = gradient_accumulation_steps
        self.lr_lambda = lr_lambda or (lambda step: 1.0)
        self.completed_steps, self._micro = 0, 0
        self.mlp_drop = float(getattr(self.config, "mlp_drop", 0.0))
        if not 0.0 <= self.mlp_drop < 1.0:
            raise ValueError(f"config.mlp_drop must be in [0, 1), got {self.mlp_drop!r}")
        self.dropout_seed, self._drop_call = int(dropout_seed), 0   # the counter advances once per forward_backward
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if self.ema_decay is not None:
            ema_decay_at(self.ema_decay, 1, self.ema_warmup)   # ValueError outside [0, 1]
        self.label_smoothing, self.z_loss, self.frame_weights = objective_settings(label_smoothing, z_loss, frame_weights, self.config.T)
        self._objective = make_objective(self.label_smoothing, self.z_loss, self.frame_weights)   # None: neutral
        self.last_ce = None   # plain masked CE of the last micro-batch (0-dim device tensor)
        self.distill_alpha, self.distill_temperature = distill_settings(distill_alpha, distill_temperature)
        if teacher is not None:
            check_teacher(self.config, teacher.config)
            if teacher._device() != dev:
                raise ValueError(f"the teacher is on {teacher._device()}, the student on {dev}")
        self.teacher = teacher
        self._distilling = np.float32(self.distill_alpha) != 0.0   # the library's alpha is a float
        self._teacher_logits = None   # (B, T, S, V) f32, per batch size
        self.last_kd = self.last_teacher_ce = None   # tau^2 KL and the teacher's own CE per counted token, of the last micro-batch

        named = dict(model.named_parameters())
        shapes = {n: tuple(p.shape) for n, p in named.items()}
        self.lora, self.lora_targets, adapters = lora, [], {}
        if lora is not None:
            if not isinstance(lora, LoraConfig):
                raise TypeError(f"lora must be a LoraConfig, got {type(lora).__name__}")
            self.lora_targets = _lora.select_targets(self.config, lora.targets)
            adapters = _lora.adapter_shapes(self.lora_targets, shapes, lora.rank)
            shapes.update(adapters)
        self._shapes = shapes
        if trainable is None:
            chosen = None
        elif callable(trainable):
            chosen = {n for n in named if trainable(n)}
            if not chosen:
                raise ValueError("no trainable parameter is left: `trainable` accepts no parameter name")
        else:
            chosen = select_trainable(named.keys(), train_only=trainable)
        if lora is not None:   # the adapters, and what `trainable` names beside them
            both = sorted(set(chosen or ()) & set(self.lora_targets))
            if both:
                raise ValueError(f"{both[:4]} are adapted by `lora` and named by `trainable`: a weight trains fully or through its adapter")
            chosen = set(chosen or ()) | set(adapters)
        self.lr_scale = dict(lr_scale) if lr_scale else None
        self.muon, muon_names = muon, ()
        if muon is not None:
            if not isinstance(muon, MuonConfig):
                raise TypeError(f"muon must be a MuonConfig, got {type(muon).__name__}")
            muon_names = _muon.muon_names(self.config, muon.targets, set(shapes) if chosen is None else chosen)
        lay = self.layout = FlatLayout(self.config, {n: int(np.prod(s)) for n, s in shapes.items()}, chosen, self.lr_scale, muon_names)
        self.order, self.offsets, self.n_flat, self.n_train = lay.order, lay.offsets, lay.n_flat, lay.n_train
        self.trainable = [n for n in self.order if n in lay.trainable]   # the prefix, in ready order
        offs = self.offsets
        self.params = torch.zeros(self.n_flat, dtype=torch.float32, device=dev)
        # gradients, moments (and the average) exist for the trainable prefix alone
        self.grads = torch.zeros(self.n_train, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.grads)
        self.exp_avg_sq = torch.zeros_like(self.grads)
        with torch.no_grad():
            for n in self.order:
                lo, hi = offs[n]
                if n in adapters:   # B stays zero
                    if n.endswith(_lora.SUFFIX_A):
                        self.params[lo:hi].copy_(torch.from_numpy(_lora.draw_a(n, shapes[n], lora.seed)).reshape(-1))
                    continue
                view = self.params[lo:hi].view(named[n].shape)
                view.copy_(named[n].data)
                named[n].data = view  # the module now reads (and checkpoints) the flat buffer
        # every replica starts from rank 0's parameters, as DistributedDataParallel does when it wraps the module
        # (the reference relies on that broadcast: train.py:441 `accelerator.prepare`); the trainer itself only
        # all-reduces gradients, so replicas that start apart would stay apart
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.broadcast(self.params, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        # the average starts from the (broadcast) parameters; padding is zero in both and stays zero
        self.ema = self.params[:self.n_train].clone() if self.ema_decay is not None else None
        self.ema_updates, self._in_ema_scope = 0, False
        model.refresh_weights()
        self.p_views = {n: self.params[offs[n][0]:offs[n][1]] for n in self.order}
        self.g_views = {n: self.grads[offs[n][0]:offs[n][1]].view(shapes[n]) for n in self.trainable}
        # 16-bit operand copies of the Linear weights, both orientations (bf16: 1 plane, f16x3: [hi | lo])
        self.w16 = self.w16T = None
        self.wT_table = None
        if self.precision != "exact":
            npl = 1 if self.precision == "bf16" else 2
            lin = linear_weight_names(self.config)
            self.w16 = {n: torch.empty((npl,) + tuple(named[n].shape), dtype=torch.int16, device=dev) for n in lin}
            self.w16T = {n: torch.empty((npl,) + tuple(named[n].shape)[::-1], dtype=torch.int16, device=dev) for n in lin}
            self.wT_table, self._wTk = weights_table(self.config, {}, self.w16T)
        self.w_table, self._wk = weights_table(self.config, {n: named[n].data for n in self.order if n in named}, self.w16)
        g_entries = self.g_views
        if lora is not None:   # an adapted weight's gradient-table entry is its dW scratch: the backward computes it, the repack selects it
            g_entries = dict(self.g_views, **self._lora_setup(named, dev))
        self.g_table, self._gk = weights_table(self.config, g_entries)   # NULL members: frozen tensors (genie_hip.h, "Frozen tensors")
        self.pack_weights()
        # AdamW ranges: maximal runs of consecutive trainable tensors with the same (decay flag, lr factor)
        self.adam_runs = lay.adam_runs
        # all-reduce buckets: the segments of the groups that hold a trainable tensor ([head, layer L-1, ..., layer 0, embeddings] when
        # everything trains), merged up to bucket_mb
        self.segments = lay.segments
        self._group_hi = {k: hi for k, _, hi in lay.groups}   # group -> "gradients [0, hi) are final" once its backward is enqueued
        self.reducer = BucketReducer(self.grads, bucket_bounds(self.segments, bucket_mb * (1 << 20) // 4), group)
        self._dw_scratch = None   # where the gradient of a frozen action_proj.weight goes (genie_action_rows_backward needs a d_weight)
        # [sum loss, sum hits, n]; with an objective [sum w l, sum hits, W, sum plain nll, n]
        # distilling: [.., sum plain kd, sum teacher plain nll]
        self.sums = torch.zeros(7 if self._distilling else (3 if self._objective is None else 5), dtype=torch.float64, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.scratch = torch.zeros(1024, dtype=torch.float64, device=dev)
        self._acts = self._ws = None
        self._B = 0
        self._d_rows = None   # (1 + B T, d) scratch: d loss / d rows of a model conditioned on action vectors, overwritten per call
        if muon is not None:
            self._muon_setup(muon_names, dev)

    # ------------------------------------------------------------------ Muon
    def _muon_setup(self, names, dev):
        """The item tables (one per chunk of same-shape matrices) and the workspace, once: the pointers never move."""
        self.muon_names = list(names)
        entries = []   # MuonItems, each carrying its tensor's name (q, k and v of a fused qkv share one)
        for n in self.muon_names:
            lo = self.offsets[n][0]
            for r0, rows, cols in _muon.blocks(n, self._shapes[n]):
                off = 4 * (lo + r0 * cols)
                it = _muon.item(rows, cols, self.params.data_ptr() + off, self.grads.data_ptr() + off, self.exp_avg.data_ptr() + off,
                                None if self.ema is None else self.ema.data_ptr() + off)
                it.name = n
                entries.append(it)
        self.muon_items = entries
        self._muon_tables = [(part, *_muon.table(part)) for part in _muon.chunks(entries)]
        need = 0
        for _, arr, k in self._muon_tables:
            b = self.lib.genie_muon_workspace_bytes(arr, k)
            if b == 0:
                _lib.check(_lib.E_ARG, "genie_muon_workspace_bytes")
            need = max(need, b)
        self._muon_ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def muon_launches(self):
        """Kernel launches of the Muon part of one optimizer step."""
        return _muon.launches(self.muon_items, self.muon.ns_steps) if self.muon is not None else 0

    def _muon_step(self, lr, mult, ss, clip, omd, st):
        stg = _muon.settings(self.muon, grad_mult=mult, grad_sumsq=ss.data_ptr() if clip > 0 else None, max_grad_norm=clip,
                             ema_one_minus_decay=0.0 if omd is None else omd)
        for part, arr, k in self._muon_tables:
            for i, it in enumerate(part):
                arr[i].lr = lr * self.layout.lr_factor[it.name]
                arr[i].weight_decay = self.weight_decay if decays(it.name) else 0.0
            _lib.check(self.lib.genie_muon_step(arr, k, stg, self._muon_ws.data_ptr(), self._muon_ws.numel(), st), "genie_muon_step")

    # ------------------------------------------------------------------ LoRA adapters
    def _lora_setup(self, named, dev):
        """The base weights, the dW scratch and the item tables.  Returns {adapted weight name: its dW scratch view}."""
        lc, shapes = self.lora, self._shapes
        self.w0 = {n: named[n].data.clone() for n in self.lora_targets}   # after the rank-0 broadcast; B = 0: the parameters ARE W0
        # one layer's worth of dW, shared by every layer (a layer's backward is projected before the next one runs); the head's own
        short = lambda n: n.split(".", 3)[3] if n.startswith("decoder.layers.") else n   # noqa: E731
        dw = {}
        for n in self.lora_targets:
            if short(n) not in dw:
                dw[short(n)] = torch.zeros(shapes[n], dtype=torch.float32, device=dev)
        self._lora_dw = dw
        self._lora_items, self._lora_dw_of, merge_items = {}, {}, []   # group key ("head" or a layer index) -> [LoraItem], [dW scratch]
        for n in self.lora_targets:
            (o, i), (na, nb) = shapes[n], _lora.adapter_names(n)
            it = _lora.item(lc.scale, o, i, lc.rank, self.p_views[na].data_ptr(), self.p_views[nb].data_ptr(), w=named[n].data.data_ptr(),
                            w0=self.w0[n].data_ptr(), dw=dw[short(n)].data_ptr(), da=self.g_views[na].data_ptr(),
                            db=self.g_views[nb].data_ptr())
            key = _layer_of(n)
            key = "head" if key is None else key
            self._lora_items.setdefault(key, []).append(it)
            self._lora_dw_of.setdefault(key, []).append(dw[short(n)])
            merge_items.append(it)
        self._lora_merge_items = merge_items
        self._lora_tables = {k: _lora.table(v) for k, v in self._lora_items.items()}
        need = max(self.lib.genie_lora_project_scratch_bytes(arr, n) for arr, n in self._lora_tables.values())
        if need == 0:
            _lib.check(_lib.E_ARG, "genie_lora_project_scratch_bytes")
        self._lora_scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        return {n: dw[short(n)] for n in self.lora_targets}

    def _lora_merge(self):
        """W = W0 + s B A into the module's parameters, from whatever the flat buffer holds for A and B now."""
        _lora.merge(self.lib, self._lora_merge_items, self._stream())

    def _lora_zero_dw(self, key):
        """accumulate: the backward's flag applies to every gradient of the call, dW included -- the reused scratch starts from zero."""
        for t in self._lora_dw_of.get(key, ()):
            t.zero_()

    def _lora_project(self, key, acc_flag):
        """dW scratch of group `key` -> dA, dB in the flat gradient buffer (added when acc_flag)."""
        if key in self._lora_tables:
            arr, n = self._lora_tables[key]
            _lib.check(self.lib.genie_lora_project(arr, n, acc_flag, self._lora_scratch.data_ptr(), self._lora_scratch.numel(),
                                                   self._stream()), "genie_lora_project")

    def adapter_state_dict(self):
        """{<linear>.lora_A / .lora_B: clone} of the adapters (inside ema_scope(): of their averages)."""
        self._need_lora("adapter_state_dict")
        return {n: self.p_views[n].view(self._shapes[n]).clone() for t in self.lora_targets for n in _lora.adapter_names(t)}

    def load_adapter_state_dict(self, sd):
        """Inverse of `adapter_state_dict`: copies the tensors (names and shapes must match exactly: ValueError), merges and repacks."""
        self._need_lora("load_adapter_state_dict")
        self._not_in_ema_scope("load_adapter_state_dict")
        want = {n: self._shapes[n] for t in self.lora_targets for n in _lora.adapter_names(t)}
        if set(sd) != set(want):
            raise ValueError(f"adapter tensors do not match this trainer's: missing {sorted(set(want) - set(sd))[:4]}, unexpected "
                             f"{sorted(set(sd) - set(want))[:4]}")
        for n, shp in want.items():
            if tuple(sd[n].shape) != shp:
                raise ValueError(f"adapter tensor {n} has shape {tuple(sd[n].shape)}, expected {shp}")
        for n in want:
            self.p_views[n].copy_(torch.as_tensor(sd[n]).to(self.params.device, torch.float32).reshape(-1))
        self._pack_trained()
        self.model.refresh_weights()

    def save_adapter(self, save_directory):
        """adapter_config.json (rank, alpha, target names, the base's shape fields) + adapter.safetensors: what STMaskGIT.load_adapter takes."""
        self._need_lora("save_adapter")
        _lora.save_adapter(save_directory, _lora.adapter_config(self.lora, self.lora_targets, self.config), self.adapter_state_dict())

    def _need_lora(self, what):
        if self.lora is None:
            raise RuntimeError(f"GenieTrainer.{what} needs a trainer built with lora=")

    def pack_weights(self):
        """Refresh the 16-bit weight copies from the f32 parameters (no-op in the exact precision).  Call this (or
        `sync_external_weights`) after ANY weight mutation the trainer did not make itself -- `model.load_state_dict`,
        `load_numpy_state_dict` -- or the 16-bit GEMM operands keep the old weights until the next optimizer step."""
        if self.precision != "exact":
            _lib.check(self.lib.genie_train_pack_weights(self.cfg, self.w_table, self.w_table, self.wT_table,
                                                         self._stream()), "genie_train_pack_weights")

    def _pack_trained(self):
        """pack_weights after a change the trainer made itself (optimizer step, EMA exchange): those move the trainable prefix alone,
        so only the trainable Linears are repacked -- the gradient table says which."""
        if self.lora is not None:   # the adapters moved: the effective weights follow, and the gradient table selects them below
            self._lora_merge()
        if self.layout.all:
            return self.pack_weights()
        if self.precision != "exact":
            _lib.check(self.lib.genie_train_pack_weights_some(self.cfg, self.w_table, self.w_table, self.wT_table, self.g_table,
                                                              self._stream()), "genie_train_pack_weights_some")

    def sync_external_weights(self):
        """After the caller changed the model's parameters in place (they are views of the flat buffer): repack the
        16-bit operand copies here and the inference-side copies of the module."""
        self.pack_weights()
        self.model.refresh_weights()

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B):
        if B != self._B:
            self._acts = self._ws = self._teacher_logits = None
            na = _lib.call_recompute(self.lib, "genie_train_activation_bytes", self.recompute, self.cfg, B)
            nw = _lib.call_recompute(self.lib, "genie_train_workspace_bytes", self.recompute, self.cfg, B)
            if na == 0 or nw == 0:
                _lib.check(self.lib.genie_check_config(self.cfg), "genie_check_config")
            self._acts = torch.empty(na, dtype=torch.uint8, device=self.params.device)
            self._ws = torch.empty(nw, dtype=torch.uint8, device=self.params.device)
            if self._distilling and self.teacher is not None:
                V = self.config.factored_vocab_size * self.config.num_factored_vocabs
                self._teacher_logits = torch.empty(B, self.config.T, self.config.S, V, dtype=torch.float32, device=self.params.device)
                self.teacher._workspace(B)   # the teacher's own workspace, allocated here and not inside the first step
            self._B = B
        return self._acts, self._ws

    def _frame_cond(self, model, action_ids, action_vectors, drop, B):
        """The genie_frame_cond of `model` (the student or a conditioned teacher) for one micro-batch; `drop`: checked (B,) bool or None."""
        cond = model._cond(action_ids, B, action_vectors=action_vectors)
        if drop is not None:
            vectors = cond.vectors
            rows_ids = torch.where(drop.to(cond.keep.device)[:, None], model.NULL_ROW, cond.keep).contiguous()
            cond = model._frame_cond(rows_ids, like=cond)
            cond.vectors = vectors
        return cond

    def _distill(self, ids, B, teacher_logits, action_ids, action_vectors, drop):
        """The genie_distill of one micro-batch (None when not distilling): the teacher's logits of the ids the student sees, from the
        caller or from the live teacher (one inference forward on this stream into the trainer's buffer)."""
        if not self._distilling:
            if teacher_logits is not None:
                raise ValueError("teacher_logits given to a trainer with distill_alpha == 0")
            return None
        c = self.config
        shape = (B, c.T, c.S, c.factored_vocab_size * c.num_factored_vocabs)
        if teacher_logits is not None:
            tl = teacher_logits
            if not (tl.is_cuda and tl.dtype == torch.float32 and tuple(tl.shape) == shape):
                raise RuntimeError(f"expected teacher_logits of shape {shape}, float32, on the device; got {tuple(tl.shape)} {tl.dtype} "
                                   f"{tl.device}")
            tl = tl.contiguous()
        elif self.teacher is not None:
            t = self.teacher
            conditioned = t.config.action_vocab_size or t.config.action_dim
            cond = self._frame_cond(t, action_ids, action_vectors, drop, B) if conditioned else None
            with torch.no_grad():
                tl = t.compute_logits_frames(ids, 0, c.T, "token", out=self._teacher_logits, cond=cond)
        else:
            raise ValueError(f"distill_alpha = {self.distill_alpha} needs a teacher: build the trainer with teacher=, or pass teacher_logits=")
        ds = _lib.Distill(alpha=self.distill_alpha, temperature=self.distill_temperature, teacher_logits=tl.data_ptr())
        ds.keep = tl   # the logits live as long as the struct
        return ds

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _dropout(self):
        """The genie_dropout of the next micro-batch (None without dropout: the entry points of before), advancing the counter."""
        if self.mlp_drop == 0.0:
            return None
        rank = dist.get_rank(self.reducer.group) if dist.is_available() and dist.is_initialized() else 0
        dr = _lib.Dropout(p=self.mlp_drop, call=self._drop_call & 0xFFFFFFFF, seed=(self.dropout_seed + rank) & (2 ** 64 - 1))
        self._drop_call += 1
        return dr

    # ------------------------------------------------------------------ forward / backward (train.py:611-617)
    def forward_backward(self, input_ids, labels, accumulate=False, reduce=True, action_ids=None, action_vectors=None, action_drop=None,
                         teacher_logits=None):
        """One micro-batch: loss/acc of STMaskGIT.forward and gradients into the flat buffer (added when
        `accumulate`).  Returns (loss, acc) as 0-dim float64 CUDA tensors (no host sync).
        action_ids: (B, T) per-frame actions of an action-conditioned model (config.action_vocab_size > 0).
        action_vectors: (B, T, action_dim) float actions of a model with config.action_dim > 0: projected into per-frame rows (one launch),
        the existing forward and backward run on those rows, and d loss / d rows -- a (1 + B T, d) scratch, row 0 the null row's -- becomes
        the gradients of action_proj (genie_action_rows_backward, one launch) and of action_null.
        action_drop: (B,) bool with action_vectors (action dropout, data.maskgit_collate): a dropped clip's frames read the null row, so
        their projected rows get a zero gradient and the null row theirs.
        teacher_logits: (B, T, S, V) f32 device logits of a teacher on these input_ids, token-major, for a trainer with distill_alpha > 0
        (offline distillation from saved logits): used instead of the trainer's teacher.  They are read, never written."""
        self._not_in_ema_scope("forward_backward")
        if not (input_ids.is_cuda and labels.is_cuda):
            raise RuntimeError("1xgpt_amd runs on the GPU only (no CPU fallback): move the batch to cuda")
        ids = input_ids.to(torch.int64).contiguous()
        lab = labels.to(torch.int64).contiguous()
        B = ids.shape[0]
        assert ids.shape == lab.shape == (B, self.config.T * self.config.S), ids.shape
        vec = self.config.action_dim > 0
        if action_drop is not None and not vec:
            raise ValueError("action_drop needs a model conditioned on action vectors (config.action_dim > 0)")
        drop = None
        if action_drop is not None:
            drop = torch.as_tensor(action_drop)
            if drop.dtype != torch.bool or tuple(drop.shape) != (B,):
                raise RuntimeError(f"expected action_drop of shape ({B},) and dtype bool, got {tuple(drop.shape)} {drop.dtype}")
        cond = self._frame_cond(self.model, action_ids, action_vectors, drop, B)
        acts, ws = self._buffers(B)
        distill = self._distill(ids, B, teacher_logits, action_ids, action_vectors, drop)
        lib, cfg, st = self.lib, self.cfg, self._stream()
        acc_flag = 1 if accumulate else 0
        drop = self._dropout()
        if distill is not None:   # the same forward, the distillation loss kernel behind it; the backward reads its d logits as before
            _lib.check(lib.genie_train_forward_distill(cfg, self.w_table, ids.data_ptr(), lab.data_ptr(), B, acts.data_ptr(), acts.numel(),
                                                       self.sums.data_ptr(), st, cond, self.recompute, drop, self._objective, distill),
                       "genie_train_forward_distill")
        elif self._objective is None:
            _lib.check(_lib.call_drop(lib, "genie_train_forward", self.recompute, drop, cfg, self.w_table, ids.data_ptr(), lab.data_ptr(), B,
                                      acts.data_ptr(), acts.numel(), self.sums.data_ptr(), st, cond=cond), "genie_train_forward")
        else:   # the same forward, the general loss kernel behind it; every backward call below reads its d logits as before
            _lib.check(lib.genie_train_forward_obj(cfg, self.w_table, ids.data_ptr(), lab.data_ptr(), B, acts.data_ptr(), acts.numel(),
                                                   self.sums.data_ptr(), st, cond, self.recompute, drop, self._objective),
                       "genie_train_forward_obj")
        sums = self.sums.clone()
        self.reducer.reset()
        if self.lora is not None and accumulate:
            self._lora_zero_dw("head")
        _lib.check(_lib.call_recompute(lib, "genie_train_backward_head", self.recompute, cfg, self.w_table, self.wT_table,
                                       self.g_table, B, acts.data_ptr(), ws.data_ptr(), ws.numel(), acc_flag, st),
                   "genie_train_backward_head")
        if self.lora is not None:
            self._lora_project("head", acc_flag)
        ready = self._group_hi.get   # None: the group holds no trainable tensor, nothing of it is exchanged
        if reduce and ready("head") is not None:
            self.reducer.ready(ready("head"))
        L = self.config.num_layers
        for layer in reversed(range(self.layout.stop, L)):   # below `stop` nothing trains: no backward, no recomputation
            if self.lora is not None and accumulate:
                self._lora_zero_dw(layer)
            _lib.check(_lib.call_drop(lib, "genie_train_backward_layer", self.recompute, drop, cfg, self.w_table, self.wT_table,
                                      self.g_table, layer, B, acts.data_ptr(), ws.data_ptr(), ws.numel(), acc_flag, st),
                       "genie_train_backward_layer")
            if self.lora is not None:
                self._lora_project(layer, acc_flag)
            if reduce and ready(layer) is not None:
                self.reducer.ready(ready(layer))
        g = self.g_views.get
        # the action tensors train one by one: without a trainable one the conditioning leaves the embedding backward
        vec_on = vec and cond is not None and any(g(n) is not None for n in ("action_proj.weight", "action_proj.bias", "action_null"))
        ids_on = not vec and cond is not None and g("action_embed.weight") is not None
        if not self.layout.embed:
            pass
        elif vec_on:
            n, d = B * self.config.T, self.config.d_model
            if self._d_rows is None or self._d_rows.shape[0] != 1 + n:
                self._d_rows = torch.empty(1 + n, d, dtype=torch.float32, device=self.params.device)
            if accumulate:   # the table gradient shares the embeddings' accumulate flag: start the scratch from zero instead
                self._d_rows.zero_()
            _lib.check(lib.genie_train_backward_embed_cond(cfg, self.g_table, ids.data_ptr(), B, ws.data_ptr(), ws.numel(),
                                                           acc_flag, st, self._d_rows.data_ptr(), cond),
                       "genie_train_backward_embed_cond")
            g_w, g_b = g("action_proj.weight"), g("action_proj.bias")
            if g_w is not None or g_b is not None:
                if g_w is None:   # the entry point needs a d_weight: a frozen weight's gradient lands in a scratch nobody reads
                    if self._dw_scratch is None:
                        self._dw_scratch = torch.zeros(d, self.config.action_dim, dtype=torch.float32, device=self.params.device)
                    g_w = self._dw_scratch
                _lib.check(lib.genie_action_rows_backward(self.model._action_proj_struct(), cond.vectors.data_ptr(),
                                                          self._d_rows[1:].data_ptr(), n, d, g_w.data_ptr(), _ptr(g_b), acc_flag, st),
                           "genie_action_rows_backward")
            g_null = g("action_null")
            if g_null is not None:
                g_null.add_(self._d_rows[0]) if accumulate else g_null.copy_(self._d_rows[0])
        elif ids_on:
            _lib.check(lib.genie_train_backward_embed_cond(cfg, self.g_table, ids.data_ptr(), B, ws.data_ptr(), ws.numel(),
                                                           acc_flag, st, g("action_embed.weight").data_ptr(), cond),
                       "genie_train_backward_embed_cond")
        else:
            _lib.check(lib.genie_train_backward_embed(cfg, self.g_table, ids.data_ptr(), B, ws.data_ptr(), ws.numel(),
                                                      acc_flag, st), "genie_train_backward_embed")
        if reduce:
            self.reducer.finish()
        loss = sums[0] / sums[2]
        if distill is not None:
            self.last_ce, self.last_kd, self.last_teacher_ce = sums[3] / sums[4], sums[5] / sums[4], sums[6] / sums[4]
            return loss, sums[1] / sums[4]
        if self._objective is None:
            self.last_ce = loss
            return loss, sums[1] / sums[2]
        self.last_ce = sums[3] / sums[4]   # hits and the plain CE are taken over every counted token, whatever its frame weighs
        return loss, sums[1] / sums[4]

    # ------------------------------------------------------------------ clip + AdamW + scheduler (train.py:628-633)
    def grad_sumsq(self):
        self.sumsq.zero_()
        _lib.check(self.lib.genie_sumsq(self.grads.data_ptr(), self.n_train, self.sumsq.data_ptr(),
                                        self.scratch.data_ptr(), self._stream()), "genie_sumsq")
        return self.sumsq

    def current_lr(self):
        return self.base_lr * self.lr_lambda(self.completed_steps)

    def optimizer_step(self):
        self._not_in_ema_scope("optimizer_step")
        world = self.reducer.world
        mult = 1.0 / (world * self.accum)
        ss = self.grad_sumsq()
        lr = self.current_lr()
        clip = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        step = self.completed_steps + 1
        st = self._stream()
        omd = None if self.ema is None else ema_one_minus_decay(self.ema_decay, self.ema_updates + 1, self.ema_warmup)
        for lo, hi, dk, factor in self.adam_runs:
            off = lo * 4
            scalars = (hi - lo, lr * factor, self.betas[0], self.betas[1], self.eps, self.weight_decay if dk else 0.0, step, mult,
                       ss.data_ptr() if clip > 0 else None, clip)
            if omd is None:
                _lib.check(self.lib.genie_adamw_step(
                    self.params.data_ptr() + off, self.grads.data_ptr() + off, self.exp_avg.data_ptr() + off,
                    self.exp_avg_sq.data_ptr() + off, *scalars, st), "genie_adamw_step")
            else:   # the same update and the average's, in one pass over the run
                _lib.check(self.lib.genie_adamw_ema_step(
                    self.params.data_ptr() + off, self.grads.data_ptr() + off, self.exp_avg.data_ptr() + off,
                    self.exp_avg_sq.data_ptr() + off, self.ema.data_ptr() + off, *scalars, omd, st), "genie_adamw_ema_step")
        if self.muon is not None:
            self._muon_step(lr, mult, ss, clip, omd, st)
        self.completed_steps += 1
        if omd is not None:
            self.ema_updates += 1
        self._pack_trained()
        self.model.refresh_weights()  # the module's own 16-bit copies (inference entry points) are stale
        return torch.sqrt(ss[0]) * mult, lr

    def train_step(self, batch):
        """One micro-batch of the reference loop (train.py:604-633); the optimizer runs every
        `gradient_accumulation_steps` calls.  Returns device scalars (no host sync)."""
        self._not_in_ema_scope("train_step")
        is_update = (self._micro + 1) % self.accum == 0
        loss, acc = self.forward_backward(batch["input_ids"], batch["labels"], accumulate=self._micro % self.accum != 0,
                                          reduce=is_update and self.accum == 1, action_ids=batch.get("action_ids"),
                                          action_vectors=batch.get("action_vectors"), action_drop=batch.get("action_drop"),
                                          # (a trainer that does not distil ignores the key, as it ignores every key it does not know)
                                          teacher_logits=batch.get("teacher_logits") if self._distilling else None)
        self._micro += 1
        out = {"loss": loss, "acc": acc}
        if self._objective is not None or self._distilling:
            out["ce"] = self.last_ce
        if self._distilling:
            out["kd"], out["teacher_ce"] = self.last_kd, self.last_teacher_ce
        if is_update:
            if self.accum > 1 and self.reducer.world > 1:  # no_sync() micro-batches: reduce once, after the last
                self.reducer.reset()
                self.reducer.finish()
            out["grad_norm"], out["lr"] = self.optimizer_step()
        return out

    def gradients(self):
        """{state-dict name: gradient view} (shapes of the parameters) of the trainable tensors."""
        return self.g_views

    # ------------------------------------------------------------------ EMA of the weights
    def _not_in_ema_scope(self, what):
        if self._in_ema_scope:
            raise RuntimeError(f"GenieTrainer.{what} inside ema_scope(): the parameters hold the averaged weights")

    def _need_ema(self, what):
        if self.ema is None:
            raise RuntimeError(f"GenieTrainer.{what} needs a trainer built with ema_decay")

    def _swap_ema(self):
        # the trainable prefix alone: a frozen tensor's average is the tensor itself
        _lib.check(self.lib.genie_swap_f32(self.params.data_ptr(), self.ema.data_ptr(), self.n_train, self._stream()), "genie_swap_f32")
        self._pack_trained()
        self.model.refresh_weights()

    @contextlib.contextmanager
    def ema_scope(self):
        """Run `self.model` on the averaged weights: the flat parameter buffer and `self.ema` are exchanged in place (one launch) and the
        16-bit operand copies repacked, so every entry point of the model -- forward, generate, save_pretrained -- sees the average, in
        every precision; on exit (also when the body raises) the same exchange and repack put the raw weights back, bit for bit.
        Training calls inside the scope raise RuntimeError; scopes do not nest."""
        self._need_ema("ema_scope")
        self._not_in_ema_scope("ema_scope")
        self._swap_ema()
        self._in_ema_scope = True
        try:
            yield self.model
        finally:
            self._in_ema_scope = False
            self._swap_ema()

    def ema_state_dict(self):
        """{state-dict name: clone of the averaged weights} in the parameters' shapes, for every tensor: a frozen tensor's average is
        the tensor itself."""
        self._need_ema("ema_state_dict")
        if self.lora is not None and not self._in_ema_scope:   # an adapted weight's average is merge(W0, averaged adapters): made by the scope
            with self.ema_scope():
                return self.ema_state_dict()
        avg = self.params if self._in_ema_scope else self.ema   # inside the scope the two buffers have changed places
        src = lambda n: avg if n in self.g_views else self.params   # noqa: E731
        return {n: src(n)[self.offsets[n][0]:self.offsets[n][1]].view(self._shapes[n]).clone() for n in self.order}

    def save_ema_pretrained(self, save_directory):
        """`model.save_pretrained(save_directory)` with the averaged weights: STMaskGIT.from_pretrained loads it as an ordinary checkpoint."""
        self._need_ema("save_ema_pretrained")
        if self._in_ema_scope:
            self.model.save_pretrained(save_directory)
        else:
            with self.ema_scope():
                self.model.save_pretrained(save_directory)

    # ------------------------------------------------------------------ optimizer checkpoint (train.py:560-590 resume)
    def state_dict(self):
        """Optimizer state in torch.optim.AdamW's vocabulary, keyed by parameter NAME (the model's own weights are
        saved by `model.save_pretrained` / `state_dict`)."""
        self._not_in_ema_scope("state_dict")
        st = {}
        for n in self.trainable:   # a frozen tensor has no moments
            lo, hi = self.offsets[n]
            st[n] = {"exp_avg": self.exp_avg[lo:hi].view(self._shapes[n]).clone(),
                     "exp_avg_sq": self.exp_avg_sq[lo:hi].view(self._shapes[n]).clone()}
        out = {"state": st, "completed_steps": self.completed_steps, "micro_step": self._micro,
               "trainable": sorted(self.trainable),
               "dropout": {"seed": self.dropout_seed, "call": self._drop_call},
               "hyper": {"lr": self.base_lr, "betas": tuple(self.betas), "eps": self.eps,
                         "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm,
                         "gradient_accumulation_steps": self.accum, "recompute": bool(self.recompute),
                         "label_smoothing": self.label_smoothing, "z_loss": self.z_loss, "frame_weights": self.frame_weights,
                         "lr_scale": self.lr_scale}}
        if self.muon is not None:   # (a trainer on AdamW alone keeps the state of before, key for key)
            out["muon"] = dict(self.muon.settings_dict(), names=list(self.muon_names))
        if self._distilling:   # (a trainer that does not distil keeps the state of before, key for key)
            out["hyper"].update(distill_alpha=self.distill_alpha, distill_temperature=self.distill_temperature)
        if self.ema is not None:
            avg = {n: self.ema[self.offsets[n][0]:self.offsets[n][1]].view(self._shapes[n]).clone() for n in self.trainable}
            out["ema"] = {"state": avg, "updates": self.ema_updates, "decay": self.ema_decay,
                          "warmup": self.ema_warmup}
        return out

    def load_state_dict(self, sd):
        """Inverse of `state_dict` (moments, step counters); hyper-parameters stay those of this trainer (a warning
        names every saved value that differs).  The average: a saved "ema" entry restores `self.ema` and `ema_updates`; a state without
        one loaded into a trainer with EMA restarts the average from the current parameters, and a saved average loaded into a trainer
        without EMA is ignored -- each with a warning."""
        self._not_in_ema_scope("load_state_dict")
        saved_muon = sd.get("muon")
        mine_muon = None if self.muon is None else dict(self.muon.settings_dict(), names=list(self.muon_names))
        norm = lambda d: None if d is None else {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in d.items()}   # noqa: E731
        if norm(saved_muon) != norm(mine_muon):   # an exp_avg range means a Muon momentum on one side and Adam's first moment on the other
            raise ValueError("GenieTrainer.load_state_dict: the state was saved under "
                             + ("AdamW alone" if saved_muon is None else f"Muon settings {saved_muon}") + ", this trainer runs "
                             + ("AdamW alone" if mine_muon is None else f"Muon settings {mine_muon}"))
        saved_ema = sd.get("ema")
        mine = {"lr": self.base_lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm, "gradient_accumulation_steps": self.accum,
                "label_smoothing": self.label_smoothing, "z_loss": self.z_loss, "frame_weights": self.frame_weights,
                "lr_scale": self.lr_scale, "distill_alpha": self.distill_alpha, "distill_temperature": self.distill_temperature}
        diff = {k: (v, mine[k]) for k, v in (sd.get("hyper") or {}).items()
                if k in mine and (tuple(v) if isinstance(v, (list, tuple)) else v) != mine[k]}
        if saved_ema is not None and self.ema is not None:
            for k, cur in (("decay", self.ema_decay), ("warmup", self.ema_warmup)):
                if saved_ema.get(k) != cur:
                    diff["ema_" + k] = (saved_ema.get(k), cur)
        if diff:
            warnings.warn("GenieTrainer.load_state_dict: resuming with different hyper-parameters (saved, current): "
                          + ", ".join(f"{k}={a}->{b}" for k, (a, b) in diff.items()))
        # the names trainable on both sides are restored; a tensor that was frozen when the state was saved starts from zero moments
        saved = set(sd["state"])
        only_saved, only_here = sorted(saved - set(self.trainable)), [n for n in self.trainable if n not in saved]
        if only_saved or only_here:
            warnings.warn("GenieTrainer.load_state_dict: resuming with a different selection of trainable tensors: "
                          f"{len(only_saved)} saved ones are frozen here and their state is ignored ({', '.join(only_saved[:4])}"
                          f"{', ...' if len(only_saved) > 4 else ''}); {len(only_here)} trainable here were frozen there and start from "
                          f"zero moments ({', '.join(only_here[:4])}{', ...' if len(only_here) > 4 else ''})")
        for n in self.trainable:
            lo, hi = self.offsets[n]
            if n in saved:
                self.exp_avg[lo:hi].copy_(sd["state"][n]["exp_avg"].reshape(-1))
                self.exp_avg_sq[lo:hi].copy_(sd["state"][n]["exp_avg_sq"].reshape(-1))
            else:
                self.exp_avg[lo:hi].zero_()
                self.exp_avg_sq[lo:hi].zero_()
        self.completed_steps = int(sd["completed_steps"])
        self._micro = int(sd.get("micro_step", 0))
        if "dropout" in sd:   # the masks of the resumed run are those the saved one would have drawn next
            self.dropout_seed, self._drop_call = int(sd["dropout"]["seed"]), int(sd["dropout"]["call"])
        if self.ema is not None:
            if saved_ema is None:
                warnings.warn("GenieTrainer.load_state_dict: the saved state has no EMA of the weights: the average restarts from the "
                              "current parameters")
                self.ema.copy_(self.params[:self.n_train])
                self.ema_updates = 0
            else:
                for n in self.trainable:   # a tensor without a saved average (frozen there) restarts its own from the parameter
                    lo, hi = self.offsets[n]
                    self.ema[lo:hi].copy_(saved_ema["state"][n].reshape(-1) if n in saved_ema["state"] else self.params[lo:hi])
                self.ema_updates = int(saved_ema["updates"])
        elif saved_ema is not None:
            warnings.warn("GenieTrainer.load_state_dict: the saved state carries an EMA of the weights, this trainer keeps none: ignored")
        self.pack_weights()
