"""Muon on the hidden weight matrices (include/genie_hip.h, "Muon"; Jordan et al. 2024; counterpart: torch.optim.Muon).

Momentum, then a Newton-Schulz orthogonalisation of each target matrix's update, in f32 on the matrix cores (genie_muon_step); every
other tensor stays on AdamW.  What is here is the host side the trainer (1xgpt_amd/train.py) uses: the settings, target selection, the
q / k / v split of a fused qkv weight, the item tables and their chunks.  No model math: there is no CPU fallback for the kernels.
"""
import fnmatch
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .lora import linear_weight_names

DEFAULT_COEFFICIENTS = (3.4445, -4.7750, 2.0315)


@dataclass
class MuonConfig:
    """momentum: mu in [0, 1); nesterov; ns_steps: 0 .. 99 iterations; ns_coefficients: (a, b, c) of p(s) = a s + b s^3 + c s^5; eps: floor of
    the Frobenius norm; adjust_lr: "match_rms_adamw" (lr * 0.2 sqrt(max(rows, cols)): one schedule serves both optimizers) or "original"
    (lr * sqrt(max(1, rows / cols))); targets: fnmatch patterns over `linear_weight_names(config)` (a list or one comma-separated string;
    "decoder.layers.*" = the six Linears of every layer; the readout "out_x_proj.weight" is eligible, not in the default)."""
    momentum: float = 0.95
    nesterov: bool = True
    ns_steps: int = 5
    ns_coefficients: tuple = DEFAULT_COEFFICIENTS
    eps: float = 1e-7
    adjust_lr: str = "match_rms_adamw"
    targets: object = "decoder.layers.*"

    def __post_init__(self):
        self.momentum = float(self.momentum)
        if not 0.0 <= self.momentum < 1.0:   # (False for NaN)
            raise ValueError(f"MuonConfig.momentum must be in [0, 1), got {self.momentum!r}")
        self.nesterov = bool(self.nesterov)
        if isinstance(self.ns_steps, bool) or not isinstance(self.ns_steps, (int, np.integer)) or not 0 <= int(self.ns_steps) < 100:
            raise ValueError(f"MuonConfig.ns_steps must be an integer in 0 .. 99, got {self.ns_steps!r}")
        self.ns_steps = int(self.ns_steps)
        try:
            coef = tuple(float(v) for v in self.ns_coefficients)
        except TypeError:
            coef = ()
        if len(coef) != 3 or not all(math.isfinite(v) for v in coef):
            raise ValueError(f"MuonConfig.ns_coefficients must be three finite numbers, got {self.ns_coefficients!r}")
        self.ns_coefficients = coef
        self.eps = float(self.eps)
        if not (self.eps > 0.0 and math.isfinite(self.eps)):
            raise ValueError(f"MuonConfig.eps must be finite and > 0, got {self.eps!r}")
        if self.adjust_lr not in _lib.MUON_ADJUST:
            raise ValueError(f"MuonConfig.adjust_lr must be one of {sorted(_lib.MUON_ADJUST)}, got {self.adjust_lr!r}")
        pats = [q for q in self.targets.split(",") if q] if isinstance(self.targets, str) else list(self.targets or ())
        if not pats or not all(isinstance(q, str) for q in pats):
            raise ValueError(f"MuonConfig.targets needs at least one pattern, got {self.targets!r}")
        self.targets = pats

    def settings_dict(self):
        """What `GenieTrainer.state_dict` carries and `load_state_dict` compares."""
        return {"momentum": self.momentum, "nesterov": self.nesterov, "ns_steps": self.ns_steps,
                "ns_coefficients": tuple(self.ns_coefficients), "eps": self.eps, "adjust_lr": self.adjust_lr}


def select_targets(config, patterns):
    """The targeted Linear weight names, in `linear_weight_names` order.  ValueError for a pattern that matches none of them."""
    names = linear_weight_names(config)
    hit = set()
    for p in patterns:
        m = [n for n in names if fnmatch.fnmatchcase(n, p)]
        if not m:
            raise ValueError(f"muon target pattern {p!r} matches no Linear weight (linear_weight_names)")
        hit.update(m)
    return [n for n in names if n in hit]


def muon_names(config, patterns, trainable):
    """The Muon tensors: the targets that train.  A frozen target (the base weight of a LoRA-adapted Linear included) is skipped;
    ValueError when nothing is left."""
    chosen = [n for n in select_targets(config, patterns) if n in trainable]
    if not chosen:
        raise ValueError("no trainable tensor is left for Muon: every target its patterns select is frozen")
    return chosen


def blocks(name, shape):
    """[(first row, rows, cols)] of the matrices one weight holds: a fused qkv weight (3d, d) is q, k and v, orthogonalised separately."""
    rows, cols = shape
    if name.endswith(".qkv.weight"):
        assert rows % 3 == 0, (name, shape)
        return [(i * (rows // 3), rows // 3, cols) for i in range(3)]
    return [(0, rows, cols)]


def adjust(mode, rows, cols):
    """adj of step 9."""
    return 0.2 * math.sqrt(max(rows, cols)) if mode == "match_rms_adamw" else math.sqrt(max(1.0, rows / cols))


def item(rows, cols, param, grad, momentum, ema=None, lr=0.0, weight_decay=0.0):
    """One genie_muon_item from device pointers (integers; ema None = no average)."""
    return _lib.MuonItem(param=param, grad=grad, momentum=momentum, ema=ema, rows=rows, cols=cols, lr=lr, weight_decay=weight_decay)


def chunks(entries, n=_lib.MUON_MAX_ITEMS):
    """Sort (stably) by shape and cut into tables of at most GENIE_MUON_MAX_ITEMS: equal shapes share the launches of a table, and the
    launch count of a step grows with the number of matrices only through ceil(items / n).  `entries`: objects with .rows and .cols."""
    by_shape = sorted(entries, key=lambda e: (e.rows, e.cols))
    return [by_shape[i:i + n] for i in range(0, len(by_shape), n)]


def table(items):
    """(ctypes array, n) of a list of MuonItem, at most GENIE_MUON_MAX_ITEMS."""
    assert 1 <= len(items) <= _lib.MUON_MAX_ITEMS, len(items)
    return (_lib.MuonItem * len(items))(*items), len(items)


def settings(cfg, grad_mult=1.0, grad_sumsq=None, max_grad_norm=0.0, ema_one_minus_decay=0.0):
    """The genie_muon_settings of a MuonConfig and one step's scalars (grad_sumsq: a device pointer or None)."""
    a, b, c = cfg.ns_coefficients
    return _lib.MuonSettings(momentum=cfg.momentum, a=a, b=b, c=c, eps=cfg.eps, grad_mult=grad_mult, max_grad_norm=max_grad_norm,
                             ema_one_minus_decay=ema_one_minus_decay, nesterov=int(cfg.nesterov), ns_steps=cfg.ns_steps,
                             adjust=_lib.MUON_ADJUST[cfg.adjust_lr], reserved=0, grad_sumsq=grad_sumsq)


def launches(items, ns_steps):
    """The kernel launches of one optimizer step's Muon part for these items (objects with .rows, .cols): per table of `chunks`, momentum,
    normalise and apply, and 3 * ns_steps products per distinct shape."""
    return sum(3 + 3 * ns_steps * len({(e.rows, e.cols) for e in part}) for part in chunks(items))
