"""NumPy restatement of the Muon step (include/genie_hip.h, "Muon", steps 1 to 10) and of a whole optimizer step that mixes Muon and
AdamW tensors, in float64 (the reference) or float32 (what the rounding of the format alone costs).  Imports nothing from the package."""
import math

import numpy as np

DEFAULT_COEFFICIENTS = (3.4445, -4.7750, 2.0315)


def clip_coef(sumsq, grad_mult=1.0, max_norm=0.0, dtype=np.float64):
    """grad_mult * min(1, max_norm / (grad_mult * sqrt(sumsq) + 1e-6)); max_norm <= 0 or sumsq None: grad_mult alone."""
    t = dtype
    coef = t(grad_mult)
    if sumsq is not None and max_norm > 0:
        tn = t(math.sqrt(sumsq)) * t(grad_mult)
        coef = coef * min(t(1.0), t(max_norm) / (tn + t(1e-6)))
    return t(coef)


def newton_schulz(u, steps=5, coefficients=DEFAULT_COEFFICIENTS, eps=1e-7, dtype=np.float64):
    """Steps 4 to 7 on one (rows, cols) matrix."""
    t = dtype
    a, b, c = (t(v) for v in coefficients)
    x = np.asarray(u, dtype=t)
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    nrm = t(math.sqrt(float(np.sum(x.astype(np.float64) ** 2)))) if t is np.float32 else np.sqrt(np.sum(x * x))
    x = x / max(nrm, t(eps))
    for _ in range(steps):
        g = x @ x.T
        p = b * g + c * (g @ g)
        x = a * x + p @ x
    return np.ascontiguousarray(x.T if tall else x).astype(t)


def adjust(mode, rows, cols):
    return 0.2 * math.sqrt(max(rows, cols)) if mode == "match_rms_adamw" else math.sqrt(max(1.0, rows / cols))


def momentum_update(g, buf, coef, mu=0.95, nesterov=True, dtype=np.float64):
    """Steps 1 to 3: returns (u, new B)."""
    t = dtype
    gi = np.asarray(g, dtype=t) * t(coef)
    b = t(mu) * np.asarray(buf, dtype=t) + gi
    return (gi + t(mu) * b if nesterov else b), b


def muon_matrix(w, g, buf, lr, weight_decay=0.0, coef=1.0, mu=0.95, nesterov=True, steps=5, coefficients=DEFAULT_COEFFICIENTS, eps=1e-7,
                adjust_lr="match_rms_adamw", dtype=np.float64):
    """Steps 1 to 9 on one matrix: returns (new W, new B, O)."""
    t = dtype
    u, b = momentum_update(g, buf, coef, mu, nesterov, t)
    o = newton_schulz(u, steps, coefficients, eps, t)
    rows, cols = o.shape
    decay, s = t(1.0 - lr * weight_decay), t(lr * adjust(adjust_lr, rows, cols))
    return np.asarray(w, dtype=t) * decay - s * o, b, o


def blocks(name, shape):
    """[(first row, rows)] of the matrices one weight holds: a fused qkv weight is q, k and v."""
    rows = shape[0]
    if name.endswith(".qkv.weight"):
        return [(i * (rows // 3), rows // 3) for i in range(3)]
    return [(0, rows)]


def ema_line(ema, p, omd, dtype=np.float64):
    t = dtype
    e = np.asarray(ema, dtype=t)
    return e - t(omd) * (e - np.asarray(p, dtype=t))


def adamw_tensor(w, g, m, v, lr, weight_decay, step, coef=1.0, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
    """torch.optim.AdamW on one tensor: returns (new W, m, v)."""
    t = dtype
    gi = np.asarray(g, dtype=t) * t(coef)
    m = t(betas[0]) * np.asarray(m, dtype=t) + t(1 - betas[0]) * gi
    v = t(betas[1]) * np.asarray(v, dtype=t) + t(1 - betas[1]) * gi * gi
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    denom = np.sqrt(v) * t(1.0 / math.sqrt(bc2)) + t(eps)
    return np.asarray(w, dtype=t) * t(1.0 - lr * weight_decay) - t(lr / bc1) * (m / denom), m, v


class MixedOptimizer:
    """A whole optimizer step over {name: array}: Muon on `muon_names` (a fused qkv weight as three matrices), AdamW on the rest, one
    global clip over all gradients.  Carries its own state (momentum / moments, step count, optional EMA)."""

    def __init__(self, params, muon_names, lr, weight_decay=0.0, max_norm=1.0, decays=lambda n: True, lr_factor=None, mu=0.95, nesterov=True,
                 steps=5, coefficients=DEFAULT_COEFFICIENTS, eps=1e-7, adjust_lr="match_rms_adamw", ema_omd=None, dtype=np.float64):
        self.t = dtype
        self.p = {n: np.asarray(v, dtype=dtype).copy() for n, v in params.items()}
        self.muon_names = set(muon_names)
        self.lr, self.wd, self.max_norm, self.decays, self.lr_factor = lr, weight_decay, max_norm, decays, lr_factor or {}
        self.kw = dict(mu=mu, nesterov=nesterov, steps=steps, coefficients=coefficients, eps=eps, adjust_lr=adjust_lr)
        self.m = {n: np.zeros_like(v) for n, v in self.p.items()}
        self.v = {n: np.zeros_like(v) for n, v in self.p.items()}
        self.ema = None if ema_omd is None else {n: v.copy() for n, v in self.p.items()}
        self.ema_omd, self.step_count = ema_omd, 0

    def step(self, grads, grad_mult=1.0):
        """grads: {name: array} for every parameter that trains (the others are left alone)."""
        t = self.t
        self.step_count += 1
        sumsq = float(sum(np.sum(np.asarray(g, dtype=np.float64) ** 2) for g in grads.values()))
        coef = clip_coef(sumsq, grad_mult, self.max_norm or 0.0, t)
        for n, g in grads.items():
            lr = self.lr * self.lr_factor.get(n, 1.0)
            wd = self.wd if self.decays(n) else 0.0
            if n in self.muon_names:
                for r0, rows in blocks(n, self.p[n].shape):
                    sl = slice(r0, r0 + rows)
                    self.p[n][sl], self.m[n][sl], _ = muon_matrix(self.p[n][sl], g[sl], self.m[n][sl], lr, wd, coef, dtype=t, **self.kw)
            else:
                self.p[n], self.m[n], self.v[n] = adamw_tensor(self.p[n], g, self.m[n], self.v[n], lr, wd, self.step_count, coef, dtype=t)
            if self.ema is not None:
                self.ema[n] = ema_line(self.ema[n], self.p[n], self.ema_omd, t)
        return math.sqrt(sumsq) * grad_mult
