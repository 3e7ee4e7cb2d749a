"""Yardsticks of the distillation tests (tests/test_train_distill_cpu.py, tests/test_hip_train_distill.py), written without the library:
the contract of include/genie_hip.h ("Distillation") in NumPy, and a float64 torch-autograd training step.

    ce_distill(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, alpha, tau, eps, zeta, weights)      float64: (d logits, seven sums)
    ce_distill_f32(... the same ...)                                                                     f32, in the kernel's order
    forward_logits(cfg, sd, ids)                                                                         float64 logits (B, T, S, V)
    autograd_step(cfg, sd, ids, labels, teacher_logits, alpha, tau, eps, zeta, weights, masks, p)        (loss, grads, ce, acc, kd, teacher_ce)

ce_distill works from the closed forms; autograd_step builds the loss from F.kl_div(log_softmax(z / tau), softmax(u / tau)) * tau^2,
F.cross_entropy(label_smoothing=eps) and zeta * logsumexp^2 and lets autograd differentiate it; tests/test_train_distill_cpu.py holds one
against the other.  ce_distill_f32 restates ce_distill_kernel (csrc/kernels_loss.hip) operation by operation in float32 -- lane l owns
classes l + 64 j, summed j ascending, then the xor butterfly over the 64 lanes -- with NumPy's exp and log in place of the device's: it
carries the roundings of the soft term that the neutral kernel does not have.
"""
import numpy as np

import dropout_model as DM
import objective_model as OM

# The step settings of the GPU tests: tag -> (alpha, tau, with the three objective knobs of objective_model.settings(name)["all"])
STEP_SETTINGS = {"a1t1": (1.0, 1.0, False), "a05t2": (0.5, 2.0, False), "a05t2+obj": (0.5, 2.0, True)}
# The teachers of the step cases: name -> (num_heads, d_model, num_layers, qk_norm): another width and depth than the student's
TEACHERS = {"ln3": (2, 128, 2, False), "qk3": (2, 64, 2, False)}


def step_setting(name, tag):
    """(alpha, tau, eps, zeta, weights) of a step setting for case `name`."""
    alpha, tau, knobs = STEP_SETTINGS[tag]
    eps, zeta, weights = OM.settings(name)["all"] if knobs else (0.0, 0.0, None)
    return alpha, tau, eps, zeta, weights


def _targets(labels, N, vf, nfac):
    lab = np.asarray(labels, dtype=np.int64).reshape(N)
    return np.stack([(lab // vf ** f) % vf for f in range(nfac)], axis=1)


def ce_distill(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, alpha=0.0, tau=1.0, eps=0.0, zeta=0.0, weights=None):
    """The contract in float64.  alpha, tau, eps, zeta are taken as the f32 values the library receives.  Returns (d logits (N, nfac * vf),
    sums (7,) = [sum w l, sum hits, W, sum plain nll, n, sum plain kd, sum teacher plain nll])."""
    alpha, tau, eps, zeta = (float(np.float32(v)) for v in (alpha, tau, eps, zeta))
    z = np.asarray(logits, dtype=np.float64).reshape(-1, nfac, vf)
    u = np.asarray(teacher, dtype=np.float64).reshape(-1, nfac, vf)
    N = z.shape[0]
    counted = OM.counted_mask(ids, T, S, mask_id)
    w = OM.frame_weights(weights, T)
    c_t = counted.sum(axis=(0, 2)).astype(np.float64)
    W, n = float((w * c_t).sum()), float(c_t.sum())
    wn = np.broadcast_to(w[None, :, None], counted.shape).reshape(N)
    counted = counted.reshape(N)
    y = _targets(labels, N, vf, nfac)

    def log_softmax(a):
        a = a - a.max(-1, keepdims=True)
        return a - np.log(np.exp(a).sum(-1, keepdims=True))
    lp, lpt, lr, lq = log_softmax(z), log_softmax(z / tau), log_softmax(u / tau), log_softmax(u)
    lse = (z - lp)[..., 0]
    nll = -np.take_along_axis(lp, y[..., None], -1)[..., 0]
    tnll = -np.take_along_axis(lq, y[..., None], -1)[..., 0]
    p, pt, r = np.exp(lp), np.exp(lpt), np.exp(lr)
    kd = tau * tau * (r * (lr - lpt)).sum(-1)
    hard = (1.0 - eps) * nll + eps * (lse - z.mean(-1))
    l = (1.0 - alpha) * hard + alpha * kd + zeta * lse ** 2
    q = np.full_like(z, eps / vf)
    np.put_along_axis(q, y[..., None], (1.0 - eps) + eps / vf, -1)
    dl = (1.0 - alpha) * (p - q) + (2.0 * zeta * lse)[..., None] * p + alpha * tau * (pt - r)
    live = counted & (wn > 0)
    scale = np.zeros(N)
    if W > 0:
        scale[live] = wn[live] / W
    d = dl * scale[:, None, None]
    d[~live] = 0.0
    hits = (z.argmax(-1) == y).all(-1)
    sums = np.array([(wn * l.sum(-1))[live].sum(), float(hits[counted].sum()), W, nll.sum(-1)[counted].sum(), n,
                     kd.sum(-1)[counted].sum(), tnll.sum(-1)[counted].sum()])
    return d.reshape(N, nfac * vf), sums


def _wave_sum(x):
    """Sum over the last axis (vf classes) as a wave takes it, in x's dtype: lane l adds its classes l + 64 j with j ascending from 0.0,
    then the xor butterfly over offsets 32 .. 1 (every lane ends with the same value; lane 0's is returned)."""
    vf = x.shape[-1]
    J = (vf + 63) // 64
    pad = np.zeros(x.shape[:-1] + (J * 64,), x.dtype)
    pad[..., :vf] = x
    pad = pad.reshape(x.shape[:-1] + (J, 64))
    lane = np.zeros(x.shape[:-1] + (64,), x.dtype)
    for j in range(J):
        lane = lane + pad[..., j, :]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[..., idx ^ o]
    return lane[..., 0]


def ce_distill_f32(logits, teacher, ids, labels, T, S, vf, nfac, mask_id, alpha=0.0, tau=1.0, eps=0.0, zeta=0.0, weights=None):
    """ce_distill_kernel restated in float32, operation by operation (see the module docstring).  Returns (d logits f32, sums (7,) f64)."""
    f = np.float32
    alpha, tau, eps, zeta = f(alpha), f(tau), f(eps), f(zeta)
    one = f(1)
    z = np.asarray(logits, dtype=f).reshape(-1, nfac, vf)
    u = np.asarray(teacher, dtype=f).reshape(-1, nfac, vf)
    N = z.shape[0]
    counted = OM.counted_mask(ids, T, S, mask_id)
    w32 = np.ones(T, f) if weights is None else np.asarray(weights, dtype=f)
    c_t = counted.sum(axis=(0, 2)).astype(np.float64)
    W, n = float((w32.astype(np.float64) * c_t).sum()), float(c_t.sum())
    wt = np.broadcast_to(w32[None, :, None], counted.shape).reshape(N)
    counted = counted.reshape(N)
    y = _targets(labels, N, vf, nfac)
    live = counted & (wt > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where(live, (wt.astype(np.float64) / W).astype(f), f(0))
    q_off = eps / f(vf)
    q_on = (one - eps) + q_off
    inv_vf = one / f(vf)
    oma, at, inv_tau = one - alpha, alpha * tau, one / tau
    tau1 = tau == one
    mx, mu = z.max(-1, keepdims=True), u.max(-1, keepdims=True)
    sz = _wave_sum(z)
    zy = np.take_along_axis(z, y[..., None], -1)[..., 0]
    uy = np.take_along_axis(u, y[..., None], -1)[..., 0]
    d, c = z - mx, u - mu
    e = np.exp(d)
    se = _wave_sum(e)
    if tau1:
        et, ru = e, np.exp(c)
        st, su = se, _wave_sum(ru)
        su1 = su
    else:
        su1 = _wave_sum(np.exp(c))
        d, c = d * inv_tau, c * inv_tau
        et, ru = np.exp(d), np.exp(c)
        st, su = _wave_sum(et), _wave_sum(ru)
    log_se, log_su = np.log(se), np.log(su)
    log_st = log_se if tau1 else np.log(st)
    lse = log_se + mx[..., 0]
    nll_f = lse - zy
    tnll_f = ((log_su if tau1 else np.log(su1)) + mu[..., 0]) - uy
    inv, inv_su = one / se, one / su
    inv_st = inv if tau1 else one / st
    zl2 = (f(2) * zeta) * lse
    p = e * inv[..., None]
    pt = p if tau1 else et * inv_st[..., None]
    r = ru * inv_su[..., None]
    kl = _wave_sum(r * ((c - d) - (log_su - log_st)[..., None]))
    q = np.full_like(z, q_off)
    np.put_along_axis(q, y[..., None], q_on, -1)
    g = (oma * (p - q) + zl2[..., None] * p) + at * (pt - r)
    out = g * wgt[:, None, None]
    out[~live] = f(0)
    kd_f = (tau * tau) * kl
    hard_f = (one - eps) * nll_f + eps * (lse - sz * inv_vf)
    loss = np.zeros(N, f)
    nll, kdt, tnll = np.zeros(N, f), np.zeros(N, f), np.zeros(N, f)
    for k in range(nfac):   # the kernel adds the factors in order
        loss = loss + ((oma * hard_f[:, k] + alpha * kd_f[:, k]) + zeta * (lse[:, k] * lse[:, k]))
        nll, kdt, tnll = nll + nll_f[:, k], kdt + kd_f[:, k], tnll + tnll_f[:, k]
    hits = (z.argmax(-1) == y).all(-1)
    sums = np.array([(wt.astype(np.float64) * loss.astype(np.float64))[counted].sum(), float(hits[counted].sum()), W,
                     nll.astype(np.float64)[counted].sum(), n, kdt.astype(np.float64)[counted].sum(), tnll.astype(np.float64)[counted].sum()])
    return out.reshape(N, nfac * vf), sums


def _logits(cfg, t, ids, masks=None, p=0.0):
    """The float64 torch forward of objective_model.autograd_step up to the logits (B, T, S, V); `t`: {name: tensor}."""
    import torch
    F = torch.nn.functional
    B = ids.shape[0]
    T, S, Vf, nv = cfg.T, cfg.S, cfg.factored_vocab_size, cfg.num_factored_vocabs
    x_in = torch.from_numpy(np.asarray(ids, dtype=np.int64)).reshape(B, T, S)
    is_mask = x_in == cfg.image_vocab_size
    safe = torch.where(is_mask, torch.zeros_like(x_in), x_in)
    e = None
    for j in range(nv):
        ej = t[f"token_embed.factored_embeds.{j}.weight"][(safe // Vf ** j) % Vf]
        e = ej if e is None else e + ej
    x = torch.where(is_mask[..., None], t["token_embed.mask_token_embed"][0], e) + t["pos_embed_TSC"]
    for i in range(cfg.num_layers):
        m0 = m1 = None
        if masks is not None:
            m0, m1 = (torch.from_numpy(m.astype(np.float64)).reshape(B, T, S, -1) for m in masks[i])
        x = DM._block(x, t, i, cfg, m0, m1, p)
    if cfg.use_mup:
        x = x * cfg.readout_mult
    return F.linear(x, t["out_x_proj.weight"], t["out_x_proj.bias"]), is_mask


def forward_logits(cfg, sd, ids):
    """Float64 logits (B, T, S, V) of the model `sd` on `ids` (B, T * S), as NumPy: the teacher of the step tests (rounded to f32 there)."""
    import torch
    with torch.no_grad():
        t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in sd.items()}
        return _logits(cfg, t, ids)[0].numpy()


def autograd_step(cfg, sd, ids, labels, teacher_logits, alpha, tau, eps=0.0, zeta=0.0, weights=None, masks=None, p=0.0):
    """(loss, {name: gradient}, plain CE, acc, kd, teacher CE) of the distillation step in float64 torch autograd: per factor
    (1 - alpha) F.cross_entropy(label_smoothing=eps) + alpha tau^2 F.kl_div(log_softmax(z / tau), softmax(u / tau)) + zeta logsumexp^2,
    weighted per frame and divided by the summed weights of the counted tokens.  teacher_logits (B, T, S, V) are taken as given (f32
    values).  The plain CE, accuracy, kd and the teacher's CE are taken over every counted token."""
    import torch
    from oracle import genie_oracle as go
    F = torch.nn.functional
    alpha, tau, eps, zeta = (float(np.float32(v)) for v in (alpha, tau, eps, zeta))
    with torch.enable_grad():   # the package switches autograd off when it is imported
        t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for k, v in sd.items()}
        B = ids.shape[0]
        T, S, Vf, nv = cfg.T, cfg.S, cfg.factored_vocab_size, cfg.num_factored_vocabs
        logits, is_mask = _logits(cfg, t, ids, masks, p)
        fl = logits[:, 1:].reshape(B, T - 1, S, nv, Vf)
        tl = torch.from_numpy(np.asarray(teacher_logits, dtype=np.float64)).reshape(B, T, S, nv, Vf)[:, 1:]
        ft = torch.from_numpy(go.factorize_token_ids(np.asarray(labels, dtype=np.int64).reshape(B, T, S)[:, 1:], nv, Vf))
        flat, tflat, tgt = fl.reshape(-1, Vf), tl.reshape(-1, Vf), ft.reshape(-1)
        hard = F.cross_entropy(flat, tgt, label_smoothing=eps, reduction="none")
        kd = F.kl_div(F.log_softmax(flat / tau, -1), F.softmax(tflat / tau, -1), reduction="none").sum(-1) * tau ** 2
        per = (1.0 - alpha) * hard + alpha * kd + zeta * torch.logsumexp(flat, -1) ** 2
        per = per.reshape(B, T - 1, S, nv).sum(-1)
        plain = F.cross_entropy(flat, tgt, reduction="none").reshape(B, T - 1, S, nv).sum(-1)
        tplain = F.cross_entropy(tflat, tgt, reduction="none").reshape(B, T - 1, S, nv).sum(-1)
        relevant = is_mask[:, 1:]
        w = torch.from_numpy(OM.frame_weights(weights, T))[None, 1:, None]
        W = (w * relevant).sum()
        loss = (per * w * relevant).sum() / W
        loss.backward()
        hits = (fl.argmax(-1) == ft).all(-1)
        nrel = relevant.sum()
        ce = float((plain * relevant).sum().detach() / nrel)
        kd_mean = float((kd.detach().reshape(B, T - 1, S, nv).sum(-1) * relevant).sum() / nrel)
        tce = float((tplain * relevant).sum() / nrel)
        acc = float((hits & relevant).sum() / nrel)
    grads = {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}
    return float(loss.detach()), grads, ce, acc, kd_mean, tce
