"""Yardsticks of the training-objective tests (tests/test_train_objective_cpu.py, tests/test_hip_train_objective.py), written without the
library: the contract of include/genie_hip.h ("Training objective") in float64 NumPy, and a float64 torch-autograd training step.

    ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id, eps, zeta, weights)   (d logits, the five sums)
    autograd_step(cfg, sd, ids, labels, eps, zeta, weights, masks=None, p=0.0)      (loss, {name: gradient}, plain CE, acc)

ce_objective works from the formulas (softmax, smoothed target, the 1 + 2 zeta lse factor); autograd_step builds the loss from
F.cross_entropy(label_smoothing=eps, reduction="none") + zeta * logsumexp ** 2 and lets autograd differentiate it: the two share
nothing but the contract, and tests/test_train_objective_cpu.py holds one against the other.
"""
import numpy as np

import dropout_model as DM

# The step cases of the GPU tests: name -> (data seed of tests/test_hip_train_dropout.py::make_case, frame weights, counted tokens per
# frame).  ln3: a zero-weight frame that holds counted tokens.  qk3 takes data seed 2: seed 0 counts tokens in frame 7 only, where the
# weights cancel out of the loss.
STEP_CASES = {
    "ln3": (0, (1.0, 0.0, 0.5, 2.0), [0, 20, 19, 24]),
    "qk3": (2, (1.0, 0.5, 1.0, 1.5, 2.0, 0.0, 3.0, 0.25), [0, 35, 32, 13, 30, 38, 29, 17]),
}
EPS, ZETA = 0.1, 1e-2   # zeta = 1e-4 moves the gradients by 5.6e-4 only: too little for a step test to tell it from zero


def settings(name):
    """{tag: (eps, zeta, weights)}: each knob alone, and all three."""
    w = STEP_CASES[name][1]
    return {"eps": (EPS, 0.0, None), "zeta": (0.0, ZETA, None), "weights": (0.0, 0.0, w), "all": (EPS, ZETA, w)}


def counted_mask(ids, T, S, mask_id):
    """(n_clips, T, S) bool: frame >= 1 and input id == mask id."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, T, S)
    c = ids == mask_id
    c[:, 0] = False
    return c


def frame_weights(weights, T):
    """(T,) float64 of the f32 values the library is handed; None = all ones."""
    if weights is None:
        return np.ones(T, np.float64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    assert w.shape == (T,), (w.shape, T)
    return w


def ce_objective(logits, ids, labels, T, S, vf, nfac, mask_id, eps=0.0, zeta=0.0, weights=None):
    """The contract in float64.  logits (n_clips * T * S, nfac * vf), ids and labels (n_clips * T * S) or any shape of those sizes.
    eps and zeta are taken as the f32 values the library receives.  Returns (d logits (N, nfac * vf) float64, sums (5,) float64 =
    [sum w l, sum hits, W, sum plain nll, n]); rows of uncounted and of zero-weight tokens are zero; W = 0 leaves every row zero."""
    eps, zeta = float(np.float32(eps)), float(np.float32(zeta))
    z = np.asarray(logits, dtype=np.float64).reshape(-1, nfac, vf)
    N = z.shape[0]
    counted = counted_mask(ids, T, S, mask_id)
    w = frame_weights(weights, T)
    c_t = counted.sum(axis=(0, 2)).astype(np.float64)
    W = float((w * c_t).sum())
    n = float(c_t.sum())
    wn = np.broadcast_to(w[None, :, None], counted.shape).reshape(N)
    counted = counted.reshape(N)
    lab = np.asarray(labels, dtype=np.int64).reshape(N)
    y = np.stack([(lab // vf ** f) % vf for f in range(nfac)], axis=1)                     # (N, nfac)
    mx = z.max(-1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))[..., 0]                      # (N, nfac)
    zy = np.take_along_axis(z, y[..., None], -1)[..., 0]
    nll = lse - zy
    l = (1.0 - eps) * nll + eps * (lse - z.mean(-1)) + zeta * lse ** 2
    p = np.exp(z - lse[..., None])
    q = np.full_like(z, eps / vf)
    np.put_along_axis(q, y[..., None], (1.0 - eps) + eps / vf, -1)
    dl = p * (1.0 + 2.0 * zeta * lse)[..., None] - q
    live = counted & (wn > 0)
    scale = np.zeros(N)
    if W > 0:
        scale[live] = wn[live] / W
    d = dl * scale[:, None, None]
    d[~live] = 0.0
    hits = (z.argmax(-1) == y).all(-1)
    sums = np.array([(wn * l.sum(-1))[live].sum(), float(hits[counted].sum()), W, nll.sum(-1)[counted].sum(), n])
    return d.reshape(N, nfac * vf), sums


def autograd_step(cfg, sd, ids, labels, eps=0.0, zeta=0.0, weights=None, masks=None, p=0.0):
    """(loss, {name: gradient}, plain CE, acc) of the training objective in float64 torch autograd: dropout_model.autograd_step up
    to the logits (its block, its optional dropout masks), then per factor F.cross_entropy(label_smoothing=eps, reduction="none")
    + zeta * logsumexp ** 2, weighted per frame and divided by the summed weights of the counted tokens.  The plain CE and the
    accuracy are taken over every counted token.  W = 0: loss NaN, all gradients zero."""
    import torch
    from oracle import genie_oracle as go
    F = torch.nn.functional
    eps, zeta = float(np.float32(eps)), float(np.float32(zeta))
    with torch.enable_grad():   # the package switches autograd off when it is imported
        t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for k, v in sd.items()}
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
        fl = F.linear(x, t["out_x_proj.weight"], t["out_x_proj.bias"])[:, 1:].reshape(B, T - 1, S, nv, Vf)
        ft = torch.from_numpy(go.factorize_token_ids(np.asarray(labels, dtype=np.int64).reshape(B, T, S)[:, 1:], nv, Vf))
        flat, tgt = fl.reshape(-1, Vf), ft.reshape(-1)
        per = F.cross_entropy(flat, tgt, label_smoothing=eps, reduction="none") + zeta * torch.logsumexp(flat, -1) ** 2
        per = per.reshape(B, T - 1, S, nv).sum(-1)
        plain = F.cross_entropy(flat, tgt, reduction="none").reshape(B, T - 1, S, nv).sum(-1)
        relevant = is_mask[:, 1:]
        w = torch.from_numpy(frame_weights(weights, T))[None, 1:, None]
        W = (w * relevant).sum()
        loss = (per * w * relevant).sum() / W
        if float(W) > 0:
            loss.backward()
        hits = (fl.argmax(-1) == ft).all(-1)
        ce = float((plain * relevant).sum().detach() / relevant.sum())
        acc = float((hits & relevant).sum() / relevant.sum())
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in t.items()}
    if float(W) > 0:
        grads = {k: g for k, g in grads.items() if t[k].grad is not None}
    return float(loss.detach()), grads, ce, acc
