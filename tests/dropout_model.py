"""Helpers of the MLP dropout tests (tests/test_train_dropout_cpu.py, tests/test_hip_train_dropout.py): the mask law of
include/genie_hip.h ("MLP dropout") restated in NumPy integers, and a float64 torch-autograd training step that takes masks.

    keep_mask(seed, call, layer, site, n, p)   the n keep bytes of one mask, bit for bit what the kernels draw
    step_masks(cfg, B, seed, call, p)          per layer (m0 (M, hidden), m1 (M, d_model)), token-major rows
    mlp(x, w1, b1, w2, b2, m0, m1, p)          drop(fc2(drop(gelu(fc1(x))))) with given masks (st_transformer.py:22-25)
    autograd_step(cfg, sd, ids, labels, masks, p)   (loss, {name: gradient}) in float64; masks None = no dropout

The step is tests/test_train_long_window_cpu.torch_autograd_step with its own block (oracle/genie_torch_port._block restated with the
two masks in the MLP; the attention is that module's own).
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: four uint32-valued arrays (or scalars) of one shape, key: two; returns four uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & U32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def threshold(p):
    """floor((double)p * 2^32) of the f32 value p, as the library computes it."""
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def keep_mask(seed, call, layer, site, n, p):
    """keep[e] for e in [0, n): word (e % 4) of Philox(counter = (g lo, g hi, layer * 2 + site, call), key = seed) with g = e // 4,
    kept iff word >= threshold(p)."""
    seed = int(seed) & (2 ** 64 - 1)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((g & U32, g >> np.uint64(32), layer * 2 + site, call), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    return (w >= np.uint64(threshold(p))).astype(np.uint8)


def step_masks(cfg, B, seed, call, p):
    """[(m0, m1)] per layer: uint8 (M, hidden) and (M, d_model), rows in token order (b, t, s)."""
    M, d = B * cfg.T * cfg.S, cfg.d_model
    hid = int(d * cfg.mlp_ratio)
    return [(keep_mask(seed, call, l, 0, M * hid, p).reshape(M, hid), keep_mask(seed, call, l, 1, M * d, p).reshape(M, d))
            for l in range(cfg.num_layers)]


def ones_masks(cfg, B):
    M, d = B * cfg.T * cfg.S, cfg.d_model
    return [(np.ones((M, int(d * cfg.mlp_ratio)), np.uint8), np.ones((M, d), np.uint8)) for _ in range(cfg.num_layers)]


def mlp(x, w1, b1, w2, b2, m0, m1, p):
    """st_transformer.py:22-25 with the two draws of its nn.Dropout given: m * value / (1 - p), behind the GELU and behind fc2 + b2."""
    import torch
    F = torch.nn.functional
    h = F.gelu(F.linear(x, w1, b1))
    if m0 is not None:
        h = h * m0 / (1.0 - p)
    t = F.linear(h, w2, b2)
    if m1 is not None:
        t = t * m1 / (1.0 - p)
    return t


def _block(x, sd, i, cfg, m0, m1, p):
    """st_transformer.py:70-83; m0 / m1: (B, T, S, hidden) / (B, T, S, d) float64 tensors or None."""
    import torch
    from oracle import genie_torch_port as tp
    F = torch.nn.functional
    B, T, S, C = x.shape
    q = f"decoder.layers.{i}."
    xs = x.reshape(B * T, S, C)
    u = xs if cfg.qk_norm else F.layer_norm(xs, (C,), sd[q + "norm1.weight"], sd[q + "norm1.bias"], 1e-5)
    xs = xs + tp._attention(u, sd, q + "spatial_attn.", cfg, False)
    xt = xs.reshape(B, T, S, C).transpose(1, 2).reshape(B * S, T, C)
    xt = xt + tp._attention(xt, sd, q + "temporal_attn.", cfg, True)
    x2 = xt.reshape(B, S, T, C).transpose(1, 2)   # back to (B, T, S, C): the masks are indexed by token-major rows
    u = x2 if cfg.qk_norm else F.layer_norm(x2, (C,), sd[q + "norm2.weight"], sd[q + "norm2.bias"], 1e-5)
    bias = (lambda n: sd.get(q + n)) if cfg.mlp_bias else (lambda n: None)
    return x2 + mlp(u, sd[q + "mlp.fc1.weight"], bias("mlp.fc1.bias"), sd[q + "mlp.fc2.weight"], bias("mlp.fc2.bias"), m0, m1, p)


def autograd_step(cfg, sd, ids, labels, masks=None, p=0.0):
    """(loss, {name: gradient}) of the training objective in float64 torch autograd, with the keep masks of step_masks (None: no
    dropout, which all-ones masks with p = 0 reproduce)."""
    import torch
    from oracle import genie_oracle as go
    F = torch.nn.functional
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
            x = _block(x, t, i, cfg, m0, m1, p)
        if cfg.use_mup:
            x = x * cfg.readout_mult
        fl = F.linear(x, t["out_x_proj.weight"], t["out_x_proj.bias"])[:, 1:].reshape(B, T - 1, S, nv, Vf)
        ft = torch.from_numpy(go.factorize_token_ids(np.asarray(labels, dtype=np.int64).reshape(B, T, S)[:, 1:], nv, Vf))
        ce = (torch.logsumexp(fl, -1) - torch.gather(fl, -1, ft[..., None])[..., 0]).sum(-1)
        relevant = is_mask[:, 1:]
        loss = (ce * relevant).sum() / relevant.sum()
        loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}
