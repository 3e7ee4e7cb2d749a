"""NumPy model of decoding a frame in which some tokens are known (include/genie_hip.h, "known tokens"): the start state, the per-clip
re-mask counts, the per-clip mask step and a one-frame loop.  Built on oracle/genie_oracle.py, which it leaves as it is: with no known
tokens every function here reduces to the oracle's.  A token is known when 0 <= known < mask_id."""
import math

import numpy as np

from oracle import genie_oracle as O


def is_known(known, mask_id):
    known = np.asarray(known)
    return (known >= 0) & (known < mask_id)


def start_state(known, mask_id):
    """(tokens, unmasked) a frame starts from: the known token where there is one, the mask id elsewhere; unmasked exactly where known."""
    k = is_known(known, mask_id)
    return np.where(k, known, mask_id).astype(np.int64), k.copy()


def fraction(step, steps):
    """cos(pi/2 * (step+1)/steps) in Python float math: what genie_mask_fraction returns, bit for bit."""
    return math.cos((step + 1) / steps * math.pi / 2)


def counts(steps, M):
    """n re-masked after each non-final step of a clip with M tokens to generate."""
    return [math.ceil(fraction(s, steps) * M) for s in range(steps - 1)]


def mask_step(samples, keys, unmasked, known, step, steps, mask_id, frame):
    """One mask step of a (B, S) frame, in place on samples / unmasked / frame, each clip with its own count.  Non-final: the oracle's
    mask_step row by row with n_b = counts(steps, M_b)[step]; then, as in every step, previously unmasked tokens keep the frame's value
    and the frame takes the samples."""
    B, S = samples.shape
    prev = unmasked.copy()
    if step != steps - 1:
        K = np.zeros(B, dtype=np.int64) if known is None else is_known(known, mask_id).reshape(B, S).sum(1)
        for b in range(B):
            n = counts(steps, S - int(K[b]))[step]
            O.mask_step(samples[b:b + 1], np.asarray(keys)[b:b + 1], unmasked[b:b + 1], n, mask_id)
    samples[prev] = frame[prev]
    frame[...] = samples


def generate_frame(prompt_BTHW, out_t, known, cfg, steps, logits_fn, temperature=0.0, unmask_mode="random", noise=None, uniforms=None):
    """The one-frame loop with known tokens (B, H, W) or None; mutates prompt_BTHW[:, out_t] -> (samples (B, H, W), unmasked (B, S), the
    masked count of every clip after each step).  logits_fn(prompt) -> (B, V, T, H, W) as in oracle.genie_oracle.maskgit_generate."""
    B, T, H, W = prompt_BTHW.shape
    S, mask_id = H * W, cfg.image_vocab_size
    assert np.all(prompt_BTHW[:, out_t:] == mask_id)
    kn = np.full((B, S), mask_id, dtype=np.int64) if known is None else np.asarray(known).reshape(B, S)
    frame, unmasked = start_state(kn, mask_id)
    prompt_BTHW[:, out_t] = frame.reshape(B, H, W)
    masked = []
    samples = None
    for step in range(steps):
        logits = logits_fn(prompt_BTHW)[:, :, out_t]
        s, conf = O.sample_frame(logits, cfg, temperature, None if uniforms is None else uniforms[step])
        samples = s.reshape(B, S).copy()
        keys = None
        if step != steps - 1:
            keys = conf.reshape(B, S) if unmask_mode == "greedy" else np.asarray(noise[step]).reshape(B, S)
        mask_step(samples, keys, unmasked, kn, step, steps, mask_id, frame)
        prompt_BTHW[:, out_t] = frame.reshape(B, H, W)
        masked.append((frame == mask_id).sum(1))
    return samples.reshape(B, H, W), unmasked, masked
