"""float64 NumPy model of the sampling law of include/genie_hip.h (genie_sampling): logit temperature, top-k, top-p, inverse-CDF
draw over the kept entries, confidence under the tempered unfiltered softmax, and the "confidence" unmasking key.  Test
infrastructure for tests/test_sampling_cpu.py and tests/test_hip_sampling.py; vectorised over leading axes.

The only f32 step is the one the contract names: z = logit * (1.0f / tau), one f32 multiply.  Top-k is decided on those f32
values (exact); every mass is f64.
"""
import numpy as np

MARGIN = 2e-6   # of the total: the margin of tests/test_hip_parity.py::test_sample_temperature_exact_outside_cdf_margins


def temper(logits, tau):
    """z = logit * (1.0f / tau) in f32."""
    inv = np.float32(1.0) / np.float32(tau)
    return (np.asarray(logits, np.float32) * inv).astype(np.float32)


def stable_rank(z):
    """rank_i = #{j : z_j > z_i or (z_j == z_i and j < i)} along the last axis."""
    order = np.argsort(-z.astype(np.float64), axis=-1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(z.shape[-1]), z.shape).copy(), axis=-1)
    return rank, order


def factor_law(logits, tau=1.0, top_k=0, top_p=1.0):
    """One factored vocabulary (last axis).  Returns a dict:
    z (f32), e = exp(z - max) (f64), kept (bool), rank, order, mass_before (f64, in rank order, normalised over the top-k
    survivors; meaningful for survivors), in_k (bool)."""
    z = temper(logits, tau)
    vf = z.shape[-1]
    zd = z.astype(np.float64)
    e = np.exp(zd - zd.max(-1, keepdims=True))
    rank, order = stable_rank(z)
    k_on = 0 < top_k < vf
    in_k = rank < top_k if k_on else np.ones(z.shape, bool)
    kept = in_k.copy()
    e_sorted = np.take_along_axis(np.where(in_k, e, 0.0), order, -1)
    tot_k = e_sorted.sum(-1, keepdims=True)
    before_sorted = (np.cumsum(e_sorted, -1) - e_sorted) / tot_k       # mass of the survivors ranked strictly before, by rank
    mass_before = np.empty_like(before_sorted)
    np.put_along_axis(mass_before, order, before_sorted, axis=-1)
    if 0.0 < top_p < 1.0:
        kept &= (mass_before < top_p) | (rank == 0)                    # the best entry is always kept
    return dict(z=z, e=e, kept=kept, in_k=in_k, rank=rank, order=order, mass_before=mass_before)


def draw(law, u):
    """Inverse-CDF draw in index order over the kept entries: position = #{kept prefix sums < u * total}, then the kept entry at
    that position (the last kept one at most).  Returns (pick, ambiguous_cdf): ambiguous when the target lies within MARGIN
    (of the total) of a CDF step of the kept entries."""
    kept, e = law["kept"], law["e"]
    ek = np.where(kept, e, 0.0)
    cdf = np.cumsum(ek, -1)
    total = cdf[..., -1]
    target = np.asarray(u, np.float64) * total
    pos = ((cdf < target[..., None]) & kept).sum(-1)
    n_kept = kept.sum(-1)
    pos = np.minimum(pos, n_kept - 1)
    kept_count = np.cumsum(kept, -1)                                    # the kept entry number `pos`: first index with pos + 1 kept
    pick = (kept_count < (pos + 1)[..., None]).sum(-1)
    dist = np.where(kept, np.abs(cdf - target[..., None]), np.inf).min(-1) / total
    return pick, dist < MARGIN


def top_p_ambiguous(law, top_p):
    """With top-p on: the mass before some surviving rank >= 1 lies within MARGIN of top_p."""
    if not (0.0 < top_p < 1.0):
        return np.zeros(law["z"].shape[:-1], bool)
    near = law["in_k"] & (law["rank"] >= 1) & (np.abs(law["mass_before"] - top_p) < MARGIN)
    return near.any(-1)


def widened_kept(law, top_p):
    """The kept set plus every top-k survivor whose top-p decision lies within MARGIN of the bar (what an f32 mass may flip)."""
    if not (0.0 < top_p < 1.0):
        return law["kept"]
    return law["kept"] | (law["in_k"] & (np.abs(law["mass_before"] - top_p) < MARGIN))


def sample(logits, uniforms, vf, tau=1.0, top_k=0, top_p=1.0, temperature=1.0):
    """logits (..., nv * vf), uniforms (nv, ...) in draw order (most significant vocabulary first).  Returns a dict:
    ids (hi * vf + lo ...), conf (f64, tempered unfiltered softmax of the picks), ambiguous (bool), inside (bool: every pick
    lies in its widened kept set -- trivially true here), picks, laws."""
    logits = np.asarray(logits)
    nv = logits.shape[-1] // vf
    ids = np.zeros(logits.shape[:-1], np.int64)
    conf = np.ones(logits.shape[:-1])
    ambiguous = np.zeros(logits.shape[:-1], bool)
    picks, laws = [], []
    for k, f in enumerate(range(nv - 1, -1, -1)):
        law = factor_law(logits[..., f * vf:(f + 1) * vf], tau, top_k, top_p)
        if temperature > 1e-8:
            pick, amb = draw(law, uniforms[k])
            ambiguous |= amb | top_p_ambiguous(law, top_p)
        else:
            pick = law["z"].argmax(-1)                                  # first maximum wins; no filter changes it
        ids = ids * vf + pick
        conf *= np.take_along_axis(law["e"], pick[..., None], -1)[..., 0] / law["e"].sum(-1)
        picks.append(pick)
        laws.append(law)
    return dict(ids=ids, conf=conf, ambiguous=ambiguous, picks=picks, laws=laws)


def filtered_probs(logits, tau=1.0, top_k=0, top_p=1.0):
    """The filtered, tempered distribution of one factor (sums to 1 over the kept entries)."""
    law = factor_law(logits, tau, top_k, top_p)
    p = np.where(law["kept"], law["e"], 0.0)
    return p / p.sum(-1, keepdims=True), law["kept"]


def confidence_keys(conf, noise, c, step, steps):
    """log(conf) + c * (1 - (step + 1) / steps) * g, g = -log(-log(u)), u clamped to [2^-24, 1 - 2^-24]."""
    u = np.clip(np.asarray(noise, np.float64), 2.0 ** -24, 1.0 - 2.0 ** -24)
    g = -np.log(-np.log(u))
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(conf, np.float64)) + c * (1.0 - (step + 1) / steps) * g


def plain_inverse_cdf(logits, uniforms, vf):
    """The model of test_sample_temperature_exact_outside_cdf_margins (no law): ids and the ambiguous mask."""
    nv = logits.shape[-1] // vf
    ids = np.zeros(logits.shape[:-1], np.int64)
    ambiguous = np.zeros(logits.shape[:-1], bool)
    for k, f in enumerate(range(nv - 1, -1, -1)):
        l = logits[..., f * vf:(f + 1) * vf].astype(np.float64)
        e = np.exp(l - l.max(-1, keepdims=True))
        tot = e.sum(-1)
        cdf = np.cumsum(e, -1)
        target = uniforms[k].astype(np.float64) * tot
        pick = np.minimum((cdf < target[..., None]).sum(-1), vf - 1)
        ambiguous |= (np.abs(cdf - target[..., None]).min(-1) / tot) < MARGIN
        ids = ids * vf + pick
    return ids, ambiguous
