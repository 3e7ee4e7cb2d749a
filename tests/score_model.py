"""NumPy restatement of the per-token arithmetic of score_rows_kernel (and of ce_token_major_kernel, whose arithmetic it shares), in f32
and in float64: per factor f (least significant first: target factor f = (id // vf**f) % vf)

    mx = max(v);  se = sum(exp(v - mx));  loss += (log(se) + mx) - v[target factor]

and the first-max-wins argmax the kernel's `hits` counts with.  The f32 form rounds after every operation as the kernel does; it does not
copy the kernel's summation order (lanes, then a butterfly), so its own distance from float64 is what a correct f32 evaluation of these
formulas costs -- the yardstick tests/test_hip_score.py holds the kernel to."""
import numpy as np


def factor_targets(targets, vf, nfac):
    """(...,) int64 ids -> (..., nfac): factor f = (id // vf**f) % vf."""
    t = np.asarray(targets, dtype=np.int64)
    return np.stack([(t // vf ** f) % vf for f in range(nfac)], axis=-1)


def token_nll(logits, targets, vf, nfac, dtype=np.float64):
    """logits (..., nfac * vf), targets (...,) -> the per-token loss (...,) in `dtype` (np.float32: every operation rounds to f32)."""
    lg = np.asarray(logits, dtype=dtype).reshape(np.shape(logits)[:-1] + (nfac, vf))
    tf = factor_targets(targets, vf, nfac)
    loss = np.zeros(lg.shape[:-2], dtype=dtype)
    for f in range(nfac):
        v = lg[..., f, :]
        mx = v.max(-1)
        se = np.exp(v - mx[..., None], dtype=dtype).sum(-1, dtype=dtype)
        tv = np.take_along_axis(v, tf[..., f][..., None], axis=-1)[..., 0]
        loss = (loss + ((np.log(se, dtype=dtype) + mx) - tv)).astype(dtype)
    return loss


def token_hits(logits, targets, vf, nfac):
    """bool (...,): does the first-max-wins argmax of every factor equal the target's factor?  (np.argmax returns the first maximum.)"""
    lg = np.asarray(logits).reshape(np.shape(logits)[:-1] + (nfac, vf))
    return (lg.argmax(-1) == factor_targets(targets, vf, nfac)).all(-1)


def row_scores(logits_NSV, targets_CS, K, vf, nfac, dtype=np.float64):
    """What genie_score_logits returns for rows (N, S, V) against clip targets (N / K, S): (nll (N,) float64 sums of the per-token loss
    in `dtype`, hits (N,) counts, token_nll (N, S) in `dtype`): row i reads the targets of clip i // K."""
    tg = np.repeat(np.asarray(targets_CS), K, axis=0)
    tok = token_nll(logits_NSV, tg, vf, nfac, dtype)
    return tok.astype(np.float64).sum(-1), token_hits(logits_NSV, tg, vf, nfac).sum(-1).astype(np.float64), tok
