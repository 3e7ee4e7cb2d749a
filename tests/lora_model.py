"""A float64 NumPy model of the LoRA kernels (include/genie_hip.h, "LoRA adapters") and the error bound the tests hold them to.

    merge    W  = W0 + s B A
    project  dA = s B^T dW   (+ old dA)         dB = s dW A^T   (+ old dB)

The bound is derived, not measured: an f32 result that adds n products (each product exact inside an fma, or rounded once) in any order,
multiplies by s once and adds one more term (w0, or the old gradient) differs from the float64 value by at most
(n + 2) * 2^-24 * sum |terms| to first order -- n - 1 additions, the scale, the last addition and one spare for the inputs' products.
`sum |terms|` is |s| * sum_k |x_k y_k| plus the magnitude of the added term, from this model.
"""
import numpy as np

U = 2.0 ** -24


def f64(x):
    return np.asarray(x, np.float64)


def merge(w0, a, b, s):
    """(W, bound) as float64 arrays of shape (out, in)."""
    w0, a, b = f64(w0), f64(a), f64(b)
    r = a.shape[0]
    mag = np.abs(w0) + abs(s) * (np.abs(b) @ np.abs(a))
    return w0 + s * (b @ a), (r + 2) * U * mag


def project(dw, a, b, s, da_old=None, db_old=None):
    """(dA, dB, bound of dA, bound of dB), float64; *_old: what accumulate = 1 adds to (None: accumulate = 0)."""
    dw, a, b = f64(dw), f64(a), f64(b)
    out, in_ = dw.shape
    da = s * (b.T @ dw)
    db = s * (dw @ a.T)
    mag_a = abs(s) * (np.abs(b).T @ np.abs(dw))
    mag_b = abs(s) * (np.abs(dw) @ np.abs(a).T)
    if da_old is not None:
        da, mag_a = da + f64(da_old), mag_a + np.abs(f64(da_old))
    if db_old is not None:
        db, mag_b = db + f64(db_old), mag_b + np.abs(f64(db_old))
    return da, db, (out + 2) * U * mag_a, (in_ + 2) * U * mag_b


def within(got, want, bound, what):
    err = np.abs(f64(got) - want)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "elements beyond the bound; worst ratio",
                           float((err / np.maximum(bound, 1e-300)).max()))
