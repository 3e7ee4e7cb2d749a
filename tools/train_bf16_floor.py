"""Noise floor of the bf16 training step against its number model (CPU, the bars of tests/test_hip_train_bf16.py).

A bf16 step differs from oracle.genie_train_oracle.BF16_TRAIN by accumulation order, and each order difference that flips a bf16
rounding propagates through the rest of the step.  Its size is measured here on the oracle itself: the distance between BF16_TRAIN
on the case's weights and on the same weights scaled by 1 + 2e-7 N(0, 1) (f32-level noise), over many seeds.  Prints, per case,
p50 / p95 / max over the seeds of the worst-tensor median / max / Frobenius error, the loss error and the global-norm error, and the
distance that switching off the spatial-backward rounding points (bwd_*) alone makes on the spatial-attention tensors.

    python tools/train_bf16_floor.py [--seeds 100] [--jobs 8] [case ...]

A case is an id of tests/test_hip_train_bf16.py (all of them when none is named), train_shape_dh64, or an id of
tests/test_hip_train_long_window.py (T = 32 / 64; only when named).
"""
import argparse
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402

from oracle import genie_train_oracle as TO  # noqa: E402

METRICS = ("median", "max", "fro", "loss", "norm")


def load(name):
    import test_hip_train_bf16 as T
    import test_hip_train_long_window as LW
    if name in LW.CASES:
        return (T,) + LW.make_case(name)
    if name == "train_shape_dh64":
        from conftest import load_golden
        z, cfg, sd = load_golden(name)
        return T, cfg, sd, z["s0_input_ids"], z["s0_labels"]
    return (T,) + T.make_case(name)


def distance(T, g, loss, g2, loss2):
    worst = np.max([T.errors(g2[k], g[k]) for k in g], axis=0)
    gn, gn2 = TO.grad_norm(g), TO.grad_norm(g2)
    return np.array([worst[0], worst[1], worst[2], abs(loss2 - loss), abs(gn2 - gn) / gn])


def one(args):
    name, seed = args
    T, cfg, sd, ids, labels = load(name)
    loss, _, g = TO.forward_backward(ids, labels, sd, cfg, nm=TO.BF16_TRAIN)
    rng = np.random.default_rng(seed)
    sd2 = {k: (v * (1 + 2e-7 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in sd.items()}
    loss2, _, g2 = TO.forward_backward(ids, labels, sd2, cfg, nm=TO.BF16_TRAIN)
    return distance(T, g, loss, g2, loss2)


def bwd16_points(name):
    """Frobenius distance on the spatial-attention gradients when only the bwd_* rounding points are switched off."""
    T, cfg, sd, ids, labels = load(name)
    _, _, g = TO.forward_backward(ids, labels, sd, cfg, nm=TO.BF16_TRAIN)
    nm = TO.BF16_TRAIN
    for p in ("bwd_qk", "bwd_v", "bwd_do", "bwd_p", "bwd_ds"):
        nm = nm.without(p)
    _, _, g2 = TO.forward_backward(ids, labels, sd, cfg, nm=nm)
    return {k: T.errors(g2[k], g[k])[2] for k in g if "spatial_attn" in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    import test_hip_train_bf16 as T
    cases = a.cases or list(T.CASES) + ["train_shape_dh64"]
    from multiprocessing import Pool
    with Pool(a.jobs) as pool:
        for name in cases:
            d = np.array(pool.map(one, [(name, s) for s in range(a.seeds)]))
            print(f"{name}  ({a.seeds} seeds: p50 / p95 / max)")
            for i, m in enumerate(METRICS):
                q = np.percentile(d[:, i], [50, 95, 100])
                print(f"  {m:7s} {q[0]:.2e} / {q[1]:.2e} / {q[2]:.2e}")
            if load(name)[1].S == 256:
                f = bwd16_points(name)
                print(f"  bwd_* points off, spatial-attention Frobenius: {min(f.values()):.2e} .. {max(f.values()):.2e}")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
