"""NumPy f32 restatement of the EMA of the weights (include/genie_hip.h, "EMA of the weights"; reference: magvit2/modules/ema.py,
LitEma.forward): the schedule, one update, and the replay over a recorded parameter sequence.  Every operation is one f32 operation
rounded on its own, which is what the kernels compute with __fsub_rn / __fmul_rn.  No GPU, no torch."""
import numpy as np

F32 = np.float32


def decay_at(decay, n, warmup=False):
    """d_n of update n = 1, 2, ...: float32(decay), or with warm-up min(float32(decay), float32(1 + n) / float32(10 + n))."""
    d = F32(decay)
    if warmup:
        d = min(d, F32(1 + n) / F32(10 + n))
    return F32(d)


def one_minus_decay(decay, n, warmup=False):
    return F32(F32(1) - decay_at(decay, n, warmup))


def update(ema, params, omd):
    """ema - (omd * (ema - params)), three f32 operations; returns a new array."""
    ema, params, omd = np.asarray(ema, F32), np.asarray(params, F32), F32(omd)
    with np.errstate(under="ignore"):
        diff = (ema - params).astype(F32)
        step = (omd * diff).astype(F32)
        return (ema - step).astype(F32)


def replay(start, sequence, decay, warmup=False):
    """The average after each update: it starts as `start`, update n = 1 .. len(sequence) sees sequence[n - 1]."""
    ema, out = np.asarray(start, F32).copy(), []
    for n, p in enumerate(sequence, 1):
        ema = update(ema, p, one_minus_decay(decay, n, warmup))
        out.append(ema)
    return out
