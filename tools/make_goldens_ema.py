#!/usr/bin/env python3
"""Generate tests/golden/ema_litema.npz by driving the REFERENCE's own LitEma (magvit2/modules/ema.py) on the CPU.

Build-container only, like the other tools/make_goldens*.py: /root/reference does not exist on the GPU box, so the arrays are
committed and this script documents how they were made.  Nothing of the reference's source is copied; only inputs and what it computed.
LitEma is loaded by file path (importlib.util.spec_from_file_location), so magvit2/__init__ and its imports are not pulled in.

A module of three f32 parameters of 5, 130 and 1027 elements ("a", "blk.w", "blk.sub.v": the dotted names take LitEma's own renaming)
is given a recorded sequence of 1 + 12 parameter states; LitEma is built on state 0 and called after each of states 1 .. 12.  Decays
0.999 and 0.9, each with and without use_num_upates.  The states hold zeros, elements that become zero, values near 1e-38 that move by
about 1e-41 (the difference and its product with 1 - decay are denormal), values near 1e30, and a tensor that never moves.
Stored: p0 / p1 / p2 (13, n) the states; per configuration TAG in d999 / d999w / d9 / d9w: TAG_s0 / _s1 / _s2 (12, n) the shadow after
every update and TAG_d (12,) the decay LitEma used (its own expression over its own buffers, evaluated after the call); decays, warm.
tests/test_train_ema_cpu.py holds tests/ema_model.py to these arrays bit for bit, tests/test_hip_train_ema.py the kernels.
"""
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EMA = "/root/reference/magvit2/modules/ema.py"
OUT = os.path.join(REPO, "tests", "golden", "ema_litema.npz")
SIZES, UPDATES = (5, 130, 1027), 12
CONFIGS = {"d999": (0.999, False), "d999w": (0.999, True), "d9": (0.9, False), "d9w": (0.9, True)}


def sequence():
    g = np.random.default_rng(20261)
    a = np.tile(np.array([0.0, 1.5, -2.25, 1e-3, -7.0], np.float32), (UPDATES + 1, 1))          # never moves
    b = np.empty((UPDATES + 1, SIZES[1]), np.float32)
    b[0] = g.standard_normal(SIZES[1]) * 0.5
    b[0, :16] = 0.0                                                                              # zero throughout
    for n in range(1, UPDATES + 1):
        b[n] = b[n - 1] - np.float32(0.05) * g.standard_normal(SIZES[1]).astype(np.float32)
        b[n, :16] = 0.0
        if n >= 5:
            b[n, 16:32] = 0.0                                                                    # becomes zero at update 5
    c = np.empty((UPDATES + 1, SIZES[2]), np.float32)
    c[0] = g.standard_normal(SIZES[2]) * 0.02
    c[0, :64] = np.float32(1e-38) * (1 + g.random(64)).astype(np.float32)
    c[0, 64:128] = np.float32(1e30) * g.standard_normal(64).astype(np.float32)
    for n in range(1, UPDATES + 1):
        c[n] = c[n - 1] - np.float32(1e-3) * g.standard_normal(SIZES[2]).astype(np.float32)
        c[n, :64] = c[n - 1, :64] + np.float32(1e-41) * g.standard_normal(64).astype(np.float32)
        c[n, 64:128] = c[n - 1, 64:128] * np.float32(1.01)
        c[n, 128:160] = c[0, 128:160]                                                            # a stretch that never moves
    return [a, b, c]


class Sub(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.v = torch.nn.Parameter(torch.zeros(n))


class Blk(torch.nn.Module):
    def __init__(self, n, m):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(n))
        self.sub = Sub(m)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(SIZES[0]))
        self.blk = Blk(SIZES[1], SIZES[2])


def main():
    spec = importlib.util.spec_from_file_location("reference_ema", REF_EMA)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seq = sequence()
    names = ["a", "blk.w", "blk.sub.v"]
    out = {f"p{k}": s for k, s in enumerate(seq)}
    out["decays"] = np.array([0.999, 0.9], np.float64)
    for tag, (decay, warm) in CONFIGS.items():
        net = Net()
        params = dict(net.named_parameters())
        assert list(params) == names and [p.numel() for p in params.values()] == list(SIZES)
        with torch.no_grad():
            for k, n in enumerate(names):
                params[n].copy_(torch.from_numpy(seq[k][0]))
        ema = mod.LitEma(net, decay=decay, use_num_upates=warm)
        shadows, used = [[] for _ in names], []
        for u in range(1, UPDATES + 1):
            with torch.no_grad():
                for k, n in enumerate(names):
                    params[n].copy_(torch.from_numpy(seq[k][u]))
            ema(net)
            bufs = dict(ema.named_buffers())
            for k, n in enumerate(names):
                shadows[k].append(bufs[ema.m_name2s_name[n]].detach().numpy().copy())
            d = ema.decay
            if warm:
                assert int(ema.num_updates) == u
                d = min(ema.decay, (1 + ema.num_updates) / (10 + ema.num_updates))
            used.append(np.float32(float(d)))
            assert torch.as_tensor(d).dtype == torch.float32
        for k in range(len(names)):
            out[f"{tag}_s{k}"] = np.stack(shadows[k]).astype(np.float32)
            assert out[f"{tag}_s{k}"].shape == (UPDATES, SIZES[k])
        out[f"{tag}_d"] = np.array(used, np.float32)
        assert np.array_equal(out[f"{tag}_s0"], seq[0][1:])            # the tensor that never moves: the average stays on it
        assert not np.array_equal(out[f"{tag}_s2"][-1], seq[2][-1])
    for arr in out.values():
        assert np.isfinite(arr).all()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
