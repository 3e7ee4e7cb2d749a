#!/usr/bin/env python3
"""Launch cost of the filtered sampler: genie_sample (temperature 0.8) against genie_sample_ex at (tau 0.7, top-k 50, top-p 0.9)
on the logits of one frame of 1 and 16 clips and of the evaluator's 128 x 15 frames; same process, interleaved repeats, medians
of HIP-event times; bytes/s = the 4 KB of logits per token over the launch time.
    python tools/bench_sampler.py [--reps 20]"""
import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 128 * 15])
    a = ap.parse_args()
    lib = importlib.import_module("1xgpt_amd._lib")
    L = lib.load()
    cfg = importlib.import_module("1xgpt_amd.config").c138()
    c = lib.make_cfg(cfg, lib.PREC_F16X3)
    S, V = cfg.S, cfg.factored_vocab_size * cfg.num_factored_vocabs
    law = lib.Sampling(0.7, 50, 0.9, 4.5)
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for R in a.frames:
        g = torch.Generator(device="cuda").manual_seed(R)
        logits = torch.randn(R, S, V, device="cuda", generator=g) * 2.5
        uni = torch.rand(2, R, S, device="cuda", generator=g)
        noise = torch.rand(R, S, device="cuda", generator=g)
        samples = torch.empty(R, S, dtype=torch.int64, device="cuda")
        conf = torch.empty(R, S, dtype=torch.float32, device="cuda")
        keys = torch.empty(R, S, dtype=torch.float32, device="cuda")

        def old():
            lib.check(L.genie_sample(c, logits.data_ptr(), 0, R, 0.8, uni.data_ptr(), samples.data_ptr(), conf.data_ptr(), st), "sample")

        def new():
            lib.check(L.genie_sample_ex(c, logits.data_ptr(), 0, R, 0.8, uni.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, law,
                                        0, 0, 0.0), "sample_ex")

        def new_keys():
            lib.check(L.genie_sample_ex(c, logits.data_ptr(), 0, R, 0.8, uni.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, law,
                                        keys.data_ptr(), noise.data_ptr(), 0.5), "sample_ex")

        fns = {"genie_sample": old, "genie_sample_ex": new, "genie_sample_ex+keys": new_keys}
        times = {k: [] for k in fns}
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        row = {"frames": R, "tokens": R * S, "logit_bytes": R * S * V * 4}
        for name, t in times.items():
            us = statistics.median(t)
            row[name] = {"median_us": round(us, 2), "min_us": round(min(t), 2), "TB_per_s": round(R * S * V * 4 / us / 1e6, 3)}
        res.append(row)
        print(row, flush=True)
    print(json.dumps({"workload": "sampler launch, 2 x 512 vocabulary, token-major", "results": res}))


if __name__ == "__main__":
    main()
