#!/usr/bin/env python3
"""Cost of per-frame action conditioning: the same GENIE_138M-shape model (synthetic weights) unconditioned and with an action
table, in alternating repeats on one box -- generate 8 -> 8 frames on the KV cache (MaskGIT steps 2) at batch 1 and 16 (ms per
generated frame), and the teacher-forced evaluator on the prefix-reuse path at 128 clips.  The conditioned model is the
unconditioned one plus `action_embed`, so both run the same kernels except the embedding's ACT instantiation."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--actions", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eval_clips", type=int, default=128)
    a = ap.parse_args()
    P = lambda n: importlib.import_module("1xgpt_amd." + n)  # noqa: E731
    cfgmod, synth, G, ev_mod = P("config"), P("synthetic"), P("generate"), P("evaluate")
    STMaskGIT = P("st_mask_git").STMaskGIT
    c0 = cfgmod.c138()
    ca = cfgmod.GenieConfig(**dict(vars(c0), action_vocab_size=a.actions))
    sd = synth.make_state_dict(c0, seed=0)
    sda = dict(sd, **{"action_embed.weight": (0.5 * np.random.default_rng(1).standard_normal((a.actions, c0.d_model))).astype(np.float32)})
    models = {"uncond": STMaskGIT(c0, precision=a.precision).load_numpy_state_dict(sd).to("cuda"),
              "cond": STMaskGIT(ca, precision=a.precision).load_numpy_state_dict(sda).to("cuda")}
    g = torch.Generator().manual_seed(2)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {}
    for B in (1, 16):
        ex = torch.from_numpy(synth.make_clips(B, c0, seed=7)).cuda().view(B, 16, 16, 16)
        act = torch.randint(0, a.actions, (B, 16), generator=g).cuda()
        noise = torch.rand(8, 1, B, c0.S, generator=g).cuda()
        runs = {k: (lambda m=m, k=k: G.generate_frames_cached(m, ex, 8, 2, 0.0, False, noise=noise,
                                                               action_ids=act if k == "cond" else None))
                for k, m in models.items()}
        for fn in runs.values():   # warm-up
            fn()
            fn()
        t = {k: [] for k in runs}
        for _ in range(a.reps):    # alternating
            for k, fn in runs.items():
                t[k].append(timed(fn) / (8 * B) * 1e3)
        res[f"generate_b{B}_s2_ms_per_frame"] = {k: round(statistics.median(v), 4) for k, v in t.items()}
        print(res, flush=True)
    clips = torch.from_numpy(synth.make_clips(a.eval_clips, c0, seed=11))
    acts = torch.randint(0, a.actions, (a.eval_clips, 16), generator=g)
    args = SimpleNamespace(maskgit_steps=2, temperature=0.0, latent_h=16, latent_w=16)
    evs = {k: ev_mod.GenieEvaluator(args, None, "cuda", model=m) for k, m in models.items()}
    runs = {k: (lambda e=e, k=k: ev_mod.evaluate_clips(e, clips, batch_size=16, noise_seed=3,
                                                       action_ids=acts if k == "cond" else None)) for k, e in evs.items()}
    for fn in runs.values():
        fn()
    t = {k: [] for k in runs}
    for _ in range(max(1, a.reps // 2)):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    res[f"evaluate_{a.eval_clips}clips_s"] = {k: round(statistics.median(v), 4) for k, v in t.items()}
    print(json.dumps({"workload": f"c138 {a.precision}, {a.actions} actions, alternating repeats", "results": res}))


if __name__ == "__main__":
    main()
