#!/usr/bin/env python3
"""generate.py workload (BASELINE config 3): prompt 8 frames -> sample 8 frames, MaskGIT steps 2 and 8, temperature 0,
GENIE_138M-shape, full-forward schedule vs temporal KV cache, at batch 1 (the reference's CLI) and batched."""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def guidance_ab(a, m, cfg, extra):
    """guided(B) against unguided(B) and unguided(2B) of the same library, one call per leg per round, legs interleaved: per leg the
    median and the min-max spread over the rounds."""
    synth = importlib.import_module("1xgpt_amd.synthetic")
    G = importlib.import_module("1xgpt_amd.generate")
    guide = importlib.import_module("1xgpt_amd.sampling").Guidance(a.guidance_scale, 0)
    res = []
    for B in a.batches:
        for steps in a.steps:
            legs = {}
            for name, nb, g in (("unguided_B", B, None), ("unguided_2B", 2 * B, None), ("guided_B", B, guide)):
                ex = torch.from_numpy(synth.make_clips(nb, cfg, seed=7)).cuda().view(nb, 16, 16, 16)
                acts = torch.randint(1, cfg.action_vocab_size, (nb, cfg.T), generator=torch.Generator().manual_seed(nb)).cuda()
                noise = torch.rand(8, max(steps - 1, 1), nb, cfg.S, device="cuda")
                legs[name] = dict(args=(m, ex, 8, steps, a.temperature, False), kw=dict(noise=noise, action_ids=acts, guidance=g, **extra),
                                  times=[], frames=8 * B)
            for leg in legs.values():
                for _ in range(2):
                    G.generate_frames_cached(*leg["args"], **leg["kw"])
            for _ in range(a.repeats):
                for leg in legs.values():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    G.generate_frames_cached(*leg["args"], **leg["kw"])
                    torch.cuda.synchronize()
                    leg["times"].append(time.perf_counter() - t0)
            for name, leg in legs.items():
                t = sorted(leg["times"])
                res.append({"leg": name, "batch": B, "maskgit_steps": steps, "guidance_scale": a.guidance_scale, "sampler": bool(a.sampler),
                            "median_ms": 1e3 * t[len(t) // 2], "min_ms": 1e3 * t[0], "max_ms": 1e3 * t[-1],
                            "ms_per_frame": 1e3 * t[len(t) // 2] / leg["frames"]})
                print(res[-1], flush=True)
    print(json.dumps({"workload": "generate 8->8 frames under guidance, " + a.model + " " + a.precision, "results": res}))


def rollout_ab(a, m, cfg, extra):
    """rollout_frames at N new frames against generate_frames_cached at T - P new frames (P = 8, keep = --keep), one call per leg per round,
    legs interleaved: per leg the median and the min-max spread over the rounds, in ms per generated frame.  --rollout 0 runs the
    in-window leg alone (the A/B of a library that lacks the rollout)."""
    synth = importlib.import_module("1xgpt_amd.synthetic")
    G = importlib.import_module("1xgpt_amd.generate")
    P, T, N = 8, cfg.T, a.rollout
    res = []
    for B in a.batches:
        ex = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, T, 16, 16)
        for steps in a.steps:
            legs = {"in_window": dict(fn=lambda ex=ex, steps=steps, nz=torch.rand(T - P, max(steps - 1, 1), B, cfg.S, device="cuda"):
                                      G.generate_frames_cached(m, ex, P, steps, a.temperature, False, noise=nz, **extra),
                                      frames=T - P, times=[])}
            if N:
                legs["rollout"] = dict(fn=lambda ex=ex, steps=steps, nz=torch.rand(N, max(steps - 1, 1), B, cfg.S, device="cuda"):
                                       G.rollout_frames(m, ex[:, :P], N, keep=a.keep, maskgit_steps=steps, temperature=a.temperature,
                                                        noise=nz, **extra),
                                       frames=N, times=[])
            for leg in legs.values():
                for _ in range(2):
                    leg["fn"]()
            for _ in range(a.repeats):
                for leg in legs.values():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg["fn"]()
                    torch.cuda.synchronize()
                    leg["times"].append(time.perf_counter() - t0)
            for name, leg in legs.items():
                t = [1e3 * x / leg["frames"] for x in sorted(leg["times"])]
                res.append({"leg": name, "batch": B, "maskgit_steps": steps, "prompt": P, "keep": a.keep or P, "new_frames": leg["frames"],
                            "sampler": bool(a.sampler), "ms_per_frame_median": t[len(t) // 2], "ms_per_frame_min": t[0],
                            "ms_per_frame_max": t[-1]})
                print(res[-1], flush=True)
    print(json.dumps({"workload": f"rollout {P}->{N} frames against generate {P}->{T - P}, " + a.model + " " + a.precision, "results": res}))


def fanout_ab(a, m, cfg, extra):
    """fanout_frames at (B, K) against generate_frames_cached on the K-times replicated batch (prompt 8, 8 new frames), one call per leg
    per round, legs interleaved: per leg the median and the min-max spread over the rounds, and the peak cache bytes of each."""
    synth = importlib.import_module("1xgpt_amd.synthetic")
    G = importlib.import_module("1xgpt_amd.generate")
    L = importlib.import_module("1xgpt_amd._lib")
    lib, c = L.load(), m._weights()[0]
    P, T, K = 8, cfg.T, a.fanout
    N = T - P
    res = []
    for B in a.batches:
        ex = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, T, 16, 16)
        rep = ex.repeat_interleave(K, dim=0).contiguous()
        for steps in a.steps:
            nz = torch.rand(N, max(steps - 1, 1), B * K, cfg.S, device="cuda")
            legs = {"fanout": dict(fn=lambda steps=steps, nz=nz: G.fanout_frames(m, ex[:, :P], N, K=K, maskgit_steps=steps,
                                                                                 temperature=a.temperature, noise=nz, **extra),
                                   cache=lib.genie_prefix_cache_bytes(c, B) + lib.genie_fanout_branch_bytes(c, B, K, N), times=[]),
                    "replicated": dict(fn=lambda steps=steps, nz=nz: G.generate_frames_cached(m, rep, P, steps, a.temperature, False, noise=nz,
                                                                                              **extra),
                                       cache=lib.genie_prefix_cache_bytes(c, B * K), times=[])}
            for leg in legs.values():
                for _ in range(2):
                    leg["fn"]()
            for _ in range(a.repeats):
                for leg in legs.values():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg["fn"]()
                    torch.cuda.synchronize()
                    leg["times"].append(time.perf_counter() - t0)
            for name, leg in legs.items():
                t = sorted(leg["times"])
                res.append({"leg": name, "batch": B, "K": K, "maskgit_steps": steps, "prompt": P, "new_frames": N, "sampler": bool(a.sampler),
                            "median_ms": 1e3 * t[len(t) // 2], "min_ms": 1e3 * t[0], "max_ms": 1e3 * t[-1], "cache_bytes": leg["cache"]})
                print(res[-1], flush=True)
    print(json.dumps({"workload": f"fan-out {P}->{N} frames x K={K} against the replicated batch, " + a.model + " " + a.precision, "results": res}))


def teacher_forced_logits0(m, ex, P, cond=None):
    """The step-0 logits (B, n, S, V) of genie_generate_cached_ex teacher-forced in time at one MaskGIT step: the route to per-frame
    likelihoods without genie_score_fanout."""
    L = importlib.import_module("1xgpt_amd._lib")
    lib = L.load()
    cfg, w = m._weights()[:2]
    c = m.config
    B, T = ex.shape[:2]
    ids = ex.reshape(B, T, c.S).contiguous()
    V = c.factored_vocab_size * c.num_factored_vocabs
    gen = torch.empty(B, T - P, c.S, dtype=torch.int64, device="cuda")
    lg = torch.empty(B, T - P, c.S, V, dtype=torch.float32, device="cuda")
    ws = m._workspace(B, generate_prompt_frames=P)
    nbytes = lib.genie_prefix_cache_bytes(cfg, B)
    cache = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(L.call_guided(lib, "genie_generate_cached", cond, None, None, cfg, w, ids.data_ptr(), B, P, T - P, 1, 0.0, L.UNMASK_GREEDY, 0, 0, 1, 1,
                          gen.data_ptr(), lg.data_ptr(), cache.data_ptr(), nbytes, ws.data_ptr(), ws.numel(),
                          torch.cuda.current_stream().cuda_stream), "genie_generate_cached")
    return lg


def score_ab(a, m, cfg, extra):
    """score_frames at (B, K) (prompt 8, 8 scored frames) against (1) the teacher-forced cached loop at one MaskGIT step on the K-times
    replicated batch with its step-0 logits written out and the NLL taken in torch, and (2) fanout_frames at two steps on the same shape;
    one call per leg per round, legs interleaved: per leg the median and the min-max spread, and the cache and logits bytes of each."""
    synth = importlib.import_module("1xgpt_amd.synthetic")
    G = importlib.import_module("1xgpt_amd.generate")
    L = importlib.import_module("1xgpt_amd._lib")
    lib, c = L.load(), m._weights()[0]
    P, T, K = 8, cfg.T, a.score
    N = T - P
    V, nf, vf = cfg.factored_vocab_size * cfg.num_factored_vocabs, cfg.num_factored_vocabs, cfg.factored_vocab_size
    res = []

    def torch_nll(rep):
        lg = teacher_forced_logits0(m, rep, P)                                       # (B K, N, S, V)
        tg = rep[:, P:].reshape(-1, N, cfg.S)
        nll = torch.zeros(tg.shape, dtype=torch.float32, device="cuda")
        for f in range(nf):
            lp = torch.log_softmax(lg[..., f * vf:(f + 1) * vf], dim=-1)
            nll -= lp.gather(-1, ((tg // vf ** f) % vf)[..., None])[..., 0]
        return nll.double().sum(-1)

    for B in a.batches:
        ex = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, T, 16, 16)
        rep = ex.repeat_interleave(K, dim=0).contiguous()
        nz = torch.rand(N, 1, B * K, cfg.S, device="cuda")
        split = lib.genie_prefix_cache_bytes(c, B) + lib.genie_fanout_branch_bytes(c, B, K, N)
        legs = {"score": dict(fn=lambda: G.score_frames(m, ex, P, K=K), cache=split, logits=B * K * cfg.S * V * 4, times=[]),
                "replicated_logits0_torch_ce": dict(fn=lambda: torch_nll(rep), cache=lib.genie_prefix_cache_bytes(c, B * K),
                                                    logits=B * K * (N + 1) * cfg.S * V * 4, times=[]),
                "fanout_steps2": dict(fn=lambda: G.fanout_frames(m, ex[:, :P], N, K=K, maskgit_steps=2, temperature=a.temperature, noise=nz,
                                                                 **extra), cache=split, logits=B * K * cfg.S * V * 4, times=[])}
        for leg in legs.values():
            for _ in range(2):
                leg["fn"]()
        for _ in range(a.repeats):
            for leg in legs.values():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg["fn"]()
                torch.cuda.synchronize()
                leg["times"].append(time.perf_counter() - t0)
        for name, leg in legs.items():
            t = sorted(leg["times"])
            res.append({"leg": name, "batch": B, "K": K, "prompt": P, "frames": N, "median_ms": 1e3 * t[len(t) // 2], "min_ms": 1e3 * t[0],
                        "max_ms": 1e3 * t[-1], "cache_bytes": leg["cache"], "logits_bytes": leg["logits"]})
            print(res[-1], flush=True)
    print(json.dumps({"workload": f"score {N} observed frames behind {P} x K={K}, " + a.model + " " + a.precision, "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--model", default="c138")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--schedules", nargs="+", default=["full_forward", "kv_cache"], choices=["full_forward", "kv_cache"])
    ap.add_argument("--temperature", type=float, default=0.0, help="the reference's arg-max / sampling switch (does not temper)")
    ap.add_argument("--sampler", action="store_true",
                    help="decode under a sampling law (default tau 0.7, top-k 50, top-p 0.9; implies --temperature 1 unless given)")
    ap.add_argument("--logit_temperature", type=float, default=0.7)
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--top_p", type=float, default=0.9)
    ap.add_argument("--unmask_mode", default="random", choices=["random", "greedy", "confidence"])
    ap.add_argument("--guidance_scale", type=float, default=None,
                    help="classifier-free guidance A/B on an action-conditioned variant of the model (8 actions, null action 0), KV-cache "
                         "schedule: per batch B, interleaved in one process, unguided at B, unguided at 2B and guided at B with this scale")
    ap.add_argument("--action_dim", type=int, default=0,
                    help="plain run on a variant of the model conditioned on continuous action vectors of this many values per frame")
    ap.add_argument("--action_vocab_size", type=int, default=0, help="plain run on an action-conditioned variant with this many action ids")
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds of the guidance A/B and of the rollout leg")
    ap.add_argument("--rollout", type=int, default=None,
                    help="rollout leg: ms per generated frame of rollout_frames at this many new frames (prompt 8) against generate_frames_cached "
                         "at T - 8, interleaved in one process; 0 = the in-window leg alone")
    ap.add_argument("--fanout", type=int, default=None,
                    help="fan-out leg: per batch B, fanout_frames at (B, K) against generate_frames_cached on the K-times replicated batch "
                         "(prompt 8, 8 new frames), interleaved in one process, with the cache bytes of each")
    ap.add_argument("--score", type=int, default=None,
                    help="scoring leg: per batch B, score_frames at (B, K) against the teacher-forced cached loop with its step-0 logits and a "
                         "torch CE on the K-times replicated batch, and against fanout_frames at two steps (prompt 8, 8 frames), interleaved")
    ap.add_argument("--keep", type=int, default=None, help="context frames the rollout re-runs per window (default: the prompt's 8)")
    a = ap.parse_args()
    extra = {}
    if a.sampler:
        SC = importlib.import_module("1xgpt_amd.sampling").SamplingConfig
        extra = dict(sampling=SC(a.logit_temperature, a.top_k, a.top_p), unmask_mode=a.unmask_mode)
        if a.temperature == 0.0:
            a.temperature = 1.0
    cfgmod = importlib.import_module("1xgpt_amd.config")
    synth = importlib.import_module("1xgpt_amd.synthetic")
    G = importlib.import_module("1xgpt_amd.generate")
    STMaskGIT = importlib.import_module("1xgpt_amd.st_mask_git").STMaskGIT
    cfg = cfgmod.c138() if a.model == "c138" else cfgmod.c35()
    if a.guidance_scale is not None:
        cfg.action_vocab_size = 8
    elif a.action_dim:
        cfg = cfgmod.GenieConfig(**{**vars(cfg), "action_dim": a.action_dim})
    elif a.action_vocab_size:
        cfg.action_vocab_size = a.action_vocab_size
    m = STMaskGIT(cfg, precision=a.precision).load_numpy_state_dict(synth.make_state_dict(cfg, seed=0)).to("cuda")
    if a.guidance_scale is not None:
        return guidance_ab(a, m, cfg, extra)
    if a.rollout is not None:
        return rollout_ab(a, m, cfg, extra)
    if a.fanout is not None:
        return fanout_ab(a, m, cfg, extra)
    if a.score is not None:
        return score_ab(a, m, cfg, extra)
    res = []
    for B in a.batches:
        ex = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, 16, 16, 16)
        for steps in a.steps:
            noise = torch.rand(8, max(steps - 1, 1), B, cfg.S, device="cuda")
            if cfg.action_dim:
                extra["action_vectors"] = torch.randn(B, cfg.T, cfg.action_dim, generator=torch.Generator().manual_seed(B)).cuda()
            elif cfg.action_vocab_size:
                extra["action_ids"] = torch.randint(0, cfg.action_vocab_size, (B, cfg.T), generator=torch.Generator().manual_seed(B)).cuda()
            for name, fn in (("full_forward", G.generate_frames), ("kv_cache", G.generate_frames_cached)):
                if name not in a.schedules or (name == "full_forward" and B * steps > 64):
                    continue
                for _ in range(2):   # (the cached schedule captures its HIP graphs on the second call)
                    fn(m, ex, 8, steps, a.temperature, False, noise=noise, **extra)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                reps = 3
                for _ in range(reps):
                    out = fn(m, ex, 8, steps, a.temperature, False, noise=noise, **extra)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / reps
                res.append({"schedule": name, "batch": B, "maskgit_steps": steps, "sampler": bool(a.sampler), "action_dim": cfg.action_dim,
                            "action_vocab_size": cfg.action_vocab_size,
                            "temperature": a.temperature, "seconds": dt,
                            "frames_per_sec": 8 * B / dt, "s_per_frame": dt / (8 * B)})
                print(res[-1], flush=True)
    print(json.dumps({"workload": "generate 8->8 frames, " + a.model + " " + a.precision, "results": res}))


if __name__ == "__main__":
    main()
