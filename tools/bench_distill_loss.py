#!/usr/bin/env python3
"""Time the loss launches alone, on the same student logits: the objective kernel (genie_ce_objective with a struct: count_frames_kernel +
ce_objective_kernel), where the loaded library has it the distillation kernel (genie_ce_distill: count_frames_kernel + ce_distill_kernel),
the neutral step's loss (genie_ce_objective without a struct: count_masked_kernel + ce_fwd_bwd_kernel), the evaluator's cross-entropy
(genie_factored_ce, token-major with weight_ids: ce_token_major_kernel) and the scoring kernel (genie_score_logits: score_rows_kernel).

    python tools/bench_distill_loss.py                         # 32,768 tokens of 2 x 512 (c138, B = 8), tau 1 and 2
    GENIE_HIP_LIBRARY=1xgpt_amd/lib_ab_parent.so python tools/bench_distill_loss.py      # another build

One process measures one library; an A/B alternates processes (profiles/train_distill.txt, profiles/loss_kernels_ab.txt).  Every launch
works on a fresh copy of the logits (the training kernels replace them by gradients) and is timed by its own pair of device events after
`--warmup` untimed launches; the per-kernel milliseconds of the library's profiler (genie_profile_kernels) are printed beside them as
kernel_ms_mean.  The last three launches are bracketed by no profiler scope: their kernel_ms_mean is the mean of the call's event times
(memset and count kernel included for the neutral loss).  Bytes: a COUNTED token's row (frame >= 1 and a masked id) costs 8 bytes per
logit element in the training losses (read + write) and 12 in the distillation kernel (the teacher's row is read too); an uncounted
token's row is only written with zeros, 4 bytes per element.  The evaluator reads the rows of the masked ids of every frame, the scoring
kernel every row, once.  kernel_GBps is computed from the counted fraction of this input (about half the ids are masked)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_lib = importlib.import_module("1xgpt_amd._lib")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--vf", type=int, default=512)
    ap.add_argument("--nfac", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--taus", type=str, default="1,2")
    ap.add_argument("--labels", choices=["random", "argmax"], default="random",
                    help="random: no token of random logits is a hit, so the hit sum of every workgroup is zero and its atomicAdd is skipped; "
                         "argmax: every token is a hit (a trained model's case: every workgroup adds to every sum)")
    a = ap.parse_args()
    lib = _lib.load()
    N, V, mask_id = a.clips * a.T * a.S, a.vf * a.nfac, a.vf ** a.nfac
    g = torch.Generator(device="cuda").manual_seed(0)
    src = 3.0 * torch.randn(N, V, generator=g, device="cuda")
    teacher = 3.0 * torch.randn(N, V, generator=g, device="cuda")
    logits = torch.empty_like(src)
    labels = torch.randint(0, mask_id, (N,), generator=g, device="cuda")
    if a.labels == "argmax":   # (after the draw: the logits, teacher rows and masked ids are the same input either way)
        labels = (src.view(N, a.nfac, a.vf).argmax(-1) * a.vf ** torch.arange(a.nfac, device="cuda")).sum(-1)
    ids = torch.where(torch.rand(N, generator=g, device="cuda") < 0.5, torch.full_like(labels, mask_id), labels)
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ob = _lib.Objective(label_smoothing=0.1, z_loss=1e-4, n_frames=0)
    geom = (a.clips, a.T, a.S, a.vf, a.nfac, mask_id)

    def objective():
        return lib.genie_ce_objective(logits.data_ptr(), ids.data_ptr(), labels.data_ptr(), *geom, ob, sums.data_ptr(), st)

    def distill(tau):
        ds = _lib.Distill(alpha=0.5, temperature=tau, teacher_logits=teacher.data_ptr())
        return lambda: lib.genie_ce_distill(logits.data_ptr(), teacher.data_ptr(), ids.data_ptr(), labels.data_ptr(), *geom, ob, ds,
                                            sums.data_ptr(), st)
    counted = float(((ids == mask_id).view(a.clips, a.T, a.S)[:, 1:]).sum()) / N
    masked = float((ids == mask_id).sum()) / N
    config = importlib.import_module("1xgpt_amd.config").GenieConfig(num_layers=1, num_heads=8, d_model=256, T=a.T, S=a.S, num_factored_vocabs=a.nfac,
                                                                     image_vocab_size=mask_id)
    cfg = _lib.make_cfg(config)
    rows = a.clips * a.T   # the scoring kernel's rows: one frame each, against its own S labels
    nll, hits = torch.zeros(rows, dtype=torch.float64, device="cuda"), torch.zeros(rows, dtype=torch.float64, device="cuda")
    token_nll = torch.zeros(N, device="cuda")

    def neutral():
        return lib.genie_ce_objective(logits.data_ptr(), ids.data_ptr(), labels.data_ptr(), *geom, None, sums.data_ptr(), st)

    def factored_ce():   # (adds to sums[:3]: they grow over the launches and stay finite)
        return lib.genie_factored_ce(cfg, logits.data_ptr(), _lib.LAYOUT_TOKEN_MAJOR, labels.data_ptr(), ids.data_ptr(), a.clips, 0, a.T,
                                     sums.data_ptr(), st)

    def score():
        return lib.genie_score_logits(cfg, logits.data_ptr(), labels.data_ptr(), a.S, 1, rows, nll.data_ptr(), 1, hits.data_ptr(),
                                      token_nll.data_ptr(), a.S, st)
    # (name, the profiler's name of the kernel or None, bytes per logit element of this input, the call)
    runs = [("ce_objective", "ce_objective_kernel", 8 * counted + 4 * (1 - counted), objective)]
    if hasattr(lib, "genie_ce_distill"):
        runs += [(f"ce_distill tau={tau:g}", "ce_distill_kernel", 12 * counted + 4 * (1 - counted), distill(tau))
                 for tau in (float(t) for t in a.taus.split(","))]
    runs += [("ce_fwd_bwd", None, 8 * counted + 4 * (1 - counted), neutral), ("ce_token_major", None, 4 * masked, factored_ce),
             ("score_rows", None, 4.0, score)]
    out = {"library": os.path.basename(_lib.LIB_PATH), "tokens": N, "vocab": f"{a.nfac}x{a.vf}", "counted_fraction": counted}
    for name, kernel, bytes_per, call in runs:
        sums.zero_()
        for _ in range(a.warmup):
            logits.copy_(src)
            _lib.check(call(), name)
        torch.cuda.synchronize()
        lib.genie_profile_enable(0x1F)
        lib.genie_profile_reset()
        ev = []
        for _ in range(a.iters):
            logits.copy_(src)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            _lib.check(call(), name)
            e[1].record()
            ev.append(e)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        kbuf = C.create_string_buffer(16384)
        _lib.check(lib.genie_profile_kernels(_lib.KC_OTHER, kbuf, len(kbuf)), "profile_kernels")
        lib.genie_profile_enable(0)
        kern = {ln.split("\t")[0]: float(ln.split("\t")[2]) / float(ln.split("\t")[1]) for ln in kbuf.value.decode().splitlines() if ln}
        k_ms = kern.get(kernel, float("nan")) if kernel else sum(ms) / len(ms)
        out[name] = {"call_ms_min": ms[0], "call_ms_median": ms[len(ms) // 2], "call_ms_max": ms[-1], "kernel_ms_mean": k_ms,
                     "count_frames_ms_mean": kern.get("count_frames_kernel", float("nan")),
                     "kernel_MB": bytes_per * N * V / 1e6, "kernel_GBps": bytes_per * N * V / (k_ms * 1e-3) / 1e9}
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(sums[:5]).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
