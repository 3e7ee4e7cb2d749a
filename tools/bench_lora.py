#!/usr/bin/env python3
"""Time genie_lora_merge and genie_lora_project (csrc/kernels_lora.hip) at a model's Linear shapes, as the trainer launches them.

    python tools/bench_lora.py --config c138 --rank 8 [--iters 20]

One launch per layer carries the layer's six Linears.  The merge walks all layers' own W0 / W (what follows an optimizer step); the
projection reads ONE layer's worth of dW, reused by every layer as in the trainer, and writes each layer's own dA / dB.  Per kernel the
line holds the event-timed mean per launch, the bytes the launch must move (merge: W0 in, W out, A, B; project: dW, A, B in, the partial
slabs out; reduce: the slabs in, dA, dB out) and those bytes over 6.3 TB/s.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`; the kernels are lora_merge_kernel, lora_project_kernel<KP> and lora_reduce_kernel.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c138", choices=["c35", "c138"])
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    P = lambda n: importlib.import_module("1xgpt_amd." + n)  # noqa: E731
    _lib, L, cfgm = P("_lib"), P("lora"), P("config")
    lib = _lib.load()
    cfg = cfgm.c138() if a.config == "c138" else cfgm.c35()
    d, h = cfg.d_model, int(cfg.d_model * cfg.mlp_ratio)
    shapes = [(3 * d, d), (d, d), (3 * d, d), (d, d), (h, d), (d, h)]
    r, s, nl = a.rank, 2.0, cfg.num_layers
    f = lambda *shape: torch.randn(*shape, device="cuda")  # noqa: E731
    dw = [f(o, i) for o, i in shapes]
    layers = []
    for _ in range(nl):
        items = []
        for (o, i), g in zip(shapes, dw):
            t = dict(w0=f(o, i), w=torch.empty(o, i, device="cuda"), a=f(r, i), b=f(o, r), da=torch.empty(r, i, device="cuda"),
                     db=torch.empty(o, r, device="cuda"))
            items.append((t, L.item(s, o, i, r, t["a"].data_ptr(), t["b"].data_ptr(), w=t["w"].data_ptr(), w0=t["w0"].data_ptr(),
                                    dw=g.data_ptr(), da=t["da"].data_ptr(), db=t["db"].data_ptr())))
        layers.append((items, L.table([it for _, it in items])))
    arr0, n0 = layers[0][1]
    need = lib.genie_lora_project_scratch_bytes(arr0, n0)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    elems = sum(o * i for o, i in shapes)
    small = sum(r * i + o * r for o, i in shapes)
    byt = {"merge": 4 * (2 * elems + small), "project+reduce": 4 * (elems + small) + 2 * need + 4 * small}

    def merge_all():
        for _, (arr, n) in layers:
            _lib.check(lib.genie_lora_merge(arr, n, st), "genie_lora_merge")

    def project_all():
        for _, (arr, n) in layers:
            _lib.check(lib.genie_lora_project(arr, n, 0, scratch.data_ptr(), need, st), "genie_lora_project")

    for name, fn in (("merge", merge_all), ("project+reduce", project_all)):
        fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / (a.iters * nl)
        bound = byt[name] / HBM * 1e6
        print(json.dumps({"config": a.config, "rank": r, "call": name, "layers": nl, "us_per_layer_call": round(us, 3),
                          "bytes_per_layer_call": byt[name], "us_at_6.3TBps": round(bound, 3), "share_of_bound": round(bound / us, 4),
                          "scratch_bytes": need}), flush=True)


if __name__ == "__main__":
    main()
