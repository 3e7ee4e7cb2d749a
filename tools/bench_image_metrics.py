#!/usr/bin/env python3
"""Cost of the image-space metrics against the decode they follow: for 240 frame pairs of 3 x 256 x 256 (16 clips x 15 predicted frames)
  (a) genie_frame_metrics (one call: sse, sae and the SSIM sum of every pair),
  (b) HipDecoder.decode_tokens of the same 240 frames, in this process -- the yardstick: the evaluator decodes twice per scored frame,
  (c) a torch restatement of the same SSIM (grouped conv2d in f32), for context only: it lives here, not in the package,
and the traffic floor of (a): both frames read once over the HBM rate.

    python tools/bench_image_metrics.py [--pairs 240] [--reps 5] [--out profiles/image_metrics_cost.txt]

Timing: device events around a window of back-to-back calls after a warm-up of the same shape; `reps` windows, median and range."""
import argparse
import importlib
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12   # bytes / s: float4 copy measured on MI355X, and the datasheet


def windows(fn, calls, reps, warmup=2):
    """ms per call over `reps` windows of `calls` back-to-back calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def fmt(name, ms, extra=""):
    return f"{name:48s} median {statistics.median(ms):9.4f} ms   range {min(ms):9.4f} .. {max(ms):9.4f} ms{extra}"


def torch_ssim(a, b):
    """Mean SSIM per frame, the definition of include/genie_hip.h on torch ops: f32, pixels pivoted by 128, two grouped conv2d passes."""
    r = torch.arange(11, dtype=torch.float64, device=a.device) - 5
    g = torch.exp(-r * r / 4.5)
    g = (g / g.sum()).float()
    x, y = a.float() - 128, b.float() - 128
    f = torch.cat([x, y, x * x, y * y, x * y], dim=1)
    ch = f.shape[1]
    f = torch.nn.functional.conv2d(f, g.view(1, 1, 1, 11).repeat(ch, 1, 1, 1), groups=ch)
    f = torch.nn.functional.conv2d(f, g.view(1, 1, 11, 1).repeat(ch, 1, 1, 1), groups=ch)
    mx, my, xx, yy, xy = f.chunk(5, dim=1)
    vx, vy, cxy = xx - mx * mx, yy - my * my, xy - mx * my
    ux, uy = mx + 128, my + 128
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * ux * uy + c1) * (2 * cxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.double().mean(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64, help="frames per decode_tokens call (tools/bench_e2e.py's)")
    ap.add_argument("--out", type=str, default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_image_metrics.py: needs the GPU (no CPU fallback)")
    mv = importlib.import_module("1xgpt_amd.magvit2")
    IM = importlib.import_module("1xgpt_amd.image_metrics")
    _lib = importlib.import_module("1xgpt_amd._lib")
    lib = _lib.load()
    n, C, H, W = a.pairs, 3, 256, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8, device="cuda", generator=g)
    noise = torch.randint(-20, 21, (n, C, H, W), dtype=torch.int16, device="cuda", generator=g)
    target = (pred.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    del noise

    # (a) the library call alone, buffers allocated once
    nbytes = lib.genie_frame_metrics_workspace_bytes(n, C, H, W)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    out = torch.empty(n, 4, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def metrics():
        _lib.check(lib.genie_frame_metrics(pred.data_ptr(), target.data_ptr(), n, C, H, W, out.data_ptr(), ws.data_ptr(), nbytes, st),
                   "genie_frame_metrics")

    t_a = windows(metrics, 200, a.reps)
    t_py = windows(lambda: IM.frame_metrics(pred, target), 50, a.reps)

    # (b) the decoder on the same number of frames
    vq = mv.VQModel(mv.VQConfig())
    vq.load_state_dict({k: torch.from_numpy(v) for k, v in mv.make_vq_state_dict(vq, seed=1).items()})
    hd = vq.to(device="cuda").eval().hip_decoder()
    tokens = torch.randint(0, 262144, (n, 16, 16), dtype=torch.int64, device="cuda", generator=g)

    def decode():
        return torch.cat([hd.decode_tokens(tokens[i:i + a.chunk]) for i in range(0, n, a.chunk)])

    assert tuple(decode().shape) == (n, C, H, W)
    t_b = windows(decode, 3, a.reps, warmup=1)

    # (c) torch, f32 grouped conv2d
    t_c = windows(lambda: torch_ssim(pred, target), 3, a.reps, warmup=1)
    fm = IM.frame_metrics(pred, target)
    d_torch = float((torch_ssim(pred, target) - fm.ssim).abs().max())

    med = statistics.median
    floor_ms = 2 * C * H * W * n / HBM_MEASURED * 1e3
    lines = [
        f"image-space metrics, {n} frame pairs of {C} x {H} x {W} uint8 ({torch.cuda.get_device_name(0)}); ms per call of all {n} pairs",
        fmt("(a) genie_frame_metrics", t_a),
        fmt("    image_metrics.frame_metrics (a + allocs + 4 torch ops)", t_py),
        fmt(f"(b) HipDecoder.decode_tokens, {a.chunk} frames per call", t_b),
        fmt("(c) torch restatement (grouped conv2d, f32)", t_c, f"   max |SSIM - (a)| {d_torch:.2e}"),
        f"(a) / (b) = {100 * med(t_a) / med(t_b):.2f} %   (the evaluator decodes twice per scored frame: {100 * med(t_a) / (2 * med(t_b)):.2f} % of that)",
        f"(c) / (a) = {med(t_c) / med(t_a):.1f} x",
        f"traffic floor of (a): 2 x {C * H * W:,} bytes per pair = {2 * C * H * W * n / 1e6:.1f} MB; {floor_ms * 1e3:.1f} us at {HBM_MEASURED / 1e12:.2f} TB/s measured "
        f"copy rate ({2 * C * H * W * n / HBM_SPEC * 1e6:.1f} us at the {HBM_SPEC / 1e12:.1f} TB/s datasheet rate); (a) is {med(t_a) / floor_ms:.1f} x the floor",
        f"mean over the pairs: PSNR {float(fm.psnr.mean()):.3f} dB, SSIM {float(fm.ssim.mean()):.5f}, MSE {float(fm.mse.mean()):.3f}",
    ]
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
