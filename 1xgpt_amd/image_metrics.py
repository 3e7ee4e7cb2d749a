"""Image-space metrics of uint8 frames on the device: MSE, MAE, PSNR and SSIM per frame (genie_frame_metrics, one fused HIP pass).

The reference's only image-space metric is LPIPS (eval_utils.py:80-88), a perceptual network whose weights cannot be shipped or pinned;
PSNR and SSIM take its place: they need no weights and have closed definitions (include/genie_hip.h states SSIM's, constants included:
11 x 11 Gaussian window with sigma 1.5, population moments, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, valid windows only).
"""
from typing import NamedTuple

import torch

from . import _lib

WINDOW = 11        # SSIM window edge: frames must be at least this large
PSNR_CAP = 100.0   # dB at which running means count a frame with mse == 0 (frame_metrics itself keeps inf)


class FrameMetrics(NamedTuple):
    """Per-frame metrics, each an f64 device tensor of the inputs' leading shape; psnr is inf where mse == 0."""
    mse: torch.Tensor
    mae: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor


def _check(pred_u8, target_u8):
    for name, t in (("pred", pred_u8), ("target", target_u8)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError(f"frame_metrics: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
    if pred_u8.shape != target_u8.shape:
        raise ValueError(f"frame_metrics: pred {tuple(pred_u8.shape)} and target {tuple(target_u8.shape)} differ in shape")
    if pred_u8.dim() < 3:
        raise ValueError(f"frame_metrics: frames must be (..., C, H, W), got {tuple(pred_u8.shape)}")
    C, H, W = pred_u8.shape[-3:]
    if C < 1 or H < WINDOW or W < WINDOW:
        raise ValueError(f"frame_metrics: frames of {C} x {H} x {W} are smaller than the {WINDOW} x {WINDOW} SSIM window")
    if not (pred_u8.is_cuda and target_u8.is_cuda):
        raise RuntimeError("1xgpt_amd runs on the GPU only (no CPU fallback): frames must be on cuda")
    if pred_u8.device != target_u8.device:
        raise RuntimeError(f"frame_metrics: pred on {pred_u8.device}, target on {target_u8.device}")


def frame_metric_sums(pred_u8: torch.Tensor, target_u8: torch.Tensor) -> torch.Tensor:
    """(..., C, H, W) uint8 CUDA tensors of equal shape -> (n, 4) f64 device tensor, n the product of the leading dimensions, rows
    [sum (a - b)^2, sum |a - b|, sum of SSIM over the valid windows, number of those windows] (the first two exact)."""
    _check(pred_u8, target_u8)
    C, H, W = pred_u8.shape[-3:]
    a = pred_u8.reshape(-1, C, H, W).contiguous()
    b = target_u8.reshape(-1, C, H, W).contiguous()
    n = a.shape[0]
    out = torch.empty(n, 4, dtype=torch.float64, device=a.device)
    if n == 0:
        return out
    lib = _lib.load()
    nbytes = lib.genie_frame_metrics_workspace_bytes(n, C, H, W)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.genie_frame_metrics(a.data_ptr(), b.data_ptr(), n, C, H, W, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, st),
                   "genie_frame_metrics")
    return out


def frame_metrics(pred_u8: torch.Tensor, target_u8: torch.Tensor) -> FrameMetrics:
    """MSE, MAE, PSNR (10 log10(255^2 / mse), inf where mse == 0) and mean SSIM of every frame pair; (..., C, H, W) uint8 CUDA tensors of
    equal shape, frames at least 11 x 11; the leading dimensions are kept.  Nothing is synchronised and nothing leaves the device."""
    sums = frame_metric_sums(pred_u8, target_u8)
    lead, (C, H, W) = pred_u8.shape[:-3], pred_u8.shape[-3:]
    # a device tensor, so that the divisions are true divisions (a Python scalar divisor is applied as a product with its inverse)
    npix = torch.full((), float(C * H * W), dtype=torch.float64, device=sums.device)
    mse = sums[:, 0] / npix
    psnr = 10.0 * torch.log10((255.0 * 255.0 * npix) / sums[:, 0])     # x / 0 = inf, log10(inf) = inf
    return FrameMetrics(mse.reshape(lead), (sums[:, 1] / npix).reshape(lead), psnr.reshape(lead), (sums[:, 2] / sums[:, 3]).reshape(lead))
