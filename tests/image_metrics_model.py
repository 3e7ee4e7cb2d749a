"""Float64 NumPy restatement of genie_frame_metrics (include/genie_hip.h): exact sums of (a - b)^2 and |a - b|, and the Gaussian-window SSIM
index of Wang et al. 2004 summed over the valid windows.  Stated from the definition, window by window along each axis; no scipy here
(tests/test_image_metrics_cpu.py compares it with scipy.ndimage.gaussian_filter)."""
import numpy as np

WINDOW, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def taps():
    r = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-r * r / (2 * SIGMA * SIGMA))
    return g / g.sum()


def window_mean(img):
    """(..., H, W) f64 -> (..., H - 10, W - 10): the Gaussian-weighted mean of every 11 x 11 window that lies inside the image."""
    g = taps()
    H, W = img.shape[-2:]
    rows = sum(g[k] * img[..., :, k:k + W - WINDOW + 1] for k in range(WINDOW))
    return sum(g[k] * rows[..., k:k + H - WINDOW + 1, :] for k in range(WINDOW))


def ssim_map(a, b):
    """(..., H, W) uint8 pair -> the SSIM index at every valid window position, (..., H - 10, W - 10) f64."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    mx, my = window_mean(x), window_mean(y)
    vx, vy, cxy = window_mean(x * x) - mx * mx, window_mean(y * y) - my * my, window_mean(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def frame_sums(a, b):
    """(n, C, H, W) uint8 pair -> (sse (n,) int64, sae (n,) int64, ssim_sum (n,) f64, n_win int)."""
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 4
    d = a.astype(np.int64) - b.astype(np.int64)
    n, C, H, W = a.shape
    return ((d * d).reshape(n, -1).sum(1), np.abs(d).reshape(n, -1).sum(1), ssim_map(a, b).reshape(n, -1).sum(1),
            C * (H - WINDOW + 1) * (W - WINDOW + 1))


def frame_metrics(a, b):
    """(..., C, H, W) uint8 pair -> dict of mse, mae, psnr (inf where mse == 0), ssim, each f64 of the leading shape."""
    lead, tail = a.shape[:-3], a.shape[-3:]
    sse, sae, ss, n_win = frame_sums(a.reshape(-1, *tail), b.reshape(-1, *tail))
    npix = float(np.prod(tail))
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(255.0 * 255.0 * npix / sse.astype(np.float64))
    return dict(mse=(sse / npix).reshape(lead), mae=(sae / npix).reshape(lead), psnr=psnr.reshape(lead), ssim=(ss / n_win).reshape(lead))


# ------------------------------------------------------------------ the cases of the kernel tests
SHAPES = [(1, 11, 11), (3, 12, 37), (3, 64, 80), (3, 75, 131), (3, 256, 256)]
CONTENTS = ["noise", "smooth", "flat", "identical", "black_white", "one_pixel"]


def make_pair(content, n, shape, seed=0):
    """A seeded (n, C, H, W) uint8 pair: uniform noise +-20 around a random image; a smooth sinusoid +-3; flat 255 against 254; identical;
    black against white; a pair differing in one pixel, at the last row and column of the last channel."""
    C, H, W = shape
    g = np.random.default_rng([seed, n, C, H, W, CONTENTS.index(content)])
    base = g.integers(0, 256, (n, C, H, W))
    if content == "noise":
        a, b = base, base + g.integers(-20, 21, base.shape)
    elif content == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ph = g.uniform(0, 2 * np.pi, (n, C, 1, 1))
        a = np.rint(127.5 + 100 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 - ph))
        b = a + np.rint(3 * np.sin(xx / 5.0 - 2 * ph))
    elif content == "flat":
        a, b = np.full(base.shape, 255), np.full(base.shape, 254)
    elif content == "identical":
        a, b = base, base.copy()
    elif content == "black_white":
        a, b = np.zeros(base.shape), np.full(base.shape, 255)
    elif content == "one_pixel":
        a, b = base, base.copy()
        b[:, -1, -1, -1] = (b[:, -1, -1, -1] + 128) % 256
    else:
        raise ValueError(content)
    return np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8)
