"""GPU (-m gpu): genie_frame_metrics against the f64 NumPy model (tests/image_metrics_model.py), its invariants (batch, run to run, stale
memory, 64-bit offsets), the Python layer, and the evaluator's image-space metrics against the model applied on the host to the same
decoded frames.

SSIM bar.  Per frame |mean SSIM (kernel) - mean SSIM (model)|.  The kernel accumulates every moment in f64 on pixels pivoted by 128; the
model does the same sums in f64 in another order on raw pixels, so the two differ by the rounding of f64 sums only.  Measured on an MI355X
over the whole case list below (60 cases): at most 6.23e-14, on the flat pair (255 against 254, where the model's own raw-pixel
sigma^2 = E[x^2] - mu^2 cancels twelve digits; smooth 4.7e-14, noise 1.2e-15, one pixel 6.7e-16, black / white 1.1e-16, identical 0;
DESIGN.md section 8.10 lists them).  The bar is 4x that, rounded up to one digit.  The condition on the arithmetic -- a bar of at most
1e-5, which a plain-f32 sigma^2 = E[x^2] - mu^2 misses on the flat pair -- is met with seven orders of magnitude to spare."""
import ast
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import image_metrics_model as M
from conftest import GOLDEN, pkg, record_measure
from stale_memory import poisoned, poison_tensor

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SSIM_BAR = 3e-13
assert SSIM_BAR <= 1e-5      # the condition on the arithmetic, whatever is measured


@functools.lru_cache(maxsize=None)
def case(content, n, shape):
    """(a, b, model sums) of one seeded case, computed once and shared; the arrays are read-only."""
    a, b = M.make_pair(content, n, shape)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, M.frame_sums(a, b)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()      # (a writable copy: the shared cases are read-only)


def sums_of(a, b):
    return pkg("image_metrics").frame_metric_sums(dev(a), dev(b)).cpu().numpy()


# ------------------------------------------------------------------ the kernel against the model
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_model(shape, n):
    worst = 0.0
    for content in M.CONTENTS:
        a, b, (sse, sae, ss, n_win) = case(content, n, shape)
        got = sums_of(a, b)
        assert got.shape == (n, 4) and got.dtype == np.float64
        assert np.array_equal(got[:, 0], sse.astype(np.float64)), (content, got[:, 0], sse)      # exact
        assert np.array_equal(got[:, 1], sae.astype(np.float64)), (content, got[:, 1], sae)      # exact
        assert np.all(got[:, 3] == n_win), (content, got[:, 3], n_win)
        d = float(np.abs(got[:, 2] / got[:, 3] - ss / n_win).max())
        print(f"ssim delta {content} n={n} {shape}: {d:.3e}")
        record_measure(f"image_metrics_ssim_delta_{content}_n{n}_{'x'.join(map(str, shape))}", d)
        worst = max(worst, d)
    assert worst <= SSIM_BAR, worst


def test_closed_forms_on_the_device():
    for shape in M.SHAPES[:4]:
        a, b, _ = case("identical", 5, shape)
        got = sums_of(a, b)
        assert np.all(got[:, :2] == 0) and np.array_equal(got[:, 2], got[:, 3])       # every window's index is exactly 1.0
        a, b, _ = case("black_white", 1, shape)
        got = sums_of(a, b)
        assert abs(got[0, 2] / got[0, 3] - (M.C1 * M.C2) / ((255.0 ** 2 + M.C1) * M.C2)) < 1e-15
        assert got[0, 0] == 255.0 ** 2 * np.prod(shape) and got[0, 1] == 255.0 * np.prod(shape)


@pytest.mark.parametrize("shape", M.SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_batch_invariance_and_determinism(shape):
    for content in ("noise", "smooth", "one_pixel"):
        a, b, _ = case(content, 5, shape)
        full = sums_of(a, b)
        assert np.array_equal(full, sums_of(a, b)), content                        # run to run: the same bits
        for i in range(5):
            assert np.array_equal(sums_of(a[i:i + 1], b[i:i + 1]), full[i:i + 1]), (content, i)
        assert np.array_equal(sums_of(a[::-1], b[::-1])[::-1], full), content


@pytest.mark.parametrize("shape", [(3, 12, 37), (3, 75, 131)], ids=lambda s: "x".join(map(str, s)))
def test_stale_memory_does_not_reach_the_results(shape):
    IM = pkg("image_metrics")
    a, b, _ = case("noise", 5, shape)
    da, db = dev(a), dev(b)
    clean = IM.frame_metric_sums(da, db)
    for byte in (0xFF, 0x3C):
        with poisoned(byte):         # out and the workspace come from torch.empty
            assert torch.equal(IM.frame_metric_sums(da, db), clean), hex(byte)
    # the same through the C ABI with buffers the test owns and a workspace larger than needed: nothing beyond the need is written
    lib = pkg("_lib").load()
    n, (C, H, W) = 5, shape
    need = lib.genie_frame_metrics_workspace_bytes(n, C, H, W)
    out = poison_tensor(torch.empty(n + 1, 4, dtype=torch.float64, device="cuda"), 0xFF)
    ws = poison_tensor(torch.empty(need + 64, dtype=torch.uint8, device="cuda"), 0xFF)
    rc = lib.genie_frame_metrics(da.data_ptr(), db.data_ptr(), n, C, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(out[:n], clean) and bool(torch.isnan(out[n]).all())
    assert bool((ws[need:] == 0xFF).all())


def test_empty_batch_and_small_frames_touch_nothing():
    L = pkg("_lib")
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    a = torch.zeros(2, 3, 10, 16, dtype=torch.uint8, device="cuda")
    out = poison_tensor(torch.empty(2, 4, dtype=torch.float64, device="cuda"), 0xFF)
    ws = poison_tensor(torch.empty(1024, dtype=torch.uint8, device="cuda"), 0xFF)
    args = (out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert lib.genie_frame_metrics(a.data_ptr(), a.data_ptr(), 0, 3, 16, 10, *args) == L.E_SHAPE
    assert lib.genie_frame_metrics(a.data_ptr(), a.data_ptr(), 2, 3, 10, 16, *args) == L.E_SHAPE      # H = 10
    assert b"11 x 11" in lib.genie_last_error()
    assert lib.genie_frame_metrics(a.data_ptr(), a.data_ptr(), 0, 3, 16, 16, *args) == 0              # n = 0: success
    assert lib.genie_frame_metrics(a.data_ptr(), a.data_ptr(), 2, 3, 16, 16, out.data_ptr(), ws.data_ptr(), 8, st) == L.E_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((ws == 0xFF).all())
    IM = pkg("image_metrics")
    e = IM.frame_metrics(a.new_zeros(0, 3, 16, 16), a.new_zeros(0, 3, 16, 16))
    assert all(tuple(t.shape) == (0,) and t.dtype == torch.float64 and t.is_cuda for t in e)
    with pytest.raises(ValueError, match="11 x 11"):
        IM.frame_metrics(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IM.frame_metrics(a.new_zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16, dtype=torch.uint8))


def test_element_offsets_past_2_31():
    """More than 2^31 pixels per batch: the last pair, whose offsets no 32-bit index reaches, has the bits of the same pair alone, and the
    identical pairs in front of it score exactly 0 / 0 / n_win."""
    IM = pkg("image_metrics")
    C, H, W = 3, 256, 256
    n = (1 << 31) // (C * H * W) + 2
    assert (n - 1) * C * H * W > (1 << 31)
    g = torch.Generator(device="cuda").manual_seed(7)
    a = torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8, device="cuda", generator=g)
    b = a.clone()
    pa, pb, _ = case("noise", 1, (C, H, W))
    a[-1], b[-1] = dev(pa[0]), dev(pb[0])
    got = IM.frame_metric_sums(a, b)
    alone = IM.frame_metric_sums(a[-1:], b[-1:])
    n_win = float(C * (H - 10) * (W - 10))
    assert torch.equal(got[-1:], alone) and float(alone[0, 0]) > 0
    want = torch.tensor([0.0, 0.0, n_win, n_win], dtype=torch.float64, device="cuda")
    assert bool((got[:-1] == want).all())


# ------------------------------------------------------------------ the Python layer
def test_frame_metrics_keeps_the_leading_shape_and_psnr_is_from_the_exact_sse():
    IM = pkg("image_metrics")
    a, b = M.make_pair("noise", 6, (3, 12, 37), seed=3)
    a, b = a.reshape(2, 3, 3, 12, 37).copy(), b.reshape(2, 3, 3, 12, 37).copy()
    b[1, 2] = a[1, 2]                                  # one identical pair
    fm = IM.frame_metrics(dev(a), dev(b))
    want = M.frame_metrics(a, b)
    sse = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).reshape(2, 3, -1).sum(-1)
    N = 3 * 12 * 37
    for name in ("mse", "mae", "psnr", "ssim"):
        t = getattr(fm, name)
        assert tuple(t.shape) == (2, 3) and t.dtype == torch.float64 and t.is_cuda, name
    assert np.array_equal(fm.mse.cpu().numpy(), sse / N) and np.array_equal(fm.mae.cpu().numpy(), want["mae"])
    psnr = fm.psnr.cpu().numpy()
    assert np.isposinf(psnr[1, 2]) and float(fm.mse[1, 2]) == 0 and float(fm.ssim[1, 2]) == 1.0
    fin = np.isfinite(psnr)
    assert fin.sum() == 5
    with np.errstate(divide="ignore"):
        ref = 10 * np.log10(255.0 ** 2 * N / sse)
    assert np.allclose(psnr[fin], ref[fin], rtol=1e-12, atol=0)
    assert np.abs(fm.ssim.cpu().numpy() - want["ssim"]).max() <= SSIM_BAR
    # non-contiguous views are taken as they index, and the eval_utils wrapper flattens in (b t) order with the cap applied
    v = IM.frame_metrics(dev(a).transpose(0, 1), dev(b).transpose(0, 1))
    assert torch.equal(v.ssim, fm.ssim.t()) and torch.equal(v.mse, fm.mse.t())
    lists = pkg("eval_utils").compute_image_metrics(dev(b), dev(a), psnr_cap=100.0)
    assert sorted(lists) == ["mse", "psnr", "ssim"] and all(len(x) == 6 and isinstance(x[0], float) for x in lists.values())
    assert lists["psnr"][5] == 100.0 and lists["mse"] == fm.mse.flatten().tolist()
    assert np.isposinf(pkg("eval_utils").compute_image_metrics(dev(b), dev(a))["psnr"][5])


# ------------------------------------------------------------------ tokenizer and evaluator
@pytest.fixture(scope="module")
def tiny_vq():
    """The tiny tokenizer of tests/test_hip_conv.py::test_encoder_batch_invariance: two levels, so a 16 x 16 token grid is a 32 x 32 frame."""
    mv = pkg("magvit2")
    z = np.load(f"{GOLDEN}/magvit_mid.npz")
    m = mv.VQModel(mv.VQConfig(**ast.literal_eval(str(z["cfg"]))))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in mv.make_vq_state_dict(m, int(z["weight_seed"])).items()})
    return m.to("cuda").eval(), torch.from_numpy(z["enc_frames"]).cuda()


def test_reconstruction_metrics_is_encode_decode_score(tiny_vq):
    vq, frames = tiny_vq
    IM = pkg("image_metrics")
    got = vq.reconstruction_metrics(frames)
    rec = vq.decode_tokens(vq.encode_tokens(frames))
    assert rec.shape == frames.shape and rec.dtype == torch.uint8
    want = IM.frame_metrics(rec, frames)
    for g, w in zip(got, want):
        assert tuple(g.shape) == (3,) and torch.equal(g, w)
    host = M.frame_metrics(rec.cpu().numpy(), frames.cpu().numpy())
    assert np.abs(got.ssim.cpu().numpy() - host["ssim"]).max() <= SSIM_BAR and np.array_equal(got.mse.cpu().numpy(), host["mse"])
    assert float(got.mse.min()) > 0           # a lossy round trip: the metric has something to say


@pytest.fixture(scope="module")
def tiny_eval(tiny_vq):
    """A 2-layer synthetic STMaskGIT at the real token geometry (T = 16, S = 256), 3 clips, and evaluators with the tiny tokenizer."""
    vq, _ = tiny_vq
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False,
                                    use_mup=False)
    sd = pkg("synthetic").make_state_dict(cfg, seed=22, law="conditioned")
    clips = torch.from_numpy(pkg("synthetic").make_clips(3, cfg, seed=5)).cuda()
    model = pkg("st_mask_git").STMaskGIT(cfg, precision="f16x3").load_numpy_state_dict(sd).to("cuda")
    dec = pkg("magvit2").decode_latents_wrapper(batch_size=16, model=vq, device="cuda")

    def make(steps):
        args = SimpleNamespace(maskgit_steps=steps, temperature=0, latent_h=16, latent_w=16)
        return pkg("evaluate").GenieEvaluator(args, dec, "cuda", model=model)
    return cfg, clips, make


def host_per_horizon(ev, clips, samples, psnr_cap=100.0):
    """The model on the host over the frames predict_next_frames and decode_tokens return: (mse, capped psnr, ssim), each (N, T-1)."""
    T = ev.model.config.T
    pred = ev.predict_next_frames(samples).cpu().numpy()
    gt = pkg("eval_utils").decode_tokens(clips.view(-1, T, 16, 16)[:, 1:], ev.decode_latents).cpu().numpy()
    assert pred.shape == gt.shape == (clips.shape[0], T - 1, 3, 32, 32) and pred.dtype == np.uint8
    h = M.frame_metrics(pred, gt)
    return h["mse"], np.minimum(h["psnr"], psnr_cap), h["ssim"]


@pytest.mark.parametrize("reuse", [True, False], ids=["reuse", "full"])
def test_evaluate_clips_image_metrics(tiny_eval, reuse):
    cfg, clips, make = tiny_eval
    E = pkg("evaluate")
    ev = make(2)
    off = E.evaluate_clips(ev, clips, batch_size=2, noise_seed=100, reuse=reuse)
    on = E.evaluate_clips(ev, clips, batch_size=2, noise_seed=100, reuse=reuse, image_metrics=True)
    assert sorted(off) == ["acc", "clips", "frames", "frames_per_sec", "loss", "seconds"]
    for k in ("loss", "acc", "frames", "clips"):
        assert on[k] == off[k], k                     # the same bits
    assert set(on) - set(off) == {"psnr", "ssim", "mse", "psnr_per_frame", "ssim_per_frame", "mse_per_frame"}
    # the frames behind those numbers: the same draws, batch by batch
    n_h = cfg.T - 1
    rows = []
    for i in range(0, 3, 2):
        batch = clips[i:i + 2]
        g = torch.Generator(device="cpu").manual_seed(100 + i)
        noise = torch.rand(n_h, 1, batch.shape[0], cfg.S, generator=g).cuda()
        fn = ev.evaluate_metric_sums_reuse if reuse else ev.evaluate_metric_sums
        _, samples = fn(batch, noise=noise, return_samples=True)
        assert tuple(samples.shape) == (batch.shape[0], n_h, 16, 16)
        rows.append(host_per_horizon(ev, batch, samples))
    mse, psnr, ssim = (np.concatenate([r[k] for r in rows]) for k in range(3))
    for key, want, tol in (("mse", mse, None), ("psnr", psnr, None), ("ssim", ssim, SSIM_BAR)):
        got = np.array(on[key + "_per_frame"])
        assert got.shape == (n_h,)
        if tol is None:
            assert np.allclose(got, want.mean(0), rtol=1e-12, atol=0), key
            assert abs(on[key] - want.mean()) <= 1e-12 * abs(want.mean()), key
        else:
            assert np.abs(got - want.mean(0)).max() <= tol and abs(on[key] - want.mean()) <= tol, key
    assert 0 < on["psnr"] < 100 and -1 <= on["ssim"] < 1 and on["mse"] > 0
    # two shards' totals add up to the job's: what the all-reduce of the per-horizon sums does (shard boundary = a batch boundary)
    s0 = E.evaluate_clips(ev, clips[:2], batch_size=2, noise_seed=100, reuse=reuse, image_metrics=True)
    s1 = E.evaluate_clips(ev, clips[2:], batch_size=2, noise_seed=100, reuse=reuse, image_metrics=True, clip_offset=2)
    for key in ("psnr", "ssim", "mse"):
        both = (2 * np.array(s0[key + "_per_frame"]) + np.array(s1[key + "_per_frame"])) / 3
        assert np.allclose(both, on[key + "_per_frame"], rtol=1e-13, atol=0), key


def test_psnr_cap_counts_perfect_frames(tiny_eval):
    """Predicted tokens equal to the ground truth decode to the same frames: mse 0, and the running mean counts them at the cap."""
    cfg, clips, make = tiny_eval
    ev = make(1)
    s = ev.image_metric_sums(clips[:2], clips[:2].view(2, cfg.T, 16, 16)[:, 1:].contiguous(), psnr_cap=60.0).cpu().numpy()
    assert s.shape == (4, cfg.T - 1)
    assert np.all(s[0] == 0) and np.all(s[1] == 120.0) and np.all(s[2] == 2.0) and np.all(s[3] == 2.0)


def test_reference_style_loop_decodes_and_scores(tiny_eval):
    cfg, clips, make = tiny_eval
    E = pkg("evaluate")
    ev = make(1)                     # one MaskGIT step: no unmasking draws, so two runs sample the same frames
    batches = [{"input_ids": clips[i:i + 2], "labels": clips[i:i + 2]} for i in (0, 2)]
    off = E.run_reference_style_loop(ev, batches, verbose=False)
    on = E.run_reference_style_loop(ev, batches, verbose=False, decode_image_metrics=True)
    assert sorted(off) == ["acc", "gen_time", "loss"]
    assert sorted(on) == ["acc", "dec_time", "gen_time", "loss", "pred_mse", "pred_psnr", "pred_ssim"]
    for k in ("loss", "acc"):
        assert (on[k].total, on[k].count) == (off[k].total, off[k].count), k
    samples = torch.cat([ev.predict_zframe_logits(b["input_ids"], return_logits=False)[0] for b in batches])
    mse, psnr, ssim = host_per_horizon(ev, clips, samples)
    assert on["pred_psnr"].count == on["pred_ssim"].count == on["pred_mse"].count == 3 * (cfg.T - 1)
    assert abs(on["pred_mse"].mean() - mse.mean()) <= 1e-12 * mse.mean()
    assert abs(on["pred_psnr"].mean() - psnr.mean()) <= 1e-12 * psnr.mean()
    assert abs(on["pred_ssim"].mean() - ssim.mean()) <= SSIM_BAR
    # without a decoder the keyword changes nothing
    bare = E.GenieEvaluator(ev.args, None, "cuda", model=ev.model)
    assert sorted(E.run_reference_style_loop(bare, batches[:1], verbose=False, decode_image_metrics=True)) == ["acc", "gen_time", "loss"]
