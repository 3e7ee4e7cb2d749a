"""Continuous per-frame action vectors on the HIP path (genie_action_proj: genie_action_rows / genie_action_rows_backward, and the
action_vectors argument of every public path).  Two layers of pinning, neither needing a reference implementation:
  * the two kernels against the NumPy f32 restatement of the order include/genie_hip.h states (bit for bit) and, independently, against
    f64 within the standard bound of sequentially rounded sums;
  * the model against the DISCRETE path it reuses: a model with action_dim on vectors v must equal, bit for bit, a model with
    action_vocab_size = 1 + B T whose table is [null row ; NumPy projection of v] on the ids that address it -- over the inference
    battery, guidance, the rollout and the training step.
Needs a GPU: -m gpu."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg
from oracle import genie_train_oracle as TO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECISIONS = ["exact", "f16x3", "bf16"]
AD = 5          # action_dim of the model tests
STEPS = 2
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ------------------------------------------------------------------ the NumPy f32 restatement (include/genie_hip.h, genie_action_proj)
def np_z(v, mean=None, inv_std=None):
    z = np.asarray(v, F32)
    if mean is not None:
        z = z - mean[None]
    if inv_std is not None:
        z = z * inv_std[None]
    return z


def np_rows(W, bias, z):
    acc = np.zeros((z.shape[0], W.shape[0]), F32) if bias is None else np.repeat(bias[None], z.shape[0], 0).astype(F32)
    for j in range(W.shape[1]):                       # j ascending; product and sum rounded separately
        acc = acc + (W[None, :, j] * z[:, j, None])
    return acc


def np_backward(z, d_rows):
    dW, db = np.zeros((d_rows.shape[1], z.shape[1]), F32), np.zeros(d_rows.shape[1], F32)
    for r in range(z.shape[0]):                       # n ascending, strictly in sequence
        dW = dW + (d_rows[r][:, None] * z[r][None, :])
        db = db + d_rows[r]
    return dW, db


# ------------------------------------------------------------------ the two kernels
SHAPES = [(1, 1, 64), (3, 5, 64), (17, 25, 320), (300, 7, 1024)]


def kernel_case(n, A, d, bias, norm, seed=0):
    """Inputs scaled so that some W z terms cancel: z of both signs, and pairs of equal-magnitude weight columns of opposite sign."""
    g = np.random.default_rng([seed, n, A, d])
    W = g.standard_normal((d, A)).astype(F32)
    v = g.standard_normal((n, A)).astype(F32)
    if A >= 2:
        W[:, 1] = -W[:, 0] * F32(1 + 2 ** -20)
        v[:, 1] = v[:, 0]
    b = (0.05 * g.standard_normal(d)).astype(F32) if bias else None
    mean = (0.3 * g.standard_normal(A)).astype(F32) if norm else None
    inv_std = (F32(1) / (0.5 + g.random(A)).astype(F32)).astype(F32) if norm else None
    d_rows = g.standard_normal((n, d)).astype(F32)
    return W, b, mean, inv_std, v, d_rows


def proj_struct(L, W, b, mean, inv_std, keep):
    t = {k: (None if a is None else dev(a)) for k, a in (("w", W), ("b", b), ("m", mean), ("s", inv_std))}
    keep.append(t)
    return L.ActionProj(weight=t["w"].data_ptr(), bias=None if b is None else t["b"].data_ptr(),
                        mean=None if mean is None else t["m"].data_ptr(), inv_std=None if inv_std is None else t["s"].data_ptr(),
                        action_dim=W.shape[1])


def run_rows(p, v, d):
    L = pkg("_lib")
    vv, out = dev(v), torch.full((v.shape[0], d), float("nan"), device="cuda")
    L.check(L.load().genie_action_rows(p, vv.data_ptr(), out.data_ptr(), v.shape[0], d, torch.cuda.current_stream().cuda_stream),
            "genie_action_rows")
    return out.cpu().numpy()


def run_backward(p, v, d_rows, A, dW=None, db=None, accumulate=0, bias=True):
    L = pkg("_lib")
    d = d_rows.shape[1]
    vv, dr = dev(v), dev(d_rows)
    dW = torch.full((d, A), float("nan"), device="cuda") if dW is None else dW
    db = (torch.full((d,), float("nan"), device="cuda") if db is None else db) if bias else None
    L.check(L.load().genie_action_rows_backward(p, vv.data_ptr(), dr.data_ptr(), v.shape[0], d, dW.data_ptr(),
                                                None if db is None else db.data_ptr(), accumulate,
                                                torch.cuda.current_stream().cuda_stream), "genie_action_rows_backward")
    return dW, db


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n,A,d", SHAPES)
def test_forward_kernel(n, A, d, bias, norm):
    L, keep = pkg("_lib"), []
    W, b, mean, inv_std, v, _ = kernel_case(n, A, d, bias, norm)
    got = run_rows(proj_struct(L, W, b, mean, inv_std, keep), v, d)
    z = np_z(v, mean, inv_std)
    assert np.array_equal(got.view(np.uint32), np_rows(W, b, z).view(np.uint32))          # the stated order, bit for bit
    # ... and independently against f64 on the same f32 z: A sequentially rounded products and adds
    z64, W64 = z.astype(np.float64), W.astype(np.float64)
    ref = z64 @ W64.T + (0 if b is None else b.astype(np.float64)[None])
    mag = np.abs(z64) @ np.abs(W64).T + (0 if b is None else np.abs(b.astype(np.float64))[None])
    err = np.abs(got.astype(np.float64) - ref)
    print(f"forward {n, A, d}: max err / bound = {(err / (A * 2.0 ** -23 * mag + 1e-300)).max():.3f}")
    assert np.all(err <= A * 2.0 ** -23 * mag)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n,A,d", SHAPES)
def test_backward_kernel(n, A, d, bias, norm):
    L, keep = pkg("_lib"), []
    W, b, mean, inv_std, v, d_rows = kernel_case(n, A, d, bias, norm)
    p = proj_struct(L, W, b, mean, inv_std, keep)
    dW, db = run_backward(p, v, d_rows, A, bias=bias)
    z = np_z(v, mean, inv_std)
    wW, wb = np_backward(z, d_rows)
    gW = dW.cpu().numpy()
    assert np.array_equal(gW.view(np.uint32), wW.view(np.uint32))
    if bias:
        assert np.array_equal(db.cpu().numpy().view(np.uint32), wb.view(np.uint32))
    z64, g64 = z.astype(np.float64), d_rows.astype(np.float64)
    err = np.abs(gW.astype(np.float64) - g64.T @ z64)
    bound = (n + 1) * 2.0 ** -23 * (np.abs(g64).T @ np.abs(z64))
    print(f"backward {n, A, d}: max err / bound = {(err / (bound + 1e-300)).max():.3f}")
    assert np.all(err <= bound)
    if bias:
        assert np.all(np.abs(db.cpu().numpy().astype(np.float64) - g64.sum(0)) <= (n + 1) * 2.0 ** -23 * np.abs(g64).sum(0))
    # two identical calls: identical bytes
    dW2, db2 = run_backward(p, v, d_rows, A, bias=bias)
    assert torch.equal(dW, dW2) and (not bias or torch.equal(db, db2))
    # accumulate = 1 after accumulate = 0: the f32 sum of the two results (one add)
    _, _, _, _, v3, d_rows3 = kernel_case(n, A, d, bias, norm, seed=1)
    dW3, db3 = run_backward(p, v3, d_rows3, A, bias=bias)
    accW, accb = run_backward(p, v3, d_rows3, A, dW=dW.clone(), db=db.clone() if bias else None, accumulate=1, bias=bias)
    assert np.array_equal(accW.cpu().numpy(), gW + dW3.cpu().numpy())
    if bias:
        assert np.array_equal(accb.cpu().numpy(), db.cpu().numpy() + db3.cpu().numpy())


def test_rows_are_independent_of_the_batch():
    L, keep = pkg("_lib"), []
    n, A, d = 300, 7, 1024
    W, b, mean, inv_std, v, _ = kernel_case(n, A, d, True, True)
    p = proj_struct(L, W, b, mean, inv_std, keep)
    full = run_rows(p, v, d)
    for i in (0, 137, 299):
        assert np.array_equal(run_rows(p, v[i:i + 1], d)[0].view(np.uint32), full[i].view(np.uint32)), i
    # n == 0: success, nothing written
    out = torch.full((1, d), 7.0, device="cuda")
    assert L.load().genie_action_rows(p, out.data_ptr(), out.data_ptr(), 0, d, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ the model against the discrete path on the projected table
def cfgs(n_rows, ad=AD, **kw):
    args = dict(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    args.update(kw)
    C = pkg("config").GenieConfig
    return C(**args), C(**args, action_vocab_size=n_rows), C(**args, action_dim=ad)


def proj_weights(d, ad=AD, seed=3, zero=False):
    g = np.random.default_rng(seed)
    if zero:
        return {"action_proj.weight": np.zeros((d, ad), F32), "action_proj.bias": np.zeros(d, F32), "action_null": np.zeros(d, F32),
                "action_mean": np.zeros(ad, F32), "action_std": np.ones(ad, F32)}
    return {"action_proj.weight": (0.3 * g.standard_normal((d, ad))).astype(F32), "action_proj.bias": (0.1 * g.standard_normal(d)).astype(F32),
            "action_null": (0.5 * g.standard_normal(d)).astype(F32), "action_mean": (0.2 * g.standard_normal(ad)).astype(F32),
            "action_std": (0.5 + g.random(ad)).astype(F32)}


def projected_table(pw, vecs_nA):
    """[null row ; NumPy projection of the (n, A) vectors]: the action table of the equivalent discrete model."""
    z = np_z(vecs_nA, pw["action_mean"], (F32(1) / pw["action_std"]).astype(F32))
    return np.concatenate([pw["action_null"][None], np_rows(pw["action_proj.weight"], pw["action_proj.bias"], z)]).astype(F32)


def model(cfg, sd, precision):
    return pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")


def evaluator(m):
    return pkg("evaluate").GenieEvaluator(SimpleNamespace(maskgit_steps=STEPS, temperature=0.0, latent_h=16, latent_w=16),
                                          None, "cuda", model=m)


def clips(B, cfg, seed):
    ids = dev(pkg("synthetic").make_clips(B, cfg, seed=seed)).view(B, cfg.T, cfg.S)
    ids[:, 2, ::5] = cfg.image_vocab_size
    return ids


def battery(m, ids, key, act, noise_seed=9, guidance=None):
    """Every inference entry point that embeds token ids (the battery of tests/test_hip_actions.py), the actions passed as `key`
    ("action_ids" / "action_vectors" / None)."""
    G = pkg("generate")
    cfg = m.config
    B, T, S = ids.shape
    H = 16
    out = {}
    kw = {} if key is None else {key: act}
    kw7 = {} if key is None else {key: act[:, :7]}
    gk = {} if guidance is None else {"guidance": guidance}
    g = torch.Generator(device="cpu").manual_seed(noise_seed)
    x = ids.view(B, T, H, H)
    if guidance is None:
        out["compute_logits"] = m.compute_logits(x, **kw)
    p = x.clone()
    p[:, 5:] = cfg.image_vocab_size
    noise = torch.rand(STEPS - 1, B, S, generator=g).cuda()
    s, lg = m.maskgit_generate(p, 5, maskgit_steps=STEPS, noise=noise, **kw, **gk)
    out["maskgit_samples"], out["maskgit_logits0"], out["maskgit_prompt"] = s, lg, p
    nz = torch.rand(4, STEPS - 1, B, S, generator=g).cuda()
    out["generate_kv"] = m.generate(ids[:, :4].reshape(B, -1), max_new_tokens=3 * S, maskgit_steps=STEPS, noise=nz[:3],
                                    return_logits=True, kv_cache=True, **kw7, **gk)
    out["generate_full"] = m.generate(ids[:, :12].reshape(B, -1), max_new_tokens=4 * S, maskgit_steps=STEPS, noise=nz,
                                      return_logits=True, kv_cache=False, **kw, **gk)
    for P in (1, 8, 15):
        nzP = torch.rand(T - P, STEPS - 1, B, S, generator=g).cuda()
        for tf in (False, True):
            for host in (False, True):
                out[f"cached_P{P}_tf{int(tf)}_host{int(host)}"] = G.generate_frames_cached(
                    m, x, num_prompt_frames=P, maskgit_steps=STEPS, teacher_force_time=tf, noise=nzP, host_loop=host, **kw, **gk)
    if guidance is None:
        ev = evaluator(m)
        nzE = torch.rand(T - 1, STEPS - 1, B, S, generator=g).cuda()
        out["reuse_samples"], out["reuse_logits"] = ev.predict_zframe_logits_reuse(ids.reshape(B, -1), noise=nzE, **kw)
        out["metric_sums_reuse"] = ev.evaluate_metric_sums_reuse(ids.reshape(B, -1), noise=nzE, **kw)
    return out


def flat(v):
    return [t for t in (v if isinstance(v, tuple) else (v,)) if t is not None]


def assert_bit_identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        for x, y in zip(flat(a[k]), flat(b[k])):
            assert torch.equal(x, y), k


def pair(precision, B=2, seed=21, zero=False):
    """(unconditioned model, id model on the projected table, vector model, clips, ids, vectors): a different vector per frame and clip."""
    c0, ci, cv = cfgs(1 + B * 16)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=seed)
    pw = proj_weights(c0.d_model, zero=zero)
    v = np.random.default_rng(seed + 1).standard_normal((B, c0.T, AD)).astype(F32)
    mi = model(ci, dict(sd0, **{"action_embed.weight": projected_table(pw, v.reshape(B * c0.T, AD))}), precision)
    mv = model(cv, dict(sd0, **pw), precision)
    rows = dev(1 + np.arange(B * c0.T).reshape(B, c0.T))
    return (c0, sd0), mi, mv, clips(B, c0, seed + 2), rows, dev(v)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_vectors_equal_ids_on_the_projected_table(precision):
    (c0, sd0), mi, mv, ids, rows, v = pair(precision)
    got = battery(mv, ids, "action_vectors", v)
    assert_bit_identical(got, battery(mi, ids, "action_ids", rows))
    # and the vectors matter
    m0 = model(c0, sd0, precision)
    assert not torch.equal(got["compute_logits"], m0.compute_logits(ids.view(2, c0.T, 16, 16)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_projection_is_the_unconditioned_model(precision):
    (c0, sd0), _, mv, ids, _, v = pair(precision, seed=24, zero=True)
    assert_bit_identical(battery(mv, ids, "action_vectors", v), battery(model(c0, sd0, precision), ids, None, None))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_guidance_uses_the_model_s_null_row(precision):
    Gd = pkg("sampling").Guidance
    _, mi, mv, ids, rows, v = pair(precision, seed=27)
    # scale 3: maskgit_generate, generate and generate_frames_cached (both loop forms), all against the id model under null_action = 0
    assert_bit_identical(battery(mv, ids, "action_vectors", v, guidance=Gd(3.0)), battery(mi, ids, "action_ids", rows, guidance=Gd(3.0, 0)))
    x = ids.view(2, 16, 16, 16)
    G = pkg("generate")
    nz = torch.rand(8, STEPS - 1, 2, 256, generator=torch.Generator().manual_seed(4)).cuda()
    run = lambda m, **kw: G.generate_frames_cached(m, x, num_prompt_frames=8, maskgit_steps=STEPS, noise=nz, **kw)
    assert torch.equal(run(mv, action_vectors=v, guidance=Gd(1.0)), run(mv, action_vectors=v))                 # scale 1: unguided
    assert torch.equal(run(mv, action_vectors=v, guidance=Gd(0.0)), run(mi, action_ids=torch.zeros_like(rows)))  # scale 0: the null stream
    with pytest.raises(ValueError):
        run(mv, action_vectors=v, guidance=Gd(3.0, 2))     # the null row's index is the model's, not the caller's


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rollout_past_the_window(precision):
    """T = 16, P = 4, keep = 8, 20 new frames (two slides): rollout_frames on vectors == the id model on the frame-major projected table,
    and Rollout.step frame by frame (each projecting only its own B vectors) == rollout_frames."""
    G = pkg("generate")
    B, P, keep, n_new = 2, 4, 8, 20
    cap = P + n_new
    c0, ci, cv = cfgs(1 + B * cap)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=61)
    pw = proj_weights(c0.d_model, seed=5)
    v = np.random.default_rng(62).standard_normal((B, cap, AD)).astype(F32)
    table = projected_table(pw, v.transpose(1, 0, 2).reshape(cap * B, AD))      # row 1 + f B + b
    rows = dev(1 + np.arange(cap)[None, :] * B + np.arange(B)[:, None])
    mi = model(ci, dict(sd0, **{"action_embed.weight": table}), precision)
    mv = model(cv, dict(sd0, **pw), precision)
    prompt = clips(B, c0, 63)[:, :P].reshape(B, P, 16, 16)
    nz = torch.rand(n_new, STEPS - 1, B, 256, generator=torch.Generator().manual_seed(5)).cuda()
    want = G.rollout_frames(mi, prompt, n_new, keep=keep, maskgit_steps=STEPS, noise=nz, action_ids=rows)
    got = G.rollout_frames(mv, prompt, n_new, keep=keep, maskgit_steps=STEPS, noise=nz, action_vectors=dev(v))
    assert torch.equal(got, want)
    assert torch.equal(mv.rollout(prompt, n_new, keep=keep, maskgit_steps=STEPS, noise=nz, action_vectors=dev(v)), want)
    r = G.Rollout(mv, prompt, keep=keep, prompt_vectors=dev(v[:, :P]), maskgit_steps=STEPS, capacity=8)   # (capacity 8: the buffers grow twice)
    for k in range(n_new):
        r.step(dev(v[:, P + k]), noise=nz[k])
    assert torch.equal(r.frames, want)
    r2 = G.Rollout(mv, prompt, keep=keep, prompt_vectors=dev(v[:, :P]), maskgit_steps=STEPS)
    r2.extend(7, noise=nz[:7], action_vectors=dev(v[:, P:P + 7]))
    r2.extend(13, noise=nz[7:], action_vectors=dev(v[:, P + 7:]))
    assert torch.equal(r2.frames, want)


# ------------------------------------------------------------------ training
def train_cfgs(B):
    return cfgs(1 + B * 4, num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_prompt_frames=2)


def trainer(cfg, sd, precision):
    return pkg("train").GenieTrainer(model(cfg, sd, precision))


NEW = ("action_proj.weight", "action_proj.bias", "action_null")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_training_step_equals_the_id_model_and_the_projection_gradients(precision, B):
    c0, ci, cv = train_cfgs(B)
    syn = pkg("synthetic")
    sd0 = syn.make_state_dict(c0, seed=31)
    pw = proj_weights(c0.d_model, seed=9)
    v = np.random.default_rng(34).standard_normal((B, c0.T, AD)).astype(F32)
    z = np_z(v.reshape(-1, AD), pw["action_mean"], (F32(1) / pw["action_std"]).astype(F32))
    rows = 1 + np.arange(B * c0.T).reshape(B, c0.T)
    batch = TO.maskgit_collate(syn.make_clips(B, c0, seed=32), c0, TO.NumpyDraws(33))
    ids, lab = dev(batch["input_ids"]), dev(batch["labels"])
    ti = trainer(ci, dict(sd0, **{"action_embed.weight": projected_table(pw, v.reshape(-1, AD))}), precision)
    tv = trainer(cv, dict(sd0, **pw), precision)

    def check(drop):
        r = np.where(drop[:, None], 0, rows)
        li, _ = ti.forward_backward(ids, lab, action_ids=dev(r))
        lv, _ = tv.forward_backward(ids, lab, action_vectors=dev(v), action_drop=dev(drop) if drop.any() else None)
        assert float(li) == float(lv)
        gi, gv = ti.gradients(), tv.gradients()
        assert set(gv) == (set(gi) - {"action_embed.weight"}) | set(NEW)
        for k in gv:
            if k not in NEW:
                assert torch.equal(gv[k], gi[k]), k
        dt = gi["action_embed.weight"].cpu().numpy()
        wW, wb = np_backward(z, dt[1:])
        assert np.array_equal(gv["action_proj.weight"].cpu().numpy().view(np.uint32), wW.view(np.uint32))
        assert np.array_equal(gv["action_proj.bias"].cpu().numpy().view(np.uint32), wb.view(np.uint32))
        assert np.array_equal(gv["action_null"].cpu().numpy(), dt[0])
        return dt

    dt = check(np.zeros(B, bool))
    assert np.all(dt[0] == 0) and np.any(dt[1:] != 0)
    g1 = tv.grads.clone()
    tv.forward_backward(ids, lab, action_vectors=dev(v))                       # bit-reproducible run to run
    assert torch.equal(g1, tv.grads)
    # every clip dropped: of the three new tensors only the null row gets a gradient, the id model's null-row gradient
    dt = check(np.ones(B, bool))
    gv = tv.gradients()
    assert np.any(dt[0] != 0) and not bool(gv["action_proj.weight"].any()) and not bool(gv["action_proj.bias"].any())
    if B > 1:
        check(np.arange(B) % 2 == 1)
    # accumulate adds (the criterion of test_training_step_folds_and_the_table_gradient)
    v2 = np.random.default_rng(35).standard_normal((B, c0.T, AD)).astype(F32)
    tv.forward_backward(ids, lab, action_vectors=dev(v2))
    g2 = tv.grads.clone()
    tv.forward_backward(ids, lab, action_vectors=dev(v))
    tv.forward_backward(ids, lab, action_vectors=dev(v2), accumulate=True)
    assert float((tv.grads - (g1 + g2)).abs().max()) <= 1e-6 * float(g1.abs().max())


TRAIN_STEPS = 200
CE_RATIO = 0.1   # measured: 0.285 vs 57.7 after 200 steps (ratio 0.005, a factor 20 of margin)


def test_training_learns_to_use_the_vectors():
    """The recipe of test_training_learns_to_use_the_actions with A = 2: the action of pattern k is a fixed 2-vector per k plus small
    noise.  After 200 seeded steps the masked CE under the true vectors must be below CE_RATIO times the CE under shuffled vectors.
    Measured on an MI355X: masked CE 0.2851 under the true vectors, 57.6737 shuffled."""
    D = pkg("data")
    _, _, cv = cfgs(0, ad=2, num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_prompt_frames=1)
    torch.manual_seed(0)
    random.seed(0)
    m = pkg("st_mask_git").STMaskGIT(cv).to("cuda")
    m.init_weights()
    tr = pkg("train").GenieTrainer(m, lr=3e-3)
    g = np.random.default_rng(0)
    pattern = g.integers(0, 512, (4, cv.S)) * 513
    centre = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], F32)

    def make(n):
        k = g.integers(0, 4, (n, cv.T))
        vec = centre[k] + (0.05 * g.standard_normal((n, cv.T, 2))).astype(F32)
        return dev(pattern[k].reshape(n, -1)), dev(vec.astype(F32))

    for _ in range(TRAIN_STEPS):
        x, vec = make(16)
        tr.train_step(D.maskgit_collate(x, cv, action_vectors=vec))
    x, vec = make(64)
    masked = x.clone()
    masked[:, cv.S:] = cv.image_vocab_size
    shuffled = vec[torch.randperm(64, device="cuda")]
    ce_true = float(m(masked, x, action_vectors=vec).loss)
    ce_shuf = float(m(masked, x, action_vectors=shuffled).loss)
    print(f"after {TRAIN_STEPS} steps: masked CE {ce_true:.4f} with the true vectors, {ce_shuf:.4f} shuffled")
    assert ce_true < CE_RATIO * ce_shuf, (ce_true, ce_shuf)


def test_input_errors_raise_before_anything_is_enqueued():
    c0, ci, cv = cfgs(6, num_layers=1)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=51)
    mv = model(cv, dict(sd0, **proj_weights(c0.d_model)), "exact")
    mi = model(ci, dict(sd0, **{"action_embed.weight": np.zeros((6, c0.d_model), F32)}), "exact")
    m0 = model(c0, sd0, "exact")
    ids = clips(1, c0, 9)
    x = ids.view(1, c0.T, 16, 16)
    good = dev(np.zeros((1, c0.T, AD), F32))
    good_ids = dev(np.zeros((1, c0.T), np.int64))
    with pytest.raises(ValueError):
        mv.compute_logits(x)                                                  # missing
    with pytest.raises(ValueError):
        mv.compute_logits(x, action_ids=good_ids, action_vectors=good)       # both kinds
    with pytest.raises(ValueError):
        mi.compute_logits(x, action_ids=good_ids, action_vectors=good)
    with pytest.raises(ValueError):
        mv.compute_logits(x, action_ids=good_ids)                             # ids to a vector model
    with pytest.raises(ValueError):
        mi.compute_logits(x, action_vectors=good)                             # vectors to an id model
    with pytest.raises(ValueError):
        m0.compute_logits(x, action_vectors=good)                             # ... and to an unconditioned one
    with pytest.raises(RuntimeError):
        mv.compute_logits(x, action_vectors=good[:, :, :4])                   # wrong last dimension
    with pytest.raises(RuntimeError):
        mv.compute_logits(x, action_vectors=good[:, :5])
    with pytest.raises(RuntimeError):
        mv.compute_logits(x, action_vectors=good_ids[..., None].expand(1, c0.T, AD))   # not floating point
    bad = good.clone()
    bad[0, 3, 1] = float("nan")
    p = x.clone()
    p[:, 3:] = c0.image_vocab_size
    before = p.clone()
    with pytest.raises(ValueError):
        mv.maskgit_generate(p, 3, action_vectors=bad)                         # a non-finite entry
    bad[0, 3, 1] = float("inf")
    with pytest.raises(ValueError):
        mv.maskgit_generate(p, 3, action_vectors=bad)
    assert torch.equal(p, before)   # the in-place prompt was never touched
    G = pkg("generate")
    with pytest.raises(ValueError):
        G.generate_frames_cached(mv, x, num_prompt_frames=8)
    with pytest.raises(ValueError):
        G.rollout_frames(mv, x[:, :4], 3)
    with pytest.raises(RuntimeError):
        G.rollout_frames(mv, x[:, :4], 3, action_vectors=good[:, :6])        # needs P + n_new = 7 frames
    with pytest.raises(ValueError):
        evaluator(mv).evaluate_metric_sums_reuse(ids.reshape(1, -1))
    with pytest.raises(ValueError):
        evaluator(mv).evaluate_metric_sums(ids.reshape(1, -1), action_vectors=bad)
    _, _, tcv = train_cfgs(1)
    tr = trainer(tcv, pkg("synthetic").make_state_dict(tcv, seed=52), "exact")
    batch = TO.maskgit_collate(pkg("synthetic").make_clips(1, tcv, seed=53), tcv, TO.NumpyDraws(54))
    g0 = tr.grads.clone()
    with pytest.raises(ValueError):
        tr.train_step({k: dev(v) for k, v in batch.items()})
    with pytest.raises(RuntimeError):
        tr.forward_backward(dev(batch["input_ids"]), dev(batch["labels"]), action_vectors=dev(np.zeros((1, 4, AD + 1), F32)))
    assert torch.equal(g0, tr.grads)
