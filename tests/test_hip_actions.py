"""Per-frame action conditioning on the HIP path (genie_frame_cond, the *_cond entry points).  Pinned without a reference
implementation by one identity: the action row is added to the position row before the token term, so a clip with actions
a_0..a_{T-1} is BIT-IDENTICAL to the unconditioned model whose positional table is pos + table[a_t] (computed in f32), and an
all-zero table is the unconditioned model.  Every entry point that embeds token ids is checked against that fold, the window
passes at t0 > 0 included; the batch against single clips, the CPU oracle on the folded weights, the training step (the
action-table gradient against the positional gradient) and one end-to-end training run.  Needs a GPU: -m gpu."""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg
from oracle import genie_oracle as O
from oracle import genie_train_oracle as TO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECISIONS = ["exact", "f16x3", "bf16"]
A = 6
STEPS = 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def cfgs(A=A, **kw):
    args = dict(num_layers=2, num_heads=2, d_model=128, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    args.update(kw)
    C = pkg("config").GenieConfig
    return C(**args), C(**args, action_vocab_size=A)


def action_table(d, seed=3, zero=False):
    if zero:
        return np.zeros((A, d), np.float32)
    return (0.5 * np.random.default_rng(seed).standard_normal((A, d))).astype(np.float32)


def fold(sd0, table, a):
    """The unconditioned state dict whose positional table carries the actions a (T,): pos + table[a_t] in f32."""
    sd = dict(sd0)
    sd["pos_embed_TSC"] = (sd0["pos_embed_TSC"] + table[np.asarray(a)][None, :, None, :]).astype(np.float32)
    return sd


def model(cfg, sd, precision):
    return pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")


def evaluator(m):
    return pkg("evaluate").GenieEvaluator(SimpleNamespace(maskgit_steps=STEPS, temperature=0.0, latent_h=16, latent_w=16),
                                          None, "cuda", model=m)


def battery(m, ids, act, noise_seed=9):
    """Every inference entry point that embeds token ids, on clips ids (B, T, S) with actions act ((B, T) or None).
    Returns {name: tensor}; the caller compares two runs bit for bit."""
    G = pkg("generate")
    cfg = m.config
    B, T, S = ids.shape
    H = 16
    out = {}
    kw = {} if act is None else {"action_ids": act}
    g = torch.Generator(device="cpu").manual_seed(noise_seed)
    x = ids.view(B, T, H, H)
    out["compute_logits"] = m.compute_logits(x, **kw)
    p = x.clone()
    p[:, 5:] = cfg.image_vocab_size
    noise = torch.rand(STEPS - 1, B, S, generator=g).cuda()
    s, lg = m.maskgit_generate(p, 5, maskgit_steps=STEPS, noise=noise, **kw)
    out["maskgit_samples"], out["maskgit_logits0"], out["maskgit_prompt"] = s, lg, p
    # generate(): KV cache (4 prompt + 3 new frames: the action ids are padded to T) and the full-forward schedule
    nz = torch.rand(4, STEPS - 1, B, S, generator=g).cuda()
    kw7 = {} if act is None else {"action_ids": act[:, :7]}
    out["generate_kv"] = m.generate(ids[:, :4].reshape(B, -1), max_new_tokens=3 * S, maskgit_steps=STEPS, noise=nz[:3],
                                    return_logits=True, kv_cache=True, **kw7)
    out["generate_full"] = m.generate(ids[:, :12].reshape(B, -1), max_new_tokens=4 * S, maskgit_steps=STEPS, noise=nz,
                                      return_logits=True, kv_cache=False, **kw)
    for P in (1, 8, 15):
        nzP = torch.rand(T - P, STEPS - 1, B, S, generator=g).cuda()
        for tf in (False, True):
            for host in (False, True):
                out[f"cached_P{P}_tf{int(tf)}_host{int(host)}"] = G.generate_frames_cached(
                    m, x, num_prompt_frames=P, maskgit_steps=STEPS, teacher_force_time=tf, noise=nzP, host_loop=host, **kw)
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


def clips(B, cfg, seed):
    ids = dev(pkg("synthetic").make_clips(B, cfg, seed=seed)).view(B, cfg.T, cfg.S)
    ids[:, 2, ::5] = cfg.image_vocab_size   # some mask tokens in the context too (the action row is added to them as well)
    return ids


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_table_is_the_unconditioned_model(precision):
    c0, ca = cfgs()
    sd0 = pkg("synthetic").make_state_dict(c0, seed=21)
    m0 = model(c0, sd0, precision)
    ma = model(ca, dict(sd0, **{"action_embed.weight": action_table(c0.d_model, zero=True)}), precision)
    B = 2
    ids = clips(B, c0, 5)
    act = dev(np.random.default_rng(1).integers(0, A, (B, c0.T)))
    assert_bit_identical(battery(ma, ids, act), battery(m0, ids, None))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_actions_fold_into_the_positional_table(precision):
    """B = 1: every entry point with table / actions a == the unconditioned model on pos + table[a] -- the window passes
    (genie_frames_pass at t0 > 0, genie_masked_frames_logits at frame0 = 1, the clean pass) read the action of the ABSOLUTE frame."""
    c0, ca = cfgs()
    sd0 = pkg("synthetic").make_state_dict(c0, seed=22)
    table = action_table(c0.d_model)
    a = np.random.default_rng(2).integers(0, A, c0.T)
    a[:4] = [5, 0, 3, 3]
    ma = model(ca, dict(sd0, **{"action_embed.weight": table}), precision)
    mf = model(c0, fold(sd0, table, a), precision)
    ids = clips(1, c0, 6)
    got = battery(ma, ids, dev(a[None]))
    assert_bit_identical(got, battery(mf, ids, None))
    # and the actions matter
    m0 = model(c0, sd0, precision)
    assert not torch.equal(got["compute_logits"], m0.compute_logits(ids.view(1, c0.T, 16, 16)))


BATCH_TOL = {"exact": 2e-5, "f16x3": 2e-5, "bf16": 8e-2}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_of_clips_with_their_own_actions(precision):
    c0, ca = cfgs()
    sd0 = pkg("synthetic").make_state_dict(c0, seed=23)
    ma = model(ca, dict(sd0, **{"action_embed.weight": action_table(c0.d_model)}), precision)
    B, T, S = 16, c0.T, c0.S
    ids = clips(B, c0, 7)
    act = dev(np.random.default_rng(3).integers(0, A, (B, T)))
    x = ids.view(B, T, 16, 16)
    full = ma.compute_logits(x, action_ids=act)
    tol = BATCH_TOL[precision]
    for b in (0, 7, 15):
        one = ma.compute_logits(x[b:b + 1].contiguous(), action_ids=act[b:b + 1])
        assert float((one - full[b:b + 1]).abs().max()) < tol, b
    # one clip's actions change that clip's logits and no other clip's
    act2 = act.clone()
    act2[3] = (act2[3] + 1) % A
    full2 = ma.compute_logits(x, action_ids=act2)
    for b in range(B):
        assert torch.equal(full[b], full2[b]) == (b != 3), b
    # the window passes at B > 1 read clip b's ids at b * T: generate (prompt pass + one-frame passes) and the evaluator's passes
    B4 = 4
    lg4 = ma.generate(ids[:B4, :8].reshape(B4, -1), max_new_tokens=S, maskgit_steps=1, return_logits=True,
                      action_ids=act[:B4, :9])[1]
    _, r4 = evaluator(ma).predict_zframe_logits_reuse(ids[:B4].reshape(B4, -1), unmask_mode="greedy", action_ids=act[:B4])
    for b in range(B4):
        lg1 = ma.generate(ids[b:b + 1, :8].reshape(1, -1), max_new_tokens=S, maskgit_steps=1, return_logits=True,
                          action_ids=act[b:b + 1, :9])[1]
        assert float((lg1 - lg4[b:b + 1]).abs().max()) < tol, b
        _, r1 = evaluator(ma).predict_zframe_logits_reuse(ids[b:b + 1].reshape(1, -1), unmask_mode="greedy",
                                                          action_ids=act[b:b + 1])
        assert float((r1 - r4[b:b + 1]).abs().max()) < tol, b


@pytest.mark.parametrize("precision", PRECISIONS)
def test_clips_against_the_cpu_oracle_on_the_folded_weights(precision):
    c0, ca = cfgs()
    sd0 = pkg("synthetic").make_state_dict(c0, seed=24)
    table = action_table(c0.d_model, seed=8)
    ma = model(ca, dict(sd0, **{"action_embed.weight": table}), precision)
    B = 2
    ids = clips(B, c0, 8)
    x = ids.view(B, c0.T, 16, 16)
    x[:, 9:] = c0.image_vocab_size
    act = np.random.default_rng(4).integers(0, A, (B, c0.T))
    lg = ma.compute_logits(x, action_ids=dev(act)).cpu().numpy()
    xn = x.cpu().numpy()
    for b in range(B):
        ref = O.compute_logits(xn[b:b + 1], fold(sd0, table, act[b]), c0, O.BF16_MFMA if precision == "bf16" else O.F32)
        err = np.abs(lg[b:b + 1] - ref)
        scale = max(1.0, float(np.abs(ref).max()) / 8)
        if precision == "bf16":   # same rounding points as the oracle's 16-bit contract (test_hip_configs.py's bars)
            assert np.median(err) < 4e-3 and err.max() < 8e-2, (b, np.median(err), err.max())
        else:
            assert err.max() < 5e-5 * scale, (b, err.max())


# ------------------------------------------------------------------ training
def train_cfgs():
    return cfgs(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_prompt_frames=2)


def trainer(cfg, sd, precision):
    return pkg("train").GenieTrainer(model(cfg, sd, precision))


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30))


def dtable_from_dpos(dpos, a):
    """d table[k] = sum over frames t with a_t == k of sum_s d pos[t, s]  (f64)."""
    per_frame = dpos.astype(np.float64).reshape(len(a), -1, dpos.shape[-1]).sum(1)
    out = np.zeros((A, dpos.shape[-1]))
    for t, k in enumerate(a):
        out[k] += per_frame[t]
    return out


@pytest.mark.parametrize("precision", ["exact", "bf16"])
def test_training_step_folds_and_the_table_gradient(precision):
    c0, ca = train_cfgs()
    syn = pkg("synthetic")
    sd0 = syn.make_state_dict(c0, seed=31)
    table = action_table(c0.d_model, seed=9)
    a = np.array([4, 1, 4, 0])       # ids 2, 3, 5 unused
    batch = TO.maskgit_collate(syn.make_clips(1, c0, seed=32), c0, TO.NumpyDraws(33))
    ids, lab = dev(batch["input_ids"]), dev(batch["labels"])
    ta = trainer(ca, dict(sd0, **{"action_embed.weight": table}), precision)
    tf = trainer(c0, fold(sd0, table, a), precision)
    la, _ = ta.forward_backward(ids, lab, action_ids=dev(a[None]))
    lf, _ = tf.forward_backward(ids, lab)
    assert float(la) == float(lf)
    ga, gf = ta.gradients(), tf.gradients()
    assert set(ga) == set(gf) | {"action_embed.weight"}
    for k in gf:
        assert torch.equal(ga[k], gf[k]), k
    dt = ga["action_embed.weight"].cpu().numpy()
    want = dtable_from_dpos(gf["pos_embed_TSC"].cpu().numpy()[0], a)
    assert rel_err(dt, want) < 1e-6
    assert np.all(dt[[2, 3, 5]] == 0)
    # bit-reproducible, and accumulate adds
    g1 = ta.grads.clone()
    ta.forward_backward(ids, lab, action_ids=dev(a[None]))
    assert torch.equal(g1, ta.grads)
    a2 = np.array([2, 2, 3, 5])
    ta.forward_backward(ids, lab, action_ids=dev(a2[None]))
    g2 = ta.grads.clone()
    ta.forward_backward(ids, lab, action_ids=dev(a[None]))
    ta.forward_backward(ids, lab, action_ids=dev(a2[None]), accumulate=True)
    assert float((ta.grads - (g1 + g2)).abs().max()) <= 1e-6 * float(g1.abs().max())


def test_training_batch_vs_the_oracle_on_the_folded_weights():
    c0, ca = train_cfgs()
    syn = pkg("synthetic")
    sd0 = syn.make_state_dict(c0, seed=41)
    table = action_table(c0.d_model, seed=10)
    a = np.array([1, 3, 3, 0])
    B = 4
    batch = TO.maskgit_collate(syn.make_clips(B, c0, seed=42), c0, TO.NumpyDraws(43))
    sdf = fold(sd0, table, a)
    loss_o, _, g_o = TO.forward_backward(batch["input_ids"], batch["labels"], sdf, c0)
    ta = trainer(ca, dict(sd0, **{"action_embed.weight": table}), "exact")
    loss, _ = ta.forward_backward(dev(batch["input_ids"]), dev(batch["labels"]), action_ids=dev(np.tile(a, (B, 1))))
    assert abs(float(loss) - loss_o) < 1e-5 * abs(loss_o)
    g = ta.gradients()
    for k in g_o:
        assert rel_err(g[k].cpu().numpy(), g_o[k]) < 1e-4, k
    assert rel_err(g["action_embed.weight"].cpu().numpy(), dtable_from_dpos(g_o["pos_embed_TSC"][0], a)) < 1e-4


TRAIN_STEPS = 200
CE_RATIO = 0.1   # measured: 0.185 vs 49.6 after 200 steps (ratio 0.004)


def test_training_learns_to_use_the_actions():
    """A tiny model on synthetic clips where every frame is a fixed function of its action: after a fixed number of seeded
    trainer steps the CE of frames 1..T-1 (all masked, frame 0 visible) with the true actions is far below the CE with shuffled
    actions."""
    import random
    D = pkg("data")
    c0, ca = cfgs(A=4, num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_prompt_frames=1)
    torch.manual_seed(0)
    random.seed(0)
    m = pkg("st_mask_git").STMaskGIT(ca).to("cuda")
    m.init_weights()
    tr = pkg("train").GenieTrainer(m, lr=3e-3)
    g = np.random.default_rng(0)
    pattern = g.integers(0, 512, (4, ca.S)) * 513          # frame of action k: one fixed token pattern (both factors equal)

    def make(n):
        act = g.integers(0, 4, (n, ca.T))
        return dev(pattern[act].reshape(n, -1)), dev(act)

    for _ in range(TRAIN_STEPS):
        x, act = make(16)
        tr.train_step(D.maskgit_collate(x, ca, action_ids=act))
    x, act = make(64)
    masked = x.clone()
    masked[:, ca.S:] = ca.image_vocab_size
    shuffled = act[torch.randperm(64, device="cuda")]
    ce_true = float(m(masked, x, action_ids=act).loss)
    ce_shuf = float(m(masked, x, action_ids=shuffled).loss)
    print(f"after {TRAIN_STEPS} steps: masked CE {ce_true:.4f} with the true actions, {ce_shuf:.4f} shuffled")
    assert ce_true < CE_RATIO * ce_shuf, (ce_true, ce_shuf)


def test_input_errors_raise_before_anything_is_enqueued():
    c0, ca = cfgs(num_layers=1)
    sd0 = pkg("synthetic").make_state_dict(c0, seed=51)
    ma = model(ca, dict(sd0, **{"action_embed.weight": action_table(c0.d_model)}), "exact")
    m0 = model(c0, sd0, "exact")
    ids = clips(1, c0, 9)
    x = ids.view(1, c0.T, 16, 16)
    good = dev(np.zeros((1, c0.T), np.int64))
    with pytest.raises(ValueError):
        ma.compute_logits(x)
    with pytest.raises(ValueError):
        m0.compute_logits(x, action_ids=good)
    with pytest.raises(IndexError):
        ma.compute_logits(x, action_ids=good + A)
    with pytest.raises(RuntimeError):
        ma.compute_logits(x, action_ids=good[:, :5])
    p = x.clone()
    p[:, 3:] = c0.image_vocab_size
    before = p.clone()
    with pytest.raises(IndexError):
        ma.maskgit_generate(p, 3, action_ids=good - 1)
    assert torch.equal(p, before)   # the in-place prompt was never touched
    with pytest.raises(ValueError):
        pkg("generate").generate_frames_cached(ma, x, num_prompt_frames=8)
    with pytest.raises(ValueError):
        evaluator(ma).evaluate_metric_sums_reuse(ids.reshape(1, -1))
    tc0, tca = train_cfgs()
    tr = trainer(tca, pkg("synthetic").make_state_dict(tca, seed=52), "exact")
    batch = TO.maskgit_collate(pkg("synthetic").make_clips(1, tca, seed=53), tca, TO.NumpyDraws(54))
    g0 = tr.grads.clone()
    with pytest.raises(ValueError):
        tr.train_step({k: dev(v) for k, v in batch.items()})
    with pytest.raises(IndexError):
        tr.forward_backward(dev(batch["input_ids"]), dev(batch["labels"]), action_ids=dev(np.full((1, 4), A)))
    assert torch.equal(g0, tr.grads)
