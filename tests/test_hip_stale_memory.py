"""GPU (-m gpu): inference gives the same bits whatever the memory it works in held before the call.

Every inference entry point works in memory its caller takes from torch.empty: the model workspace, the prefix / rollout / fan-out
caches, the packed 16-bit weight streams, the MAGVIT2 scratch, every output.  A fresh process reads zeros there, so a kernel that masks
a cache slot by p = 0 times its value row, pads a ragged tile from unwritten rows, or leaves a corner of an output unwritten passes every
other test of this suite and fails on the first recycled block.  Here each call runs

    twice clean (every such byte 0x00)     -> bit-identical: the determinism the rest stands on
    once under 0xFF, once under 0x3C       -> torch.equal to the clean run, in every output
    (tests/stale_memory.py: NaN in every float type / small finite values that survive fmaxf, comparisons and flags)

and every output is written in full: floats finite, tokens in [0, image_vocab_size) -- index outputs are pre-filled with the mask id,
which no finished output may hold.  Two scopes, so that a failure names its side: *build* (the model is constructed and its weight table
packed under poison: the w16 planes and the temporal_fused / spatial_fused / mlp_fused / frame_stream streams) and *call* (a model built
clean; its cached workspace, any cached cache and everything the call allocates are poisoned).  "Re-use" runs the production case: one
object across calls of other batch sizes, paths and precisions, each call bit-equal to the same call on a freshly built object.

The only outputs with a tolerance are scalars the library sums with atomicAdd on doubles, whose order is free:
    out.loss of STMaskGIT.forward and the loss of GenieTrainer.forward_backward  (the CE sum of kernels_loss.hip; sums[0] / sums[2])
at 1e-9 relative -- a reordering moves a sum of N <= 2^20 addends by at most N * 2^-53 * sum|a_i| ~ 1.2e-10 of it.  The accuracy sums
(counts, exact in a double in any order) and everything else are compared with torch.equal.

Integer regions inside the byte workspaces cannot be given an in-range sentinel, so they were read first (csrc/generate_api.hip
carve_loop / carve_guided_prompt, csrc/api.hip carve; csrc/st_block.hip carves no integers).  Each is written before it is read:
    GenScratch.idsP      context token ids (NBctx, P, S)   put_frame_ids (generate_cached, fan-out prologue) / rollout_window_kernel, all
                         `copies`, before run_context reads them; a context of one frame is read from the caller's frames through fin
    GenScratch.two       the two-frame commit pass          both frames put by commit_slot (final tokens, all-mask) before run_pass
    GenScratch.cur       the frame being decoded            put_frame_ids(fill = mask id) at the top of every slot, all copies; the guided
                         loop mirrors rows [0, B) into [B, 2B) after every step
    GenScratch.fin       the one-frame commit pass          put by commit_slot / run_context before the pass
    GenScratch.samples   sampled ids                        written by the sample launch of the step before the mask step reads them
    GenScratch.unmasked  bytes, one per token               hipMemsetAsync at the top of every slot
    GenScratch.acts      (NB, T) action ids                 guided_actions_kernel / rollout_window_kernel (every window) /
    GenScratch.acts_ctx  (NBctx, T)                         fanout_actions_kernel (both tables in one launch); only with actions
    GuidedPrompt.prompt2, .acts                             put_frame_ids(copies = 2) / guided_actions_kernel before the first forward
    Workspace.samples    sampled ids (maskgit_generate)     sample launch before the mask step and the copy-out
    Workspace.unmasked   bytes                              hipMemsetAsync before the first step
Counters and flags the CALLER must zero are not scratch: status_flag, the `sums` of genie_readout_ce / genie_factored_ce /
genie_metric_hits, `unmasked` of genie_mask_step (include/genie_hip.h, "Memory the caller provides").

Geometries: the smallest that reaches each dispatch branch, two layers, conditioned synthetic weights:
    gen     d 64, 2 heads, T 8, S 16                generic kernels
    gen32   d 64, 4 heads of 16, T 32, S 16, qk     generic T > 16 temporal path
    s256    d 128, 2 heads, T 16, S 256             attn_spatial_dma, the split kernels, the MFMA temporal kernels, the fragment-order passes
    s256qk  d 64, 2 heads of 32, T 16, S 256, qk    the same with qk-norm
    fused   d 256, 8 heads of 32, T 16, S 256       the fused sub-block kernels: bf16 at B = 8 (all three), 2 (temporal + MLP), 1 (none);
                                                    f16x3 at B = 3; launches asserted by kernel name"""
import ast
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, pkg
from stale_memory import PATTERNS, poison_tensor, poisoned

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PRECISIONS = ["exact", "f16x3", "bf16"]
STEPS = 2
REL = 1e-9   # the atomically summed scalars (module docstring); nothing else has a tolerance

GEOMETRY = {   # tag: (d_model, heads, T, S, qk_norm)
    "gen": (64, 2, 8, 16, False),
    "gen32": (64, 4, 32, 16, True),
    "s256": (128, 2, 16, 256, False),
    "s256qk": (64, 2, 16, 256, True),
    "fused": (256, 8, 16, 256, False),
}


# ------------------------------------------------------------------ cases, computed once and never written to
@functools.lru_cache(maxsize=None)
def case(tag, A=0):
    d, H, T, S, qk = GEOMETRY[tag]
    cfg = pkg("config").GenieConfig(num_layers=2, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk, use_mup=False,
                                    action_vocab_size=A)
    sd = pkg("synthetic").make_state_dict(cfg, seed=300 + d + H, law="conditioned")
    if A:
        sd["action_embed.weight"] = (0.5 * np.random.default_rng(9).standard_normal(sd["action_embed.weight"].shape)).astype(np.float32)
    return cfg, sd


def build(tag, precision, A=0):
    cfg, sd = case(tag, A)
    return pkg("st_mask_git").STMaskGIT(cfg, precision=precision).load_numpy_state_dict(sd).to("cuda")


@functools.lru_cache(maxsize=None)
def shared_model(tag, precision, A=0):
    """One model per case for the call-scope tests: its workspace is re-used (and poisoned) from test to test."""
    m = build(tag, precision, A)
    m._weights()
    return m


@functools.lru_cache(maxsize=None)
def clips(tag, B, seed=0):
    """(B, T, h, w) int64 device clips; callers clone before a call that writes into them."""
    cfg, _ = case(tag)
    side = math.isqrt(cfg.S)
    return torch.from_numpy(pkg("synthetic").make_clips(B, cfg, seed=500 + seed + B)).cuda().view(B, cfg.T, side, side)


@functools.lru_cache(maxsize=None)
def masked_clips(tag, B):
    """The clips with the second half of the frames all-mask and a third of frame 1 masked: (input ids, labels), both (B, T * S)."""
    cfg, _ = case(tag)
    lab = clips(tag, B).reshape(B, cfg.T, cfg.S)
    x = lab.clone()
    x[:, cfg.T // 2:] = cfg.image_vocab_size
    x[:, 1, ::3] = cfg.image_vocab_size
    return x.reshape(B, -1), lab.reshape(B, -1).clone()


def draws(cfg, n, rows, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(n, STEPS - 1, rows, cfg.S, generator=g).cuda()
    uni = torch.rand(n, STEPS, cfg.num_factored_vocabs, rows, cfg.S, generator=g).cuda()
    return noise, uni


def actions(B, n, A, seed=7):
    return torch.randint(0, A - 1, (B, n), generator=torch.Generator().manual_seed(seed)).cuda()


# ------------------------------------------------------------------ the comparison
def written(out, cfg, what):
    """Every output was written in full: floats finite, ids in [0, image_vocab_size)."""
    for k, v in out.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"{what}: {k} holds {int((~torch.isfinite(v)).sum())} non-finite values of {v.numel()}"
        else:
            bad = int(((v < 0) | (v >= cfg.image_vocab_size)).sum())
            assert bad == 0, f"{what}: {k} holds {bad} ids of {v.numel()} outside [0, {cfg.image_vocab_size})"


def same(ref, got, what, bars=()):
    assert ref.keys() == got.keys()
    for k, a in ref.items():
        b = got[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        if k in bars:
            a, b = float(a), float(b)
            assert a == b or abs(a - b) <= REL * abs(a), f"{what}: {k} {a!r} vs {b!r}"
        else:
            assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} values"


def snapshot(out):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


def stale_check(run, cfg, what, bars=()):
    """run(byte) -> {name: tensor}: twice clean, then once per poison; see the module docstring."""
    ref = run(0x00)
    written(ref, cfg, what + " (clean)")
    same(ref, run(0x00), what + ": two clean runs differ (not deterministic: nothing can be said about stale memory)", bars)
    for byte in PATTERNS:
        got = run(byte)
        written(got, cfg, f"{what} under {byte:#04x}")
        same(ref, got, f"{what} under {byte:#04x}", bars)


def call_scope(m, fn, owned=lambda: ()):
    """run(byte) for a model built clean: its cached workspace and the buffers owned() names are poisoned, then fn() runs under poison."""
    def run(byte):
        for t in (m._ws, *owned()):
            poison_tensor(t, byte)
        with poisoned(byte, sentinel=m.mask_token_id):
            out = fn()
        return snapshot(out)
    return run


def launched(fn):
    """fn() with the fused-kernel profile on -> (result, {kernel name: launches})."""
    L = pkg("_lib")
    lib = L.load()
    L.check(lib.genie_profile_enable(1 << L.KC_FUSED), "profile_enable")
    lib.genie_profile_reset()
    out = fn()
    kbuf = ctypes.create_string_buffer(4096)
    L.check(lib.genie_profile_kernels(L.KC_FUSED, kbuf, len(kbuf)), "profile_kernels")
    lib.genie_profile_enable(0)
    return out, {ln.split("\t")[0].split(" ")[0]: int(float(ln.split("\t")[1])) for ln in kbuf.value.decode().splitlines()}


def assert_forward_launches(m, x, precision, B):
    """The fused case is only a case if the fused kernels ran (a silent fall-back would make it vacuous)."""
    L = m.config.num_layers
    _, n = launched(lambda: m.hidden_states(x).sum().item())
    mlp = sum(v for k, v in n.items() if k.startswith("mlp_fused_bf16_kernel"))
    got = (n.get("spatial_attn_proj_bf16_kernel", 0), n.get("temporal_fused_bf16_kernel", 0), mlp, n.get("temporal_qkv_attn_f16x3_kernel<0>", 0))
    want = {("bf16", 8): (L, L, L, 0), ("bf16", 2): (0, L, L, 0), ("bf16", 1): (0, 0, 0, 0), ("f16x3", 3): (0, 0, 0, L)}.get((precision, B), (0, 0, 0, 0))
    assert got == want, (precision, B, n)


# ------------------------------------------------------------------ hidden_states, compute_logits, forward
FORWARD = [(tag, p, 2 if tag == "gen32" else 3) for tag in ("gen", "gen32", "s256", "s256qk") for p in PRECISIONS]
FORWARD += [("fused", "bf16", 8), ("fused", "bf16", 2), ("fused", "bf16", 1), ("fused", "f16x3", 3), ("fused", "exact", 2)]


def forward_outputs(m, tag, B):
    cfg = m.config
    x, lab = masked_clips(tag, B)
    side = math.isqrt(cfg.S)
    hidden = m.hidden_states(x.view(B, cfg.T, side, side)).clone()     # (a view of the workspace)
    last = m.compute_logits_frames(x.view(B, cfg.T, side, side), cfg.T - 2, cfg.T, "token")
    out = m(x, lab)
    return dict(hidden=hidden, last_frames=last, logits=out.logits, loss=out.loss, acc=out.acc)


@pytest.mark.parametrize("tag,precision,B", FORWARD)
def test_forward_call_scope(tag, precision, B):
    m = shared_model(tag, precision)
    if tag == "fused":
        side = math.isqrt(m.config.S)
        assert_forward_launches(m, masked_clips(tag, B)[0].view(B, m.config.T, side, side), precision, B)
    stale_check(call_scope(m, lambda: forward_outputs(m, tag, B)), m.config, f"forward/{tag}/{precision}/B{B}", bars=("loss",))


BUILD = [(tag, p, 8 if (tag, p) == ("fused", "bf16") else 3 if tag != "gen32" else 2) for tag in GEOMETRY for p in ("f16x3", "bf16")]


@pytest.mark.parametrize("tag,precision,B", BUILD)
def test_forward_build_scope(tag, precision, B):
    """The model and its packed 16-bit streams are made under poison; the calls then run clean.  On S = 256 a short cached generate
    follows the forward: the frame_stream copies (f16x3) are read by the one-frame passes only."""
    cfg, _ = case(tag)
    P = cfg.T - 2
    noise, uni = draws(cfg, 2, B, seed=21)

    def run(byte):
        with poisoned(byte, sentinel=cfg.image_vocab_size):
            m = build(tag, precision)
            m._weights()
        out = forward_outputs(m, tag, B)
        if cfg.S == 256:
            prompt = clips(tag, B)[:, :P].reshape(B, P * cfg.S)
            tokens, lg0 = m.generate(prompt, max_new_tokens=2 * cfg.S, return_logits=True, maskgit_steps=STEPS, temperature=1.0, noise=noise,
                                     uniforms=uni)
            out.update(gen_tokens=tokens, gen_logits0=lg0)
        return snapshot(out)

    stale_check(run, cfg, f"build/{tag}/{precision}/B{B}", bars=("loss",))


# ------------------------------------------------------------------ maskgit_generate
@pytest.mark.parametrize("variant", ["random", "confidence", "top_k_top_p"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["gen", "s256"])
def test_maskgit_generate(tag, precision, variant):
    m = shared_model(tag, precision)
    cfg = m.config
    B, out_t = (3, 5) if tag == "gen" else (2, 9)
    noise, uni = draws(cfg, 1, B, seed=31)
    law = pkg("sampling").SamplingConfig(0.7, 8, 0.9) if variant != "random" else None
    base = clips(tag, B).clone()
    base[:, out_t:] = cfg.image_vocab_size

    def fn():
        prompt = base.clone()
        samples, lg0 = m.maskgit_generate(prompt, out_t, maskgit_steps=STEPS, temperature=1.0, noise=noise[0], uniforms=uni[0],
                                          unmask_mode="confidence" if variant == "confidence" else "random", sampling=law)
        return dict(samples=samples, logits0=lg0.contiguous(), frame=prompt[:, out_t])

    stale_check(call_scope(m, fn), cfg, f"maskgit_generate/{tag}/{precision}/{variant}")


# ------------------------------------------------------------------ the evaluator's prefix cache
def evaluator(m, steps=STEPS):
    side = math.isqrt(m.config.S)
    return pkg("evaluate").GenieEvaluator(SimpleNamespace(maskgit_steps=steps, temperature=0, latent_h=side, latent_w=side), None, "cuda", model=m)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["gen", "s256", "fused"])
def test_evaluator_prefix_reuse(tag, precision):
    """predict_zframe_logits_reuse: the clean pass over frames 0 .. T - 2, then two masked passes over the cache it left."""
    m = shared_model(tag, precision)
    cfg = m.config
    B = 3
    ev = evaluator(m)
    ids = clips(tag, B).reshape(B, -1)
    noise = torch.rand(cfg.T - 1, STEPS - 1, B, cfg.S, generator=torch.Generator().manual_seed(41)).cuda()

    def fn():
        samples, fl = ev.predict_zframe_logits_reuse(ids, noise=noise)
        return dict(samples=samples, logits=fl.contiguous())

    if tag == "fused" and precision != "exact":
        _, n = launched(lambda: fn()["samples"].sum().item())
        name = "temporal_prefix_fused_bf16_kernel" if precision == "bf16" else "temporal_qkv_attn_f16x3_kernel"
        assert n.get(name + "<1>", 0) == cfg.num_layers and n.get(name + "<2>", 0) == STEPS * cfg.num_layers, n
    stale_check(call_scope(m, fn, owned=lambda: (getattr(ev, "_cache", None),)), cfg, f"evaluator/{tag}/{precision}")


PREFIX = {"gen": [(5, 1), (4, 0)], "s256": [(12, 1), (9, 0)], "fused": [(12, 1), (9, 0), (11, 0)]}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", list(PREFIX))
def test_prefix_passes_on_a_poisoned_cache(tag, precision):
    """genie_clean_pass over n < T - 1 frames (phantom frame slots in the kernels' fixed tiles), then genie_masked_frames_logits with
    frame0 = 1 and 0 (slot i sees the cached frames < i only), through the C ABI on a cache and logits the test owns."""
    L = pkg("_lib")
    lib = L.load()
    m = shared_model(tag, precision)
    cfg = m.config
    c, w = m._weights()[:2]
    B, S, V = 3, cfg.S, cfg.factored_vocab_size * cfg.num_factored_vocabs
    ids = clips(tag, B, seed=1).reshape(B, cfg.T, S)
    nbytes = lib.genie_prefix_cache_bytes(c, B)
    hide = torch.rand(B, cfg.T, S, generator=torch.Generator().manual_seed(5)).cuda() < 0.6
    for n, frame0 in PREFIX[tag]:
        ctx = ids[:, :n].contiguous()
        masked = torch.where(hide, cfg.image_vocab_size, ids)[:, frame0:frame0 + n].contiguous()

        def run(byte):
            poison_tensor(m._ws, byte)
            with poisoned(byte, sentinel=cfg.image_vocab_size):
                ws = m._workspace(B)
                cache = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                logits = torch.empty(B, n, S, V, dtype=torch.float32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            L.check(lib.genie_clean_pass(c, w, ctx.data_ptr(), B, n, n, cache.data_ptr(), nbytes, ws.data_ptr(), ws.numel(), st), "clean")
            L.check(lib.genie_masked_frames_logits(c, w, masked.data_ptr(), B, frame0, n, cache.data_ptr(), nbytes, logits.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), st), "masked")
            return snapshot(dict(logits=logits))

        stale_check(run, cfg, f"prefix passes/{tag}/{precision}/n{n}/frame0={frame0}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["gen", "s256"])
def test_frame_passes_on_a_poisoned_cache(tag, precision):
    """genie_frame_pass / genie_frames_pass through the C ABI: the decode at t = 1 attends one written slot of the kernels' 16-slot tiles,
    the decode at t = T - 1 all of them; the two-frame pass (fragment-order kernels) attends the slot it writes."""
    L = pkg("_lib")
    lib = L.load()
    m = shared_model(tag, precision)
    cfg = m.config
    c, w = m._weights()[:2]
    B, T, S, V = 2, cfg.T, cfg.S, cfg.factored_vocab_size * cfg.num_factored_vocabs
    ids = clips(tag, B, seed=2).reshape(B, T, S).clone()
    ids[:, 1, ::3] = cfg.image_vocab_size
    ids[:, T - 1] = cfg.image_vocab_size
    nbytes = lib.genie_prefix_cache_bytes(c, B)
    two = ids[:, 2:4].contiguous()

    def run(byte):
        poison_tensor(m._ws, byte)
        with poisoned(byte, sentinel=cfg.image_vocab_size):
            ws = m._workspace(B)
            cache = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            lg = {k: torch.empty(B, S, V, dtype=torch.float32, device="cuda") for k in ("t1", "two", "last")}
        st = torch.cuda.current_stream().cuda_stream

        def one(t, logits=None):
            L.check(lib.genie_frame_pass(c, w, ids[:, t].contiguous().data_ptr(), B, t, cache.data_ptr(), nbytes,
                                         0 if logits is None else logits.data_ptr(), ws.data_ptr(), ws.numel(), st), "genie_frame_pass")

        one(0)
        one(1, lg["t1"])
        rc = lib.genie_frames_pass(c, w, two.data_ptr(), B, 2, 2, cache.data_ptr(), nbytes, lg["two"].data_ptr(), ws.data_ptr(), ws.numel(), st)
        if rc == L.E_UNSUPPORTED:   # (one frame per pass outside the fragment-order kernels)
            one(2)
            one(3, lg["two"])
        else:
            L.check(rc, "genie_frames_pass")
        for t in range(4, T - 1):
            one(t)
        one(T - 1, lg["last"])
        return snapshot(lg)

    stale_check(run, cfg, f"frame passes/{tag}/{precision}")


# ------------------------------------------------------------------ cached generate
@pytest.mark.parametrize("variant", ["plain", "actions", "guided"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["gen", "s256"])
def test_generate_cached(tag, precision, variant):
    """generate() on the temporal KV cache (genie_generate_cached): P = 8 of T = 16 on s256, P = 2 of 8 on gen; under guidance every pass
    runs 2 B clips.  The cache is allocated by the call, under poison."""
    A = 0 if variant == "plain" else 5
    m = shared_model(tag, precision, A)
    cfg = m.config
    B, P = 2, (8 if tag == "s256" else 2)
    n_new = cfg.T - P
    noise, uni = draws(cfg, n_new, B, seed=51)
    prompt = clips(tag, B)[:, :P].reshape(B, P * cfg.S)
    kw = dict(action_ids=actions(B, cfg.T, A)) if A else {}
    if variant == "guided":
        kw["guidance"] = pkg("sampling").Guidance(3.0, A - 1)

    def fn():
        tokens, lg0 = m.generate(prompt, max_new_tokens=n_new * cfg.S, return_logits=True, maskgit_steps=STEPS, temperature=1.0, noise=noise,
                                 uniforms=uni, **kw)
        return dict(tokens=tokens, logits0=lg0.contiguous())

    stale_check(call_scope(m, fn), cfg, f"generate/{tag}/{precision}/{variant}")


# ------------------------------------------------------------------ the rollout past the window
def poison_unowned_slots(r, byte):
    """Between two calls of a Rollout the cache slots from the pending frame's on belong to nobody (the next call commits the pending frame
    first); when the next frame opens a window the whole cache does.  The 16-bit cache of bf16 keeps its slots in the first half of each
    layer's slice."""
    m, cache = r.model, r._cache
    c = m.config
    _, start, slot = r.window
    NB = cache.numel() // (c.num_layers * c.T * c.S * 3 * c.d_model * 4)
    if r.n == r.P or (r.n >= c.T and slot == r.keep):
        poison_tensor(cache, byte)
        return
    if m.precision == "bf16" and c.T <= 16 and c.d_model // c.num_heads in (32, 64):
        v = cache.view(c.num_layers, 2, NB, c.T, -1)[:, 0]
    else:
        v = cache.view(c.num_layers, NB, c.T, -1)
    v[:, :, slot - 1:] = byte


@pytest.mark.parametrize("tag,precision", [("s256", "f16x3"), ("s256", "bf16"), ("gen", "exact")])
def test_rollout_recycles_poisoned_slots(tag, precision):
    """A Rollout with keep < P, far enough past the window that every cache slot is recycled twice (three windows), split into an extend,
    a step and an extend; between the calls the slots the object does not own are poisoned again."""
    G = pkg("generate")
    m = shared_model(tag, precision)
    cfg = m.config
    B = 2
    P, keep, N, first = (14, 13, 7, 3) if tag == "s256" else (3, 2, 15, 7)
    assert len(G.window_schedule(P, keep, cfg.T, N)) == 3
    noise, uni = draws(cfg, N, B, seed=61)
    prompt = clips(tag, B)[:, :P]
    kw = dict(unmask_mode="confidence", sampling=pkg("sampling").SamplingConfig(0.7, 8, 0.9))

    def run(byte):
        poison_tensor(m._ws, byte)
        with poisoned(byte, sentinel=cfg.image_vocab_size):
            r = G.Rollout(m, prompt, keep=keep, maskgit_steps=STEPS, temperature=1.0, **kw)
            r.extend(first, noise=noise[:first], uniforms=uni[:first])
            poison_unowned_slots(r, byte)
            poison_tensor(m._ws, byte)
            r.step(noise=noise[first], uniforms=uni[first])
            poison_unowned_slots(r, byte)
            poison_tensor(m._ws, byte)
            r.extend(N - first - 1, noise=noise[first + 1:], uniforms=uni[first + 1:])
        return snapshot(dict(frames=r.frames))

    stale_check(run, cfg, f"rollout/{tag}/{precision}")


# ------------------------------------------------------------------ fan-out and scoring
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["gen", "s256"])
def test_fanout_and_score(tag, precision):
    """genie_generate_fanout and genie_score_fanout, K = 3 branches of B = 2 clips, on a trunk and a branch cache the test owns (the
    decode passes read fixed tiles of trunk slots [0, P) and of the branch's own slots); the workspace is the call's, under poison."""
    G, L = pkg("generate"), pkg("_lib")
    lib = L.load()
    m = shared_model(tag, precision)
    cfg = m.config
    c = m._weights()[0]
    B, K, n = 2, 3, 2
    P = 8 if tag == "s256" else 3
    clip = clips(tag, B, seed=3)[:, :P + n].reshape(B, P + n, cfg.S).contiguous()
    prompt = clip[:, :P].contiguous()
    noise, uni = draws(cfg, n, B * K, seed=71)
    dec = G._Decode(m, STEPS, 1.0, "random", None, None, True)

    def run(byte):
        with poisoned(byte, sentinel=cfg.image_vocab_size):
            out = {}
            for what in ("fanout", "score"):
                trunk = torch.empty(lib.genie_prefix_cache_bytes(c, B), dtype=torch.uint8, device="cuda")
                branch = torch.empty(lib.genie_fanout_branch_bytes(c, B, K, n), dtype=torch.uint8, device="cuda")
                if what == "fanout":
                    out["tokens"] = G.fanout_call(m, prompt, K, n, None, dec, noise, uni, trunk=trunk, branch=branch)
                else:
                    out["nll"], out["hits"], out["token_nll"] = G.score_call(m, clip, P, K, None, per_token=True, trunk=trunk, branch=branch)
        return snapshot(out)

    stale_check(run, cfg, f"fanout+score/{tag}/{precision}")


# ------------------------------------------------------------------ MAGVIT2
def test_magvit_tokenizer_ends_at_the_small_fixture():
    """The tokenizer ends on the magvit_small fixture under poisoned torch.empty: bits <- tokens, tokens <- bits, u8 <- floats (their
    outputs come from torch.empty in magvit2.py).  The conv stack refuses this fixture's 32/64-wide config (test_hip_harness.py::
    test_single_backend), so the encode -> decode chain runs on magvit_mid below."""
    mv = pkg("magvit2")
    z = np.load(f"{GOLDEN}/magvit_small.npz")
    ids, bits = torch.from_numpy(z["bits_ids"]).cuda(), torch.from_numpy(z["bits_z"]).cuda()
    y = torch.from_numpy(z["dec_out_f32"]).cuda()
    y16 = torch.from_numpy(z["dec_out_bf16_as_f32"]).cuda().to(torch.bfloat16)
    for byte in (0x00,) + PATTERNS:
        with poisoned(byte, sentinel=1 << 18):
            got = (mv.bits_from_tokens(ids), mv.tokens_from_bits(bits), mv.rescale_magvit_output(y), mv.rescale_magvit_output(y16))
        torch.cuda.synchronize()
        for g, want in zip(got, ("bits_z", "bits_ids", "dec_u8_f32", "dec_u8_bf16")):
            assert np.array_equal(g.cpu().numpy(), z[want]), (hex(byte), want)
        small = mv.VQModel(mv.VQConfig(**ast.literal_eval(str(z["cfg"])))).to("cuda")
        with poisoned(byte), pytest.raises(ValueError, match="multiples of 64"):
            small.decode_tokens(torch.from_numpy(z["dec_tokens"]).cuda())


def test_magvit_encode_decode_chain():
    """frames -> HipEncoder.encode_tokens -> tokens -> HipDecoder.decode_tokens -> frames on the smallest fixture the conv stack covers
    (magvit_mid): the packed weights, the NHWC activations, the GroupNorm statistics and partials, the token and byte outputs all come
    from torch.empty in magvit2.py.  Build + call under poison, then the call alone."""
    mv = pkg("magvit2")
    z = np.load(f"{GOLDEN}/magvit_mid.npz")
    vq = mv.VQModel(mv.VQConfig(**ast.literal_eval(str(z["cfg"]))))
    vq.load_state_dict({k: torch.from_numpy(v) for k, v in mv.make_vq_state_dict(vq, int(z["weight_seed"])).items()})
    vq = vq.to("cuda")
    frames = torch.from_numpy(z["enc_frames"]).cuda()
    vocab = SimpleNamespace(image_vocab_size=1 << 18)
    kept = {}

    def run(byte, rebuild):
        with poisoned(byte, sentinel=1 << 18):
            if rebuild or not kept:
                kept["enc"], kept["dec"] = mv.HipEncoder(vq.encoder), mv.HipDecoder(vq.decoder)
            tokens = kept["enc"].encode_tokens(frames)
            pixels = kept["dec"].decode_tokens(tokens)
            floats = kept["dec"].decode_tokens(tokens, return_float=True)
        return snapshot(dict(tokens=tokens, pixels=pixels.to(torch.int64), floats=floats.float()))

    stale_check(lambda byte: run(byte, True), vocab, "magvit chain, build + call")
    stale_check(lambda byte: run(byte, False), vocab, "magvit chain, call")


# ------------------------------------------------------------------ re-use across calls: plausible leftovers, not a byte pattern
def logits_of(m, tag, B):
    return m.compute_logits(clips(tag, B, seed=4))


def generate_of(m, tag, B):
    cfg = m.config
    P, n_new = 8, 3
    noise, uni = draws(cfg, n_new, B, seed=81)
    return m.generate(clips(tag, B, seed=5)[:, :P].reshape(B, P * cfg.S), max_new_tokens=n_new * cfg.S, maskgit_steps=STEPS, temperature=1.0,
                      noise=noise, uniforms=uni)


def rollout_of(m, tag, B):
    cfg = m.config
    P, keep, N = 14, 13, 7   # windows of 2, 3 and 2 frames
    noise, uni = draws(cfg, N, B, seed=82)
    return m.rollout(clips(tag, B, seed=6)[:, :P], N, keep=keep, maskgit_steps=STEPS, temperature=1.0, noise=noise, uniforms=uni)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag,Bs", [("s256", (3, 2, 3)), ("fused", (8, 1, 8))])
def test_one_model_across_calls(tag, Bs, precision):
    """compute_logits at B0, a cached generate, a rollout past the window, compute_logits at B1 and at B0 again on ONE model: each call
    bit-equal to the same call on a model built for it (whose workspace no other call has used)."""
    m = build(tag, precision)
    cfg = m.config
    seq = [("logits", logits_of, Bs[0]), ("generate", generate_of, Bs[0]), ("rollout", rollout_of, 2), ("logits", logits_of, Bs[1]),
           ("logits", logits_of, Bs[0])]
    for i, (name, call, B) in enumerate(seq):
        got = snapshot(dict(out=call(m, tag, B)))
        want = snapshot(dict(out=call(build(tag, precision), tag, B)))
        written(got, cfg, f"call {i} ({name}, B = {B})")
        same(want, got, f"re-use/{tag}/{precision}: call {i} ({name}, B = {B}) on the re-used model vs a fresh one")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag,Bs", [("s256", (3, 2, 3)), ("fused", (8, 1, 8))])
def test_one_evaluator_across_batch_sizes(tag, Bs, precision):
    ev = evaluator(build(tag, precision))
    cfg = ev.model.config
    for i, B in enumerate(Bs):
        ids = clips(tag, B, seed=7).reshape(B, -1)
        noise = torch.rand(cfg.T - 1, STEPS - 1, B, cfg.S, generator=torch.Generator().manual_seed(91)).cuda()
        outs = []
        for e in (ev, evaluator(build(tag, precision))):
            samples, fl = e.predict_zframe_logits_reuse(ids, noise=noise)
            outs.append(snapshot(dict(samples=samples, logits=fl.contiguous())))
        written(outs[0], cfg, f"call {i} (B = {B})")
        same(outs[1], outs[0], f"evaluator re-use/{tag}/{precision}: call {i} (B = {B}) vs a fresh evaluator")


@pytest.mark.parametrize("tag,B", [("s256", 3), ("fused", 8)])
def test_set_precision_keeps_the_workspace(tag, B):
    """exact -> bf16 -> f16x3 on one model: the workspace still holds the previous precision's bytes."""
    m = build(tag, "exact")
    for precision in ("exact", "bf16", "f16x3"):
        m.set_precision(precision)
        got = snapshot(dict(logits=logits_of(m, tag, B), hidden=m.hidden_states(clips(tag, B, seed=4))))
        f = build(tag, precision)
        want = snapshot(dict(logits=logits_of(f, tag, B), hidden=f.hidden_states(clips(tag, B, seed=4))))
        written(got, m.config, f"{tag}/{precision}")
        same(want, got, f"set_precision/{tag}: {precision} after the precisions before it vs a fresh {precision} model")


# ------------------------------------------------------------------ training: exact and f16x3 (bf16: test_hip_train_recompute / _dropout)
@pytest.mark.parametrize("precision,name", [("f16x3", "d64"), ("f16x3", "d256qk"), ("exact", "d64")])
def test_training_step_on_stale_buffers(precision, name):
    """The activation buffer and the workspace of GenieTrainer hold 0xFF (then 0x3C) in every byte before the step: the whole flat
    gradient is torch.equal to the clean step's; the loss (the atomically summed CE, module docstring) agrees to 1e-9.  Cases of
    tests/test_hip_train_bf16.py: d64 (64 tokens) and d256qk (transposed-copy path with token slabs in f16x3)."""
    from test_hip_train_bf16 import make_case, make_trainer
    cfg, sd, ids, labels = make_case(name)
    ids, labels = torch.from_numpy(ids).cuda(), torch.from_numpy(labels).cuda()
    B = ids.shape[0]

    def run(byte):
        tr = make_trainer(cfg, sd, precision)
        for buf in tr._buffers(B):
            poison_tensor(buf, byte)
        loss, acc = tr.forward_backward(ids, labels)
        return snapshot(dict(grads=tr.grads, loss=torch.as_tensor(loss), acc=torch.as_tensor(acc)))

    stale_check(run, cfg, f"train/{precision}/{name}", bars=("loss",))
