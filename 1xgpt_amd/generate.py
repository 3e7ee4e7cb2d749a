"""Prompted generation harness -- counterpart of the reference's genie/generate.py:62-116.

Prompt ``num_prompt_frames`` frames, MaskGIT-decode the remaining ``window_size - num_prompt_frames`` frames
autoregressively (or teacher-forced in time), and write ``[prompt | generated | ground truth]`` as ``video.bin``
+ ``metadata.json`` in the dataset layout.  Batched: the reference generates one example, this takes (B, T, H, W).
The reference's ``--teacher_force_time`` branch reads a non-existent ``model.image_mask_token`` (generate.py:86);
here it uses ``mask_token_id``, which is what that line means.
"""
import json
from pathlib import Path

import numpy as np
import torch

STRIDE = 15


def known_tokens(frames, keep, mask_token_id):
    """The ``known=`` tensor of the generate functions from ``frames`` (..., H, W) and a boolean ``keep`` mask, (H, W) or of the frames' full
    shape: the frame's token where keep is true, ``mask_token_id`` (model.mask_token_id: "generate this one") where it is false."""
    frames = torch.as_tensor(frames).to(torch.int64)
    keep = torch.as_tensor(keep, device=frames.device)
    if keep.dtype != torch.bool:
        raise RuntimeError(f"keep must be a boolean mask, got {keep.dtype}")
    if tuple(keep.shape) not in (tuple(frames.shape), tuple(frames.shape[-2:])):
        raise RuntimeError(f"keep must have shape {tuple(frames.shape[-2:])} or {tuple(frames.shape)}, got {tuple(keep.shape)}")
    return torch.where(keep, frames, torch.full_like(frames, int(mask_token_id))).contiguous()


def check_known(known, shape, device, what="known"):
    """The checked ``known`` tensor of a generate call: int64, on ``device``, exactly ``shape`` -- raised before any launch; returned
    contiguous.  Values are not inspected (that would need a host synchronisation): a value in [0, image_vocab_size) is a known token, any
    other marks a token to generate.  None -> None."""
    if known is None:
        return None
    if not isinstance(known, torch.Tensor):
        raise RuntimeError(f"{what} must be a torch tensor, got {type(known).__name__}")
    if known.dtype != torch.int64:
        raise RuntimeError(f"{what} must be an int64 tensor, got {known.dtype}")
    if tuple(known.shape) != tuple(shape):
        raise RuntimeError(f"expected {what} of shape {tuple(shape)}, got {tuple(known.shape)}")
    if known.device != torch.device(device):
        raise RuntimeError(f"{what} must be on {device}, got {known.device}")
    return known.contiguous()


@torch.no_grad()
def generate_frames(model, example_THW: torch.LongTensor, num_prompt_frames=8, maskgit_steps=2, temperature=0.0,
                    teacher_force_time=False, noise=None, action_ids=None, sampling=None, unmask_mode="random", uniforms=None,
                    guidance=None, action_vectors=None, known=None):
    """example_THW (B, T, H, W) on the model's device -> outputs (B, T + (T - num_prompt_frames), H, W):
    [prompt frames | predicted frames | ground-truth frames] (generate.py:97-103).
    noise: optional (T - num_prompt_frames, maskgit_steps-1, B, S).
    action_ids: (B, T) per-frame actions of an action-conditioned model (config.action_vocab_size > 0).
    sampling: a SamplingConfig (1xgpt_amd/sampling.py) or None = the reference's law; unmask_mode: "random" (the reference's
    harness), "greedy" or "confidence"; uniforms: optional (T - num_prompt_frames, maskgit_steps, num_factored_vocabs, B, S).
    guidance: a Guidance(scale, null_action) or None: classifier-free guidance of an action-conditioned model.
    action_vectors: (B, T, action_dim) float actions of a model with config.action_dim > 0 (then Guidance(scale) suffices).
    known: optional (B, T - num_prompt_frames, H, W) int64 known tokens of the predicted frames (known_tokens; mask_token_id = generate)."""
    window_size = example_THW.shape[1]
    assert num_prompt_frames <= window_size
    example_THW = example_THW.to(torch.int64).contiguous()
    known = check_known(known, (example_THW.shape[0], window_size - num_prompt_frames) + tuple(example_THW.shape[2:]), example_THW.device)
    samples = []
    prompt_THW = example_THW.clone()
    prompt_THW[:, num_prompt_frames:] = model.mask_token_id
    for k, timestep in enumerate(range(num_prompt_frames, window_size)):
        if teacher_force_time:
            prompt_THW = example_THW.clone()
            prompt_THW[:, timestep:] = model.mask_token_id
        samples_HW, _ = model.maskgit_generate(prompt_THW, out_t=timestep, maskgit_steps=maskgit_steps,
                                               temperature=temperature, noise=None if noise is None else noise[k],
                                               return_logits=False, action_ids=action_ids, action_vectors=action_vectors, sampling=sampling,
                                               unmask_mode=unmask_mode, uniforms=None if uniforms is None else uniforms[k],
                                               guidance=guidance, known=None if known is None else known[:, k])
        samples.append(samples_HW)
        if not teacher_force_time:
            prompt_THW[:, timestep] = samples_HW  # autoregressive (already written in place by maskgit_generate)
    outputs = torch.stack(samples, dim=1)
    outputs = torch.cat([example_THW[:, :num_prompt_frames], outputs], dim=1)
    return torch.cat([outputs, example_THW[:, num_prompt_frames:]], dim=1)


@torch.no_grad()
def generate_frames_cached(model, example_THW: torch.LongTensor, num_prompt_frames=8, maskgit_steps=2, temperature=0.0,
                           teacher_force_time=False, noise=None, unmask_mode="random", merge_commit=True, host_loop=False,
                           action_ids=None, sampling=None, uniforms=None, guidance=None, action_vectors=None, known=None):
    """``generate_frames`` with a temporal KV cache (genie_frame_pass): every pass runs ONE frame through the stack
    against the cached temporal keys/values of the earlier frames instead of the full 16-frame forward --
    one P-frame pass for the prompt + (T-P)*(steps+1) single-frame passes (= 2 full-pass equivalents at P=8, steps=2) instead of (T-P)*steps full
    forwards (16).  Same outputs (per-row arithmetic is unchanged).
    merge_commit: where the library covers it (genie_frames_pass: f16x3, heads of 64 or 32, up to 16,384 rows per pass) the pass that commits frame t's
    final tokens also carries MaskGIT step 0 of frame t+1, so a frame costs `steps` passes instead of `steps + 1`.
    host_loop: False = the whole loop is ONE library call (genie_generate_cached: every pass, sampling and mask step enqueued
    without a host step in between); True = the same loop driven from Python (one C-ABI call per pass / sample / mask step).
    action_ids: (B, T) per-frame actions of an action-conditioned model (config.action_vocab_size > 0); every pass embeds
    frame t with action_ids[:, t].  action_vectors: (B, T, action_dim) float actions of a model with config.action_dim > 0 instead:
    one extra launch projects them into per-frame rows before the first pass, and every pass is the one the ids would run.
    sampling: a SamplingConfig or None = the reference's law; unmask_mode may be "confidence" (both as in maskgit_generate);
    uniforms: optional (T - num_prompt_frames, maskgit_steps, num_factored_vocabs, B, S) sampling draws to replay.
    guidance: a Guidance(scale, null_action) or None: classifier-free guidance.  Every pass then runs 2 B clips -- the clips under their
    actions, and the same tokens under null_action at every frame --, genie_sample_guided draws B rows from scale * conditional +
    (1 - scale) * null, and the frame's current tokens are mirrored into the second half before the next pass (both loop forms).
    known: optional (B, T - num_prompt_frames, H, W) int64 known tokens of the predicted frames (known_tokens): every frame starts from
    them, each clip re-masks by its own count of tokens left to generate, and its output keeps them (both loop forms)."""
    import math
    from . import _lib
    from .sampling import SamplingConfig, as_struct, unmask_code
    lib = _lib.load()
    mode = unmask_code(unmask_mode)
    law = as_struct(sampling)
    if mode == _lib.UNMASK_CONFIDENCE and law is None:
        law = as_struct(SamplingConfig())
    nv = model.config.num_factored_vocabs
    if uniforms is not None:
        uniforms = uniforms.to(device=example_THW.device, dtype=torch.float32).contiguous()
    cfg, w = model._weights()[:2]
    ex = example_THW.to(torch.int64).contiguous()
    B, T = ex.shape[0], ex.shape[1]
    S, V = model.config.S, model.config.factored_vocab_size * model.config.num_factored_vocabs
    P = num_prompt_frames
    assert P <= T and P >= 1
    dev = ex.device
    ids = ex.view(B, T, S)
    known = check_known(known, (B, T - P) + tuple(ex.shape[2:]), dev)
    kn = None if known is None else known.view(B, T - P, S)
    guide = model._guidance(guidance)
    cond = model._cond(action_ids, B, n_frames=T, action_vectors=action_vectors)
    NB = B if guide is None else 2 * B   # clips per pass: [conditional ; null] under guidance
    ws = model._workspace(B, generate_prompt_frames=P, guided=guide is not None)
    nbytes = lib.genie_prefix_cache_bytes(cfg, NB)
    cache = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    if not host_loop and P < T:
        steps = int(maskgit_steps)
        nz = None
        if steps > 1 and unmask_mode != "greedy":   # the draws of torch.rand_like (st_mask_git.py:204-206): the caller's, or fresh ones
            nz = (torch.rand(T - P, steps - 1, B, S, device=dev) if noise is None
                  else noise.to(dev)[:, :steps - 1].reshape(T - P, steps - 1, B, S).float().contiguous())
        uni = None
        if temperature > 1e-8:
            uni = torch.rand(T - P, steps, nv, B, S, device=dev) if uniforms is None else uniforms
            assert uni.numel() == (T - P) * steps * nv * B * S, "uniforms: (T - P, maskgit_steps, num_factored_vocabs, B, S)"
        gen = torch.empty(B, T - P, S, dtype=torch.int64, device=dev)
        _lib.check(_lib.call_known(lib, "genie_generate_cached", cond, law, guide, _lib.make_known(kn, T - P, S), cfg, w, ids.data_ptr(), B,
                                             P, T - P, steps, float(temperature), mode,
                                             0 if nz is None else nz.data_ptr(), 0 if uni is None else uni.data_ptr(),
                                             int(bool(teacher_force_time)), int(bool(merge_commit)), gen.data_ptr(), 0, cache.data_ptr(),
                                             nbytes, ws.data_ptr(), ws.numel(), st), "genie_generate_cached")
        outputs = torch.cat([ex[:, :P], gen.view(B, T - P, model.h, model.w)], dim=1)
        return torch.cat([outputs, ex[:, P:]], dim=1)

    if guide is not None:   # the doubled inputs: tokens twice, actions [the clips' ; null_action]
        cond = model._frame_cond(torch.cat([cond.keep, torch.full_like(cond.keep, guide.null_action)]).contiguous(), like=cond)
        ids = torch.cat([ids, ids]).contiguous()

    def frame_pass(tokens_BS, t, logits=None):
        _lib.check(_lib.call_cond(lib, "genie_frame_pass", cond, cfg, w, tokens_BS.data_ptr(), NB, t, cache.data_ptr(), nbytes,
                                  0 if logits is None else logits.data_ptr(), ws.data_ptr(), ws.numel(), st),
                   "genie_frame_pass")

    def commit_and_open(final_BS, mask_BS, t, logits):
        """Commit the final tokens of frame t AND run MaskGIT step 0 of frame t + 1 (all-mask tokens) in ONE two-frame pass
        (genie_frames_pass): frame t + 1 attends the slot the same pass writes.  False = the library does not cover two
        frames per pass for this model / batch (nothing was enqueued): the caller runs the two passes one by one."""
        two = torch.stack([final_BS, mask_BS], dim=1).contiguous()
        rc = _lib.call_cond(lib, "genie_frames_pass", cond, cfg, w, two.data_ptr(), NB, t, 2, cache.data_ptr(), nbytes,
                            logits.data_ptr(), ws.data_ptr(), ws.numel(), st)
        if rc == _lib.E_UNSUPPORTED:
            return False
        _lib.check(rc, "genie_frames_pass")
        return True

    # the prompt fills slots 0..P-1 of the cache in ONE P-frame pass: on the fragment-order kernels where they cover the model
    # (genie_frames_pass with nf = P), else genie_clean_pass with the cache's T-frame layout; geometries neither covers fill the
    # slots frame by frame
    rc = _lib.E_UNSUPPORTED
    if P > 1:
        rc = _lib.call_cond(lib, "genie_frames_pass", cond, cfg, w, ids[:, :P].contiguous().data_ptr(), NB, 0, P, cache.data_ptr(),
                            nbytes, 0, ws.data_ptr(), ws.numel(), st)
        if rc == _lib.E_UNSUPPORTED:
            rc = _lib.call_cond(lib, "genie_clean_pass", cond, cfg, w, ids[:, :P].contiguous().data_ptr(), NB, P, T, cache.data_ptr(),
                                nbytes, ws.data_ptr(), ws.numel(), st)
    if rc == _lib.E_UNSUPPORTED:
        for t in range(P):
            frame_pass(ids[:, t].contiguous(), t)
    else:
        _lib.check(rc, "genie_frames_pass / genie_clean_pass (prompt)")
    logits = torch.empty(NB, S, V, dtype=torch.float32, device=dev)
    samples = torch.empty(B, S, dtype=torch.int64, device=dev)
    conf = torch.empty(B, S, dtype=torch.float32, device=dev)
    gen = []
    opened = False   # step 0 of the current frame already ran inside the previous frame's commit pass
    for k, t in enumerate(range(P, T)):
        cur = torch.full((NB, S), model.mask_token_id, dtype=torch.int64, device=dev)   # (mask step: rows [0, B))
        unmasked = torch.zeros(B, S, dtype=torch.uint8, device=dev)
        if kn is not None:   # the frame starts from its known tokens, in both halves under guidance
            _lib.check(lib.genie_known_begin(kn[:, k].data_ptr(), (T - P) * S, model.mask_token_id, cur.data_ptr(), S, unmasked.data_ptr(),
                                             B, S, NB // B, st), "genie_known_begin")
        for step in range(maskgit_steps):
            if not (step == 0 and opened):
                frame_pass(cur, t, logits)
            uni = None
            if temperature > 1e-8:
                uni = (torch.rand(nv, B, S, device=dev) if uniforms is None
                       else uniforms.view(T - P, maskgit_steps, nv, B, S)[k, step].contiguous())
            last = step == maskgit_steps - 1
            keys, n = None, 0
            if not last:
                n = math.ceil(math.cos((step + 1) / maskgit_steps * math.pi / 2) * S)
                if unmask_mode == "greedy":
                    keys = conf
                elif noise is None:
                    keys = torch.rand(B, S, device=dev)
                else:
                    keys = noise[k][step].to(dev).reshape(B, S).float().contiguous()
            by_conf = mode == _lib.UNMASK_CONFIDENCE and not last
            if guide is not None:
                draws, keys = keys, (torch.empty(B, S, device=dev) if by_conf else keys)
                _lib.check(lib.genie_sample_guided(cfg, logits[:B].data_ptr(), logits[B:].data_ptr(), _lib.LAYOUT_TOKEN_MAJOR, B,
                                                   float(temperature), 0 if uni is None else uni.data_ptr(), samples.data_ptr(),
                                                   conf.data_ptr(), st, law, keys.data_ptr() if by_conf else 0,
                                                   draws.data_ptr() if by_conf else 0, 1.0 - (step + 1) / maskgit_steps, guide.scale),
                           "genie_sample_guided")
            elif law is None:
                _lib.check(lib.genie_sample(cfg, logits.data_ptr(), _lib.LAYOUT_TOKEN_MAJOR, B, float(temperature),
                                            0 if uni is None else uni.data_ptr(), samples.data_ptr(), conf.data_ptr(), st),
                           "genie_sample")
            else:   # "confidence": the same launch turns the step's draws into its keys
                draws, keys = keys, (torch.empty(B, S, device=dev) if by_conf else keys)
                _lib.check(lib.genie_sample_ex(cfg, logits.data_ptr(), _lib.LAYOUT_TOKEN_MAJOR, B, float(temperature),
                                               0 if uni is None else uni.data_ptr(), samples.data_ptr(), conf.data_ptr(), st, law,
                                               keys.data_ptr() if by_conf else 0, draws.data_ptr() if by_conf else 0,
                                               1.0 - (step + 1) / maskgit_steps), "genie_sample_ex")
            if kn is not None:   # each clip's own count: ceil(frac * (S - its known tokens)), taken by the kernel
                frac = 0.0 if last else lib.genie_mask_fraction(step, maskgit_steps)
                _lib.check(lib.genie_mask_step_known(0 if keys is None else keys.data_ptr(), frac, int(last), model.mask_token_id,
                                                     kn[:, k].data_ptr(), (T - P) * S, unmasked.data_ptr(), samples.data_ptr(),
                                                     cur.data_ptr(), S, B, S, st), "genie_mask_step_known")
            else:
                _lib.check(lib.genie_mask_step(0 if keys is None else keys.data_ptr(), n, int(last), model.mask_token_id,
                                               unmasked.data_ptr(), samples.data_ptr(), cur.data_ptr(), S, B, S, st),
                           "genie_mask_step")
            if guide is not None:
                cur[B:] = cur[:B]   # the null half sees the same tokens
        gen.append(cur[:B].view(B, model.h, model.w))
        opened = False
        if t + 1 < T:  # commit frame t (its final tokens, or the ground truth when teacher-forcing in time)
            final = ids[:, t].contiguous() if teacher_force_time else cur
            if merge_commit:
                nxt = torch.full_like(cur, model.mask_token_id)
                if kn is not None:   # the slot the commit opens starts from ITS known tokens
                    _lib.check(lib.genie_known_begin(kn[:, k + 1].data_ptr(), (T - P) * S, model.mask_token_id, nxt.data_ptr(), S, 0, B, S,
                                                     NB // B, st), "genie_known_begin")
                opened = commit_and_open(final, nxt, t, logits)
                merge_commit = opened   # (unsupported once = unsupported for the whole call)
            if not opened:
                frame_pass(final, t)
    outputs = torch.cat([ex[:, :P], torch.stack(gen, dim=1)], dim=1)
    return torch.cat([outputs, ex[:, P:]], dim=1)


def frame_window(f, P, keep, T):
    """(j, start, slot) of the generated absolute frame f >= P: it is decoded in slot ``slot`` of window ``j``, which starts at absolute
    frame ``start`` (include/genie_hip.h, "rollout past the context window"); its context is the frames [start, f)."""
    hop = T - keep
    j = 0 if f < T else 1 + (f - T) // hop
    return j, j * hop, f - j * hop


def window_schedule(P, keep, T, n_new):
    """The windows of a rollout of n_new frames behind P prompt frames: a list of (j, start, f_begin, f_end), in order -- window j holds
    the absolute frames [start, start + T) in its T slots, runs [start, f_begin) as its context and decodes [f_begin, f_end).  Window 0
    decodes up to T - P frames, every later one up to hop = T - keep."""
    if not (1 <= P <= T - 1 and 1 <= keep <= T - 1):
        raise ValueError(f"rollout: prompt frames {P} and keep {keep} must lie in [1, {T - 1}]")
    out, f, end = [], P, P + n_new
    while f < end:
        j, start, _ = frame_window(f, P, keep, T)
        nxt = min(start + T, end)
        out.append((j, start, f, nxt))
        f = nxt
    return out


def _rollout_actions(model, action_ids, B, n, what="action_ids"):
    """Checked (B, n) int64 device actions of a rollout, or None for a model without actions."""
    A = model.config.action_vocab_size
    if not A:
        if action_ids is not None:
            raise ValueError(f"{what} given to a model without actions (config.action_vocab_size == 0)")
        return None
    if action_ids is None:
        raise ValueError(f"this model is action-conditioned (action_vocab_size={A}): pass {what} ({B}, {n})")
    a = torch.as_tensor(action_ids)
    if a.dtype.is_floating_point or a.dtype == torch.bool:
        raise RuntimeError(f"{what} must be an integer tensor, got {a.dtype}")
    if tuple(a.shape) != (B, n):
        raise RuntimeError(f"expected {what} of shape ({B}, {n}), got {tuple(a.shape)}")
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= A):
        raise IndexError(f"action id out of range [0, {A}): min {int(a.min())}, max {int(a.max())}")
    return a.to(device=model.pos_embed_TSC.device, dtype=torch.int64).contiguous()


def _rollout_vectors(model, action_vectors, B, n, what="action_vectors"):
    """Checked (n, B, action_dim) float32 device vectors of n rollout frames, frame-major (the order of their rows)."""
    v = model.check_action_vectors(action_vectors, (B, n, model.config.action_dim), what)
    return v.transpose(0, 1).contiguous()


def _rollout_row_ids(B, cap, dev):
    """(B, cap) int64: frame f of clip b reads row 1 + f B + b -- frame-major behind the null row 0, so a growing rollout appends rows."""
    return (1 + torch.arange(cap, device=dev)[None, :] * B + torch.arange(B, device=dev)[:, None]).to(torch.int64).contiguous()


def _rollout_inputs(model, action_ids, action_vectors, B, n, what="action_ids"):
    """(ids, vectors) of n rollout frames, one of them None -- or both for an unconditioned model; raises like STMaskGIT._cond."""
    if action_ids is not None and action_vectors is not None:
        raise ValueError("pass action_ids or action_vectors, not both")
    if model.config.action_dim:
        if action_ids is not None:
            raise ValueError(f"{what} given to a model conditioned on action vectors (action_dim={model.config.action_dim})")
        return None, _rollout_vectors(model, action_vectors, B, n)
    if action_vectors is not None:
        raise ValueError("action_vectors given to a model without continuous actions (config.action_dim == 0)")
    return _rollout_actions(model, action_ids, B, n, what), None


class _Decode:
    """The decode options of a rollout, resolved once: MaskGIT steps, unmasking mode, sampling law, guidance."""

    def __init__(self, model, maskgit_steps, temperature, unmask_mode, sampling, guidance, merge_commit):
        from . import _lib
        from .sampling import SamplingConfig, as_struct, unmask_code
        self.steps, self.temperature, self.merge_commit = int(maskgit_steps), float(temperature), bool(merge_commit)
        self.unmask_mode, self.mode, self.law = unmask_mode, unmask_code(unmask_mode), as_struct(sampling)
        if self.mode == _lib.UNMASK_CONFIDENCE and self.law is None:
            self.law = as_struct(SamplingConfig())
        self.guide = model._guidance(guidance)

    def draws(self, model, n, B, noise, uniforms, dev):
        """The (n, steps - 1, B, S) unmasking draws and (n, steps, nv, B, S) sampling draws of n frames: the caller's, or torch.rand."""
        S, nv, steps = model.config.S, model.config.num_factored_vocabs, self.steps
        nz = uni = None
        if steps > 1 and self.unmask_mode != "greedy":
            nz = (torch.rand(n, steps - 1, B, S, device=dev) if noise is None
                  else noise.to(dev).reshape(n, -1, B, S)[:, :steps - 1].float().contiguous())
        if self.temperature > 1e-8:
            uni = (torch.rand(n, steps, nv, B, S, device=dev) if uniforms is None
                   else uniforms.to(device=dev, dtype=torch.float32).contiguous())
            assert uni.numel() == n * steps * nv * B * S, "uniforms: (n frames, maskgit_steps, num_factored_vocabs, B, S)"
        return nz, uni


def rollout_call(model, frames_BcS, actions_Bc, P, keep, f0, f1, resume, cache, dec, nz, uni, rows=None, known=None):
    """ONE genie_rollout_cached call: generates the absolute frames [f0, f1) of frames_BcS (B, cap, S) int64 in place.  actions_Bc: (B, cap)
    int64 or None -- rows of the model's action table, or of `rows` (a projected row table of a model conditioned on action vectors); cache: uint8 tensor of genie_prefix_cache_bytes(cfg, NB); dec: the _Decode options; nz / uni: this call's draws.
    known: (B, f1 - f0, S) int64 contiguous known tokens of this call's frames, or None."""
    from . import _lib
    lib = _lib.load()
    cfg, w = model._weights()[:2]
    B, cap, S = frames_BcS.shape
    assert frames_BcS.dtype == torch.int64 and frames_BcS.is_contiguous()
    T = model.config.T
    cond = None
    if actions_Bc is not None:
        assert actions_Bc.shape == (B, cap) and actions_Bc.dtype == torch.int64 and actions_Bc.is_contiguous()
        if rows is not None:
            cond = _lib.FrameCond(table=rows.data_ptr(), ids=actions_Bc.data_ptr(), n_actions=rows.shape[0])
        else:
            cond = _lib.FrameCond(table=model.action_embed.weight.data_ptr(), ids=actions_Bc.data_ptr(),
                                  n_actions=model.config.action_vocab_size)
    # the largest context the call runs sizes its workspace: `keep` for every window it opens after its first, and for the first the frames
    # before f0 -- unless the call resumes in mid-window, where it runs none
    wins = [w for w in window_schedule(P, keep, T, f1 - P) if w[3] > f0]
    ctx = [fb - start for _, start, fb, _ in wins[1:]]
    ctx.append(f0 - wins[0][1] if (not resume or f0 == wins[0][2]) else 1)
    ws = model._workspace(B, guided=dec.guide is not None, rollout_ctx=max(ctx))
    if known is not None:
        assert known.shape == (B, f1 - f0, S) and known.dtype == torch.int64 and known.is_contiguous()
    _lib.check(_lib.call_known3(lib, "genie_rollout_cached", _lib.make_known(known, f1 - f0, S), cfg, w, frames_BcS.data_ptr(), B, P, keep,
                                cap, f0, f1, int(resume), dec.steps, dec.temperature,
                                dec.mode, 0 if nz is None else nz.data_ptr(), 0 if uni is None else uni.data_ptr(),
                                int(dec.merge_commit), cache.data_ptr(), cache.numel(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream, cond, dec.law, dec.guide), "genie_rollout_cached")


def _rollout_cache(model, B, dec, dev):
    from . import _lib
    cfg = model._weights()[0]
    return torch.empty(_lib.load().genie_prefix_cache_bytes(cfg, B if dec.guide is None else 2 * B), dtype=torch.uint8, device=dev)


@torch.no_grad()
def rollout_frames(model, prompt_BPHW: torch.LongTensor, n_new, keep=None, maskgit_steps=2, temperature=0.0, unmask_mode="random",
                   noise=None, uniforms=None, action_ids=None, sampling=None, guidance=None, merge_commit=True, action_vectors=None,
                   known=None):
    """Generate n_new frames behind the P prompt frames of prompt_BPHW (B, P, H, W), past the model's window T if need be, in ONE library
    call (genie_rollout_cached) -> (B, P + n_new, H, W).  Window 0 decodes frames [P, T); after that the window slides: the last ``keep``
    frames (default P; 1 <= keep <= T - 1) are re-run as the context of the next hop = T - keep frames (window_schedule; positions are
    absolute, so the KV cache cannot be shifted).  keep is a quality / cost dial: keep = T - 1 is the true sliding window.  Equal, bit
    for bit, to chaining generate_frames_cached window by window on the same draws.
    noise: optional (n_new, maskgit_steps - 1, B, S); uniforms: optional (n_new, maskgit_steps, num_factored_vocabs, B, S); fresh
    torch.rand draws otherwise.  action_ids: (B, P + n_new), the actions of the absolute frames; action_vectors: (B, P + n_new, action_dim)
    for a model with config.action_dim > 0 (one launch projects all of them before the call).  The other options: generate_frames_cached.
    known: optional (B, n_new, H, W) int64 known tokens of the generated frames (known_tokens)."""
    cfg = model.config
    pr = prompt_BPHW.to(torch.int64)
    B, P = pr.shape[0], pr.shape[1]
    known = check_known(known, (B, int(n_new), model.h, model.w), pr.device)
    keep = P if keep is None else int(keep)
    n_new = int(n_new)
    if n_new < 1:
        raise ValueError("rollout_frames: n_new must be >= 1")
    window_schedule(P, keep, cfg.T, n_new)   # (checks P and keep)
    dev = pr.device
    dec = _Decode(model, maskgit_steps, temperature, unmask_mode, sampling, guidance, merge_commit)
    acts, vecs = _rollout_inputs(model, action_ids, action_vectors, B, P + n_new)
    rows = None
    if vecs is not None:
        rows = model.new_row_table((P + n_new) * B)
        model.project_actions(vecs.view(-1, vecs.shape[-1]), rows[1:])
        acts = _rollout_row_ids(B, P + n_new, dev)
    frames = torch.full((B, P + n_new, cfg.S), model.mask_token_id, dtype=torch.int64, device=dev)
    frames[:, :P] = pr.reshape(B, P, cfg.S)
    nz, uni = dec.draws(model, n_new, B, noise, uniforms, dev)
    rollout_call(model, frames, acts, P, keep, P, P + n_new, 0, _rollout_cache(model, B, dec, dev), dec, nz, uni, rows=rows,
                 known=None if known is None else known.view(B, n_new, cfg.S))
    return frames.view(B, P + n_new, model.h, model.w)


def _fanout_inputs(model, prompt_BPHW, n_new, K, action_ids, action_vectors, prompt_actions, prompt_action_vectors):
    """The checked inputs of fanout_frames, before the library is touched -> (B, P, K, prompt ids (B, P) or None, branch ids (B K, n_new)
    or None, prompt vectors (B, P, A) or None, branch vectors (B K, n_new, A) or None); raises in the style of _rollout_inputs."""
    cfg = model.config
    if prompt_BPHW.dim() != 4 or prompt_BPHW.shape[2] * prompt_BPHW.shape[3] != cfg.S:
        raise RuntimeError(f"expected prompt frames (B, P, H, W) of {cfg.S} tokens each, got {tuple(prompt_BPHW.shape)}")
    B, P, n_new = prompt_BPHW.shape[0], prompt_BPHW.shape[1], int(n_new)
    if n_new < 1 or P < 1 or P + n_new > cfg.T:
        raise ValueError(f"fanout_frames: {P} prompt + {n_new} new frames must lie inside the window of {cfg.T} (in-window generation; "
                         "a longer horizon continues with rollout_frames on the B * K results)")
    if action_ids is not None and action_vectors is not None:
        raise ValueError("pass action_ids or action_vectors, not both")
    given = action_ids if action_ids is not None else action_vectors
    want = 3 if action_ids is not None else 4
    if given is not None:
        g = torch.as_tensor(given)
        if g.dim() != want or g.shape[0] != B or g.shape[2] != n_new:
            what = "action_ids" if action_ids is not None else "action_vectors"
            shape = f"({B}, K, {n_new})" if action_ids is not None else f"({B}, K, {n_new}, {cfg.action_dim})"
            raise RuntimeError(f"expected {what} of shape {shape}, got {tuple(g.shape)}")
        if K is not None and int(K) != g.shape[1]:
            raise ValueError(f"K = {K} but the actions hold {g.shape[1]} branches per clip")
        K = g.shape[1]
    if K is None:
        raise ValueError("fanout_frames: pass K (branches per clip), or per-branch actions that carry it")
    K = int(K)
    if K < 1:
        raise ValueError(f"fanout_frames: K = {K} must be >= 1")
    if cfg.action_dim:
        if action_ids is not None or prompt_actions is not None:
            raise ValueError(f"action ids given to a model conditioned on action vectors (action_dim={cfg.action_dim})")
        pv = model.check_action_vectors(prompt_action_vectors, (B, P, cfg.action_dim), "prompt_action_vectors")
        bv = model.check_action_vectors(action_vectors, (B, K, n_new, cfg.action_dim))
        return B, P, K, None, None, pv, bv.view(B * K, n_new, cfg.action_dim)
    if action_vectors is not None or prompt_action_vectors is not None:
        raise ValueError("action vectors given to a model without continuous actions (config.action_dim == 0)")
    pa = _rollout_actions(model, prompt_actions, B, P, "prompt_actions")
    ba = _rollout_actions(model, None if action_ids is None else torch.as_tensor(action_ids).reshape(B * K, n_new), B * K, n_new)
    return B, P, K, pa, ba, None, None


@torch.no_grad()
def fanout_frames(model, prompt_BPHW: torch.LongTensor, n_new, K=None, action_ids=None, action_vectors=None, prompt_actions=None,
                  prompt_action_vectors=None, maskgit_steps=2, temperature=0.0, unmask_mode="random", sampling=None, guidance=None,
                  merge_commit=True, noise=None, uniforms=None, known=None):
    """K candidate futures of n_new frames for each of the B prompts (B, P, H, W) -> (B, K, n_new, H, W), in ONE library call
    (genie_generate_fanout): the context runs once per clip into a shared trunk cache, and the decode passes run B * K clips that read the
    trunk's slots [0, P) and keep only their own n_new slots.  In-window: P + n_new <= T.  Branch k of clip b equals clip b * K + k of
    generate_frames_cached on the K-times replicated batch with that branch's actions and draws.
    action_ids: (B, K, n_new) actions of the new frames, with prompt_actions (B, P) for the prompt; a model with config.action_dim > 0
    takes action_vectors (B, K, n_new, action_dim) and prompt_action_vectors (B, P, action_dim) instead (one launch each projects them into
    one row table; row 0 is action_null).  K is taken from them; an unconditioned model takes K explicitly, and its branches differ by
    their draws only.  noise: optional (n_new, maskgit_steps - 1, B * K, S); uniforms: optional (n_new, maskgit_steps, num_factored_vocabs,
    B * K, S); fresh torch.rand draws otherwise.  The other options: generate_frames_cached.
    known: optional int64 known tokens of the new frames (known_tokens), (B, K, n_new, H, W) per branch or (B, n_new, H, W) for all K.
    A longer horizon continues by handing the (B * K) results, behind their prompts, to rollout_frames as prompts."""
    B, P, K, pa, ba, pv, bv = _fanout_inputs(model, prompt_BPHW, n_new, K, action_ids, action_vectors, prompt_actions, prompt_action_vectors)
    n_new = int(n_new)
    dec = _Decode(model, maskgit_steps, temperature, unmask_mode, sampling, guidance, merge_commit)
    pr = prompt_BPHW.to(torch.int64).reshape(B, P, model.config.S).contiguous()
    if isinstance(known, torch.Tensor) and known.dim() == 4:   # one set of known tokens for the K branches of a clip
        known = check_known(known, (B, n_new, model.h, model.w), pr.device)[:, None].expand(B, K, n_new, model.h, model.w)
    known = check_known(known, (B, K, n_new, model.h, model.w), pr.device)
    cond = fanout_cond(model, B, P, K, n_new, pa, ba, pv, bv, pr.device)
    nz, uni = dec.draws(model, n_new, B * K, noise, uniforms, pr.device)
    return fanout_call(model, pr, K, n_new, cond, dec, nz, uni,
                       known=None if known is None else known.reshape(B * K, n_new, model.config.S)).view(B, K, n_new, model.h, model.w)


def fanout_cond(model, B, P, K, n_new, prompt_ids, branch_ids, prompt_vectors, branch_vectors, dev):
    """The genie_frame_cond of a fan-out call from checked inputs (_fanout_inputs), None for an unconditioned model: ids (B K, T),
    branch-major -- the prompt's actions in every branch, then the branch's own, 0 past P + n_new (never embedded).  Vectors are projected
    into one row table (one launch for the prompt's, one for the branches'); row 0 is action_null."""
    from . import _lib
    if branch_ids is None and branch_vectors is None:
        return None
    ids = torch.zeros(B, K, model.config.T, dtype=torch.int64, device=dev)
    if branch_vectors is not None:
        rows = model.new_row_table(B * P + B * K * n_new)
        model.project_actions(prompt_vectors.view(B * P, -1), rows[1:1 + B * P])
        model.project_actions(branch_vectors.view(B * K * n_new, -1), rows[1 + B * P:])
        ids[:, :, :P] = (1 + torch.arange(B * P, device=dev)).view(B, 1, P)
        ids[:, :, P:P + n_new] = (1 + B * P + torch.arange(B * K * n_new, device=dev)).view(B, K, n_new)
        cond = _lib.FrameCond(table=rows.data_ptr(), ids=ids.data_ptr(), n_actions=rows.shape[0])
        cond.rows = rows
    else:
        ids[:, :, :P] = prompt_ids[:, None]
        ids[:, :, P:P + n_new] = branch_ids.view(B, K, n_new)
        cond = _lib.FrameCond(table=model.action_embed.weight.data_ptr(), ids=ids.data_ptr(), n_actions=model.config.action_vocab_size)
    cond.keep = ids   # the ids tensor lives as long as the struct
    return cond


def fanout_call(model, prompt_BPS, K, n_new, cond, dec, nz, uni, trunk=None, branch=None, known=None):
    """ONE genie_generate_fanout call -> gen (B, K, n_new, S) int64.  prompt_BPS: (B, P, S) int64, contiguous; cond: fanout_cond; dec: the
    _Decode options; nz / uni: the call's draws over B K rows.  trunk / branch: uint8 tensors of genie_prefix_cache_bytes(cfg, NB) and
    genie_fanout_branch_bytes(cfg, NB, K, n_new) to keep what the call leaves in them (allocated here otherwise).  known: (B K, n_new, S)
    int64 contiguous known tokens of the branches' frames, or None."""
    from . import _lib
    lib = _lib.load()
    cfg, w = model._weights()[:2]
    B, P, S = prompt_BPS.shape
    assert prompt_BPS.dtype == torch.int64 and prompt_BPS.is_contiguous()
    if known is not None:
        assert known.shape == (B * K, n_new, S) and known.dtype == torch.int64 and known.is_contiguous()
    dev = prompt_BPS.device
    NB = B if dec.guide is None else 2 * B
    if trunk is None:
        trunk = torch.empty(lib.genie_prefix_cache_bytes(cfg, NB), dtype=torch.uint8, device=dev)
    if branch is None:
        branch = torch.empty(lib.genie_fanout_branch_bytes(cfg, NB, K, n_new), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.genie_fanout_workspace_bytes(cfg, B, K, P, int(dec.guide is not None)), dtype=torch.uint8, device=dev)
    gen = torch.empty(B, K, n_new, S, dtype=torch.int64, device=dev)
    _lib.check(_lib.call_known3(lib, "genie_generate_fanout", _lib.make_known(known, n_new, S), cfg, w, prompt_BPS.data_ptr(), B, K, P, n_new,
                                dec.steps, dec.temperature, dec.mode,
                                0 if nz is None else nz.data_ptr(), 0 if uni is None else uni.data_ptr(), int(dec.merge_commit),
                                gen.data_ptr(), trunk.data_ptr(), trunk.numel(), branch.data_ptr(), branch.numel(), ws.data_ptr(),
                                ws.numel(), torch.cuda.current_stream().cuda_stream, cond, dec.law, dec.guide), "genie_generate_fanout")
    return gen


class Score:
    """What score_frames returns: nll (B, K, n) float64, the negative log-likelihood of each observed frame under each branch; hits
    (B, K, n) float64, the count of tokens whose argmax equals the observed token in every factor; token_nll (B, K, n, H, W) float32, or
    None unless per_token was asked for."""

    def __init__(self, nll, hits, token_nll=None):
        self.nll, self.hits, self.token_nll = nll, hits, token_nll

    def __repr__(self):
        return f"Score(nll={tuple(self.nll.shape)}, per_token={self.token_nll is not None})"


def _score_inputs(model, clip_BTHW, num_prompt_frames, K, action_ids, action_vectors, prompt_actions, prompt_action_vectors):
    """The checked inputs of score_frames, before the library is touched -> (B, P, n, K, prompt ids, branch ids, prompt vectors, branch
    vectors) with the last four as _fanout_inputs returns them; raises in its style."""
    cfg = model.config
    clip = torch.as_tensor(clip_BTHW)
    if clip.dim() != 4 or clip.shape[2] * clip.shape[3] != cfg.S:
        raise RuntimeError(f"expected an observed clip (B, P + n, H, W) of {cfg.S} tokens per frame, got {tuple(clip.shape)}")
    if clip.dtype.is_floating_point or clip.dtype == torch.bool:
        raise RuntimeError(f"the clip must be an integer tensor of token ids, got {clip.dtype}")
    P, n = int(num_prompt_frames), clip.shape[1] - int(num_prompt_frames)
    if P < 1 or n < 1 or P + n > cfg.T:
        raise ValueError(f"score_frames: {P} prompt + {n} scored frames must lie inside the window of {cfg.T}, with at least one of each")
    if clip.numel() and (int(clip.min()) < 0 or int(clip.max()) >= cfg.image_vocab_size):
        raise IndexError(f"token id out of range [0, {cfg.image_vocab_size}): min {int(clip.min())}, max {int(clip.max())} (an observed "
                         "clip holds no mask tokens)")
    if K is None and action_ids is None and action_vectors is None:
        raise ValueError("score_frames: pass K (hypotheses per clip; 1 scores the clip itself), or per-branch actions that carry it")
    B, P, K, pa, ba, pv, bv = _fanout_inputs(model, clip[:, :P], n, K, action_ids, action_vectors, prompt_actions, prompt_action_vectors)
    return B, P, n, K, pa, ba, pv, bv


def score_call(model, clip_BTS, P, K, cond, merge_commit=True, per_token=False, trunk=None, branch=None):
    """ONE genie_score_fanout call -> (nll (B, K, n) float64, hits (B, K, n) float64, token_nll (B, K, n, S) float32 or None).  clip_BTS:
    (B, P + n, S) int64, contiguous, the observed tokens; cond: fanout_cond.  trunk / branch: uint8 tensors of genie_prefix_cache_bytes(cfg,
    B) and genie_fanout_branch_bytes(cfg, B, K, n) to keep what the call leaves in them (allocated here otherwise)."""
    from . import _lib
    lib = _lib.load()
    cfg, w = model._weights()[:2]
    B, Tc, S = clip_BTS.shape
    n = Tc - P
    assert clip_BTS.dtype == torch.int64 and clip_BTS.is_contiguous()
    dev = clip_BTS.device
    if trunk is None:
        trunk = torch.empty(lib.genie_prefix_cache_bytes(cfg, B), dtype=torch.uint8, device=dev)
    if branch is None:
        branch = torch.empty(lib.genie_fanout_branch_bytes(cfg, B, K, n), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.genie_score_workspace_bytes(cfg, B, K, P), dtype=torch.uint8, device=dev)
    nll = torch.empty(B, K, n, dtype=torch.float64, device=dev)
    hits = torch.empty(B, K, n, dtype=torch.float64, device=dev)
    tok = torch.empty(B, K, n, S, dtype=torch.float32, device=dev) if per_token else None
    _lib.check(lib.genie_score_fanout(cfg, w, clip_BTS.data_ptr(), B, K, P, n, int(bool(merge_commit)), nll.data_ptr(), hits.data_ptr(),
                                      0 if tok is None else tok.data_ptr(), trunk.data_ptr(), trunk.numel(), branch.data_ptr(), branch.numel(),
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream, cond), "genie_score_fanout")
    return nll, hits, tok


@torch.no_grad()
def score_frames(model, clip_BTHW: torch.LongTensor, num_prompt_frames, K=None, action_ids=None, action_vectors=None, prompt_actions=None,
                 prompt_action_vectors=None, per_token=False, merge_commit=True):
    """How likely is what DID happen under each of K action hypotheses?  clip_BTHW (B, P + n, H, W): the observed tokens, P =
    num_prompt_frames of them context.  -> Score with nll[b, k, j] = - sum over the frame's tokens and factors of log softmax(logits)[observed
    token], the logits being MaskGIT step 0 of frame P + j (all-mask) behind the observed frames before it, under branch k's actions --
    what generate_frames_cached(teacher_force_time=True) reports as its step-0 logits.  ONE library call (genie_score_fanout): the context
    runs once per clip, the B * K hypotheses read it through the fan-out cache, and no logits leave the library.  In-window: P + n <= T.
    action_ids (B, K, n) with prompt_actions (B, P), or action_vectors (B, K, n, action_dim) with prompt_action_vectors (B, P, action_dim),
    as in fanout_frames; K is taken from them.  An unconditioned model takes K explicitly (K = 1: per-clip, per-frame scoring).
    per_token: also return token_nll (B, K, n, H, W)."""
    B, P, n, K, pa, ba, pv, bv = _score_inputs(model, clip_BTHW, num_prompt_frames, K, action_ids, action_vectors, prompt_actions,
                                               prompt_action_vectors)
    clip = torch.as_tensor(clip_BTHW).to(device=model._device(), dtype=torch.int64).reshape(B, P + n, model.config.S).contiguous()
    cond = fanout_cond(model, B, P, K, n, pa, ba, pv, bv, clip.device)
    nll, hits, tok = score_call(model, clip, P, K, cond, merge_commit=merge_commit, per_token=per_token)
    return Score(nll, hits, None if tok is None else tok.view(B, K, n, model.h, model.w))


def infer_actions(model, clip_BTHW, num_prompt_frames, **kwargs):
    """Inverse dynamics by likelihood: which of the K action sequences explains the observed frames best?  -> (best (B,) int64, the argmin
    over k of nll.sum(-1); nll (B, K, n) float64).  Arguments: score_frames.  The model does not promise that this recovers the actions a
    future was generated with."""
    nll = score_frames(model, clip_BTHW, num_prompt_frames, **kwargs).nll
    return nll.sum(-1).argmin(dim=1), nll


class Rollout:
    """An open-ended rollout: ``step(action)`` returns the next frame, ``extend(n, action_ids)`` the next n, each ONE
    genie_rollout_cached call that resumes the temporal KV cache of the call before it (the first runs the prompt).  Same frames as
    rollout_frames on the same draws, however the calls are split.  The object owns the (B, cap, S) token and (B, cap) action buffers
    and the cache; the buffers grow by doubling cap (a copy, which leaves the cache valid).
    prompt_actions: (B, P) actions of the prompt frames of an action-conditioned model; keep and the decode options: rollout_frames.
    A model with config.action_dim > 0 takes prompt_vectors (B, P, action_dim) here and (B, action_dim) / (B, n, action_dim) floats in
    step / extend: each call projects only its new frames' vectors (one launch) into rows appended to the object's row table."""

    def __init__(self, model, prompt_BPHW, keep=None, prompt_actions=None, maskgit_steps=2, temperature=0.0, unmask_mode="random",
                 sampling=None, guidance=None, merge_commit=True, capacity=None, prompt_vectors=None):
        cfg = model.config
        pr = prompt_BPHW.to(torch.int64)
        self.model, self.B, self.P = model, pr.shape[0], pr.shape[1]
        self.keep = self.P if keep is None else int(keep)
        window_schedule(self.P, self.keep, cfg.T, 0)   # (checks P and keep)
        self.dec = _Decode(model, maskgit_steps, temperature, unmask_mode, sampling, guidance, merge_commit)
        self.n = self.P   # frames so far
        cap = max(self.P + 1, 2 * cfg.T if capacity is None else int(capacity))
        self._frames = torch.full((self.B, cap, cfg.S), model.mask_token_id, dtype=torch.int64, device=pr.device)
        self._frames[:, :self.P] = pr.reshape(self.B, self.P, cfg.S)
        acts, vecs = _rollout_inputs(model, prompt_actions, prompt_vectors, self.B, self.P, "prompt_actions")
        self._acts = self._rows = None
        if vecs is not None:
            self._rows = model.new_row_table(cap * self.B)
            model.project_actions(vecs.view(-1, vecs.shape[-1]), self._rows[1:1 + self.P * self.B])
            self._acts = _rollout_row_ids(self.B, cap, pr.device)
        elif acts is not None:
            self._acts = torch.zeros(self.B, cap, dtype=torch.int64, device=pr.device)
            self._acts[:, :self.P] = acts
        self._cache = _rollout_cache(model, self.B, self.dec, pr.device)
        self._resume = 0

    @property
    def frames(self):
        """(B, n_so_far, H, W): the prompt and every frame generated so far."""
        return self._frames[:, :self.n].reshape(self.B, self.n, self.model.h, self.model.w)

    @property
    def window(self):
        """(j, start, slot) of the NEXT frame (frame_window)."""
        return frame_window(self.n, self.P, self.keep, self.model.config.T)

    def _grow(self, need):
        cap = self._frames.shape[1]
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        frames = torch.full((self.B, cap, self._frames.shape[2]), self.model.mask_token_id, dtype=torch.int64, device=self._frames.device)
        frames[:, :self.n] = self._frames[:, :self.n]
        self._frames = frames
        if self._rows is not None:
            rows = self.model.new_row_table(cap * self.B)
            rows[:1 + self.n * self.B] = self._rows[:1 + self.n * self.B]
            self._rows, self._acts = rows, _rollout_row_ids(self.B, cap, frames.device)
        elif self._acts is not None:
            acts = torch.zeros(self.B, cap, dtype=torch.int64, device=frames.device)
            acts[:, :self.n] = self._acts[:, :self.n]
            self._acts = acts

    @torch.no_grad()
    def extend(self, n, action_ids=None, noise=None, uniforms=None, action_vectors=None, known=None):
        """Generate the next n frames -> (B, n, H, W).  action_ids: (B, n) actions of the new frames (action_vectors: (B, n, action_dim)
        for a model with config.action_dim > 0); noise (n, steps - 1, B, S) and
        uniforms (n, steps, nv, B, S): this call's draws, or fresh torch.rand ones.  known: optional (B, n, H, W) int64 known tokens of
        the new frames (known_tokens)."""
        n = int(n)
        if n < 1:
            raise ValueError("Rollout.extend: n must be >= 1")
        known = check_known(known, (self.B, n, self.model.h, self.model.w), self._frames.device)
        acts, vecs = _rollout_inputs(self.model, action_ids, action_vectors, self.B, n)
        f0, f1 = self.n, self.n + n
        self._grow(f1)
        if vecs is not None:
            self.model.project_actions(vecs.view(-1, vecs.shape[-1]), self._rows[1 + f0 * self.B:1 + f1 * self.B])
        elif acts is not None:
            self._acts[:, f0:f1] = acts
        nz, uni = self.dec.draws(self.model, n, self.B, noise, uniforms, self._frames.device)
        rollout_call(self.model, self._frames, self._acts, self.P, self.keep, f0, f1, self._resume, self._cache, self.dec, nz, uni,
                     rows=self._rows, known=None if known is None else known.view(self.B, n, -1))
        self.n, self._resume = f1, 1
        return self._frames[:, f0:f1].reshape(self.B, n, self.model.h, self.model.w)

    def step(self, action=None, noise=None, uniforms=None, known=None):
        """Generate the next frame under ``action`` (B,) -> (B, H, W); a model with config.action_dim > 0 takes the frame's (B, action_dim)
        float vectors.  noise (steps - 1, B, S), uniforms (steps, nv, B, S): its draws.  known: optional (B, H, W) int64 known tokens."""
        known = None if known is None else check_known(known, (self.B, self.model.h, self.model.w), self._frames.device)[:, None]
        nz, uni = None if noise is None else noise[None], None if uniforms is None else uniforms[None]
        if self.model.config.action_dim and action is not None:
            v = torch.as_tensor(action)
            if v.dim() != 2 or v.shape[0] != self.B:
                raise RuntimeError(f"expected the frame's action vectors of shape ({self.B}, {self.model.config.action_dim}), got {tuple(v.shape)}")
            return self.extend(1, None, nz, uni, action_vectors=v[:, None], known=known)[:, 0]
        a = None if action is None else torch.as_tensor(action).reshape(self.B, 1)
        return self.extend(1, a, nz, uni, known=known)[:, 0]


def write_outputs(outputs_THW: torch.LongTensor, output_dir, dataset_metadata: dict, args: dict):
    """video.bin (token_dtype of the source dataset) + metadata.json with the reference's extra keys
    (generate.py:105-116).  outputs for ONE example: (1, n, H, W) or (n, H, W)."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    out = outputs_THW.reshape(-1, *outputs_THW.shape[-2:]).cpu().numpy()
    out.astype(np.dtype(dataset_metadata.get("token_dtype", "uint32"))).tofile(output_dir / "video.bin")
    side = int(out.shape[-1])
    meta = dict(args) | dict(dataset_metadata) | {"num_images": int(out.shape[0]), "h": side, "w": side,
                                                   "t": int(args.get("window_size", 16))}
    with open(output_dir / "metadata.json", "w") as f:
        json.dump(meta, f)
    return meta
