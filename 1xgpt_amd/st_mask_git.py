"""STMaskGIT -- the GENIE world model (embed -> ST transformer -> factored readout) and its MaskGIT decoder.

Drop-in for the reference's ``genie.st_mask_git.STMaskGIT`` (st_mask_git.py:29-313): same constructor,
attributes (``mask_token_id``, ``config``, ``h``, ``w``), state-dict keys and methods
(``compute_logits``, ``forward``, ``compute_loss_and_acc``, ``maskgit_generate``, ``generate``,
``init_weights``, ``from_pretrained``/``save_pretrained``).  All arithmetic runs in libgenie_hip.so
(hand-written gfx950 kernels) on the module's device; PyTorch only owns the buffers and the stream.
There is no CPU fallback: calling a method with CPU tensors raises.

Differences that are deliberate and visible:
  * ``maskgit_generate`` takes two optional extras, ``noise`` (the U[0,1) draws the reference takes from
    ``torch.rand_like``, :206) and ``uniforms`` (for temperature > 0), so a test can replay an exact stream.
  * ``precision``: "exact" (f32 MFMA), "f16x3" (split-f16 operands on the f16 matrix cores, f32-class
    results: the parity-grade fast mode) or "bf16" (bf16 MFMA operands, f32 accumulate: throughput mode).
  * per-frame action conditioning (not in the reference): with ``config.action_vocab_size = A > 0`` the model has an
    ``action_embed`` table (A, d_model) and every entry point takes ``action_ids`` (B, T): row ``action_ids[b, t]`` is
    added to every token of frame t of clip b, next to the positional embedding.
  * continuous per-frame actions (not in the reference): with ``config.action_dim = A > 0`` the model has a learned
    ``action_proj`` Linear(A, d_model), a learned ``action_null`` row and the buffers ``action_mean`` / ``action_std``; every entry
    point takes ``action_vectors`` (B, T, A) float32, projected once per call (genie_action_rows) into a row table that the same
    per-frame conditioning then addresses by index.
  * classifier-free guidance (not in the reference): ``maskgit_generate`` / ``generate`` take ``guidance=Guidance(scale, null_action)``.
"""
import json
import math
import os

import torch
import torch.nn as nn

from . import _lib
from .config import GenieConfig
from .factorization_utils import FactorizedEmbedding
from .sampling import SamplingConfig, as_struct, guidance_struct, unmask_code
from .st_transformer import STTransformerDecoder

_PRECISIONS = {"exact": _lib.PREC_EXACT, "f32": _lib.PREC_EXACT, "bf16": _lib.PREC_BF16, "fast": _lib.PREC_BF16,
               "f16x3": _lib.PREC_F16X3}


def cosine_schedule(u):
    """Fraction of tokens still masked after a share ``u`` of the MaskGIT steps: cos(pi u / 2), for a Python float
    (the decoder's own use) or a tensor; anything else is refused like the reference does (st_mask_git.py:17-26)."""
    if isinstance(u, float):
        return math.cos(0.5 * math.pi * u)
    if isinstance(u, torch.Tensor):
        return torch.cos(u * (0.5 * torch.pi))
    raise NotImplementedError(f"Unexpected {type(u)=} {u=}")


class _Packer:
    """16-bit copies of the Linear weights in the layout the kernels of one precision read, made once per weight table.

    ``packer(weight)`` returns the device pointer of the packed copy (bf16, or the [hi | lo] f16 planes of f16x3);
    ``is_wide(ptr)`` tells whether that f16x3 tensor breaks the |w| < 32 range contract of the fast split GEMM (the caller
    writes the answer into the ``w16_wide`` field next to the pointer: the flag travels with the table, the library keeps no
    registry); ``temporal_fused`` / ``mlp_fused`` build the fragment streams of the fused sub-block kernels
    (csrc/kernels_fused.hip) for the geometry they cover and return 0 otherwise."""

    def __init__(self, lib, prec, dev, config):
        self.lib, self.prec, self.dev, self.config = lib, prec, dev, config
        self.keep, self.wide = [], set()

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def __call__(self, wt):
        if self.prec == _lib.PREC_BF16:
            t = torch.empty(wt.shape, dtype=torch.bfloat16, device=self.dev)
            _lib.check(self.lib.genie_pack_bf16(wt.data_ptr(), t.data_ptr(), wt.numel(), self._stream()), "genie_pack_bf16")
        else:  # f16x3: [hi plane | lo plane], wt ~ hi + lo / 2048
            t = torch.empty((2,) + tuple(wt.shape), dtype=torch.float16, device=self.dev)
            _lib.check(self.lib.genie_pack_split_f16(wt.data_ptr(), t.data_ptr(), wt.numel(), self._stream()),
                       "genie_pack_split_f16")
            # Range contract, checked on the packed hi plane at load time.  Beyond the f16 range the precision cannot represent
            # the tensor at all; from 32 up the 256x256 GEMM's 2^11 scaling of the hi plane would overflow, so the tensor is
            # flagged and its Linear runs on the two-accumulator kernels (same f32-class result, slower for that tensor only).
            if not bool(torch.isfinite(t[0]).all()):
                raise ValueError("f16x3 precision needs finite |weight| < 65504 (the f16 range of the split's hi plane); this "
                                 "checkpoint has a larger or non-finite weight -- use precision='exact' or 'bf16'")
            if float(t[0].abs().max()) >= 31.98:
                import warnings
                self.wide.add(t.data_ptr())
                warnings.warn(f"f16x3: a weight tensor of shape {tuple(wt.shape)} has |w| >= 32 (max {float(wt.abs().max()):.3g}): "
                              "its Linear runs on the two-accumulator split GEMM instead of the 256x256 kernel (same results, "
                              "lower throughput for that layer)")
        self.keep.append(t)
        return t.data_ptr()

    def is_wide(self, ptr):
        return ptr in self.wide

    def _fused_geometry(self):
        c = self.config
        return (self.prec == _lib.PREC_BF16 and c.d_model == 256 and c.num_heads == 8 and not c.qk_norm
                and os.environ.get("GENIE_NO_FUSED", "0") != "1")

    def temporal_fused(self, attn):
        c = self.config
        if (self.prec == _lib.PREC_F16X3 and c.d_model == 256 and c.num_heads == 8 and not c.qk_norm and c.T <= 16
                and os.environ.get("GENIE_NO_FUSED", "0") != "1"):
            # f16x3: the temporal qkv Linear + attention run as one kernel (csrc/kernels_fused_f16x3.hip) on this split-f16 stream
            t = torch.empty(_lib.TEMPORAL_QKV_F16X3_ELEMS, dtype=torch.float16, device=self.dev)
            _lib.check(self.lib.genie_pack_temporal_qkv_f16x3(attn.qkv.weight.data_ptr(), t.data_ptr(), self._stream()),
                       "genie_pack_temporal_qkv_f16x3")
            self.keep.append(t)
            return t.data_ptr()
        if not (self._fused_geometry() and self.config.T == 16):
            return 0
        t = torch.empty(_lib.TEMPORAL_FUSED_ELEMS, dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.lib.genie_pack_temporal_fused_bf16(attn.qkv.weight.data_ptr(), attn.proj.weight.data_ptr(), t.data_ptr(),
                                                           self._stream()), "genie_pack_temporal_fused_bf16")
        self.keep.append(t)
        return t.data_ptr()

    def spatial_fused(self, attn):
        if not (self._fused_geometry() and self.config.S == 256):
            return 0
        # [out-projection stream | qkv stream]: the second part lets the previous block's fused MLP kernel write this block's operand planes
        t = torch.empty(_lib.SPATIAL_PROJ_FUSED_ELEMS + _lib.SPATIAL_QKV_FUSED_ELEMS, dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.lib.genie_pack_spatial_proj_fused_bf16(attn.proj.weight.data_ptr(), t.data_ptr(), self._stream()),
                   "genie_pack_spatial_proj_fused_bf16")
        _lib.check(self.lib.genie_pack_spatial_qkv_fused_bf16(attn.qkv.weight.data_ptr(), t.data_ptr() + 2 * _lib.SPATIAL_PROJ_FUSED_ELEMS,
                                                              self._stream()), "genie_pack_spatial_qkv_fused_bf16")
        self.keep.append(t)
        return t.data_ptr()

    def _frame_geometry(self):
        # the fragment-order kernels of the one-frame passes (csrc/kernels_frame.hip): f16x3, LayerNorm or qk-norm blocks, heads of 64 or 32
        c = self.config
        return (self.prec == _lib.PREC_F16X3 and c.S == 256 and c.d_model in (128, 256, 512)
                and c.d_model in (64 * c.num_heads, 32 * c.num_heads) and os.environ.get("GENIE_NO_FRAME_KERNELS", "0") != "1")

    def frame_stream(self, *weights):
        """The given Linear weights back to back as split f16 in fragment order (genie_pack_frame_w16), or 0."""
        if not self._frame_geometry() or any(w.shape[0] % 64 or w.shape[1] % 64 for w in weights):
            return 0   # (output widths in 64-column tiles -- no tail handling in gemm16_fr --, contraction in 64-k blocks)
        t = torch.empty(sum(2 * w.numel() for w in weights), dtype=torch.float16, device=self.dev)
        off = 0
        for w in weights:
            _lib.check(self.lib.genie_pack_frame_w16(w.data_ptr(), t.data_ptr() + 2 * off, w.shape[0], w.shape[1], self._stream()),
                       "genie_pack_frame_w16")
            off += 2 * w.numel()
        self.keep.append(t)
        return t.data_ptr()

    def mlp_fused(self, mlp):
        if not (self._fused_geometry() and mlp.fc1.weight.shape[0] == 1024):
            return 0
        t = torch.empty(_lib.MLP_FUSED_ELEMS, dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.lib.genie_pack_mlp_fused_bf16(mlp.fc1.weight.data_ptr(), mlp.fc2.weight.data_ptr(), t.data_ptr(),
                                                      self._stream()), "genie_pack_mlp_fused_bf16")
        self.keep.append(t)
        return t.data_ptr()


class GenieOutput(dict):
    """Minimal stand-in for transformers' ModelOutput: attribute and key access to loss / acc / logits."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class STMaskGIT(nn.Module):
    def __init__(self, config: GenieConfig, precision: str = "exact"):
        super().__init__()
        self.h = self.w = math.isqrt(config.S)
        assert self.h ** 2 == config.S, "Expected S to be square"
        self.decoder = STTransformerDecoder(
            num_layers=config.num_layers, num_heads=config.num_heads, d_model=config.d_model,
            qkv_bias=config.qkv_bias, proj_bias=config.proj_bias, qk_norm=config.qk_norm, use_mup=config.use_mup,
            attn_drop=config.attn_drop, mlp_ratio=config.mlp_ratio, mlp_bias=config.mlp_bias,
            mlp_drop=config.mlp_drop)
        self.pos_embed_TSC = nn.Parameter(torch.zeros(1, config.T, config.S, config.d_model))
        self.mask_token_id = config.image_vocab_size
        self.token_embed = FactorizedEmbedding(
            factored_vocab_size=config.factored_vocab_size, num_factored_vocabs=config.num_factored_vocabs,
            d_model=config.d_model, mask_token_id=self.mask_token_id)
        # nn.Linear holds the readout parameters for both the plain and the muP readout; the muP factor
        # output_mult/width_mult (reference :316-323) is applied inside the readout GEMM (cfg.readout_mult).
        self.out_x_proj = nn.Linear(config.d_model, config.factored_vocab_size * config.num_factored_vocabs)
        if config.action_vocab_size:
            self.action_embed = nn.Embedding(config.action_vocab_size, config.d_model)
        if config.action_dim:
            if config.action_dim > _lib.ACTION_MAX_DIM:
                raise ValueError(f"action_dim {config.action_dim} > {_lib.ACTION_MAX_DIM} (GENIE_ACTION_MAX_DIM)")
            self.action_proj = nn.Linear(config.action_dim, config.d_model)
            self.action_null = nn.Parameter(torch.zeros(config.d_model))   # the learned "no action" row (guidance, action dropout)
            self.register_buffer("action_mean", torch.zeros(config.action_dim))
            self.register_buffer("action_std", torch.ones(config.action_dim))
        self._inv_std = self._rows = None
        self._row_ids = {}
        self.config = config
        self._table = None
        self._wide = []
        self.set_precision(precision)
        self._ws = None
        self.requires_grad_(False)

    # ------------------------------------------------------------------ plumbing
    def set_precision(self, precision: str):
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self._prec = _PRECISIONS[precision]
        self._invalidate()
        return self

    def _apply(self, fn, *a, **k):  # .to()/.cuda()/.float() move parameters: cached pointers are stale
        self._invalidate()
        self._ws = self._inv_std = self._rows = None
        self._row_ids = {}
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._invalidate()
        self._inv_std = None
        return super().load_state_dict(*a, **k)

    def _device(self):
        dev = self.pos_embed_TSC.device
        if dev.type != "cuda":
            raise RuntimeError("1xgpt_amd.STMaskGIT runs on the GPU only (no CPU fallback): call .to('cuda') first")
        return dev

    def refresh_weights(self):
        """Rebuild the device pointer table (and bf16 copies).  Call after mutating parameters in place."""
        self._invalidate()

    def _invalidate(self):
        """Forget the cached pointer table (packed copies, fused streams and range flags go with it)."""
        self._table = None
        self._wide = []
        self._null_row_set = False   # row 0 of the cached action-row table is a copy of action_null

    def _weights(self):
        if self._table is not None:
            return self._table
        dev = self._device()
        lib = _lib.load()
        for n, p in self.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"parameter {n} must be contiguous float32 (got {p.dtype})")
        cfg = _lib.make_cfg(self.config, self._prec)
        _lib.check(lib.genie_check_config(cfg), "genie_check_config")
        packed = _Packer(lib, self._prec, dev, self.config) if self._prec != _lib.PREC_EXACT else None
        L = self.config.num_layers
        layers = (_lib.LayerWeights * L)(*[blk.layer_struct(packed) for blk in self.decoder.layers])
        w = _lib.Weights()
        w.pos_embed = self.pos_embed_TSC.data_ptr()
        w.mask_embed = self.token_embed.mask_token_embed.data_ptr()
        for j, e in enumerate(self.token_embed.factored_embeds):
            w.embed[j] = e.weight.data_ptr()
        w.out_w, w.out_b = self.out_x_proj.weight.data_ptr(), self.out_x_proj.bias.data_ptr()
        if packed is not None:
            w.out_w16 = packed(self.out_x_proj.weight)
            w.out_w16_wide = int(packed.is_wide(w.out_w16))
            w.out_frame_w16 = packed.frame_stream(self.out_x_proj.weight)
        w.layers_host = layers
        self._table = (cfg, w, layers, packed)
        self._wide = sorted(packed.wide) if packed is not None else []
        return self._table

    def _workspace(self, B, generate_prompt_frames=0, guided=False, rollout_ctx=0):
        """The model's workspace for B clips; generate_prompt_frames = P > 0: large enough for genie_generate_cached with P prompt frames too;
        guided: for the guided loops on B clips (their passes run 2 B); rollout_ctx > 0: for genie_rollout_cached with contexts up to
        that many frames too."""
        cfg = self._weights()[0]
        need = _lib.load().genie_workspace_bytes(cfg, B)
        if rollout_ctx:
            need = max(need, _lib.load().genie_rollout_workspace_bytes(cfg, B, rollout_ctx, int(guided)))
        if guided:
            need = max(need, _lib.load().genie_generate_guided_workspace_bytes(cfg, B, generate_prompt_frames or 1))
        elif generate_prompt_frames:
            need = max(need, _lib.load().genie_generate_workspace_bytes(cfg, B, generate_prompt_frames))
        if self._ws is None or self._ws.numel() < need or self._ws.device != self._device():
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._device())
        return self._ws

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _cond(self, action_ids, B, n_frames=None, action_vectors=None):
        """The genie_frame_cond of a call on B clips (None for an unconditioned model), checked on the host before anything
        is enqueued.  action_ids: (B, T) integers in [0, A); (B, n_frames) with n_frames < T is padded to T (frames the
        call never embeds).  action_vectors: (B, T, action_dim) floats of a model with config.action_dim > 0, padded alike."""
        A, T = self.config.action_vocab_size, self.config.T
        if action_ids is not None and action_vectors is not None:
            raise ValueError("pass action_ids or action_vectors, not both")
        if self.config.action_dim:
            if action_ids is not None:
                raise ValueError(f"action_ids given to a model conditioned on action vectors (action_dim={self.config.action_dim}): "
                                 "pass action_vectors")
            return self._cond_vectors(action_vectors, B, n_frames)
        if action_vectors is not None:
            raise ValueError("action_vectors given to a model without continuous actions (config.action_dim == 0)")
        if not A:
            if action_ids is not None:
                raise ValueError("action_ids given to a model without actions (config.action_vocab_size == 0)")
            return None
        if action_ids is None:
            raise ValueError(f"this model is action-conditioned (action_vocab_size={A}): pass action_ids (B, T)")
        a = torch.as_tensor(action_ids)
        if a.dtype.is_floating_point or a.dtype == torch.bool:
            raise RuntimeError(f"action_ids must be an integer tensor, got {a.dtype}")
        n = T if n_frames is None else n_frames
        if a.dim() != 2 or a.shape[0] != B or a.shape[1] not in (n, T):
            raise RuntimeError(f"expected action_ids of shape ({B}, {T}), got {tuple(a.shape)}")
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= A):
            raise IndexError(f"action id out of range [0, {A}): min {int(a.min())}, max {int(a.max())}")
        a = a.to(device=self._device(), dtype=torch.int64)
        if a.shape[1] < T:
            a = torch.cat([a, a.new_zeros(B, T - a.shape[1])], dim=1)
        a = a.contiguous()
        return self._frame_cond(a)

    def _check_cond(self, action_ids, B, action_vectors=None, n_frames=None):
        """The host-side checks of _cond alone: raises what _cond would raise, enqueues nothing."""
        if self.config.action_dim and action_ids is None and action_vectors is not None:
            T = self.config.T
            self.check_action_vectors(action_vectors, (B, (T if n_frames is None else n_frames, T), self.config.action_dim))
        else:
            self._cond(action_ids, B, n_frames=n_frames, action_vectors=action_vectors)

    def _frame_cond(self, a, like=None):
        """genie_frame_cond of checked, contiguous int64 device ids (rows, T): over the model's action table, or over the
        table of the genie_frame_cond `like` (the per-call row table of a model conditioned on action vectors)."""
        if like is not None:
            fc = _lib.FrameCond(table=like.table, ids=a.data_ptr(), n_actions=like.n_actions)
            fc.rows = getattr(like, "rows", None)
        else:
            fc = _lib.FrameCond(table=self.action_embed.weight.data_ptr(), ids=a.data_ptr(), n_actions=self.config.action_vocab_size)
        fc.keep = a   # the ids tensor lives as long as the struct
        return fc

    # ---- continuous actions: project once per call, then the discrete path (genie_action_proj in include/genie_hip.h)
    NULL_ROW = 0   # index of the learned null row in every per-call row table

    def set_action_stats(self, mean, std):
        """The input normalisation z = (a - mean) / std of the action vectors: (action_dim,) each, std > 0."""
        D = self.config.action_dim
        if not D:
            raise ValueError("set_action_stats: this model has no continuous actions (config.action_dim == 0)")
        mean = torch.as_tensor(mean, dtype=torch.float32).reshape(-1).cpu()
        std = torch.as_tensor(std, dtype=torch.float32).reshape(-1).cpu()
        if mean.numel() != D or std.numel() != D:
            raise ValueError(f"set_action_stats: expected {D} means and {D} stds, got {mean.numel()} and {std.numel()}")
        if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all()) and bool((std > 0).all())):
            raise ValueError("set_action_stats: mean must be finite and std finite and > 0")
        with torch.no_grad():
            self.action_mean.copy_(mean)
            self.action_std.copy_(std)
        self._inv_std = None
        return self

    def check_action_vectors(self, action_vectors, shape, what="action_vectors"):
        """Host-side checks of a float action tensor against `shape` (its last entry is action_dim; an entry that is a tuple allows
        any of its members) -> contiguous float32 on the model's device.  Nothing is enqueued before a check fails."""
        if action_vectors is None:
            raise ValueError(f"this model is conditioned on action vectors (action_dim={self.config.action_dim}): pass {what} "
                             f"{tuple(shape)}")
        v = torch.as_tensor(action_vectors)
        if not v.dtype.is_floating_point:
            raise RuntimeError(f"{what} must be a floating-point tensor, got {v.dtype}")
        ok = v.dim() == len(shape) and all(g in e if isinstance(e, tuple) else g == e for g, e in zip(v.shape, shape))
        if not ok:
            raise RuntimeError(f"expected {what} of shape {tuple(shape)}, got {tuple(v.shape)}")
        if not bool(torch.isfinite(v).all()):
            raise ValueError(f"{what} holds a non-finite entry")
        return v.to(device=self._device(), dtype=torch.float32).contiguous()

    def _action_proj_struct(self):
        """The genie_action_proj over the parameters as they are now (pointers are read per call: a trainer re-points them)."""
        if self._inv_std is None:   # 1 / std in f32 on the host (one read-back per set_action_stats / load / move)
            import numpy as np
            std = self.action_std.detach().cpu().numpy().astype(np.float32)
            self._inv_std = torch.from_numpy(np.float32(1.0) / std).to(self._device())
        p = _lib.ActionProj(weight=self.action_proj.weight.data_ptr(), bias=self.action_proj.bias.data_ptr(),
                            mean=self.action_mean.data_ptr(), inv_std=self._inv_std.data_ptr(), action_dim=self.config.action_dim)
        return p

    def project_actions(self, vecs_nA, rows_nd):
        """rows_nd (n, d_model) <- the projection of vecs_nA (n, action_dim), both contiguous f32 on the device: ONE launch."""
        n = vecs_nA.shape[0]
        assert vecs_nA.is_contiguous() and rows_nd.is_contiguous() and rows_nd.shape == (n, self.config.d_model)
        for nm, t in (("action_proj.weight", self.action_proj.weight), ("action_proj.bias", self.action_proj.bias)):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"parameter {nm} must be contiguous float32 (got {t.dtype})")
        _lib.check(_lib.load().genie_action_rows(self._action_proj_struct(), vecs_nA.data_ptr(), rows_nd.data_ptr(), n,
                                                 self.config.d_model, self._stream()), "genie_action_rows")

    def new_row_table(self, n_rows):
        """A (1 + n_rows, d_model) row table whose row NULL_ROW is a copy of action_null (the others are the caller's to project)."""
        t = torch.empty(1 + n_rows, self.config.d_model, dtype=torch.float32, device=self._device())
        t[self.NULL_ROW].copy_(self.action_null.detach())
        return t

    def _cond_vectors(self, action_vectors, B, n_frames=None):
        """genie_frame_cond of (B, T, action_dim) vectors: ONE genie_action_rows launch into the cached (1 + B T, d) table -- row 0
        the null row, row 1 + b T + t frame (b, t) -- and the ids that address it."""
        T, D = self.config.T, self.config.action_dim
        n = T if n_frames is None else n_frames
        v = self.check_action_vectors(action_vectors, (B, (n, T), D))
        if v.shape[1] < T:   # frames the call never embeds
            v = torch.cat([v, v.new_zeros(B, T - v.shape[1], D)], dim=1).contiguous()
        if self._rows is None or self._rows.shape[0] < 1 + B * T or self._rows.device != v.device:
            self._rows, self._null_row_set = self.new_row_table(B * T), True
        elif not self._null_row_set:
            self._rows[self.NULL_ROW].copy_(self.action_null.detach())
            self._null_row_set = True
        self.project_actions(v.view(B * T, D), self._rows[1:1 + B * T])
        ids = self._row_ids.get(B)
        if ids is None or ids.device != v.device:
            ids = self._row_ids[B] = torch.arange(1, 1 + B * T, dtype=torch.int64, device=v.device).view(B, T)
        fc = _lib.FrameCond(table=self._rows.data_ptr(), ids=ids.data_ptr(), n_actions=1 + B * T)
        fc.keep, fc.rows, fc.vectors = ids, self._rows, v
        return fc

    def _guidance(self, guidance):
        """The genie_guidance of a call (None = unguided), checked on the host: a model without actions raises, like action_ids does."""
        if self.config.action_dim:   # the model supplies the null row's index
            return guidance_struct(guidance, null_row=self.NULL_ROW)
        return guidance_struct(guidance, self.config.action_vocab_size)

    def _ids(self, t, whole_clips=False):
        if not t.is_cuda:
            raise RuntimeError("1xgpt_amd runs on the GPU only (no CPU fallback): move inputs to cuda")
        if whole_clips and (t.dim() < 2 or t.numel() != t.shape[0] * self.config.T * self.config.S):
            # (the reference fails on such an input too -- the positional table does not broadcast, st_mask_git.py:261 --; the
            # library takes B from dim 0 and would read past the tensor)
            raise RuntimeError(f"expected token ids of {self.config.T} frames x {self.config.S} tokens per clip (B, T, H, W) / "
                               f"(B, T*S), got {tuple(t.shape)}")
        return t.to(torch.int64).contiguous()

    # ------------------------------------------------------------------ forward pieces
    def hidden_states(self, x_THW: torch.LongTensor, action_ids=None, action_vectors=None):
        """Run embed + decoder; the (B,T,S,d) result stays at offset 0 of the workspace (returned as a view)."""
        lib = _lib.load()
        cfg, w = self._weights()[:2]
        ids = self._ids(x_THW, whole_clips=True)
        B = ids.shape[0]
        cond = self._cond(action_ids, B, action_vectors=action_vectors)
        ws = self._workspace(B)
        _lib.check(_lib.call_cond(lib, "genie_compute_logits", cond, cfg, w, ids.data_ptr(), B, 0, 0, 0, ws.data_ptr(),
                                  ws.data_ptr(), ws.numel(), self._stream()), "genie_compute_logits(hidden)")
        n = B * self.config.T * self.config.S * self.config.d_model
        return ws[: n * 4].view(torch.float32).view(B, self.config.T, self.config.S, self.config.d_model)

    def compute_logits_frames(self, x_THW, t0, t1, layout="bcthw", action_ids=None, action_vectors=None, out=None, cond=None):
        """Logits of frames [t0,t1): (B, V, t1-t0, H, W) for layout='bcthw', (B, t1-t0, S, V) for 'token'.
        out: a contiguous f32 tensor of that many elements on the device to write into (and return) instead of a new one.
        cond: a genie_frame_cond the caller built from this model (`_cond` / `_frame_cond`), used instead of action_ids / action_vectors."""
        lib = _lib.load()
        cfg, w = self._weights()[:2]
        ids = self._ids(x_THW, whole_clips=True)
        B = ids.shape[0]
        if cond is None:
            cond = self._cond(action_ids, B, action_vectors=action_vectors)
        ws = self._workspace(B)
        nt, V = t1 - t0, self.config.factored_vocab_size * self.config.num_factored_vocabs
        shape = (B, V, nt, self.h, self.w) if layout == "bcthw" else (B, nt, self.config.S, V)
        lay = _lib.LAYOUT_BCTHW if layout == "bcthw" else _lib.LAYOUT_TOKEN_MAJOR
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=ids.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == math.prod(shape)):
            raise RuntimeError(f"compute_logits_frames: out must be a contiguous float32 device tensor of {math.prod(shape)} elements")
        else:
            out = out.view(shape)
        _lib.check(_lib.call_cond(lib, "genie_compute_logits", cond, cfg, w, ids.data_ptr(), B, t0, t1, lay, out.data_ptr(),
                                  ws.data_ptr(), ws.numel(), self._stream()), "genie_compute_logits")
        return out

    def compute_logits(self, x_THW, action_ids=None, action_vectors=None):
        """ids (B,T,H,W) -> logits (B, V, T, H, W), channels [vocab0(512) | vocab1(512)]  (reference :255-265)."""
        return self.compute_logits_frames(x_THW, 0, self.config.T, "bcthw", action_ids=action_ids, action_vectors=action_vectors)

    def ce_sums(self, x_THW, labels_THW, t0=1, t1=None, masked_only=True, action_ids=None, action_vectors=None):
        """Fused forward + readout + factored CE: returns a (3,) float64 device tensor
        [sum CE, sum all-factors-correct, n counted] over frames [t0,t1); no logits leave the workspace."""
        lib = _lib.load()
        cfg, w = self._weights()[:2]
        ids, lab = self._ids(x_THW, whole_clips=True), self._ids(labels_THW, whole_clips=True)
        B = ids.shape[0]
        t1 = self.config.T if t1 is None else t1
        self._check_cond(action_ids, B, action_vectors)   # (argument errors before anything is enqueued)
        ws = self._workspace(B)
        self.hidden_states(ids, action_ids=action_ids, action_vectors=action_vectors)
        sums = torch.zeros(3, dtype=torch.float64, device=ids.device)
        _lib.check(lib.genie_readout_ce(cfg, w, ws.data_ptr(), lab.data_ptr(), ids.data_ptr() if masked_only else 0,
                                        B, t0, t1, sums.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "genie_readout_ce")
        return sums

    def compute_loss_and_acc(self, logits_CTHW, targets_THW, relevant_mask_THW):
        """Masked mean of the summed factored CE and of 'all factors argmax-correct' (reference :231-253)."""
        lib = _lib.load()
        cfg = self._weights()[0]
        B, T = targets_THW.shape[0], self.config.T
        lg = logits_CTHW[:, :, 1:].contiguous().float()
        tg = self._ids(targets_THW).view(B, T, -1)
        wid = torch.zeros_like(tg)
        wid[:, 1:] = torch.where(relevant_mask_THW.reshape(B, T - 1, -1).bool(), self.mask_token_id, 0)
        sums = torch.zeros(3, dtype=torch.float64, device=lg.device)
        _lib.check(lib.genie_factored_ce(cfg, lg.data_ptr(), _lib.LAYOUT_BCTHW, tg.data_ptr(), wid.data_ptr(), B, 1, T,
                                         sums.data_ptr(), self._stream()), "genie_factored_ce")
        return (sums[0] / sums[2]).float(), (sums[1] / sums[2]).float()  # 0/0 -> nan like the reference

    def forward(self, input_ids, labels, action_ids=None, action_vectors=None):
        """(B, T*H*W) ids + labels -> GenieOutput(loss, acc, logits (B,V,T,H,W))  (reference :267-279)."""
        T, H, W = self.config.T, self.h, self.w
        x_THW = self._ids(input_ids).view(-1, T, H, W)
        lab = self._ids(labels).view(-1, T, H, W)
        if lab.shape != x_THW.shape:
            raise RuntimeError(f"labels {tuple(labels.shape)} do not match input_ids {tuple(input_ids.shape)}")
        self._check_cond(action_ids, x_THW.shape[0], action_vectors)
        logits = self.compute_logits(x_THW, action_ids=action_ids, action_vectors=action_vectors)  # leaves the hidden state in the workspace
        lib = _lib.load()
        cfg, w = self._weights()[:2]
        B = x_THW.shape[0]
        ws = self._workspace(B)
        sums = torch.zeros(3, dtype=torch.float64, device=x_THW.device)
        _lib.check(lib.genie_readout_ce(cfg, w, ws.data_ptr(), lab.data_ptr(), x_THW.data_ptr(), B, 1, T,
                                        sums.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "genie_readout_ce")
        loss, acc = (sums[0] / sums[2]).float(), (sums[1] / sums[2]).float()
        return GenieOutput(loss=loss, acc=acc, logits=logits)

    # ------------------------------------------------------------------ MaskGIT
    @staticmethod
    def init_mask(prompt_THW):
        H, W = prompt_THW.size(2), prompt_THW.size(3)
        return torch.zeros(prompt_THW.size(0), H * W, dtype=torch.bool, device=prompt_THW.device)

    @torch.no_grad()
    def maskgit_generate(self, prompt_THW, out_t, maskgit_steps=1, temperature=0.0, unmask_mode="random",
                         noise=None, uniforms=None, return_logits=True, check=True, action_ids=None, sampling=None, guidance=None,
                         action_vectors=None, known=None):
        """MaskGIT decode of frame ``out_t`` (reference :123-229): the whole loop runs on the device.

        Mutates ``prompt_THW[:, out_t]`` in place (reference :223) and returns
        ``(samples (B,H,W) int64, step-0 factored logits (B, 512, 2, H, W))``.
        noise: optional (maskgit_steps-1, B, S) float32 draws for "random" unmasking (default: torch.rand).
        uniforms: (maskgit_steps, num_factored_vocabs, B, S) for temperature > 1e-8 (default: torch.rand).
        action_ids: (B, T) actions of an action-conditioned model (config.action_vocab_size > 0), else None.
        action_vectors: (B, T, action_dim) float actions of a model with config.action_dim > 0, else None; there ``Guidance(scale)``
        needs no null_action (the model's learned null row is used).
        sampling: a ``SamplingConfig`` (logit temperature, top-k, top-p; 1xgpt_amd/sampling.py) or None = the reference's law.
        unmask_mode "confidence" (no reference counterpart) re-masks by confidence plus annealed Gumbel noise, drawn from ``noise``.
        guidance: a ``Guidance(scale, null_action)`` (1xgpt_amd/sampling.py) or None: classifier-free guidance of an action-conditioned
        model -- every forward runs the clips twice, under their actions and under the null action, and the law is applied to
        scale * conditional + (1 - scale) * null; the returned step-0 logits are the guided ones.
        known: optional (B, H, W) int64 known tokens of the frame (generate.known_tokens): a value in [0, image_vocab_size) is kept,
        ``mask_token_id`` (any other value) is generated.  The prompt's frame ``out_t`` is still passed all-mask; each clip re-masks by
        its own count of tokens left to generate; the step-0 logits at known positions are the model's logits there, as for any
        unmasked input token.  The reference has no counterpart (it asserts an all-mask frame, st_mask_git.py:155).
        """
        mode = unmask_code(unmask_mode)
        law = as_struct(sampling)
        guide = self._guidance(guidance)
        assert out_t, "maskgit_generate requires out_t > 0"
        lib = _lib.load()
        cfg, w = self._weights()[:2]
        if not prompt_THW.is_cuda:
            raise RuntimeError("1xgpt_amd runs on the GPU only (no CPU fallback): move inputs to cuda")
        in_place = prompt_THW.dtype == torch.int64 and prompt_THW.is_contiguous()
        prompt = prompt_THW if in_place else prompt_THW.to(torch.int64).contiguous()
        B, T = prompt.shape[0], prompt.shape[1]
        if T != self.config.T or prompt.numel() != B * T * self.config.S:
            # (the reference fails here too: `x_TSC + self.pos_embed_TSC` does not broadcast, st_mask_git.py:261; the library would
            # read past the tensor)
            raise RuntimeError(f"maskgit_generate expects a (B, T={self.config.T}, H, W) prompt, got {tuple(prompt_THW.shape)}")
        S, V = self.config.S, self.config.factored_vocab_size * self.config.num_factored_vocabs
        dev = prompt.device
        from .generate import check_known
        known = check_known(known, (B, self.h, self.w), dev)
        cond = self._cond(action_ids, B, action_vectors=action_vectors)
        ws = self._workspace(B, guided=guide is not None)
        if unmask_mode != "greedy" and maskgit_steps > 1:
            if noise is None:
                noise = torch.rand(maskgit_steps - 1, B, S, dtype=torch.float32, device=dev)
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            assert noise.numel() == (maskgit_steps - 1) * B * S, "noise must be (maskgit_steps-1, B, S)"
        else:
            noise = None
        if temperature > 1e-8:
            if uniforms is None:
                uniforms = torch.rand(maskgit_steps, self.config.num_factored_vocabs, B, S, device=dev)
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        else:
            uniforms = None
        samples = torch.empty(B, self.h, self.w, dtype=torch.int64, device=dev)
        logits0 = torch.empty(B, V, self.h, self.w, dtype=torch.float32, device=dev) if return_logits else None
        status = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
        if mode == _lib.UNMASK_CONFIDENCE and law is None:
            law = as_struct(SamplingConfig())
        rc = _lib.call_known(
            lib, "genie_maskgit_generate", cond, law, guide, _lib.make_known(known, 1, S), cfg, w, prompt.data_ptr(), B, int(out_t), int(maskgit_steps), float(temperature),
            mode,
            0 if noise is None else noise.data_ptr(), 0 if uniforms is None else uniforms.data_ptr(),
            samples.data_ptr(), 0 if logits0 is None else logits0.data_ptr(), _lib.LAYOUT_BCTHW,
            0 if status is None else status.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(rc, "genie_maskgit_generate")
        if check and int(status.item()) != 0:  # host sync, like the reference's assert torch.all(...) (:155)
            raise AssertionError(f"when generating z{out_t}, frames {out_t} and later must be masked")
        if not in_place:
            prompt_THW.copy_(prompt.view_as(prompt_THW))
        if logits0 is None:
            return samples, None
        nv, vf = self.config.num_factored_vocabs, self.config.factored_vocab_size
        # "B (num_vocabs vocab_size) H W -> B vocab_size num_vocabs H W"  (reference :226-229)
        return samples, logits0.view(B, nv, vf, self.h, self.w).permute(0, 2, 1, 3, 4)

    def generate(self, input_ids, attention_mask=None, max_new_tokens=None, min_new_tokens=None, return_logits=False,
                 maskgit_steps=1, temperature=0.0, noise=None, kv_cache=True, action_ids=None, sampling=None,
                 unmask_mode="random", uniforms=None, guidance=None, action_vectors=None):
        """Autoregressive frame generation behind the reference's Llama-style signature (st_mask_git.py:65-113):
        ``input_ids`` (B, n_prompt_frames * S) holds the prompt frames; ``max_new_tokens // S`` further frames are decoded one
        after the other with ``maskgit_generate``, each seeing every frame before it.  Returns the (B, (n_prompt + n_new) * S)
        token ids, plus -- with ``return_logits`` -- the step-0 factored logits of the new frames stacked on dim 3.
        ``attention_mask`` is accepted and ignored, as in the reference.  ``min_new_tokens`` may only repeat ``max_new_tokens``.
        noise: optional (n_new_frames, maskgit_steps - 1, B, S) unmasking draws to replay (the reference draws them itself).
        kv_cache: True (default) = the frames are decoded by one-frame passes against a temporal KV cache; False = the reference's
        own schedule, a full forward over the canvas per MaskGIT step (same frames up to f32 accumulation order).
        action_ids: (B, T) -- or (B, n_prompt + n_new), padded to T -- actions of an action-conditioned model.
        action_vectors: (B, T, action_dim) -- or (B, n_prompt + n_new, action_dim) -- float actions of a model with config.action_dim > 0.
        sampling / unmask_mode: as in ``maskgit_generate`` (the reference's generate always unmasks at random).
        uniforms: optional (n_new_frames, maskgit_steps, num_factored_vocabs, B, S) sampling draws to replay (temperature > 1e-8).
        guidance: as in ``maskgit_generate``; with ``return_logits`` the step-0 logits are the guided ones."""
        mode = unmask_code(unmask_mode)
        law = as_struct(sampling)
        guide = self._guidance(guidance)
        if mode == _lib.UNMASK_CONFIDENCE and law is None:
            law = as_struct(SamplingConfig())
        S = self.config.S
        if min_new_tokens is not None and min_new_tokens != max_new_tokens:
            raise AssertionError("Expecting `min_new_tokens`, if specified, to match `max_new_tokens`.")
        if max_new_tokens % S:
            raise AssertionError("Expecting `max_new_tokens` to be a multiple of `self.config.S`.")
        ids = self._ids(input_ids)
        B, n_new = ids.size(0), max_new_tokens // S
        n_prompt = ids.numel() // (B * S)
        cond = self._cond(action_ids, B, n_frames=n_prompt + n_new, action_vectors=action_vectors)
        if kv_cache and n_new >= 1 and n_prompt >= 1 and n_prompt + n_new <= self.config.T:
            # the same frames on the temporal KV cache, the whole loop one library call (genie_generate_cached): every MaskGIT step
            # runs the rows of the frame being decoded instead of a full forward over the canvas (causal in time: the all-MASK
            # frames behind it never reach it).  Equal to the loop below up to f32 accumulation order.
            lib = _lib.load()
            cfg, w = self._weights()[:2]
            dev = ids.device
            steps = int(maskgit_steps)
            V = self.config.factored_vocab_size * self.config.num_factored_vocabs
            clip = torch.full((B, n_prompt + n_new, S), self.mask_token_id, dtype=torch.int64, device=dev)
            clip[:, :n_prompt] = ids.view(B, n_prompt, S)
            nz = None
            if steps > 1 and unmask_mode != "greedy":   # torch.rand_like of st_mask_git.py:204-206: the caller's draws, or fresh ones
                nz = (torch.rand(n_new, steps - 1, B, S, device=dev) if noise is None
                      else noise.to(dev)[:, :steps - 1].reshape(n_new, steps - 1, B, S).float().contiguous())
            uni = None
            if temperature > 1e-8:
                uni = (torch.rand(n_new, steps, self.config.num_factored_vocabs, B, S, device=dev) if uniforms is None
                       else uniforms.to(device=dev, dtype=torch.float32).contiguous())
                assert uni.numel() == n_new * steps * self.config.num_factored_vocabs * B * S, "uniforms: (n_new, steps, nv, B, S)"
            gen = torch.empty(B, n_new, S, dtype=torch.int64, device=dev)
            lg0 = torch.empty(B, n_new, S, V, dtype=torch.float32, device=dev) if return_logits else None
            nbytes = lib.genie_prefix_cache_bytes(cfg, B if guide is None else 2 * B)   # (guided passes run [conditional ; null])
            cache = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ws = self._workspace(B, generate_prompt_frames=n_prompt, guided=guide is not None)
            _lib.check(_lib.call_guided(lib, "genie_generate_cached", cond, law, guide, cfg, w, clip.data_ptr(), B, n_prompt, n_new, steps,
                                      float(temperature), mode,
                                      0 if nz is None else nz.data_ptr(), 0 if uni is None else uni.data_ptr(), 0, 1,
                                      gen.data_ptr(), 0 if lg0 is None else lg0.data_ptr(), cache.data_ptr(), nbytes,
                                      ws.data_ptr(), ws.numel(), self._stream()), "genie_generate_cached")
            tokens = torch.cat([ids.view(B, n_prompt * S), gen.view(B, n_new * S)], dim=1)
            if not return_logits:
                return tokens
            nv, vf = self.config.num_factored_vocabs, self.config.factored_vocab_size
            # (B, n, S, [vocab0 | vocab1]) -> "B vocab_size num_vocabs n H W": the per-frame (B, 512, 2, H, W) logits stacked on dim 3
            return tokens, lg0.view(B, n_new, self.h, self.w, nv, vf).permute(0, 5, 4, 1, 2, 3)
        # one (B, n_prompt + n_new, H, W) canvas: prompt frames up front, the frames to come all-MASK; maskgit_generate fills
        # canvas[:, t] in place, which is exactly what the next frame's context must contain
        canvas = torch.full((B, n_prompt + n_new, self.h, self.w), self.mask_token_id, dtype=torch.long, device=ids.device)
        canvas[:, :n_prompt] = ids.view(B, n_prompt, self.h, self.w)
        step0_logits = []
        for k in range(n_new):
            frame, logits = self.maskgit_generate(canvas, n_prompt + k, maskgit_steps=maskgit_steps, temperature=temperature,
                                                  noise=None if noise is None else noise[k], return_logits=return_logits,
                                                  action_ids=None if cond is None or self.config.action_dim else cond.keep,
                                                  action_vectors=cond.vectors if self.config.action_dim else None, sampling=sampling,
                                                  unmask_mode=unmask_mode, uniforms=None if uniforms is None else uniforms[k],
                                                  guidance=guidance)
            canvas[:, n_prompt + k] = frame
            step0_logits.append(logits)
        tokens = canvas.view(B, -1)
        return (tokens, torch.stack(step0_logits, dim=3)) if return_logits else tokens

    def rollout(self, prompt_BPHW, n_new, keep=None, **kwargs):
        """n_new frames behind the prompt frames (B, P, H, W), past the window T if need be -> (B, P + n_new, H, W): generate.rollout_frames
        (one library call; the window slides by T - keep frames, re-running the last `keep` as its context; known=(B, n_new, H, W)
        keeps given tokens of the generated frames)."""
        from .generate import rollout_frames
        return rollout_frames(self, prompt_BPHW, n_new, keep=keep, **kwargs)

    def fanout(self, prompt_BPHW, n_new, K=None, **kwargs):
        """K candidate futures of n_new frames per prompt (B, P, H, W) -> (B, K, n_new, H, W) over one shared context cache:
        generate.fanout_frames (one library call, in-window: P + n_new <= T; known=(B, K, n_new, H, W) or (B, n_new, H, W) keeps given
        tokens of the new frames)."""
        from .generate import fanout_frames
        return fanout_frames(self, prompt_BPHW, n_new, K=K, **kwargs)

    def score(self, clip_BTHW, num_prompt_frames, K=None, **kwargs):
        """Per-frame negative log-likelihood of the observed frames behind the prompt under K action hypotheses per clip -> a Score with
        nll (B, K, n) float64: generate.score_frames (one library call, in-window)."""
        from .generate import score_frames
        return score_frames(self, clip_BTHW, num_prompt_frames, K=K, **kwargs)

    # ------------------------------------------------------------------ weights
    def init_weights(self):
        """N(0, 0.02) Linear/Embedding weights, zero biases (reference :281-296; the muP branch of the
        reference needs the un-vendored ``mup`` package and is not reproduced)."""
        std = 0.02
        for module in self.modules():
            if isinstance(module, nn.Linear):
                module.weight.data.normal_(mean=0.0, std=std)
                if module.bias is not None:
                    module.bias.data.zero_()
            elif isinstance(module, nn.Embedding):
                module.weight.data.normal_(mean=0.0, std=std)
        self._invalidate()

    def set_mup_shapes(self, rescale_params=False):
        """The reference attaches muP infshapes for training (:298-304).  At inference the only effect is the
        readout factor output_mult/width_mult with base width 256, which cfg.readout_mult already carries."""
        return None

    def save_pretrained(self, save_directory):
        """config.json (flat GenieConfig dict) + model.safetensors, the layout the reference's
        PyTorchModelHubMixin writes.  An unconditioned model's config.json has no action key."""
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config.to_json_dict(), f)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()},
                  os.path.join(save_directory, "model.safetensors"))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, precision="exact", action_vocab_size=None, action_dim=None, **kwargs):
        """Load a local HF-style checkpoint directory (hub ids need a network and are not supported offline).
        action_vocab_size=A > 0 on an unconditioned checkpoint: a warm start -- every stored tensor loads strictly and the new
        action table is zero, so the model computes exactly what the checkpoint does until the table is trained.
        action_dim=A > 0 on an unconditioned checkpoint: the same warm start for continuous actions -- zero projection weight, bias
        and null row, mean 0 and std 1."""
        from safetensors.torch import load_file
        d = str(pretrained_model_name_or_path)
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d} is not a local checkpoint directory (no network access for hub ids)")
        with open(os.path.join(d, "config.json")) as f:
            raw = json.load(f)
        raw = raw.get("config", raw)
        from dataclasses import fields
        known = {f.name for f in fields(GenieConfig)}
        config = GenieConfig(**{k: v for k, v in raw.items() if k in known})
        if config.use_mup:
            import warnings
            warnings.warn("use_mup=True: the readout factor follows mup's documented formula output_mult * x / width_mult "
                          "(base width 256); the reference's own mup fork is not vendored, so this factor is not pinned "
                          "against reference outputs (DESIGN.md section 7, 'parity unpinned')")
        sd = load_file(os.path.join(d, "model.safetensors"))
        warm = False
        if action_vocab_size is not None and action_vocab_size != config.action_vocab_size:
            if config.action_vocab_size or config.action_dim:
                raise ValueError(f"checkpoint has action_vocab_size={config.action_vocab_size}, action_dim={config.action_dim}; "
                                 f"asked for action_vocab_size={action_vocab_size}")
            config.action_vocab_size = int(action_vocab_size)
            warm = config.action_vocab_size > 0
        warm_vec = False
        if action_dim is not None and action_dim != config.action_dim:
            if config.action_dim or config.action_vocab_size:
                raise ValueError(f"checkpoint has action_dim={config.action_dim}, action_vocab_size={config.action_vocab_size}; "
                                 f"asked for action_dim={action_dim}")
            config = GenieConfig(**{**vars(config), "action_dim": int(action_dim)})   # (runs the exclusivity check)
            warm_vec = config.action_dim > 0
        model = cls(config, precision=precision)
        if warm:
            sd = dict(sd)
            sd["action_embed.weight"] = torch.zeros(config.action_vocab_size, config.d_model)
        if warm_vec:
            sd = dict(sd)
            sd.update({"action_proj.weight": torch.zeros(config.d_model, config.action_dim), "action_proj.bias": torch.zeros(config.d_model),
                       "action_null": torch.zeros(config.d_model), "action_mean": torch.zeros(config.action_dim),
                       "action_std": torch.ones(config.action_dim)})
        model.load_state_dict(sd, strict=True)
        model.eval()
        return model

    # ------------------------------------------------------------------ LoRA adapters (lora.py; include/genie_hip.h, "LoRA adapters")
    def load_adapter(self, adapter):
        """Serve an adapter: every targeted Linear weight becomes W0 + (alpha / rank) B A, merged in place by genie_lora_merge (the kernel
        the trainer merges with: the logits are the trained model's bits), and the packed copies are rebuilt.  `adapter`: a directory
        GenieTrainer.save_adapter wrote, or (config dict, {name: tensor}).  The base tensors that were replaced are remembered:
        `unload_adapter()` puts their bits back; loading a second adapter unloads the first.  ValueError -- the model unchanged -- for an
        adapter of another base geometry, a target that is no Linear of this model, or a missing, surplus or wrong-shaped tensor."""
        from . import lora as _lora
        dev = self._device()
        cfg, tensors = _lora.load_adapter_files(adapter) if isinstance(adapter, (str, os.PathLike)) else adapter
        named = dict(self.named_parameters())
        rank, scale, targets = _lora.check_adapter(cfg, tensors, self.config, {n: tuple(p.shape) for n, p in named.items()})
        self.unload_adapter()
        keep = {n: torch.as_tensor(t).to(dev, torch.float32).contiguous() for n, t in tensors.items()}
        base, items = {}, []
        for n in targets:
            w = named[n].data
            base[n] = w.clone()
            a, b = _lora.adapter_names(n)
            items.append(_lora.item(scale, w.shape[0], w.shape[1], rank, keep[a].data_ptr(), keep[b].data_ptr(), w=w.data_ptr(),
                                    w0=w.data_ptr()))
        try:
            _lora.merge(_lib.load(), items, self._stream())
        except Exception:
            for n, t in base.items():
                named[n].data.copy_(t)
            raise
        self._adapter_base = base
        self.refresh_weights()
        return self

    def unload_adapter(self):
        """Put back the base weights `load_adapter` replaced (their saved bits) and rebuild the packed copies.  No adapter: nothing happens."""
        base = getattr(self, "_adapter_base", None)
        if base:
            named = dict(self.named_parameters())
            for n, t in base.items():
                named[n].data.copy_(t)
            self.refresh_weights()
        self._adapter_base = None
        return self

    def load_numpy_state_dict(self, sd: dict):
        """Load {key: ndarray} (e.g. from 1xgpt_amd.synthetic.make_state_dict)."""
        self.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return self


class FixedMuReadout(nn.Linear):
    """Name kept for import compatibility (reference :316-323): y = Linear(output_mult * x / width_mult).
    Inside STMaskGIT the factor is fused into the readout GEMM; this standalone module applies it through
    the same HIP GEMM."""
    output_mult = 1.0

    def width_mult(self):
        return self.in_features / 256

    def forward(self, x):
        from .attention import hip_linear
        shp = x.shape
        x2 = (x.contiguous().view(-1, shp[-1]).float() * (self.output_mult / self.width_mult()))
        return hip_linear(x2, self.weight, self.bias).view(*shp[:-1], -1)
