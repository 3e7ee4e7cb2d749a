/* genie_hip.h -- C ABI of libgenie_hip.so: the MI355X (gfx950) GENIE forward / MaskGIT sampling path.
 *
 * The reference (1x-technologies/1xgpt) has no FFI of its own: its seam is the Python nn.Module
 * surface.  Each entry point below names the reference call it replaces
 * (file:line relative to the reference tree); the drop-in Python module in 1xgpt_amd/ binds them with
 * ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - every function returns 0 on success, a negative GENIE_E_* code otherwise; nothing throws or aborts;
 *    genie_last_error() returns a thread-local description of the last failure.
 *  - all pointers are DEVICE pointers unless the name ends in _host; they are borrowed for the call only.
 *  - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - no allocation: the caller owns the workspace (genie_workspace_bytes) and every output buffer.
 *  - token ids are int64 (torch.LongTensor), activations/logits float32, flags uint8.
 *  - activations are token-major (B, T, S, C) row-major; nothing is ever physically transposed to
 *    (B S) T C (reference st_transformer.py:77,82): the temporal kernel reads frame-strided rows.
 *
 * Memory the caller provides
 *  The library never allocates, so every buffer below is the caller's, and most of them are re-used from call to call with other
 *  batch sizes, prompt lengths and precisions.  What a buffer may hold ON ENTRY:
 *  - ANYTHING (uninitialised, NaN, the leftovers of any earlier call):
 *      `workspace` of every entry point.  The library initialises whatever it reads there: the loops' id tables (context ids, the
 *        one- and two-frame pass rows, the frame being decoded, samples, the per-call action tables) are written by a launch before
 *        the pass that reads them, and their `unmasked` bytes are cleared by the call at the top of every frame.
 *      `cache` of genie_clean_pass* (whole), of genie_frame(s)_pass* (the slots >= t0: a pass reads slots [0, t0) and writes its own),
 *        of genie_generate_cached*, of genie_rollout_cached with resume == 0 or at the first frame of a window, and `trunk` / `branch`
 *        of genie_generate_fanout / genie_score_fanout.  The attention kernels read fixed-size tiles of frame slots; slots no pass
 *        has written must not reach a result: a kernel clamps or predicates such loads, and never masks one by 0 * value, which a
 *        stale NaN survives.
 *      every OUTPUT: logits, logits0_out, hidden states, samples_out, gen_out, conf, keys_out, nll / hits / token_nll, the
 *        destinations of the genie_pack_* functions (bf16 / split-f16 planes, the fused and fragment-order streams), the MAGVIT2
 *        conv outputs, GroupNorm statistics and partials.  Outputs are WRITTEN IN FULL: after the call no element of the documented
 *        shape holds what was there before.  (Argument errors return before anything is enqueued and leave them untouched.)
 *  - ZEROED BY THE CALLER, because the entry point accumulates into it:
 *      sums_out of genie_factored_ce / genie_readout_ce (3 doubles, atomicAdd) and sums6[2] of genie_metric_hits;
 *      status_flag of genie_maskgit_generate* (set on a violation, never cleared);
 *      `unmasked` of genie_mask_step before the first step of a frame (in/out across the steps of that frame).
 *  - CARRIED OVER from the call that produced it, byte for byte:
 *      `cache` between genie_clean_pass* and the genie_masked_frames_logits* calls that read it (same B and nframes), and between
 *        consecutive genie_frame(s)_pass* calls (slots [0, t0));
 *      `cache` of genie_rollout_cached with resume == 1 in mid-window: the slots of [start_j, f0 - 1).  The slot of the pending frame
 *        f0 - 1 and every later slot may hold anything, and so may the whole cache when f0 opens a window;
 *      `frames` [0, f0) of genie_rollout_cached; `prompt` of genie_maskgit_generate* (in/out).
 *  Training (genie_train_*): the activation buffer and the workspace may hold anything before genie_train_forward*; between the forward
 *  and the backward calls of one step both are carried over.
 *  Enforced by tests/test_hip_stale_memory.py: every call above gives the same bits on buffers filled with 0x00, 0xFF and 0x3C bytes.
 */
#ifndef GENIE_HIP_H
#define GENIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GENIE_ABI_VERSION 3

enum {
    GENIE_OK = 0,
    GENIE_E_ARG = -1,         /* null pointer / bad size */
    GENIE_E_SHAPE = -2,       /* shape not supported by the kernels (see genie_check_config) */
    GENIE_E_UNSUPPORTED = -3, /* feature flag not supported */
    GENIE_E_LAUNCH = -4,      /* HIP reported a launch / runtime error */
    GENIE_E_ASSERT = -5       /* a reference `assert` would have fired (st_mask_git.py:154-156) */
};

enum { GENIE_PREC_EXACT = 0, /* f32 MFMA (v_mfma_f32_32x32x2_f32), f32 everywhere */
       GENIE_PREC_BF16 = 1,  /* bf16 MFMA operands, f32 accumulate/residual/LN/softmax: throughput mode */
       GENIE_PREC_F16X3 = 2  /* every Linear on the f16 matrix cores with split operands a = hi + lo/2048:
                                hi.hi + (hi.lo + lo.hi)/2048 in f32 = 22-bit operands, f32-class results at
                                1/3 of the f16 MFMA rate; attention, LN, softmax, residual stay f32 */ };

enum { GENIE_LAYOUT_TOKEN_MAJOR = 0, /* (B, nt, S, V)              */
       GENIE_LAYOUT_BCTHW = 1        /* (B, V, nt, S) == "B C T H W" (st_mask_git.py:264) */ };

enum { GENIE_UNMASK_RANDOM = 0, GENIE_UNMASK_GREEDY = 1 }; /* st_mask_git.py:200-209 */
enum { GENIE_UNMASK_CONFIDENCE = 2 }; /* no reference counterpart: confidence + annealed Gumbel noise (genie_sampling below) */

/* GenieConfig (genie/config.py:7-55) reduced to what the kernels need. */
typedef struct genie_cfg {
    int32_t num_layers, num_heads, head_dim, d_model;
    int32_t T, S;
    int32_t hidden;            /* int(d_model * mlp_ratio) */
    int32_t factored_vocab;    /* 512 */
    int32_t num_factored;      /* 1 or 2 */
    int32_t image_vocab_size;  /* == mask token id (st_mask_git.py:51) */
    int32_t qk_norm, use_mup, qkv_bias, proj_bias, mlp_bias;
    float attn_scale;          /* use_mup ? 8/Dh : Dh^-0.5 (attention.py:26) */
    float readout_mult;        /* use_mup ? output_mult/width_mult : 1 (st_mask_git.py:316-323) */
    int32_t precision;         /* GENIE_PREC_* */
} genie_cfg;

/* SelfAttention parameters (genie/attention.py:27-34). *_w16 are bf16 copies made by
 * genie_pack_bf16 (only read when precision == GENIE_PREC_BF16). */
typedef struct genie_attn_weights {
    const float* qkv_w;  /* (3d, d) */
    const float* qkv_b;  /* (3d) or NULL */
    const float* proj_w; /* (d, d) */
    const float* proj_b; /* (d) or NULL */
    const float* norm_w; /* (Dh) qk-norm affine shared by q and k, or NULL */
    const float* norm_b;
    const uint16_t* qkv_w16;
    const uint16_t* proj_w16;
    /* GENIE_PREC_BF16, shipped geometry (d 256, 8 heads of 32), or NULL (unfused launches): in the TEMPORAL attention's struct
     * (T 16) the qkv and proj weights as the fragment stream of the fused qkv + attention + proj kernel
     * (genie_pack_temporal_fused_bf16); in the SPATIAL attention's struct (S 256) the proj weights as the fragment stream of
     * the fused attention + proj kernel (genie_pack_spatial_proj_fused_bf16). */
    const uint16_t* fused_w16;
    /* GENIE_PREC_F16X3 range flags of the packed tensors (bit 0: qkv_w16, bit 1: proj_w16): set when the tensor's hi plane
     * reaches |w| >= 32, see "range contract" below.  0 in the other precisions. */
    int32_t w16_wide;
    /* GENIE_PREC_F16X3, head_dim 64 or 32 (ABI 3), or NULL (the one-frame passes then run the row-major kernels): [qkv | proj] as split
     * f16 in FRAGMENT ORDER for the one-frame passes of generate (genie_pack_frame_w16, genie_frames_pass). */
    const uint16_t* frame_w16;
} genie_attn_weights;

/* STBlock parameters (genie/st_transformer.py:28-68). */
typedef struct genie_layer_weights {
    const float* norm1_w; /* (d) or NULL when qk_norm (Identity) */
    const float* norm1_b;
    genie_attn_weights spatial;
    genie_attn_weights temporal;
    const float* norm2_w;
    const float* norm2_b;
    const float* fc1_w; /* (hidden, d) */
    const float* fc1_b;
    const float* fc2_w; /* (d, hidden) */
    const float* fc2_b;
    const uint16_t* fc1_w16;
    const uint16_t* fc2_w16;
    /* GENIE_PREC_BF16, d 256 / hidden 1024: fc1 and fc2 as the fragment stream of the fused LayerNorm + MLP kernel
     * (genie_pack_mlp_fused_bf16), or NULL (unfused launches). */
    const uint16_t* mlp_fused_w16;
    int32_t w16_wide; /* f16x3 range flags: bit 0 fc1_w16, bit 1 fc2_w16 */
    const uint16_t* mlp_frame_w16; /* GENIE_PREC_F16X3 (ABI 3): [fc1 | fc2] in fragment order (genie_pack_frame_w16), or NULL */
} genie_layer_weights;

/* STMaskGIT parameters (genie/st_mask_git.py:36-61); `layers` is a HOST array of num_layers entries. */
typedef struct genie_weights {
    const float* pos_embed;  /* (T, S, d) */
    const float* mask_embed; /* (d) */
    const float* embed[4];   /* num_factored tables of (factored_vocab, d) */
    const float* out_w;      /* (num_factored*factored_vocab, d) */
    const float* out_b;
    const uint16_t* out_w16;
    const genie_layer_weights* layers_host;
    int32_t out_w16_wide; /* f16x3 range flag of out_w16 */
    const uint16_t* out_frame_w16; /* GENIE_PREC_F16X3 (ABI 3): out_w in fragment order (genie_pack_frame_w16), or NULL */
} genie_weights;

/* Per-frame action conditioning (ABI 3 addition; the structs above are unchanged).  The model has a learned table of
 * n_actions rows of d_model; row ids[b, t] is added to every token of frame t of clip b, masked tokens included, where the
 * positional embedding is added:  x[b,t,s] = token_embed(id) + (pos_embed[t,s] + table[ids[b,t]])  -- position row plus
 * action row first, so one clip with actions is bit-identical to an unconditioned model whose positional table is
 * pos + table[a_t].  The *_cond entry points below take this as a trailing argument; NULL (or n_actions == 0) is exactly the
 * unconditioned entry point.  `ids` always addresses ABSOLUTE clip frames with a clip stride of cfg->T, also in the
 * window passes (genie_frames_pass at t0, genie_masked_frames_logits at frame0, ...): frame i of such a pass reads
 * ids[b * cfg->T + t0 + i].  An id outside [0, n_actions) adds zero (callers should reject it: nn.Embedding raises). */
typedef struct genie_frame_cond {
    const float* table;   /* (n_actions, d_model) f32, device */
    const int64_t* ids;   /* (B, T) device: action of clip b at ABSOLUTE frame t (clip stride = cfg->T) */
    int32_t n_actions;
} genie_frame_cond;

/* The sampling law of the MaskGIT decoder (ABI 3 addition; NULL = every field off = the reference's behaviour, bit for bit).
 * Departure from the reference: st_mask_git.py:184-186 builds Categorical(probs=probs / temperature), which renormalises, so
 * its `temperature` only switches arg-max to sampling and there is no top-k or nucleus filter.  Here, per token and per factored
 * vocabulary (most significant first):
 *   z_i = logit_i * (1.0f / logit_temperature)                                     -- one f32 multiply; off at 1
 *   top_k: keep i iff #{j : z_j > z_i or (z_j == z_i and j < i)} < top_k             -- stable rank by count; off at 0 or >= factored_vocab
 *   top_p: among those survivors in that rank order, keep i iff the probability mass (softmax of z over the survivors) of the
 *          survivors ranked strictly before i is < top_p; the best entry is always kept   -- off at >= 1 (and <= 0)
 * temperature > 1e-8 draws by the inverse CDF in index order over the kept entries on the caller's uniform (pick = #{kept prefix
 * sums < u * total}, the last kept entry at most); temperature <= 1e-8 takes the arg-max, which no filter changes.  The
 * confidence is the picked entry's probability under the TEMPERED, UNFILTERED softmax (top_k = 1 does not report 1 everywhere).
 * choice_temperature c >= 0 belongs to GENIE_UNMASK_CONFIDENCE (the MaskGIT paper's schedule, which the reference lacks; its
 * docstring notes that greedy unmasking "tends to copy the previous frame"): at step `step` of `steps` the re-masking key of a
 * token is log(conf) + c * (1 - (step + 1) / steps) * g, g = -log(-log(u)), u = the caller's U[0,1) draw of the `noise` array the
 * random mode takes (same shape), clamped to [2^-24, 1 - 2^-24]; the keys go through genie_mask_step unchanged. */
typedef struct genie_sampling {
    float logit_temperature;  /* tau > 0 */
    int32_t top_k;            /* >= 0 */
    float top_p;
    float choice_temperature; /* c >= 0 */
} genie_sampling;

/* Classifier-free guidance of an action-conditioned model (ABI 3 addition; NULL = none).  null_action is a row id in [0, n_actions)
 * of the action table: the "no action" row, which training learns by replacing a clip's actions with it some of the time (action
 * dropout, 1xgpt_amd/data.py).  scale is w, finite: 1 = plain conditional sampling, 0 = the null stream alone, > 1 = guidance.  For every
 * token, every factored vocabulary and every entry i, with c_i the logit under the clip's actions and u_i the logit of the same tokens
 * with null_action at every frame, the guided logit is, in f32 with three separately rounded operations and no FMA contraction,
 *     omw = 1.0f - w          (computed once on the host)
 *     g_i = (w * c_i) + (omw * u_i)
 * -- reproducible bit for bit in NumPy f32, and w = 1 gives g = c, w = 0 gives g = u, both up to the sign of a zero (which neither the
 * ordering nor exp sees).  Everything after that is the genie_sampling law applied to g: z = g * (1 / tau), confidence from the tempered
 * unfiltered softmax of z, top-k, top-p, the inverse-CDF draw, arg-max at temperature <= 1e-8, the confidence-mode key from the same
 * launch.  A NULL genie_sampling under guidance is the all-off law.  Reference counterpart: none. */
typedef struct genie_guidance {
    float scale;         /* w, finite */
    int32_t null_action; /* in [0, n_actions) */
} genie_guidance;

int genie_version(void);
/* sizeof(genie_guidance) and the offsets of its two fields, in declaration order: writes min(n, 3) entries, returns 3. */
int genie_guidance_layout(size_t* out_host, int n);
/* sizeof(genie_sampling) and the offsets of its four fields, in declaration order: writes min(n, 5) entries, returns 5. */
int genie_sampling_layout(size_t* out_host, int n);
/* The compiler's view of the POD structs above, for bindings to check their own declarations against (tests/test_abi_and_host.py):
 * out[0..8) = sizeof(genie_cfg), sizeof(genie_attn_weights), offsetof(.., fused_w16), offsetof(.., w16_wide),
 * sizeof(genie_layer_weights), offsetof(.., mlp_fused_w16), offsetof(.., w16_wide), sizeof(genie_weights),
 * offsetof(.., out_w16_wide), then (ABI 3) offsetof(genie_attn_weights, frame_w16), offsetof(genie_layer_weights, mlp_frame_w16),
 * offsetof(genie_weights, out_frame_w16).  Writes min(n, 12) entries, returns 12. */
int genie_abi_layout(size_t* out_host, int n);
const char* genie_last_error(void);
/* 0 if the kernels support this configuration, GENIE_E_SHAPE otherwise (message in genie_last_error). */
int genie_check_config(const genie_cfg* cfg);
/* Bytes of workspace genie_compute_* / genie_maskgit_generate need for a batch of B clips. */
size_t genie_workspace_bytes(const genie_cfg* cfg, int B);

/* f32 -> bf16 (round-to-nearest-even) weight packing for GENIE_PREC_BF16. */
int genie_pack_bf16(const float* src, uint16_t* dst, size_t n, void* stream);
/* f32 -> f16 split planes for GENIE_PREC_F16X3: dst[0..n) = hi, dst[n..2n) = lo with src ~ hi + lo/2048.
 * In that precision the *_w16 pointers of the weight tables point at such 2n-element buffers. */
int genie_pack_split_f16(const float* src, uint16_t* dst, size_t n, void* stream);
/* GENIE_PREC_F16X3 range contract per weight tensor.  The chip-filling split GEMM scales the weight's hi plane by 2^11 in f16
 * registers, which is exact for |w| < 32 only.  A caller that packs a tensor whose hi plane reaches 32 (finite in f16, i.e.
 * |w| < 65504) sets the tensor's bit in the `w16_wide` field of the struct that carries its pointer; every Linear reading that
 * tensor then runs on the two-accumulator kernels, which scale nothing (same f32-class result, lower rate for that tensor
 * only).  The flag travels with the weight table: there is no process-global state.
 * Reference counterpart: none (the reference's Linear layers are f32: st_transformer.py:16-25, attention.py:27-29). */
enum { GENIE_WIDE_QKV = 1, GENIE_WIDE_PROJ = 2, GENIE_WIDE_FC1 = 1, GENIE_WIDE_FC2 = 2,
       GENIE_FUSED_QKV_STREAM = 4 /* genie_attn_weights.w16_wide of a SPATIAL attention: fused_w16 also holds the qkv fragment stream (below) */ };

/* Fragment streams of the fused sub-block kernels (GENIE_PREC_BF16, magvit_n32_h8_d256 geometry; csrc/kernels_fused.hip).
 * temporal: qkv_w (768, 256) and proj_w (256, 256) f32 -> 262,144 bf16 values;  mlp: fc1_w (1024, 256) and fc2_w (256, 1024)
 * f32 -> 524,288 bf16 values.  Reference counterpart: the nn.Linear weights of attention.py:27-29 / st_transformer.py:16-25. */
#define GENIE_TEMPORAL_FUSED_ELEMS 262144
#define GENIE_MLP_FUSED_ELEMS 524288
#define GENIE_SPATIAL_PROJ_FUSED_ELEMS 65536 /* spatial: proj_w (256, 256) f32 -> the out-projection's fragments per head */
/* spatial, optional second part of the same buffer (at element GENIE_SPATIAL_PROJ_FUSED_ELEMS): qkv_w (768, 256) f32 -> 24 stages of 16
 * fragments.  With it (and GENIE_FUSED_QKV_STREAM set) the PREVIOUS block's fused MLP kernel also runs this block's norm1 and spatial qkv
 * Linear (st_transformer.py:74, attention.py:37) and writes the attention kernel's operand planes: no LayerNorm, no qkv GEMM launch. */
#define GENIE_SPATIAL_QKV_FUSED_ELEMS 196608
#define GENIE_SPATIAL_FUSED_ELEMS (GENIE_SPATIAL_PROJ_FUSED_ELEMS + GENIE_SPATIAL_QKV_FUSED_ELEMS)
int genie_pack_temporal_fused_bf16(const float* qkv_w, const float* proj_w, uint16_t* dst, void* stream);
/* GENIE_PREC_F16X3, same geometry (d 256, 8 heads of 32): the TEMPORAL attention's `fused_w16` holds the split-f16 fragment stream of its
 * qkv weights (768, 256) f32 -> 393,216 f16 values, and the temporal qkv Linear + temporal attention run as one kernel on the f32 rows of x
 * (csrc/kernels_fused_f16x3.hip; st_transformer.py:77-78, attention.py:36-58).  No |w| < 32 contract: nothing is scaled. */
#define GENIE_TEMPORAL_QKV_F16X3_ELEMS 393216
int genie_pack_temporal_qkv_f16x3(const float* qkv_w, uint16_t* dst, void* stream);
/* Unit entry points of the fused sub-blocks (parity tests, tuning).  All update the f32 residual stream x in place and return
 * GENIE_E_UNSUPPORTED outside the geometry above or below their size thresholds -- temporal / mlp: 2 clips' worth of rows (8,192), spatial:
 * 128 sequences; measured break-evens, DESIGN.md section 4 -- (the layer drivers then run the unfused launches).
 *   temporal: x (B,16,S,256) += proj(causal_attention_T(qkv(x16))), x16 = bf16 copy of x (B,16,S,256), or NULL: the kernel rounds its
 *             operands from x itself (same values, no second buffer read); needs aw->fused_w16.
 *             Reference: st_transformer.py:77-78 (the permute to (B S) T C is never materialised), attention.py:36-61.
 *   spatial:  x (n_seq*256, 256) += proj(softmax(q k^T) v) from the operand planes [Q scale log2e | K | V^T] of the spatial qkv GEMM
 *             (n_seq sequences of 256 tokens, 8 heads of 32), x16 = bf16 copy of the result (NULL: not written); needs aw->fused_w16.
 *             Reference: st_transformer.py:73-74, attention.py:48-60.  (The planes are an internal format of the block driver:
 *             this entry exists for tuning -- tools/bench_spatial_fused.py; tests/test_hip_fused.py checks the planes' formats
 *             element-wise at their producer, genie_mlp_fused_qkv_bf16, and this kernel through the block.)
 *   mlp:      x (rows,256) += fc2(gelu(fc1(LayerNorm(x; norm2)))), rows % 128 == 0; x16_out (or NULL) receives the bf16 copy
 *             of the result, or -- when next_norm_w / next_norm_b are given -- LayerNorm(result; next_norm_*) in bf16 (the next
 *             block's norm1 output, st_transformer.py:73); needs lw->mlp_fused_w16.  Reference: st_transformer.py:81, 16-25. */
int genie_temporal_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, const uint16_t* x16, float* x, int B, void* stream);
/* ... of the prefix-cache passes (cfg->T = the model's T, nframes < T the pass's frames; x (B, nframes, S, 256)):
 *   genie_temporal_prefix_fused_bf16: x += proj_t(attention(qkv_t(x))) in GENIE_PREC_BF16; mode 1 = causal + the K / V fragment images written to
 *     `kv` (B * S * 16 KB), mode 2 = query slot i attends the images' slots j < i + shift and its own key (evaluate.py:107-116).
 *   genie_temporal_qkv_attn_f16x3: a = attention(qkv_t(x)) in GENIE_PREC_F16X3 as operand planes a16 = [hi | lo'] `plane_elems` apart, rows
 *     (B nframes S) x 256; mode 0 = plain causal (nframes <= T, kv unused), 1 / 2 as above with the f32 k / v accumulators in `kv` (B * S * 32 KB).
 * Reference counterpart: st_transformer.py:77-78, attention.py:36-61.  Tests: tests/test_hip_fused.py, tests/test_hip_fused_f16x3.py. */
int genie_temporal_prefix_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, float* x, uint16_t* kv, int B, int nframes, int mode,
                                     int shift, void* stream);
int genie_temporal_qkv_attn_f16x3(const genie_cfg* cfg, const genie_attn_weights* aw, const float* x, uint16_t* a16, int64_t plane_elems,
                                  float* kv, int B, int nframes, int mode, int shift, void* stream);
int genie_spatial_attn_proj_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, const uint16_t* qkv_planes, float* x,
                                       uint16_t* x16, int64_t n_seq, void* stream);
int genie_mlp_fused_bf16(const genie_cfg* cfg, const genie_layer_weights* lw, float* x, uint16_t* x16_out, int64_t rows,
                         const float* next_norm_w, const float* next_norm_b, void* stream);
/* The same kernel in the form the block driver uses between two blocks: besides x += mlp(...) it runs the NEXT block's norm1 and spatial qkv
 * Linear (next->norm1_*, next->spatial.fused_w16 with GENIE_FUSED_QKV_STREAM) and writes that block's attention operand planes into
 * `planes` (3 * rows * 256 bf16 values: [Q | K | V^T]; sequences of 256 consecutive rows, 8 heads of 32):
 *   Q[((seq * 8 + head) * 256 + pos) * 32 + f]   = q * attn_scale * log2(e)          K likewise, unscaled
 *   V^T[((seq * 8 + head) * 32 + f) * 256 + p']  with p' = 16 * (pos / 16) + perm(pos % 16), perm = {0-3 -> 0-3, 8-11 -> 4-7, 4-7 -> 8-11, 12-15 -> 12-15}
 * (the formats genie_spatial_attn_proj_fused_bf16 consumes).  GENIE_E_UNSUPPORTED with qkv_bias or outside the geometry.
 * Reference: st_transformer.py:81 then :74 (norm1) and attention.py:37 (qkv) of the following block. */
int genie_mlp_fused_qkv_bf16(const genie_cfg* cfg, const genie_layer_weights* lw, const genie_layer_weights* next, float* x,
                             uint16_t* planes, int64_t rows, void* stream);
int genie_pack_mlp_fused_bf16(const float* fc1_w, const float* fc2_w, uint16_t* dst, void* stream);
int genie_pack_spatial_proj_fused_bf16(const float* proj_w, uint16_t* dst, void* stream);
int genie_pack_spatial_qkv_fused_bf16(const float* qkv_w, uint16_t* dst, void* stream);   /* dst: GENIE_SPATIAL_QKV_FUSED_ELEMS values */

/* ---- unit entry points (one reference op each; used by the parity tests) -------------------------- */

/* FactorizedEmbedding.forward + pos-embed add (factorization_utils.py:29-52, st_mask_git.py:257-261).
 * ids (B,T,S) int64 -> x (B,T,S,d). */
int genie_embed(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, float* x, void* stream);
int genie_embed_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, float* x, void* stream,
                     const genie_frame_cond* cond);

/* nn.LayerNorm(C, eps) over the last dim of (rows, C) (st_transformer.py:44,67). */
int genie_layer_norm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps,
                     void* stream);

/* nn.Linear: y = x W^T (+b) with optional fused erf-GELU and residual accumulate (y += ...).
 * x (M,K), W (N,K), y (M,N).  (attention.py:27,29; st_transformer.py:16-25) */
int genie_linear(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int gelu,
                 int accumulate, void* stream);

/* The same Linear on the 16-bit matrix cores with PRE-PACKED operands (unit entry for parity tests and tuning):
 * GENIE_PREC_BF16: x16 (M,K), W16 (N,K) bf16 (genie_pack_bf16);  GENIE_PREC_F16X3: split planes [hi | lo] of
 * each (genie_pack_split_f16).  y (M,N) f32. */
int genie_linear_lowp(int precision, const uint16_t* x16, const uint16_t* W16, const float* b, float* y, int M, int N,
                      int K, int gelu, int accumulate, void* stream);

/* softmax(scale q k^T [+causal]) v on a packed qkv buffer (attention.py:38-59).
 * qkv (B,T,S,3d) with feature index = which*d + head*Dh + i; out (B,T,S,d).
 * spatial: sequences are the S tokens of one (b,t), non-causal (st_transformer.py:73-74);
 * temporal: sequences are the T frames of one (b,s), causal (st_transformer.py:77-78). */
int genie_spatial_attention(const genie_cfg* cfg, const genie_attn_weights* aw, const float* qkv, float* out, int B,
                            void* stream);
int genie_temporal_attention(const genie_cfg* cfg, const genie_attn_weights* aw, const float* qkv, float* out, int B,
                             void* stream);

/* The same core on contiguous sequences: qkv (n_seq, N, 3*H*Dh) -> out (n_seq, N, H*Dh); this is the
 * body of SelfAttention.forward(x, causal) between the qkv and proj Linears (attention.py:38-59) and the
 * shape test_attention.py exercises.  norm_w/norm_b NULL = no qk-norm. */
int genie_attention_core(const float* qkv, float* out, int n_seq, int N, int num_heads, int head_dim, float scale,
                         int causal, const float* norm_w, const float* norm_b, void* stream);

/* STBlock.forward in place on x (B,T,S,d) (st_transformer.py:70-83). */
int genie_st_block_forward(const genie_cfg* cfg, const genie_layer_weights* lw_host, float* x, int B, void* workspace,
                           size_t workspace_bytes, void* stream);
/* STTransformerDecoder.forward in place (st_transformer.py:115-120). */
int genie_decoder_forward(const genie_cfg* cfg, const genie_weights* w, float* x, int B, void* workspace,
                          size_t workspace_bytes, void* stream);

/* out_x_proj (+ muP pre-scale) for frames [t0,t1) (st_mask_git.py:60-61,262-264,316-323). */
int genie_readout_logits(const genie_cfg* cfg, const genie_weights* w, const float* x, int B, int t0, int t1,
                         int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- whole-path entry points ------------------------------------------------------------------------ */

/* STMaskGIT.compute_logits (st_mask_git.py:255-265): ids (B,T,S) -> logits of frames [t0,t1). */
int genie_compute_logits(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int t0, int t1,
                         int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream);
int genie_compute_logits_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int t0, int t1,
                              int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream,
                              const genie_frame_cond* cond);

/* ---- teacher-forced prefix reuse (evaluate.py:107-116 recomputes frames < t in every timeline) -----------------
 * Temporal attention is causal and every other op is per-frame, so in the evaluator's timeline t the activations of
 * the ground-truth frames < t equal those of ONE forward over the ground-truth clip ("clean pass"), and frame t
 * itself only needs their temporal keys/values.
 *   genie_clean_pass: `ids` (B, nframes, S) = clip frames 0..nframes-1; runs that forward and stores every layer's
 *     temporal qkv f32 in `cache`, laid out (L, B, cache_frames, S, 3d) with cache_frames >= nframes (0 = nframes).  The
 *     evaluator needs nframes = cache_frames = T-1 (no timeline has the last frame as context); generate() fills the
 *     prompt's slots of its T-frame KV cache in one pass with nframes = P, cache_frames = T (then genie_frame_pass
 *     continues from slot P).  cache_frames != nframes at B > 1 needs 8 <= nframes <= 16 and head_dim 32/64
 *     (GENIE_E_UNSUPPORTED otherwise: fill the cache with genie_frame_pass instead).
 *   genie_masked_frames_logits: evaluates "frame t in timeline t" for nframes timelines at once: slot i of `frames`
 *     (B, nframes, S) holds the current tokens of clip frame frame0 + i in its own timeline (all-mask at MaskGIT step 0);
 *     it attends the cached keys of clip frames < frame0 + i and its own key.  `cache` comes from a clean pass with the
 *     same nframes; frame0 is 1 (slots = clip frames 1..nframes, the evaluator's case) or 0 (slot 0 = frame 0 seeing
 *     only itself).  logits: token-major (B, nframes, S, V).
 * Same per-row arithmetic as the full forwards: (1 + steps) passes over T-1 frames instead of 15*steps over T.
 * genie_prefix_cache_bytes is the size for nframes = T (an upper bound).
 * The cache is opaque to the caller and only valid for the precision that wrote it: GENIE_PREC_EXACT / _F16X3 store f32;
 * GENIE_PREC_BF16 stores bf16 values (models with T <= 16 and head_dim 32 / 64) in the first half of each layer's slice --
 * the slice strides stay those of the f32 layout, so the size above holds for every precision.
 * A clean pass with cache_frames == nframes < T makes a cache for genie_masked_frames_logits ONLY (a cache genie_frame_pass can
 * continue has T frame slots: cache_frames = T).  For the shipped geometry in GENIE_PREC_BF16 (d 256, 8 heads of 32, fused
 * streams present, 8 <= nframes < T, B * S >= 512) such a cache holds, per (clip, position, head), the K and V operand
 * fragments of the fused temporal kernel instead of qkv rows (csrc/kernels_fused_prefix.hip: both passes run the temporal
 * sub-block as one kernel), and in GENIE_PREC_F16X3 (same geometry, temporal fused_w16 = the genie_pack_temporal_qkv_f16x3
 * stream, 11 <= nframes < T) the f32 k / v accumulators of csrc/kernels_fused_f16x3.hip; producer and consumer decide by the
 * same predicate of (cfg, weights, B, nframes). */
size_t genie_prefix_cache_bytes(const genie_cfg* cfg, int B);
int genie_clean_pass(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int nframes, int cache_frames,
                     float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream);
int genie_clean_pass_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int nframes,
                          int cache_frames, float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond);
int genie_masked_frames_logits(const genie_cfg* cfg, const genie_weights* w, const int64_t* frames, int B, int frame0,
                               int nframes, const float* cache, size_t cache_bytes, float* logits, void* workspace,
                               size_t workspace_bytes, void* stream);
int genie_masked_frames_logits_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* frames, int B,
                                    int frame0, int nframes, const float* cache, size_t cache_bytes, float* logits,
                                    void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond);

/* Temporal KV cache for autoregressive generation (generate.py:81-95 re-runs the full 16-frame forward for every
 * MaskGIT step of every new frame): run ONE frame (frame_ids (B,S), frame index t) through the stack; each layer writes
 * the frame's temporal qkv into slot t of `cache` (same layout as genie_clean_pass) and attends slots 0..t.  Calling
 * it for t = 0..P-1 on the prompt frames fills the cache; for a new frame call it once per MaskGIT step on the current
 * (partially masked) tokens to get `logits` (B,S,V) token-major (NULL = not wanted), and once more on the final tokens
 * to commit them.  Same per-row arithmetic as the full forward restricted to frame t. */
int genie_frame_pass(const genie_cfg* cfg, const genie_weights* w, const int64_t* frame_ids, int B, int t, float* cache,
                     size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream);
int genie_frame_pass_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* frame_ids, int B, int t,
                          float* cache, size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond);
/* The same for nf CONSECUTIVE frames t0 .. t0 + nf - 1 in one pass (ABI 3): frame_ids (B, nf, S); every layer writes the nf
 * cache slots and frame t0 + i attends slots 0 .. t0 + i (those of this pass included); `logits` (B, S, V) token-major are those
 * of the LAST frame of the pass (NULL = not wanted).  generate()'s use: the pass that commits the final tokens of frame t also
 * carries the first MaskGIT step of frame t + 1 (all-mask tokens), so a new frame costs `steps` passes instead of `steps + 1`
 * (generate.py:81-95: the reference recomputes everything per step).  nf == 1 is genie_frame_pass; nf > 1 returns
 * GENIE_E_UNSUPPORTED (nothing enqueued) unless the fragment-order kernels cover the model (GENIE_PREC_F16X3, head_dim 64 or 32,
 * LayerNorm or qk-norm blocks, S 256, vocabulary columns % 64 == 0, frame_w16 streams present, B * nf * S <= 16,384 rows): the caller then
 * runs the frames one by one. */
int genie_frames_pass(const genie_cfg* cfg, const genie_weights* w, const int64_t* frame_ids, int B, int t0, int nf, float* cache,
                      size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream);
int genie_frames_pass_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* frame_ids, int B, int t0, int nf,
                           float* cache, size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes,
                           void* stream, const genie_frame_cond* cond);
/* generate.py:77-103 / STMaskGIT.generate (st_mask_git.py:65-113) on the temporal KV cache, the WHOLE loop enqueued by one call (no
 * host synchronisation, no host work between passes): ids (B, P + n_new, S) = the clip (frames [0, P) are the prompt; frames >= P are
 * read only when teacher_force_time); gen_out (B, n_new, S) receives the generated frames; logits0_out (B, n_new, S, V) f32
 * token-major (or NULL) the step-0 logits of every new frame (what maskgit_generate returns, st_mask_git.py:165,226).  P + n_new <= T.
 * Per new frame: `steps` MaskGIT steps of one-frame passes (genie_frames_pass), genie_sample, genie_mask_step; the commit of frame t
 * shares a two-frame pass with step 0 of frame t + 1 where the library covers it and merge_commit != 0.  noise: the unmasking draws
 * (n_new, steps - 1, B, S) f32 ('random' mode with steps > 1; st_mask_git.py:204-206 draws them with torch.rand_like); uniforms:
 * (n_new, steps, num_factored, B, S) for temperature > 0; both may be NULL otherwise.  cache: genie_prefix_cache_bytes(cfg, B);
 * workspace: genie_generate_workspace_bytes(cfg, B, P) (the loop keeps its token / sample / logits scratch behind the workspace of its
 * largest pass; for models whose T exceeds max(P, 2) genie_workspace_bytes(cfg, B) is that large too).  Same frames as the full-forward
 * schedule (generate.py:81-95) up to f32 accumulation order. */
size_t genie_generate_workspace_bytes(const genie_cfg* cfg, int B, int P);
int genie_generate_cached(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int P, int n_new, int steps,
                          float temperature, int unmask_mode, const float* noise, const float* uniforms, int teacher_force_time,
                          int merge_commit, int64_t* gen_out, float* logits0_out, float* cache, size_t cache_bytes, void* workspace,
                          size_t workspace_bytes, void* stream);
int genie_generate_cached_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int P, int n_new,
                               int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                               int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                               size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                               const genie_frame_cond* cond);
/* The same under a genie_sampling law (NULL = genie_generate_cached_cond); accepts GENIE_UNMASK_CONFIDENCE, whose draws are
 * `noise` (n_new, steps - 1, B, S), required when steps > 1.  The reference's generate has no counterpart of either. */
int genie_generate_cached_ex(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int P, int n_new,
                             int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                             int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                             size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                             const genie_frame_cond* cond, const genie_sampling* sampling);
/* f32 (N, K) row-major weight -> split f16 in FRAGMENT ORDER (2 N K 16-bit values) for the one-frame kernels
 * (csrc/kernels_frame.hip): blocks of 32 rows x 64 k, per block [plane hi | lo'][MFMA step 0..3] fragments of 1 KB = the 64 lanes'
 * 16-byte operand pieces (lane 32 h + r: row r, k = 16 step + 8 h .. + 7), so that every operand load of those kernels is a
 * contiguous 1 KB read.  N % 32 == 0, K % 64 == 0.  Same split as genie_pack_split_f16.
 * Reference counterpart: none (nn.Linear weights are f32: st_transformer.py:16-25, attention.py:27-29, st_mask_git.py:60-61). */
int genie_pack_frame_w16(const float* src, uint16_t* dst, int N, int K, void* stream);
/* y (M, N) f32 = a . w^T + bias on the one-frame kernels, both operands split f16 in fragment order (genie_pack_frame_w16 packs
 * an (M, K) activation the same way as an (N, K) weight): the unit the parity tests and the micro-benchmark call.  mode 0 = the kernel
 * a frame pass of M rows would take, 1 = register-direct kernel (K <= 512), 2 = LDS-tiled kernel (M % 128 == 0, N % 64 == 0).
 * Reference counterpart: nn.Linear.forward (st_transformer.py:16-25, attention.py:27-29). */
int genie_frame_linear(const uint16_t* a_fr, const uint16_t* w_fr, const float* bias, float* y, int M, int N, int K, int mode,
                       void* stream);

/* Factored cross-entropy + accuracy partial sums from token-major or BCTHW logits of frames [t0,t1)
 * (st_mask_git.py:231-253; eval_utils.py:44-77).
 *   targets (B,T,S) int64 (full clip; frames [t0,t1) are read)
 *   weight_ids: if non-NULL (B,T,S) int64, a token counts only where weight_ids == mask id
 *               (STMaskGIT.forward's relevant_mask, st_mask_git.py:276); NULL = every token (compute_loss).
 *   sums_out: 3 doubles, ACCUMULATED: [sum CE, sum (all factors argmax-correct), n tokens counted].  */
int genie_factored_ce(const genie_cfg* cfg, const float* logits, int layout, const int64_t* targets,
                      const int64_t* weight_ids, int B, int t0, int t1, double* sums_out, void* stream);

/* The evaluator's metric vector (evaluate.py:167-179 / eval_utils.py:16-25) as six device-side f64 sums
 *   sums6 = [sum CE, n CE tokens, sum (sample == ground truth), n sampled tokens, n frames, n clips].
 * genie_metric_hits ADDS the number of equal entries of two (batch, n_per_batch) int64 views (batch strides in elements) to
 * sums6[2] (zero it first), writes sums6[3..5] = n_tokens, n_frames, n_clips, and -- when ce3 (the 3-vector
 * genie_factored_ce accumulated on the same stream) is not NULL -- sums6[0] = ce3[0], sums6[1] = ce3[2]. */
int genie_metric_hits(const int64_t* truth, int64_t truth_batch_stride, const int64_t* samples, int64_t samples_batch_stride,
                      int batch, int64_t n_per_batch, const double* ce3, double n_tokens, double n_frames, double n_clips,
                      double* sums6, void* stream);

/* Fused readout + CE for frames [t0,t1) without materialising logits for the caller. */
int genie_readout_ce(const genie_cfg* cfg, const genie_weights* w, const float* x, const int64_t* targets,
                     const int64_t* weight_ids, int B, int t0, int t1, double* sums_out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* MaskGIT sampling half (st_mask_git.py:171-190) on one frame's logits.
 *   logits: (B,S,V) token-major or (B,V,S) BCTHW with nt == 1
 *   temperature <= 1e-8 -> argmax (first max wins); otherwise inverse-CDF sampling with caller-supplied
 *   uniforms (num_factored, B, S) float32, factor order = most significant first (flip(2), :179).
 *   samples (B,S) int64 = hi*Vf + lo;  conf (B,S) float32 = prod p[sample]. */
int genie_sample(const genie_cfg* cfg, const float* logits, int layout, int B, float temperature,
                 const float* uniforms, int64_t* samples, float* conf, void* stream);

/* genie_sample under a genie_sampling law (above).  sampling NULL or all-off and keys_out NULL: genie_sample itself.
 *   keys_out (B,S) float32 or NULL: the GENIE_UNMASK_CONFIDENCE key of every token, log(conf) + sampling->choice_temperature *
 *   anneal * g(noise), written by the same launch; needs noise (B,S) float32 U[0,1); anneal = 1 - (step + 1) / steps.
 *   keys_out may be the conf pointer itself: then only the keys are written.
 * Argument errors (logit_temperature <= 0 or not finite, top_k < 0, NaN top_p, choice_temperature < 0 or NaN, keys_out without
 * noise) return GENIE_E_ARG before anything is enqueued.  Reference counterpart: none beyond st_mask_git.py:171-190. */
int genie_sample_ex(const genie_cfg* cfg, const float* logits, int layout, int B, float temperature, const float* uniforms,
                    int64_t* samples, float* conf, void* stream, const genie_sampling* sampling, float* keys_out,
                    const float* noise, float anneal);

/* genie_sample_ex on guided logits (genie_guidance above): logits_cond / logits_null are the conditional and the null logits of the same
 * B * S tokens, both in `layout`; the guided logit is formed as the kernel loads them (no extra pass, nothing materialised).
 * scale == 1 is exactly genie_sample_ex on logits_cond (logits_null is not read); a non-finite scale returns GENIE_E_ARG before
 * anything is enqueued.  Reference counterpart: none. */
int genie_sample_guided(const genie_cfg* cfg, const float* logits_cond, const float* logits_null, int layout, int B, float temperature,
                        const float* uniforms, int64_t* samples, float* conf, void* stream, const genie_sampling* sampling,
                        float* keys_out, const float* noise, float anneal, float scale);
/* out[i] = (scale * cond[i]) + ((1.0f - scale) * null[i]), i < n: the guided logits materialised (what the guided loops return as the
 * step-0 logits).  out may alias cond or null. */
int genie_guide_logits(const float* cond, const float* null_logits, float* out, size_t n, float scale, void* stream);

/* MaskGIT mask half for one step (st_mask_git.py:192-223), one frame of B clips.
 *   keys (B,S) float32: caller's torch.rand draws ("random") or conf ("greedy"); ignored if last_step
 *   n: tokens to re-mask (ceil(cos(pi/2 (step+1)/steps) S)); unmasked (B,S) uint8 in/out;
 *   samples (B,S) int64 in/out; prompt_frame: pointer to prompt[0, out_t, 0], clip stride in elements.
 *   Writes the final samples back into the prompt frame (in-place semantics of :223). */
int genie_mask_step(const float* keys, int n, int last_step, int64_t mask_id, uint8_t* unmasked, int64_t* samples,
                    int64_t* prompt_frame, int64_t prompt_clip_stride, int B, int S, void* stream);

/* STMaskGIT.maskgit_generate (st_mask_git.py:123-229), whole loop on the device, no host sync.
 *   prompt (B,T,S) int64, frames >= out_t must be all-mask (checked on device: violation sets *status_flag
 *   (device int32, may be NULL) to GENIE_E_ASSERT); prompt[:, out_t] is overwritten in place.
 *   noise: (steps-1, B, S) float32 U[0,1) draws for GENIE_UNMASK_RANDOM (NULL allowed when steps == 1 or greedy)
 *   uniforms: (steps, num_factored, B, S) for temperature > 1e-8, else NULL
 *   samples_out (B,S) int64; logits0_out: step-0 logits of frame out_t in `layout` (NULL = not wanted). */
int genie_maskgit_generate(const genie_cfg* cfg, const genie_weights* w, int64_t* prompt, int B, int out_t, int steps,
                           float temperature, int unmask_mode, const float* noise, const float* uniforms,
                           int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                           void* workspace, size_t workspace_bytes, void* stream);
int genie_maskgit_generate_cond(const genie_cfg* cfg, const genie_weights* w, int64_t* prompt, int B, int out_t, int steps,
                                float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond);
/* The same under a genie_sampling law (NULL = genie_maskgit_generate_cond); accepts GENIE_UNMASK_CONFIDENCE, whose draws are
 * `noise` (steps-1, B, S), required when steps > 1.  The reference has no counterpart of the law or of that mode. */
int genie_maskgit_generate_ex(const genie_cfg* cfg, const genie_weights* w, int64_t* prompt, int B, int out_t, int steps,
                              float temperature, int unmask_mode, const float* noise, const float* uniforms,
                              int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                              void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                              const genie_sampling* sampling);

/* genie_maskgit_generate_ex / genie_generate_cached_ex under classifier-free guidance: the _ex arguments plus a trailing genie_guidance.
 * NULL or scale == 1 is the _ex entry point itself (the null half does not run; cache and workspace as there).  Otherwise the library
 * builds the doubled inputs itself on the stream -- tokens duplicated to 2B clips, actions [cond->ids ; null_action] of shape (2B, T) --,
 * runs the passes of the _ex loop at batch 2B, samples B rows from rows b and b + B of the logits with the guided kernel
 * (genie_sample_guided), runs genie_mask_step on B rows and mirrors the frame's current tokens into the second half before the next pass.
 * noise, uniforms, gen_out / samples_out and logits0_out keep their shapes (per B); logits0_out carries the GUIDED step-0 logits;
 * teacher_force_time and merge_commit keep their meaning, and a pass that 2B clips take out of the fragment-order kernels' coverage
 * (genie_frames_pass) falls back as the unguided loop does at that batch.  Guidance needs a non-NULL cond with n_actions > 0, null_action
 * in [0, n_actions) and a finite scale: GENIE_E_ARG otherwise, nothing enqueued.
 * Sizes under guidance: cache = genie_prefix_cache_bytes(cfg, 2 * B); workspace = genie_generate_guided_workspace_bytes(cfg, B, P), which
 * for any P in [1, T] is also enough for genie_maskgit_generate_guided.  Reference counterpart: none. */
size_t genie_generate_guided_workspace_bytes(const genie_cfg* cfg, int B, int P);
int genie_maskgit_generate_guided(const genie_cfg* cfg, const genie_weights* w, int64_t* prompt, int B, int out_t, int steps,
                                  float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                  int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                  void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                  const genie_sampling* sampling, const genie_guidance* guidance);
int genie_generate_cached_guided(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int P, int n_new,
                                 int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                 size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                 const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance);

/* ---- rollout past the context window (ABI 3 addition; reference counterpart: none -- generate.py:77-103 stops at the window) ----------
 * Positions are absolute (x = token_embed + (pos_embed[t, s] + action_row), genie_frame_cond above), so a frame that moves from slot t to
 * slot t - hop changes its K / V in every layer: the temporal KV cache cannot be shifted.  A slide therefore RE-RUNS the kept context in
 * its new slots, with the prompt sequence of genie_generate_cached (one multi-frame pass, else the clean pass, else frame by frame), and
 * nothing of the cache is reused across a slide.
 * Schedule.  T = cfg->T, prompt 1 <= P <= T - 1, 1 <= keep <= T - 1, hop = T - keep.  Frames are numbered absolutely over the whole rollout;
 * frames [0, P) are the prompt.  A generated frame f >= P belongs to window
 *     j(f) = 0 if f < T, else 1 + (f - T) / hop   (integer division);    start_j = j * hop;    slot(f) = f - start_j
 * (slot in [P, T) for j = 0, in [keep, T) for j >= 1) and is decoded in slot(f) of window j(f): its context is the absolute frames
 * [start_j, f) in slots 0 .. slot(f) - 1, its position rows are pos_embed[slot], and its action and those of its context are the actions
 * of the ABSOLUTE frames.  Inside a window everything is the loop of genie_generate_cached_guided: `steps` one-frame passes, sample and
 * mask step per frame, the commit of slot t merged with step 0 of slot t + 1 where merge_commit is set and the library covers it, and the
 * last slot of a window is never committed.  The first frame of a window (f == P, or f >= T with slot(f) == keep) first has its context
 * run into slots 0 .. slot(f) - 1; its step 0 is then a one-frame pass.
 * Consequence: a rollout of N frames equals, in tokens, bit for bit, in every precision, chaining genie_generate_cached_ex / _guided
 * window by window -- first P prompt frames and min(T - P, N) new ones, then the last `keep` frames as the prompt of min(hop, remaining)
 * new ones --, each call with its window's slice of actions, noise and uniforms.  Cost: `steps` passes per frame plus one keep-frame
 * context pass per hop frames; keep = T - 1 is the true sliding window.
 *   frames (B, cap, S) int64, clip stride cap * S, in/out: [0, P) holds the prompt on entry, [0, f0) must be final; the call generates the
 *     absolute frames [f0, f1), P <= f0 < f1 <= cap, writes each one's final tokens in place and reads its context from the same buffer.
 *   resume 0: the context of f0's window, [start_j(f0), f0), is run from `frames` before f0 is decoded -- always valid; equal to
 *     genie_generate_cached_ex on that window with f0 - start_j prompt frames.  resume 1: `cache` is what a previous call that ended at f0
 *     left behind (slots of [start_j, f0 - 1) committed, frame f0 - 1 pending: a call NEVER commits its last frame); the call then begins
 *     with the commit of f0 - 1 from `frames`, merged with step 0 of f0 by the rule above, so split calls enqueue the passes of one call.
 *     Where f0 is the first frame of a window, resume is ignored and the context is re-run.
 *   steps, temperature, unmask_mode, merge_commit, sampling, guidance: as genie_generate_cached_guided, same argument checks.
 *   noise (f1 - f0, steps - 1, B, S), uniforms (f1 - f0, steps, num_factored, B, S): the draws of the frames of THIS call.
 *   cond: ids is (B, cap) with clip stride `cap` -- the ONE place where the stride is not cfg->T -- and holds the actions of the absolute
 *     frames; entries of frames >= f1 may be read but are never embedded.  One launch per window gathers the window's context tokens and its (NB, T) actions
 *     (slots past cap: action 0, never embedded; under guidance the null half) for the passes, so a whole rollout is enqueued without a
 *     host synchronisation.  There is no teacher_force_time and no logits0_out: neither has a meaning past the window.
 *   cache: genie_prefix_cache_bytes(cfg, NB), NB = 2 B under guidance of scale != 1, else B.
 *   workspace: genie_rollout_workspace_bytes(cfg, B, ctx_max, guided) with ctx_max = the largest context the call runs: max(P, keep) for
 *     rollouts from the prompt and for resumed calls, f0 - start_j for a resume == 0 call in mid-window; >= the generate size of that
 *     context; 0 on bad arguments (ctx_max outside [1, T - 1]).
 * Argument errors return GENIE_E_ARG before anything is enqueued.  Tests: tests/test_rollout_cpu.py, tests/test_hip_rollout.py. */
size_t genie_rollout_workspace_bytes(const genie_cfg* cfg, int B, int ctx_max, int guided);
int genie_rollout_cached(const genie_cfg* cfg, const genie_weights* w, int64_t* frames, int B, int P, int keep, int cap, int f0, int f1,
                         int resume, int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                         int merge_commit, float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                         const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance);

/* ---- fan-out generation: K futures per clip over one shared context cache (ABI 3 addition; reference counterpart: none) ---------------
 * A world model's user holds an observed context and asks what happens under action sequence 1, 2, ... K.  As K extra clips of a batch
 * that costs the context pass K times on identical tokens and K full T-slot caches whose first P slots hold the same bytes.  Here the
 * context of the B clips (NB = 2 B under guidance of scale != 1, else B) runs ONCE into `trunk`, an ordinary cache of NB clips, and the
 * loop of genie_generate_cached_guided then decodes B * K clips, NBK = NB * K per pass, clip i being branch i % K of parent i / K, over a
 * split cache:
 *     slot j <  P  of clip i:   trunk  + ((i / K) * T  +  j     ) * S * 3d      (per layer; read only -- every decode pass has t0 >= P)
 *     slot j >= P  of clip i:   branch + ( i      * Tb + (j - P)) * S * 3d      branch: (L, NBK, Tb, S, 3d) f32, Tb = n_new
 * GENIE_PREC_BF16 with a 16-bit cache keeps its rule in both: 16-bit values in the first half of each layer's slice, slices at the f32
 * strides.  Everything else is that loop: `steps` passes per frame, the commit of slot t merged with step 0 of slot t + 1 where
 * merge_commit is set and the library covers NBK clips (the 16,384-row cut is taken at the pass's own row count), the sampling law, the
 * three unmask modes, guidance (trunk [cond ; null] of 2 B clips, branches [cond B K ; null B K], parent i / K in both halves), no host
 * synchronisation.  In-window only: P + n_new <= T; there is no teacher_force_time and no logits0_out.  K = 1 enqueues the launches of
 * genie_generate_cached_guided with other addresses: same tokens, bit for bit.  In general the tokens equal those of the K-times
 * replicated batch (clip b * K + k = clip b under branch k's actions and draws) through the one-pass loop at NBK clips per pass.
 *   ids (B, P, S): the prompts only.  gen_out (B, K, n_new, S).  noise (n_new, steps - 1, B * K, S), uniforms (n_new, steps, num_factored,
 *   B * K, S): rows of clip b * K + k.
 *   cond->ids (B * K, T), branch-major: row b * K + k, clip stride cfg->T.  The context reads frames < P from row b * K (branch 0); frames
 *   < P of the other branches are never read.  One launch builds the (NB, T) and (NBK, T) ids the passes embed with, null halves included.
 *   trunk: genie_prefix_cache_bytes(cfg, NB); the caller may read the context's K / V there afterwards.
 *   branch: genie_fanout_branch_bytes(cfg, NB, K, n_new) = L * NB * K * n_new * S * 3d * 4; 0 on bad arguments.
 *   workspace: genie_fanout_workspace_bytes(cfg, B, K, P, guided): the larger of the context pass (NB clips, P frames) and a two-frame
 *   pass of NBK clips, plus the loop's scratch; 0 on bad arguments.
 * Argument errors (NULL pointers, K < 1, P + n_new > T, a buffer too small, NB * K beyond 2^30 - 1) return GENIE_E_ARG before anything is
 * enqueued.  A longer horizon continues by handing the B * K results as prompts to genie_rollout_cached.
 * Tests: tests/test_fanout_cpu.py, tests/test_hip_fanout.py. */
size_t genie_fanout_branch_bytes(const genie_cfg* cfg, int NB, int K, int n_new);
size_t genie_fanout_workspace_bytes(const genie_cfg* cfg, int B, int K, int P, int guided);
int genie_generate_fanout(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int K, int P, int n_new, int steps,
                          float temperature, int unmask_mode, const float* noise, const float* uniforms, int merge_commit, int64_t* gen_out,
                          float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance);
/* The decode attention of one layer over that split cache, alone (the `single` kernel family; the fragment-order passes have their own
 * flavour of it): query slot t >= P0 of NBK clips against slots 0..t, out (NBK, S, d) f32 rows.  trunk_slice: (NBK / K, cfg->T, S, 3d),
 * branch_slice: (NBK, Tb, S, 3d); in16 != 0: both hold bf16 values.  K = 1, P0 = 0, Tb = cfg->T reads branch_slice as an ordinary cache
 * (trunk_slice may then be NULL).  Reads only the attention geometry of cfg (heads of 8 are admitted here) and aw->norm_w / norm_b. */
int genie_temporal_attention_decode_fanout(const genie_cfg* cfg, const genie_attn_weights* aw, const float* trunk_slice,
                                           const float* branch_slice, float* out, int NBK, int K, int P0, int Tb, int t, int in16,
                                           void* stream);

/* ---- scoring observed futures: per-branch NLL over the fan-out cache (ABI 3 addition; reference counterpart: none) ---------------------
 * The reverse question of genie_generate_fanout: this is what DID happen -- how likely was it under each of K action hypotheses?
 *     nll[b, k, j] = - sum over the S tokens and the factors of  log softmax(logits_j)[observed token]
 * where logits_j are the MaskGIT step-0 logits of slot P + j with that slot all-mask, slots < P + j holding the OBSERVED tokens, and the
 * actions of branch k: the logits genie_generate_cached_ex(teacher_force_time = 1) returns as logits0_out, and the per-token loss of
 * genie_factored_ce.  Unguided, in-window (P + n <= T).  K = 1 scores each clip of an unconditioned or conditioned model per frame.
 *
 * genie_score_logits: the kernel alone, on token-major logits (N, S, V) of ONE frame (16-byte aligned).  Row i is scored against the S
 *   int64 targets at targets + (i / K) * target_clip_stride (the K branches of a clip share its tokens; targets must lie in
 *   [0, image_vocab_size)).  nll[i * nll_stride] (f64) = the row's NLL; hits[i * nll_stride] (f64, may be NULL) = the number of tokens
 *   whose first-max-wins argmax equals the target in every factor; token_nll[i * token_stride + s] (f32, may be NULL) = each token's
 *   loss.  One wave per token, ce_token_major_kernel's arithmetic (per factor: max, sum of expf(v - max), (logf(sum) + max) - target
 *   logit); the row's sum is taken in f64 in a fixed order inside one workgroup, without atomics: two launches give identical bits.
 * genie_score_fanout: ids (B, P + n, S), the observed clips.  Their P context frames run ONCE into `trunk` as in genie_generate_fanout;
 *   then per slot t = P + j: the all-mask pass of B * K clips over the split cache (riding the commit of slot t - 1 as one two-frame pass
 *   where merge_commit is set and the library covers it, by the rule of genie_generate_cached), the score launch against ids[:, P + j]
 *   of the parent clip, and the commit of the observed tokens (not for the last slot).  No sample or mask-step launches, no draws, no
 *   host synchronisation.  nll, hits (may be NULL): (B, K, n) f64; token_nll (may be NULL): (B, K, n, S) f32.
 *   cond->ids (B * K, T), branch-major, as in genie_generate_fanout.  trunk: genie_prefix_cache_bytes(cfg, B); branch:
 *   genie_fanout_branch_bytes(cfg, B, K, n); workspace: genie_score_workspace_bytes(cfg, B, K, P) (0 on bad arguments).
 *   K = 1 gives, bit for bit, genie_score_logits of the logits0_out of the teacher-forced genie_generate_cached_ex; K > 1 the K = 1
 *   scores of the K-times replicated batch.
 * Argument errors (NULL pointers, K < 1, P < 1, n < 1, P + n > T, a buffer too small) return GENIE_E_ARG before anything is enqueued.
 * Tests: tests/test_score_cpu.py, tests/test_hip_score.py. */
int genie_score_logits(const genie_cfg* cfg, const float* logits, const int64_t* targets, int64_t target_clip_stride, int K, int64_t N,
                       double* nll, int64_t nll_stride, double* hits, float* token_nll, int64_t token_stride, void* stream);
size_t genie_score_workspace_bytes(const genie_cfg* cfg, int B, int K, int P);
int genie_score_fanout(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int K, int P, int n, int merge_commit,
                       double* nll, double* hits, float* token_nll, float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes,
                       void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond);

/* ---- known tokens: inpainting through every MaskGIT decode loop (ABI 3 addition; reference counterpart: none -- st_mask_git.py:155
 * asserts the opposite, that the frame being decoded is all-mask) ---------------------------------------------------------------------
 * Some tokens of a frame are given and only the rest are generated: a partial observation, a counterfactual edit of a region, a crop to
 * complete.  `known` is shaped like the frames a call decodes.  A value v with 0 <= v < image_vocab_size is a known token; ANY other value
 * (image_vocab_size, the mask id, is the conventional one) marks a token to generate.  Values are never inspected on the host.
 * For one frame of clip b let K_b be its number of known tokens and M_b = S - K_b.
 *   1. Start: the frame's current tokens are the known tokens and the mask id elsewhere; unmasked[b, s] = 1 exactly where a token is known.
 *   2. Each step: the pass runs on the current tokens and all S rows are sampled as without known tokens -- noise and uniforms keep their
 *      shapes; draws at known positions have no effect on any output.
 *   3. Mask step of a non-final step: unmasked tokens carry key +inf; n_b = ceil(frac(step) * M_b) with
 *      frac(step) = cos(pi/2 * (step + 1) / steps), computed once on the host in double (genie_mask_fraction, the expression of the
 *      all-mask count) and passed to the kernel, which performs the double multiply and the ceil: host and device agree bit for bit.  The
 *      n_b still-masked tokens of lowest stable rank are re-masked, the rest become unmasked.  K_b = 0 gives the count of genie_mask_step's
 *      callers exactly, ceil(frac * S).  A clip's schedule does not depend on the other clips of its batch.
 *   4. Final step: every still-masked token takes its sample.  The final tokens equal `known` at every known position and never contain
 *      the mask id.
 *   5. A fully known frame (M_b = 0) is legal: its passes still run (the other clips need them, and the slot is committed); its output is
 *      `known`.
 *   6. Merged commits: whenever the two-frame pass of a commit opens slot t (the pending-slot commit of a resumed rollout included), its
 *      second frame carries the start tokens of slot t by rule 1 instead of all-mask.
 *   7. Guidance: both halves of every pass see the same tokens, known ones included.
 *   8. logits0_out rows at known positions are the model's logits at those positions, as for any unmasked input token.
 * genie_known_begin: rule 1 for one frame of B clips in one launch: frame rows b (and b + B when copies == 2) at clip stride
 *   frame_clip_stride, and unmasked (B, S) unless NULL.  A token is known when 0 <= known[b * known_clip_stride + s] < mask_id.
 * genie_mask_step_known: genie_mask_step with the count of rule 3 per clip; known == NULL means M_b = S for every clip.  One block per
 *   clip counts K_b from the clip's known row each step (8 S bytes; the loops' workspace holds no new buffer), S <= 8192.
 * The four loops: the arguments of the widest existing variant plus a trailing genie_known*.  NULL is that variant itself.  Otherwise
 *   ids == NULL or a clip_stride below (frames the call decodes) * S is GENIE_E_ARG before anything is enqueued.  Sizes of cache, trunk,
 *   branch and workspace are those of the variant.
 *   genie_maskgit_generate_known: the frame is out_t (j = 0); prompt[:, out_t:] must still be all-mask on entry (same device check); the
 *     call lays the known tokens itself.  samples_out equals the final prompt frame.
 *   genie_generate_cached_known: j counts the n_new frames.  Under teacher_force_time the committed tokens are the ground truth of `ids`
 *     as before; gen_out still keeps `known`.
 *   genie_rollout_cached_known: j = f - f0, the frames of THIS call, like noise and uniforms.
 *   genie_generate_fanout_known: rows are the B * K branches, row b * K + k.
 * Tests: tests/test_inpaint_cpu.py, tests/test_hip_inpaint.py. */
typedef struct genie_known {
    const int64_t* ids;  /* device; token s of the call's j-th decoded frame of clip b: ids[b*clip_stride + j*S + s] */
    int64_t clip_stride; /* elements, >= (frames the call decodes) * S */
} genie_known;
/* sizeof(genie_known) and the offsets of its two fields, in declaration order: writes min(n, 3) entries, returns 3. */
int genie_known_layout(size_t* out_host, int n);
/* cos(pi/2 * (step + 1) / steps): the host double the loops pass to genie_mask_step_known (0 when steps < 1). */
double genie_mask_fraction(int step, int steps);
int genie_known_begin(const int64_t* known, int64_t known_clip_stride, int64_t mask_id, int64_t* frame, int64_t frame_clip_stride,
                      uint8_t* unmasked /* (B,S) or NULL */, int B, int S, int copies, void* stream);
int genie_mask_step_known(const float* keys, double frac, int last_step, int64_t mask_id, const int64_t* known, int64_t known_clip_stride,
                          uint8_t* unmasked, int64_t* samples, int64_t* prompt_frame, int64_t prompt_clip_stride, int B, int S, void* stream);
int genie_maskgit_generate_known(const genie_cfg* cfg, const genie_weights* w, int64_t* prompt, int B, int out_t, int steps,
                                 float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                 void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                 const genie_sampling* sampling, const genie_guidance* guidance, const genie_known* known);
int genie_generate_cached_known(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int P, int n_new,
                                int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance,
                                const genie_known* known);
int genie_rollout_cached_known(const genie_cfg* cfg, const genie_weights* w, int64_t* frames, int B, int P, int keep, int cap, int f0,
                               int f1, int resume, int steps, float temperature, int unmask_mode, const float* noise,
                               const float* uniforms, int merge_commit, float* cache, size_t cache_bytes, void* workspace,
                               size_t workspace_bytes, void* stream, const genie_frame_cond* cond, const genie_sampling* sampling,
                               const genie_guidance* guidance, const genie_known* known);
int genie_generate_fanout_known(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, int K, int P, int n_new,
                                int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int merge_commit, int64_t* gen_out, float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes,
                                void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                const genie_sampling* sampling, const genie_guidance* guidance, const genie_known* known);

/* ---- optional per-launch timing (bench.py's roofline leg) ------------------------------------------------
 * When enabled, every launch of a kernel whose class bit is set in `class_mask` is bracketed by a pair of
 * HIP events recorded on the launch stream.  genie_profile_read synchronises those events and returns, for
 * one class, out[0..3] = {launches, total milliseconds, total algorithmic FLOPs, total algorithmic bytes}.
 * Process-global, not thread-safe; at most GENIE_PROFILE_MAX_LAUNCHES launches are timed between resets
 * (later ones run untimed and are not counted). */
enum { GENIE_KC_GEMM = 0, GENIE_KC_ATTN_SPATIAL = 1, GENIE_KC_ATTN_TEMPORAL = 2, GENIE_KC_LAYERNORM = 3,
       GENIE_KC_OTHER = 4, GENIE_KC_FUSED = 5 /* fused sub-block kernels (kernels_fused.hip) */, GENIE_KC_COUNT = 6 };
#define GENIE_PROFILE_MAX_LAUNCHES 32768
int genie_profile_enable(int class_mask); /* 0 disables */
int genie_profile_reset(void);
int genie_profile_read(int kernel_class, double* out4);
/* Which kernels the timed launches of one class actually were: one line per distinct kernel,
 * "name\tlaunches\tmilliseconds\tflops\n", written NUL-terminated into buf (truncated at buf_bytes).  bench.py derives
 * roofline.kernel from this instead of assuming the dispatch (a small batch or an override routes elsewhere). */
int genie_profile_kernels(int kernel_class, char* buf, size_t buf_bytes);
/* 1 when the library was compiled with -DGENIE_STUDY (ablation / reduced-precision knobs are live: measurements of such a
 * build are study data, never the product's), 0 for the shipping build, whose launch paths read no such knob. */
int genie_study_build(void);

/* LFQ.get_codebook_entry(...).flip(1) (lookup_free_quantize.py:181-194, visualize.py:115):
 * ids (n, hw) int64 -> z (n, bits, hw) float32 in {-1,+1}, channel c = bit c (LSB first). */
int genie_bits_from_tokens(const int64_t* ids, float* z, int n, int hw, int bits, void* stream);

/* rescale_magvit_output (visualize.py:84-92): u8 = trunc(clamp((x + 1) * 127.5, 0, 255)).  The reference applies
 * it to the decoder's bf16 output with bf16 arithmetic (each op rounds to bf16); `x` holds bf16 bits and the same
 * roundings are reproduced, so the bytes are identical for identical decoder outputs.  n elements. */
int genie_rescale_u8_bf16(const uint16_t* x, uint8_t* out, size_t n, void* stream);
/* f32 variant (no intermediate bf16 rounding), for an f32 decoder. */
int genie_rescale_u8_f32(const float* x, uint8_t* out, size_t n, void* stream);

/* Dataset-compatible LFQ index of an encoder output h (n, bits, hw) f32: id = sum_c [h_c > 0] << c (LSB first;
 * the inverse of genie_bits_from_tokens; cf. lookup_free_quantize.py:241-257 which packs MSB-first and is NOT
 * the dataset convention).  ids (n, hw) int64. */
int genie_tokens_from_bits(const float* h, int64_t* ids, int n, int hw, int bits, void* stream);

/* ---- MAGVIT2 decoder convolutions (improved_model.py:12-51, 124-237), activations NHWC bf16, f32 accumulate ------
 * genie_pack_conv_weight: (C_out, C_in, kh*kw) f32 torch layout -> (C_out, kh*kw, C_in) bf16 (tap-major K).
 * genie_conv3x3_bf16: 3x3 / pad 1 / stride 1 implicit GEMM on the bf16 matrix cores; C_in %% 64 == 0, C_out %% 8 == 0 (%% 32 with depth-to-space);
 *   residual (same shape as the output) is added before the bf16 store (ResBlock skip); depth_to_space != 0 writes
 *   the Upsampler's DCR-permuted (n, 2H, 2W, C_out/4) image; zero_page: >= 16 zero bytes for out-of-image taps.
 * genie_conv1x1_bf16: the 1x1 nin_shortcut (a plain Linear over pixels).
 * genie_conv_direct_bf16: direct 3x3 conv for the edge layers (C_in = 18 -> 512, 128 -> 3); out_mode 0 = NHWC bf16,
 *   1 = NCHW f32.
 * genie_group_norm_swish_bf16: GroupNorm(groups, eps) [+ x*sigmoid(x)] of an NHWC bf16 image (improved_model.py:24-34);
 *   stats_ws: genie_group_norm_scratch_floats(n, HW, groups) f32 of scratch.  The statistics are reduced in a fixed order
 *   (no atomics): the same input gives the same bytes on every call.
 * genie_bits_from_tokens_nhwc_bf16: tokens (n_pix) -> (n_pix, cpad) bf16: channel c < bits = +-1 for bit c (a18 in
 *   operand layout), channels >= bits zero (cpad %% 64 == 0 lets conv_in run on the implicit GEMM).
 * genie_rescale_u8_nhwc_bf16: decoder tail: (n, HW, cpad) bf16 -> (n, cout, HW) uint8 with the reference's bf16 rescale.
 * Tests: tests/test_hip_conv.py holds every entry point of this section to the plain references of tests/conv_reference.py (f64 conv2d /
 *   matmul / group_norm, bit-exact NumPy tokenizer ends; pinned on the CPU by tests/test_conv_reference_cpu.py) and checks that an image's
 *   bytes do not depend on the rest of the batch; tests/test_hip_harness.py: the decoder / encoder stacks against the reference's goldens. */
int genie_pack_conv_weight(const float* w, uint16_t* out, int Cout, int Cin, int taps, void* stream);
int genie_conv3x3_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* residual, uint16_t* y,
                       const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, int depth_to_space, void* stream);
/* The encoder's downsample: 3x3 / pad 1 / stride 2 (improved_model.py:90); H, W are the OUTPUT size, input is (2H, 2W).
 * Tests: tests/test_hip_conv.py::test_conv3x3_s2_against_f64. */
int genie_conv3x3_s2_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, uint16_t* y,
                          const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, void* stream);
/* Encoder ends: uint8 frames (n, cin, HW) -> (n, HW, cpad) bf16 in [-1,1] (x/127.5 - 1; channels >= cin zero), and the
 * encoder code (n_pix, cpad) bf16 -> dataset-convention token ids, bit c = [h_c > 0]. */
int genie_frames_to_nhwc_bf16(const uint8_t* frames, uint16_t* x, int n, int HW, int cin, int cpad, void* stream);
int genie_tokens_from_code_nhwc_bf16(const uint16_t* h, int64_t* ids, int64_t n_pix, int bits, int cpad, void* stream);
int genie_conv1x1_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, uint16_t* y, int n_pix, int Cin,
                       int Cout, void* stream);
int genie_conv_direct_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, void* y, int n, int H, int W,
                           int Cin, int Cout, int out_mode, void* stream);
size_t genie_group_norm_scratch_floats(int n, int HW, int groups);
int genie_group_norm_swish_bf16(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* stats_ws, int n,
                                int HW, int C, int groups, float eps, int apply_swish, void* stream);
/* GroupNorm statistics fused into the producing convolution ("fused GN+swish").
 * genie_conv3x3_gn_bf16 = genie_conv3x3_bf16 / genie_conv3x3_s2_bf16 (stride 1 or 2) that also writes, per 256-pixel x
 *   128-channel output tile, the (sum, sumsq) of the STORED bf16 output for each GroupNorm(groups) group of the tile
 *   (gn_part: genie_conv_gn_part_floats(n, H, W, Cout) floats; fixed reduction order, no atomics).  Needs H*W %% 256 == 0,
 *   C_out %% 128 == 0 and groups of 4, 8 or 16 channels; returns GENIE_E_UNSUPPORTED otherwise
 *   without launching, and the caller uses the separate-statistics path.
 * genie_group_norm_swish_fused_bf16: GroupNorm(groups, eps) [+ swish] of that convolution's output x from its partials:
 *   no statistics pass over x.  H, W, Cout, depth_to_space are the CONVOLUTION's; stats_ws: n * groups * 2 floats.
 * Tests: tests/test_hip_harness.py::test_conv_fused_groupnorm_statistics (against the separate pass and f64 group_norm);
 *   tests/test_hip_conv.py (same bytes as the plain convolution, refusal without a write, batch invariance). */
size_t genie_conv_gn_part_floats(int n, int H, int W, int Cout);
int genie_conv3x3_gn_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* residual, uint16_t* y,
                          const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, int depth_to_space, int stride,
                          float* gn_part, int groups, void* stream);
int genie_group_norm_swish_fused_bf16(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y,
                                      const float* gn_part, float* stats_ws, int n, int H, int W, int Cout, int depth_to_space,
                                      int groups, float eps, int apply_swish, void* stream);
int genie_bits_from_tokens_nhwc_bf16(const int64_t* ids, uint16_t* z, int64_t n_pix, int bits, int cpad, void* stream);
int genie_rescale_u8_nhwc_bf16(const uint16_t* x, uint8_t* out, int n, int HW, int cpad, int cout, void* stream);

/* ---- training step (train.py:600-633) -------------------------------------------
 * All three precisions; both the LayerNorm (qk_norm = false, the shipped config) and the qk-norm block variants.
 * GENIE_PREC_EXACT: every contraction on the f32 matrix instruction.  GENIE_PREC_F16X3 / GENIE_PREC_BF16: every
 * Linear product (forward, input gradient, weight gradient) on the 16-bit matrix cores with f32 accumulation --
 * f16x3 keeps f32-class gradients (split operands), bf16 is what `accelerate --mixed_precision bf16` computes --
 * while LayerNorm, both attention cores, GELU, the residual stream, the loss and every gradient reduction stay f32.
 * The 16-bit precisions need 16-bit copies of the Linear weights in both orientations (genie_train_pack_weights,
 * again after every optimizer step); parameters, gradients and optimizer state are always f32.  Gradients travel in a second genie_weights table whose pointers address the caller's
 * gradient buffers (same shapes as the parameters; the *_w16 members are ignored).  `accumulate` = 0 overwrites the
 * gradients (optimizer.zero_grad() + backward), 1 adds to them (gradient accumulation, train.py:607-617).
 * GENIE_PREC_F16X3 splits the gradient operands of those products as 2^12 times their value (undone in the accumulator's scale), so
 * that gradients far below the f16 normal range keep all 22 bits; a gradient element of magnitude 16 or more saturates there.
 * Every reduction feeding a gradient has a fixed order: results are bit-reproducible run to run.
 * Geometry the step admits (checked by every entry point before anything is enqueued, GENIE_E_SHAPE otherwise): head_dim 32
 * or 64 (head_dim 16 is inference only: the temporal attention backward and the qk-norm backward have no such kernel), T <= 64
 * (a power of two, by genie_check_config), S, d_model and hidden multiples of 16; the 16-bit precisions also need d_model, hidden, T * S and the vocabulary rows to be
 * multiples of 64. */

/* Bytes of the saved-activation buffer / of the backward scratch for B clips. */
size_t genie_train_activation_bytes(const genie_cfg* cfg, int B);
size_t genie_train_workspace_bytes(const genie_cfg* cfg, int B);

/* STMaskGIT.forward in training mode (st_mask_git.py:267-279; without dropout -- mlp_drop > 0 is genie_train_forward_drop below): embeds
 * input_ids (B,T,S), runs the L blocks keeping what the backward needs, the readout, and the masked factored CE of
 * compute_loss_and_acc (:231-253) against labels (B,T,S).  sums_out (3 doubles, overwritten) =
 * [sum CE over counted tokens, sum (all factors argmax-correct), n counted] with counted = frame >= 1 and
 * input id == mask id; loss = sums[0]/sums[2], acc = sums[1]/sums[2] (0/0 = nan as in the reference).
 * On return the logits slot of `acts` holds d loss / d logits. */
int genie_train_forward(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                        int B, float* acts, size_t acts_bytes, double* sums_out, void* stream);
int genie_train_forward_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                             int B, float* acts, size_t acts_bytes, double* sums_out, void* stream,
                             const genie_frame_cond* cond);

/* 16-bit precisions only: refresh the 16-bit copies of every Linear weight from the f32 parameters in `w`:
 * row-major (out, in) into the *_w16 members of `w16` (read by the forward) and transposed (in, out) into the *_w16
 * members of `w16T` (read by the input-gradient products; pass it as `wT` below, NULL for GENIE_PREC_EXACT).
 * bf16: one plane; f16x3: [hi | lo] planes as genie_pack_split_f16. */
int genie_train_pack_weights(const genie_cfg* cfg, const genie_weights* w, const genie_weights* w16,
                             const genie_weights* w16T, void* stream);

/* loss.backward() (train.py:617), split so that the caller can all-reduce finished gradients while earlier layers
 * are still running: head (readout weight/bias, d loss / d x_L into the workspace), then layers L-1 .. 0 (each
 * consumes and replaces the running d loss / d x in the workspace), then the embedding tables, mask embedding and
 * pos_embed.  Must be called in exactly that order on one stream after genie_train_forward. */
int genie_train_backward_head(const genie_cfg* cfg, const genie_weights* w, const genie_weights* wT,
                              const genie_weights* grads, int B, float* acts, void* workspace, size_t workspace_bytes,
                              int accumulate, void* stream);
int genie_train_backward_layer(const genie_cfg* cfg, const genie_weights* w, const genie_weights* wT,
                               const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                               size_t workspace_bytes, int accumulate, void* stream);
int genie_train_backward_embed(const genie_cfg* cfg, const genie_weights* grads, const int64_t* input_ids, int B,
                               void* workspace, size_t workspace_bytes, int accumulate, void* stream);
/* ... and, with actions, the gradient of the action table into d_table (n_actions, d_model): the sum over the frames whose
 * action is k of their tokens' d loss / d x, in a fixed order (no atomics); rows of unused actions are 0 (or kept with
 * `accumulate`).  Its scratch is a region of the training workspace that is dead by then (same workspace size). */
int genie_train_backward_embed_cond(const genie_cfg* cfg, const genie_weights* grads, const int64_t* input_ids, int B,
                                    void* workspace, size_t workspace_bytes, int accumulate, void* stream,
                                    float* d_table, const genie_frame_cond* cond);

/* Activation recomputation (additions; nothing above changes).  The *_ex forms take `recompute`: 0 is the entry point of the same
 * name without _ex (every intermediate of every layer is saved); 1 keeps only each layer's f32 input (L checkpoints of B*T*S*d_model
 * floats), one layer's worth of intermediates that every layer reuses, and the tail (final x, logits), and
 * genie_train_backward_layer_ex first rebuilds layer `layer`'s intermediates from its checkpoint with the forward's own kernels
 * (all but the second MLP product, whose output no backward reads).  Those kernels are bit-reproducible: losses and every gradient
 * are the same bits as with recompute = 0, for about one more layer forward (less fc2) per layer of time.  With recompute = 1
 *     genie_train_activation_bytes_ex(cfg, B, 1) <= genie_train_activation_bytes(cfg with num_layers = 1, B)
 *                                                   + num_layers * roundup256(B*T*S*d_model*4),
 * the workspace size is that of recompute = 0, and EVERY genie_train_backward_layer_ex call overwrites the shared intermediates:
 * the order stays forward, head, layers L-1 .. 0, embed, all with the same `recompute` and buffers sized for it.
 * genie_train_backward_embed[_cond] does not read the activation buffer and serves both modes.  Any other `recompute`: the size
 * functions return 0, the others GENIE_E_ARG before any other check. */
size_t genie_train_activation_bytes_ex(const genie_cfg* cfg, int B, int recompute);
size_t genie_train_workspace_bytes_ex(const genie_cfg* cfg, int B, int recompute);
int genie_train_forward_ex(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                           int B, float* acts, size_t acts_bytes, double* sums_out, void* stream,
                           const genie_frame_cond* cond, int recompute);
int genie_train_backward_head_ex(const genie_cfg* cfg, const genie_weights* w, const genie_weights* wT,
                                 const genie_weights* grads, int B, float* acts, void* workspace, size_t workspace_bytes,
                                 int accumulate, void* stream, int recompute);
int genie_train_backward_layer_ex(const genie_cfg* cfg, const genie_weights* w, const genie_weights* wT,
                                  const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                                  size_t workspace_bytes, int accumulate, void* stream, int recompute);

/* MLP dropout in the training step (additions; nothing above changes).  Reference: st_transformer.py:22-25 and :81, one
 * nn.Dropout(mlp_drop) behind the GELU (site 0) and behind fc2 (site 1):
 *     h  = m0 * s * gelu(fc1(u2))           (M, hidden)
 *     x3 = x2 + m1 * s * (fc2(h) + b2)      (M, d_model)          s = 1 / (1 - p) in f32, keep masks m in {0, 1}
 * Training only: no inference entry point takes a genie_dropout.  The masks are never stored: every kernel that applies one makes it
 * in registers from Philox4x32-10 with
 *     key = (seed low 32, seed high 32),  counter = (g low 32, g high 32, layer * 2 + site, call),  g = e / 4,
 * whose four output words serve elements 4g .. 4g + 3; e is the row-major index into the (M, hidden) or (M, d_model) matrix with
 * token-major rows, M = B*T*S.  Element e is kept iff its word >= floor((double)p * 2^32): integers only, bit-exact in NumPy.
 * `call` is the caller's micro-batch counter; under data parallelism the caller adds its rank to the seed.
 * The *_drop forms take the arguments of the *_ex forms and the struct: dr == NULL or dr->p == 0 is the *_ex call itself (same
 * launches, same bits); p < 0, p >= 1 or NaN: GENIE_E_ARG before any other check.  The forward and every backward_layer call of one
 * step get the same struct, in both `recompute` modes (the recomputation draws the forward's masks again: same gradient bits as
 * recompute = 0).  Head and embed backward do not depend on it.  Buffer sizes are those of the *_ex forms: the two passes' scratch
 * are regions that are dead when they run.  The struct is read on the host during the call. */
typedef struct genie_dropout {
    float p;         /* drop probability, 0 <= p < 1 */
    uint32_t call;   /* counter word 3 */
    uint64_t seed;   /* Philox key */
} genie_dropout;
/* sizeof(genie_dropout) and the offsets of p, call, seed: writes min(n, 4) entries, returns 4. */
int genie_dropout_layout(size_t* out_host, int n);
/* keep[e] = 1 / 0 for e in [0, n): the mask of (layer, site) under *dr, as the step's kernels draw it (a window for tests; the step
 * never materialises a mask).  p = 0 keeps everything.  NULL dr, a bad p, layer < 0, site not 0 / 1, n < 0: GENIE_E_ARG. */
int genie_dropout_mask(const genie_dropout* dr, int layer, int site, int64_t n, uint8_t* keep, void* stream);
int genie_train_forward_drop(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                             int B, float* acts, size_t acts_bytes, double* sums_out, void* stream,
                             const genie_frame_cond* cond, int recompute, const genie_dropout* dr);
int genie_train_backward_layer_drop(const genie_cfg* cfg, const genie_weights* w, const genie_weights* wT,
                                    const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                                    size_t workspace_bytes, int accumulate, void* stream, int recompute,
                                    const genie_dropout* dr);

/* Training objective (additions; nothing above changes): label smoothing eps, z-loss zeta and per-frame loss weights w_t in the fused
 * loss kernel.  A token n in frame t is counted iff t >= 1 and its input id is the mask id (the rule above).  For a counted token and
 * factor f with logits z (vf values) and target y:
 *     lse   = max + log sum_k exp(z_k - max)
 *     nll_f = lse - z_y
 *     l_f   = (1 - eps) nll_f + eps (lse - (1/vf) sum_k z_k) + zeta lse^2          l_n = sum_f l_f
 *     p_k   = exp(z_k - lse),   q_k = (1 - eps) [k = y] + eps / vf
 *     d l_f / d z_k = p_k (1 + 2 zeta lse) - q_k
 * (the first two terms are F.cross_entropy(label_smoothing = eps) per factor).  With frame weights w_0 .. w_{T-1} (w_0 is never used;
 * all ones by default):
 *     c_t  = number of counted tokens in frame t (integers, exact)
 *     W    = sum_t (double) w_t c_t   (t ascending),        n = sum_t c_t
 *     loss = sum_counted w_t l_n / W
 *     d loss / d z_k = (float)((double) w_t / W) d l_f / d z_k
 * Uncounted tokens and counted tokens with w_t = 0 get a zero row and are never multiplied by 1 / W; W = 0 with n > 0 gives loss NaN
 * (0/0, as the empty mask above) and all-zero gradients.  The sums buffer holds FIVE doubles
 *     [sum w l, sum hits, W, sum plain nll, n]        loss = s0 / s2,  acc = s1 / s4,  ce = s3 / s4
 * with hits (all factors argmax-correct) and the plain nll (l_n at eps = zeta = 0) taken over ALL counted tokens whatever their
 * weight, so that acc and ce stay comparable between runs with different objectives and with the evaluators.  f32 in all three
 * precisions; per token nll is evaluated as (logf(se) + max) - z_y and an element as (p (1 + 2 zeta lse) - q) wgt, in the summation
 * order of the neutral kernel: with eps = zeta = 0 and all weights 1 the rows are that kernel's bits.  d logits has a fixed summation
 * order and no atomics (the same bytes run to run); the three loss sums are accumulated with double atomics, as the neutral step's.
 * Neutral means eps == 0, zeta == 0 and n_frames == 0.  The struct is read on the host during the call; the weights travel in the
 * kernel arguments (no copy, no sync).  Refused with GENIE_E_ARG before any other check: eps outside [0, 1) or NaN; zeta negative
 * or not finite; n_frames neither 0 nor T; a negative or non-finite weight among the first n_frames. */
typedef struct genie_objective {
    float label_smoothing;   /* eps, 0 <= eps < 1 */
    float z_loss;            /* zeta >= 0 */
    int32_t n_frames;        /* 0 = all frames weigh 1, else == T */
    int32_t reserved;        /* 0 */
    float frame_weight[64];  /* w_t, t < n_frames */
} genie_objective;
/* sizeof(genie_objective) and the offsets of its five fields, in declaration order: writes min(n, 6) entries, returns 6. */
int genie_objective_layout(size_t* out_host, int n);
/* genie_train_forward_drop with the objective: the same arguments and `obj`; sums_out always has room for five doubles.  obj == NULL
 * or neutral: the call IS the _drop call (same launches, same bits, only three doubles written).  Else the five sums above, and the
 * logits slot holds d loss / d logits of this objective: head, layers and embed backward are untouched (recomputation and dropout
 * compose as they are). */
int genie_train_forward_obj(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                            int B, float* acts, size_t acts_bytes, double* sums_out, void* stream,
                            const genie_frame_cond* cond, int recompute, const genie_dropout* dr, const genie_objective* obj);
/* The loss launch alone on caller-owned logits (n_clips, T, S, nfac * vf) f32, replaced by d loss / d logits; ids and labels
 * (n_clips, T, S) int64; no genie_cfg and no geometry limits beyond vf >= 1 and 1 <= nfac <= 4 (n_frames == T needs T <= 64).
 * obj == NULL: the neutral step's own kernels, sums_out = its three doubles.  obj != NULL: always the general kernels, also at
 * neutral values, five doubles.  sums_out is overwritten.  A NULL pointer, n_clips, T, S or vf < 1, nfac outside 1 .. 4, or (obj ==
 * NULL) a mask_id beyond int32: GENIE_E_ARG, nothing enqueued. */
int genie_ce_objective(float* logits, const int64_t* ids, const int64_t* labels, int n_clips, int T, int S, int vf, int nfac,
                       int64_t mask_id, const genie_objective* obj, double* sums_out, void* stream);

/* Distillation (additions; nothing above changes): soft targets from a teacher's logits in the fused loss kernel.  The counted-token rule,
 * the frame weights, c_t, W, n and the (float)((double) w_t / W) gradient scale are those of "Training objective".  For a counted token and
 * factor f with student logits z (vf values), teacher logits u (vf values; f32, token-major, the student's (n_clips, T, S, nfac * vf)
 * shape), target y, mix alpha in [0, 1] and temperature tau > 0:
 *     lse    = logsumexp(z)                    p_k  = exp(z_k - lse)
 *     pt_k   = softmax(z / tau)_k              r_k  = softmax(u / tau)_k
 *     hard_f = (1 - eps) (lse - z_y) + eps (lse - mean_k z_k)                      (the smoothed CE above)
 *     kd_f   = tau^2 sum_k r_k (log r_k - log pt_k)                                (tau^2 KL(r || pt), Hinton et al. 2015)
 *     l_f    = (1 - alpha) hard_f + alpha kd_f + zeta lse^2                        l_n = sum_f l_f
 *     d l_f / d z_k = (1 - alpha)(p_k - q_k) + 2 zeta lse p_k + alpha tau (pt_k - r_k)
 * with q the smoothed target above: at alpha = 0 the formula of "Training objective", term for term.  log r_k and log pt_k are evaluated in
 * log-softmax form, (u_k - max u) / tau - log sum_j exp((u_j - max u) / tau), never as the log of a probability: a class whose r_k
 * underflowed to 0 contributes 0.  Logits are finite.  The sums buffer holds SEVEN doubles
 *     [sum w l, sum hits, W, sum plain nll, n, sum plain kd, sum teacher plain nll]
 *     loss = s0 / s2,  acc = s1 / s4,  ce = s3 / s4,  kd = s5 / s4,  teacher_ce = s6 / s4
 * entries 5 and 6 over ALL counted tokens whatever their weight, as hits and the plain nll: kd is the unweighted tau^2 KL per token, and
 * teacher_ce the teacher's own cross-entropy sum_f (logsumexp(u) - u_y) on the same tokens -- the cheap check that the teacher is wired
 * to the same ids, layout and vocabulary order.  f32 in all three precisions: per lane and factor, with inv_tau = 1.0f / tau,
 * d = (z - max z) [* inv_tau], c = (u - max u) [* inv_tau] (the products only when tau != 1), kd_f = (tau * tau) * wave sum of
 * r ((c - d) - (log su - log st)), an element ((1 - alpha)(p - q) + (2 zeta lse) p + (alpha tau)(pt - r)) wgt; tests/distill_model.py
 * restates the order.  The student logits are replaced by d loss / d logits; the teacher logits are read only.  Fixed summation order and
 * no atomics on d logits (the same bytes run to run); the five accumulated sums use double atomics.
 * Neutral means ds == NULL or alpha == 0: the call of before, and the teacher pointer is never dereferenced.  A struct that is given is
 * validated BEFORE the neutral shortcut is taken: alpha == 0 with a temperature <= 0 is refused, not passed on.  The struct is read on the
 * host during the call.  Refused with GENIE_E_ARG before anything is enqueued: alpha outside [0, 1] or NaN; a temperature that is not
 * finite or <= 0; alpha > 0 with a NULL teacher pointer; teacher logits that overlap the student logits or the seven sums; and
 * everything "Training objective" refuses. */
typedef struct genie_distill {
    float alpha;                  /* mix, 0 <= alpha <= 1; 0 = no distillation */
    float temperature;            /* tau > 0 */
    const float* teacher_logits;  /* (n_clips, T, S, nfac * vf) f32 on the device, read only */
} genie_distill;
/* sizeof(genie_distill) and the offsets of alpha, temperature, teacher_logits: writes min(n, 4) entries, returns 4. */
int genie_distill_layout(size_t* out_host, int n);
/* genie_train_forward_obj with distillation: the same arguments and `ds`; sums_out always has room for seven doubles.  ds == NULL or
 * alpha == 0: the call IS the _obj call (same launches, same bits, three or five doubles written).  Else the seven sums above, and the
 * logits slot holds d loss / d logits of the mixed loss: head, layers and embed backward are untouched (recomputation, dropout, frozen
 * tensors and accumulation compose as they are). */
int genie_train_forward_distill(const genie_cfg* cfg, const genie_weights* w, const int64_t* input_ids, const int64_t* labels,
                                int B, float* acts, size_t acts_bytes, double* sums_out, void* stream,
                                const genie_frame_cond* cond, int recompute, const genie_dropout* dr, const genie_objective* obj,
                                const genie_distill* ds);
/* The loss launch alone on caller-owned buffers, the counterpart of genie_ce_objective (its geometry freedom; obj == NULL: eps = zeta = 0,
 * all frames weigh 1).  The teacher rows are `teacher_logits`; alpha and temperature come from `ds`, whose own pointer is not read.
 * ds == NULL or alpha == 0: the call IS genie_ce_objective(logits, ids, labels, ..., obj, sums_out, stream).  Else seven doubles,
 * overwritten. */
int genie_ce_distill(float* logits, const float* teacher_logits, const int64_t* ids, const int64_t* labels, int n_clips, int T, int S,
                     int vf, int nfac, int64_t mask_id, const genie_objective* obj, const genie_distill* ds, double* sums_out,
                     void* stream);

/* The temporal (causal, over the T frames of one spatial position) attention backward of the step, alone -- the counterpart of
 * genie_attention_core for the backward; f32 in every precision.  qkv (B,T,S,3*d_model) is the saved q | k | v; qk holds the q | k the
 * scores were made from, q at column 0 and k at column d_model of rows of qk_ld floats: qkv itself (qk_ld = 3*d_model) or the
 * qk-norm copies (qk_ld = 2*d_model); d_out (B,T,S,d_model) is d loss / d (attention output).  d_qkv (B,T,S,3*d_model) is
 * OVERWRITTEN with dq | dk | dv (with qk-norm: the gradients of the normalised q, k):
 *     p = softmax_j(scale q_i.k_j), j <= i;  dp = d_out_i.v_j;  ds = p (dp - sum_j p dp);
 *     dq = scale ds K;  dk = scale ds^T Q;  dv = p^T d_out
 * in a fixed summation order, no atomics: the same bytes run to run.  T <= 64 and a power of two; T = 32 / 64 need head_dim 32
 * or 64, T <= 16 also admits 128.  NULL pointers or B <= 0: GENIE_E_ARG; T > 64 or not a power of two, head_dim * num_heads !=
 * d_model, qk_ld not 2*d_model or 3*d_model: GENIE_E_SHAPE -- both before the device or the stream is touched. */
int genie_temporal_attention_backward(const float* qkv, const float* qk, int64_t qk_ld, const float* d_out,
                                      float* d_qkv, int B, int T, int S, int d_model, int num_heads, int head_dim,
                                      float scale, void* stream);

/* The spatial (non-causal, over the S tokens of one frame) attention backward of the step, alone, by the implementation `path`
 * names.  qkv (n_frames,S,3*d_model) is the saved q | k | v; qk, qk_ld and d_out (n_frames,S,d_model) as above; d_qkv
 * (n_frames,S,3*d_model) is OVERWRITTEN with dq | dk | dv:
 *     p = softmax_j(scale q_i.k_j);  dp = d_out_i.v_j;  ds = p (dp - sum_j p dp);
 *     dq = scale ds K;  dk = scale ds^T Q;  dv = p^T d_out
 * in a fixed summation order, no atomics: the same bytes run to run.  This is the dispatch the training step runs: the step passes
 * GENIE_SPATIAL_BWD_BF16 in the bf16 precision where that path takes the geometry and GENIE_SPATIAL_BWD_AUTO everywhere else.
 *   AUTO          f32: FUSED where it takes the geometry, else MATERIALISED
 *   FUSED         one f32 kernel, nothing of size S x S in memory; S = 256 and head_dim 32 / 64
 *   MATERIALISED  f32 scores in the workspace (five batched GEMMs and a row softmax pair); every S, head_dim that are multiples of 16
 *   BF16          the two kernels of the bf16 precision (operands of every product rounded to bf16, f32 accumulation and softmax);
 *                 S = 256 and head_dim 32 / 64
 * genie_spatial_attention_backward_workspace_bytes: what `workspace` must hold for that path (0: none, workspace may be NULL; AUTO
 * answers for MATERIALISED, which covers either outcome; an unknown path, n_frames, S or num_heads <= 0: 0).
 * NULL qkv / qk / d_out / d_qkv, n_frames <= 0, a non-positive dimension, an unknown path: GENIE_E_ARG; S or head_dim not a multiple of
 * 16, head_dim * num_heads != d_model, qk_ld not 2*d_model or 3*d_model: GENIE_E_SHAPE; FUSED or BF16 outside their geometry:
 * GENIE_E_UNSUPPORTED; a workspace smaller than the path taken needs (or NULL where it needs one): GENIE_E_ARG -- all before the
 * device or the stream is touched, d_qkv untouched. */
enum { GENIE_SPATIAL_BWD_AUTO = 0, GENIE_SPATIAL_BWD_FUSED = 1, GENIE_SPATIAL_BWD_MATERIALISED = 2, GENIE_SPATIAL_BWD_BF16 = 3 };
size_t genie_spatial_attention_backward_workspace_bytes(int path, int n_frames, int S, int num_heads);
int genie_spatial_attention_backward(const float* qkv, const float* qk, int64_t qk_ld, const float* d_out, float* d_qkv,
                                     int n_frames, int S, int d_model, int num_heads, int head_dim, float scale, int path,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* qk-norm (LayerNorm over head_dim of every q and k head row, eps 1e-5, ONE affine norm_w / norm_b (head_dim) shared by q, k and all
 * heads), alone; head_dim 32 / 64 / 128 (others: GENIE_E_UNSUPPORTED), d_model = num_heads * head_dim.
 * genie_qk_norm_forward: qkv (rows,3*d_model) -> qkn (rows,2*d_model) = [LN(q) | LN(k)], the operands the attention backwards read with
 * qk_ld = 2*d_model.
 * genie_qk_norm_backward: d_qkv (rows,3*d_model) holds d loss / d (normalised q | k) in its q | k columns and is turned IN PLACE into
 * d loss / d (raw q | k); its v columns are neither read nor written.  d_norm_w / d_norm_b (head_dim) receive the affine's gradient
 * summed over rows, q and k, and heads (accumulate != 0: added to what they hold; 0: overwritten), in a fixed order.  A NULL d_norm_w
 * or d_norm_b is a frozen tensor ("Frozen tensors" above): nothing is written for it; both NULL: no reduction runs and `scratch` is not
 * touched (it may be NULL).  Otherwise scratch holds genie_qk_norm_backward_scratch_bytes(head_dim) bytes (0 for an unsupported
 * head_dim).
 * NULL qkv / qkn / norm_w / norm_b / d_qkv, rows, num_heads or head_dim <= 0, a scratch that is too small: GENIE_E_ARG, before the
 * device or the stream is touched. */
int genie_qk_norm_forward(const float* qkv, float* qkn, const float* norm_w, const float* norm_b, int64_t rows, int num_heads,
                          int head_dim, void* stream);
size_t genie_qk_norm_backward_scratch_bytes(int head_dim);
int genie_qk_norm_backward(const float* qkv, float* d_qkv, const float* norm_w, float* d_norm_w, float* d_norm_b, int64_t rows,
                           int num_heads, int head_dim, int accumulate, void* scratch, size_t scratch_bytes, void* stream);

/* *out += sum x[i]^2 in f64, two-stage with a fixed order (scratch: 1024 doubles).  The global gradient norm of
 * clip_grad_norm_ (train.py:628-629) is sqrt of this summed over all gradient buffers. */
int genie_sumsq(const float* x, size_t n, double* out, double* scratch, void* stream);

/* torch.optim.AdamW.step() on one flat range (train.py:440-441, 631): decoupled decay p *= 1 - lr*wd, then the
 * bias-corrected Adam update; `step` counts from 1.  The gradient is first multiplied by grad_mult (1/world_size
 * after a SUM all-reduce, 1/accumulation steps) and, when grad_sumsq != NULL and max_grad_norm > 0, by
 * min(1, max_grad_norm / (grad_mult * sqrt(*grad_sumsq) + 1e-6)) -- clip_grad_norm_ without a host sync.
 * The reference's grouping (train.py:426-437) is the caller's: weight_decay = 0 for names containing "bias". */
int genie_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_mult, const double* grad_sumsq,
                     float max_grad_norm, void* stream);

/* EMA of the weights (additions; nothing above changes).  Reference: magvit2/modules/ema.py, LitEma.forward.  The averaged buffer
 * `ema` has the layout of `params` (same offsets; padding that is zero stays zero: 0 - omd * (0 - 0)) and starts as a copy of it.
 * After the optimizer has produced an element's p_new:
 *     ema = ema - (omd * (ema - p_new))
 * three f32 operations, each rounded on its own, no FMA contraction -- LitEma's `shadow.sub_(one_minus_decay * (shadow - param))`
 * bit for bit, and restated in NumPy f32 by tests/ema_model.py.  omd is the CALLER's float: omd = float32(1) - d_n with
 *     d_n = float32(decay)                                        without warm-up,
 *     d_n = min(float32(decay), float32((1 + n) / (10 + n)))      with it (LitEma's use_num_upates),
 * n = 1, 2, ... the number of EMA updates including this one (1xgpt_amd/train.py, ema_decay_at).
 * genie_adamw_ema_step: genie_adamw_step (same arguments, the same bits in params / exp_avg / exp_avg_sq) and that line on `ema` in
 * ONE pass over the range -- 36 bytes per element against 28 + 12 for the two calls.  genie_ema_update: the line alone, for a caller
 * with another optimizer.  genie_swap_f32: a[i] <-> b[i] in place (evaluate with the averaged weights: swap params and ema, repack
 * the 16-bit copies, evaluate, swap back -- exact by construction).  All three: one launch, 16-byte loads and stores when every
 * pointer is 16-byte aligned (any n; the n % 4 tail and a misaligned pointer take a one-element path), no atomics: the same bytes
 * run to run.  `ema` must not overlap the other ranges.  Refused with GENIE_E_ARG before the device or the stream is touched, outputs
 * as they were: a NULL pointer with n > 0; step < 1; one_minus_decay < 0, > 1 or not finite; overlapping a / b.  n == 0: GENIE_OK,
 * nothing enqueued. */
int genie_adamw_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, float grad_mult,
                         const double* grad_sumsq, float max_grad_norm, float ema_one_minus_decay, void* stream);
int genie_ema_update(float* ema, const float* params, size_t n, float one_minus_decay, void* stream);
int genie_swap_f32(float* a, float* b, size_t n, void* stream);

/* Frozen tensors (additions; nothing above changes).  Fine-tuning trains a subset of the weights (torch: requires_grad = False on the
 * rest; torch.optim.AdamW and clip_grad_norm_ skip them).  A NULL member of the `grads` table passed to genie_train_backward_head[_ex],
 * genie_train_backward_layer[_ex|_drop] or genie_train_backward_embed[_cond] means "this tensor is frozen": its gradient is not
 * computed and nothing is written for it, with or without `accumulate`.  The running d loss / d x is propagated exactly as before, so
 * a caller may also stop calling genie_train_backward_layer* below the lowest layer that holds a trainable tensor (and skip the
 * embedding call when nothing on that side trains); with recompute = 1 the layers never called are never rebuilt.  (Before this
 * section a NULL member was undefined: no defined behaviour changes.  A bias the configuration does not have was and is ignored.)
 * With every member non-NULL each call enqueues the launches it always did; the gradients that are computed are the same bits
 * whatever else is frozen -- they come from the same kernels in the same order.  What a NULL skips:
 *   a Linear weight   exact: the weight-gradient product.  16-bit: that product, the transposed copy of the saved activation and the
 *                     transposed planes of the gradient operand; the row-major operand of the input-gradient product (f16x3: scaled
 *                     by 2^12 and saturated as above; fc1: with gelu' folded in) is made as before, by a rows-only form of the same
 *                     kernel, and with a trainable bias the column sums keep their slab layout and order;
 *   a Linear bias     the column sums and their reduction;
 *   norm1 / norm2 / a qk-norm's weight and bias   both NULL: a parameter-free backward kernel (no accumulators, no LDS reduction, no
 *                     partial store) and none of the three reductions behind it; one NULL: the full kernel, and only the wanted half
 *                     of the reduction;
 *   pos_embed, mask_embed, embed[j]   that part of the embedding backward, each on its own; all NULL and no actions: nothing is
 *                     enqueued.  (d_table of genie_train_backward_embed_cond stays required with actions: a caller whose action table
 *                     is frozen passes cond = NULL.)
 * genie_train_pack_weights_some: genie_train_pack_weights for the Linears whose *_w member (qkv_w, proj_w, fc1_w, fc2_w, out_w) in
 * `select` is non-NULL -- the caller's gradient table serves: a frozen weight has not moved, so its 16-bit copies are current.
 * select == NULL packs everything.  GENIE_PREC_EXACT: GENIE_E_ARG, like genie_train_pack_weights.
 * genie_adamw_step, genie_adamw_ema_step, genie_sumsq and genie_swap_f32 are unchanged: the caller runs them over the ranges that
 * hold trainable tensors. */
int genie_train_pack_weights_some(const genie_cfg* cfg, const genie_weights* w, const genie_weights* w16,
                                  const genie_weights* w16T, const genie_weights* select, void* stream);

/* LoRA adapters (additions; nothing above changes).  Hu et al. 2021; reference counterpart: none.  An adapted Linear (out, in) keeps its
 * base weight W0 and trains A (rank, in) and B (out, rank), row-major f32, with s = alpha / rank the caller's float:
 *     W = W0 + s B A                                                  (genie_lora_merge)
 * Every entry point above runs on W and is untouched; the step's weight gradient dW = d loss / d W is then projected onto the adapters,
 *     dA = s B^T dW        dB = s dW A^T                              (genie_lora_project)
 * which by the chain rule are the gradients of the adapters.  The weight-gradient product of an adapted Linear still runs.
 * Arithmetic, f32: an element of W is fma(s, sum_k b[i,k] a[k,j], w0[i,j]) with the sum built by one fma per k, ascending from 0.0f.
 * An element of dA is a sum over the `out` rows: within each run of 64 rows one fma per row, ascending; the ceil(out / 64) run sums
 * ("slabs", in `scratch`) are then added in four interleaved chains t = 0, 4, .. / 1, 5, .. / 2, 6, .. / 3, 7, .. combined as
 * (c0 + c1) + (c2 + c3), and the result is fma(s, sum, accumulate ? old : 0.0f).  dB likewise over runs of 64 of the `in` columns.
 * No atomics and no dependence on what scratch held: the same bytes run to run.  dw is read from memory once for both results.
 * One call serves 1 .. GENIE_LORA_MAX_ITEMS Linears of any mix of shapes in ONE launch (project: one more for the slab sums); the table
 * is read on the host during the call and travels to the kernels by value.  Per item: out >= 1; in >= 16 and a multiple of 16;
 * 1 <= rank <= GENIE_LORA_MAX_RANK; w, w0, a, dw and da 16-byte aligned.  genie_lora_merge reads w0, a, b and writes w, which may BE w0
 * (the in-place merge; any other overlap of the two is refused); dw, da, db are ignored.  genie_lora_project reads dw, a, b and writes
 * da and db (accumulate = 1: adds to them); w and w0 are ignored.
 * Every function validates all items before the device or the stream is touched and never allocates.  Refused with GENIE_E_ARG, every
 * buffer as it was: a NULL table or a NULL pointer the call uses; n outside 1 .. GENIE_LORA_MAX_ITEMS; out < 1; rank outside
 * 1 .. GENIE_LORA_MAX_RANK; in not a positive multiple of 16; a scale that is not finite; a misaligned pointer; a or b overlapping an
 * output of its item (w; da, db), or dw overlapping da or db; a NULL scratch or fewer scratch_bytes than
 * genie_lora_project_scratch_bytes(items, n), which returns 0 for a table it refuses. */
#define GENIE_LORA_MAX_ITEMS 8
#define GENIE_LORA_MAX_RANK 64
typedef struct genie_lora_item {
    float* w;          /* merge: (out, in) result; may be w0 */
    const float* w0;   /* merge: (out, in) base weight */
    const float* a;    /* (rank, in) */
    const float* b;    /* (out, rank) */
    const float* dw;   /* project: (out, in) d loss / d W */
    float* da;         /* project: (rank, in) */
    float* db;         /* project: (out, rank) */
    int32_t out, in, rank;
    float scale;       /* s = alpha / rank */
} genie_lora_item;
/* sizeof(genie_lora_item) and the offsets of its eleven fields, in declaration order: writes min(n, 12) entries, returns 12. */
int genie_lora_layout(size_t* out_host, int n);
int genie_lora_merge(const genie_lora_item* items, int n, void* stream);
size_t genie_lora_project_scratch_bytes(const genie_lora_item* items, int n);
int genie_lora_project(const genie_lora_item* items, int n, int accumulate, void* scratch, size_t scratch_bytes, void* stream);

/* Muon (additions; nothing above changes).  Jordan et al. 2024; counterpart: torch.optim.Muon.  Momentum, then a Newton-Schulz
 * orthogonalisation of each target matrix's update.  For a matrix W (rows, cols), row-major f32, with this step's gradient g, momentum
 * buffer B (same shape; starts at zero) and the settings below:
 *      1. g' = coef * g                    coef = grad_mult * min(1, max_grad_norm / (grad_mult * sqrt(*grad_sumsq) + 1e-6)), the
 *                                          coefficient of genie_adamw_step (grad_sumsq == NULL or max_grad_norm <= 0: grad_mult alone)
 *      2. B  = mu * B + g'
 *      3. u  = g' + mu * B  (nesterov)     u = B  (otherwise)
 *      4. X  = u  if rows <= cols, else u^T                       -- X is (m, n) with m = min(rows, cols)
 *      5. X  = X / max(||X||_F, eps)
 *      6. ns_steps times:   A = X X^T;   P = b A + c A A;   X = a X + P X
 *      7. O  = X, transposed back if it was transposed
 *      8. W  = W * (1 - lr * weight_decay)
 *      9. W  = W - (lr * adj) * O          adj = 0.2 * sqrt(max(rows, cols))      GENIE_MUON_ADJUST_MATCH_RMS_ADAMW
 *                                          adj = sqrt(max(1, rows / cols))        GENIE_MUON_ADJUST_ORIGINAL
 *     10. ema = ema - omd * (ema - W)      when the item's ema is not NULL: the line of "EMA of the weights", in the pass that writes W
 * torch.optim.Muon keeps (1 - mu) B and forms (1 - mu) u (its lerp_ form): the same X after step 5, up to rounding and the eps clamp.
 * It runs steps 4 to 7 in bf16; here they are f32 in all three training precisions (the relative distance of torch's bf16 iteration
 * from a float64 one is 1e-2 on Gaussian and 0.4 .. 0.8 on low-rank inputs, of this one 1e-6 and 1e-5).
 * Arithmetic, f32 with every operation rounded on its own (no contraction) unless said: steps 1 to 3 as written; ||X||_F^2 is summed
 * in f64 in a fixed two-stage order (64 partial sums per matrix, each a grid-stride walk, added ascending), no atomics; step 5 is one
 * more elementwise pass, x / max((float)sqrt(sum), eps), not folded into the first product.  A tall matrix is never transposed in
 * memory: its products are A = X^T X and X = a X + X P on the stored (rows, cols) array.  Each product is a batched matrix-core GEMM
 * C_i = beta * R_i + alpha * op(A_i) op(B_i) on v_mfma_f32_32x32x2_f32 over all matrices of one shape in ONE launch: an output element
 * is the MFMA fmaf chain over k ascending from 0.0f, then (beta * r) + (alpha * acc) (without R: alpha * acc).  The order depends on
 * the shape alone: the same input gives the same bits run to run, whatever other items share the launch and whatever the workspace
 * held.  A and P are computed in full (all tiles; they come out bit-symmetric).  Step 8: decay = (float)(1.0 - (double) lr *
 * weight_decay), s = (float)((double) lr * adj) with adj in double; W = (W * decay) - (s * O).
 * genie_muon_step: 1 .. GENIE_MUON_MAX_ITEMS matrices of any mix of shapes.  Launches: one for steps 1 to 3 and the partial sums of the
 * whole table, one for step 5, 3 * ns_steps per distinct (rows, cols) among the items, one for steps 8 to 10.  The table and the
 * settings are read on the host during the call and travel to the kernels by value.  Reads grad; updates param, momentum and, when
 * given, ema.  genie_newton_schulz: steps 4 to 7 alone on `batch` contiguous (rows, cols) matrices, in -> out (in == out allowed; any
 * other overlap refused).  Workspace layout (both; bytes from genie_muon_workspace_bytes, for the unit entry point of `batch` items of
 * (rows, cols)): [64 doubles per item | X0: every item's u, later X | X1: the same layout, the iteration's other buffer | A | P: the
 * largest shape group's (m, m) Grams], every part 256-byte aligned.
 * Validated before the device or the stream is touched, never allocating; refused with GENIE_E_ARG, every buffer as it was: a NULL
 * table, settings, param, grad or momentum; n outside 1 .. GENIE_MUON_MAX_ITEMS; rows or cols not a positive multiple of 16; a
 * pointer not 16-byte aligned; ns_steps outside 0 .. 99; an adjust mode that is neither; a momentum, coefficient, eps, grad_mult,
 * max_grad_norm, lr or weight_decay that is not finite; omd outside [0, 1] when an ema is given; a NULL or misaligned workspace or
 * fewer workspace_bytes than genie_muon_workspace_bytes, which returns 0 for a table it refuses. */
#define GENIE_MUON_MAX_ITEMS 64
#define GENIE_MUON_ADJUST_ORIGINAL 0
#define GENIE_MUON_ADJUST_MATCH_RMS_ADAMW 1
typedef struct genie_muon_item {
    float* param;         /* (rows, cols) W */
    const float* grad;    /* (rows, cols) g */
    float* momentum;      /* (rows, cols) B */
    float* ema;           /* (rows, cols) average of W, or NULL */
    int32_t rows, cols;
    float lr, weight_decay;
} genie_muon_item;
typedef struct genie_muon_settings {
    float momentum;              /* mu */
    float a, b, c;               /* the polynomial's coefficients */
    float eps;                   /* floor of the norm in step 5 */
    float grad_mult;             /* 1 / (world size * accumulation steps) */
    float max_grad_norm;         /* <= 0: no clip */
    float ema_one_minus_decay;   /* omd of step 10; read only when an item has an ema */
    int32_t nesterov;            /* 0 / 1 */
    int32_t ns_steps;            /* 0 .. 99 */
    int32_t adjust;              /* GENIE_MUON_ADJUST_* */
    int32_t reserved;            /* 0 */
    const double* grad_sumsq;    /* device: the sum of squares of ALL gradients (genie_sumsq), or NULL */
} genie_muon_settings;
/* sizeof(genie_muon_item), the offsets of its eight fields, sizeof(genie_muon_settings) and the offsets of its thirteen fields, in
 * declaration order: writes min(n, 23) entries, returns 23. */
int genie_muon_layout(size_t* out_host, int n);
size_t genie_muon_workspace_bytes(const genie_muon_item* items, int n);
int genie_muon_step(const genie_muon_item* items, int n, const genie_muon_settings* settings, void* workspace, size_t workspace_bytes,
                    void* stream);
/* workspace_bytes: genie_muon_workspace_bytes of `batch` items of (rows, cols); 1 <= batch <= GENIE_MUON_MAX_ITEMS. */
int genie_newton_schulz(const float* in, float* out, int rows, int cols, int batch, int steps, float a, float b, float c, float eps,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Continuous per-frame actions (ABI 3 addition; nothing above changes).  A model conditioned on float action vectors of A values per
 * frame projects them, once per call, into the rows that genie_frame_cond addresses: the caller builds a table of one learned "no
 * action" row plus one projected row per frame of the call, points cond->table at it and cond->ids at "row of frame (b, t)", and every
 * *_cond / *_ex / *_guided / rollout entry point and genie_guidance.null_action then work by index, unchanged.  Reference counterpart:
 * none (its README announces raw actions; its data.py leaves them commented out).
 * The arithmetic, in f32 with every operation rounded on its own and no FMA contraction, reproducible bit for bit in NumPy f32:
 *     z_j   = (a_j - mean_j) * inv_std_j          -- a NULL mean skips the subtraction, a NULL inv_std the product (not "with 0 or 1")
 *     row_c = bias_c (0.0f when bias is NULL); then for j = 0 .. A-1 ascending:  row_c = row_c + (W[c,j] * z_j)
 * and for the gradients, given d_rows = d loss / d rows (n, d_model), both sums starting from 0.0f and walking n = 0 .. n-1 ascending,
 * strictly in sequence (one level, no chunks, no atomics: the same bytes run to run):
 *     d_bias[c]     = sum_n d_rows[n,c]
 *     d_weight[c,j] = sum_n (d_rows[n,c] * z[n,j])
 * accumulate = 0 stores the finished sum; accumulate = 1 stores old + sum (one add).
 * Sizes: 1 <= A <= GENIE_ACTION_MAX_DIM, 1 <= d_model <= 1024 (GENIE_E_SHAPE beyond).  A NULL p / vecs / rows / d_rows / d_weight / p->weight
 * (forward), A < 1, d_model < 1 or n < 0: GENIE_E_ARG, nothing enqueued.  n == 0: success, nothing enqueued, nothing written.  d_bias may
 * be NULL (no bias gradient).  The struct is read on the host during the call; its pointers are device pointers. */
#define GENIE_ACTION_MAX_DIM 256
typedef struct genie_action_proj {
    const float* weight;   /* (d_model, A) f32, nn.Linear layout */
    const float* bias;     /* (d_model) or NULL */
    const float* mean;     /* (A) or NULL: input normalisation */
    const float* inv_std;  /* (A) or NULL; 1/std computed by the caller in f32 */
    int32_t action_dim;    /* A >= 1 */
} genie_action_proj;
/* sizeof(genie_action_proj) and the offsets of its five fields, in declaration order: writes min(n, 6) entries, returns 6. */
int genie_action_proj_layout(size_t* out_host, int n);
/* rows (n, d_model) <- the projection of vecs (n, A): one launch. */
int genie_action_rows(const genie_action_proj* p, const float* vecs, float* rows, int64_t n, int d_model, void* stream);
/* d_weight (d_model, A) and d_bias (d_model) from d_rows (n, d_model) and the same vecs (n, A): one launch; p->weight is not read. */
int genie_action_rows_backward(const genie_action_proj* p, const float* vecs, const float* d_rows, int64_t n, int d_model,
                               float* d_weight, float* d_bias, int accumulate, void* stream);

/* Image-space metrics of two uint8 frame batches (ABI 3 addition; nothing above changes).  a and b are (n, C, H, W) planar uint8 device
 * tensors, contiguous, as genie_conv_direct_bf16's uint8 output mode (HipDecoder.decode_tokens) leaves them.  Row i of out (n, 4) f64 is
 *     sse      = sum over C*H*W of (a - b)^2                       -- exact (integer sums, < 2^53)
 *     sae      = sum over C*H*W of |a - b|                         -- exact
 *     ssim_sum = sum of the SSIM index (Wang, Bovik, Sheikh, Simoncelli 2004) over every valid window position of every channel
 *     n_win    = C * (H - 10) * (W - 10)                           -- the number of those positions; mean SSIM = ssim_sum / n_win
 * so that MSE = sse / (C*H*W), MAE = sae / (C*H*W), PSNR = 10 log10(255^2 / MSE).  The SSIM index is fixed to:
 *     window   11 x 11 separable Gaussian, sigma 1.5: taps g_r = exp(-r^2 / 4.5), r = -5 .. 5, divided by their sum
 *     moments  weighted, population: mu_x = sum g x, var_x = sum g x^2 - mu_x^2, cov_xy = sum g xy - mu_x mu_y (likewise y)
 *     C1 = (0.01 * 255)^2 = 6.5025,  C2 = (0.03 * 255)^2 = 58.5225
 *     SSIM     = (2 mu_x mu_y + C1)(2 cov_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2))
 *     border   none: only the (H - 10)(W - 10) windows that lie inside the image count (no padding)
 * which is the image skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=255)
 * averages.  Moments are accumulated in f64 on pixel values pivoted by 128, so the variances do not cancel on flat frames; measured
 * |SSIM - f64 model| per frame: DESIGN.md section 8.10.  Results are bit-identical run to run and do not depend on n (fixed-order sums, no
 * float atomics).  Neither out nor the workspace is read before it is written.  Two launches; 64-bit element offsets.
 * Reference counterpart: none (its image-space metric is LPIPS, eval_utils.py:80-88, which needs a network's weights).
 * Errors, each before anything is enqueued, out and workspace untouched: NULL a / b / out, n < 0, C < 1, a NULL or short workspace at
 * n > 0: GENIE_E_ARG; H < 11 or W < 11, or more than 2^31 - 1 tiles (n * C * ceil((H - 10) / 32) * ceil((W - 10) / 32)): GENIE_E_SHAPE.
 * n == 0: success, nothing enqueued, nothing written. */
/* bytes of workspace genie_frame_metrics needs (0 for arguments it refuses and for n == 0) */
size_t genie_frame_metrics_workspace_bytes(int64_t n, int C, int H, int W);
int genie_frame_metrics(const uint8_t* a, const uint8_t* b, int64_t n, int C, int H, int W, double* out, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENIE_HIP_H */
