// Host-side launchers of the gfx950 kernels (one block of declarations per kernels_*.hip file) and the pass / workspace types of the
// layer drivers (st_block.hip, kernels_frame.hip), which api.hip's entry points and the loops of generate_api.hip call.
#pragma once
#include "common.hpp"

namespace genie {

enum { GEMM_GELU = 1, GEMM_ACCUM = 2, GEMM_BIAS_ALONG_M = 4 };

// Workspace carving shared by api.hip and the layer drivers (see carve() in api.hip): buffers only.  What kind of
// pass a layer call belongs to is a BlockPass, what one block hands to the next a BlockCarry (both below).
struct Workspace {
    float* x;          // (M, d)   residual stream, f32 in every precision; offset 0 of the workspace
    void* xn;          // (M, d) x 4 bytes: exact = LayerNorm / attention output (f32);
                       //                   bf16  = [bf16 shadow of x | bf16 LayerNorm / attention output]
    void* big;         // (M, max(3d, hidden)) x 4 bytes: qkv, later the MLP hidden
    float* logits;     // (M, V)   token-major logits scratch
    int64_t* samples;  // (B, S)
    float* conf;       // (B, S)
    uint8_t* unmasked; // (B, S)
    void* aux;         // (M, d) x 4 bytes: f16x3 = split planes of the LayerNorm / attention output
    size_t total;
};

// What one layer call is: built once per layer by the constructor function of its kind, read-only from then on.
//   PLAIN   a full forward; no cache
//   CLEAN   teacher-forced prefix reuse, first half: the temporal qkv GEMM writes this layer's slice of the cache
//   PREFIX  ... second half (masked-frames pass): temporal attention takes keys j < i + tshift from the cached qkv
//   DECODE  single-frame decode (generate with a temporal KV cache): the block runs on dense (B, nf, S, *) buffers; its temporal qkv is
//           written into slot `frame_t` of this layer's cache slice and the attention reads slots 0..frame_t
//           fan-out flavour (decode_fanout): the B clips of the pass are K branches each of B / K parents.  Slots < fan_P0 are read from the
//           parent's clip of `trunk` (an ordinary model_T-slot slice of B / K clips, never written here); slot j >= fan_P0 is slot
//           j - fan_P0 of the clip's own `cache`, a slice of frame_T = Tb slots per clip
struct BlockPass {
    enum Kind { PLAIN, CLEAN, PREFIX, DECODE };
    const Kind kind;
    float* const cache;     // this layer's slice of the temporal KV cache (NULL in a PLAIN pass).  A PREFIX pass only reads it: the
                            // pointer is non-const because the fused temporal kernels take one `kv` argument for both directions
    const int tq_frames;    // CLEAN: frames per clip in the cache layout; > cfg.T when a short clean pass fills a full-length cache
                            // (generate: prompt frames into the T-frame KV cache)
    const int tshift;       // PREFIX: clip-frame offset of the masked-frames buffers against the cache (0 or 1)
    const int frame_t;      // DECODE: the cache slot of the pass's first frame
    const int frame_T;      // DECODE: frames per clip in the cache layout
    const int model_T;      // T of the MODEL's config (cache passes run on private copies with fewer frames): decides, once per model,
                            // whether GENIE_PREC_BF16 keeps its temporal qkv / KV cache in bf16 (temporal_qkv16)
    const bool stop_after_tqkv;   // CLEAN, last layer: only the temporal qkv (the cache entry) is needed -- the block returns right after it
    // the block that follows (NULL after the last one) and whether it opens with a LayerNorm: then this block's last GEMM need not
    // refresh the 16-bit shadow of x, and the GENIE_PREC_BF16 fused MLP kernel can apply that norm1 in its epilogue (BlockCarry)
    const genie_layer_weights* const next_layer;
    const bool next_is_ln;
    const float* const trunk = nullptr;   // DECODE, fan-out: this layer's slice of the shared context cache (NULL: an ordinary decode pass)
    const int fan_P0 = 0;                 // ... its slots [0, fan_P0) are the ones read; 0 in an ordinary decode pass
    const int fan_K = 1;                  // ... branches per parent clip

    static BlockPass plain(const genie_cfg& c, const genie_layer_weights* next, int model_T) {
        return {PLAIN, nullptr, 0, 0, -1, 0, model_T, false, next, next && !c.qk_norm};
    }
    static BlockPass clean(const genie_cfg& c, const genie_layer_weights* next, int model_T, float* slice, int cache_frames) {
        return {CLEAN, slice, cache_frames, 0, -1, 0, model_T, /*stop_after_tqkv=*/next == nullptr, next, next && !c.qk_norm};
    }
    static BlockPass prefix(const genie_cfg& c, const genie_layer_weights* next, int model_T, const float* slice, int tshift) {
        return {PREFIX, const_cast<float*>(slice), 0, tshift, -1, 0, model_T, false, next, next && !c.qk_norm};
    }
    static BlockPass decode(const genie_cfg& c, const genie_layer_weights* next, int model_T, float* slice, int frame_t) {
        return {DECODE, slice, 0, 0, frame_t, model_T, model_T, false, next, next && !c.qk_norm};
    }
    static BlockPass decode_fanout(const genie_cfg& c, const genie_layer_weights* next, int model_T, float* branch_slice, int frame_t,
                                   const float* trunk_slice, int P0, int K, int Tb) {
        return {DECODE, branch_slice, 0, 0, frame_t, Tb, model_T, false, next, next && !c.qk_norm, trunk_slice, P0, K};
    }
    bool is_plain() const { return kind == PLAIN; }
    bool is_fanout() const { return trunk != nullptr; }
    bool is_decode() const { return kind == DECODE; }
    bool writes_cache() const { return kind == CLEAN; }   // (DECODE writes its slot too, through its own GEMM shape)
    bool reads_cache() const { return kind == PREFIX; }
    bool is_cache_pass() const { return kind == CLEAN || kind == PREFIX; }
    // frames per clip in the layout the temporal qkv GEMM writes (T = the pass's own frame count)
    int tq_stride(int T) const { return kind == CLEAN && tq_frames > T ? tq_frames : T; }
    bool strided(int T) const { return tq_stride(T) != T; }
    int fused_mode() const { return kind == CLEAN ? 1 : kind == PREFIX ? 2 : 0; }   // `mode` of the fused temporal kernels
};

// What one block of a pass leaves for the next one (GENIE_PREC_BF16, fused MLP kernel).  Owned by the layer loop, which starts every
// pass with a fresh one.
struct BlockCarry {
    bool ln1_done = false;          // norm1 of the next block is already applied (in xn16): that block skips its LayerNorm launch
    bool qkv_planes_done = false;   // ... or even its spatial operand planes (in `big`): that block goes straight to its attention kernel
};

// GENIE_PREC_BF16: the temporal qkv buffer and the temporal KV cache hold bf16 values (half the bytes of the HBM-bound temporal
// attention kernels and of the qkv GEMM's output) whenever the bf16-input kernels cover every pass the model can run: T <= 16
// frames, head_dim 32 / 64.  The cache slices keep their f32-sized strides (a caller sizes the cache with
// genie_prefix_cache_bytes either way); only the first half of a slice is used.
inline bool temporal_qkv16(const genie_cfg& c, int model_T) {
    return c.precision == GENIE_PREC_BF16 && (model_T > 0 ? model_T : c.T) <= 16 && (c.head_dim == 32 || c.head_dim == 64);
}

// kernels_fused.hip: fused sub-blocks of the shipped geometry (GENIE_PREC_BF16, d 256); GENIE_E_UNSUPPORTED otherwise
int launch_pack_temporal_fused(const float* qkv_w, const float* proj_w, uint16_t* out, hipStream_t st);
int launch_pack_mlp_fused(const float* fc1_w, const float* fc2_w, uint16_t* out, hipStream_t st);
int launch_pack_spatial_proj(const float* proj_w, uint16_t* out, hipStream_t st);
int launch_spatial_attn_proj_bf16(const genie_cfg& c, const genie_attn_weights& aw, const uint16_t* qkv16, float* x, uint16_t* x16,
                                  long n_seq, hipStream_t st);
int launch_temporal_fused_bf16(const genie_cfg& c, const genie_attn_weights& aw, const uint16_t* x16, float* x, int B,
                               hipStream_t st);
int launch_mlp_fused_bf16(const genie_cfg& c, const genie_layer_weights& lw, float* x, uint16_t* x16_out, long rows, hipStream_t st,
                          const float* nx_g = nullptr, const float* nx_b = nullptr, const uint16_t* nx_qkv_stream = nullptr,
                          uint16_t* planes = nullptr);
int launch_pack_spatial_qkv(const float* qkv_w, uint16_t* out, hipStream_t st);
bool temporal_fused_takes(const genie_cfg& c, const genie_attn_weights& aw, int B);   // will launch_temporal_fused_bf16 run this problem?
// kernels_fused_prefix.hip: the same sub-block in the prefix-cache passes (mode 1 clean pass: K / V fragment images written to `kv`, the
// layer's cache slice; mode 2 masked pass: read back).  `takes` is the ONE predicate of producer and consumer.
bool temporal_prefix_fused_takes(const genie_cfg& c, const genie_attn_weights& aw, int B, int model_T);
int launch_temporal_prefix_fused_bf16(const genie_cfg& c, const genie_attn_weights& aw, float* x, uint16_t* kv, int B, int mode,
                                      int shift, int model_T, hipStream_t st);

// kernels_fused_f16x3.hip: temporal qkv Linear + temporal attention of the shipped geometry in GENIE_PREC_F16X3 (mode 0 plain, 1 clean pass
// writing the k / v accumulators to `kv`, 2 masked pass reading them); aw.fused_w16 = the stream of genie_pack_temporal_qkv_f16x3
bool temporal_qkv_attn_f16x3_takes(const genie_cfg& c, const genie_attn_weights& aw, int B, int model_T, bool cache_mode);
int launch_temporal_qkv_attn_f16x3(const genie_cfg& c, const genie_attn_weights& aw, const float* x, uint16_t* a16, long plane, float* kv, int B,
                                   int mode, int shift, int model_T, hipStream_t st);
int launch_pack_temporal_qkv_f16x3(const float* qkv_w, uint16_t* out, hipStream_t st);

// Study builds only (-DGENIE_STUDY): which Linear of the block the next GEMM launch is, and the layer it belongs to, so that
// tools/precision_study.py can run individual classes / layer ranges on 2 of the 3 split-f16 terms.
#ifdef GENIE_STUDY
extern int g_study_gemm_class;   // 0 qkv_s, 1 qkv_t, 2 proj_s, 3 proj_t, 4 fc1, 5 fc2, 6 readout
extern int g_study_layer;
int study_terms();                // 3, or 2 when GENIE_F16_TERMS2_CLASSES / _LAYER_LO / _LAYER_HI select the current launch
#define GENIE_STUDY_CLASS(k) (genie::g_study_gemm_class = (k))
#define GENIE_STUDY_LAYER(i) (genie::g_study_layer = (i))
#else
#define GENIE_STUDY_CLASS(k) ((void)0)
#define GENIE_STUDY_LAYER(i) ((void)0)
#endif

// Brackets one launch with HIP events when profiling of `cls` is enabled (see genie_profile_* in the ABI).
struct ProfScope {
    int slot;
    hipStream_t st;
    // kernel: a string LITERAL naming what is launched inside the scope (reported by genie_profile_kernels)
    ProfScope(int cls, double flops, double bytes, hipStream_t st, const char* kernel = nullptr);
    ~ProfScope();
};

// Per-frame action conditioning of the embedding (genie_frame_cond): token (b, t, s) of a pass over c.T frames adds row
// ids[b * clip_stride + t] of `table` (n_act rows of d_model) to its position row; `ids` already points at the pass's first
// frame (the absolute frame t0 of a window pass: ids = cond->ids + t0, clip_stride = the model's T).
struct EmbedAct {
    const float* table = nullptr;
    const int64_t* ids = nullptr;
    long clip_stride = 0;
    int S = 1;
    int n_act = 0;
};
// genie_frame_cond -> EmbedAct of a pass over frames [t0, t0 + pass T) of clips with model_T frames; NULL = unconditioned
inline const EmbedAct* frame_act(const genie_frame_cond* fc, int S, int t0, int model_T, EmbedAct& a) {
    if (!fc || fc->n_actions <= 0) return nullptr;
    a.table = fc->table;
    a.ids = fc->ids + t0;
    a.clip_stride = model_T;
    a.S = S;
    a.n_act = fc->n_actions;
    return &a;
}
inline int check_frame_cond(const genie_frame_cond* fc, const char* where) {
    if (!fc) return GENIE_OK;
    GENIE_CHECK_ARG(fc->n_actions >= 0, "%s: n_actions = %d", where, (int)fc->n_actions);
    GENIE_CHECK_ARG(fc->n_actions == 0 || (fc->table && fc->ids), "%s: frame condition without table / ids", where);
    return GENIE_OK;
}
// act == NULL or act->n_act == 0: the unconditioned kernel
int launch_embed(const genie_cfg& c, const genie_weights& w, const int64_t* ids, int B, float* x, hipStream_t st,
                 const EmbedAct* act = nullptr);
int launch_layer_norm(const float* x, const float* g, const float* b, float* y, long rows, int C, float eps,
                      hipStream_t st);
int launch_layer_norm_bf16(const float* x, const float* g, const float* b, uint16_t* y, long rows, int C, float eps,
                           hipStream_t st);
// C[batch][M,N] (+)= epi(alpha * A[batch][M,K] . W[batch][N,K]^T + bias)
int launch_gemm_f32(const float* A, long lda, long strideA, const float* W, long ldw, long strideW, const float* bias,
                    float* C, long ldc, long strideC, int M, int N, int K, int batch, int flags, float alpha,
                    hipStream_t st);
int launch_attn_generic(const float* qkv, float* out, int N, long n_seq, int inner, long outer_stride,
                        long inner_stride, long pos_stride, int d, int H, int Dh, float scale, int causal,
                        const float* nw, const float* nb, hipStream_t st);
int launch_attn_generic_bf16(const uint16_t* qkv, uint16_t* out, int N, long n_seq, int inner, long outer_stride,
                             long inner_stride, long pos_stride, int d, int H, int Dh, float scale, int causal,
                             const float* nw, const float* nb, hipStream_t st);
// out16 != NULL: write the result 16-bit instead of f32 `out`: plane != 0 -> f16 split planes (hi at out16, lo at
// out16 + plane); plane == 0 -> bf16
int launch_attn_spatial_f32_mfma(const float* qkv, float* out, int S, long n_seq, int d, int H, int Dh, float scale,
                                 const float* nw, const float* nb, hipStream_t st, uint16_t* out16 = nullptr,
                                 size_t plane = 0);
int launch_attn_spatial_split(const float* qkv, float* out, int S, long n_seq, int d, int H, int Dh, float scale,
                              const float* nw, const float* nb, hipStream_t st, uint16_t* out16 = nullptr,
                              size_t plane = 0);
// kernels_attn_temporal.hip: causal temporal attention (out16 / plane as above; in16: the qkv rows / the cache hold bf16, temporal_qkv16)
int launch_attn_temporal_f32_mfma(const float* qkv, float* out, int B, int T, int S, int d, int H, int Dh, float scale,
                                  const float* nw, const float* nb, hipStream_t st, uint16_t* out16 = nullptr,
                                  size_t plane = 0, int Tq = 0, bool in16 = false);
int launch_attn_temporal_prefix(const float* cur, const float* cache, float* out, int B, int T, int S, int d, int H,
                                int Dh, float scale, const float* nw, const float* nb, hipStream_t st,
                                uint16_t* out16 = nullptr, size_t plane = 0, int sh = 0, bool in16 = false);
int launch_attn_temporal_single(const float* cache, float* out, int B, int T, int S, int t, int d, int H, int Dh,
                                float scale, const float* nw, const float* nb, hipStream_t st,
                                uint16_t* out16 = nullptr, size_t plane = 0, bool in16 = false);
// The split cache of a fan-out decode pass as the decode attention kernels see it (BlockPass::decode_fanout): clip i reads slots
// j < P0 at trunk + ((i / K) * T + j) * S * 3d and slots j >= P0 at branch + (i * Tb + (j - P0)) * S * 3d.  The ordinary flavour carries
// nothing: its instantiations are the kernels without the split.
template <bool FAN>
struct FanSplit {};
template <>
struct FanSplit<true> {
    const void* trunk;   // same element type as the branch slice
    int T, P0, K;        // slots per clip of the trunk; first branch slot; branches per parent
};
// cache slot j of one (clip, position, head): `own` + j slots, or (FAN) the trunk below P0 and slot j - P0 of the branch from P0 on
template <bool FAN, typename TI>
__device__ __forceinline__ const TI* fan_slot(const TI* own, const TI* trunk, int j, int P0, size_t tok) {
    if constexpr (FAN) {
        const bool lo = j < P0;
        return (lo ? trunk : own) + (size_t)(lo ? j : j - P0) * tok;
    } else {
        return own + (size_t)j * tok;
    }
}
// launch_attn_temporal_single over that split cache: `cache` is the branch slice and T its slots per clip (Tb); t >= fan.P0
int launch_attn_temporal_single_fanout(const float* cache, float* out, int B, int T, int S, int t, int d, int H, int Dh, float scale,
                                       const float* nw, const float* nb, hipStream_t st, uint16_t* out16, size_t plane, bool in16,
                                       const FanSplit<true>& fan);
// kernels_exact.hip, continued
int launch_layer_norm_split(const float* x, const float* g, const float* b, uint16_t* y, size_t plane, long rows, int C,
                            float eps, hipStream_t st);
int launch_split_f16(const float* src, uint16_t* dst, size_t plane, size_t n, hipStream_t st);
int launch_transpose(const float* in, float* out, int batch, int rows, int cols, hipStream_t st);
int launch_sample(const genie_cfg& c, const float* logits, int layout, int B, float temperature,
                  const float* uniforms, int64_t* samples, float* conf, hipStream_t st);
// kernels_sample.hip: the tempered / top-k / top-p filtered law (genie_sampling); NULL or all-off without keys_out = launch_sample
bool sampling_is_neutral(const genie_sampling* sp, int vf);
int launch_sample_ex(const genie_cfg& c, const float* logits, int layout, int B, float temperature, const float* uniforms,
                     int64_t* samples, float* conf, const genie_sampling* sp, float* keys_out, const float* noise, float anneal,
                     hipStream_t st);
// ... under classifier-free guidance (genie_guidance): logits g = (scale * cond) + ((1 - scale) * null) formed at load time; scale == 1
// is launch_sample_ex on the conditional logits.  launch_guide_logits materialises g for `rows` rows of `len` values (row strides in elements).
int launch_sample_guided(const genie_cfg& c, const float* logits_c, const float* logits_u, int layout, int B, float temperature,
                         const float* uniforms, int64_t* samples, float* conf, const genie_sampling* sp, float* keys_out,
                         const float* noise, float anneal, float scale, hipStream_t st);
int launch_guide_logits(const float* cond, const float* null_, float* out, long rows, long len, long in_stride, long out_stride, float scale,
                        hipStream_t st);
// continuous actions (kernels_action.hip; arithmetic: genie_action_proj in genie_hip.h)
int launch_action_rows(const genie_action_proj& p, const float* vecs, float* rows, long n, int d, hipStream_t st);
int launch_action_rows_backward(const genie_action_proj& p, const float* vecs, const float* d_rows, long n, int d, float* d_weight,
                                float* d_bias, int accumulate, hipStream_t st);
int launch_mask_step(const float* keys, int n, int last_step, int64_t mask_id, uint8_t* unmasked, int64_t* samples,
                     int64_t* prompt_frame, long clip_stride, int B, int S, hipStream_t st);
// known tokens (kernels_known.hip): a frame's start state, and the mask step with a per-clip count n_b = ceil(frac * (S - K_b))
int launch_known_begin(const int64_t* known, long known_stride, int64_t mask_id, int64_t* frame, long frame_stride, uint8_t* unmasked, int B,
                       int S, int copies, hipStream_t st);
int launch_mask_step_known(const float* keys, double frac, int last_step, int64_t mask_id, const int64_t* known, long known_stride,
                           uint8_t* unmasked, int64_t* samples, int64_t* prompt_frame, long clip_stride, int B, int S, hipStream_t st);
int launch_check_masked(const int64_t* prompt, int B, int T, int S, int out_t, int64_t mask_id, int32_t* flag,
                        hipStream_t st);
int launch_bits(const int64_t* ids, float* z, int n, int hw, int bits, hipStream_t st);
int launch_rescale_u8(const void* x, int is_bf16, uint8_t* out, size_t n, hipStream_t st);
int launch_tokens_from_bits(const float* h, int64_t* ids, int n, int hw, int bits, hipStream_t st);
int launch_conv3x3_igemm(const uint16_t* X, const uint16_t* Wt, const float* bias, const uint16_t* residual, uint16_t* Y,
                         const uint16_t* zero_page, int n_img, int H, int Wd, int Cin, int Cout, int d2s, hipStream_t st,
                         int stride = 1, float* gn_part = nullptr, int gn_groups = 0);
size_t conv_gn_part_floats(int n_img, int H, int Wd, int Cout);
int launch_gn_swish_tiles(const uint16_t* X, const float* gamma, const float* beta, uint16_t* Y, const float* part, float* stats,
                          int n_img, int H, int Wd, int Cout, int d2s, int groups, float eps, int apply_swish, hipStream_t st);
int launch_frames_to_nhwc(const uint8_t* f, uint16_t* x, long n_img, int HW, int cin, int cpad, hipStream_t st);
int launch_tokens_from_nhwc(const uint16_t* h, int64_t* ids, long n_pix, int bits, int cpad, hipStream_t st);
size_t gn_scratch_floats(int n_img, int HW, int groups);
int launch_gn_swish(const uint16_t* X, const float* gamma, const float* beta, uint16_t* Y, float* stats, int n_img, int HW,
                    int C, int groups, float eps, int apply_swish, hipStream_t st);
int launch_conv_direct(const uint16_t* X, const uint16_t* Wt, const float* bias, void* Y, int n_img, int H, int Wd, int Cin,
                       int Cout, int out_mode, hipStream_t st);
int launch_bits_nhwc(const int64_t* ids, uint16_t* z, long n_pix, int bits, int cpad, hipStream_t st);
int launch_rescale_nhwc_u8(const uint16_t* x, uint8_t* out, long n_img, int HW, int cpad, int cout, hipStream_t st);
int launch_pack_conv_weight(const float* w, uint16_t* out, int Cout, int Cin, int taps, hipStream_t st);
int launch_gemm_bf16_out16(const uint16_t* A16, const uint16_t* W16, const float* bias, uint16_t* C16, int M, int N, int K,
                           hipStream_t st);
int launch_pack_bf16(const float* src, uint16_t* dst, size_t n, hipStream_t st);

// ---- loss and scoring (kernels_loss.hip; the contract of each loss heads that file) ----
int launch_count_equal(const int64_t* a, long sa, const int64_t* b, long sb, int batch, long n, const double* ce3, double* sums6,
                       double n_tokens, double n_frames, double n_clips, hipStream_t st);
int launch_factored_ce(const genie_cfg& c, const float* logits, int layout, const int64_t* targets,
                       const int64_t* weight_ids, int B, int t0, int t1, double* sums, hipStream_t st);
// per-row NLL of one frame's token-major (N, S, V) logits: row i against the S targets at targets + (i / K) * target_clip_stride.
// nll / hits: f64, row i at [i * nll_stride] (hits may be NULL); token_nll: NULL or f32, row i at [i * token_stride + s].  Fixed-order
// f64 reduction inside the workgroup, no atomics.
int launch_score_rows(const genie_cfg& c, const float* logits, const int64_t* targets, long target_clip_stride, int K, long N, double* nll,
                      long nll_stride, double* hits, float* token_nll, long token_stride, hipStream_t st);
// the training losses on (n_clips, T, S) tokens of nfac factors of vf logits, d logits in place; each is its count kernel, then its loss
// kernel, into sums the caller zeroed.  Neutral step: three sums.
int launch_ce_fwd_bwd(const genie_cfg& c, float* logits, const int64_t* ids, const int64_t* labels, int B, double* sums,
                      hipStream_t st);
// the general objective (label smoothing, z-loss, per-frame weights; include/genie_hip.h, "Training objective"): five sums.  `obj` was
// checked by the caller (objective_ok in train_api.hip).
int launch_ce_objective(float* logits, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S, int vf, int nfac,
                        int64_t mask_id, const genie_objective& obj, double* sums, hipStream_t st);
// ... with a read-only row of teacher logits beside every student row (include/genie_hip.h, "Distillation"): seven sums.  obj, alpha,
// tau were checked by the caller.
int launch_ce_distill(float* logits, const float* teacher, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S,
                      int vf, int nfac, int64_t mask_id, const genie_objective& obj, float alpha, float tau, double* sums,
                      hipStream_t st);
// the loss launch of a training call: zeroes the 3 / 5 / 7 sums (a failure is reported under `fn`), then one of the three above --
// ds (non-neutral distillation of `teacher`), else obj (a struct), else (both NULL) the neutral step
int launch_train_loss(const char* fn, float* logits, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S, int vf,
                      int nfac, int64_t mask_id, const genie_objective* obj, const genie_distill* ds, const float* teacher, double* sums,
                      hipStream_t st);

// ---- training step (kernels_train.hip) ----
// C[b1][b2][M,N] = alpha * A.B (+bias) (+R); ta/tb: operand stored k-major; nsplit > 1: slabs C + s*sCsplit
int launch_gemm_f32_gen(bool ta, bool tb, const float* A, long lda, long sA1, long sA2, const float* W, long ldw, long sW1,
                        long sW2, const float* bias, const float* R, float* C, long ldc, long sC1, long sC2, int M, int N,
                        int K, int batch1, int batch2, int nsplit, long sCsplit, float alpha, hipStream_t st);
// what: NULL, or a string LITERAL under which the launch is bracketed for the profile (genie_profile_kernels, GENIE_KC_OTHER)
int launch_slab_reduce(const float* part, int ns, size_t n, float* out, float beta, hipStream_t st, const char* what = nullptr);
int launch_wgrad_f32(const float* dY, long ldy, const float* X, long ldx, float* dW, int Mtok, int N, int K, float alpha,
                     float beta, float* slabs, size_t slab_floats, hipStream_t st);
constexpr int COLSUM_CHUNKS = 256;  // row chunks of the two-stage column sums (= slabs of their scratch)
int launch_colsum(const float* Y, long ld, long rows, int N, float* out, float beta, float* part, hipStream_t st);
size_t ln_bwd_scratch_floats(int C);
int launch_ln_bwd(const float* x, const float* gamma, const float* dy, float* dxout, float* dgamma, float* dbeta,
                  long rows, int C, float eps, float beta, float* part, hipStream_t st);
int launch_gelu_fwd(const float* z, float* h, size_t n, hipStream_t st);
int launch_gelu_bwd(const float* z, float* g, size_t n, hipStream_t st);
int launch_embed_bwd(const genie_cfg& c, const float* dx, const int64_t* ids, int B, float* dpos, float* dmask,
                     float* const* tables_host, float beta, float* colpart, hipStream_t st);
// gradient of the action table: d_table[k] = sum over frames (b, t) with act_ids[b, t] == k (ascending) of sum_s dx[b, t, s, :];
// frame_sums: (B * T, d) f32 scratch.  Fixed order, no atomics.
int launch_action_embed_bwd(const genie_cfg& c, const float* dx, const int64_t* act_ids, int n_act, int B, float* d_table,
                            float beta, float* frame_sums, hipStream_t st);
int launch_sumsq(const float* x, size_t n, double* out, double* scratch, hipStream_t st);
// kernels_dropout.hip: MLP dropout of the training step.  DropKey: one mask of one call -- the Philox key (the seed), counter words 2
// and 3 (stream = layer * 2 + site, the caller's micro-batch counter) and the keep threshold (element kept iff its word >= thr)
struct DropKey { uint32_t k0, k1, stream, call, thr; };
int launch_drop_gelu_fwd(const float* z, float* h, size_t n, const DropKey& k, hipStream_t st);   // h = m * gelu(z)
int launch_drop_gelu_bwd(const float* z, float* g, size_t n, const DropKey& k, hipStream_t st);   // g = m * g * gelu'(z), in place
// out = (add, NULL: 0) + m * (s * in), n f32 values (in == out, add == out allowed); npl_out 1 / 2: also out16 = launch_cast16(npl_out, out)
int launch_drop_axpy(int npl_out, const float* in, const float* add, float* out, uint16_t* out16, size_t n, float s, const DropKey& k,
                     hipStream_t st);
int launch_drop_zero16(int npl, uint16_t* h16, size_t n, const DropKey& k, hipStream_t st);       // h16 = m * h16 in every plane, in place
int launch_dropout_mask(uint8_t* keep, size_t n, const DropKey& k, hipStream_t st);              // the keep bytes (genie_dropout_mask)
// 16-bit operand copies (kernels_train16.hip); npl = 1 bf16, 2 = f16 split planes [hi | lo]
// colpart != NULL: also the column sums of the (post-gelu') values: slabs [rows/64][cols] for launch_slab_reduce
// scale16 (npl == 2 only): the split copies hold in * scale16, saturated at +-65504 (the column sums and the MODE 1 write-back
// are unscaled); the consumer folds 1 / scale16 into its alpha
int launch_cast_transpose16(int npl, float* in, long ld, const float* z, uint16_t* out16, uint16_t* out16T, int rows,
                            int cols, hipStream_t st, float* colpart = nullptr, float scale16 = 1.0f);
// f16x3 training: every gradient operand (d logits, dY, dz) is split as hi + lo/2048 of 2^12 times its value.  A loss averaged
// over n tokens has gradients of order 1/n and below; under 2^-14 an f16 hi is flushed to zero (split_f16), the value then lives in
// lo alone and the three-product GEMM (hi.hi + hi.lo + lo.hi, no lo.lo) multiplies it with the hi half of the other operand only:
// 11 bits of the weight or activation instead of 22, 1e-4 of a gradient tensor's largest element at a few hundred tokens.  Scaled
// by 2^12 values down to 1.5e-8 keep a normal hi; values of 16 and above saturate at the f16 range instead of overflowing.
constexpr float GRAD_SCALE16 = 4096.0f;
int launch_transpose16(int npl, const uint16_t* in, uint16_t* outT, int rows, int cols, hipStream_t st);
// bf16 copy in the same orientation (+ gelu'(z)) and the [rows/64][cols] column-sum partials; no transposed copy
int launch_cast_rows16(const float* in, long ld, const float* z, uint16_t* out16, int rows, int cols, hipStream_t st,
                       float* colpart);
// dW[N,K] (beta*dW +)= alpha * dY^T . X from ROW-MAJOR bf16 dY (Mtok, N) and X (Mtok, K) (kernels_gemm_tn.hip)
int launch_wgrad16_tn(const uint16_t* dY, long ldy, const uint16_t* X, long ldx, float* dW, int Mtok, int N, int K, float alpha,
                      float beta, float* slabs, size_t slab_floats, hipStream_t st);
int launch_cast16(int npl, const float* src, uint16_t* dst, size_t n, hipStream_t st);
// The flags of the 16-bit GEMMs (launch_gemm16_ex and the launchers behind it), the one vocabulary of kernels and drivers
enum { G16X_GELU = 1, G16X_ACCUM = 2, G16X_OUT16 = 4, G16X_OUTF32 = 8,
       G16X_GELU16 = 16 /* GELU on the 16-bit output only (bf16: gelu16_2 polynomial): Cf keeps the pre-activation (training forward) */,
       G16X_NT = 32 /* non-temporal output stores: the output is larger than the on-die caches (set by the launchers) */,
       G16X_QKV = 64 /* gemm16_pp only: the spatial-attention operand layout, see launch_gemm16_pp */,
       G16X_QKNORM = 128 /* with G16X_QKV: q and k leave through the per-head LayerNorm (qn_g, qn_b; attention.py:31-34, 42-47) */,
       // launch_gemm16_ex only: read and stripped there, they never reach a kernel
       G16X_WIDEW = 1024 /* f16x3: W is not a |w| < 32 weight matrix (a `w16_wide` tensor of genie_hip.h, or an activation / gradient
                            operand of the training step): keep it off the 2^11-scaling single-accumulator kernel (gemm16_pp) */,
       G16X_NOSM = 2048 /* not the in-workgroup split-K kernel of small problems (gemm16_sm): the caller splits K itself, or promises a
                           sum order that does not depend on the problem size */ };
int launch_gemm16_ex(int npl, const uint16_t* A, long lda, long planeA, const uint16_t* W, long ldw, long planeW,
                     const float* bias, const float* Rf, float* Cf, uint16_t* C16, long plane16, long ldc, int M, int N,
                     int K, int flags, float alpha, hipStream_t st, int batch, long strideA, long strideW, long strideC);
// kernels_gemm_pp.hip: the 256x256 two-group phase-scheduled GEMM; GENIE_E_UNSUPPORTED when the shape does not fit it
int launch_gemm16_pp(int npl, int terms, int f16, const uint16_t* A, long lda, long planeA, const uint16_t* W, long ldw,
                     long planeW, const float* bias, const float* Rf, float* Cf, uint16_t* C16, long plane16, long ldc, int M,
                     int N, int K, int flags, float alpha, hipStream_t st, int batch, long strideA, long strideW, long strideC,
                     float qscale = 1.0f, int head_dim = 0, const float* qn_g = nullptr, const float* qn_b = nullptr);
// kernels_attn_bwd.hip: the f32 attention backward of the training step (every precision's temporal backward; the spatial one of exact
// and f16x3) and the qk-norm pair around it
int launch_softmax_rows(float* P, long rows, int N, hipStream_t st);
int launch_softmax_bwd_rows(const float* P, float* dP, long rows, int N, hipStream_t st);
// q, k rows are read from `qk` (leading dim qk_ld; q at column 0, k at column d), v from qkv
int launch_attn_temporal_bwd(const float* qkv, const float* qk, long qk_ld, const float* dO, float* dqkv, int B, int T,
                             int S, int d, int H, int Dh, float scale, hipStream_t st);
int launch_attn_spatial_bwd_fused(const float* qkv, const float* qk, long qk_ld, const float* dO, float* dqkv, long n_bt, int S,
                                  int d, int H, int Dh, float scale, hipStream_t st);
// the geometries the fused kernel takes (its launcher answers GENIE_E_UNSUPPORTED for the others)
inline bool attn_spatial_bwd_fused_takes(int S, int Dh) { return S == 256 && (Dh == 64 || Dh == 32); }
// floats of `part` behind launch_qk_norm_bwd (0: head_dim not in {32, 64, 128})
size_t qk_norm_bwd_scratch_floats(int Dh);
int launch_qk_norm_fwd(const float* qkv, float* qkn, const float* nw, const float* nb, long M, int H, int Dh, int d,
                       hipStream_t st);
int launch_qk_norm_bwd(const float* qkv, float* dqkv, const float* nw, float* dnw, float* dnb, long M, int H, int Dh,
                       int d, float beta, float* part, hipStream_t st);
// kernels_attn_bwd16.hip: spatial attention backward on the bf16 matrix cores (bf16 training precision)
int launch_attn_spatial_bwd_bf16(const float* qkv, const float* qk, long qk_ld, const float* dO, float* dqkv, float* stats, long n_bt,
                                 int S, int d, int H, int Dh, float scale, hipStream_t st);
inline bool attn_spatial_bwd_bf16_takes(int S, int Dh, long qk_ld, int d) {
    return S == 256 && (Dh == 64 || Dh == 32) && qk_ld % 4 == 0 && d % 4 == 0;
}
// the operand form of src (M, N) f32 as that call's G16X_OUT16 epilogue writes it for (M, N, K), row-major operands (kernels_bf16.hip)
int launch_cast16_like_gemm(int npl, const float* src, uint16_t* dst, int M, int N, int K, int flags, hipStream_t st);
// kernels_gemm_sm.hip: small (latency-bound) problems; GENIE_E_UNSUPPORTED = not small / tiling does not fit
bool gemm16_sm_takes(int npl, long lda, long planeA, long ldw, long planeW, long plane16, long ldc, int M, int N, int K, int flags,
                     int batch);
int launch_gemm16_sm(int npl, const uint16_t* A, long lda, long planeA, const uint16_t* W, long ldw, long planeW,
                     const float* bias, const float* Rf, float* Cf, uint16_t* C16, long plane16, long ldc, int M, int N, int K,
                     int flags, float alpha, hipStream_t st, int batch, long strideA, long strideW, long strideC);
int launch_gemm16_sm_ln(int npl, const float* x, long ldx, const float* ln_g, const float* ln_b, float eps, const uint16_t* W,
                        long ldw, long planeW, const float* bias, const float* Rf, float* Cf, uint16_t* C16, long plane16, long ldc,
                        int M, int N, int K, int flags, float alpha, hipStream_t st);
// kernels_frame.hip: the one-frame passes of generate on fragment-ordered operands (GENIE_PREC_F16X3)
int launch_pack_frame_w16(const float* src, uint16_t* dst, int N, int K, hipStream_t st);
bool frame_path_takes(const genie_cfg& c, const genie_layer_weights& lw, long rows);
int frame_prepare_f16x3(const genie_cfg& c, const float* x, Workspace& w, int B, int nf, hipStream_t st);
// p: the DECODE pass of this layer (cache slice, first slot, frames per clip of the cache)
int st_block_frame_f16x3(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, int B, int nf,
                         bool want_xs, hipStream_t st);
int launch_frame_linear(const uint16_t* A, const uint16_t* W, const float* bias, float* y, int M, int N, int K, int mode, hipStream_t st);
int readout_frame_f16x3(const genie_cfg& c, const genie_weights& wt, Workspace& w, int B, int nf, int f_out, float* logits,
                        hipStream_t st);
// kernels_attn_dma.hip: spatial attention over the operand planes written by launch_gemm16_pp(G16X_OUT16 | G16X_QKV)
int launch_attn_spatial_dma(int npl, const uint16_t* qkv16, long n_seq, int d, int H, int Dh, uint16_t* out16, size_t out_plane,
                            hipStream_t st);
// st_block.hip: the layer drivers (exact; 16-bit = GENIE_PREC_BF16 or GENIE_PREC_F16X3 by c.precision), what runs in front of the first
// 16-bit layer and the readout behind the last one (all three precisions)
int st_block_exact(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, int B, hipStream_t st);
int st_block16(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, BlockCarry& carry, int B,
               hipStream_t st);
int prepare16(const genie_cfg& c, const float* x, Workspace& w, int B, hipStream_t st);
int readout(const genie_cfg& c, const genie_weights& wt, const float* x, Workspace& w, int B, int t0, int t1, int layout, float* logits,
            hipStream_t st);
// kernels_bf16.hip: elementwise steps of those drivers, and the 16-bit Linear entries of the C ABI
int launch_splitk2_residual(float* x, const float* s0, const float* s1, const float* bias, size_t n4, int N, hipStream_t st);
int launch_shadow_bf16(const float* src, uint16_t* dst, size_t n, hipStream_t st);
int launch_pack_split(const float* src, uint16_t* dst, size_t n, hipStream_t st);
int launch_linear_lowp(int precision, const uint16_t* x16, const uint16_t* W16, const float* b, float* y, int M, int N, int K, int gelu,
                       int accumulate, hipStream_t st);

// (One description of the GEMM in place of the three copies of its decode / strided / dense shape logic in the drivers.)
// Where the temporal qkv GEMM of a pass writes and how it is batched: `base + off` (f32 elements; a bf16 qkv lives at the same element
// offset of the same base), `rows` rows per batch entry, `batch` entries strideA / strideC elements apart.
//   DECODE: slot frame_t of the cache slice (fan-out: slot frame_t - fan_P0 of the branch slice), one entry per clip;  a short CLEAN pass into a longer cache at B > 1: one entry per clip;
//   otherwise ONE dense (M, 3d) GEMM into the cache slice (CLEAN) or into `dense`
struct TemporalQkv {
    float* base;
    size_t off;
    int rows, batch;
    long strideA, strideC;
};
inline TemporalQkv temporal_qkv_target(const genie_cfg& c, const BlockPass& p, float* dense, int B) {
    const int d = c.d_model, Tq = p.tq_stride(c.T);
    if (p.is_decode())
        return {p.cache, (size_t)(p.frame_t - p.fan_P0) * c.S * 3 * d, c.S, B, (long)c.S * d, (long)p.frame_T * c.S * 3 * d};
    float* base = p.writes_cache() ? p.cache : dense;
    if (Tq != c.T && B > 1) return {base, 0, c.T * c.S, B, (long)c.T * c.S * d, (long)Tq * c.S * 3 * d};
    return {base, 0, B * c.T * c.S, 1, 0, 0};
}
// f32 rows -> a 16-bit driver's operand form: f16 split planes (plane != 0: hi at out16, lo at out16 + plane) or bf16 (plane == 0) --
// the (out16, plane) convention of the attention launchers above, which take the same pair
inline int launch_to_operand16(const float* src, uint16_t* out16, size_t plane, size_t n, hipStream_t st) {
    return plane ? launch_split_f16(src, out16, plane, n, st) : launch_pack_bf16(src, out16, n, st);
}
// Temporal attention behind that GEMM (st_block.hip), for all drivers: decode slot / prefix / f32-MFMA / generic kernel.  The result leaves as
// f32 rows (out) or, out16 != NULL, 16-bit: bf16 (plane == 0) or f16 split planes (hi at out16, lo at out16 + plane); a kernel that
// cannot write 16-bit writes f32 into w.logits and a convert follows.  in16: the qkv and the cache hold bf16 (temporal_qkv16).
int temporal_attention(const genie_cfg& c, const genie_attn_weights& aw, const BlockPass& p, const TemporalQkv& tq, float* out,
                       uint16_t* out16, size_t plane, bool in16, Workspace& w, int B, hipStream_t st);

int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, float grad_mult, const double* sumsq, float max_norm, hipStream_t st);
// EMA of the weights (kernels_train.hip): launch_adamw's update and ema -= omd * (ema - p_new) in one pass; that line alone; a <-> b
int launch_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_mult, const double* sumsq, float max_norm, float omd, hipStream_t st);
int launch_ema_update(float* ema, const float* p, size_t n, float omd, hipStream_t st);
int launch_swap_f32(float* a, float* b, size_t n, hipStream_t st);

// LoRA adapters (kernels_lora.hip): what one launch is told, by value -- the caller's items, the running tile counts of the merge /
// project grid (`first`) and block counts of the reduce grid (`rfirst`, segments dA, dB per item), and where each item's slabs lie
constexpr int LORA_MAX_ITEMS = GENIE_LORA_MAX_ITEMS, LORA_MAX_RANK = GENIE_LORA_MAX_RANK;
struct LoraTable {
    genie_lora_item it[LORA_MAX_ITEMS];
    size_t da_off[LORA_MAX_ITEMS], db_off[LORA_MAX_ITEMS];   // floats into scratch
    float* scratch;
    int first[LORA_MAX_ITEMS + 1], rfirst[2 * LORA_MAX_ITEMS + 1];
    int n;
};
bool lora_table(const genie_lora_item* items, int n, LoraTable& tb, size_t& scratch_floats);
int launch_lora_merge(const LoraTable& tb, hipStream_t st);
int launch_lora_project(const LoraTable& tb, int accumulate, hipStream_t st);

// Muon (kernels_muon.hip): how one table is laid out in the workspace.  Items of equal (rows, cols) form a group (in order of first
// appearance) and lie back to back in X0 and X1, so each product of the iteration is one launch per group with the item index in the grid.
constexpr int MUON_MAX_ITEMS = GENIE_MUON_MAX_ITEMS;
struct MuonPlan {
    struct Group {
        int rows, cols, first, count;   // items order[first .. first + count)
        size_t x_off;                   // floats into X0 / X1
    } group[MUON_MAX_ITEMS];
    int order[MUON_MAX_ITEMS];
    size_t x_of[MUON_MAX_ITEMS];        // per item (caller's index): floats into X0 / X1
    size_t off_x0, off_x1, off_a, off_p, total_floats;   // floats into the workspace; the 64 f64 partial sums per item lie at 0
    int n, ngroups;
};
bool muon_plan(const genie_muon_item* items, int n, MuonPlan& pl);
int launch_muon_step(const genie_muon_item* items, const MuonPlan& pl, const genie_muon_settings& s, float* ws, hipStream_t st);
int launch_newton_schulz(const float* in, float* out, int rows, int cols, int batch, int steps, float a, float b, float c, float eps,
                         const MuonPlan& pl, float* ws, hipStream_t st);

// api.hip: the host helpers its entry points share with the generate loops (generate_api.hip)
Workspace carve(const genie_cfg& c, int B, void* base);   // base == NULL: sizes only
int check_cfg(const genie_cfg* c);
int check_ws(const genie_cfg& c, int B, void* ws, size_t bytes);
int decoder(const genie_cfg& c, const genie_weights& wt, float* x, Workspace& w, int B, hipStream_t st);
int mask_count(int step, int steps, int S);
double mask_fraction(int step, int steps);   // cos(pi/2 * (step+1)/steps) as mask_count takes it
// what a caller's decode options must satisfy, checked on the host before anything is enqueued (NULL = none; where: the entry point)
int check_sampling(const genie_sampling* sp, const char* where);
int check_unmask(int unmask_mode, bool ex, int steps, const float* noise, const char* where);
int check_guidance(const genie_guidance* g, const genie_frame_cond* cond, const char* where);
extern const genie_sampling kDefaultSampling;
// The split cache of a fan-out call (genie_generate_fanout): the B clips of a decode pass are K branches each of B / K parent clips.
// Slots [0, P0) live in `trunk`, a T-slot cache of B / K clips that the context pass filled and no decode pass writes; slot j >= P0 is
// slot j - P0 of the pass's own cache, (L, B, Tb, S, 3d).
struct FanOut {
    const float* trunk;
    int K, P0, Tb;
};
inline size_t fanout_branch_bytes(const genie_cfg& c, size_t NBK, int Tb) {
    return (size_t)c.num_layers * NBK * Tb * c.S * 3 * c.d_model * sizeof(float);
}
// genie_frames_pass_cond, and with fan != NULL the decode pass of a fan-out call
int frames_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t0, int nf, float* cache,
                size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                const FanOut* fan);

// kernels_metrics.hip: image-space metrics of two (n, C, H, W) uint8 batches (genie_frame_metrics).  The caller has checked H, W >= 11 and
// that n * frame_metrics_tiles (the workgroups of the launch, one workspace record each) is at most 2^31 - 1
long frame_metrics_tiles(int C, int H, int W);
size_t frame_metrics_workspace_bytes(long n, int C, int H, int W);
int launch_frame_metrics(const uint8_t* a, const uint8_t* b, long n, int C, int H, int W, double* out, void* workspace, hipStream_t st);

}  // namespace genie
