// C ABI of libgenie_hip.so (include/genie_hip.h): argument checking, workspace carving and the
// launch sequences of the single passes (the layer itself and the readout: st_block.hip; the generate loops over these passes:
// generate_api.hip).  All work is enqueued on the caller's stream; nothing here allocates, synchronises or touches the host-side of any tensor.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "common.hpp"
#include "kernels.hpp"

namespace genie {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-launch event profiler ------------------------------------------------------------------
static int g_prof_mask = 0;
static int g_prof_n = 0;
static hipEvent_t* g_prof_ev = nullptr;  // 2 * GENIE_PROFILE_MAX_LAUNCHES events, created on first enable
static int g_prof_cls[GENIE_PROFILE_MAX_LAUNCHES];
static double g_prof_flops[GENIE_PROFILE_MAX_LAUNCHES], g_prof_bytes[GENIE_PROFILE_MAX_LAUNCHES];
static const char* g_prof_name[GENIE_PROFILE_MAX_LAUNCHES];

ProfScope::ProfScope(int cls, double flops, double bytes, hipStream_t s, const char* kernel) : slot(-1), st(s) {
    if (!(g_prof_mask & (1 << cls)) || g_prof_n >= GENIE_PROFILE_MAX_LAUNCHES || !g_prof_ev) return;
    slot = g_prof_n++;
    g_prof_cls[slot] = cls;
    g_prof_flops[slot] = flops;
    g_prof_bytes[slot] = bytes;
    g_prof_name[slot] = kernel ? kernel : "(unnamed)";
    (void)hipEventRecord(g_prof_ev[2 * slot], st);
}
ProfScope::~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof_ev[2 * slot + 1], st);
}

// Workspace carving (struct Workspace: kernels.hpp).  All offsets 256-byte aligned.
Workspace carve(const genie_cfg& c, int B, void* base) {
    Workspace w;
    const size_t M = (size_t)B * c.T * c.S;
    const size_t wide = (size_t)(3 * c.d_model > c.hidden ? 3 * c.d_model : c.hidden);
    const size_t V = (size_t)c.factored_vocab * c.num_factored;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* r = p ? (void*)(p + off) : nullptr;
        off += align_up(bytes, 256);
        return r;
    };
    w.x = (float*)take(M * c.d_model * 4);
    w.xn = take(M * c.d_model * 4);
    w.big = take(M * wide * 4);
    // w.logits doubles as the (M, d) f32 scratch of the 16-bit blocks' generic attention path (st_block.hip): V < d happens
    w.logits = (float*)take(M * (V > (size_t)c.d_model ? V : (size_t)c.d_model) * 4);
    w.samples = (int64_t*)take((size_t)B * c.S * 8);
    w.conf = (float*)take((size_t)B * c.S * 4);
    w.unmasked = (uint8_t*)take((size_t)B * c.S);
    w.aux = take(M * c.d_model * 4);
    w.total = off;
    return w;
}

int check_cfg(const genie_cfg* c) {
    GENIE_CHECK_ARG(c != nullptr, "cfg is NULL");
    GENIE_CHECK_SHAPE(c->num_layers >= 1 && c->num_heads >= 1, "num_layers/num_heads must be >= 1");
    GENIE_CHECK_SHAPE(c->d_model == c->num_heads * c->head_dim, "d_model %d != num_heads %d * head_dim %d", c->d_model,
                      c->num_heads, c->head_dim);
    GENIE_CHECK_SHAPE(c->head_dim == 16 || c->head_dim == 32 || c->head_dim == 64,
                      "head_dim %d unsupported (16/32/64)", c->head_dim);
    GENIE_CHECK_SHAPE(c->d_model % 16 == 0 && c->d_model <= 2048, "d_model %d must be a multiple of 16, <= 2048",
                      c->d_model);
    GENIE_CHECK_SHAPE(c->hidden % 16 == 0 && c->hidden > 0, "hidden %d must be a positive multiple of 16", c->hidden);
    GENIE_CHECK_SHAPE(c->T >= 1 && c->T <= 64 && (c->T & (c->T - 1)) == 0, "T=%d must be a power of two <= 64", c->T);
    GENIE_CHECK_SHAPE(c->S >= 1 && c->S <= 1024, "S=%d must be in [1,1024]", c->S);
    GENIE_CHECK_SHAPE((size_t)c->S * c->head_dim * 8 <= 160 * 1024, "S=%d x head_dim=%d exceeds LDS", c->S,
                      c->head_dim);
    GENIE_CHECK_SHAPE(c->num_factored >= 1 && c->num_factored <= 4, "num_factored %d unsupported", c->num_factored);
    GENIE_CHECK_SHAPE(c->factored_vocab >= 1, "factored_vocab must be >= 1");
    {   // image_vocab_size (the mask id) must be factored_vocab ^ num_factored: sampled ids hi * vf + lo stay below it
        int64_t p = 1;
        for (int j = 0; j < c->num_factored && p <= c->image_vocab_size; ++j) p *= c->factored_vocab;
        GENIE_CHECK_SHAPE(p == c->image_vocab_size, "image_vocab_size %d != factored_vocab %d ^ num_factored %d",
                          c->image_vocab_size, c->factored_vocab, c->num_factored);
    }
    GENIE_CHECK_SHAPE(c->precision == GENIE_PREC_EXACT || c->precision == GENIE_PREC_BF16 ||
                          c->precision == GENIE_PREC_F16X3,
                      "unknown precision %d", c->precision);
    if (c->precision == GENIE_PREC_BF16)
        GENIE_CHECK_SHAPE(c->d_model % 64 == 0 && c->hidden % 64 == 0, "bf16 precision needs d_model, hidden %% 64 == 0");
    if (c->precision == GENIE_PREC_F16X3)
        GENIE_CHECK_SHAPE(c->d_model % 32 == 0 && c->hidden % 32 == 0, "f16x3 precision needs d_model, hidden %% 32 == 0");
    return GENIE_OK;
}

int check_ws(const genie_cfg& c, int B, void* ws, size_t bytes) {
    GENIE_CHECK_ARG(B >= 1, "B=%d must be >= 1", B);
    GENIE_CHECK_ARG(ws != nullptr, "workspace is NULL");
    size_t need = carve(c, B, nullptr).total;
    GENIE_CHECK_ARG(bytes >= need, "workspace too small: %zu < %zu bytes", bytes, need);
    return GENIE_OK;
}

// The layer loop of every pass: what runs in front of the first block, then `n` blocks, block i as the pass `make(i, next)` says
// (next = the block behind it, NULL after the last).  The hand-offs between consecutive blocks live and die here.
template <class MakePass>
static int run_layers(const genie_cfg& c, const genie_layer_weights* layers, int n, float* x, Workspace& w, int B, hipStream_t st,
                      MakePass make) {
    const bool exact = c.precision == GENIE_PREC_EXACT;   // else a 16-bit precision: one driver for both (st_block.hip)
    if (!exact) GENIE_TRY(prepare16(c, x, w, B, st));
    BlockCarry carry;
    for (int i = 0; i < n; ++i) {
        const BlockPass p = make(i, i + 1 < n ? &layers[i + 1] : nullptr);
        GENIE_STUDY_LAYER(i);
        if (exact) GENIE_TRY(st_block_exact(c, layers[i], x, w, p, B, st));
        else GENIE_TRY(st_block16(c, layers[i], x, w, p, carry, B, st));
    }
    return GENIE_OK;
}

int decoder(const genie_cfg& c, const genie_weights& wt, float* x, Workspace& w, int B, hipStream_t st) {
    return run_layers(c, wt.layers_host, c.num_layers, x, w, B, st,
                      [&](int, const genie_layer_weights* next) { return BlockPass::plain(c, next, c.T); });
}

double mask_fraction(int step, int steps) {
    double u = (double)(step + 1) / (double)steps;
    return cos(u * M_PI / 2.0);
}

int mask_count(int step, int steps, int S) {
    // n = ceil(cos(pi/2 * (step+1)/steps) * S), python float math (st_mask_git.py:17-26,199)
    return (int)ceil(mask_fraction(step, steps) * (double)S);
}

// a genie_sampling law (NULL = none), checked on the host before anything is enqueued
int check_sampling(const genie_sampling* sp, const char* where) {
    if (!sp) return GENIE_OK;
    GENIE_CHECK_ARG(sp->logit_temperature > 0.f && sp->logit_temperature <= 3.0e38f,
                    "%s: sampling: logit_temperature %g must be positive and finite", where, (double)sp->logit_temperature);
    GENIE_CHECK_ARG(sp->top_k >= 0, "%s: sampling: top_k %d must be >= 0", where, sp->top_k);
    GENIE_CHECK_ARG(sp->top_p == sp->top_p, "%s: sampling: top_p is NaN", where);
    GENIE_CHECK_ARG(sp->choice_temperature >= 0.f, "%s: sampling: choice_temperature %g must be >= 0", where,
                    (double)sp->choice_temperature);
    return GENIE_OK;
}
// unmask_mode and the draws it needs; GENIE_UNMASK_CONFIDENCE only through the *_ex entry points (ex)
int check_unmask(int unmask_mode, bool ex, int steps, const float* noise, const char* where) {
    const bool known = unmask_mode == GENIE_UNMASK_RANDOM || unmask_mode == GENIE_UNMASK_GREEDY ||
                       (ex && unmask_mode == GENIE_UNMASK_CONFIDENCE);
    if (!known) {
        set_error(ex ? "Expected `unmask_mode` to be one of ['greedy', 'random', 'confidence']"
                     : "Expected `unmask_mode` to be one of ['greedy', 'random']");
        return GENIE_E_UNSUPPORTED;
    }
    GENIE_CHECK_ARG(steps <= 1 || unmask_mode == GENIE_UNMASK_GREEDY || noise,
                    "%s: '%s' unmasking with steps > 1 needs the caller's U[0,1) draws", where,
                    unmask_mode == GENIE_UNMASK_CONFIDENCE ? "confidence" : "random");
    return GENIE_OK;
}
// a genie_guidance (NULL = none) and the condition it needs, checked on the host before anything is enqueued
int check_guidance(const genie_guidance* g, const genie_frame_cond* cond, const char* where) {
    if (!g) return GENIE_OK;
    GENIE_CHECK_ARG(isfinite(g->scale), "%s: guidance: scale %g must be finite", where, (double)g->scale);
    GENIE_CHECK_ARG(cond && cond->n_actions > 0, "%s: guidance needs an action condition (cond with n_actions > 0)", where);
    GENIE_CHECK_ARG(g->null_action >= 0 && g->null_action < cond->n_actions, "%s: guidance: null_action %d outside [0, %d)", where,
                    (int)g->null_action, (int)cond->n_actions);
    return GENIE_OK;
}
// the confidence mode's scale when the caller gave no law: the documented default of choice_temperature
const genie_sampling kDefaultSampling = {1.0f, 0, 1.0f, 4.5f};

}  // namespace genie

using namespace genie;

extern "C" {

int genie_version(void) { return GENIE_ABI_VERSION; }
int genie_abi_layout(size_t* out_host, int n) {
    const size_t v[12] = {sizeof(genie_cfg), sizeof(genie_attn_weights), offsetof(genie_attn_weights, fused_w16),
                          offsetof(genie_attn_weights, w16_wide), sizeof(genie_layer_weights),
                          offsetof(genie_layer_weights, mlp_fused_w16), offsetof(genie_layer_weights, w16_wide),
                          sizeof(genie_weights), offsetof(genie_weights, out_w16_wide), offsetof(genie_attn_weights, frame_w16),
                          offsetof(genie_layer_weights, mlp_frame_w16), offsetof(genie_weights, out_frame_w16)};
    for (int i = 0; i < n && i < 12 && out_host; ++i) out_host[i] = v[i];
    return 12;
}
int genie_sampling_layout(size_t* out_host, int n) {
    const size_t v[5] = {sizeof(genie_sampling), offsetof(genie_sampling, logit_temperature), offsetof(genie_sampling, top_k),
                         offsetof(genie_sampling, top_p), offsetof(genie_sampling, choice_temperature)};
    for (int i = 0; i < n && i < 5 && out_host; ++i) out_host[i] = v[i];
    return 5;
}
int genie_guidance_layout(size_t* out_host, int n) {
    const size_t v[3] = {sizeof(genie_guidance), offsetof(genie_guidance, scale), offsetof(genie_guidance, null_action)};
    for (int i = 0; i < n && i < 3 && out_host; ++i) out_host[i] = v[i];
    return 3;
}
int genie_known_layout(size_t* out_host, int n) {
    const size_t v[3] = {sizeof(genie_known), offsetof(genie_known, ids), offsetof(genie_known, clip_stride)};
    for (int i = 0; i < n && i < 3 && out_host; ++i) out_host[i] = v[i];
    return 3;
}
int genie_action_proj_layout(size_t* out_host, int n) {
    const size_t v[6] = {sizeof(genie_action_proj), offsetof(genie_action_proj, weight), offsetof(genie_action_proj, bias),
                         offsetof(genie_action_proj, mean), offsetof(genie_action_proj, inv_std), offsetof(genie_action_proj, action_dim)};
    for (int i = 0; i < n && i < 6 && out_host; ++i) out_host[i] = v[i];
    return 6;
}
static int check_action_proj(const genie_action_proj* p, int64_t n, int d_model, const char* where) {
    GENIE_CHECK_ARG(p != nullptr, "%s: NULL genie_action_proj", where);
    GENIE_CHECK_ARG(p->action_dim >= 1 && d_model >= 1 && n >= 0, "%s: action_dim %d, d_model %d, n %lld must be >= 1, >= 1, >= 0", where,
                    p->action_dim, d_model, (long long)n);
    GENIE_CHECK_SHAPE(p->action_dim <= GENIE_ACTION_MAX_DIM && d_model <= 1024, "%s: action_dim %d / d_model %d beyond %d / 1024", where,
                      p->action_dim, d_model, GENIE_ACTION_MAX_DIM);
    return GENIE_OK;
}
int genie_action_rows(const genie_action_proj* p, const float* vecs, float* rows, int64_t n, int d_model, void* stream) {
    GENIE_TRY(check_action_proj(p, n, d_model, "genie_action_rows"));
    GENIE_CHECK_ARG(p->weight && vecs && rows, "genie_action_rows: NULL pointer");
    return launch_action_rows(*p, vecs, rows, (long)n, d_model, as_stream(stream));
}
int genie_action_rows_backward(const genie_action_proj* p, const float* vecs, const float* d_rows, int64_t n, int d_model,
                               float* d_weight, float* d_bias, int accumulate, void* stream) {
    GENIE_TRY(check_action_proj(p, n, d_model, "genie_action_rows_backward"));
    GENIE_CHECK_ARG(vecs && d_rows && d_weight, "genie_action_rows_backward: NULL pointer");
    if (n == 0) return GENIE_OK;
    return launch_action_rows_backward(*p, vecs, d_rows, (long)n, d_model, d_weight, d_bias, accumulate, as_stream(stream));
}
static int check_frame_metrics(int64_t n, int C, int H, int W) {
    GENIE_CHECK_ARG(n >= 0 && C >= 1, "genie_frame_metrics: n %lld, C %d must be >= 0, >= 1", (long long)n, C);
    GENIE_CHECK_SHAPE(H >= 11 && W >= 11, "genie_frame_metrics: frames of %d x %d are smaller than the 11 x 11 SSIM window", H, W);
    // one workgroup per (image, channel, tile); the first factor in double, so that the product cannot wrap
    GENIE_CHECK_SHAPE((double)C * ((double)H / 32 + 1) * ((double)W / 32 + 1) < 2.0e9 && n <= 0x7fffffffL / frame_metrics_tiles(C, H, W),
                      "genie_frame_metrics: n %lld x %d x %d x %d exceeds the 2^31 - 1 tiles of one call", (long long)n, C, H, W);
    return GENIE_OK;
}
size_t genie_frame_metrics_workspace_bytes(int64_t n, int C, int H, int W) {
    if (check_frame_metrics(n, C, H, W) != GENIE_OK) return 0;
    return frame_metrics_workspace_bytes((long)n, C, H, W);
}
int genie_frame_metrics(const uint8_t* a, const uint8_t* b, int64_t n, int C, int H, int W, double* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    GENIE_CHECK_ARG(a && b && out, "genie_frame_metrics: NULL pointer");
    GENIE_TRY(check_frame_metrics(n, C, H, W));
    if (n == 0) return GENIE_OK;
    const size_t need = frame_metrics_workspace_bytes((long)n, C, H, W);
    GENIE_CHECK_ARG(workspace && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0 && (uintptr_t)out % 8 == 0,
                    "genie_frame_metrics: workspace of %zu bytes, %zu needed (8-byte aligned, like out)", workspace ? workspace_bytes : (size_t)0, need);
    return launch_frame_metrics(a, b, (long)n, C, H, W, out, workspace, as_stream(stream));
}
const char* genie_last_error(void) { return g_err; }
int genie_check_config(const genie_cfg* cfg) { return check_cfg(cfg); }

size_t genie_workspace_bytes(const genie_cfg* cfg, int B) {
    if (check_cfg(cfg) != GENIE_OK || B < 1) return 0;
    return carve(*cfg, B, nullptr).total;
}

int genie_pack_bf16(const float* src, uint16_t* dst, size_t n, void* stream) {
    GENIE_CHECK_ARG(src && dst, "pack_bf16: NULL pointer");
    return launch_pack_bf16(src, dst, n, as_stream(stream));
}

int genie_pack_split_f16(const float* src, uint16_t* dst, size_t n, void* stream) {
    GENIE_CHECK_ARG(src && dst, "pack_split_f16: NULL pointer");
    return launch_pack_split(src, dst, n, as_stream(stream));
}

int genie_embed(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, float* x, void* stream) {
    return genie_embed_cond(cfg, w, ids, B, x, stream, nullptr);
}

int genie_embed_cond(const genie_cfg* cfg, const genie_weights* w, const int64_t* ids, int B, float* x, void* stream,
                     const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(w && ids && x && B >= 1, "embed: bad argument");
    GENIE_CHECK_ARG(w->pos_embed && w->mask_embed && w->embed[0], "embed: weight table incomplete");
    GENIE_TRY(check_frame_cond(cond, "embed"));
    EmbedAct act;
    return launch_embed(*cfg, *w, ids, B, x, as_stream(stream), frame_act(cond, cfg->S, 0, cfg->T, act));
}

int genie_layer_norm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps,
                     void* stream) {
    GENIE_CHECK_ARG(x && gamma && beta && y && rows >= 0 && C >= 1, "layer_norm: bad argument");
    if (rows == 0) return GENIE_OK;
    return launch_layer_norm(x, gamma, beta, y, rows, C, eps, as_stream(stream));
}

int genie_linear(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int gelu,
                 int accumulate, void* stream) {
    GENIE_CHECK_ARG(x && W && y && M >= 0 && N >= 1 && K >= 1, "linear: bad argument");
    int flags = (gelu ? GEMM_GELU : 0) | (accumulate ? GEMM_ACCUM : 0);
    return launch_gemm_f32(x, K, 0, W, K, 0, b, y, N, 0, M, N, K, 1, flags, 1.0f, as_stream(stream));
}

int genie_spatial_attention(const genie_cfg* cfg, const genie_attn_weights* aw, const float* qkv, float* out, int B,
                            void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && qkv && out && B >= 1, "spatial_attention: bad argument");
    const genie_cfg& c = *cfg;
    const float* nw = c.qk_norm ? aw->norm_w : nullptr;
    const float* nb = c.qk_norm ? aw->norm_b : nullptr;
    int rc = launch_attn_spatial_f32_mfma(qkv, out, c.S, (long)B * c.T, c.d_model, c.num_heads, c.head_dim,
                                          c.attn_scale, nw, nb, as_stream(stream));
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    return launch_attn_generic(qkv, out, c.S, (long)B * c.T, 1, c.S, 0, 1, c.d_model, c.num_heads, c.head_dim,
                               c.attn_scale, 0, nw, nb, as_stream(stream));
}

int genie_temporal_attention(const genie_cfg* cfg, const genie_attn_weights* aw, const float* qkv, float* out, int B,
                             void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && qkv && out && B >= 1, "temporal_attention: bad argument");
    const genie_cfg& c = *cfg;
    const float* nw = c.qk_norm ? aw->norm_w : nullptr;
    const float* nb = c.qk_norm ? aw->norm_b : nullptr;
    int rc = launch_attn_temporal_f32_mfma(qkv, out, B, c.T, c.S, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw,
                                           nb, as_stream(stream));
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    return launch_attn_generic(qkv, out, c.T, (long)B * c.S, c.S, (long)c.T * c.S, 1, c.S, c.d_model, c.num_heads,
                               c.head_dim, c.attn_scale, 1, nw, nb, as_stream(stream));
}

int genie_linear_lowp(int precision, const uint16_t* x16, const uint16_t* W16, const float* b, float* y, int M, int N,
                      int K, int gelu, int accumulate, void* stream) {
    GENIE_CHECK_ARG(x16 && W16 && y && M >= 0 && N >= 1 && K >= 1, "linear_lowp: bad argument");
    return launch_linear_lowp(precision, x16, W16, b, y, M, N, K, gelu, accumulate, as_stream(stream));
}

int genie_attention_core(const float* qkv, float* out, int n_seq, int N, int num_heads, int head_dim, float scale,
                         int causal, const float* norm_w, const float* norm_b, void* stream) {
    GENIE_CHECK_ARG(qkv && out && n_seq >= 0 && N >= 1 && num_heads >= 1, "attention_core: bad argument");
    GENIE_CHECK_ARG((norm_w == nullptr) == (norm_b == nullptr), "attention_core: norm_w/norm_b must come together");
    if (n_seq == 0) return GENIE_OK;
    if (!causal) {
        int rc = launch_attn_spatial_f32_mfma(qkv, out, N, n_seq, num_heads * head_dim, num_heads, head_dim, scale,
                                              norm_w, norm_b, as_stream(stream));
        if (rc != GENIE_E_UNSUPPORTED) return rc;
    }
    return launch_attn_generic(qkv, out, N, n_seq, 1, N, 0, 1, num_heads * head_dim, num_heads, head_dim, scale,
                               causal, norm_w, norm_b, as_stream(stream));
}

int genie_st_block_forward(const genie_cfg* cfg, const genie_layer_weights* lw_host, float* x, int B, void* workspace,
                           size_t workspace_bytes, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(lw_host && x, "st_block_forward: NULL pointer");
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    Workspace w = carve(*cfg, B, workspace);
    return run_layers(*cfg, lw_host, 1, x, w, B, as_stream(stream),
                      [&](int, const genie_layer_weights* next) { return BlockPass::plain(*cfg, next, cfg->T); });
}

int genie_decoder_forward(const genie_cfg* cfg, const genie_weights* wt, float* x, int B, void* workspace,
                          size_t workspace_bytes, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && wt->layers_host && x, "decoder_forward: NULL pointer");
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    Workspace w = carve(*cfg, B, workspace);
    return decoder(*cfg, *wt, x, w, B, as_stream(stream));
}

int genie_readout_logits(const genie_cfg* cfg, const genie_weights* wt, const float* x, int B, int t0, int t1,
                         int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && x && logits && B >= 1, "readout_logits: bad argument");
    GENIE_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= cfg->T, "readout_logits: bad frame range [%d,%d)", t0, t1);
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    Workspace w = carve(*cfg, B, workspace);
    if (t0 == t1) return GENIE_OK;
    return readout(*cfg, *wt, x, w, B, t0, t1, layout, logits, as_stream(stream));
}

int genie_compute_logits(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int t0, int t1,
                         int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    return genie_compute_logits_cond(cfg, wt, ids, B, t0, t1, layout, logits, workspace, workspace_bytes, stream, nullptr);
}

int genie_compute_logits_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int t0, int t1,
                              int layout, float* logits, void* workspace, size_t workspace_bytes, void* stream,
                              const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && logits, "compute_logits: NULL pointer");
    GENIE_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= cfg->T, "compute_logits: bad frame range [%d,%d)", t0, t1);
    GENIE_TRY(check_frame_cond(cond, "compute_logits"));
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    Workspace w = carve(*cfg, B, workspace);
    hipStream_t st = as_stream(stream);
    EmbedAct act;
    GENIE_TRY(launch_embed(*cfg, *wt, ids, B, w.x, st, frame_act(cond, cfg->S, 0, cfg->T, act)));
    GENIE_TRY(decoder(*cfg, *wt, w.x, w, B, st));
    if (t0 == t1) return GENIE_OK;
    return readout(*cfg, *wt, w.x, w, B, t0, t1, layout, logits, st);
}

// ---- teacher-forced prefix reuse ---------------------------------------------------------------------
size_t genie_prefix_cache_bytes(const genie_cfg* cfg, int B) {
    if (check_cfg(cfg) != GENIE_OK || B < 1) return 0;
    return (size_t)cfg->num_layers * B * cfg->T * cfg->S * 3 * cfg->d_model * sizeof(float);
}

// model_T: T of the model's own config (c is the pass's private copy with fewer frames)
static int prefix_forward(const genie_cfg& c, const genie_weights& wt, const int64_t* ids, int B, float* cache, bool clean, int tshift,
                          int model_T, Workspace& w, hipStream_t st, int cache_frames = 0, const EmbedAct* act = nullptr) {
    if (cache_frames <= 0) cache_frames = c.T;  // frames per clip in the cache layout (L, B, cache_frames, S, 3d)
    const size_t per_layer = (size_t)B * cache_frames * c.S * 3 * c.d_model;
    GENIE_TRY(launch_embed(c, wt, ids, B, w.x, st, act));
    return run_layers(c, wt.layers_host, c.num_layers, w.x, w, B, st, [&](int i, const genie_layer_weights* next) {
        float* slice = cache + i * per_layer;  // (a clean pass stops after its last temporal qkv: nothing reads its final hidden state)
        return clean ? BlockPass::clean(c, next, model_T, slice, cache_frames) : BlockPass::prefix(c, next, model_T, slice, tshift);
    });
}

// The prefix passes run on `nframes` <= T frame slots per clip: a private copy of the config with T = nframes (dense
// (B, nframes, S, *) buffers) and the positional table advanced to clip frame `frame0`.
static int prefix_view(const genie_cfg* cfg, const genie_weights* wt, int B, int frame0, int nframes, size_t cache_bytes,
                       genie_cfg& c2, genie_weights& w2, int cache_frames = 0) {
    if (cache_frames <= 0) cache_frames = nframes;
    GENIE_CHECK_ARG(nframes >= 1 && frame0 >= 0 && frame0 + nframes <= cfg->T, "prefix pass: frames [%d, %d) outside the clip (T=%d)",
                    frame0, frame0 + nframes, cfg->T);
    c2 = *cfg;
    c2.T = nframes;
    w2 = *wt;
    w2.pos_embed = wt->pos_embed + (size_t)frame0 * cfg->S * cfg->d_model;  // pos_embed_TSC[0, frame0 + i]
    GENIE_CHECK_ARG(cache_frames >= nframes && cache_frames <= cfg->T, "prefix pass: cache_frames %d outside [%d, %d]", cache_frames,
                    nframes, cfg->T);
    const size_t need = (size_t)cfg->num_layers * B * cache_frames * cfg->S * 3 * cfg->d_model * sizeof(float);
    GENIE_CHECK_ARG(cache_bytes >= need, "prefix pass: cache too small (%zu < %zu bytes)", cache_bytes, need);
    return GENIE_OK;
}

int genie_clean_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int nframes, int cache_frames,
                     float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return genie_clean_pass_cond(cfg, wt, ids, B, nframes, cache_frames, cache, cache_bytes, workspace, workspace_bytes, stream,
                                 nullptr);
}

int genie_clean_pass_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int nframes,
                          int cache_frames, float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && cache, "clean_pass: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "clean_pass"));
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    genie_cfg c2;
    genie_weights w2;
    GENIE_TRY(prefix_view(cfg, wt, B, 0, nframes, cache_bytes, c2, w2, cache_frames));
    if (cache_frames != nframes && B > 1 && !(nframes >= 8 && nframes <= 16 && (cfg->head_dim == 32 || cfg->head_dim == 64))) {
        set_error("clean_pass: a strided cache (cache_frames %d != nframes %d) at B > 1 needs 8 <= nframes <= 16 and head_dim 32/64",
                  cache_frames, nframes);
        return GENIE_E_UNSUPPORTED;
    }
    Workspace w = carve(c2, B, workspace);
    EmbedAct act;
    return prefix_forward(c2, w2, ids, B, cache, true, 0, cfg->T, w, as_stream(stream), cache_frames,
                          frame_act(cond, cfg->S, 0, cfg->T, act));
}

int genie_masked_frames_logits(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frames, int B, int frame0,
                               int nframes, const float* cache, size_t cache_bytes, float* logits, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return genie_masked_frames_logits_cond(cfg, wt, frames, B, frame0, nframes, cache, cache_bytes, logits, workspace,
                                           workspace_bytes, stream, nullptr);
}

int genie_masked_frames_logits_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frames, int B,
                                    int frame0, int nframes, const float* cache, size_t cache_bytes, float* logits,
                                    void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && wt->layers_host && frames && cache && logits, "masked_frames_logits: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "masked_frames_logits"));
    GENIE_CHECK_ARG(frame0 == 0 || frame0 == 1, "masked_frames_logits: frame0 = %d (0 or 1)", frame0);
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    genie_cfg c2;
    genie_weights w2;
    GENIE_TRY(prefix_view(cfg, wt, B, frame0, nframes, cache_bytes, c2, w2));
    Workspace w = carve(c2, B, workspace);
    hipStream_t st = as_stream(stream);
    EmbedAct act;   // slot i is clip frame frame0 + i
    GENIE_TRY(prefix_forward(c2, w2, frames, B, const_cast<float*>(cache), false, frame0, cfg->T, w, st, 0,
                             frame_act(cond, cfg->S, frame0, cfg->T, act)));
    return readout(c2, w2, w.x, w, B, 0, nframes, GENIE_LAYOUT_TOKEN_MAJOR, logits, st);
}

int genie_frames_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t0, int nf, float* cache,
                      size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    return genie_frames_pass_cond(cfg, wt, frame_ids, B, t0, nf, cache, cache_bytes, logits, workspace, workspace_bytes, stream,
                                  nullptr);
}

}  // extern "C"

// genie_frames_pass_cond, and with fan != NULL the decode pass of a fan-out call (generate_api.hip): `cache` is then the branch cache, and
// every such pass has t0 >= P0 -- nothing writes the trunk after the context pass
int genie::frames_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t0, int nf, float* cache,
                       size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream,
                       const genie_frame_cond* cond, const FanOut* fan) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && wt->layers_host && frame_ids && cache, "frames_pass: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "frames_pass"));
    GENIE_CHECK_ARG(nf >= 1 && t0 >= 0 && t0 + nf <= cfg->T, "frames_pass: frames [%d, %d) out of range", t0, t0 + nf);
    genie_cfg c1 = *cfg;
    c1.T = nf;  // every buffer of this pass is a dense (B, nf, S, *) tensor
    if (fan) {   // (the call sized its workspace for its own passes, not for B * K clips of T frames)
        GENIE_CHECK_ARG(B >= 1 && fan->K >= 1 && B % fan->K == 0 && fan->trunk, "frames_pass: %d clips in branches of %d", B, fan->K);
        GENIE_CHECK_ARG(t0 >= fan->P0 && t0 + nf <= fan->P0 + fan->Tb, "frames_pass: frames [%d, %d) outside the branch slots [%d, %d)", t0,
                        t0 + nf, fan->P0, fan->P0 + fan->Tb);
        GENIE_CHECK_ARG(cache_bytes >= fanout_branch_bytes(*cfg, (size_t)B, fan->Tb), "frames_pass: branch cache too small");
        GENIE_CHECK_ARG(workspace && workspace_bytes >= carve(c1, B, nullptr).total, "frames_pass: workspace too small");
    } else {
        GENIE_CHECK_ARG(cache_bytes >= genie_prefix_cache_bytes(cfg, B), "frames_pass: cache too small");
        GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    }
    // the fragment-order kernels (kernels_frame.hip) take the pass when they cover every layer; several frames per pass exist
    // only there
    // (the decode attention kernel holds 16 cache slots; the readout Linear writes 64-column tiles with no tail handling)
    bool fr = cfg->precision == GENIE_PREC_F16X3 && wt->out_frame_w16 && cfg->T <= 16 && (cfg->factored_vocab * cfg->num_factored) % 64 == 0;
    for (int i = 0; fr && i < c1.num_layers; ++i) fr = frame_path_takes(c1, wt->layers_host[i], (long)B * nf * cfg->S);
    if (nf > 1 && !fr) {
        set_error("frames_pass: %d frames per pass need the fragment-order kernels (f16x3, head_dim 64 or 32, frame_w16 "
                  "streams, B * nf * S <= 16,384 rows)", nf);
        return GENIE_E_UNSUPPORTED;
    }
    Workspace w = carve(c1, B, workspace);
    hipStream_t st = as_stream(stream);
    genie_weights w1 = *wt;
    w1.pos_embed = wt->pos_embed + (size_t)t0 * cfg->S * cfg->d_model;  // pos_embed_TSC[0, t0 + i]
    EmbedAct act;   // ... and the action of clip frame t0 + i
    GENIE_TRY(launch_embed(c1, w1, frame_ids, B, w.x, st, frame_act(cond, cfg->S, t0, cfg->T, act)));
    const size_t slot = (size_t)cfg->S * 3 * cfg->d_model;
    const size_t per_layer = (size_t)B * (fan ? fan->Tb : cfg->T) * slot, per_trunk = fan ? (size_t)(B / fan->K) * cfg->T * slot : 0;
    auto make = [&](int i, const genie_layer_weights* next) {
        if (fan)
            return BlockPass::decode_fanout(c1, next, cfg->T, cache + i * per_layer, t0, fan->trunk + i * per_trunk, fan->P0, fan->K, fan->Tb);
        return BlockPass::decode(c1, next, cfg->T, cache + i * per_layer, t0);
    };
    if (!fr) {
        GENIE_TRY(run_layers(c1, wt->layers_host, c1.num_layers, w.x, w, B, st, make));
    } else {
        GENIE_TRY(frame_prepare_f16x3(c1, w.x, w, B, nf, st));
        for (int i = 0; i < c1.num_layers; ++i) {
            const BlockPass p = make(i, i + 1 < c1.num_layers ? &wt->layers_host[i + 1] : nullptr);
            GENIE_TRY(st_block_frame_f16x3(c1, wt->layers_host[i], w.x, w, p, B, nf, logits && !p.next_is_ln, st));
        }
    }
    if (!logits) return GENIE_OK;
    if (fr) return readout_frame_f16x3(c1, *wt, w, B, nf, nf - 1, logits, st);
    return readout(c1, *wt, w.x, w, B, 0, 1, GENIE_LAYOUT_TOKEN_MAJOR, logits, st);
}

extern "C" {

int genie_frames_pass_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t0, int nf,
                           float* cache, size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes,
                           void* stream, const genie_frame_cond* cond) {
    return frames_pass(cfg, wt, frame_ids, B, t0, nf, cache, cache_bytes, logits, workspace, workspace_bytes, stream, cond, nullptr);
}

int genie_frame_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t, float* cache,
                     size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    return genie_frame_pass_cond(cfg, wt, frame_ids, B, t, cache, cache_bytes, logits, workspace, workspace_bytes, stream, nullptr);
}

int genie_frame_pass_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t,
                          float* cache, size_t cache_bytes, float* logits, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond) {
    return genie_frames_pass_cond(cfg, wt, frame_ids, B, t, 1, cache, cache_bytes, logits, workspace, workspace_bytes, stream,
                                  cond);
}

int genie_frame_linear(const uint16_t* a_fr, const uint16_t* w_fr, const float* bias, float* y, int M, int N, int K, int mode, void* stream) {
    GENIE_CHECK_ARG(a_fr && w_fr && y && mode >= 0 && mode <= 2, "frame_linear: bad argument");
    return launch_frame_linear(a_fr, w_fr, bias, y, M, N, K, mode, as_stream(stream));
}

int genie_score_logits(const genie_cfg* cfg, const float* logits, const int64_t* targets, int64_t target_clip_stride, int K, int64_t N,
                       double* nll, int64_t nll_stride, double* hits, float* token_nll, int64_t token_stride, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(logits && targets && nll, "score_logits: NULL pointer");
    GENIE_CHECK_ARG(K >= 1 && N >= 1 && N <= 0x7fffffffLL, "score_logits: %lld rows in branches of %d", (long long)N, K);
    GENIE_CHECK_ARG(target_clip_stride >= 0 && nll_stride >= 1, "score_logits: target stride %lld, nll stride %lld", (long long)target_clip_stride,
                    (long long)nll_stride);
    GENIE_CHECK_ARG(!token_nll || token_stride >= cfg->S, "score_logits: token_nll stride %lld below S = %d", (long long)token_stride, cfg->S);
    GENIE_CHECK_ARG(((uintptr_t)logits & 15) == 0, "score_logits: logits must be 16-byte aligned");
    return launch_score_rows(*cfg, logits, targets, (long)target_clip_stride, K, (long)N, nll, (long)nll_stride, hits, token_nll,
                             (long)token_stride, as_stream(stream));
}

int genie_temporal_attention_decode_fanout(const genie_cfg* cfg, const genie_attn_weights* aw, const float* trunk_slice,
                                           const float* branch_slice, float* out, int NBK, int K, int P0, int Tb, int t, int in16,
                                           void* stream) {
    GENIE_CHECK_ARG(cfg && aw && branch_slice && out, "temporal_attention_decode_fanout: NULL pointer");
    const genie_cfg& c = *cfg;   // (only the attention geometry is read: head_dim 8 is not a model's, but it is this kernel's)
    GENIE_CHECK_SHAPE(c.num_heads >= 1 && c.d_model == c.num_heads * c.head_dim && c.S >= 1 && c.T >= 1 && c.T <= 64,
                      "temporal_attention_decode_fanout: d_model %d, %d heads of %d, S=%d, T=%d", c.d_model, c.num_heads, c.head_dim, c.S, c.T);
    GENIE_CHECK_ARG(NBK >= 1 && K >= 1 && NBK % K == 0, "temporal_attention_decode_fanout: %d clips in branches of %d", NBK, K);
    GENIE_CHECK_ARG(P0 >= 0 && P0 <= t && t < c.T && Tb >= 1 && t - P0 < Tb, "temporal_attention_decode_fanout: slot %d, trunk slots [0, %d) of %d, "
                    "%d branch slots", t, P0, c.T, Tb);
    GENIE_CHECK_ARG(trunk_slice || P0 == 0, "temporal_attention_decode_fanout: NULL trunk with P0 = %d", P0);
    GENIE_CHECK_ARG(!c.qk_norm || (aw->norm_w && aw->norm_b), "temporal_attention_decode_fanout: qk_norm without norm_w / norm_b");
    const float* nw = c.qk_norm ? aw->norm_w : nullptr;
    const float* nb = c.qk_norm ? aw->norm_b : nullptr;
    // the dense form (no trunk, one branch per clip) is the ordinary decode kernel; that launcher refuses slices of more than 64 slots
    if (!trunk_slice && K == 1 && P0 == 0 && Tb <= 64)
        return launch_attn_temporal_single(branch_slice, out, NBK, Tb, c.S, t, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw, nb,
                                           as_stream(stream), nullptr, 0, in16 != 0);
    return launch_attn_temporal_single_fanout(branch_slice, out, NBK, Tb, c.S, t, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw, nb,
                                              as_stream(stream), nullptr, 0, in16 != 0,
                                              FanSplit<true>{trunk_slice ? trunk_slice : branch_slice, c.T, P0, K});
}

int genie_pack_frame_w16(const float* src, uint16_t* dst, int N, int K, void* stream) {
    GENIE_CHECK_ARG(src && dst, "pack_frame_w16: NULL pointer");
    return launch_pack_frame_w16(src, dst, N, K, as_stream(stream));
}

int genie_factored_ce(const genie_cfg* cfg, const float* logits, int layout, const int64_t* targets,
                      const int64_t* weight_ids, int B, int t0, int t1, double* sums_out, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(logits && targets && sums_out && B >= 1, "factored_ce: bad argument");
    GENIE_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= cfg->T, "factored_ce: bad frame range [%d,%d)", t0, t1);
    return launch_factored_ce(*cfg, logits, layout, targets, weight_ids, B, t0, t1, sums_out, as_stream(stream));
}

int genie_metric_hits(const int64_t* truth, int64_t truth_batch_stride, const int64_t* samples, int64_t samples_batch_stride,
                      int batch, int64_t n_per_batch, const double* ce3, double n_tokens, double n_frames, double n_clips,
                      double* sums6, void* stream) {
    GENIE_CHECK_ARG(truth && samples && sums6 && batch >= 0 && n_per_batch >= 0, "metric_hits: bad argument");
    return launch_count_equal(truth, (long)truth_batch_stride, samples, (long)samples_batch_stride, batch, (long)n_per_batch, ce3,
                              sums6, n_tokens, n_frames, n_clips, as_stream(stream));
}

int genie_readout_ce(const genie_cfg* cfg, const genie_weights* wt, const float* x, const int64_t* targets,
                     const int64_t* weight_ids, int B, int t0, int t1, double* sums_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(wt && x && targets && sums_out, "readout_ce: NULL pointer");
    GENIE_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= cfg->T, "readout_ce: bad frame range [%d,%d)", t0, t1);
    GENIE_TRY(check_ws(*cfg, B, workspace, workspace_bytes));
    if (t0 == t1) return GENIE_OK;
    Workspace w = carve(*cfg, B, workspace);
    hipStream_t st = as_stream(stream);
    GENIE_TRY(readout(*cfg, *wt, x, w, B, t0, t1, GENIE_LAYOUT_TOKEN_MAJOR, w.logits, st));
    return launch_factored_ce(*cfg, w.logits, GENIE_LAYOUT_TOKEN_MAJOR, targets, weight_ids, B, t0, t1, sums_out, st);
}

int genie_sample(const genie_cfg* cfg, const float* logits, int layout, int B, float temperature,
                 const float* uniforms, int64_t* samples, float* conf, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(logits && samples && conf && B >= 1, "sample: bad argument");
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "sample: temperature > 0 needs caller-supplied uniforms");
    return launch_sample(*cfg, logits, layout, B, temperature, uniforms, samples, conf, as_stream(stream));
}

int genie_sample_ex(const genie_cfg* cfg, const float* logits, int layout, int B, float temperature, const float* uniforms,
                    int64_t* samples, float* conf, void* stream, const genie_sampling* sampling, float* keys_out,
                    const float* noise, float anneal) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(logits && samples && conf && B >= 1, "sample: bad argument");
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "sample: temperature > 0 needs caller-supplied uniforms");
    GENIE_TRY(check_sampling(sampling, "sample"));
    GENIE_CHECK_ARG(!keys_out || noise, "sample: keys_out needs the caller's U[0,1) noise draws");
    GENIE_CHECK_ARG(!keys_out || anneal == anneal, "sample: anneal is NaN");
    return launch_sample_ex(*cfg, logits, layout, B, temperature, uniforms, samples, conf,
                            (keys_out && !sampling) ? &kDefaultSampling : sampling, keys_out, noise, anneal, as_stream(stream));
}

int genie_sample_guided(const genie_cfg* cfg, const float* logits_cond, const float* logits_null, int layout, int B, float temperature,
                        const float* uniforms, int64_t* samples, float* conf, void* stream, const genie_sampling* sampling,
                        float* keys_out, const float* noise, float anneal, float scale) {
    GENIE_CHECK_ARG(isfinite(scale), "sample_guided: scale %g must be finite", (double)scale);
    if (scale == 1.0f)
        return genie_sample_ex(cfg, logits_cond, layout, B, temperature, uniforms, samples, conf, stream, sampling, keys_out, noise, anneal);
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(logits_cond && logits_null && samples && conf && B >= 1, "sample_guided: bad argument");
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "sample_guided: temperature > 0 needs caller-supplied uniforms");
    GENIE_TRY(check_sampling(sampling, "sample_guided"));
    GENIE_CHECK_ARG(!keys_out || noise, "sample_guided: keys_out needs the caller's U[0,1) noise draws");
    GENIE_CHECK_ARG(!keys_out || anneal == anneal, "sample_guided: anneal is NaN");
    return launch_sample_guided(*cfg, logits_cond, logits_null, layout, B, temperature, uniforms, samples, conf,
                                (keys_out && !sampling) ? &kDefaultSampling : sampling, keys_out, noise, anneal, scale, as_stream(stream));
}

int genie_guide_logits(const float* cond, const float* null_logits, float* out, size_t n, float scale, void* stream) {
    GENIE_CHECK_ARG(isfinite(scale), "guide_logits: scale %g must be finite", (double)scale);
    GENIE_CHECK_ARG(cond && null_logits && out && n <= (size_t)0x7fffffffffffffffLL, "guide_logits: bad argument");
    return launch_guide_logits(cond, null_logits, out, 1, (long)n, 0, 0, scale, as_stream(stream));
}

int genie_mask_step(const float* keys, int n, int last_step, int64_t mask_id, uint8_t* unmasked, int64_t* samples,
                    int64_t* prompt_frame, int64_t prompt_clip_stride, int B, int S, void* stream) {
    GENIE_CHECK_ARG(unmasked && samples && prompt_frame && B >= 1 && S >= 1, "mask_step: bad argument");
    GENIE_CHECK_ARG(last_step || keys, "mask_step: keys required unless last_step");
    GENIE_CHECK_ARG(last_step || (n >= 0 && n <= S), "mask_step: n=%d out of range", n);
    return launch_mask_step(keys, n, last_step, mask_id, unmasked, samples, prompt_frame, (long)prompt_clip_stride, B,
                            S, as_stream(stream));
}

double genie_mask_fraction(int step, int steps) { return steps >= 1 ? mask_fraction(step, steps) : 0.0; }

int genie_known_begin(const int64_t* known, int64_t known_clip_stride, int64_t mask_id, int64_t* frame, int64_t frame_clip_stride,
                      uint8_t* unmasked, int B, int S, int copies, void* stream) {
    GENIE_CHECK_ARG(known && frame && B >= 1 && S >= 1 && (copies == 1 || copies == 2), "known_begin: bad argument");
    GENIE_CHECK_ARG(B <= 0x3fffffff, "known_begin: B=%d too large", B);
    return launch_known_begin(known, (long)known_clip_stride, mask_id, frame, (long)frame_clip_stride, unmasked, B, S, copies,
                              as_stream(stream));
}

int genie_mask_step_known(const float* keys, double frac, int last_step, int64_t mask_id, const int64_t* known, int64_t known_clip_stride,
                          uint8_t* unmasked, int64_t* samples, int64_t* prompt_frame, int64_t prompt_clip_stride, int B, int S,
                          void* stream) {
    GENIE_CHECK_ARG(unmasked && samples && prompt_frame && B >= 1 && S >= 1, "mask_step_known: bad argument");
    GENIE_CHECK_ARG(last_step || keys, "mask_step_known: keys required unless last_step");
    GENIE_CHECK_ARG(last_step || (frac >= 0.0 && frac <= 1.0), "mask_step_known: frac=%g outside [0, 1]", frac);
    return launch_mask_step_known(keys, frac, last_step, mask_id, known, (long)known_clip_stride, unmasked, samples, prompt_frame,
                                  (long)prompt_clip_stride, B, S, as_stream(stream));
}

int genie_profile_enable(int class_mask) {
    if (class_mask && !g_prof_ev) {
        g_prof_ev = new hipEvent_t[2 * GENIE_PROFILE_MAX_LAUNCHES];
        for (int i = 0; i < 2 * GENIE_PROFILE_MAX_LAUNCHES; ++i) {
            if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) {
                set_error("profile: hipEventCreate failed at %d", i);
                return GENIE_E_LAUNCH;
            }
        }
    }
    g_prof_mask = class_mask;
    return GENIE_OK;
}

int genie_profile_reset(void) {
    g_prof_n = 0;
    return GENIE_OK;
}

int genie_profile_read(int kernel_class, double* out4) {
    GENIE_CHECK_ARG(out4 && kernel_class >= 0 && kernel_class < GENIE_KC_COUNT, "profile_read: bad argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    for (int i = 0; i < g_prof_n; ++i) {
        if (g_prof_cls[i] != kernel_class) continue;
        if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) { set_error("profile: sync failed"); return GENIE_E_LAUNCH; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess) {
            set_error("profile: elapsed failed");
            return GENIE_E_LAUNCH;
        }
        out4[0] += 1.0;
        out4[1] += ms;
        out4[2] += g_prof_flops[i];
        out4[3] += g_prof_bytes[i];
    }
    return GENIE_OK;
}

int genie_profile_kernels(int kernel_class, char* buf, size_t buf_bytes) {
    GENIE_CHECK_ARG(buf && buf_bytes >= 64 && kernel_class >= 0 && kernel_class < GENIE_KC_COUNT, "profile_kernels: bad argument");
    // distinct kernel names of the class (string literals: compared by content), launches / ms / flops each
    constexpr int MAXK = 32;
    const char* names[MAXK];
    double n[MAXK], ms[MAXK], fl[MAXK];
    int nk = 0;
    for (int i = 0; i < g_prof_n; ++i) {
        if (g_prof_cls[i] != kernel_class) continue;
        int k = 0;
        while (k < nk && strcmp(names[k], g_prof_name[i]) != 0) ++k;
        if (k == nk) {
            if (nk == MAXK) continue;
            names[nk] = g_prof_name[i]; n[nk] = ms[nk] = fl[nk] = 0.0; ++nk;
        }
        if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) { set_error("profile: sync failed"); return GENIE_E_LAUNCH; }
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess) { set_error("profile: elapsed failed"); return GENIE_E_LAUNCH; }
        n[k] += 1.0; ms[k] += t; fl[k] += g_prof_flops[i];
    }
    size_t off = 0;
    buf[0] = 0;
    for (int k = 0; k < nk; ++k) {
        const int w = snprintf(buf + off, buf_bytes - off, "%s\t%.0f\t%.6f\t%.6e\n", names[k], n[k], ms[k], fl[k]);
        if (w < 0 || (size_t)w >= buf_bytes - off) break;
        off += (size_t)w;
    }
    return GENIE_OK;
}

int genie_pack_temporal_fused_bf16(const float* qkv_w, const float* proj_w, uint16_t* dst, void* stream) {
    GENIE_CHECK_ARG(qkv_w && proj_w && dst, "pack_temporal_fused: NULL pointer");
    return launch_pack_temporal_fused(qkv_w, proj_w, dst, as_stream(stream));
}
int genie_pack_temporal_qkv_f16x3(const float* qkv_w, uint16_t* dst, void* stream) {
    GENIE_CHECK_ARG(qkv_w && dst, "pack_temporal_qkv_f16x3: NULL pointer");
    return launch_pack_temporal_qkv_f16x3(qkv_w, dst, as_stream(stream));
}
int genie_temporal_prefix_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, float* x, uint16_t* kv, int B, int nframes, int mode,
                                     int shift, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && x && kv && B >= 1 && nframes >= 1, "temporal_prefix_fused: bad argument");
    genie_cfg c2 = *cfg;
    c2.T = nframes;   // the pass's frames; cfg->T is the model's
    return launch_temporal_prefix_fused_bf16(c2, *aw, x, kv, B, mode, shift, cfg->T, as_stream(stream));
}
int genie_temporal_qkv_attn_f16x3(const genie_cfg* cfg, const genie_attn_weights* aw, const float* x, uint16_t* a16, int64_t plane_elems,
                                  float* kv, int B, int nframes, int mode, int shift, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && x && a16 && B >= 1 && nframes >= 1, "temporal_qkv_attn_f16x3: bad argument");
    genie_cfg c2 = *cfg;
    c2.T = nframes;
    return launch_temporal_qkv_attn_f16x3(c2, *aw, x, a16, (long)plane_elems, kv, B, mode, shift, cfg->T, as_stream(stream));
}
int genie_temporal_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, const uint16_t* x16, float* x, int B, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && x && B >= 1, "temporal_fused: bad argument");   // x16 == NULL: operands rounded from x itself
    return launch_temporal_fused_bf16(*cfg, *aw, x16, x, B, as_stream(stream));
}
int genie_mlp_fused_bf16(const genie_cfg* cfg, const genie_layer_weights* lw, float* x, uint16_t* x16_out, int64_t rows,
                         const float* next_norm_w, const float* next_norm_b, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(lw && x && rows >= 0, "mlp_fused: bad argument");
    return launch_mlp_fused_bf16(*cfg, *lw, x, x16_out, (long)rows, as_stream(stream), next_norm_w, next_norm_b);
}
int genie_mlp_fused_qkv_bf16(const genie_cfg* cfg, const genie_layer_weights* lw, const genie_layer_weights* next, float* x,
                             uint16_t* planes, int64_t rows, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(lw && next && x && planes && rows >= 0, "mlp_fused_qkv: bad argument");
    if (!next->spatial.fused_w16 || !(next->spatial.w16_wide & GENIE_FUSED_QKV_STREAM) || !next->norm1_w || !next->norm1_b)
        return GENIE_E_UNSUPPORTED;
    return launch_mlp_fused_bf16(*cfg, *lw, x, nullptr, (long)rows, as_stream(stream), next->norm1_w, next->norm1_b,
                                 next->spatial.fused_w16 + GENIE_SPATIAL_PROJ_FUSED_ELEMS, planes);
}
int genie_pack_spatial_proj_fused_bf16(const float* proj_w, uint16_t* dst, void* stream) {
    GENIE_CHECK_ARG(proj_w && dst, "pack_spatial_proj_fused: NULL pointer");
    return launch_pack_spatial_proj(proj_w, dst, as_stream(stream));
}
int genie_pack_spatial_qkv_fused_bf16(const float* qkv_w, uint16_t* dst, void* stream) {
    GENIE_CHECK_ARG(qkv_w && dst, "pack_spatial_qkv_fused: NULL pointer");
    return launch_pack_spatial_qkv(qkv_w, dst, as_stream(stream));
}
int genie_spatial_attn_proj_fused_bf16(const genie_cfg* cfg, const genie_attn_weights* aw, const uint16_t* qkv_planes, float* x,
                                       uint16_t* x16, int64_t n_seq, void* stream) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_CHECK_ARG(aw && qkv_planes && x && n_seq >= 1, "spatial_attn_proj_fused: bad argument");   // x16 == NULL: no bf16 shadow written
    return launch_spatial_attn_proj_bf16(*cfg, *aw, qkv_planes, x, x16, (long)n_seq, as_stream(stream));
}
int genie_pack_mlp_fused_bf16(const float* fc1_w, const float* fc2_w, uint16_t* dst, void* stream) {
    GENIE_CHECK_ARG(fc1_w && fc2_w && dst, "pack_mlp_fused: NULL pointer");
    return launch_pack_mlp_fused(fc1_w, fc2_w, dst, as_stream(stream));
}

int genie_study_build(void) { return kStudyBuild ? 1 : 0; }

int genie_bits_from_tokens(const int64_t* ids, float* z, int n, int hw, int bits, void* stream) {
    GENIE_CHECK_ARG(ids && z && n >= 0 && hw >= 1 && bits >= 1 && bits <= 62, "bits_from_tokens: bad argument");
    return launch_bits(ids, z, n, hw, bits, as_stream(stream));
}

int genie_rescale_u8_bf16(const uint16_t* x, uint8_t* out, size_t n, void* stream) {
    GENIE_CHECK_ARG(x && out, "rescale_u8: NULL pointer");
    return launch_rescale_u8(x, 1, out, n, as_stream(stream));
}
int genie_rescale_u8_f32(const float* x, uint8_t* out, size_t n, void* stream) {
    GENIE_CHECK_ARG(x && out, "rescale_u8: NULL pointer");
    return launch_rescale_u8(x, 0, out, n, as_stream(stream));
}
int genie_tokens_from_bits(const float* h, int64_t* ids, int n, int hw, int bits, void* stream) {
    GENIE_CHECK_ARG(h && ids && n >= 0 && hw >= 1 && bits >= 1 && bits <= 62, "tokens_from_bits: bad argument");
    return launch_tokens_from_bits(h, ids, n, hw, bits, as_stream(stream));
}

int genie_pack_conv_weight(const float* w, uint16_t* out, int Cout, int Cin, int taps, void* stream) {
    GENIE_CHECK_ARG(w && out && Cout >= 1 && Cin >= 1 && taps >= 1, "pack_conv_weight: bad argument");
    return launch_pack_conv_weight(w, out, Cout, Cin, taps, as_stream(stream));
}
int genie_conv3x3_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* residual, uint16_t* y,
                       const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, int depth_to_space, void* stream) {
    GENIE_CHECK_ARG(x && w_packed && y && zero_page && n >= 0 && H >= 1 && W >= 1, "conv3x3: bad argument");
    return launch_conv3x3_igemm(x, w_packed, bias, residual, y, zero_page, n, H, W, Cin, Cout, depth_to_space,
                                as_stream(stream));
}
int genie_conv3x3_s2_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, uint16_t* y,
                          const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, void* stream) {
    GENIE_CHECK_ARG(x && w_packed && y && zero_page && n >= 0 && H >= 1 && W >= 1, "conv3x3_s2: bad argument");
    return launch_conv3x3_igemm(x, w_packed, bias, nullptr, y, zero_page, n, H, W, Cin, Cout, 0, as_stream(stream), 2);
}
int genie_frames_to_nhwc_bf16(const uint8_t* frames, uint16_t* x, int n, int HW, int cin, int cpad, void* stream) {
    GENIE_CHECK_ARG(frames && x && n >= 0 && HW >= 1 && cin >= 1 && cpad >= cin, "frames_to_nhwc: bad argument");
    return launch_frames_to_nhwc(frames, x, n, HW, cin, cpad, as_stream(stream));
}
int genie_tokens_from_code_nhwc_bf16(const uint16_t* h, int64_t* ids, int64_t n_pix, int bits, int cpad, void* stream) {
    GENIE_CHECK_ARG(h && ids && n_pix >= 0 && bits >= 1 && bits <= 62 && cpad >= bits, "tokens_from_code: bad argument");
    return launch_tokens_from_nhwc(h, ids, (long)n_pix, bits, cpad, as_stream(stream));
}
int genie_conv1x1_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, uint16_t* y, int n_pix, int Cin,
                       int Cout, void* stream) {
    GENIE_CHECK_ARG(x && w_packed && y && n_pix >= 0, "conv1x1: bad argument");
    return launch_gemm_bf16_out16(x, w_packed, bias, y, n_pix, Cout, Cin, as_stream(stream));
}
int genie_conv_direct_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, void* y, int n, int H, int W,
                           int Cin, int Cout, int out_mode, void* stream) {
    GENIE_CHECK_ARG(x && w_packed && y && n >= 0 && (out_mode == 0 || out_mode == 1), "conv_direct: bad argument");
    return launch_conv_direct(x, w_packed, bias, y, n, H, W, Cin, Cout, out_mode, as_stream(stream));
}
size_t genie_group_norm_scratch_floats(int n, int HW, int groups) {
    if (n <= 0 || HW <= 0 || groups <= 0) return 0;
    return gn_scratch_floats(n, HW, groups);
}
int genie_group_norm_swish_bf16(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* stats_ws, int n,
                                int HW, int C, int groups, float eps, int apply_swish, void* stream) {
    GENIE_CHECK_ARG(x && gamma && beta && y && stats_ws && n >= 0, "group_norm_swish: bad argument");
    if (n == 0) return GENIE_OK;
    return launch_gn_swish(x, gamma, beta, y, stats_ws, n, HW, C, groups, eps, apply_swish, as_stream(stream));
}
size_t genie_conv_gn_part_floats(int n, int H, int W, int Cout) {
    if (n <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
    return conv_gn_part_floats(n, H, W, Cout);
}
int genie_conv3x3_gn_bf16(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* residual, uint16_t* y,
                          const uint16_t* zero_page, int n, int H, int W, int Cin, int Cout, int depth_to_space, int stride,
                          float* gn_part, int groups, void* stream) {
    GENIE_CHECK_ARG(x && w_packed && y && zero_page && gn_part && n >= 0 && H >= 1 && W >= 1, "conv3x3_gn: bad argument");
    return launch_conv3x3_igemm(x, w_packed, bias, residual, y, zero_page, n, H, W, Cin, Cout, depth_to_space,
                                as_stream(stream), stride, gn_part, groups);
}
int genie_group_norm_swish_fused_bf16(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y,
                                      const float* gn_part, float* stats_ws, int n, int H, int W, int Cout, int depth_to_space,
                                      int groups, float eps, int apply_swish, void* stream) {
    GENIE_CHECK_ARG(x && gamma && beta && y && gn_part && stats_ws && n >= 0 && groups >= 1, "group_norm_swish_fused: bad argument");
    if (n == 0) return GENIE_OK;
    return launch_gn_swish_tiles(x, gamma, beta, y, gn_part, stats_ws, n, H, W, Cout, depth_to_space, groups, eps, apply_swish,
                                 as_stream(stream));
}
int genie_bits_from_tokens_nhwc_bf16(const int64_t* ids, uint16_t* z, int64_t n_pix, int bits, int cpad, void* stream) {
    GENIE_CHECK_ARG(ids && z && n_pix >= 0 && bits >= 1 && bits <= 62 && cpad >= bits, "bits_nhwc: bad argument");
    return launch_bits_nhwc(ids, z, (long)n_pix, bits, cpad, as_stream(stream));
}
int genie_rescale_u8_nhwc_bf16(const uint16_t* x, uint8_t* out, int n, int HW, int cpad, int cout, void* stream) {
    GENIE_CHECK_ARG(x && out && n >= 0 && HW >= 1 && cout >= 1 && cpad >= cout, "rescale_u8_nhwc: bad argument");
    return launch_rescale_nhwc_u8(x, out, n, HW, cpad, cout, as_stream(stream));
}

}  // extern "C"
