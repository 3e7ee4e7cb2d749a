// C ABI of libgenie_hip.so (include/genie_hip.h): argument checking, workspace carving and the
// launch sequences of decoder / MaskGIT / generate (the layer itself and the readout: st_block.hip).  All work is enqueued on the caller's
// stream; nothing here allocates, synchronises or touches the host-side of any tensor.
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
static Workspace carve(const genie_cfg& c, int B, void* base) {
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

static int check_cfg(const genie_cfg* c) {
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

static int check_ws(const genie_cfg& c, int B, void* ws, size_t bytes) {
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

static int decoder(const genie_cfg& c, const genie_weights& wt, float* x, Workspace& w, int B, hipStream_t st) {
    return run_layers(c, wt.layers_host, c.num_layers, x, w, B, st,
                      [&](int, const genie_layer_weights* next) { return BlockPass::plain(c, next, c.T); });
}

static int mask_count(int step, int steps, int S) {
    // n = ceil(cos(pi/2 * (step+1)/steps) * S), python float math (st_mask_git.py:17-26,199)
    double u = (double)(step + 1) / (double)steps;
    return (int)ceil(cos(u * M_PI / 2.0) * (double)S);
}

}  // namespace genie

using namespace genie;

// a genie_sampling law (NULL = none), checked on the host before anything is enqueued
static int check_sampling(const genie_sampling* sp, const char* where) {
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
static int check_unmask(int unmask_mode, bool ex, int steps, const float* noise, const char* where) {
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
static int check_guidance(const genie_guidance* g, const genie_frame_cond* cond, const char* where) {
    if (!g) return GENIE_OK;
    GENIE_CHECK_ARG(isfinite(g->scale), "%s: guidance: scale %g must be finite", where, (double)g->scale);
    GENIE_CHECK_ARG(cond && cond->n_actions > 0, "%s: guidance needs an action condition (cond with n_actions > 0)", where);
    GENIE_CHECK_ARG(g->null_action >= 0 && g->null_action < cond->n_actions, "%s: guidance: null_action %d outside [0, %d)", where,
                    (int)g->null_action, (int)cond->n_actions);
    return GENIE_OK;
}
// the confidence mode's scale when the caller gave no law: the documented default of choice_temperature
static const genie_sampling kDefaultSampling = {1.0f, 0, 1.0f, 4.5f};

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

// The split cache of a fan-out call (genie_generate_fanout): the B clips of a decode pass are K branches each of B / K parent clips.
// Slots [0, P0) live in `trunk`, a T-slot cache of B / K clips that the context pass filled and no decode pass writes; slot j >= P0 is
// slot j - P0 of the pass's own cache, (L, B, Tb, S, 3d).
struct FanOut {
    const float* trunk;
    int K, P0, Tb;
};
static size_t fanout_branch_bytes(const genie_cfg& c, size_t NBK, int Tb) {
    return (size_t)c.num_layers * NBK * Tb * c.S * 3 * c.d_model * sizeof(float);
}

// genie_frames_pass_cond, and with fan != NULL the decode pass of a fan-out call: `cache` is then the branch cache, and every such pass
// has t0 >= P0 -- nothing writes the trunk after the context pass
static int frames_pass(const genie_cfg* cfg, const genie_weights* wt, const int64_t* frame_ids, int B, int t0, int nf, float* cache,
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

// rows of S token ids: dst[b][0..S) = src[b][0..S) (clip strides in elements) or, src == NULL, the fill value; `copies` > 1 repeats the
// B rows at dst rows B .. 2B - 1, ... (the doubled batch of the guided loops)
__global__ void frame_ids_kernel(const int64_t* __restrict__ src, long src_stride, int64_t* __restrict__ dst, long dst_stride, int S, int B,
                                 int64_t fill, int copies) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)B * S;
    if (i >= per * copies) return;
    const long r = i / per, j = i - r * per;
    const long b = j / S, s = j - b * S;
    dst[(r * B + b) * dst_stride + s] = src ? src[b * src_stride + s] : fill;
}
static int put_frame_ids(const int64_t* src, long src_stride, int64_t* dst, long dst_stride, int S, int B, int64_t fill, hipStream_t st,
                         int copies = 1) {
    frame_ids_kernel<<<(unsigned)(((long)B * S * copies + 255) / 256), 256, 0, st>>>(src, src_stride, dst, dst_stride, S, B, fill, copies);
    GENIE_LAUNCH_CHECK("frame_ids");
    return GENIE_OK;
}
// the (2B, T) actions of a guided pass: the clips' own ids, then null_action at every frame
__global__ void guided_actions_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ out, long n, int64_t null_action) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * n) out[i] = i < n ? ids[i] : null_action;
}
static int put_guided_actions(const genie_frame_cond& cond, const genie_guidance& g, int B, int T, int64_t* out, hipStream_t st) {
    const long n = (long)B * T;
    guided_actions_kernel<<<(unsigned)((2 * n + 255) / 256), 256, 0, st>>>(cond.ids, out, n, g.null_action);
    GENIE_LAUNCH_CHECK("guided_actions");
    return GENIE_OK;
}

// where the loop scratch of genie_generate_cached starts: behind the workspace of its largest pass
static size_t generate_scratch_offset(const genie_cfg& c, int B, int P) {
    genie_cfg cm = c;
    cm.T = P > 2 ? P : 2;
    return carve(cm, B, nullptr).total;
}

// The loop scratch of genie_generate_cached_*: B clips are decoded, NB clips run through every pass (NB == B, or 2 B under guidance:
// [conditional ; null]).  The size functions and the loop both carve here (base == NULL: sizes only).
// A fan-out call (genie_generate_fanout) carves the same buffers: its context runs NBctx = NB / K clips, and it keeps their (NBctx, T)
// actions beside the branches' (NB, T).
struct GenScratch {
    int64_t *idsP, *two, *cur, *fin, *samples, *acts, *acts_ctx;
    float *conf, *logits;
    uint8_t* unmasked;
    size_t end;
};
// off: where the scratch starts; NBctx: clips of the context pass (idsP)
static GenScratch carve_loop(const genie_cfg& c, int B, int NB, int NBctx, int P, size_t off, char* base, bool acts) {
    const size_t BS = (size_t)B * c.S, NBS = (size_t)NB * c.S, V = (size_t)c.factored_vocab * c.num_factored;
    auto take = [&](size_t bytes) { char* r = base ? base + off : nullptr; off += align_up(bytes, 256); return r; };
    GenScratch g;
    g.idsP = (int64_t*)take((size_t)NBctx * c.S * P * 8);
    g.two = (int64_t*)take(NBS * 2 * 8);
    g.cur = (int64_t*)take(NBS * 8);
    g.fin = (int64_t*)take(NBS * 8);
    g.samples = (int64_t*)take(BS * 8);
    g.conf = (float*)take(BS * 4);
    g.unmasked = (uint8_t*)take(BS);
    g.logits = (float*)take(NBS * V * 4);
    g.acts = acts ? (int64_t*)take((size_t)NB * c.T * 8) : nullptr;
    g.acts_ctx = NBctx != NB ? (int64_t*)take((size_t)NBctx * c.T * 8) : nullptr;
    g.end = off;
    return g;
}
static GenScratch carve_generate(const genie_cfg& c, int B, int NB, int P, char* base, bool window_acts = false) {
    return carve_loop(c, B, NB, NB, P, generate_scratch_offset(c, NB, P), base, NB != B || window_acts);   // window_acts: the rollout's action window
}
// ... of genie_generate_fanout: B * K clips are decoded, NB * K run through every decode pass, NB through the context pass.  The scratch
// starts behind the larger of the context pass (NB clips, P frames) and a two-frame pass of NB * K clips.
static GenScratch carve_fanout(const genie_cfg& c, int B, int NB, int K, int P, char* base) {
    genie_cfg cm = c;
    cm.T = P;
    const size_t ctx = carve(cm, NB, nullptr).total;
    cm.T = 2;
    const size_t two = carve(cm, NB * K, nullptr).total;
    return carve_loop(c, B * K, NB * K, NB, P, ctx > two ? ctx : two, base, true);
}
// ... of genie_maskgit_generate_guided behind the model's workspace for 2 B clips: the doubled prompt and the (2B, T) actions
struct GuidedPrompt {
    int64_t *prompt2, *acts;
    size_t end;
};
static GuidedPrompt carve_guided_prompt(const genie_cfg& c, int NB, char* base) {
    size_t off = carve(c, NB, nullptr).total;
    auto take = [&](size_t bytes) { char* r = base ? base + off : nullptr; off += align_up(bytes, 256); return r; };
    GuidedPrompt g;
    g.prompt2 = (int64_t*)take((size_t)NB * c.T * c.S * 8);
    g.acts = (int64_t*)take((size_t)NB * c.T * 8);
    g.end = off;
    return g;
}

size_t genie_generate_workspace_bytes(const genie_cfg* cfg, int B, int P) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || P < 1 || P > cfg->T) return 0;
    const size_t off = carve_generate(*cfg, B, B, P, nullptr).end;
    const size_t full = carve(*cfg, B, nullptr).total;   // (the passes themselves check against the model's own workspace size)
    return off > full ? off : full;
}

size_t genie_generate_guided_workspace_bytes(const genie_cfg* cfg, int B, int P) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || B > 0x3fffffff || P < 1 || P > cfg->T) return 0;
    const size_t off = carve_generate(*cfg, B, 2 * B, P, nullptr).end;
    const size_t full = carve_guided_prompt(*cfg, 2 * B, nullptr).end;   // (>= the model's own workspace for 2 B clips)
    return off > full ? off : full;
}

int genie_generate_cached(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new, int steps,
                          float temperature, int unmask_mode, const float* noise, const float* uniforms, int teacher_force_time,
                          int merge_commit, int64_t* gen_out, float* logits0_out, float* cache, size_t cache_bytes, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return genie_generate_cached_cond(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time,
                                      merge_commit, gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream,
                                      nullptr);
}

int genie_generate_cached_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                               int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                               int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                               size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                               const genie_frame_cond* cond) {
    if (unmask_mode == GENIE_UNMASK_CONFIDENCE) unmask_mode = -1;   // (only genie_generate_cached_ex knows that mode)
    return genie_generate_cached_ex(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time,
                                    merge_commit, gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream, cond,
                                    nullptr);
}

// What one generate / rollout call decodes with: its checked arguments and the carved scratch, shared by every window of the call.
// B clips are decoded, NB run through every pass.
struct GenLoop {
    const genie_cfg* cfg;
    const genie_weights* wt;
    int B, NB, copies, steps, unmask_mode, merge_commit;
    float temperature;
    const genie_sampling* law;
    const genie_guidance* guidance;
    bool guided;
    const genie_frame_cond* cond;   // what the passes embed with: ids (NB, cfg->T)
    float* cache;
    size_t cache_bytes;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    GenScratch g;
    const FanOut* fan = nullptr;    // a fan-out call's decode passes: `cache` is the branch cache (the context ran into fan->trunk)
};
// the decode options every loop entry point takes, checked on the host before anything is enqueued
static int check_decode(int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                        const genie_sampling* sampling, const char* where) {
    GENIE_TRY(check_sampling(sampling, where));
    GENIE_TRY(check_unmask(unmask_mode, unmask_mode != -1, steps, noise, where));
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "%s: temperature > 0 needs uniforms", where);
    return GENIE_OK;
}

// `ctx` context frames into cache slots 0 .. ctx-1: one ctx-frame pass over idsP (NB, ctx, S, already filled) where the fragment-order
// kernels cover it, else the clean pass with the cache's T-frame layout, else frame by frame from src (frame t of clip b at
// src + b * src_stride + t * S)
static int run_context(const GenLoop& L, int ctx, const int64_t* src, long src_stride) {
    const genie_cfg& c = *L.cfg;
    hipStream_t st = as_stream(L.stream);
    int rc = GENIE_E_UNSUPPORTED;
    if (ctx > 1) {
        rc = genie_frames_pass_cond(L.cfg, L.wt, L.g.idsP, L.NB, 0, ctx, L.cache, L.cache_bytes, nullptr, L.workspace, L.workspace_bytes,
                                    L.stream, L.cond);
        if (rc == GENIE_E_UNSUPPORTED)
            rc = genie_clean_pass_cond(L.cfg, L.wt, L.g.idsP, L.NB, ctx, c.T, L.cache, L.cache_bytes, L.workspace, L.workspace_bytes,
                                       L.stream, L.cond);
    }
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    for (int t = 0; t < ctx; ++t) {
        GENIE_TRY(put_frame_ids(src + (size_t)t * c.S, src_stride, L.g.fin, c.S, c.S, L.B, 0, st, L.copies));
        GENIE_TRY(genie_frames_pass_cond(L.cfg, L.wt, L.g.fin, L.NB, t, 1, L.cache, L.cache_bytes, nullptr, L.workspace, L.workspace_bytes,
                                         L.stream, L.cond));
    }
    return GENIE_OK;
}

// The window body: decodes cache slots t0 .. t0 + n - 1 one after the other (slots < t0 - 1 are committed; slot t0 - 1 too unless `pend`).
// Slot t0 + k draws from noise / uniforms [k] and its final tokens go to out + k * S (clip stride out_stride); its step-0 logits to
// logits0_out[:, k] of (B, n, S, V) when wanted.  Every slot but the LAST is committed -- from its final tokens, or from tf + k * S (clip
// stride tf_stride) when tf is given (teacher forcing in time) --, merged with step 0 of the next slot where merge_commit is set and the
// library covers it.  pend != NULL: slot t0 - 1 is still pending; its final tokens (pend, clip stride pend_stride) are committed first, by
// the same rule.
static int decode_slots(const GenLoop& L, int t0, int n, const float* noise, const float* uniforms, int64_t* out, long out_stride,
                        float* logits0_out, const int64_t* tf, long tf_stride, const int64_t* pend, long pend_stride) {
    const genie_cfg* cfg = L.cfg;
    const genie_cfg& c = *cfg;
    const genie_weights* wt = L.wt;
    const int B = L.B, NB = L.NB, copies = L.copies, steps = L.steps, unmask_mode = L.unmask_mode, S = c.S;
    const float temperature = L.temperature;
    const bool guided = L.guided, by_conf = unmask_mode == GENIE_UNMASK_CONFIDENCE;
    const genie_frame_cond* cond = L.cond;
    float* cache = L.cache;
    const size_t cache_bytes = L.cache_bytes, workspace_bytes = L.workspace_bytes;
    void *workspace = L.workspace, *stream = L.stream;
    hipStream_t st = as_stream(stream);
    const size_t BS = (size_t)B * S, V = (size_t)c.factored_vocab * c.num_factored;
    int64_t *two = L.g.two, *cur = L.g.cur, *fin = L.g.fin, *samples = L.g.samples;
    float *conf = L.g.conf, *logits = L.g.logits;
    uint8_t* unmasked = L.g.unmasked;
    const float* logits_null = logits + BS * V;   // guided: rows B .. 2B - 1 of every pass's logits
    bool opened = false, merge = L.merge_commit != 0;
    auto pass = [&](const int64_t* frame_ids, int t, int nf, float* lg) {
        return frames_pass(cfg, wt, frame_ids, NB, t, nf, cache, cache_bytes, lg, workspace, workspace_bytes, stream, cond, L.fan);
    };
    // commit slot t from fsrc: in the pass that also carries MaskGIT step 0 of slot t + 1 (all-mask tokens), or on its own
    auto commit = [&](int t, const int64_t* fsrc, long fstride) -> int {
        if (merge) {
            GENIE_TRY(put_frame_ids(fsrc, fstride, two, 2L * S, S, B, 0, st, copies));
            GENIE_TRY(put_frame_ids(nullptr, 0, two + S, 2L * S, S, B, c.image_vocab_size, st, copies));
            const int rc = pass(two, t, 2, logits);
            if (rc == GENIE_E_UNSUPPORTED) merge = false;
            else { GENIE_TRY(rc); opened = true; }
        }
        if (!opened) {
            GENIE_TRY(put_frame_ids(fsrc, fstride, fin, S, S, B, 0, st, copies));
            GENIE_TRY(pass(fin, t, 1, nullptr));
        }
        return GENIE_OK;
    };
    if (pend) GENIE_TRY(commit(t0 - 1, pend, pend_stride));
    for (int k = 0; k < n; ++k) {
        const int t = t0 + k;
        GENIE_TRY(put_frame_ids(nullptr, 0, cur, S, S, B, c.image_vocab_size, st, copies));
        if (hipMemsetAsync(unmasked, 0, BS, st) != hipSuccess) { set_error("memset failed"); return GENIE_E_LAUNCH; }
        for (int step = 0; step < steps; ++step) {
            if (!(step == 0 && opened))
                GENIE_TRY(pass(cur, t, 1, logits));
            if (step == 0 && logits0_out) {   // orig_logits of the frame (st_mask_git.py:165,226): the step-0 logits, (B, n, S, V)
                if (guided) {                 // ... the guided ones
                    GENIE_TRY(launch_guide_logits(logits, logits_null, logits0_out + (size_t)k * S * V, B, (long)(S * V), (long)(S * V),
                                                  (long)((size_t)n * S * V), L.guidance->scale, st));
                } else if (hipMemcpy2DAsync(logits0_out + (size_t)k * S * V, (size_t)n * S * V * 4, logits, (size_t)S * V * 4,
                                            (size_t)S * V * 4, (size_t)B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                    set_error("memcpy failed");
                    return GENIE_E_LAUNCH;
                }
            }
            const float* u = temperature > 1e-8f ? uniforms + ((size_t)k * steps + step) * c.num_factored * BS : nullptr;
            const bool last = step == steps - 1;
            const float* draws = (last || unmask_mode == GENIE_UNMASK_GREEDY) ? nullptr : noise + ((size_t)k * (steps - 1) + step) * BS;
            // "confidence": the sample launch writes the keys over conf (nothing else reads conf in this loop)
            const float anneal = 1.0f - (float)(step + 1) / (float)steps;
            if (guided)
                GENIE_TRY(launch_sample_guided(c, logits, logits_null, GENIE_LAYOUT_TOKEN_MAJOR, B, temperature, u, samples, conf, L.law,
                                               (by_conf && !last) ? conf : nullptr, draws, anneal, L.guidance->scale, st));
            else
                GENIE_TRY(launch_sample_ex(c, logits, GENIE_LAYOUT_TOKEN_MAJOR, B, temperature, u, samples, conf, L.law,
                                           (by_conf && !last) ? conf : nullptr, draws, anneal, st));
            const float* keys = last ? nullptr : (unmask_mode == GENIE_UNMASK_RANDOM ? draws : conf);
            GENIE_TRY(launch_mask_step(keys, last ? 0 : mask_count(step, steps, S), last, c.image_vocab_size, unmasked, samples, cur, S, B, S, st));
            if (guided) GENIE_TRY(put_frame_ids(cur, S, cur + BS, S, S, B, 0, st));   // the null half sees the same tokens
        }
        GENIE_TRY(put_frame_ids(cur, S, out + (size_t)k * S, out_stride, S, B, 0, st));
        opened = false;
        if (k + 1 < n) {   // commit slot t: its final tokens, or the ground truth when teacher-forcing in time
            if (tf) GENIE_TRY(commit(t, tf + (size_t)k * S, tf_stride));
            else GENIE_TRY(commit(t, cur, S));
        }
    }
    return GENIE_OK;
}

// genie_generate_cached_ex (guidance NULL or of scale 1) and genie_generate_cached_guided: one loop, B clips decoded, NB per pass
static int generate_cached_loop(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                                int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && gen_out && cache, "generate_cached: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "generate_cached"));
    GENIE_TRY(check_guidance(guidance, cond, "generate_cached"));
    GENIE_CHECK_ARG(B >= 1 && P >= 1 && n_new >= 1 && P + n_new <= c.T && steps >= 1,
                    "generate_cached: B=%d, %d prompt + %d new frames of at most %d, steps %d", B, P, n_new, c.T, steps);
    GENIE_TRY(check_decode(steps, temperature, unmask_mode, noise, uniforms, sampling, "generate_cached"));
    const bool by_conf = unmask_mode == GENIE_UNMASK_CONFIDENCE;
    // under guidance every pass runs 2 B clips, [conditional ; null]: rows b and b + B hold the same tokens, the second half's actions are
    // null_action at every frame; B rows are sampled, masked and written out
    const bool guided = guidance && guidance->scale != 1.0f;
    GENIE_CHECK_ARG(!guided || B <= 0x3fffffff, "generate_cached: B=%d too large for guidance", B);
    const int NB = guided ? 2 * B : B, copies = guided ? 2 : 1;
    GENIE_CHECK_ARG(cache_bytes >= genie_prefix_cache_bytes(cfg, NB), "generate_cached: cache too small");
    GENIE_TRY(check_ws(c, NB, workspace, workspace_bytes));
    hipStream_t st = as_stream(stream);
    const int S = c.S, T = P + n_new;   // frames per clip in `ids` (the cache keeps the model's c.T slots per clip)
    // scratch of the loop behind the workspace of its largest pass (the prompt's P frames; two frames for the merged passes):
    // genie_generate_workspace_bytes / genie_generate_guided_workspace_bytes (cfg, B, P) is the size to allocate
    GenLoop L = {cfg, wt, B, NB, copies, steps, unmask_mode, merge_commit, temperature, (by_conf && !sampling) ? &kDefaultSampling : sampling,
                 guidance, guided, cond, cache, cache_bytes, workspace, workspace_bytes, stream, carve_generate(c, B, NB, P, (char*)workspace)};
    GENIE_CHECK_ARG(L.g.end <= workspace_bytes, "generate_cached: workspace too small (%zu < %zu bytes: size it with %s)", workspace_bytes,
                    L.g.end, guided ? "genie_generate_guided_workspace_bytes" : "genie_generate_workspace_bytes");
    genie_frame_cond cond2;
    if (guided) {
        GENIE_TRY(put_guided_actions(*cond, *guidance, B, c.T, L.g.acts, st));
        cond2 = *cond;
        cond2.ids = L.g.acts;
        L.cond = &cond2;
    }
    // ---- the prompt fills cache slots 0 .. P-1
    for (int t = 0; t < P; ++t)
        GENIE_TRY(put_frame_ids(ids + (size_t)t * S, (long)T * S, L.g.idsP + (size_t)t * S, (long)P * S, S, B, 0, st, copies));
    GENIE_TRY(run_context(L, P, ids, (long)T * S));
    return decode_slots(L, P, n_new, noise, uniforms, gen_out, (long)n_new * S, logits0_out,
                        teacher_force_time ? ids + (size_t)P * S : nullptr, (long)T * S, nullptr, 0);
}

// What the passes of one rollout window read, gathered from the caller's (B, cap, *) buffers in one launch:
//   ctx_out (B * copies, ctx, S): the tokens of absolute frames [start, start + ctx); rows b + B (copies == 2) repeat rows b
//   act_out (B * copies, T) or NULL: slot i = the action of absolute frame start + i, 0 past cap (never embedded); rows b + B = null_action
__global__ void rollout_window_kernel(const int64_t* __restrict__ frames, const int64_t* __restrict__ actions, int64_t* __restrict__ ctx_out,
                                      int64_t* __restrict__ act_out, int B, int copies, int ctx, int S, int T, long cap, long start,
                                      int64_t null_action) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)ctx * S, ntok = (long)B * copies * per;
    if (i < ntok) {
        const long r = i / per, j = i - r * per, b = r % B;
        ctx_out[i] = frames[(b * cap + start) * S + j];
        return;
    }
    const long a = i - ntok;
    if (!act_out || a >= (long)B * copies * T) return;
    const long r = a / T, f = start + (a - r * T);
    act_out[a] = r >= B ? null_action : (f < cap ? actions[r * cap + f] : 0);
}
static int put_rollout_window(const int64_t* frames, const int64_t* actions, int64_t* ctx_out, int64_t* act_out, int B, int copies,
                              int ctx, int S, int T, long cap, long start, int64_t null_action, hipStream_t st) {
    const long n = (long)B * copies * ((long)ctx * S + (act_out ? T : 0));
    if (n == 0) return GENIE_OK;
    rollout_window_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(frames, actions, ctx_out, act_out, B, copies, ctx, S, T, cap, start,
                                                                       null_action);
    GENIE_LAUNCH_CHECK("rollout_window");
    return GENIE_OK;
}

size_t genie_rollout_workspace_bytes(const genie_cfg* cfg, int B, int ctx_max, int guided) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || B > 0x3fffffff || ctx_max < 1 || ctx_max > cfg->T - 1) return 0;
    const int NB = guided ? 2 * B : B;
    const size_t off = carve_generate(*cfg, B, NB, ctx_max, nullptr, true).end;
    const size_t full = guided ? carve_guided_prompt(*cfg, NB, nullptr).end : carve(*cfg, B, nullptr).total;
    return off > full ? off : full;
}

int genie_rollout_cached(const genie_cfg* cfg, const genie_weights* wt, int64_t* frames, int B, int P, int keep, int cap, int f0, int f1,
                         int resume, int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                         int merge_commit, float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                         const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    const int T = c.T, S = c.S;
    GENIE_CHECK_ARG(B >= 1 && steps >= 1, "rollout_cached: B=%d, steps %d", B, steps);
    GENIE_CHECK_ARG(P >= 1 && P <= T - 1, "rollout_cached: %d prompt frames outside [1, %d]", P, T - 1);
    GENIE_CHECK_ARG(keep >= 1 && keep <= T - 1, "rollout_cached: keep %d outside [1, %d]", keep, T - 1);
    GENIE_CHECK_ARG(P <= f0 && f0 < f1 && f1 <= cap, "rollout_cached: frames [%d, %d) must lie in [%d prompt frames, cap %d]", f0, f1, P, cap);
    GENIE_CHECK_ARG(resume == 0 || resume == 1, "rollout_cached: resume %d must be 0 or 1", resume);
    GENIE_TRY(check_frame_cond(cond, "rollout_cached"));
    GENIE_TRY(check_guidance(guidance, cond, "rollout_cached"));
    GENIE_TRY(check_decode(steps, temperature, unmask_mode, noise, uniforms, sampling, "rollout_cached"));
    GENIE_CHECK_ARG(wt && wt->layers_host && frames && cache, "rollout_cached: NULL pointer");
    const bool by_conf = unmask_mode == GENIE_UNMASK_CONFIDENCE, guided = guidance && guidance->scale != 1.0f;
    GENIE_CHECK_ARG(!guided || B <= 0x3fffffff, "rollout_cached: B=%d too large for guidance", B);
    const int NB = guided ? 2 * B : B, copies = guided ? 2 : 1, hop = T - keep;
    GENIE_CHECK_ARG(cache_bytes >= genie_prefix_cache_bytes(cfg, NB), "rollout_cached: cache too small");
    GENIE_TRY(check_ws(c, NB, workspace, workspace_bytes));
    // window of frame f: j = 0 below T, else 1 + (f - T) / hop; it starts at absolute frame j * hop and ends before j * hop + T
    auto start_of = [&](int f) { return f < T ? 0 : (1 + (f - T) / hop) * hop; };
    auto opens = [&](int f) { return f == P || (f >= T && f - start_of(f) == keep); };
    const int start0 = start_of(f0);
    const bool fresh0 = !resume || opens(f0);
    // the largest context this call runs sizes its scratch: that of f0 unless resumed mid-window, `keep` for every later window
    int ctx_need = fresh0 ? f0 - start0 : 1;
    if (f1 > start0 + T && keep > ctx_need) ctx_need = keep;
    GenLoop L = {cfg, wt, B, NB, copies, steps, unmask_mode, merge_commit, temperature, (by_conf && !sampling) ? &kDefaultSampling : sampling,
                 guidance, guided, cond, cache, cache_bytes, workspace, workspace_bytes, stream,
                 carve_generate(c, B, NB, ctx_need, (char*)workspace, true)};
    GENIE_CHECK_ARG(L.g.end <= workspace_bytes, "rollout_cached: workspace too small (%zu < %zu bytes: size it with "
                    "genie_rollout_workspace_bytes for a context of %d frames)", workspace_bytes, L.g.end, ctx_need);
    hipStream_t st = as_stream(stream);
    const bool acts = cond && cond->n_actions > 0;
    genie_frame_cond cond2;
    if (acts) {   // the passes read the window's actions, (NB, T) with the clip stride they expect
        cond2 = *cond;
        cond2.ids = L.g.acts;
        L.cond = &cond2;
    }
    const long stride = (long)cap * S;
    for (int f = f0; f < f1;) {
        const int start = start_of(f), end = start + T < f1 ? start + T : f1;
        const bool fresh = f != f0 || fresh0;   // the window's context is run from `frames`; else frame f - 1 is pending in the cache
        const int ctx = fresh ? f - start : 0;
        GENIE_TRY(put_rollout_window(frames, acts ? cond->ids : nullptr, L.g.idsP, acts ? L.g.acts : nullptr, B, copies, ctx, S, T, cap, start,
                                     guided ? guidance->null_action : 0, st));
        if (fresh) GENIE_TRY(run_context(L, ctx, frames + (size_t)start * S, stride));
        GENIE_TRY(decode_slots(L, f - start, end - f, noise ? noise + (size_t)(f - f0) * (steps - 1) * B * S : nullptr,
                               uniforms ? uniforms + (size_t)(f - f0) * steps * c.num_factored * B * S : nullptr, frames + (size_t)f * S,
                               stride, nullptr, nullptr, 0, fresh ? nullptr : frames + (size_t)(f - 1) * S, stride));
        f = end;
    }
    return GENIE_OK;
}

int genie_generate_cached_ex(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                             int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                             int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                             size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                             const genie_frame_cond* cond, const genie_sampling* sampling) {
    return generate_cached_loop(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time, merge_commit,
                                gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream, cond, sampling, nullptr);
}

int genie_generate_cached_guided(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                                 int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                 size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                 const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    return generate_cached_loop(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time, merge_commit,
                                gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream, cond, sampling, guidance);
}

// ---- fan-out generation: K futures per clip over one shared context cache ------------------------------------------------
// The (NB, T) actions of the context pass and the (NB * K, T) actions of the decode passes from the caller's (B * K, T) ids, null halves
// included: parent b reads its context actions from its branch 0 (row b * K; frames < P of the other branches are never read).
__global__ void fanout_actions_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ ctx_out, int64_t* __restrict__ br_out, int B, int K,
                                      int NB, int T, int P, int64_t null_action) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nctx = (long)NB * T, BK = (long)B * K;
    if (i < nctx) {
        const long r = i / T, f = i - r * T;
        ctx_out[i] = r >= B ? null_action : ids[r * K * T + f];
        return;
    }
    const long a = i - nctx;
    if (a >= nctx * K) return;
    const long r = a / T, f = a - r * T;
    br_out[a] = r >= BK ? null_action : ids[(f < P ? r / K * K : r) * T + f];
}

// NB * K as an int the passes can take, or 0
static int fanout_clips(int B, int K, bool guided) {
    if (B < 1 || K < 1) return 0;
    const long n = (long)B * K * (guided ? 2 : 1);
    return n <= 0x3fffffff ? (int)n : 0;
}

size_t genie_fanout_branch_bytes(const genie_cfg* cfg, int NB, int K, int n_new) {
    if (check_cfg(cfg) != GENIE_OK || !fanout_clips(NB, K, false) || n_new < 1 || n_new > cfg->T - 1) return 0;
    return fanout_branch_bytes(*cfg, (size_t)NB * K, n_new);
}

size_t genie_fanout_workspace_bytes(const genie_cfg* cfg, int B, int K, int P, int guided) {
    if (check_cfg(cfg) != GENIE_OK || !fanout_clips(B, K, guided != 0) || P < 1 || P > cfg->T - 1) return 0;
    const int NB = guided ? 2 * B : B;
    const size_t off = carve_fanout(*cfg, B, NB, K, P, nullptr).end;
    const size_t full = carve(*cfg, NB, nullptr).total;   // (the context passes check against the model's own workspace size)
    return off > full ? off : full;
}

int genie_generate_fanout(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int K, int P, int n_new, int steps,
                          float temperature, int unmask_mode, const float* noise, const float* uniforms, int merge_commit, int64_t* gen_out,
                          float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_TRY(check_frame_cond(cond, "generate_fanout"));
    GENIE_TRY(check_guidance(guidance, cond, "generate_fanout"));
    GENIE_CHECK_ARG(B >= 1 && K >= 1 && P >= 1 && n_new >= 1 && P + n_new <= c.T && steps >= 1,
                    "generate_fanout: B=%d, K=%d, %d prompt + %d new frames of at most %d, steps %d", B, K, P, n_new, c.T, steps);
    GENIE_TRY(check_decode(steps, temperature, unmask_mode, noise, uniforms, sampling, "generate_fanout"));
    const bool by_conf = unmask_mode == GENIE_UNMASK_CONFIDENCE, guided = guidance && guidance->scale != 1.0f;
    const int NBK = fanout_clips(B, K, guided);
    GENIE_CHECK_ARG(NBK > 0, "generate_fanout: B=%d x K=%d%s clips per pass are too many", B, K, guided ? " x 2" : "");
    const int NB = guided ? 2 * B : B, copies = guided ? 2 : 1, BK = B * K;
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && gen_out && trunk && branch && workspace, "generate_fanout: NULL pointer");
    GENIE_CHECK_ARG(trunk_bytes >= genie_prefix_cache_bytes(cfg, NB), "generate_fanout: trunk cache too small (genie_prefix_cache_bytes of %d clips)", NB);
    GENIE_CHECK_ARG(branch_bytes >= fanout_branch_bytes(c, (size_t)NBK, n_new), "generate_fanout: branch cache too small (genie_fanout_branch_bytes)");
    const GenScratch g = carve_fanout(c, B, NB, K, P, (char*)workspace);
    const size_t full = carve(c, NB, nullptr).total;
    GENIE_CHECK_ARG(workspace_bytes >= g.end && workspace_bytes >= full, "generate_fanout: workspace too small (%zu < %zu bytes: size it with "
                    "genie_fanout_workspace_bytes)", workspace_bytes, g.end > full ? g.end : full);
    hipStream_t st = as_stream(stream);
    const int S = c.S;
    const genie_sampling* law = (by_conf && !sampling) ? &kDefaultSampling : sampling;
    // the context of the NB clips runs once, into the trunk; its actions and the branches' come from one launch
    genie_frame_cond cond_ctx, cond_br;
    const bool acts = cond && cond->n_actions > 0;
    if (acts) {
        const long n = (long)NB * c.T * (1 + K);
        fanout_actions_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(cond->ids, g.acts_ctx ? g.acts_ctx : g.acts, g.acts, B, K, NB, c.T, P,
                                                                           guided ? guidance->null_action : 0);
        GENIE_LAUNCH_CHECK("fanout_actions");
        cond_ctx = cond_br = *cond;
        cond_ctx.ids = g.acts_ctx ? g.acts_ctx : g.acts;   // (K == 1: one table serves both)
        cond_br.ids = g.acts;
    }
    GenLoop Lc = {cfg, wt, B, NB, copies, steps, unmask_mode, merge_commit, temperature, law, guidance, guided, acts ? &cond_ctx : cond,
                  trunk, trunk_bytes, workspace, workspace_bytes, stream, g};
    GENIE_TRY(put_frame_ids(ids, (long)P * S, g.idsP, (long)P * S, P * S, B, 0, st, copies));
    GENIE_TRY(run_context(Lc, P, ids, (long)P * S));
    // ... then the loop of genie_generate_cached decodes B * K clips over the split cache, starting at slot P with nothing pending
    const FanOut fan = {trunk, K, P, n_new};
    const GenLoop Lb = {cfg, wt, BK, NBK, copies, steps, unmask_mode, merge_commit, temperature, law, guidance, guided, acts ? &cond_br : cond,
                        branch, branch_bytes, workspace, workspace_bytes, stream, g, &fan};
    return decode_slots(Lb, P, n_new, noise, uniforms, gen_out, (long)n_new * S, nullptr, nullptr, 0, nullptr, 0);
}

// ---- scoring observed futures: per-(clip, branch, frame) NLL over the fan-out cache ----------------------------------------
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

size_t genie_score_workspace_bytes(const genie_cfg* cfg, int B, int K, int P) { return genie_fanout_workspace_bytes(cfg, B, K, P, 0); }

// rows of S token ids for the B * K clips of a fan-out pass from their B parents: dst[i][0..S) = src[i / K][0..S) (strides in elements)
__global__ void branch_frame_ids_kernel(const int64_t* __restrict__ src, long src_stride, int64_t* __restrict__ dst, long dst_stride, int S,
                                        long BK, int K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK * S) return;
    const long r = i / S, s = i - r * S;
    dst[r * dst_stride + s] = src[(r / K) * src_stride + s];
}

// decode_slots' sibling for OBSERVED frames: per slot t0 + j the all-mask pass (riding the commit of slot t0 + j - 1 by decode_slots' own
// rule), launch_score_rows on its logits against frame j of obs (parent clip i / K of row i, clip stride obs_stride), then the commit of
// the observed tokens; the last slot is not committed.  nll / hits (L.B, n), token_nll (L.B, n, S).  No sample or mask-step launches,
// no draws, no host synchronisation.
static int score_slots(const GenLoop& L, int t0, int n, const int64_t* obs, long obs_stride, int K, double* nll, double* hits,
                       float* token_nll) {
    const genie_cfg& c = *L.cfg;
    const int BK = L.B, S = c.S;
    hipStream_t st = as_stream(L.stream);
    int64_t *two = L.g.two, *cur = L.g.cur, *fin = L.g.fin;
    float* logits = L.g.logits;
    bool opened = false, merge = L.merge_commit != 0;
    auto pass = [&](const int64_t* frame_ids, int t, int nf, float* lg) {
        return frames_pass(L.cfg, L.wt, frame_ids, L.NB, t, nf, L.cache, L.cache_bytes, lg, L.workspace, L.workspace_bytes, L.stream, L.cond,
                           L.fan);
    };
    auto put_observed = [&](const int64_t* src, int64_t* dst, long dst_stride) {
        branch_frame_ids_kernel<<<(unsigned)(((long)BK * S + 255) / 256), 256, 0, st>>>(src, obs_stride, dst, dst_stride, S, (long)BK, K);
        GENIE_LAUNCH_CHECK("branch_frame_ids");
        return GENIE_OK;
    };
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        if (!opened) {
            GENIE_TRY(put_frame_ids(nullptr, 0, cur, S, S, BK, c.image_vocab_size, st));
            GENIE_TRY(pass(cur, t, 1, logits));
        }
        GENIE_TRY(launch_score_rows(c, logits, obs + (size_t)j * S, obs_stride, K, BK, nll + j, n, hits ? hits + j : nullptr,
                                    token_nll ? token_nll + (size_t)j * S : nullptr, (long)n * S, st));
        opened = false;
        if (j + 1 == n) break;
        if (merge) {   // commit slot t in the pass that also carries the all-mask slot t + 1
            GENIE_TRY(put_observed(obs + (size_t)j * S, two, 2L * S));
            GENIE_TRY(put_frame_ids(nullptr, 0, two + S, 2L * S, S, BK, c.image_vocab_size, st));
            const int rc = pass(two, t, 2, logits);
            if (rc == GENIE_E_UNSUPPORTED) merge = false;
            else { GENIE_TRY(rc); opened = true; }
        }
        if (!opened) {
            GENIE_TRY(put_observed(obs + (size_t)j * S, fin, S));
            GENIE_TRY(pass(fin, t, 1, nullptr));
        }
    }
    return GENIE_OK;
}

int genie_score_fanout(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int K, int P, int n, int merge_commit,
                       double* nll, double* hits, float* token_nll, float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes,
                       void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_TRY(check_frame_cond(cond, "score_fanout"));
    GENIE_CHECK_ARG(B >= 1 && K >= 1 && P >= 1 && n >= 1 && P + n <= c.T, "score_fanout: B=%d, K=%d, %d prompt + %d scored frames of at most %d",
                    B, K, P, n, c.T);
    const int BK = fanout_clips(B, K, false);
    GENIE_CHECK_ARG(BK > 0, "score_fanout: B=%d x K=%d clips per pass are too many", B, K);
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && nll && trunk && branch && workspace, "score_fanout: NULL pointer");
    GENIE_CHECK_ARG(trunk_bytes >= genie_prefix_cache_bytes(cfg, B), "score_fanout: trunk cache too small (genie_prefix_cache_bytes of %d clips)", B);
    GENIE_CHECK_ARG(branch_bytes >= fanout_branch_bytes(c, (size_t)BK, n), "score_fanout: branch cache too small (genie_fanout_branch_bytes)");
    const GenScratch g = carve_fanout(c, B, B, K, P, (char*)workspace);
    const size_t full = carve(c, B, nullptr).total;
    GENIE_CHECK_ARG(workspace_bytes >= g.end && workspace_bytes >= full, "score_fanout: workspace too small (%zu < %zu bytes: size it with "
                    "genie_score_workspace_bytes)", workspace_bytes, g.end > full ? g.end : full);
    hipStream_t st = as_stream(stream);
    const int S = c.S;
    const long clip = (long)(P + n) * S;   // ids (B, P + n, S)
    genie_frame_cond cond_ctx, cond_br;
    const bool acts = cond && cond->n_actions > 0;
    if (acts) {
        const long na = (long)B * c.T * (1 + K);
        fanout_actions_kernel<<<(unsigned)((na + 255) / 256), 256, 0, st>>>(cond->ids, g.acts_ctx ? g.acts_ctx : g.acts, g.acts, B, K, B, c.T, P, 0);
        GENIE_LAUNCH_CHECK("fanout_actions");
        cond_ctx = cond_br = *cond;
        cond_ctx.ids = g.acts_ctx ? g.acts_ctx : g.acts;
        cond_br.ids = g.acts;
    }
    // the context of the B clips runs once, into the trunk, as in genie_generate_fanout
    GenLoop Lc = {cfg, wt, B, B, 1, 1, GENIE_UNMASK_GREEDY, merge_commit, 0.0f, nullptr, nullptr, false, acts ? &cond_ctx : cond,
                  trunk, trunk_bytes, workspace, workspace_bytes, stream, g};
    GENIE_TRY(put_frame_ids(ids, clip, g.idsP, (long)P * S, P * S, B, 0, st));
    GENIE_TRY(run_context(Lc, P, ids, clip));
    const FanOut fan = {trunk, K, P, n};
    const GenLoop Lb = {cfg, wt, BK, BK, 1, 1, GENIE_UNMASK_GREEDY, merge_commit, 0.0f, nullptr, nullptr, false, acts ? &cond_br : cond,
                        branch, branch_bytes, workspace, workspace_bytes, stream, g, &fan};
    return score_slots(Lb, P, n, ids + (size_t)P * S, clip, K, nll, hits, token_nll);
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
    return launch_attn_temporal_single_fanout(branch_slice, out, NBK, Tb, c.S, t, c.d_model, c.num_heads, c.head_dim, c.attn_scale,
                                              c.qk_norm ? aw->norm_w : nullptr, c.qk_norm ? aw->norm_b : nullptr, as_stream(stream), nullptr, 0,
                                              in16 != 0, FanSplit<true>{trunk_slice ? trunk_slice : branch_slice, c.T, P0, K});
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

int genie_maskgit_generate(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                           float temperature, int unmask_mode, const float* noise, const float* uniforms,
                           int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return genie_maskgit_generate_cond(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out,
                                       logits0_out, layout, status_flag, workspace, workspace_bytes, stream, nullptr);
}

int genie_maskgit_generate_cond(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                                float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond) {
    if (unmask_mode == GENIE_UNMASK_CONFIDENCE) unmask_mode = -1;   // (only genie_maskgit_generate_ex knows that mode)
    return genie_maskgit_generate_ex(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out,
                                     logits0_out, layout, status_flag, workspace, workspace_bytes, stream, cond, nullptr);
}

// genie_maskgit_generate_ex (guidance NULL or of scale 1) and genie_maskgit_generate_guided: one loop, B clips decoded, NB per forward
static int maskgit_generate_loop(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                                 float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                 void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                 const genie_sampling* sampling, const genie_guidance* guidance) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_CHECK_ARG(wt && wt->layers_host && prompt && samples_out, "maskgit_generate: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "maskgit_generate"));
    GENIE_TRY(check_guidance(guidance, cond, "maskgit_generate"));
    if (!(out_t >= 1 && out_t < c.T)) {  // assert out_t  (st_mask_git.py:154)
        set_error("maskgit_generate requires 0 < out_t < T (got %d)", out_t);
        return GENIE_E_ASSERT;
    }
    GENIE_CHECK_ARG(steps >= 1, "maskgit_generate: steps=%d must be >= 1", steps);
    GENIE_TRY(check_sampling(sampling, "maskgit_generate"));
    GENIE_TRY(check_unmask(unmask_mode, unmask_mode != -1, steps, noise, "maskgit_generate"));
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "maskgit_generate: temperature > 0 needs uniforms");
    const bool by_conf = unmask_mode == GENIE_UNMASK_CONFIDENCE;
    const genie_sampling* law = (by_conf && !sampling) ? &kDefaultSampling : sampling;
    // under guidance every forward runs 2 B clips, [conditional ; null], on a doubled copy of the prompt behind the workspace
    const bool guided = guidance && guidance->scale != 1.0f;
    GENIE_CHECK_ARG(!guided || B <= 0x3fffffff, "maskgit_generate: B=%d too large for guidance", B);
    const int NB = guided ? 2 * B : B;
    GENIE_TRY(check_ws(c, NB, workspace, workspace_bytes));
    Workspace w = carve(c, NB, workspace);
    hipStream_t st = as_stream(stream);
    const size_t BS = (size_t)B * c.S;
    const long V = (long)c.factored_vocab * c.num_factored;
    const long clip = (long)c.T * c.S;
    const int64_t* tokens = prompt;   // what every forward embeds
    genie_frame_cond cond2;
    if (guided) {
        const GuidedPrompt gp = carve_guided_prompt(c, NB, (char*)workspace);
        GENIE_CHECK_ARG(gp.end <= workspace_bytes, "maskgit_generate: workspace too small (%zu < %zu bytes: size it with "
                        "genie_generate_guided_workspace_bytes)", workspace_bytes, gp.end);
        GENIE_TRY(put_guided_actions(*cond, *guidance, B, c.T, gp.acts, st));
        cond2 = *cond;
        cond2.ids = gp.acts;
        cond = &cond2;
        GENIE_TRY(put_frame_ids(prompt, clip, gp.prompt2, clip, (int)clip, B, 0, st, 2));
        tokens = gp.prompt2;
    }
    // guided: the null half of the frame's logits, and room behind both halves for the guided step-0 logits (w.logits holds T >= 2 frames)
    const float* logits_null = w.logits + BS * V;
    float* logits_g = w.logits + 2 * BS * V;

    GENIE_TRY(launch_check_masked(prompt, B, c.T, c.S, out_t, c.image_vocab_size, status_flag, st));
    if (hipMemsetAsync(w.unmasked, 0, BS, st) != hipSuccess) { set_error("memset failed"); return GENIE_E_LAUNCH; }
    EmbedAct act;
    const EmbedAct* pact = frame_act(cond, c.S, 0, c.T, act);
    for (int step = 0; step < steps; ++step) {
        GENIE_TRY(launch_embed(c, *wt, tokens, NB, w.x, st, pact));
        GENIE_TRY(decoder(c, *wt, w.x, w, NB, st));
        GENIE_TRY(readout(c, *wt, w.x, w, NB, out_t, out_t + 1, GENIE_LAYOUT_TOKEN_MAJOR, w.logits, st));
        if (step == 0 && logits0_out) {  // orig_logits_CHW: step-0 logits are what is returned (:165,226); the guided ones under guidance
            const bool tm = layout == GENIE_LAYOUT_TOKEN_MAJOR;
            if (guided) GENIE_TRY(launch_guide_logits(w.logits, logits_null, tm ? logits0_out : logits_g, 1, (long)(BS * V), 0, 0, guidance->scale, st));
            if (tm) {
                if (!guided && hipMemcpyAsync(logits0_out, w.logits, BS * V * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                    set_error("memcpy failed");
                    return GENIE_E_LAUNCH;
                }
            } else {
                GENIE_TRY(launch_transpose(guided ? logits_g : w.logits, logits0_out, B, c.S, (int)V, st));
            }
        }
        const float* u = (temperature > 1e-8f) ? uniforms + (size_t)step * c.num_factored * BS : nullptr;
        const int last = (step == steps - 1);
        const float* draws = (last || unmask_mode == GENIE_UNMASK_GREEDY) ? nullptr : noise + (size_t)step * BS;
        // "confidence": the sample launch writes the keys over conf (nothing else reads conf in this loop)
        const float anneal = 1.0f - (float)(step + 1) / (float)steps;
        if (guided)
            GENIE_TRY(launch_sample_guided(c, w.logits, logits_null, GENIE_LAYOUT_TOKEN_MAJOR, B, temperature, u, w.samples, w.conf, law,
                                           (by_conf && !last) ? w.conf : nullptr, draws, anneal, guidance->scale, st));
        else
            GENIE_TRY(launch_sample_ex(c, w.logits, GENIE_LAYOUT_TOKEN_MAJOR, B, temperature, u, w.samples, w.conf, law,
                                       (by_conf && !last) ? w.conf : nullptr, draws, anneal, st));
        const float* keys = nullptr;
        int n = 0;
        if (!last) {
            n = mask_count(step, steps, c.S);
            keys = (unmask_mode == GENIE_UNMASK_RANDOM) ? draws : w.conf;
        }
        GENIE_TRY(launch_mask_step(keys, n, last, c.image_vocab_size, w.unmasked, w.samples,
                                   prompt + (size_t)out_t * c.S, clip, B, c.S, st));
        if (guided && !last)   // both halves of the next forward see the frame's current tokens
            GENIE_TRY(put_frame_ids(prompt + (size_t)out_t * c.S, clip, const_cast<int64_t*>(tokens) + (size_t)out_t * c.S, clip, c.S, B, 0, st, 2));
    }
    if (hipMemcpyAsync(samples_out, w.samples, BS * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("memcpy failed");
        return GENIE_E_LAUNCH;
    }
    return GENIE_OK;
}

int genie_maskgit_generate_ex(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                              float temperature, int unmask_mode, const float* noise, const float* uniforms,
                              int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                              void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                              const genie_sampling* sampling) {
    return maskgit_generate_loop(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out, logits0_out, layout,
                                 status_flag, workspace, workspace_bytes, stream, cond, sampling, nullptr);
}

int genie_maskgit_generate_guided(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                                  float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                  int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                  void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                  const genie_sampling* sampling, const genie_guidance* guidance) {
    return maskgit_generate_loop(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out, logits0_out, layout,
                                 status_flag, workspace, workspace_bytes, stream, cond, sampling, guidance);
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
