// C ABI of the training step (include/genie_hip.h, "training" section): forward with saved activations, masked
// factored CE, backward layer by layer (so the caller can overlap the gradient all-reduce of finished layers with
// the backward of earlier ones), AdamW.
//
// The STBlock is stated once for the forward (layer_forward: train_forward's loop and the recomputation in front of a layer's
// backward, which say where the layer's activations live with a LayerAt) and once for the backward (train_backward_layer), as templates over
// a backend that says how a Linear product runs and in which form its operands are saved:
//   ExactOps (GENIE_PREC_EXACT): f32 storage, every contraction on the f32 matrix instruction (launch_gemm_f32_gen);
//   Ops16 (GENIE_PREC_BF16 / _F16X3): every Linear product -- forward, dgrad, wgrad -- on the NT 16-bit GEMM of kernels_bf16.hip
//     (bf16 weight gradients on the TN kernel where the shapes allow) from 16-bit operand copies: bf16, or two f16 planes [hi | lo].
// LayerNorm, softmax, both attention cores (forward and backward; bf16: the spatial backward's products on the bf16 matrix cores,
// kernels_attn_bwd16.hip), GELU, the residual stream, CE and all gradient reductions are f32 in both.
//
// HBM layout of the saved activations (train_acts; M = B*T*S tokens, token-major rows).  Per layer l at l*per_layer, f32 unless
// marked [op] = saved in operand form (exact: f32; 16-bit: NPL planes of 16 bits, and every slot rounded up to 256 bytes):
//   x0 (M,d) layer input | u1 [op] (M,d) norm1(x0) | qkv_s (M,3d) | ao_s [op] (M,d) spatial attention output before proj | x1 (M,d)
//   | x1h [op] (M,d) x1 again (16-bit only; exact reads x1) | qkv_t (M,3d) | ao_t [op] (M,d) | x2 (M,d) | u2 [op] (M,d) norm2(x2)
//   | z (M,hid) fc1 pre-activation | h [op] (M,hid) gelu(z);
// after the layers: xL (M,d) | xL16 [op] (M,d) (16-bit only) | logits (M,V) (replaced in place by d loss / d logits).
// qk_norm: norm1 / norm2 are Identity, so u1 / u2 are x0 / x2 in operand form (exact: the f32 slots themselves, the u1 / u2 slots
// stay unused).  Exact: 21*d floats per token and layer, 5.6 GB per clip for the C138 shape; 16-bit: 52 d + 18 d NPL bytes.  In this
// layout (recompute = 0) nothing is recomputed except the attention probabilities (rebuilt inside the fused attention backward
// kernels; for S != 256 the spatial scores are materialised per layer in the workspace, never saved).
//
// recompute = 1 (the *_ex entry points) keeps one tensor per layer and rebuilds the rest in the backward:
//   L checkpoints x0[l] (M,d) f32, each rounded up to 256 bytes | ONE layer's slots u1 .. h as above, shared by every layer
//   | xL | xL16 | logits as above.
// The forward runs every layer in the shared slots, reading checkpoint l and writing checkpoint l + 1 (or xL); the backward of
// layer l first runs the same layer forward again from checkpoint l, without fc2 (its output is the next checkpoint, which no
// backward reads, and with Identity norms its 16-bit epilogue would write the NEXT layer's operand over this layer's u1), so every
// genie_train_backward_layer_ex call overwrites the shared slots.  With Identity norms in the 16-bit precisions layer l's u1 came
// from the fc2 epilogue of layer l - 1 (layer 0's from a cast); the recomputation makes it from the checkpoint in the same bits
// (Ops16::cast_like: in f16x3 the GEMM kernels do not all split a value below the f16 normal range alike).  The forward kernels are
// bit-reproducible, so the gradients are the same bits as with recompute = 0.  Size: at most the recompute = 0 size of a one-layer
// model plus the L checkpoints.
//
// MLP dropout (the *_drop entry points, genie_dropout with p > 0; kernels_dropout.hip): h = m0 s gelu(z), x3 = x2 + m1 s (fc2(h) + b2),
// keep masks recomputed from counters wherever they are applied, nothing stored.  Site 0: the h slot holds m0 gelu(z) -- zeroed, not
// scaled -- and s rides in the alpha of fc2 and of fc2's two backward products, which touches neither the bias nor its gradient; z
// keeps the pre-activation, and the backward zeroes dh with m0 before gelu'.  Site 1: the bias is inside the dropped term, so fc2
// writes t = s h . W2^T + b2 into the output slot without the residual and one pass turns it into x2 + m1 s t in place (with Identity
// norms in the 16-bit precisions it also writes the next layer's operand, in launch_cast16's rounding, which is what the recomputation
// then rebuilds it with); the backward hands fc2 a masked, scaled copy of the running dx in w.d1, dead at that point, and the residual
// branch keeps dx itself.  p = 0 launches exactly the step above.
//
// Training objective (genie_train_forward_obj, a genie_objective that is not neutral): the forward is the one above up to the logits;
// the loss launch is launch_ce_objective (kernels_loss.hip: label smoothing, z-loss, per-frame weights; five sums) instead of
// launch_ce_fwd_bwd, and leaves d loss / d logits in the same slot, so no backward entry point knows about it.  Neutral: the step above.
#include <cmath>

#include "kernels.hpp"

namespace genie {

constexpr float LN_EPS = 1e-5f;
static inline int npl_of(const genie_cfg& c) { return c.precision == GENIE_PREC_BF16 ? 1 : 2; }
static inline long PL(int npl, size_t n) { return npl == 2 ? (long)n : 0; }

struct TrainActs {                               // byte offsets
    size_t x0_stride;                            // layer l's input x0 is at x0_stride * l
    size_t slots, per_layer;                     // layer l's other slots start at slots + per_layer * l
    size_t qkvs, x1, qkvt, x2, z;                // inside a layer's slots, f32
    size_t u1, aos, x1h, aot, u2, h;             // inside a layer's slots, the operand the next Linear reads
    size_t xL, xL16, logits, total;              // in the buffer (xL16: operand)
    bool x_is_op;                                // u1 is x0 itself (and u2 is x2)
    bool recompute;
};
// recompute 0: every layer keeps its input and its slots, x0 first (x0_stride = per_layer).  1: the strip of checkpoints, then one
// layer's slots that every layer uses (per_layer = 0)
static TrainActs train_acts(const genie_cfg& c, int B, int recompute) {
    const bool exact = c.precision == GENIE_PREC_EXACT;
    const size_t M = (size_t)B * c.T * c.S, d = c.d_model, hid = c.hidden;
    const size_t V = (size_t)c.factored_vocab * c.num_factored;
    const size_t op = exact ? 4 : 2 * npl_of(c), align = exact ? 1 : 256;   // bytes of an operand element; slot alignment
    TrainActs a;
    a.recompute = recompute != 0;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + align - 1) / align * align; return at; };
    a.x0_stride = (M * d * 4 + 255) / 256 * 256;
    if (a.recompute) o = a.slots = a.x0_stride * c.num_layers;
    else { a.slots = 0; take(M * d * 4); }
    a.u1 = take(M * d * op); a.qkvs = take(M * 3 * d * 4); a.aos = take(M * d * op);
    a.x1 = take(M * d * 4); a.x1h = exact ? a.x1 : take(M * d * op); a.qkvt = take(M * 3 * d * 4); a.aot = take(M * d * op);
    a.x2 = take(M * d * 4); a.u2 = take(M * d * op); a.z = take(M * hid * 4); a.h = take(M * hid * op);
    if (a.recompute) {   // slot offsets count from a.slots
        for (size_t* off : {&a.u1, &a.qkvs, &a.aos, &a.x1, &a.x1h, &a.qkvt, &a.aot, &a.x2, &a.u2, &a.z, &a.h}) *off -= a.slots;
        a.per_layer = 0;
    } else {
        a.per_layer = a.x0_stride = o;
        o = a.per_layer * c.num_layers;
    }
    a.x_is_op = exact && c.qk_norm;   // Identity norms: the f32 residual stream is the operand
    if (a.x_is_op) a.u2 = a.x2;
    a.xL = take(M * d * 4); a.xL16 = exact ? a.xL : take(M * d * op); a.logits = take(M * V * 4);
    a.total = o;
    return a;
}

struct TrainWs {
    float *dx, *d1, *g, *p, *dp, *slabs, *lnpart, *colpart;
    float* qkn;  // (M, 2d) normalised q | k of the attention being differentiated (qk_norm only)
    double* dscratch;  // 1024 doubles (sumsq partials)
    size_t slab_floats, total;
};
static TrainWs train_ws(const genie_cfg& c, int B, void* base) {
    const size_t M = (size_t)B * c.T * c.S, d = c.d_model;
    const size_t wide = (size_t)(3 * d > (size_t)c.hidden ? 3 * d : c.hidden);
    const size_t V = (size_t)c.factored_vocab * c.num_factored;
    const size_t scores = M * c.num_heads * c.S;
    size_t maxw = (size_t)c.hidden * d;
    if (3 * d * d > maxw) maxw = 3 * d * d;
    if (V * d > maxw) maxw = V * d;
    size_t maxn = wide > V ? wide : V;
    TrainWs w;
    size_t o = 0;
    auto take = [&](size_t floats) { size_t at = o; o += (floats * 4 + 255) / 256 * 256; return at; };
    const size_t o_dx = take(M * d), o_d1 = take(M * d), o_g = take(M * wide), o_p = take(scores), o_dp = take(scores);
    w.slab_floats = 64 * maxw;
    const size_t o_sl = take(w.slab_floats), o_ln = take(ln_bwd_scratch_floats((int)d));
    const size_t cp_rows = M / 64 > (size_t)COLSUM_CHUNKS ? M / 64 : (size_t)COLSUM_CHUNKS;
    const size_t o_cp = take(cp_rows * maxn), o_ds = take(2 * 1024);
    const size_t o_qkn = take(c.qk_norm ? M * 2 * d : 0);
    w.total = o;
    char* b = (char*)base;
    w.dx = (float*)(b + o_dx); w.d1 = (float*)(b + o_d1); w.g = (float*)(b + o_g); w.p = (float*)(b + o_p);
    w.dp = (float*)(b + o_dp); w.slabs = (float*)(b + o_sl); w.lnpart = (float*)(b + o_ln);
    w.colpart = (float*)(b + o_cp); w.dscratch = (double*)(b + o_ds);
    w.qkn = (float*)(b + o_qkn);
    return w;
}

// the activation layout of the *_ex entry points: 0 saves every layer, 1 recomputes them (see the top of this file)
static inline bool mode_ok(int recompute) { return recompute == 0 || recompute == 1; }
static int check_mode(int recompute, const char* fn) {
    GENIE_CHECK_ARG(mode_ok(recompute), "%s: recompute %d is neither 0 (save) nor 1 (recompute per layer)", fn, recompute);
    return GENIE_OK;
}

static int train_check(const genie_cfg* c, int B) {
    GENIE_CHECK_ARG(c != nullptr && B > 0, "training: cfg is NULL or B <= 0");
    GENIE_TRY(genie_check_config(c));
    if (c->precision != GENIE_PREC_EXACT)  // 16-bit GEMM operands: 64x64 transposition tiles, K-steps of 64
        GENIE_CHECK_SHAPE(c->d_model % 64 == 0 && c->hidden % 64 == 0 && (c->T * c->S) % 64 == 0 &&
                              (c->factored_vocab * c->num_factored) % 64 == 0,
                          "training step (16-bit): d_model, hidden, T*S and the vocabulary rows must be multiples of 64");
    GENIE_CHECK_SHAPE(c->S % 16 == 0 && c->head_dim % 16 == 0 && c->d_model % 16 == 0 && c->hidden % 16 == 0 && c->T <= 64,
                      "training step: S, head_dim, d_model, hidden must be multiples of 16 and T <= 64");
    // the temporal attention backward and the qk-norm kernels of the backward exist for head_dim 32 / 64 only: refuse here,
    // before any forward is launched for a step that cannot finish
    GENIE_CHECK_SHAPE(c->head_dim == 32 || c->head_dim == 64, "training step: head_dim %d is not supported (32 or 64)",
                      c->head_dim);
    return GENIE_OK;
}

// one Linear y = x . W^T + b, W (N,K): the weight in every form a backend reads (wT16: the transposed 16-bit copy the 16-bit dgrad
// multiplies with), its bias (NULL: none) and, in the backward, where its gradients go (dw NULL: the weight is frozen; db NULL: no
// bias, or the bias is frozen -- include/genie_hip.h, "Frozen tensors")
struct Lin {
    const float* w; const uint16_t *w16, *wT16; const float* b;
    float *dw, *db;
    int N, K;
};
struct LayerLins { Lin qkv_s, proj_s, qkv_t, proj_t, fc1, fc2; };
// w: the layer's weights; t: their transposed 16-bit copies (NULL: forward, exact); g: its gradients (NULL: forward)
static LayerLins layer_lins(const genie_cfg& c, const genie_layer_weights& w, const genie_layer_weights* t,
                            const genie_layer_weights* g) {
    static const genie_layer_weights none{};
    const genie_layer_weights &T = t ? *t : none, &G = g ? *g : none;
    const int d = c.d_model, hid = c.hidden;
    auto lin = [](const float* W, const uint16_t* W16, const uint16_t* WT16, bool bias, const float* b, const float* dW,
                  const float* db, int N, int K) {
        return Lin{W, W16, WT16, bias ? b : nullptr, (float*)dW, bias ? (float*)db : nullptr, N, K};
    };
    auto qkv = [&](const genie_attn_weights& a, const genie_attn_weights& at, const genie_attn_weights& ag) {
        return lin(a.qkv_w, a.qkv_w16, at.qkv_w16, c.qkv_bias, a.qkv_b, ag.qkv_w, ag.qkv_b, 3 * d, d);
    };
    auto proj = [&](const genie_attn_weights& a, const genie_attn_weights& at, const genie_attn_weights& ag) {
        return lin(a.proj_w, a.proj_w16, at.proj_w16, c.proj_bias, a.proj_b, ag.proj_w, ag.proj_b, d, d);
    };
    return LayerLins{qkv(w.spatial, T.spatial, G.spatial), proj(w.spatial, T.spatial, G.spatial),
                     qkv(w.temporal, T.temporal, G.temporal), proj(w.temporal, T.temporal, G.temporal),
                     lin(w.fc1_w, w.fc1_w16, T.fc1_w16, c.mlp_bias, w.fc1_b, G.fc1_w, G.fc1_b, hid, d),
                     lin(w.fc2_w, w.fc2_w16, T.fc2_w16, c.mlp_bias, w.fc2_b, G.fc2_w, G.fc2_b, d, hid)};
}
static Lin readout_lin(const genie_cfg& c, const genie_weights* w, const genie_weights* t, const genie_weights* g) {
    return Lin{w->out_w, w->out_w16, t ? t->out_w16 : nullptr, w->out_b, g ? (float*)g->out_w : nullptr,
               g ? (float*)g->out_b : nullptr, c.factored_vocab * c.num_factored, c.d_model};
}

// attention over saved qkv rows into the operand of the projection: f32 rows in `out`, or (out16) 16-bit planes, for which the
// generic kernel goes through the f32 scratch `out`
static int attn_fwd(const genie_cfg& c, const genie_attn_weights& aw, const float* qkv, bool temporal, float* out,
                    uint16_t* out16, int npl, int B, hipStream_t st) {
    const float* nw = c.qk_norm ? aw.norm_w : nullptr;
    const float* nb = c.qk_norm ? aw.norm_b : nullptr;
    const size_t pd = (size_t)B * c.T * c.S * c.d_model, plane = out16 ? PL(npl, pd) : 0;
    float* direct = out16 ? nullptr : out;
    int rc;
    if (temporal)
        rc = launch_attn_temporal_f32_mfma(qkv, direct, B, c.T, c.S, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw, nb,
                                           st, out16, plane);
    else if (out16)
        rc = launch_attn_spatial_split(qkv, nullptr, c.S, (long)B * c.T, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw,
                                       nb, st, out16, plane);
    else
        rc = launch_attn_spatial_f32_mfma(qkv, out, c.S, (long)B * c.T, c.d_model, c.num_heads, c.head_dim, c.attn_scale, nw,
                                          nb, st);
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    if (temporal)
        GENIE_TRY(launch_attn_generic(qkv, out, c.T, (long)B * c.S, c.S, (long)c.T * c.S, 1, c.S, c.d_model, c.num_heads,
                                      c.head_dim, c.attn_scale, 1, nw, nb, st));
    else
        GENIE_TRY(launch_attn_generic(qkv, out, c.S, (long)B * c.T, 1, c.S, 0, 1, c.d_model, c.num_heads, c.head_dim,
                                      c.attn_scale, 0, nw, nb, st));
    return out16 ? launch_cast16(npl, out, out16, pd, st) : GENIE_OK;
}
// where the backward reads q and k: the saved qkv itself, or (qk_norm) their LayerNorm'd copies in w.qkn
struct QkSrc { const float* p; long ld; };
static int qk_source(const genie_cfg& c, const genie_attn_weights& aw, const float* qkv, TrainWs& w, int B, QkSrc* out,
                     hipStream_t st) {
    if (!c.qk_norm) { *out = QkSrc{qkv, 3L * c.d_model}; return GENIE_OK; }
    GENIE_TRY(launch_qk_norm_fwd(qkv, w.qkn, aw.norm_w, aw.norm_b, (long)B * c.T * c.S, c.num_heads, c.head_dim, c.d_model,
                                 st));
    *out = QkSrc{w.qkn, 2L * c.d_model};
    return GENIE_OK;
}
// d/d(normalised q,k) -> d/d(raw q,k) in place, and the shared affine's gradient
static int qk_norm_backward(const genie_cfg& c, const genie_attn_weights& aw, const genie_attn_weights& g, const float* qkv,
                            float* dqkv, TrainWs& w, int B, float beta, hipStream_t st) {
    if (!c.qk_norm) return GENIE_OK;
    return launch_qk_norm_bwd(qkv, dqkv, aw.norm_w, (float*)g.norm_w, (float*)g.norm_b, (long)B * c.T * c.S, c.num_heads,
                              c.head_dim, c.d_model, beta, w.lnpart, st);
}

// spatial attention backward: qkv (BT*S,3d), dao (BT*S,d) -> dqkv (BT*S,3d), by the implementation `path` names
// (GENIE_SPATIAL_BWD_*).  A forced path that does not take the geometry answers GENIE_E_UNSUPPORTED with nothing enqueued; AUTO is
// the fused f32 kernel where it takes the geometry, else the materialised scores.  Scratch: p and dp hold BT*H*S*S floats each for the
// materialised path; the bf16 pair keeps its row statistics (BT*H*S*4 floats) in p; the fused kernel reads neither.
static int spatial_attn_bwd(const float* qkv, QkSrc qk, const float* dao, float* dqkv, float* p, float* dp, int BT, int S, int d,
                            int H, int Dh, float sc, int path, hipStream_t st) {
    const long q3 = (long)S * 3 * d, ss = (long)S * S, hss = (long)H * ss, sd = (long)S * d;
    const long qld = qk.ld, qs = (long)S * qk.ld;
    if (path == GENIE_SPATIAL_BWD_BF16)     // the backward products on the bf16 matrix cores as well
        return launch_attn_spatial_bwd_bf16(qkv, qk.p, qk.ld, dao, dqkv, p, BT, S, d, H, Dh, sc, st);
    if (path != GENIE_SPATIAL_BWD_MATERIALISED) {   // production geometry: fused kernel, no S x S traffic
        const int rc = launch_attn_spatial_bwd_fused(qkv, qk.p, qk.ld, dao, dqkv, BT, S, d, H, Dh, sc, st);
        if (path == GENIE_SPATIAL_BWD_FUSED || rc != GENIE_E_UNSUPPORTED) return rc;
    }
    // P = softmax(scale Q K^T)
    GENIE_TRY(launch_gemm_f32_gen(false, false, qk.p, qld, qs, Dh, qk.p + d, qld, qs, Dh, nullptr, nullptr, p, S, hss,
                                  ss, S, S, Dh, BT, H, 1, 0, sc, st));
    GENIE_TRY(launch_softmax_rows(p, (long)BT * H * S, S, st));
    // dV = P^T dO
    GENIE_TRY(launch_gemm_f32_gen(true, true, p, S, hss, ss, dao, d, sd, Dh, nullptr, nullptr, dqkv + 2 * d, 3 * d, q3,
                                  Dh, S, Dh, S, BT, H, 1, 0, 1.0f, st));
    // dP = dO V^T, dS = P (dP - rowsum(P dP))
    GENIE_TRY(launch_gemm_f32_gen(false, false, dao, d, sd, Dh, qkv + 2 * d, 3 * d, q3, Dh, nullptr, nullptr, dp, S, hss,
                                  ss, S, S, Dh, BT, H, 1, 0, 1.0f, st));
    GENIE_TRY(launch_softmax_bwd_rows(p, dp, (long)BT * H * S, S, st));
    // dQ = scale dS K,  dK = scale dS^T Q
    GENIE_TRY(launch_gemm_f32_gen(false, true, dp, S, hss, ss, qk.p + d, qld, qs, Dh, nullptr, nullptr, dqkv, 3 * d, q3,
                                  Dh, S, Dh, S, BT, H, 1, 0, sc, st));
    GENIE_TRY(launch_gemm_f32_gen(true, true, dp, S, hss, ss, qk.p, qld, qs, Dh, nullptr, nullptr, dqkv + d, 3 * d, q3,
                                  Dh, S, Dh, S, BT, H, 1, 0, sc, st));
    return GENIE_OK;
}
// the training step's choice: the bf16 precision takes the bf16 pair where that takes the geometry (GENIE_ATTN_BWD16=0 in a study
// build: never), every other case the f32 kernels
static int train_spatial_bwd_path(const genie_cfg& c, long qk_ld) {
    static const int bwd16 = study_env("GENIE_ATTN_BWD16", 1);
    return c.precision == GENIE_PREC_BF16 && bwd16 && attn_spatial_bwd_bf16_takes(c.S, c.head_dim, qk_ld, c.d_model)
               ? GENIE_SPATIAL_BWD_BF16 : GENIE_SPATIAL_BWD_AUTO;
}

struct TrainWs16 {
    uint16_t *dy16, *dy16T, *xT16;
    size_t total;
};
// the 16-bit backend's gradient copies, appended behind the exact workspace
static TrainWs16 train_ws16(const genie_cfg& c, int B, int npl, void* base, size_t exact_total) {
    const size_t M = (size_t)B * c.T * c.S, d = c.d_model;
    const size_t V = (size_t)c.factored_vocab * c.num_factored;
    size_t wide = (size_t)(3 * d > (size_t)c.hidden ? 3 * d : c.hidden);
    if (V > wide) wide = V;
    size_t o = exact_total;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    const size_t o1 = take(M * wide * 2 * npl), o2 = take(M * wide * 2 * npl), o3 = take(M * wide * 2 * npl);
    TrainWs16 w;
    w.total = o;
    char* b = (char*)base;
    w.dy16 = (uint16_t*)(b + o1); w.dy16T = (uint16_t*)(b + o2); w.xT16 = (uint16_t*)(b + o3);
    return w;
}
// bf16: the weight gradient runs on the TN kernel (kernels_gemm_tn.hip) from row-major operands when the shapes allow, and then
// neither the gradient nor the saved activation needs a transposed copy (GENIE_WGRAD_TN=0: the transposed-copy path, for A/B)
static bool use_tn(int npl, int M, int N, int K) {
    static const int tn = study_env("GENIE_WGRAD_TN", 1);
    return tn && npl == 1 && M % 64 == 0 && N % 256 == 0 && K % 128 == 0;
}
// y(f32) / y16 = alpha * x16 . W16^T (+b) (+R), x16 (M,K), W16 (N,K)
static int lin16_flags(int npl, bool y, bool y16, bool R, int flags) {
    if (y) flags |= G16X_OUTF32;
    if (y16) flags |= G16X_OUT16;
    if (R) flags |= G16X_ACCUM;
    if (npl == 2) flags |= G16X_WIDEW;   // (as the wgrad products below: the step's f16x3 GEMMs all run on the two-accumulator kernels)
    return flags;
}
static int lin16(int npl, const uint16_t* x16, const uint16_t* W16, const float* b, const float* R, float* y, uint16_t* y16,
                 int M, int N, int K, float alpha, hipStream_t st, int flags = 0) {
    flags = lin16_flags(npl, y, y16, R, flags);
    return launch_gemm16_ex(npl, x16, K, PL(npl, (size_t)M * K), W16, K, PL(npl, (size_t)N * K), b, (R && R != y) ? R : nullptr,
                            y, y16, PL(npl, (size_t)M * N), N, M, N, K, flags, alpha, st, 1, 0, 0, 0);
}
// dW[N,K] (beta*dW +)= alpha * dY^T . X from the TRANSPOSED 16-bit copies dYT (N, Mtok), XT (K, Mtok)
static int wgrad16(int npl, const uint16_t* dYT, const uint16_t* XT, float* dW, int Mtok, int N, int K, float alpha,
                   float beta, float* slabs, size_t slab_floats, hipStream_t st) {
    const int tiles = ((N + 255) / 256) * ((K + 127) / 128);
    int ns = 1;
    while (ns < 64 && tiles * ns < 256 && Mtok % (64 * ns * 2) == 0 && (size_t)(ns * 2) * N * K <= slab_floats) ns *= 2;
    const long pa = PL(npl, (size_t)N * Mtok), pw = PL(npl, (size_t)K * Mtok);
    const int wide = npl == 2 ? G16X_WIDEW : 0;   // the W operand is an activation, not a |w| < 32 weight matrix
    if (ns == 1)
        return launch_gemm16_ex(npl, dYT, Mtok, pa, XT, Mtok, pw, nullptr, nullptr, dW, nullptr, 0, K, N, K, Mtok,
                                G16X_OUTF32 | (beta != 0.f ? G16X_ACCUM : 0) | wide, alpha, st, 1, 0, 0, 0);
    const int kc = Mtok / ns;
    GENIE_TRY(launch_gemm16_ex(npl, dYT, Mtok, pa, XT, Mtok, pw, nullptr, nullptr, slabs, nullptr, 0, K, N, K, kc,
                               G16X_OUTF32 | wide, alpha, st, ns, kc, kc, (long)N * K));
    return launch_slab_reduce(slabs, ns, (size_t)N * K, dW, beta, st);
}

static int need16(const genie_weights* wt, const genie_cfg& c, const char* what) {
    if (c.precision == GENIE_PREC_EXACT) return GENIE_OK;
    GENIE_CHECK_ARG(wt && wt->out_w16, "%s: 16-bit weight copies missing (genie_train_pack_weights)", what);
    for (int l = 0; l < c.num_layers; ++l) {
        const genie_layer_weights& lw = wt->layers_host[l];
        GENIE_CHECK_ARG(lw.spatial.qkv_w16 && lw.spatial.proj_w16 && lw.temporal.qkv_w16 && lw.temporal.proj_w16 &&
                            lw.fc1_w16 && lw.fc2_w16,
                        "%s: 16-bit weight copies missing in layer %d (genie_train_pack_weights)", what, l);
    }
    return GENIE_OK;
}

// MLP dropout of one call: off (p = 0, the default: no dropout kernel is launched), or the scale 1 / (1 - p) and the mask key
struct Drop {
    bool on = false;
    float s = 1.0f;
    DropKey k{};
    DropKey key(int layer, int site) const { DropKey r = k; r.stream = (uint32_t)(layer * 2 + site); return r; }
};
static bool drop_p_ok(const genie_dropout* dr) { return !dr || (dr->p >= 0.0f && dr->p < 1.0f); }   // (NaN fails both)
// the key of *dr's masks, `stream` still to be set; thr = floor((double)p * 2^32): 0 at p = 0, where every word passes
static DropKey drop_key(const genie_dropout& dr) {
    return DropKey{(uint32_t)dr.seed, (uint32_t)(dr.seed >> 32), 0u, dr.call, (uint32_t)((double)dr.p * 4294967296.0)};
}
static Drop make_drop(const genie_dropout* dr) {
    if (!dr || dr->p == 0.0f) return Drop{};
    return Drop{true, 1.0f / (1.0f - dr->p), drop_key(*dr)};
}

// The training objective of one call (genie_objective): neutral = the step's own loss kernels, untouched.  T: the frames of the call
// (n_frames is 0 or T; the struct holds 64 weights)
static bool objective_neutral(const genie_objective* ob) {
    return !ob || (ob->label_smoothing == 0.0f && ob->z_loss == 0.0f && ob->n_frames == 0);
}
static int objective_ok(const genie_objective* ob, int T, const char* fn) {
    if (!ob) return GENIE_OK;
    GENIE_CHECK_ARG(ob->label_smoothing >= 0.0f && ob->label_smoothing < 1.0f, "%s: label_smoothing %g is not in [0, 1)", fn,
                    (double)ob->label_smoothing);   // (NaN fails both)
    GENIE_CHECK_ARG(ob->z_loss >= 0.0f && std::isfinite(ob->z_loss), "%s: z_loss %g is negative or not finite", fn, (double)ob->z_loss);
    GENIE_CHECK_ARG(ob->n_frames == 0 || (ob->n_frames == T && T <= 64), "%s: n_frames %d is neither 0 nor T = %d (at most 64)", fn,
                    ob->n_frames, T);
    for (int t = 0; t < ob->n_frames; ++t)
        GENIE_CHECK_ARG(ob->frame_weight[t] >= 0.0f && std::isfinite(ob->frame_weight[t]),
                        "%s: frame_weight[%d] = %g is negative or not finite", fn, t, (double)ob->frame_weight[t]);
    return GENIE_OK;
}

// Distillation of one call (genie_distill): neutral = no struct or alpha == 0, the call of before; the teacher pointer is then never looked at
static bool distill_neutral(const genie_distill* ds) { return !ds || ds->alpha == 0.0f; }
// (teacher: the rows of this call -- the struct's pointer, or genie_ce_distill's own argument)
static int distill_ok(const genie_distill* ds, const float* teacher, const char* fn) {
    if (!ds) return GENIE_OK;
    GENIE_CHECK_ARG(ds->alpha >= 0.0f && ds->alpha <= 1.0f, "%s: distillation alpha %g is not in [0, 1]", fn, (double)ds->alpha);   // (NaN fails both)
    GENIE_CHECK_ARG(ds->temperature > 0.0f && std::isfinite(ds->temperature), "%s: distillation temperature %g is not finite and > 0", fn,
                    (double)ds->temperature);
    GENIE_CHECK_ARG(ds->alpha == 0.0f || teacher, "%s: distillation alpha %g without teacher logits", fn, (double)ds->alpha);
    return GENIE_OK;
}
// the teacher rows [teacher, teacher + floats) must not meet the student logits (same extent) or the seven sums
static int distill_apart(const float* teacher, const float* logits, size_t floats, const double* sums, const char* fn) {
    const uintptr_t t0 = (uintptr_t)teacher, t1 = t0 + floats * sizeof(float), l0 = (uintptr_t)logits, l1 = l0 + floats * sizeof(float),
                    s0 = (uintptr_t)sums, s1 = s0 + 7 * sizeof(double);
    GENIE_CHECK_ARG(t1 <= l0 || l1 <= t0, "%s: the teacher logits overlap the student logits", fn);
    GENIE_CHECK_ARG(t1 <= s0 || s1 <= t0, "%s: the teacher logits overlap the sums", fn);
    return GENIE_OK;
}
// the pointers and geometry of a loss launch on raw arguments (genie_ce_objective, genie_ce_distill)
static int loss_call_ok(const float* logits, const int64_t* ids, const int64_t* labels, const double* sums, int n_clips, int T, int S, int vf,
                        int nfac, const char* fn) {
    GENIE_CHECK_ARG(logits && ids && labels && sums, "%s: NULL argument", fn);
    GENIE_CHECK_ARG(n_clips >= 1 && T >= 1 && S >= 1 && vf >= 1 && nfac >= 1 && nfac <= 4,
                    "%s: n_clips %d, T %d, S %d, vf %d must be positive and nfac %d in 1 .. 4", fn, n_clips, T, S, vf, nfac);
    GENIE_CHECK_ARG((long)vf * nfac <= INT32_MAX, "%s: a row of %d x %d logits", fn, nfac, vf);
    return GENIE_OK;
}

// ================================================================================================
// The two backends.  Same members: Operand (the element type of a saved Linear input), cast / norm / attention (produce an
// operand), linear, linear_backward.  M tokens; beta 1 accumulates into the gradients; w is unused by the forward.
// With dropout (dr.on): hidden_drop = the fc1 call with the site 0 mask on its gelu operand, residual_drop = y = R + m s t (and y_op),
// mask_dh = the site 0 mask on dh in front of fc1's linear_backward (kGeluInMask: it applied gelu' as well, so that call gets no z).
// ================================================================================================
struct ExactOps {
    using Operand = float;
    const genie_cfg& c;
    int B, M;
    hipStream_t st;
    TrainWs w;
    float beta;
    Drop dr;
    static constexpr bool kGeluInMask = true;

    int hidden_drop(const Operand* x, const Lin& l, float* z, Operand* h, const DropKey& k) {
        GENIE_TRY(linear(x, l, nullptr, z, nullptr, nullptr));
        return launch_drop_gelu_fwd(z, h, (size_t)M * l.N, k, st);
    }
    int residual_drop(const float* t, const float* R, float* y, Operand* /*y_op*/, size_t n, const DropKey& k) {
        return launch_drop_axpy(0, t, R, y, nullptr, n, dr.s, k, st);
    }
    int mask_dh(float* dh, const float* z, size_t n, const DropKey& k) { return launch_drop_gelu_bwd(z, dh, n, k, st); }

    int cast(const float*, Operand*, size_t) { return GENIE_OK; }   // train_acts: the f32 rows are the operand
    int cast_like(const float*, Operand*, const Lin&) { return GENIE_OK; }
    int norm(const float* x, const float* g, const float* b, Operand* u) {
        return launch_layer_norm(x, g, b, u, M, c.d_model, LN_EPS, st);
    }
    int attention(bool temporal, const genie_attn_weights& aw, const float* qkv, Operand* ao) {
        return attn_fwd(c, aw, qkv, temporal, ao, nullptr, 0, B, st);
    }
    // y = alpha * x . W^T + b (+ R); gelu: also gelu(y) as the next operand.  y_op (y again, in operand form) is y itself here.
    int linear(const Operand* x, const Lin& l, const float* R, float* y, Operand* /*y_op*/, Operand* gelu, float alpha = 1.0f) {
        GENIE_TRY(launch_gemm_f32_gen(false, false, x, l.K, 0, 0, l.w, l.K, 0, 0, l.b, R, y, l.N, 0, 0, M, l.N, l.K, 1, 1, 1, 0,
                                      alpha, st));
        return gelu ? launch_gelu_fwd(y, gelu, (size_t)M * l.N, st) : GENIE_OK;
    }
    // from dy (M,N) (z: d gelu(z), turned into dz in place first) and the saved input x (M,K): l.dw, l.db and
    // dx = alpha * dy . W (+ R), W (N,K) read k-major
    int linear_backward(float* dy, const Operand* x, const Lin& l, const float* z, const float* R, float* dx, float alpha = 1.0f) {
        if (z) GENIE_TRY(launch_gelu_bwd(z, dy, (size_t)M * l.N, st));
        if (l.dw) GENIE_TRY(launch_wgrad_f32(dy, l.N, x, l.K, l.dw, M, l.N, l.K, alpha, beta, w.slabs, w.slab_floats, st));
        if (l.db) GENIE_TRY(launch_colsum(dy, l.N, M, l.N, l.db, beta, w.colpart, st));
        return launch_gemm_f32_gen(false, true, dy, l.N, 0, 0, l.w, l.K, 0, 0, nullptr, R, dx, l.K, 0, 0, M, l.K, l.N, 1, 1, 1, 0,
                                   alpha, st);
    }
};

struct Ops16 {
    using Operand = uint16_t;
    const genie_cfg& c;
    int B, M;
    hipStream_t st;
    TrainWs w;
    float beta;
    int npl;
    TrainWs16 h;   // backward only
    float* tmp;    // (M,d) f32 behind the generic attention kernels.  Forward: the logits region, free until the readout;
                   // recomputing backward: w.d1 (the logits region holds d logits until the head has run); else unused
    Drop dr;
    static constexpr bool kGeluInMask = false;   // gelu' is part of cast_t_bias

    int hidden_drop(const Operand* x, const Lin& l, float* z, Operand* h, const DropKey& k) {
        GENIE_TRY(linear(x, l, nullptr, z, nullptr, h));
        return launch_drop_zero16(npl, h, (size_t)M * l.N, k, st);
    }
    int residual_drop(const float* t, const float* R, float* y, Operand* y_op, size_t n, const DropKey& k) {
        return launch_drop_axpy(y_op ? npl : 0, t, R, y, y_op, n, dr.s, k, st);
    }
    int mask_dh(float* dh, const float*, size_t n, const DropKey& k) { return launch_drop_axpy(0, dh, nullptr, dh, nullptr, n, 1.0f, k, st); }

    int cast(const float* x, Operand* u, size_t n) { return launch_cast16(npl, x, u, n, st); }
    // y (M, l.N) -> the y_op that linear(x, l, R, y, y_op, nullptr) wrote beside it: the same bits, which in f16x3 depend on the kernel
    // that took the product (launch_cast16_like_gemm)
    int cast_like(const float* y, Operand* y_op, const Lin& l) {
        return launch_cast16_like_gemm(npl, y, y_op, M, l.N, l.K, lin16_flags(npl, true, true, true, 0), st);
    }
    int norm(const float* x, const float* g, const float* b, Operand* u) {
        if (npl == 1) return launch_layer_norm_bf16(x, g, b, u, M, c.d_model, LN_EPS, st);
        return launch_layer_norm_split(x, g, b, u, (size_t)M * c.d_model, M, c.d_model, LN_EPS, st);
    }
    int attention(bool temporal, const genie_attn_weights& aw, const float* qkv, Operand* ao) {
        return attn_fwd(c, aw, qkv, temporal, tmp, ao, npl, B, st);
    }
    // one GEMM: the epilogue writes y, y_op (y in operand form) or gelu (gelu(y) in operand form: the f32 pre-activation is kept for gelu')
    int linear(const Operand* x, const Lin& l, const float* R, float* y, Operand* y_op, Operand* gelu, float alpha = 1.0f) {
        return lin16(npl, x, l.w16, l.b, R, y, gelu ? gelu : y_op, M, l.N, l.K, alpha, st, gelu ? G16X_GELU16 : 0);
    }

    // f16x3: the gradient copies made by cast_t_bias hold GRAD_SCALE16 times the gradient (kernels.hpp); the two products of
    // linear_backward that read them take alpha / grad_scale16(), exact in f32.  bf16: 1.
    float grad_scale16() const { return npl == 2 ? GRAD_SCALE16 : 1.0f; }
    // 16-bit copies of a gradient matrix (row-major, and transposed unless its weight gradient takes the TN kernel: Kw = the K of
    // that weight gradient), with gelu'(z) applied when z, and, in the same pass, its column sums (= the bias gradient).
    // transposed = false (the weight is frozen): the row-major copy alone, from the kernel that would have made both -- the same
    // bits in h.dy16 and the same slabs in w.colpart
    int cast_t_bias(float* in, int cols, const float* z, float* dbias, int Kw, bool transposed) {
        if (use_tn(npl, M, cols, Kw))
            GENIE_TRY(launch_cast_rows16(in, cols, z, h.dy16, M, cols, st, dbias ? w.colpart : nullptr));
        else
            GENIE_TRY(launch_cast_transpose16(npl, in, cols, z, h.dy16, transposed ? h.dy16T : nullptr, M, cols, st,
                                              dbias ? w.colpart : nullptr, grad_scale16()));
        return dbias ? launch_slab_reduce(w.colpart, M / 64, (size_t)cols, dbias, beta, st) : GENIE_OK;
    }
    // weight gradient from the gradient copies in `h` and the saved row-major 16-bit activation X16 (M, K)
    int wgrad_any(const Operand* X16, float* dW, int N, int K, float alpha) {
        if (use_tn(npl, M, N, K)) {
            const int rc = launch_wgrad16_tn(h.dy16, N, X16, K, dW, M, N, K, alpha, beta, w.slabs, w.slab_floats, st);
            GENIE_CHECK_SHAPE(rc != GENIE_E_UNSUPPORTED, "wgrad: TN kernel refused N=%d K=%d after its operand was prepared", N, K);
            return rc;
        }
        GENIE_TRY(launch_transpose16(npl, X16, h.xT16, M, K, st));
        return wgrad16(npl, h.dy16T, h.xT16, dW, M, N, K, alpha, beta, w.slabs, w.slab_floats, st);
    }
    int linear_backward(float* dy, const Operand* x, const Lin& l, const float* z, const float* R, float* dx, float alpha = 1.0f) {
        const float ga = alpha / grad_scale16();
        GENIE_TRY(cast_t_bias(dy, l.N, z, l.db, l.K, l.dw != nullptr));
        if (l.dw) GENIE_TRY(wgrad_any(x, l.dw, l.N, l.K, ga));
        return lin16(npl, h.dy16, l.wT16, nullptr, R, dx, nullptr, M, l.K, l.N, ga, st);
    }
};

// ================================================================================================
// The step, once for both backends
// ================================================================================================
// where one layer's activations live: its input x0, its slots (base of the TrainActs offsets), its u1 (a slot, or x0 itself), and
// where its output goes (the next layer's x0 and u1, or xL and xL16)
template <class Operand>
struct LayerAt {
    float* x0; char* slots; Operand* u1;
    float* xnext; Operand* xnext_op;
    float* F(size_t off) const { return (float*)(slots + off); }
    Operand* X(size_t off) const { return (Operand*)(slots + off); }
};
template <class Operand>
static LayerAt<Operand> layer_at(const genie_cfg& c, char* acts, const TrainActs& a, int l) {
    auto x0 = [&](int k) { return (float*)(acts + a.x0_stride * k); };
    auto u1 = [&](int k) { return a.x_is_op ? (Operand*)x0(k) : (Operand*)(acts + a.slots + a.per_layer * k + a.u1); };
    const bool last = l + 1 == c.num_layers;
    return LayerAt<Operand>{x0(l), acts + a.slots + a.per_layer * l, u1(l), last ? (float*)(acts + a.xL) : x0(l + 1),
                            last ? (Operand*)(acts + a.xL16) : u1(l + 1)};
}

// One STBlock from p.x0 (and, with Identity norms, its operand form p.u1) into the layer's slots; fc2: and its output into
// p.xnext / p.xnext_op.  The forward runs it whole; the recomputation in front of a layer's backward stops before fc2, whose output
// no backward reads.
// qk_norm: norm1 / norm2 are Identity (st_transformer.py:44,67), so the operand of qkv_s / fc1 is the residual stream itself:
// the Linear that produces it hands it over in operand form (y_op); layer 0 (and a recomputed layer) gets its from a cast.  Else
// norm1 / norm2 produce the operand, and the readout's comes from a cast.
template <class Ops>
static int layer_forward(Ops& o, const genie_layer_weights& lw, const LayerLins& n, const TrainActs& a,
                         const LayerAt<typename Ops::Operand>& p, int layer, bool fc2) {
    const bool idn = o.c.qk_norm;
    // spatial sub-block (st_transformer.py:73-74)
    if (!idn) GENIE_TRY(o.norm(p.x0, lw.norm1_w, lw.norm1_b, p.u1));
    GENIE_TRY(o.linear(p.u1, n.qkv_s, nullptr, p.F(a.qkvs), nullptr, nullptr));
    GENIE_TRY(o.attention(false, lw.spatial, p.F(a.qkvs), p.X(a.aos)));
    GENIE_TRY(o.linear(p.X(a.aos), n.proj_s, p.x0, p.F(a.x1), p.X(a.x1h), nullptr));
    // temporal sub-block (st_transformer.py:77-78)
    GENIE_TRY(o.linear(p.X(a.x1h), n.qkv_t, nullptr, p.F(a.qkvt), nullptr, nullptr));
    GENIE_TRY(o.attention(true, lw.temporal, p.F(a.qkvt), p.X(a.aot)));
    GENIE_TRY(o.linear(p.X(a.aot), n.proj_t, p.F(a.x1), p.F(a.x2), idn ? p.X(a.u2) : nullptr, nullptr));
    // MLP sub-block (st_transformer.py:81, 16-25)
    if (!idn) GENIE_TRY(o.norm(p.F(a.x2), lw.norm2_w, lw.norm2_b, p.X(a.u2)));
    if (!o.dr.on) {
        GENIE_TRY(o.linear(p.X(a.u2), n.fc1, nullptr, p.F(a.z), nullptr, p.X(a.h)));
        if (!fc2) return GENIE_OK;
        return o.linear(p.X(a.h), n.fc2, p.F(a.x2), p.xnext, idn ? p.xnext_op : nullptr, nullptr);
    }
    // ... with dropout (st_transformer.py:22-25): h = m0 gelu(z), t = s h . W2^T + b2 in the output slot, x3 = x2 + m1 s t in place
    GENIE_TRY(o.hidden_drop(p.X(a.u2), n.fc1, p.F(a.z), p.X(a.h), o.dr.key(layer, 0)));
    if (!fc2) return GENIE_OK;
    GENIE_TRY(o.linear(p.X(a.h), n.fc2, nullptr, p.xnext, nullptr, nullptr, o.dr.s));
    return o.residual_drop(p.xnext, p.F(a.x2), p.xnext, idn ? p.xnext_op : nullptr, (size_t)o.M * o.c.d_model, o.dr.key(layer, 1));
}

template <class Ops>
static int train_forward(Ops& o, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels, char* acts,
                         const TrainActs& a, double* sums, const EmbedAct* act, const genie_objective* obj, const genie_distill* ds) {
    using Operand = typename Ops::Operand;
    const genie_cfg& c = o.c;
    const size_t pd = (size_t)o.M * c.d_model;
    float *xL = (float*)(acts + a.xL), *logits = (float*)(acts + a.logits);
    Operand* xL_op = (Operand*)(acts + a.xL16);
    const LayerAt<Operand> first = layer_at<Operand>(c, acts, a, 0);
    GENIE_TRY(launch_embed(c, *wt, input_ids, o.B, first.x0, o.st, act));
    const bool idn = c.qk_norm;
    if (idn) GENIE_TRY(o.cast(first.x0, first.u1, pd));
    for (int l = 0; l < c.num_layers; ++l) {
        const genie_layer_weights& lw = wt->layers_host[l];
        GENIE_TRY(layer_forward(o, lw, layer_lins(c, lw, nullptr, nullptr), a, layer_at<Operand>(c, acts, a, l), l, true));
    }
    if (!idn) GENIE_TRY(o.cast(xL, xL_op, pd));
    GENIE_TRY(o.linear(xL_op, readout_lin(c, wt, nullptr, nullptr), nullptr, logits, nullptr, nullptr, c.readout_mult));
    // ds (checked, not neutral): the objective's loss with the teacher's rows beside the student's
    return launch_train_loss("genie_train_forward", logits, input_ids, labels, o.B, c.T, c.S, c.factored_vocab, c.num_factored,
                             (int64_t)c.image_vocab_size, obj, ds, ds ? ds->teacher_logits : nullptr, sums, o.st);
}

// d loss / d logits (in the logits slot) -> the readout's gradients and d xL in w.dx
template <class Ops>
static int train_backward_head(Ops& o, const genie_weights* wt, const genie_weights* wT, const genie_weights* grads, char* acts,
                               const TrainActs& a) {
    return o.linear_backward((float*)(acts + a.logits), (const typename Ops::Operand*)(acts + a.xL16),
                             readout_lin(o.c, wt, wT, grads), nullptr, nullptr, o.w.dx, o.c.readout_mult);
}

// w.dx: d loss / d (the layer's output) -> d loss / d (its input), and the layer's gradients
template <class Ops>
static int train_backward_layer(Ops& o, const genie_weights* wt, const genie_weights* wT, const genie_weights* grads, int layer,
                                char* acts, const TrainActs& a) {
    const genie_cfg& c = o.c;
    const int d = c.d_model, M = o.M, B = o.B;
    const float beta = o.beta;
    hipStream_t st = o.st;
    TrainWs& w = o.w;
    const genie_layer_weights& lw = wt->layers_host[layer];
    const genie_layer_weights& g = grads->layers_host[layer];
    const LayerLins n = layer_lins(c, lw, wT ? &wT->layers_host[layer] : nullptr, &g);
    const LayerAt<typename Ops::Operand> p = layer_at<typename Ops::Operand>(c, acts, a, layer);
    auto F = [&](size_t off) { return p.F(off); };
    auto X = [&](size_t off) { return (const typename Ops::Operand*)p.X(off); };
    float* dx = w.dx;
    QkSrc qk;

    // ---- recompute: the layer's slots again from its checkpoint, as the forward made them.  Identity norms: u1 in the bits the
    // forward gave it -- layer 0's from a cast, a later layer's from the epilogue of the fc2 before it (every layer's fc2 has this
    // layer's shape; with dropout from the site 1 pass behind that fc2, which rounds as the cast does).  The 16-bit backend's
    // attention scratch is w.d1, free until the MLP's backward below.
    if (a.recompute) {
        if (c.qk_norm) GENIE_TRY(layer == 0 || o.dr.on ? o.cast(p.x0, p.u1, (size_t)M * d) : o.cast_like(p.x0, p.u1, n.fc2));
        GENIE_TRY(layer_forward(o, lw, n, a, p, layer, false));
    }

    // ---- MLP: x3 = x2 + fc2(gelu(fc1(norm2(x2))))  (st_transformer.py:81, 16-25)
    const float* z = F(a.z);
    if (!o.dr.on) {
        GENIE_TRY(o.linear_backward(dx, X(a.h), n.fc2, nullptr, nullptr, w.g));             // dh
    } else {   // fc2's dy = m1 s dx in w.d1 (the residual branch keeps dx); dh = s dy . W2; then m0 on dh
        GENIE_TRY(launch_drop_axpy(0, dx, nullptr, w.d1, nullptr, (size_t)M * d, o.dr.s, o.dr.key(layer, 1), st));
        GENIE_TRY(o.linear_backward(w.d1, X(a.h), n.fc2, nullptr, nullptr, w.g, o.dr.s));
        GENIE_TRY(o.mask_dh(w.g, z, (size_t)M * c.hidden, o.dr.key(layer, 0)));
        if (Ops::kGeluInMask) z = nullptr;
    }
    if (c.qk_norm) {
        GENIE_TRY(o.linear_backward(w.g, X(a.u2), n.fc1, z, dx, dx));                       // Identity norm: dx += dz . W1
    } else {
        GENIE_TRY(o.linear_backward(w.g, X(a.u2), n.fc1, z, nullptr, w.d1));                // d norm2 output
        GENIE_TRY(launch_ln_bwd(F(a.x2), lw.norm2_w, w.d1, dx, (float*)g.norm2_w, (float*)g.norm2_b, M, d, LN_EPS, beta,
                                w.lnpart, st));
    }

    // ---- temporal: x2 = x1 + proj(attn(qkv(x1))), no pre-norm  (st_transformer.py:77-78)
    GENIE_TRY(o.linear_backward(dx, X(a.aot), n.proj_t, nullptr, nullptr, w.d1));           // d attention output
    GENIE_TRY(qk_source(c, lw.temporal, F(a.qkvt), w, B, &qk, st));
    GENIE_TRY(launch_attn_temporal_bwd(F(a.qkvt), qk.p, qk.ld, w.d1, w.g, B, c.T, c.S, d, c.num_heads, c.head_dim,
                                       c.attn_scale, st));
    GENIE_TRY(qk_norm_backward(c, lw.temporal, g.temporal, F(a.qkvt), w.g, w, B, beta, st));
    GENIE_TRY(o.linear_backward(w.g, X(a.x1h), n.qkv_t, nullptr, dx, dx));                  // dx += dqkv . Wqkv

    // ---- spatial: x1 = x0 + proj(attn(qkv(norm1(x0))))  (st_transformer.py:73-74)
    GENIE_TRY(o.linear_backward(dx, X(a.aos), n.proj_s, nullptr, nullptr, w.d1));
    GENIE_TRY(qk_source(c, lw.spatial, F(a.qkvs), w, B, &qk, st));
    GENIE_TRY(spatial_attn_bwd(F(a.qkvs), qk, w.d1, w.g, w.p, w.dp, B * c.T, c.S, d, c.num_heads, c.head_dim, c.attn_scale,
                               train_spatial_bwd_path(c, qk.ld), st));
    GENIE_TRY(qk_norm_backward(c, lw.spatial, g.spatial, F(a.qkvs), w.g, w, B, beta, st));
    if (c.qk_norm) return o.linear_backward(w.g, p.u1, n.qkv_s, nullptr, dx, dx);
    GENIE_TRY(o.linear_backward(w.g, p.u1, n.qkv_s, nullptr, nullptr, w.d1));               // d norm1 output
    return launch_ln_bwd(p.x0, lw.norm1_w, w.d1, dx, (float*)g.norm1_w, (float*)g.norm1_b, M, d, LN_EPS, beta, w.lnpart, st);
}

}  // namespace genie

using namespace genie;

extern "C" {

size_t genie_train_activation_bytes(const genie_cfg* cfg, int B) { return genie_train_activation_bytes_ex(cfg, B, 0); }
size_t genie_train_workspace_bytes(const genie_cfg* cfg, int B) { return genie_train_workspace_bytes_ex(cfg, B, 0); }

size_t genie_train_activation_bytes_ex(const genie_cfg* cfg, int B, int recompute) {
    if (!cfg || B <= 0 || !mode_ok(recompute)) return 0;
    return train_acts(*cfg, B, recompute).total;
}
// the same in both modes: the recomputation's only scratch, behind the 16-bit backend's generic attention, is w.d1
size_t genie_train_workspace_bytes_ex(const genie_cfg* cfg, int B, int recompute) {
    if (!cfg || B <= 0 || !mode_ok(recompute)) return 0;
    const size_t exact = train_ws(*cfg, B, nullptr).total;
    if (cfg->precision != GENIE_PREC_EXACT) return train_ws16(*cfg, B, npl_of(*cfg), nullptr, exact).total;
    return exact;
}

int genie_train_pack_weights(const genie_cfg* cfg, const genie_weights* w, const genie_weights* w16,
                             const genie_weights* w16T, void* stream) {
    return genie_train_pack_weights_some(cfg, w, w16, w16T, nullptr, stream);
}

// select: NULL packs every Linear; else only those whose *_w member in it is non-NULL (the trainer's gradient table: a frozen
// weight has not moved, its copies are current)
int genie_train_pack_weights_some(const genie_cfg* cfg, const genie_weights* w, const genie_weights* w16,
                                  const genie_weights* w16T, const genie_weights* select, void* stream) {
    GENIE_CHECK_ARG(cfg && w && w16 && w16T, "genie_train_pack_weights: NULL argument");
    GENIE_CHECK_ARG(cfg->precision != GENIE_PREC_EXACT, "genie_train_pack_weights: exact precision has no 16-bit copies");
    const genie_cfg& c = *cfg;
    const int npl = npl_of(c), d = c.d_model, hid = c.hidden, V = c.factored_vocab * c.num_factored;
    hipStream_t st = (hipStream_t)stream;
    auto pack = [&](bool wanted, const float* src, const uint16_t* rowm, const uint16_t* tr, int out, int in) -> int {
        if (!wanted) return GENIE_OK;
        GENIE_CHECK_ARG(src && rowm && tr, "genie_train_pack_weights: missing pointer");
        GENIE_TRY(launch_cast16(npl, src, (uint16_t*)rowm, (size_t)out * in, st));
        return launch_cast_transpose16(npl, (float*)src, in, nullptr, nullptr, (uint16_t*)tr, out, in, st);
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const genie_layer_weights &a = w->layers_host[l], &b = w16->layers_host[l], &t = w16T->layers_host[l];
        const genie_layer_weights* s = select ? &select->layers_host[l] : nullptr;
        GENIE_TRY(pack(!s || s->spatial.qkv_w, a.spatial.qkv_w, b.spatial.qkv_w16, t.spatial.qkv_w16, 3 * d, d));
        GENIE_TRY(pack(!s || s->spatial.proj_w, a.spatial.proj_w, b.spatial.proj_w16, t.spatial.proj_w16, d, d));
        GENIE_TRY(pack(!s || s->temporal.qkv_w, a.temporal.qkv_w, b.temporal.qkv_w16, t.temporal.qkv_w16, 3 * d, d));
        GENIE_TRY(pack(!s || s->temporal.proj_w, a.temporal.proj_w, b.temporal.proj_w16, t.temporal.proj_w16, d, d));
        GENIE_TRY(pack(!s || s->fc1_w, a.fc1_w, b.fc1_w16, t.fc1_w16, hid, d));
        GENIE_TRY(pack(!s || s->fc2_w, a.fc2_w, b.fc2_w16, t.fc2_w16, d, hid));
    }
    return pack(!select || select->out_w, w->out_w, w16->out_w16, w16T->out_w16, V, d);
}

int genie_train_forward(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                        int B, float* acts, size_t acts_bytes, double* sums, void* stream) {
    return genie_train_forward_ex(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, nullptr, 0);
}

int genie_train_forward_cond(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                             int B, float* acts, size_t acts_bytes, double* sums, void* stream,
                             const genie_frame_cond* cond) {
    return genie_train_forward_ex(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, 0);
}

int genie_train_forward_ex(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                           int B, float* acts, size_t acts_bytes, double* sums, void* stream, const genie_frame_cond* cond,
                           int recompute) {
    return genie_train_forward_drop(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, recompute, nullptr);
}

// genie_train_forward_drop, and with obj != NULL (checked, not neutral) the general objective behind the same forward; with ds != NULL
// (checked, not neutral) the distillation loss there instead
static int train_forward_any(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                             int B, float* acts, size_t acts_bytes, double* sums, void* stream, const genie_frame_cond* cond,
                             int recompute, const genie_dropout* dr, const genie_objective* obj, const genie_distill* ds = nullptr) {
    GENIE_CHECK_ARG(drop_p_ok(dr), "genie_train_forward: dropout p = %g is not in [0, 1)", (double)dr->p);
    GENIE_TRY(check_mode(recompute, "genie_train_forward"));
    // argument errors (GENIE_E_ARG) are reported before geometry errors (GENIE_E_SHAPE), as they were before train_check
    // learnt to refuse a geometry that check_cfg admits
    GENIE_CHECK_ARG(cfg && wt && input_ids && labels && acts && sums, "genie_train_forward: NULL argument");
    GENIE_TRY(check_frame_cond(cond, "genie_train_forward"));
    GENIE_TRY(train_check(cfg, B));
    const genie_cfg& c = *cfg;
    EmbedAct ea;
    const EmbedAct* act = frame_act(cond, c.S, 0, c.T, ea);
    GENIE_TRY(need16(wt, c, "genie_train_forward"));
    const TrainActs a = train_acts(c, B, recompute);
    GENIE_CHECK_ARG(acts_bytes >= a.total, "genie_train_forward: activation buffer too small: %zu < %zu", acts_bytes, a.total);
    const int M = B * c.T * c.S, V = c.factored_vocab * c.num_factored;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)acts;
    if (ds) GENIE_TRY(distill_apart(ds->teacher_logits, (const float*)(base + a.logits), (size_t)M * V, sums, "genie_train_forward_distill"));
    if (c.precision == GENIE_PREC_EXACT) {
        ExactOps o{c, B, M, st, TrainWs{}, 0.0f, make_drop(dr)};
        return train_forward(o, wt, input_ids, labels, base, a, sums, act, obj, ds);
    }
    GENIE_CHECK_SHAPE(V >= c.d_model, "training step (16-bit): vocabulary rows %d < d_model %d", V, c.d_model);
    Ops16 o{c, B, M, st, TrainWs{}, 0.0f, npl_of(c), TrainWs16{}, (float*)(base + a.logits), make_drop(dr)};
    return train_forward(o, wt, input_ids, labels, base, a, sums, act, obj, ds);
}

int genie_train_forward_drop(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                             int B, float* acts, size_t acts_bytes, double* sums, void* stream, const genie_frame_cond* cond,
                             int recompute, const genie_dropout* dr) {
    return train_forward_any(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, recompute, dr, nullptr);
}

int genie_train_forward_obj(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                            int B, float* acts, size_t acts_bytes, double* sums, void* stream, const genie_frame_cond* cond,
                            int recompute, const genie_dropout* dr, const genie_objective* obj) {
    GENIE_TRY(objective_ok(obj, cfg ? cfg->T : (obj ? obj->n_frames : 0), "genie_train_forward_obj"));
    return train_forward_any(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, recompute, dr,
                             objective_neutral(obj) ? nullptr : obj);
}

int genie_train_forward_distill(const genie_cfg* cfg, const genie_weights* wt, const int64_t* input_ids, const int64_t* labels,
                                int B, float* acts, size_t acts_bytes, double* sums, void* stream, const genie_frame_cond* cond,
                                int recompute, const genie_dropout* dr, const genie_objective* obj, const genie_distill* ds) {
    GENIE_TRY(distill_ok(ds, ds ? ds->teacher_logits : nullptr, "genie_train_forward_distill"));
    if (distill_neutral(ds))
        return genie_train_forward_obj(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, recompute, dr, obj);
    GENIE_TRY(objective_ok(obj, cfg ? cfg->T : (obj ? obj->n_frames : 0), "genie_train_forward_distill"));
    return train_forward_any(cfg, wt, input_ids, labels, B, acts, acts_bytes, sums, stream, cond, recompute, dr,
                             objective_neutral(obj) ? nullptr : obj, ds);
}

int genie_train_backward_head(const genie_cfg* cfg, const genie_weights* wt, const genie_weights* wT,
                              const genie_weights* grads, int B, float* acts, void* workspace, size_t workspace_bytes,
                              int accumulate, void* stream) {
    return genie_train_backward_head_ex(cfg, wt, wT, grads, B, acts, workspace, workspace_bytes, accumulate, stream, 0);
}

int genie_train_backward_head_ex(const genie_cfg* cfg, const genie_weights* wt, const genie_weights* wT,
                                 const genie_weights* grads, int B, float* acts, void* workspace, size_t workspace_bytes,
                                 int accumulate, void* stream, int recompute) {
    GENIE_TRY(check_mode(recompute, "genie_train_backward_head"));
    GENIE_TRY(train_check(cfg, B));
    GENIE_CHECK_ARG(wt && grads && acts && workspace, "genie_train_backward_head: NULL argument");
    const genie_cfg& c = *cfg;
    const TrainWs w = train_ws(c, B, workspace);
    const TrainActs a = train_acts(c, B, recompute);
    const int M = B * c.T * c.S;
    const float beta = accumulate ? 1.0f : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    if (c.precision == GENIE_PREC_EXACT) {
        GENIE_CHECK_ARG(workspace_bytes >= w.total, "training workspace too small: %zu < %zu", workspace_bytes, w.total);
        ExactOps o{c, B, M, st, w, beta};
        return train_backward_head(o, wt, wT, grads, (char*)acts, a);
    }
    const TrainWs16 h = train_ws16(c, B, npl_of(c), workspace, w.total);
    GENIE_CHECK_ARG(workspace_bytes >= h.total, "training workspace too small: %zu < %zu", workspace_bytes, h.total);
    GENIE_TRY(need16(wT, c, "genie_train_backward_head (transposed copies)"));
    Ops16 o{c, B, M, st, w, beta, npl_of(c), h, nullptr};
    return train_backward_head(o, wt, wT, grads, (char*)acts, a);
}

int genie_train_backward_layer(const genie_cfg* cfg, const genie_weights* wt, const genie_weights* wT,
                               const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                               size_t workspace_bytes, int accumulate, void* stream) {
    return genie_train_backward_layer_ex(cfg, wt, wT, grads, layer, B, acts, workspace, workspace_bytes, accumulate, stream, 0);
}

int genie_train_backward_layer_ex(const genie_cfg* cfg, const genie_weights* wt, const genie_weights* wT,
                                  const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                                  size_t workspace_bytes, int accumulate, void* stream, int recompute) {
    return genie_train_backward_layer_drop(cfg, wt, wT, grads, layer, B, acts, workspace, workspace_bytes, accumulate, stream, recompute,
                                           nullptr);
}

int genie_train_backward_layer_drop(const genie_cfg* cfg, const genie_weights* wt, const genie_weights* wT,
                                    const genie_weights* grads, int layer, int B, float* acts, void* workspace,
                                    size_t workspace_bytes, int accumulate, void* stream, int recompute, const genie_dropout* dr) {
    GENIE_CHECK_ARG(drop_p_ok(dr), "genie_train_backward_layer: dropout p = %g is not in [0, 1)", (double)dr->p);
    GENIE_TRY(check_mode(recompute, "genie_train_backward_layer"));
    GENIE_TRY(train_check(cfg, B));
    GENIE_CHECK_ARG(wt && grads && acts && workspace, "genie_train_backward_layer: NULL argument");
    GENIE_CHECK_ARG(layer >= 0 && layer < cfg->num_layers, "genie_train_backward_layer: layer %d out of range", layer);
    const genie_cfg& c = *cfg;
    const TrainWs w = train_ws(c, B, workspace);
    const TrainActs a = train_acts(c, B, recompute);
    const int M = B * c.T * c.S;
    const float beta = accumulate ? 1.0f : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    if (c.precision == GENIE_PREC_EXACT) {
        GENIE_CHECK_ARG(workspace_bytes >= w.total, "training workspace too small: %zu < %zu", workspace_bytes, w.total);
        ExactOps o{c, B, M, st, w, beta, make_drop(dr)};
        return train_backward_layer(o, wt, wT, grads, layer, (char*)acts, a);
    }
    GENIE_TRY(need16(wT, c, "genie_train_backward_layer (transposed copies)"));
    const TrainWs16 h = train_ws16(c, B, npl_of(c), workspace, w.total);
    GENIE_CHECK_ARG(workspace_bytes >= h.total, "training workspace too small: %zu < %zu", workspace_bytes, h.total);
    Ops16 o{c, B, M, st, w, beta, npl_of(c), h, recompute ? w.d1 : nullptr, make_drop(dr)};
    return train_backward_layer(o, wt, wT, grads, layer, (char*)acts, a);
}

int genie_train_backward_embed(const genie_cfg* cfg, const genie_weights* grads, const int64_t* input_ids, int B,
                               void* workspace, size_t workspace_bytes, int accumulate, void* stream) {
    return genie_train_backward_embed_cond(cfg, grads, input_ids, B, workspace, workspace_bytes, accumulate, stream, nullptr,
                                           nullptr);
}

int genie_train_backward_embed_cond(const genie_cfg* cfg, const genie_weights* grads, const int64_t* input_ids, int B,
                                    void* workspace, size_t workspace_bytes, int accumulate, void* stream,
                                    float* d_table, const genie_frame_cond* cond) {
    GENIE_CHECK_ARG(cfg && grads && input_ids && workspace, "genie_train_backward_embed: NULL argument");
    GENIE_TRY(check_frame_cond(cond, "genie_train_backward_embed"));
    const bool act = cond && cond->n_actions > 0;
    GENIE_CHECK_ARG(!act || d_table, "genie_train_backward_embed: actions without d_table");
    GENIE_TRY(train_check(cfg, B));
    TrainWs w = train_ws(*cfg, B, workspace);
    GENIE_CHECK_ARG(workspace_bytes >= w.total, "training workspace too small: %zu < %zu", workspace_bytes, w.total);
    float* tables[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < cfg->num_factored && j < 4; ++j) tables[j] = (float*)grads->embed[j];
    const float beta = accumulate ? 1.0f : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    // NULL members are frozen tensors: launch_embed_bwd skips each one's part (all of them: nothing is enqueued)
    GENIE_TRY(launch_embed_bwd(*cfg, w.dx, input_ids, B, (float*)grads->pos_embed, (float*)grads->mask_embed, tables, beta,
                               w.colpart, st));
    if (!act) return GENIE_OK;
    // per-frame sums of dx in w.d1 ((M, d) floats, dead after the last layer's backward; B*T rows needed)
    return launch_action_embed_bwd(*cfg, w.dx, cond->ids, cond->n_actions, B, d_table, beta, w.d1, st);
}

int genie_temporal_attention_backward(const float* qkv, const float* qk, int64_t qk_ld, const float* d_out,
                                      float* d_qkv, int B, int T, int S, int d_model, int num_heads, int head_dim,
                                      float scale, void* stream) {
    GENIE_CHECK_ARG(qkv && qk && d_out && d_qkv && B > 0, "genie_temporal_attention_backward: NULL argument or B <= 0");
    GENIE_CHECK_ARG(T > 0 && S > 0 && d_model > 0 && num_heads > 0 && head_dim > 0,
                    "genie_temporal_attention_backward: T, S, d_model, num_heads, head_dim must be positive");
    GENIE_CHECK_SHAPE(T <= 64 && (T & (T - 1)) == 0, "genie_temporal_attention_backward: T=%d is not a power of two <= 64", T);
    GENIE_CHECK_SHAPE((long)head_dim * num_heads == d_model, "genie_temporal_attention_backward: head_dim %d * num_heads %d != d_model %d",
                      head_dim, num_heads, d_model);
    GENIE_CHECK_SHAPE(qk_ld == 2L * d_model || qk_ld == 3L * d_model,
                      "genie_temporal_attention_backward: qk_ld %ld is neither 2*d_model nor 3*d_model", (long)qk_ld);
    return launch_attn_temporal_bwd(qkv, qk, (long)qk_ld, d_out, d_qkv, B, T, S, d_model, num_heads, head_dim, scale,
                                    (hipStream_t)stream);
}

// the two scratch slots of spatial_attn_bwd behind one workspace pointer: byte offset of the second one (= the first one's size)
static size_t spatial_bwd_slot_bytes(int path, size_t n_frames, size_t S, size_t H) {
    size_t floats = 0;
    if (path == GENIE_SPATIAL_BWD_MATERIALISED) floats = n_frames * H * S * S;
    else if (path == GENIE_SPATIAL_BWD_BF16) floats = n_frames * H * S * 4;
    return (floats * 4 + 255) / 256 * 256;
}
static size_t spatial_bwd_bytes(int path, size_t n_frames, size_t S, size_t H) {
    return spatial_bwd_slot_bytes(path, n_frames, S, H) * (path == GENIE_SPATIAL_BWD_MATERIALISED ? 2 : 1);
}

size_t genie_spatial_attention_backward_workspace_bytes(int path, int n_frames, int S, int num_heads) {
    if (path < GENIE_SPATIAL_BWD_AUTO || path > GENIE_SPATIAL_BWD_BF16 || n_frames <= 0 || S <= 0 || num_heads <= 0) return 0;
    if (path == GENIE_SPATIAL_BWD_AUTO) path = GENIE_SPATIAL_BWD_MATERIALISED;
    return spatial_bwd_bytes(path, (size_t)n_frames, (size_t)S, (size_t)num_heads);
}

int genie_spatial_attention_backward(const float* qkv, const float* qk, int64_t qk_ld, const float* d_out, float* d_qkv,
                                     int n_frames, int S, int d_model, int num_heads, int head_dim, float scale, int path,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    GENIE_CHECK_ARG(qkv && qk && d_out && d_qkv && n_frames > 0, "genie_spatial_attention_backward: NULL argument or n_frames <= 0");
    GENIE_CHECK_ARG(S > 0 && d_model > 0 && num_heads > 0 && head_dim > 0,
                    "genie_spatial_attention_backward: S, d_model, num_heads, head_dim must be positive");
    GENIE_CHECK_ARG(path >= GENIE_SPATIAL_BWD_AUTO && path <= GENIE_SPATIAL_BWD_BF16,
                    "genie_spatial_attention_backward: path %d is not a GENIE_SPATIAL_BWD_* value", path);
    GENIE_CHECK_SHAPE(S % 16 == 0 && head_dim % 16 == 0, "genie_spatial_attention_backward: S=%d and head_dim=%d must be multiples of 16",
                      S, head_dim);
    GENIE_CHECK_SHAPE((long)head_dim * num_heads == d_model, "genie_spatial_attention_backward: head_dim %d * num_heads %d != d_model %d",
                      head_dim, num_heads, d_model);
    GENIE_CHECK_SHAPE(qk_ld == 2L * d_model || qk_ld == 3L * d_model,
                      "genie_spatial_attention_backward: qk_ld %ld is neither 2*d_model nor 3*d_model", (long)qk_ld);
    const bool takes = path == GENIE_SPATIAL_BWD_FUSED  ? attn_spatial_bwd_fused_takes(S, head_dim)
                       : path == GENIE_SPATIAL_BWD_BF16 ? attn_spatial_bwd_bf16_takes(S, head_dim, (long)qk_ld, d_model)
                                                        : true;
    if (!takes) {
        set_error("genie_spatial_attention_backward: path %d does not take S=%d, head_dim=%d (S = 256 and head_dim 32 / 64)", path, S,
                  head_dim);
        return GENIE_E_UNSUPPORTED;
    }
    // what AUTO will run decides what it needs
    const int taken = path != GENIE_SPATIAL_BWD_AUTO               ? path
                      : attn_spatial_bwd_fused_takes(S, head_dim) ? GENIE_SPATIAL_BWD_FUSED
                                                                  : GENIE_SPATIAL_BWD_MATERIALISED;
    const size_t slot = spatial_bwd_slot_bytes(taken, (size_t)n_frames, (size_t)S, (size_t)num_heads);
    const size_t need = spatial_bwd_bytes(taken, (size_t)n_frames, (size_t)S, (size_t)num_heads);
    GENIE_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
                    "genie_spatial_attention_backward: workspace too small or NULL: %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    float* p = need ? (float*)workspace : nullptr;
    float* dp = need ? (float*)((char*)workspace + slot) : nullptr;
    return spatial_attn_bwd(qkv, QkSrc{qk, (long)qk_ld}, d_out, d_qkv, p, dp, n_frames, S, d_model, num_heads, head_dim, scale, path,
                            (hipStream_t)stream);
}

int genie_qk_norm_forward(const float* qkv, float* qkn, const float* norm_w, const float* norm_b, int64_t rows, int num_heads,
                          int head_dim, void* stream) {
    GENIE_CHECK_ARG(qkv && qkn && norm_w && norm_b && rows > 0, "genie_qk_norm_forward: NULL argument or rows <= 0");
    GENIE_CHECK_ARG(num_heads > 0 && head_dim > 0, "genie_qk_norm_forward: num_heads and head_dim must be positive");
    return launch_qk_norm_fwd(qkv, qkn, norm_w, norm_b, (long)rows, num_heads, head_dim, num_heads * head_dim, (hipStream_t)stream);
}

size_t genie_qk_norm_backward_scratch_bytes(int head_dim) { return qk_norm_bwd_scratch_floats(head_dim) * sizeof(float); }

int genie_qk_norm_backward(const float* qkv, float* d_qkv, const float* norm_w, float* d_norm_w, float* d_norm_b, int64_t rows,
                           int num_heads, int head_dim, int accumulate, void* scratch, size_t scratch_bytes, void* stream) {
    GENIE_CHECK_ARG(qkv && d_qkv && norm_w && rows > 0, "genie_qk_norm_backward: NULL argument or rows <= 0");
    GENIE_CHECK_ARG(num_heads > 0 && head_dim > 0, "genie_qk_norm_backward: num_heads and head_dim must be positive");
    const size_t need = (d_norm_w || d_norm_b) ? genie_qk_norm_backward_scratch_bytes(head_dim) : 0;
    GENIE_CHECK_ARG(need == 0 || (scratch && scratch_bytes >= need), "genie_qk_norm_backward: scratch too small or NULL: %zu < %zu",
                    scratch ? scratch_bytes : (size_t)0, need);
    return launch_qk_norm_bwd(qkv, d_qkv, norm_w, d_norm_w, d_norm_b, (long)rows, num_heads, head_dim, num_heads * head_dim,
                              accumulate ? 1.0f : 0.0f, (float*)scratch, (hipStream_t)stream);
}

int genie_dropout_layout(size_t* out_host, int n) {
    const size_t v[4] = {sizeof(genie_dropout), offsetof(genie_dropout, p), offsetof(genie_dropout, call), offsetof(genie_dropout, seed)};
    for (int i = 0; i < n && i < 4 && out_host; ++i) out_host[i] = v[i];
    return 4;
}

int genie_objective_layout(size_t* out_host, int n) {
    const size_t v[6] = {sizeof(genie_objective), offsetof(genie_objective, label_smoothing), offsetof(genie_objective, z_loss),
                         offsetof(genie_objective, n_frames), offsetof(genie_objective, reserved), offsetof(genie_objective, frame_weight)};
    for (int i = 0; i < n && i < 6 && out_host; ++i) out_host[i] = v[i];
    return 6;
}

int genie_ce_objective(float* logits, const int64_t* ids, const int64_t* labels, int n_clips, int T, int S, int vf, int nfac,
                       int64_t mask_id, const genie_objective* obj, double* sums, void* stream) {
    GENIE_TRY(objective_ok(obj, T, "genie_ce_objective"));
    GENIE_TRY(loss_call_ok(logits, ids, labels, sums, n_clips, T, S, vf, nfac, "genie_ce_objective"));
    if (!obj)   // the neutral step's kernels take the geometry from a genie_cfg
        GENIE_CHECK_ARG(mask_id >= INT32_MIN && mask_id <= INT32_MAX, "genie_ce_objective: mask_id %lld beyond int32 without an objective",
                        (long long)mask_id);
    return launch_train_loss("genie_ce_objective", logits, ids, labels, n_clips, T, S, vf, nfac, mask_id, obj, nullptr, nullptr, sums,
                             (hipStream_t)stream);
}

int genie_distill_layout(size_t* out_host, int n) {
    const size_t v[4] = {sizeof(genie_distill), offsetof(genie_distill, alpha), offsetof(genie_distill, temperature),
                         offsetof(genie_distill, teacher_logits)};
    for (int i = 0; i < n && i < 4 && out_host; ++i) out_host[i] = v[i];
    return 4;
}

int genie_ce_distill(float* logits, const float* teacher_logits, const int64_t* ids, const int64_t* labels, int n_clips, int T, int S,
                     int vf, int nfac, int64_t mask_id, const genie_objective* obj, const genie_distill* ds, double* sums, void* stream) {
    GENIE_TRY(distill_ok(ds, teacher_logits, "genie_ce_distill"));
    if (distill_neutral(ds)) return genie_ce_objective(logits, ids, labels, n_clips, T, S, vf, nfac, mask_id, obj, sums, stream);
    GENIE_TRY(objective_ok(obj, T, "genie_ce_distill"));
    GENIE_TRY(loss_call_ok(logits, ids, labels, sums, n_clips, T, S, vf, nfac, "genie_ce_distill"));
    GENIE_TRY(distill_apart(teacher_logits, logits, (size_t)n_clips * T * S * vf * nfac, sums, "genie_ce_distill"));
    return launch_train_loss("genie_ce_distill", logits, ids, labels, n_clips, T, S, vf, nfac, mask_id, obj, ds, teacher_logits, sums,
                             (hipStream_t)stream);
}

int genie_dropout_mask(const genie_dropout* dr, int layer, int site, int64_t n, uint8_t* keep, void* stream) {
    GENIE_CHECK_ARG(dr != nullptr, "genie_dropout_mask: NULL genie_dropout");
    GENIE_CHECK_ARG(drop_p_ok(dr), "genie_dropout_mask: dropout p = %g is not in [0, 1)", (double)dr->p);
    GENIE_CHECK_ARG(layer >= 0 && (site == 0 || site == 1) && n >= 0 && (keep || !n), "genie_dropout_mask: layer %d, site %d, n %lld or NULL keep",
                    layer, site, (long long)n);
    return launch_dropout_mask(keep, (size_t)n, Drop{true, 1.0f, drop_key(*dr)}.key(layer, site), (hipStream_t)stream);
}

int genie_sumsq(const float* x, size_t n, double* out, double* scratch, void* stream) {
    GENIE_CHECK_ARG((x || !n) && out && scratch, "genie_sumsq: NULL argument");
    return launch_sumsq(x, n, out, scratch, (hipStream_t)stream);
}

int genie_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_mult, const double* grad_sumsq,
                     float max_grad_norm, void* stream) {
    GENIE_CHECK_ARG((params && grads && exp_avg && exp_avg_sq) || !n, "genie_adamw_step: NULL argument");
    GENIE_CHECK_ARG(step >= 1, "genie_adamw_step: step counts from 1");
    return launch_adamw(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_mult,
                        grad_sumsq, max_grad_norm, (hipStream_t)stream);
}

static bool omd_ok(float omd) { return omd >= 0.0f && omd <= 1.0f; }   // false for NaN

int genie_adamw_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, float grad_mult, const double* grad_sumsq,
                         float max_grad_norm, float ema_one_minus_decay, void* stream) {
    GENIE_CHECK_ARG((params && grads && exp_avg && exp_avg_sq && ema) || !n, "genie_adamw_ema_step: NULL argument");
    GENIE_CHECK_ARG(step >= 1, "genie_adamw_ema_step: step counts from 1");
    GENIE_CHECK_ARG(omd_ok(ema_one_minus_decay), "genie_adamw_ema_step: ema_one_minus_decay %g is not in [0, 1]", (double)ema_one_minus_decay);
    return launch_adamw_ema(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, weight_decay, step, grad_mult,
                            grad_sumsq, max_grad_norm, ema_one_minus_decay, (hipStream_t)stream);
}

int genie_ema_update(float* ema, const float* params, size_t n, float one_minus_decay, void* stream) {
    GENIE_CHECK_ARG((ema && params) || !n, "genie_ema_update: NULL argument");
    GENIE_CHECK_ARG(omd_ok(one_minus_decay), "genie_ema_update: one_minus_decay %g is not in [0, 1]", (double)one_minus_decay);
    return launch_ema_update(ema, params, n, one_minus_decay, (hipStream_t)stream);
}

int genie_swap_f32(float* a, float* b, size_t n, void* stream) {
    GENIE_CHECK_ARG((a && b) || !n, "genie_swap_f32: NULL argument");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    GENIE_CHECK_ARG(!n || ua + 4 * n <= ub || ub + 4 * n <= ua, "genie_swap_f32: the two ranges overlap");
    return launch_swap_f32(a, b, n, (hipStream_t)stream);
}

int genie_lora_layout(size_t* out_host, int n) {
    const size_t v[12] = {sizeof(genie_lora_item), offsetof(genie_lora_item, w), offsetof(genie_lora_item, w0),
                          offsetof(genie_lora_item, a), offsetof(genie_lora_item, b), offsetof(genie_lora_item, dw),
                          offsetof(genie_lora_item, da), offsetof(genie_lora_item, db), offsetof(genie_lora_item, out),
                          offsetof(genie_lora_item, in), offsetof(genie_lora_item, rank), offsetof(genie_lora_item, scale)};
    for (int i = 0; i < n && i < 12 && out_host; ++i) out_host[i] = v[i];
    return 12;
}

static bool lora_overlap(const void* p, size_t np, const void* q, size_t nq) {   // ranges of np / nq floats
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + 4 * nq && b < a + 4 * np;
}
// what genie_lora_merge (project = false) or genie_lora_project accepts, on the host alone
static int lora_ok(const genie_lora_item* items, int n, bool project, const char* where) {
    GENIE_CHECK_ARG(items != nullptr, "%s: NULL items", where);
    GENIE_CHECK_ARG(n >= 1 && n <= GENIE_LORA_MAX_ITEMS, "%s: n = %d is not in 1 .. %d", where, n, GENIE_LORA_MAX_ITEMS);
    for (int e = 0; e < n; ++e) {
        const genie_lora_item& it = items[e];
        GENIE_CHECK_ARG(it.rank >= 1 && it.rank <= GENIE_LORA_MAX_RANK, "%s: item %d: rank %d is not in 1 .. %d", where, e, it.rank,
                        GENIE_LORA_MAX_RANK);
        GENIE_CHECK_ARG(it.out >= 1, "%s: item %d: out = %d", where, e, it.out);
        GENIE_CHECK_ARG(it.in >= 16 && it.in % 16 == 0, "%s: item %d: in = %d is not a positive multiple of 16", where, e, it.in);
        GENIE_CHECK_ARG(std::isfinite(it.scale), "%s: item %d: the scale is not finite", where, e);
        const size_t nw = (size_t)it.out * it.in, na = (size_t)it.rank * it.in, nb = (size_t)it.out * it.rank;
        GENIE_CHECK_ARG(it.a && it.b, "%s: item %d: NULL a or b", where, e);
        if (!project) {
            GENIE_CHECK_ARG(it.w && it.w0, "%s: item %d: NULL w or w0", where, e);
            GENIE_CHECK_ARG(((uintptr_t)it.w | (uintptr_t)it.w0 | (uintptr_t)it.a) % 16 == 0, "%s: item %d: w, w0 and a must be 16-byte aligned",
                            where, e);
            GENIE_CHECK_ARG(it.w == it.w0 || !lora_overlap(it.w, nw, it.w0, nw), "%s: item %d: w overlaps w0 without being w0", where, e);
            GENIE_CHECK_ARG(!lora_overlap(it.a, na, it.w, nw) && !lora_overlap(it.b, nb, it.w, nw), "%s: item %d: a or b overlaps the output w",
                            where, e);
        } else {
            GENIE_CHECK_ARG(it.dw && it.da && it.db, "%s: item %d: NULL dw, da or db", where, e);
            GENIE_CHECK_ARG(((uintptr_t)it.dw | (uintptr_t)it.da) % 16 == 0, "%s: item %d: dw and da must be 16-byte aligned", where, e);
            GENIE_CHECK_ARG(!lora_overlap(it.a, na, it.da, na) && !lora_overlap(it.a, na, it.db, nb) && !lora_overlap(it.b, nb, it.da, na) &&
                                !lora_overlap(it.b, nb, it.db, nb),
                            "%s: item %d: a or b overlaps an output (da, db)", where, e);
            GENIE_CHECK_ARG(!lora_overlap(it.dw, nw, it.da, na) && !lora_overlap(it.dw, nw, it.db, nb) && !lora_overlap(it.da, na, it.db, nb),
                            "%s: item %d: dw, da and db overlap", where, e);
        }
    }
    return GENIE_OK;
}

int genie_lora_merge(const genie_lora_item* items, int n, void* stream) {
    GENIE_TRY(lora_ok(items, n, false, "genie_lora_merge"));
    LoraTable tb;
    size_t floats;
    GENIE_CHECK_ARG(lora_table(items, n, tb, floats), "genie_lora_merge: the table is beyond 2^31 tiles");
    return launch_lora_merge(tb, (hipStream_t)stream);
}

size_t genie_lora_project_scratch_bytes(const genie_lora_item* items, int n) {
    if (lora_ok(items, n, true, "genie_lora_project_scratch_bytes") != GENIE_OK) return 0;
    LoraTable tb;
    size_t floats;
    if (!lora_table(items, n, tb, floats)) {
        set_error("genie_lora_project_scratch_bytes: the table is beyond 2^31 tiles");
        return 0;
    }
    return floats * sizeof(float);
}

int genie_lora_project(const genie_lora_item* items, int n, int accumulate, void* scratch, size_t scratch_bytes, void* stream) {
    GENIE_TRY(lora_ok(items, n, true, "genie_lora_project"));
    LoraTable tb;
    size_t floats;
    GENIE_CHECK_ARG(lora_table(items, n, tb, floats), "genie_lora_project: the table is beyond 2^31 tiles");
    GENIE_CHECK_ARG(scratch != nullptr && (uintptr_t)scratch % 16 == 0, "genie_lora_project: NULL or misaligned scratch");
    GENIE_CHECK_ARG(scratch_bytes >= floats * sizeof(float), "genie_lora_project: scratch of %zu bytes, %zu needed", scratch_bytes,
                    floats * sizeof(float));
    for (int e = 0; e < n; ++e) {
        const genie_lora_item& it = items[e];
        GENIE_CHECK_ARG(!lora_overlap(scratch, floats, it.dw, (size_t)it.out * it.in) && !lora_overlap(scratch, floats, it.a, (size_t)it.rank * it.in) &&
                            !lora_overlap(scratch, floats, it.b, (size_t)it.out * it.rank) &&
                            !lora_overlap(scratch, floats, it.da, (size_t)it.rank * it.in) &&
                            !lora_overlap(scratch, floats, it.db, (size_t)it.out * it.rank),
                        "genie_lora_project: item %d: scratch overlaps one of its buffers", e);
    }
    tb.scratch = (float*)scratch;
    return launch_lora_project(tb, accumulate ? 1 : 0, (hipStream_t)stream);
}

int genie_muon_layout(size_t* out_host, int n) {
    typedef genie_muon_item I;
    typedef genie_muon_settings S;
    const size_t v[23] = {sizeof(I), offsetof(I, param), offsetof(I, grad), offsetof(I, momentum), offsetof(I, ema), offsetof(I, rows),
                          offsetof(I, cols), offsetof(I, lr), offsetof(I, weight_decay),
                          sizeof(S), offsetof(S, momentum), offsetof(S, a), offsetof(S, b), offsetof(S, c), offsetof(S, eps),
                          offsetof(S, grad_mult), offsetof(S, max_grad_norm), offsetof(S, ema_one_minus_decay), offsetof(S, nesterov),
                          offsetof(S, ns_steps), offsetof(S, adjust), offsetof(S, reserved), offsetof(S, grad_sumsq)};
    for (int i = 0; i < n && i < 23 && out_host; ++i) out_host[i] = v[i];
    return 23;
}

// what the shapes of a Muon table must satisfy (all of it that genie_muon_workspace_bytes needs), on the host alone
static int muon_shapes_ok(const genie_muon_item* items, int n, const char* where) {
    GENIE_CHECK_ARG(items != nullptr, "%s: NULL items", where);
    GENIE_CHECK_ARG(n >= 1 && n <= GENIE_MUON_MAX_ITEMS, "%s: n = %d is not in 1 .. %d", where, n, GENIE_MUON_MAX_ITEMS);
    for (int e = 0; e < n; ++e) {
        const genie_muon_item& it = items[e];
        GENIE_CHECK_ARG(it.rows >= 16 && it.rows % 16 == 0 && it.cols >= 16 && it.cols % 16 == 0,
                        "%s: item %d: (rows, cols) = (%d, %d) are not positive multiples of 16", where, e, it.rows, it.cols);
        GENIE_CHECK_ARG((size_t)it.rows * it.cols <= ((size_t)1 << 30), "%s: item %d: more than 2^30 elements", where, e);
    }
    return GENIE_OK;
}
static int muon_steps_ok(int steps, float a, float b, float c, float eps, const char* where) {
    GENIE_CHECK_ARG(steps >= 0 && steps < 100, "%s: ns_steps = %d is not in 0 .. 99", where, steps);
    GENIE_CHECK_ARG(std::isfinite(a) && std::isfinite(b) && std::isfinite(c) && std::isfinite(eps), "%s: a, b, c or eps is not finite", where);
    return GENIE_OK;
}
static int muon_ws_ok(const MuonPlan& pl, const void* ws, size_t bytes, const char* where) {
    GENIE_CHECK_ARG(ws != nullptr && (uintptr_t)ws % 16 == 0, "%s: NULL or misaligned workspace", where);
    GENIE_CHECK_ARG(bytes >= pl.total_floats * sizeof(float), "%s: workspace of %zu bytes, %zu needed", where, bytes,
                    pl.total_floats * sizeof(float));
    return GENIE_OK;
}

size_t genie_muon_workspace_bytes(const genie_muon_item* items, int n) {
    if (muon_shapes_ok(items, n, "genie_muon_workspace_bytes") != GENIE_OK) return 0;
    MuonPlan pl;
    if (!muon_plan(items, n, pl)) {
        set_error("genie_muon_workspace_bytes: the table is beyond 2^40 elements");
        return 0;
    }
    return pl.total_floats * sizeof(float);
}

int genie_muon_step(const genie_muon_item* items, int n, const genie_muon_settings* s, void* workspace, size_t workspace_bytes,
                    void* stream) {
    const char* where = "genie_muon_step";
    GENIE_TRY(muon_shapes_ok(items, n, where));
    GENIE_CHECK_ARG(s != nullptr, "%s: NULL settings", where);
    GENIE_TRY(muon_steps_ok(s->ns_steps, s->a, s->b, s->c, s->eps, where));
    GENIE_CHECK_ARG(std::isfinite(s->momentum) && std::isfinite(s->grad_mult) && std::isfinite(s->max_grad_norm),
                    "%s: momentum, grad_mult or max_grad_norm is not finite", where);
    GENIE_CHECK_ARG(s->adjust == GENIE_MUON_ADJUST_ORIGINAL || s->adjust == GENIE_MUON_ADJUST_MATCH_RMS_ADAMW, "%s: adjust = %d", where,
                    s->adjust);
    GENIE_CHECK_ARG(s->grad_sumsq == nullptr || (uintptr_t)s->grad_sumsq % 8 == 0, "%s: misaligned grad_sumsq", where);
    bool any_ema = false;
    for (int e = 0; e < n; ++e) {
        const genie_muon_item& it = items[e];
        GENIE_CHECK_ARG(it.param && it.grad && it.momentum, "%s: item %d: NULL param, grad or momentum", where, e);
        GENIE_CHECK_ARG(((uintptr_t)it.param | (uintptr_t)it.grad | (uintptr_t)it.momentum | (uintptr_t)it.ema) % 16 == 0,
                        "%s: item %d: param, grad, momentum and ema must be 16-byte aligned", where, e);
        GENIE_CHECK_ARG(std::isfinite(it.lr) && std::isfinite(it.weight_decay), "%s: item %d: lr or weight_decay is not finite", where, e);
        any_ema = any_ema || it.ema != nullptr;
    }
    GENIE_CHECK_ARG(!any_ema || (s->ema_one_minus_decay >= 0.f && s->ema_one_minus_decay <= 1.f),
                    "%s: ema_one_minus_decay is not in [0, 1]", where);
    MuonPlan pl;
    GENIE_CHECK_ARG(muon_plan(items, n, pl), "%s: the table is beyond 2^40 elements", where);
    GENIE_TRY(muon_ws_ok(pl, workspace, workspace_bytes, where));
    return launch_muon_step(items, pl, *s, (float*)workspace, (hipStream_t)stream);
}

int genie_newton_schulz(const float* in, float* out, int rows, int cols, int batch, int steps, float a, float b, float c, float eps,
                        void* workspace, size_t workspace_bytes, void* stream) {
    const char* where = "genie_newton_schulz";
    GENIE_CHECK_ARG(in && out, "%s: NULL in or out", where);
    GENIE_CHECK_ARG(batch >= 1 && batch <= GENIE_MUON_MAX_ITEMS, "%s: batch = %d is not in 1 .. %d", where, batch, GENIE_MUON_MAX_ITEMS);
    genie_muon_item items[GENIE_MUON_MAX_ITEMS] = {};
    for (int e = 0; e < batch; ++e) items[e].rows = rows, items[e].cols = cols;
    GENIE_TRY(muon_shapes_ok(items, batch, where));
    GENIE_TRY(muon_steps_ok(steps, a, b, c, eps, where));
    GENIE_CHECK_ARG(((uintptr_t)in | (uintptr_t)out) % 16 == 0, "%s: in and out must be 16-byte aligned", where);
    const size_t nall = (size_t)batch * rows * cols;
    GENIE_CHECK_ARG(in == out || !lora_overlap(in, nall, out, nall), "%s: in overlaps out without being out", where);
    MuonPlan pl;
    GENIE_CHECK_ARG(muon_plan(items, batch, pl), "%s: the batch is beyond 2^40 elements", where);
    GENIE_TRY(muon_ws_ok(pl, workspace, workspace_bytes, where));
    GENIE_CHECK_ARG(!lora_overlap(workspace, pl.total_floats, in, nall) && !lora_overlap(workspace, pl.total_floats, out, nall),
                    "%s: the workspace overlaps in or out", where);
    return launch_newton_schulz(in, out, rows, cols, batch, steps, a, b, c, eps, pl, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
