// The layer drivers: everything that takes a BlockPass.  Host code only -- each function decides which launch comes next.
//   st_block_exact                 the STBlock in f32 (attention_block x 2 + MLP)
//   st_block16 / prepare16         the STBlock on 16-bit Linear operands, stated once for GENIE_PREC_BF16 (one bf16 plane) and
//                                  GENIE_PREC_F16X3 (f16 split planes); what differs by precision is struct Backend16 and the
//                                  `if constexpr` steps of block16
//   readout                        out_x_proj behind the last block, all three precisions
//   temporal_attention             the temporal attention dispatch behind the qkv GEMM, shared by all of them
#include "common.hpp"
#include "kernels.hpp"

namespace genie {

int temporal_attention(const genie_cfg& c, const genie_attn_weights& aw, const BlockPass& p, const TemporalQkv& tq, float* out,
                       uint16_t* out16, size_t plane, bool in16, Workspace& w, int B, hipStream_t st) {
    const int d = c.d_model, H = c.num_heads, Dh = c.head_dim;
    const float* nw = c.qk_norm ? aw.norm_w : nullptr;
    const float* nb = c.qk_norm ? aw.norm_b : nullptr;
    if (p.is_decode()) {  // the GEMM filled cache slot frame_t: attend slots 0..frame_t
        if (p.is_fanout())  // ... slots below fan_P0 from the parent's clip of the trunk, the rest from the branch slice
            return launch_attn_temporal_single_fanout(p.cache, out, B, p.frame_T, c.S, p.frame_t, d, H, Dh, c.attn_scale, nw, nb, st, out16,
                                                      plane, in16, FanSplit<true>{p.trunk, p.model_T, p.fan_P0, p.fan_K});
        return launch_attn_temporal_single(p.cache, out, B, p.frame_T, c.S, p.frame_t, d, H, Dh, c.attn_scale, nw, nb, st, out16, plane,
                                           in16);
    }
    const float* qkv = tq.base;
    float* tmp = out16 ? w.logits : out;  // where a kernel without a 16-bit epilogue writes its f32 rows
    if (p.reads_cache()) {
        const int rc = launch_attn_temporal_prefix(qkv, p.cache, out, B, c.T, c.S, d, H, Dh, c.attn_scale, nw, nb, st, out16, plane,
                                                   p.tshift, in16);
        if (rc != GENIE_E_UNSUPPORTED || !out16 || in16) return rc;
        GENIE_TRY(launch_attn_temporal_prefix(qkv, p.cache, tmp, B, c.T, c.S, d, H, Dh, c.attn_scale, nw, nb, st, nullptr, 0, p.tshift));
    } else {
        const int Tq = p.tq_stride(c.T);
        const int rc = launch_attn_temporal_f32_mfma(qkv, out, B, c.T, c.S, d, H, Dh, c.attn_scale, nw, nb, st, out16, plane, Tq, in16);
        if (rc != GENIE_E_UNSUPPORTED || in16) return rc;
        if (Tq != c.T && B > 1) {  // no MFMA instantiation for this geometry, and the generic kernel reads dense clips only
            set_error("strided temporal qkv needs the MFMA temporal kernel (8 <= frames <= 16)");
            return out16 ? GENIE_E_ARG : GENIE_E_UNSUPPORTED;  // (the codes the 16-bit drivers and the exact one have always returned here)
        }
        GENIE_TRY(launch_attn_generic(qkv, tmp, c.T, (long)B * c.S, c.S, (long)c.T * c.S, 1, c.S, d, H, Dh, c.attn_scale, 1, nw, nb, st));
    }
    return out16 ? launch_to_operand16(tmp, out16, plane, (size_t)B * c.T * c.S * d, st) : GENIE_OK;
}

// ---- GENIE_PREC_EXACT ----------------------------------------------------------------------------
// one SelfAttention + residual: x += proj(attn(qkv(u)))  (attention.py:36-61, st_transformer.py:74,78)
static int attention_block(const genie_cfg& c, const genie_attn_weights& aw, const float* u, float* x, Workspace& w, const BlockPass& p,
                           int B, bool temporal, hipStream_t st) {
    const int d = c.d_model, M = B * c.T * c.S;
    float* ao = (float*)w.xn;  // u may alias w.xn: it is dead once qkv is computed
    const float* bias = c.qkv_bias ? aw.qkv_b : nullptr;
    if (temporal) {
        const TemporalQkv tq = temporal_qkv_target(c, p, (float*)w.big, B);
        GENIE_TRY(launch_gemm_f32(u, d, tq.strideA, aw.qkv_w, d, 0, bias, tq.base + tq.off, 3 * d, tq.strideC, tq.rows, 3 * d, d,
                                  tq.batch, 0, 1.0f, st));
        if (p.stop_after_tqkv) return GENIE_OK;
        GENIE_TRY(temporal_attention(c, aw, p, tq, ao, nullptr, 0, false, w, B, st));
    } else {
        float* qkv = (float*)w.big;
        const float* nw = c.qk_norm ? aw.norm_w : nullptr;
        const float* nb = c.qk_norm ? aw.norm_b : nullptr;
        GENIE_TRY(launch_gemm_f32(u, d, 0, aw.qkv_w, d, 0, bias, qkv, 3 * d, 0, M, 3 * d, d, 1, 0, 1.0f, st));
        int rc = launch_attn_spatial_f32_mfma(qkv, ao, c.S, (long)B * c.T, d, c.num_heads, c.head_dim, c.attn_scale, nw, nb, st);
        if (rc == GENIE_E_UNSUPPORTED)  // no MFMA instantiation for this geometry: generic kernel
            rc = launch_attn_generic(qkv, ao, c.S, (long)B * c.T, 1, c.S, 0, 1, d, c.num_heads, c.head_dim, c.attn_scale, 0, nw, nb, st);
        GENIE_TRY(rc);
    }
    return launch_gemm_f32(ao, d, 0, aw.proj_w, d, 0, c.proj_bias ? aw.proj_b : nullptr, x, d, 0, M, d, d, 1, GEMM_ACCUM, 1.0f, st);
}

int st_block_exact(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, int B, hipStream_t st) {
    const int d = c.d_model, M = B * c.T * c.S;
    float* xn = (float*)w.xn;
    // spatial: x += SpAttn(norm1(x))  (st_transformer.py:73-74)
    const float* u = x;
    if (!c.qk_norm) {
        GENIE_TRY(launch_layer_norm(x, lw.norm1_w, lw.norm1_b, xn, M, d, 1e-5f, st));
        u = xn;
    }
    GENIE_TRY(attention_block(c, lw.spatial, u, x, w, p, B, false, st));
    // temporal: x += TmpAttn(x, causal), no pre-norm  (st_transformer.py:77-78)
    GENIE_TRY(attention_block(c, lw.temporal, x, x, w, p, B, true, st));
    if (p.stop_after_tqkv) return GENIE_OK;
    // MLP: x += fc2(gelu(fc1(norm2(x))))  (st_transformer.py:81, 16-25)
    u = x;
    if (!c.qk_norm) {
        GENIE_TRY(launch_layer_norm(x, lw.norm2_w, lw.norm2_b, xn, M, d, 1e-5f, st));
        u = xn;
    }
    float* hid = (float*)w.big;
    GENIE_TRY(launch_gemm_f32(u, d, 0, lw.fc1_w, d, 0, c.mlp_bias ? lw.fc1_b : nullptr, hid, c.hidden, 0, M, c.hidden,
                              d, 1, GEMM_GELU, 1.0f, st));
    GENIE_TRY(launch_gemm_f32(hid, c.hidden, 0, lw.fc2_w, c.hidden, 0, c.mlp_bias ? lw.fc2_b : nullptr, x, d, 0, M, d,
                              c.hidden, 1, GEMM_ACCUM, 1.0f, st));
    return GENIE_OK;
}

// ---- GENIE_PREC_BF16 / GENIE_PREC_F16X3 -----------------------------------------------------------
// bf16 precision contract (mirrored by oracle.genie_oracle.BF16_MFMA):
//   * every nn.Linear operand is bf16 (weights packed once; activations rounded by their producer)
//   * accumulation, bias, GELU, LayerNorm and the residual stream are f32
//   * the spatial attention runs on the 16-bit operand planes its qkv GEMM writes, or from an f32 qkv on the f32-MFMA kernels of the exact
//     path; its output is rounded to bf16 for the out-projection.
// f16x3: every Linear runs on the f16 matrix cores with split operands a = hi + lo * 2^-11 (3 MFMAs per K-step); everything else is the
//   exact path: f32 qkv -> f32-MFMA attention kernels -> outputs re-split for the next Linear.

// A 16-bit operand: NPL planes of the same shape, `plane` elements apart (0: one bf16 plane)
struct In16 {
    const uint16_t* p;
    long plane;
};
struct Out16 {
    uint16_t* p = nullptr;
    long plane = 0;
    operator In16() const { return {p, plane}; }
};
// One Linear of the block: packed weight, bias (NULL when the config has none), shape, and G16X_WIDEW when the f16x3 hi plane reaches
// |w| >= 32 (the `w16_wide` flags of genie_hip.h): that Linear stays off the 2^11-scaling kernel
struct Lin16 {
    In16 w;
    const float* bias;
    int N, K, wide;
};

// What the precision decides, for one block call.
template <int NPL>
struct Backend16 {
    static constexpr bool BF16 = NPL == 1;
    static constexpr const char* kNeedWeights = BF16 ? "bf16 precision needs packed bf16 weights (genie_pack_bf16)"
                                                          : "f16x3 precision needs split-f16 weights (genie_pack_split_f16)";
    const int M, d;
    hipStream_t st;
    // where the operands live                           bf16           f16x3
    Out16 x16;        // x in operand form                  w.xn           w.xn,  planes M*d apart
    Out16 a16;        // LayerNorm, then attention output   w.xn + M*d     w.aux, planes M*d apart
    Out16 h16;        // MLP hidden                         w.big          w.big, planes M*hidden apart
    float* qkv;       // f32 qkv                            w.big          w.big
    uint16_t* qkv16;  // ... or the spatial attention's 3 * NPL operand planes of M*d values (gemm16_pp with G16X_QKV): w.big
    Lin16 qkv_s, proj_s, qkv_t, proj_t, fc1, fc2;   // the six Linears; weight planes 0 / N*K apart, wide always 0 in bf16

    Backend16(const genie_cfg& c, const genie_layer_weights& lw, Workspace& w, int M_, hipStream_t st_) : M(M_), d(c.d_model), st(st_) {
        const int hid = c.hidden;
        const long pd = BF16 ? 0 : (long)M * d;
        x16 = {(uint16_t*)w.xn, pd};
        a16 = {BF16 ? (uint16_t*)w.xn + (size_t)M * d : (uint16_t*)w.aux, pd};
        h16 = {(uint16_t*)w.big, BF16 ? 0 : (long)M * hid};
        qkv = (float*)w.big;
        qkv16 = (uint16_t*)w.big;
        auto lin = [](const uint16_t* w16, const float* b, int N, int K, bool wide) {
            return Lin16{{w16, BF16 ? 0 : (long)N * K}, b, N, K, !BF16 && wide ? G16X_WIDEW : 0};
        };
        qkv_s = lin(lw.spatial.qkv_w16, c.qkv_bias ? lw.spatial.qkv_b : nullptr, 3 * d, d, lw.spatial.w16_wide & GENIE_WIDE_QKV);
        proj_s = lin(lw.spatial.proj_w16, c.proj_bias ? lw.spatial.proj_b : nullptr, d, d, lw.spatial.w16_wide & GENIE_WIDE_PROJ);
        qkv_t = lin(lw.temporal.qkv_w16, c.qkv_bias ? lw.temporal.qkv_b : nullptr, 3 * d, d, lw.temporal.w16_wide & GENIE_WIDE_QKV);
        proj_t = lin(lw.temporal.proj_w16, c.proj_bias ? lw.temporal.proj_b : nullptr, d, d, lw.temporal.w16_wide & GENIE_WIDE_PROJ);
        fc1 = lin(lw.fc1_w16, c.mlp_bias ? lw.fc1_b : nullptr, hid, d, lw.w16_wide & GENIE_WIDE_FC1);
        fc2 = lin(lw.fc2_w16, c.mlp_bias ? lw.fc2_b : nullptr, d, hid, lw.w16_wide & GENIE_WIDE_FC2);
    }
    // LayerNorm of the f32 rows into operand form
    int norm(const float* x, const float* g, const float* b, Out16 y) const {
        if constexpr (BF16) return launch_layer_norm_bf16(x, g, b, y.p, M, d, 1e-5f, st);
        else return launch_layer_norm_split(x, g, b, y.p, (size_t)y.plane, M, d, 1e-5f, st);
    }
    // (Cf, C16) (+)= epi(A . l.w^T + l.bias) on `rows` rows; flags (G16X_*) say which of the two outputs are written
    int linear(In16 A, const Lin16& l, float* Cf, Out16 C16, int rows, int flags, int batch = 1, long strideA = 0, long strideC = 0) const {
        return launch_gemm16_ex(NPL, A.p, l.K, A.plane, l.w.p, l.K, l.w.plane, l.bias, nullptr, Cf, C16.p, C16.plane, l.N, rows, l.N, l.K,
                                flags | l.wide, 1.0f, st, batch, strideA, 0, strideC);
    }
    // ... with LayerNorm(x; g, b) as the A operand, inside the small GEMM's fragment path (one-frame passes: no LayerNorm launch);
    // GENIE_E_UNSUPPORTED when the problem is not small
    int ln_linear(const float* x, const float* g, const float* b, const Lin16& l, float* Cf, Out16 C16, int flags) const {
        return launch_gemm16_sm_ln(NPL, x, l.K, g, b, 1e-5f, l.w.p, l.K, l.w.plane, l.bias, nullptr, Cf, C16.p, C16.plane, l.N, M, l.N, l.K,
                                   flags, 1.0f, st);
    }
};

// Spatial attention on the fused operand path: the QKV GEMM writes [Q * scale * log2e | K | V^T] as 16-bit planes in the
// attention kernel's own layout (kernels_gemm_pp.hip, G16X_QKV) and kernels_attn_dma.hip streams them through LDS -- no f32
// qkv round trip, no operand split / transpose inside the attention kernel.  Covers the shipped geometry (S = 256, head_dim
// 32 / 64, d % 256 == 0, LayerNorm or qk-norm blocks, chip-filling batches); anything else returns GENIE_E_UNSUPPORTED and the caller
// runs the f32-qkv path below.
// bf16, when the geometry allows: the attention AND the out-projection + residual run as kernels_fused.hip's spatial_attn_proj kernel
// (x updated, its shadow b.x16 too when shadow16; *proj_done = true: the caller skips its proj GEMM)
template <int NPL>
static int spatial_attention_fused(const Backend16<NPL>& b, const genie_cfg& c, const genie_layer_weights& lw, In16 u, int B, float* x,
                                   bool shadow16, bool* proj_done) {
    static const int on = study_env("GENIE_ATTN_DMA", 1);
    const int d = c.d_model;
#ifdef GENIE_STUDY
    if (NPL == 2 && study_terms() != 3) return GENIE_E_UNSUPPORTED;
#endif
    if (b.qkv_s.wide) return GENIE_E_UNSUPPORTED;  // |w| >= 32: two-accumulator GEMM + f32-qkv attention
    // (qk_norm: the per-head LayerNorm of q and k is the QKV GEMM's epilogue -- G16X_QKNORM -- so the planes hold normalised, scaled
    // operands and the attention kernels below are the same in both variants)
    if (!on || c.S != 256 || (c.head_dim != 64 && c.head_dim != 32) || d % 256 || d != c.num_heads * c.head_dim ||
        (c.qk_norm && !(lw.spatial.norm_w && lw.spatial.norm_b)))
        return GENIE_E_UNSUPPORTED;
    const long n_seq = (long)B * c.T;
    const int rc = launch_gemm16_pp(NPL, 3, NPL == 2, u.p, d, u.plane, b.qkv_s.w.p, d, b.qkv_s.w.plane, b.qkv_s.bias, nullptr, nullptr,
                                    b.qkv16, (long)b.M * d, d, b.M, 3 * d, d, G16X_OUT16 | G16X_QKV | (c.qk_norm ? G16X_QKNORM : 0), 1.0f,
                                    b.st, 1, 0, 0, 0, c.attn_scale * 1.4426950408889634f, c.head_dim,
                                    c.qk_norm ? lw.spatial.norm_w : nullptr, c.qk_norm ? lw.spatial.norm_b : nullptr);
    if (rc != GENIE_OK) return rc;
    if constexpr (NPL == 1) {   // shipped geometry, bf16: attention over all heads + out-projection + residual in one kernel
        const int rf = launch_spatial_attn_proj_bf16(c, lw.spatial, b.qkv16, x, shadow16 ? b.x16.p : nullptr, n_seq, b.st);
        if (rf == GENIE_OK) { *proj_done = true; return GENIE_OK; }
        if (rf != GENIE_E_UNSUPPORTED) return rf;
    }
    return launch_attn_spatial_dma(NPL, b.qkv16, n_seq, d, c.num_heads, c.head_dim, b.a16.p, (size_t)b.a16.plane, b.st);
}

// Spatial attention from the f32 qkv: the split kernel writes the operand form itself; any other geometry goes through the generic kernel
// (f32 rows in the logits scratch) and a convert
static int spatial_attention_f32qkv(const genie_cfg& c, const genie_attn_weights& aw, const float* qkv, Workspace& w, int B, Out16 out,
                                    hipStream_t st) {
    const int d = c.d_model;
    const float* nw = c.qk_norm ? aw.norm_w : nullptr;
    const float* nb = c.qk_norm ? aw.norm_b : nullptr;
    const int rc = launch_attn_spatial_split(qkv, nullptr, c.S, (long)B * c.T, d, c.num_heads, c.head_dim, c.attn_scale, nw, nb, st,
                                             out.p, (size_t)out.plane);
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    GENIE_TRY(launch_attn_generic(qkv, w.logits, c.S, (long)B * c.T, 1, c.S, 0, 1, d, c.num_heads, c.head_dim, c.attn_scale, 0, nw, nb,
                                  st));
    return launch_to_operand16(w.logits, out.p, (size_t)out.plane, (size_t)B * c.T * c.S * d, st);
}

// ---- fc2 of the one-frame passes at 2,048-4,096 rows (generate at 8-16 clips): N = d = 512 gives 64-128 tiles of 128x128 for a
// K = 2,048 contraction -- half of the CUs idle and a 64-step K chain.  Split K in two over the GEMM's batch index (256 workgroups,
// 32 steps each) into two f32 slabs in the (idle) logits scratch, then x += bias + slab0 + slab1 in that fixed order
// (profiles/r03_fc2_splitk_ab.txt).  Only in the one-frame passes of generate (a DECODE pass) and only when the 16-bit shadow of x is
// not wanted (every layer but the last of a LayerNorm model): full forwards keep the single fused K chain at every batch size.
// Returns GENIE_E_UNSUPPORTED when the shape is not in that range (the caller then runs the fused-epilogue GEMM).
template <int NPL>
static int fc2_splitk2(const Backend16<NPL>& b, const genie_cfg& c, float* x, Workspace& w, const BlockPass& p) {
    static const int on = study_env("GENIE_FC2_SPLITK", 1);
    const int d = c.d_model, K = c.hidden, M = b.M;
    const long tiles = (long)((M + 127) / 128) * ((d + 127) / 128);
    const size_t V = (size_t)c.factored_vocab * c.num_factored;
    if (!on || !p.is_decode() /* one-frame passes only: a clip's fc2 sum order must not depend on the batch size of a full forward */ ||
        !p.next_is_ln || !w.logits || K < 2048 || K % 256 || d % 4 || tiles > 128 || (long)M * d <= (1L << 19) ||
        V < 2 * (size_t)d || b.fc2.wide)
        return GENIE_E_UNSUPPORTED;
    float* slabs = w.logits;
    GENIE_TRY(launch_gemm16_ex(NPL, b.h16.p, K, b.h16.plane, b.fc2.w.p, K, b.fc2.w.plane, nullptr, nullptr, slabs, nullptr, 0, d, M, d, K / 2,
                               G16X_OUTF32 | G16X_NOSM, 1.0f, b.st, 2, (long)(K / 2), (long)(K / 2), (long)M * d));
    return launch_splitk2_residual(x, slabs, slabs + (size_t)M * d, b.fc2.bias, (size_t)M * d / 4, d, b.st);
}

// One STBlock (st_transformer.py:70-83) on 16-bit Linear operands.  The residual stream x stays f32; its 16-bit form b.x16 is only read
// by a Linear that has no LayerNorm in front: temporal qkv always, fc1 and the next block's spatial qkv only in the qk-norm variant, the
// readout after the last block.
template <int NPL>
static int block16(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, BlockCarry& carry, int B,
                   hipStream_t st) {
    constexpr bool BF16 = NPL == 1;
    const int M = B * c.T * c.S;
    GENIE_CHECK_ARG(lw.spatial.qkv_w16 && lw.spatial.proj_w16 && lw.temporal.qkv_w16 && lw.temporal.proj_w16 &&
                        lw.fc1_w16 && lw.fc2_w16,
                    "%s", Backend16<NPL>::kNeedWeights);
    const Backend16<NPL> b(c, lw, w, M, st);
    // bf16, t16: the temporal qkv (and the KV cache slices) hold bf16 -- the qkv GEMM stores 2 bytes per value instead of 4 and the attention
    // kernels (HBM-bound) read half the bytes; softmax and both products stay f32 inside them
    const bool t16 = BF16 && temporal_qkv16(c, p.model_T);
    BlockCarry prev;          // bf16: what the previous block's fused MLP kernel already did for this one
    bool frag_t = false;      // bf16: the prefix-cache passes run the temporal sub-block as the fused kernel of kernels_fused_prefix.hip
    bool shadow16 = true;     // bf16: does the fused spatial kernel write x16?
    if constexpr (BF16) {
        prev = carry;   // taken, so that it is read once
        carry = BlockCarry();
        // Will the temporal sub-block run as a fused kernel?  Then it rounds its operands from the f32 rows itself and the spatial kernel in
        // front need not write the bf16 shadow of x (134 MB per layer at 64 clips it would write and the temporal kernel read).
        static const int no_shadow_env = study_env("GENIE_T_FROM_F32", 1);   // (a study-build knob: the shipping library reads no environment)
        const bool fused_t = p.is_plain() && t16 && temporal_fused_takes(c, lw.temporal, B);
        // ... or, in the prefix-cache passes, as the fused kernel that keeps the K / V fragment images in the cache slice
        frag_t = p.is_cache_pass() && !p.strided(c.T) && t16 && temporal_prefix_fused_takes(c, lw.temporal, B, p.model_T);
        shadow16 = !((fused_t || frag_t) && no_shadow_env);
    }

    // ---- spatial: x += proj(SpAttn(qkv(norm1(x))))
    GENIE_STUDY_CLASS(0);
    In16 u = b.x16;
    int rc = GENIE_E_UNSUPPORTED;
    bool qkv_done = false, proj_done = false;
    if constexpr (BF16) {
        if (prev.qkv_planes_done) {   // the previous block's fused MLP kernel left this block's operand planes in `big`
            rc = launch_spatial_attn_proj_bf16(c, lw.spatial, b.qkv16, x, shadow16 ? b.x16.p : nullptr, (long)B * c.T, st);
            if (rc == GENIE_OK) proj_done = true;
            else if (rc == GENIE_E_UNSUPPORTED)   // (fewer sequences than the fused kernel takes: the stand-alone attention kernel reads the same planes, proj GEMM below)
                rc = launch_attn_spatial_dma(1, b.qkv16, (long)B * c.T, c.d_model, c.num_heads, c.head_dim, b.a16.p, 0, st);
            GENIE_TRY(rc);
            qkv_done = true;
        }
    }
    if (!qkv_done && !c.qk_norm) {
        const int r2 = b.ln_linear(x, lw.norm1_w, lw.norm1_b, b.qkv_s, b.qkv, Out16{}, G16X_OUTF32);
        if (r2 == GENIE_OK) qkv_done = true;
        else if (r2 != GENIE_E_UNSUPPORTED) return r2;
    }
    if (!qkv_done) {
        if (!c.qk_norm) {
            if (!prev.ln1_done)   // (bf16, else: the previous block's fused MLP kernel wrote norm1(x) into a16)
                GENIE_TRY(b.norm(x, lw.norm1_w, lw.norm1_b, b.a16));
            u = b.a16;
        }
        rc = spatial_attention_fused(b, c, lw, u, B, x, shadow16, &proj_done);
    }
    if (rc == GENIE_E_UNSUPPORTED) {
        if (!qkv_done) GENIE_TRY(b.linear(u, b.qkv_s, b.qkv, Out16{}, M, G16X_OUTF32));
        rc = spatial_attention_f32qkv(c, lw.spatial, b.qkv, w, B, b.a16, st);
    }
    GENIE_TRY(rc);
    GENIE_STUDY_CLASS(2);
    // f16x3, the shipped geometry: temporal qkv Linear + attention as one kernel on the f32 rows of x (kernels_fused_f16x3.hip) -- the spatial
    // out-projection then need not write the split planes of x; in the prefix-cache passes the cache slice holds that kernel's k, v accumulators
    bool fused_tq = false;
    if constexpr (!BF16)
        fused_tq = !p.is_decode() && !p.strided(c.T) && temporal_qkv_attn_f16x3_takes(c, lw.temporal, B, p.model_T, p.is_cache_pass());
    if (!proj_done) GENIE_TRY(b.linear(b.a16, b.proj_s, x, b.x16, M, G16X_ACCUM | G16X_OUTF32 | (fused_tq ? 0 : G16X_OUT16)));

    // ---- temporal (no pre-norm): x += proj(TmpAttn(qkv(x), causal))
    GENIE_STUDY_CLASS(1);
    bool attn_done = false;   // the attention output is in a16
    bool proj_todo = true;    // ... and the out-projection + residual still to do
    if constexpr (BF16) {
        if (p.is_plain() && t16) {
            // plain full-clip forward of the shipped geometry: qkv + attention + proj + residual in ONE kernel, the qkv never
            // leaves the registers (kernels_fused.hip); same rounding points as the launches below
            // (the bf16 shadow of x exists unless the fused spatial kernel ran and was told not to write it)
            rc = launch_temporal_fused_bf16(c, lw.temporal, (proj_done && !shadow16) ? nullptr : b.x16.p, x, B, st);
            if (rc == GENIE_OK) proj_todo = false;
            else if (rc != GENIE_E_UNSUPPORTED) return rc;
        }
        if (frag_t) {   // prefix-cache passes of the shipped geometry: one kernel, the cache slice holds K / V fragment images
            GENIE_TRY(launch_temporal_prefix_fused_bf16(c, lw.temporal, x, reinterpret_cast<uint16_t*>(p.cache), B, p.fused_mode(), p.tshift,
                                                        p.model_T, st));
            if (p.stop_after_tqkv) return GENIE_OK;
            proj_todo = false;
        }
    } else if (fused_tq) {
        GENIE_TRY(launch_temporal_qkv_attn_f16x3(c, lw.temporal, x, b.a16.p, b.a16.plane, p.cache, B, p.fused_mode(), p.tshift, p.model_T, st));
        if (p.stop_after_tqkv) return GENIE_OK;
        attn_done = true;
    }
    if (proj_todo) {
        if (!attn_done) {
            const TemporalQkv tq = temporal_qkv_target(c, p, b.qkv, B);
            float* tq_f32 = tq.base + tq.off;
            Out16 tq_16;
            if (t16) {   // bf16: the same element offset of the same base, 2 bytes per value
                tq_16.p = reinterpret_cast<uint16_t*>(tq.base) + tq.off;
                tq_f32 = nullptr;
            }
            GENIE_TRY(b.linear(b.x16, b.qkv_t, tq_f32, tq_16, tq.rows, t16 ? G16X_OUT16 : G16X_OUTF32, tq.batch, tq.strideA, tq.strideC));
            if (p.stop_after_tqkv) return GENIE_OK;
            GENIE_TRY(temporal_attention(c, lw.temporal, p, tq, nullptr, b.a16.p, (size_t)b.a16.plane, t16, w, B, st));
        }
        GENIE_STUDY_CLASS(3);
        GENIE_TRY(b.linear(b.a16, b.proj_t, x, b.x16, M, G16X_ACCUM | G16X_OUTF32 | (c.qk_norm ? G16X_OUT16 : 0)));
    }

    // ---- MLP: x += fc2(gelu(fc1(norm2(x))))
    GENIE_STUDY_CLASS(4);
    if constexpr (BF16) {
        if (!p.is_decode()) {   // LayerNorm + fc1 + GELU + fc2 + residual in one kernel for the shipped geometry (kernels_fused.hip)
            const genie_layer_weights* nx = p.next_layer;
            if (nx && nx->norm1_w && nx->norm1_b && p.next_is_ln) {
                rc = GENIE_E_UNSUPPORTED;
                if (nx->spatial.fused_w16 && (nx->spatial.w16_wide & GENIE_FUSED_QKV_STREAM)) {
                    // ... and the next block's spatial qkv Linear too: its operand planes (in `big`, where its qkv GEMM would put them)
                    rc = launch_mlp_fused_bf16(c, lw, x, nullptr, (long)M, st, nx->norm1_w, nx->norm1_b,
                                               nx->spatial.fused_w16 + GENIE_SPATIAL_PROJ_FUSED_ELEMS, b.qkv16);
                    if (rc == GENIE_OK) carry.qkv_planes_done = true;
                }
                if (rc == GENIE_E_UNSUPPORTED) {   // ... or the next block's norm1 (into a16)
                    rc = launch_mlp_fused_bf16(c, lw, x, b.a16.p, (long)M, st, nx->norm1_w, nx->norm1_b);
                    if (rc == GENIE_OK) carry.ln1_done = true;
                }
            } else {
                rc = launch_mlp_fused_bf16(c, lw, x, p.next_is_ln ? nullptr : b.x16.p, (long)M, st);
            }
            if (rc != GENIE_E_UNSUPPORTED) return rc;
        }
    }
    u = b.x16;
    bool fc1_done = false;
    if (!c.qk_norm) {
        const int r2 = b.ln_linear(x, lw.norm2_w, lw.norm2_b, b.fc1, nullptr, b.h16, G16X_GELU | G16X_OUT16);
        if (r2 == GENIE_OK) fc1_done = true;
        else if (r2 != GENIE_E_UNSUPPORTED) return r2;
    }
    if (!fc1_done) {
        if (!c.qk_norm) {
            GENIE_TRY(b.norm(x, lw.norm2_w, lw.norm2_b, b.a16));
            u = b.a16;
        }
        GENIE_TRY(b.linear(u, b.fc1, nullptr, b.h16, M, G16X_GELU | G16X_OUT16));
    }
    GENIE_STUDY_CLASS(5);
    const int rs = fc2_splitk2(b, c, x, w, p);
    if (rs != GENIE_E_UNSUPPORTED) return rs;
    return b.linear(b.h16, b.fc2, x, b.x16, M, G16X_ACCUM | G16X_OUTF32 | (p.next_is_ln ? 0 : G16X_OUT16));
}

int st_block16(const genie_cfg& c, const genie_layer_weights& lw, float* x, Workspace& w, const BlockPass& p, BlockCarry& carry, int B,
               hipStream_t st) {
    return c.precision == GENIE_PREC_BF16 ? block16<1>(c, lw, x, w, p, carry, B, st) : block16<2>(c, lw, x, w, p, carry, B, st);
}

// The 16-bit form of x must exist before the first layer when the block has no pre-norm (qk_norm configs).  LayerNorm blocks read the
// f32 x (norm1) first and their spatial out-projection writes it before anything reads it.
int prepare16(const genie_cfg& c, const float* x, Workspace& w, int B, hipStream_t st) {
    if (!c.qk_norm) return GENIE_OK;
    const size_t n = (size_t)B * c.T * c.S * c.d_model;
    return c.precision == GENIE_PREC_BF16 ? launch_shadow_bf16(x, (uint16_t*)w.xn, n, st) : launch_split_f16(x, (uint16_t*)w.xn, n, n, st);
}

// out_x_proj on frames [t0,t1): token-major (B,nt,S,V), or BCTHW (B,V,nt,S) via the operand-swapped GEMM (exact) / the token-major
// scratch and a transpose (16-bit: from the 16-bit form of x in the workspace)
int readout(const genie_cfg& c, const genie_weights& wt, const float* x, Workspace& w, int B, int t0, int t1, int layout, float* logits,
            hipStream_t st) {
    const int d = c.d_model, nt = t1 - t0, V = c.factored_vocab * c.num_factored;
    const long rows = (long)nt * c.S, strideX = (long)c.T * c.S * d;
    if (c.precision == GENIE_PREC_EXACT) {
        const float* xa = x + (size_t)t0 * c.S * d;
        if (layout == GENIE_LAYOUT_TOKEN_MAJOR) {
            return launch_gemm_f32(xa, d, strideX, wt.out_w, d, 0, wt.out_b, logits, V, rows * V, (int)rows, V, d, B, 0,
                                   c.readout_mult, st);
        }
        return launch_gemm_f32(wt.out_w, d, 0, xa, d, strideX, wt.out_b, logits, rows, rows * V, V, (int)rows, d, B,
                               GEMM_BIAS_ALONG_M, c.readout_mult, st);
    }
    const bool bf16 = c.precision == GENIE_PREC_BF16;
    GENIE_CHECK_ARG(wt.out_w16, "%s", bf16 ? Backend16<1>::kNeedWeights : Backend16<2>::kNeedWeights);
    GENIE_CHECK_ARG((const void*)x == (const void*)w.x, "%s readout reads the workspace's own hidden state", bf16 ? "bf16" : "f16x3");
    const uint16_t* x16 = (const uint16_t*)w.xn;
    float* dst = (layout == GENIE_LAYOUT_TOKEN_MAJOR) ? logits : w.logits;
    GENIE_STUDY_CLASS(6);
    GENIE_TRY(launch_gemm16_ex(bf16 ? 1 : 2, x16 + (size_t)t0 * c.S * d, d, bf16 ? 0 : (long)B * strideX, wt.out_w16, d,
                               bf16 ? 0 : (long)V * d, wt.out_b, nullptr, dst, nullptr, 0, V, (int)rows, V, d,
                               G16X_OUTF32 | (!bf16 && wt.out_w16_wide ? G16X_WIDEW : 0), c.readout_mult, st, B, strideX, 0, rows * V));
    if (layout != GENIE_LAYOUT_TOKEN_MAJOR) GENIE_TRY(launch_transpose(w.logits, logits, B, (int)rows, V, st));
    return GENIE_OK;
}

}  // namespace genie
