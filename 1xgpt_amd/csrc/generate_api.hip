// The generate loops of the C ABI (include/genie_hip.h): cached generate, rollout past the window, fan-out, scoring of observed futures and
// the full-forward MaskGIT loop.  Each is a sequence of passes (api.hip: frames_pass, the clean pass, the full forward) with token-id,
// sample and mask-step launches between them; everything is enqueued on the caller's stream, nothing allocates or synchronises.
// What a pass needs is a PassCtx, the checked decode options of a call a Decode; the MaskGIT step (maskgit_step), the commit rule
// (commit_slot) and the fan-out prologue (fanout_prologue) are each stated once.  Known tokens (genie_known: inpainting) ride in the
// Decode: where they are set a slot starts from them (launch_known_begin) and the mask step counts per clip (launch_mask_step_known);
// where they are not, every loop enqueues the launches it always did.
#include <stddef.h>

#include "common.hpp"
#include "kernels.hpp"

using namespace genie;

// ---- token-id kernels (extern "C": their symbols are the unmangled names profiles and traces know) --------------------------
extern "C" {
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
// rows of S token ids for the B * K clips of a fan-out pass from their B parents: dst[i][0..S) = src[i / K][0..S) (strides in elements)
__global__ void branch_frame_ids_kernel(const int64_t* __restrict__ src, long src_stride, int64_t* __restrict__ dst, long dst_stride, int S,
                                        long BK, int K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK * S) return;
    const long r = i / S, s = i - r * S;
    dst[r * dst_stride + s] = src[(r / K) * src_stride + s];
}
static int put_branch_frame_ids(const int64_t* src, long src_stride, int64_t* dst, long dst_stride, int S, int BK, int K, hipStream_t st) {
    branch_frame_ids_kernel<<<(unsigned)(((long)BK * S + 255) / 256), 256, 0, st>>>(src, src_stride, dst, dst_stride, S, (long)BK, K);
    GENIE_LAUNCH_CHECK("branch_frame_ids");
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
// The (NB, T) actions of a fan-out call's context pass and the (NB * K, T) actions of its decode passes from the caller's (B * K, T) ids,
// null halves included: parent b reads its context actions from its branch 0 (row b * K; frames < P of the other branches are never read).
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
}  // extern "C"

// ---- loop scratch ----------------------------------------------------------------------------------------------------------
// The loop scratch of genie_generate_cached_* / genie_rollout_cached: B clips are decoded, NB clips run through every pass (NB == B, or
// 2 B under guidance: [conditional ; null]).  The size functions and the loops both carve here (base == NULL: sizes only).
// A fan-out call carves the same buffers: its context runs NBctx = NB / K clips, and it keeps their (NBctx, T) actions beside the
// branches' (NB, T).
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
// the model's workspace for B clips of T frames
static size_t pass_bytes(const genie_cfg& c, int B, int T) {
    genie_cfg cm = c;
    cm.T = T;
    return carve(cm, B, nullptr).total;
}
// ... behind the workspace of the call's largest pass: the prompt's P frames, two frames for the merged passes
static GenScratch carve_generate(const genie_cfg& c, int B, int NB, int P, char* base, bool window_acts = false) {
    return carve_loop(c, B, NB, NB, P, pass_bytes(c, NB, P > 2 ? P : 2), base, NB != B || window_acts);   // window_acts: the rollout's action window
}
// ... of a fan-out call: B * K clips are decoded, NB * K run through every decode pass, NB through the context pass.  The scratch starts
// behind the larger of the context pass (NB clips, P frames) and a two-frame pass of NB * K clips.
static GenScratch carve_fanout(const genie_cfg& c, int B, int NB, int K, int P, char* base) {
    const size_t ctx = pass_bytes(c, NB, P), two = pass_bytes(c, NB * K, 2);
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
// What a loop call needs of its workspace: the end of its scratch, and never less than the model's own workspace for the clips of its
// passes (the passes themselves check against that size).  `model`: carve(c, NB).total, or the end of a GuidedPrompt behind it.
static size_t loop_bytes(size_t scratch_end, size_t model) { return scratch_end > model ? scratch_end : model; }

// ---- what the loops are made of --------------------------------------------------------------------------------------------
// The checked decode options of one call: B clips are decoded, copies * B run through every pass
struct Decode {
    int steps, unmask_mode;
    float temperature;
    const genie_sampling* law;   // the caller's, or the confidence mode's default
    const genie_guidance* guidance;
    bool guided;                 // guidance of a scale other than 1: every pass runs [conditional ; null], copies = 2
    int copies;
    const int64_t* known;        // known tokens of the call's first decoded frame (clip stride known_stride), or NULL: all-mask starts
    long known_stride;
};
// a genie_known (NULL = none) over `frames` decoded frames of S tokens, checked on the host before anything is enqueued
static int check_known(const genie_known* known, long frames, int S, const char* where) {
    if (!known) return GENIE_OK;
    GENIE_CHECK_ARG(known->ids, "%s: known: ids is NULL", where);
    GENIE_CHECK_ARG(known->clip_stride >= frames * S, "%s: known: clip_stride %lld is below %ld frames x S=%d", where,
                    (long long)known->clip_stride, frames, S);
    return GENIE_OK;
}
// ... checked on the host before anything is enqueued; where: the entry point's name in the messages
static int make_decode(Decode& D, int B, int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                       const genie_sampling* sampling, const genie_guidance* guidance, const genie_frame_cond* cond, const char* where,
                       const genie_known* known) {
    GENIE_TRY(check_guidance(guidance, cond, where));
    GENIE_TRY(check_sampling(sampling, where));
    GENIE_TRY(check_unmask(unmask_mode, unmask_mode != -1, steps, noise, where));
    GENIE_CHECK_ARG(temperature <= 1e-8f || uniforms, "%s: temperature > 0 needs uniforms", where);
    D.steps = steps, D.temperature = temperature, D.unmask_mode = unmask_mode, D.guidance = guidance;
    D.law = (unmask_mode == GENIE_UNMASK_CONFIDENCE && !sampling) ? &kDefaultSampling : sampling;
    // under guidance every pass runs 2 B clips, [conditional ; null]: rows b and b + B hold the same tokens, the second half's actions are
    // null_action at every frame; B rows are sampled, masked and written out
    D.guided = guidance && guidance->scale != 1.0f;
    D.copies = D.guided ? 2 : 1;
    D.known = known ? known->ids : nullptr, D.known_stride = known ? (long)known->clip_stride : 0;
    GENIE_CHECK_ARG(!D.guided || B <= 0x3fffffff, "%s: B=%d too large for guidance", where, B);
    return GENIE_OK;
}

// What a cache pass of a loop needs, and nothing else: NB clips over `cache`
struct PassCtx {
    const genie_cfg* cfg;
    const genie_weights* wt;
    int NB;
    const genie_frame_cond* cond;   // what the passes embed with: ids (NB, cfg->T)
    float* cache;
    size_t cache_bytes;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    const FanOut* fan;   // a fan-out call's decode passes: `cache` is the branch cache (the context ran into fan->trunk); else NULL
};
static PassCtx pass_ctx(const genie_cfg* cfg, const genie_weights* wt, int NB, const genie_frame_cond* cond, float* cache, size_t cache_bytes,
                        void* workspace, size_t workspace_bytes, void* stream) {
    PassCtx X;
    X.cfg = cfg, X.wt = wt, X.NB = NB, X.cond = cond, X.cache = cache, X.cache_bytes = cache_bytes;
    X.workspace = workspace, X.workspace_bytes = workspace_bytes, X.stream = stream, X.fan = nullptr;
    return X;
}
static int run_pass(const PassCtx& X, const int64_t* frame_ids, int t, int nf, float* logits) {
    return frames_pass(X.cfg, X.wt, frame_ids, X.NB, t, nf, X.cache, X.cache_bytes, logits, X.workspace, X.workspace_bytes, X.stream, X.cond,
                       X.fan);
}

// `ctx` context frames into cache slots 0 .. ctx-1: one ctx-frame pass over g.idsP (NB, ctx, S, already filled) where the fragment-order
// kernels cover it, else the clean pass with the cache's T-frame layout, else frame by frame from src (frame t of clip b at
// src + b * src_stride + t * S; B clips, each `copies` times)
static int run_context(const PassCtx& X, const GenScratch& g, int B, int copies, int ctx, const int64_t* src, long src_stride) {
    const genie_cfg& c = *X.cfg;
    int rc = GENIE_E_UNSUPPORTED;
    if (ctx > 1) {
        rc = genie_frames_pass_cond(X.cfg, X.wt, g.idsP, X.NB, 0, ctx, X.cache, X.cache_bytes, nullptr, X.workspace, X.workspace_bytes,
                                    X.stream, X.cond);
        if (rc == GENIE_E_UNSUPPORTED)
            rc = genie_clean_pass_cond(X.cfg, X.wt, g.idsP, X.NB, ctx, c.T, X.cache, X.cache_bytes, X.workspace, X.workspace_bytes,
                                       X.stream, X.cond);
    }
    if (rc != GENIE_E_UNSUPPORTED) return rc;
    for (int t = 0; t < ctx; ++t) {
        GENIE_TRY(put_frame_ids(src + (size_t)t * c.S, src_stride, g.fin, c.S, c.S, B, 0, as_stream(X.stream), copies));
        GENIE_TRY(genie_frames_pass_cond(X.cfg, X.wt, g.fin, X.NB, t, 1, X.cache, X.cache_bytes, nullptr, X.workspace, X.workspace_bytes,
                                         X.stream, X.cond));
    }
    return GENIE_OK;
}

// The commit rule.  merge: the call still tries merged commits; opened: the last commit also ran MaskGIT step 0 of the next slot (its
// logits are in g.logits), which whoever consumes them resets.
struct Commit {
    bool merge = false, opened = false;
    const int64_t* next_known = nullptr;   // the known tokens of the slot a merged commit opens (clip stride known_stride), or NULL
    long known_stride = 0;
};
// Commit slot t from the tokens that put(dst, dst_stride) lays into the pass's rows of dst: in the two-frame pass that also carries the
// start tokens of slot t + 1 (all-mask, or cm.next_known where known; B clips, each `copies` times), for good on its own once the
// library refuses that pass
template <class Put>
static int commit_slot(const PassCtx& X, const GenScratch& g, Commit& cm, int t, int B, int copies, Put put) {
    const genie_cfg& c = *X.cfg;
    if (cm.merge) {
        GENIE_TRY(put(g.two, 2L * c.S));
        if (cm.next_known)
            GENIE_TRY(launch_known_begin(cm.next_known, cm.known_stride, c.image_vocab_size, g.two + c.S, 2L * c.S, nullptr, B, c.S, copies,
                                         as_stream(X.stream)));
        else
            GENIE_TRY(put_frame_ids(nullptr, 0, g.two + c.S, 2L * c.S, c.S, B, c.image_vocab_size, as_stream(X.stream), copies));
        const int rc = run_pass(X, g.two, t, 2, g.logits);
        if (rc == GENIE_E_UNSUPPORTED) cm.merge = false;
        else { GENIE_TRY(rc); cm.opened = true; }
    }
    if (!cm.opened) {
        GENIE_TRY(put(g.fin, (long)c.S));
        GENIE_TRY(run_pass(X, g.fin, t, 1, nullptr));
    }
    return GENIE_OK;
}

// One MaskGIT step of one frame: sample B rows from the frame's token-major logits (logits_null: the null half under guidance), then
// mask-step the samples into the frame's tokens at `frame` (clip stride in elements).  noise / uniforms: the call's draws for this frame,
// (steps - 1, B, S) and (steps, num_factored, B, S).  known: the frame's known tokens (clip stride D.known_stride): each clip re-masks
// ceil(frac * (S - K_b)) tokens, K_b counted by the kernel; NULL: mask_count of S for all.
static int maskgit_step(const genie_cfg& c, const Decode& D, int B, const float* logits, const float* logits_null, int64_t* samples,
                        float* conf, uint8_t* unmasked, int64_t* frame, long clip_stride, int step, const float* noise,
                        const float* uniforms, const int64_t* known, hipStream_t st) {
    const size_t BS = (size_t)B * c.S;
    const bool last = step == D.steps - 1, by_conf = D.unmask_mode == GENIE_UNMASK_CONFIDENCE;
    const float* u = D.temperature > 1e-8f ? uniforms + (size_t)step * c.num_factored * BS : nullptr;
    const float* draws = (last || D.unmask_mode == GENIE_UNMASK_GREEDY) ? nullptr : noise + (size_t)step * BS;
    // "confidence": the sample launch writes the keys over conf (nothing else reads conf in the loops)
    const float anneal = 1.0f - (float)(step + 1) / (float)D.steps;
    float* keys_out = (by_conf && !last) ? conf : nullptr;
    if (D.guided)
        GENIE_TRY(launch_sample_guided(c, logits, logits_null, GENIE_LAYOUT_TOKEN_MAJOR, B, D.temperature, u, samples, conf, D.law, keys_out,
                                       draws, anneal, D.guidance->scale, st));
    else
        GENIE_TRY(launch_sample_ex(c, logits, GENIE_LAYOUT_TOKEN_MAJOR, B, D.temperature, u, samples, conf, D.law, keys_out, draws, anneal, st));
    const float* keys = last ? nullptr : (D.unmask_mode == GENIE_UNMASK_RANDOM ? draws : conf);
    if (known)
        return launch_mask_step_known(keys, last ? 0.0 : mask_fraction(step, D.steps), last, c.image_vocab_size, known, D.known_stride,
                                      unmasked, samples, frame, clip_stride, B, c.S, st);
    return launch_mask_step(keys, last ? 0 : mask_count(step, D.steps, c.S), last, c.image_vocab_size, unmasked, samples, frame, clip_stride,
                            B, c.S, st);
}

// The window body: decodes cache slots t0 .. t0 + n - 1 one after the other (slots < t0 - 1 are committed; slot t0 - 1 too unless `pend`).
// Slot t0 + k draws from noise / uniforms [k] and its final tokens go to out + k * S (clip stride out_stride); its step-0 logits to
// logits0_out[:, k] of (B, n, S, V) when wanted.  Every slot but the LAST is committed -- from its final tokens, or from tf + k * S (clip
// stride tf_stride) when tf is given (teacher forcing in time) --, merged with step 0 of the next slot where merge_commit is set and the
// library covers it.  pend != NULL: slot t0 - 1 is still pending; its final tokens (pend, clip stride pend_stride) are committed first, by
// the same rule.  known != NULL: slot t0 + k starts from the known tokens at known + k * S (clip stride D.known_stride) instead of
// all-mask, in one launch, and so does the second frame of the merged commit that opens it.
static int decode_slots(const PassCtx& X, const Decode& D, int B, const GenScratch& g, int merge_commit, int t0, int n, const float* noise,
                        const float* uniforms, int64_t* out, long out_stride, float* logits0_out, const int64_t* tf, long tf_stride,
                        const int64_t* pend, long pend_stride, const int64_t* known) {
    const genie_cfg& c = *X.cfg;
    const int S = c.S, steps = D.steps;
    hipStream_t st = as_stream(X.stream);
    const size_t BS = (size_t)B * S, V = (size_t)c.factored_vocab * c.num_factored;
    const float* logits_null = g.logits + BS * V;   // guided: rows B .. 2B - 1 of every pass's logits
    Commit cm;
    cm.merge = merge_commit != 0;
    cm.known_stride = D.known_stride;
    auto commit = [&](int t, const int64_t* fsrc, long fstride, int k_next) {   // k_next: the slot it opens, t + 1 = t0 + k_next
        cm.next_known = known ? known + (size_t)k_next * S : nullptr;
        return commit_slot(X, g, cm, t, B, D.copies, [&](int64_t* dst, long dst_stride) {
            return put_frame_ids(fsrc, fstride, dst, dst_stride, S, B, 0, st, D.copies);
        });
    };
    if (pend) GENIE_TRY(commit(t0 - 1, pend, pend_stride, 0));
    for (int k = 0; k < n; ++k) {
        const int t = t0 + k;
        const int64_t* kn = known ? known + (size_t)k * S : nullptr;
        if (kn) {
            GENIE_TRY(launch_known_begin(kn, D.known_stride, c.image_vocab_size, g.cur, S, g.unmasked, B, S, D.copies, st));
        } else {
            GENIE_TRY(put_frame_ids(nullptr, 0, g.cur, S, S, B, c.image_vocab_size, st, D.copies));
            if (hipMemsetAsync(g.unmasked, 0, BS, st) != hipSuccess) { set_error("memset failed"); return GENIE_E_LAUNCH; }
        }
        for (int step = 0; step < steps; ++step) {
            if (!(step == 0 && cm.opened))
                GENIE_TRY(run_pass(X, g.cur, t, 1, g.logits));
            if (step == 0 && logits0_out) {   // orig_logits of the frame (st_mask_git.py:165,226): the step-0 logits, (B, n, S, V)
                if (D.guided) {               // ... the guided ones
                    GENIE_TRY(launch_guide_logits(g.logits, logits_null, logits0_out + (size_t)k * S * V, B, (long)(S * V), (long)(S * V),
                                                  (long)((size_t)n * S * V), D.guidance->scale, st));
                } else if (hipMemcpy2DAsync(logits0_out + (size_t)k * S * V, (size_t)n * S * V * 4, g.logits, (size_t)S * V * 4,
                                            (size_t)S * V * 4, (size_t)B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                    set_error("memcpy failed");
                    return GENIE_E_LAUNCH;
                }
            }
            GENIE_TRY(maskgit_step(c, D, B, g.logits, logits_null, g.samples, g.conf, g.unmasked, g.cur, S, step,
                                   noise ? noise + (size_t)k * (steps - 1) * BS : nullptr,
                                   uniforms ? uniforms + (size_t)k * steps * c.num_factored * BS : nullptr, kn, st));
            if (D.guided) GENIE_TRY(put_frame_ids(g.cur, S, g.cur + BS, S, S, B, 0, st));   // the null half sees the same tokens
        }
        GENIE_TRY(put_frame_ids(g.cur, S, out + (size_t)k * S, out_stride, S, B, 0, st));
        cm.opened = false;
        if (k + 1 < n)   // commit slot t: its final tokens, or the ground truth when teacher-forcing in time
            GENIE_TRY(commit(t, tf ? tf + (size_t)k * S : g.cur, tf ? tf_stride : (long)S, k + 1));
    }
    return GENIE_OK;
}

// decode_slots' sibling for OBSERVED frames of a fan-out call (X.NB = B * K clips): per slot t0 + j the all-mask pass (riding the commit of
// slot t0 + j - 1), launch_score_rows on its logits against frame j of obs (parent clip i / K of row i, clip stride obs_stride), then the
// commit of the observed tokens; the last slot is not committed.  nll / hits (X.NB, n), token_nll (X.NB, n, S).  No sample or mask-step
// launches, no draws, no host synchronisation.
static int score_slots(const PassCtx& X, const GenScratch& g, int merge_commit, int t0, int n, const int64_t* obs, long obs_stride, int K,
                       double* nll, double* hits, float* token_nll) {
    const genie_cfg& c = *X.cfg;
    const int BK = X.NB, S = c.S;
    hipStream_t st = as_stream(X.stream);
    Commit cm;
    cm.merge = merge_commit != 0;
    for (int j = 0; j < n; ++j) {
        if (!cm.opened) {
            GENIE_TRY(put_frame_ids(nullptr, 0, g.cur, S, S, BK, c.image_vocab_size, st));
            GENIE_TRY(run_pass(X, g.cur, t0 + j, 1, g.logits));
        }
        GENIE_TRY(launch_score_rows(c, g.logits, obs + (size_t)j * S, obs_stride, K, BK, nll + j, n, hits ? hits + j : nullptr,
                                    token_nll ? token_nll + (size_t)j * S : nullptr, (long)n * S, st));
        cm.opened = false;
        if (j + 1 == n) break;
        GENIE_TRY(commit_slot(X, g, cm, t0 + j, BK, 1, [&](int64_t* dst, long dst_stride) {
            return put_branch_frame_ids(obs + (size_t)j * S, obs_stride, dst, dst_stride, S, BK, K, st);
        }));
    }
    return GENIE_OK;
}

// NB * K as an int the passes can take, or 0
static int fanout_clips(int B, int K, int copies) {
    if (B < 1 || K < 1) return 0;
    const long n = (long)B * K * copies;
    return n <= 0x3fffffff ? (int)n : 0;
}

// What a fan-out call decodes or scores with, once its context has run: the passes of its B * K * copies branch clips over the split
// cache, and the scratch
struct FanCall {
    FanOut fan;
    genie_frame_cond cond_ctx, cond_br;
    PassCtx br;
    GenScratch g;
};
// The front of genie_generate_fanout and genie_score_fanout (where; sizer: the size function its workspace message names): B parent clips
// of P context frames (ids, clip stride ids_stride) and n branch slots; `copies` of every clip per pass, the second with null_action at
// every frame.  Checks the sizes, carves, lays out the actions of both kinds of pass in one launch and runs the context of the
// B * copies clips once, into the trunk.  `out`: the call's required output, for the NULL check.
static int fanout_prologue(const char* where, const char* sizer, const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids,
                           long ids_stride, const void* out, int B, int K, int P, int n, int copies, int64_t null_action, float* trunk,
                           size_t trunk_bytes, float* branch, size_t branch_bytes, void* workspace, size_t workspace_bytes, void* stream,
                           const genie_frame_cond* cond, FanCall& F) {
    const genie_cfg& c = *cfg;
    const int NBK = fanout_clips(B, K, copies), NB = B * copies;
    GENIE_CHECK_ARG(NBK > 0, "%s: B=%d x K=%d%s clips per pass are too many", where, B, K, copies == 2 ? " x 2" : "");
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && out && trunk && branch && workspace, "%s: NULL pointer", where);
    GENIE_CHECK_ARG(trunk_bytes >= genie_prefix_cache_bytes(cfg, NB), "%s: trunk cache too small (genie_prefix_cache_bytes of %d clips)", where, NB);
    GENIE_CHECK_ARG(branch_bytes >= fanout_branch_bytes(c, (size_t)NBK, n), "%s: branch cache too small (genie_fanout_branch_bytes)", where);
    F.g = carve_fanout(c, B, NB, K, P, (char*)workspace);
    const size_t need = loop_bytes(F.g.end, carve(c, NB, nullptr).total);
    GENIE_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes: size it with %s)", where, workspace_bytes, need, sizer);
    hipStream_t st = as_stream(stream);
    PassCtx ctx = pass_ctx(cfg, wt, NB, cond, trunk, trunk_bytes, workspace, workspace_bytes, stream);
    F.br = pass_ctx(cfg, wt, NBK, cond, branch, branch_bytes, workspace, workspace_bytes, stream);
    F.fan.trunk = trunk, F.fan.K = K, F.fan.P0 = P, F.fan.Tb = n;
    F.br.fan = &F.fan;
    if (cond && cond->n_actions > 0) {   // the context's actions and the branches' come from one launch
        int64_t* acts_ctx = F.g.acts_ctx ? F.g.acts_ctx : F.g.acts;   // (K == 1: one table serves both)
        const long na = (long)NB * c.T * (1 + K);
        fanout_actions_kernel<<<(unsigned)((na + 255) / 256), 256, 0, st>>>(cond->ids, acts_ctx, F.g.acts, B, K, NB, c.T, P, null_action);
        GENIE_LAUNCH_CHECK("fanout_actions");
        F.cond_ctx = F.cond_br = *cond;
        F.cond_ctx.ids = acts_ctx;
        F.cond_br.ids = F.g.acts;
        ctx.cond = &F.cond_ctx;
        F.br.cond = &F.cond_br;
    }
    GENIE_TRY(put_frame_ids(ids, ids_stride, F.g.idsP, (long)P * c.S, P * c.S, B, 0, st, copies));
    return run_context(ctx, F.g, B, copies, P, ids, ids_stride);
}

// The full-forward MaskGIT loop (genie_maskgit_generate_guided is this with known NULL, _ex with guidance NULL too): B clips decoded,
// NB per forward
int genie_maskgit_generate_known(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                                 float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                 void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                 const genie_sampling* sampling, const genie_guidance* guidance, const genie_known* known) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_TRY(check_known(known, 1, c.S, "maskgit_generate"));
    GENIE_CHECK_ARG(wt && wt->layers_host && prompt && samples_out, "maskgit_generate: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "maskgit_generate"));
    if (!(out_t >= 1 && out_t < c.T)) {  // assert out_t  (st_mask_git.py:154)
        GENIE_TRY(check_guidance(guidance, cond, "maskgit_generate"));   // (a call refused on both counts reports its guidance)
        set_error("maskgit_generate requires 0 < out_t < T (got %d)", out_t);
        return GENIE_E_ASSERT;
    }
    GENIE_CHECK_ARG(steps >= 1, "maskgit_generate: steps=%d must be >= 1", steps);
    Decode D;
    GENIE_TRY(make_decode(D, B, steps, temperature, unmask_mode, noise, uniforms, sampling, guidance, cond, "maskgit_generate", known));
    // under guidance every forward runs 2 B clips, [conditional ; null], on a doubled copy of the prompt behind the workspace
    const int NB = D.copies * B;
    GENIE_TRY(check_ws(c, NB, workspace, workspace_bytes));
    Workspace w = carve(c, NB, workspace);
    hipStream_t st = as_stream(stream);
    const size_t BS = (size_t)B * c.S;
    const long V = (long)c.factored_vocab * c.num_factored;
    const long clip = (long)c.T * c.S;
    int64_t* frame = prompt + (size_t)out_t * c.S;   // the frame being decoded
    const int64_t* tokens = prompt;                  // what every forward embeds
    genie_frame_cond cond2;
    if (D.guided) {
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
    if (D.known) {   // the frame starts from the known tokens, in the prompt and in both halves of its doubled copy
        GENIE_TRY(launch_known_begin(D.known, D.known_stride, c.image_vocab_size, frame, clip, w.unmasked, B, c.S, 1, st));
        if (D.guided)
            GENIE_TRY(launch_known_begin(D.known, D.known_stride, c.image_vocab_size, const_cast<int64_t*>(tokens) + (size_t)out_t * c.S, clip,
                                         nullptr, B, c.S, 2, st));
    } else if (hipMemsetAsync(w.unmasked, 0, BS, st) != hipSuccess) { set_error("memset failed"); return GENIE_E_LAUNCH; }
    EmbedAct act;
    const EmbedAct* pact = frame_act(cond, c.S, 0, c.T, act);
    for (int step = 0; step < steps; ++step) {
        GENIE_TRY(launch_embed(c, *wt, tokens, NB, w.x, st, pact));
        GENIE_TRY(decoder(c, *wt, w.x, w, NB, st));
        GENIE_TRY(readout(c, *wt, w.x, w, NB, out_t, out_t + 1, GENIE_LAYOUT_TOKEN_MAJOR, w.logits, st));
        if (step == 0 && logits0_out) {  // orig_logits_CHW: step-0 logits are what is returned (:165,226); the guided ones under guidance
            const bool tm = layout == GENIE_LAYOUT_TOKEN_MAJOR;
            if (D.guided) GENIE_TRY(launch_guide_logits(w.logits, logits_null, tm ? logits0_out : logits_g, 1, (long)(BS * V), 0, 0, guidance->scale, st));
            if (tm) {
                if (!D.guided && hipMemcpyAsync(logits0_out, w.logits, BS * V * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                    set_error("memcpy failed");
                    return GENIE_E_LAUNCH;
                }
            } else {
                GENIE_TRY(launch_transpose(D.guided ? logits_g : w.logits, logits0_out, B, c.S, (int)V, st));
            }
        }
        GENIE_TRY(maskgit_step(c, D, B, w.logits, logits_null, w.samples, w.conf, w.unmasked, frame, clip, step, noise, uniforms, D.known, st));
        if (D.guided && step != steps - 1)   // both halves of the next forward see the frame's current tokens
            GENIE_TRY(put_frame_ids(frame, clip, const_cast<int64_t*>(tokens) + (size_t)out_t * c.S, clip, c.S, B, 0, st, 2));
    }
    if (hipMemcpyAsync(samples_out, w.samples, BS * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("memcpy failed");
        return GENIE_E_LAUNCH;
    }
    return GENIE_OK;
}

// The cached generate loop (genie_generate_cached_guided is this with known NULL, _ex with guidance NULL too): B clips decoded, NB per pass
int genie_generate_cached_known(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                                int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance,
                                const genie_known* known) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    GENIE_TRY(check_known(known, n_new, c.S, "generate_cached"));
    GENIE_CHECK_ARG(wt && wt->layers_host && ids && gen_out && cache, "generate_cached: NULL pointer");
    GENIE_TRY(check_frame_cond(cond, "generate_cached"));
    GENIE_CHECK_ARG(B >= 1 && P >= 1 && n_new >= 1 && P + n_new <= c.T && steps >= 1,
                    "generate_cached: B=%d, %d prompt + %d new frames of at most %d, steps %d", B, P, n_new, c.T, steps);
    Decode D;
    GENIE_TRY(make_decode(D, B, steps, temperature, unmask_mode, noise, uniforms, sampling, guidance, cond, "generate_cached", known));
    const int NB = D.copies * B;
    GENIE_CHECK_ARG(cache_bytes >= genie_prefix_cache_bytes(cfg, NB), "generate_cached: cache too small");
    GENIE_TRY(check_ws(c, NB, workspace, workspace_bytes));
    hipStream_t st = as_stream(stream);
    const int S = c.S, T = P + n_new;   // frames per clip in `ids` (the cache keeps the model's c.T slots per clip)
    // scratch of the loop behind the workspace of its largest pass:
    // genie_generate_workspace_bytes / genie_generate_guided_workspace_bytes (cfg, B, P) is the size to allocate
    const GenScratch g = carve_generate(c, B, NB, P, (char*)workspace);
    GENIE_CHECK_ARG(g.end <= workspace_bytes, "generate_cached: workspace too small (%zu < %zu bytes: size it with %s)", workspace_bytes,
                    g.end, D.guided ? "genie_generate_guided_workspace_bytes" : "genie_generate_workspace_bytes");
    PassCtx X = pass_ctx(cfg, wt, NB, cond, cache, cache_bytes, workspace, workspace_bytes, stream);
    genie_frame_cond cond2;
    if (D.guided) {
        GENIE_TRY(put_guided_actions(*cond, *guidance, B, c.T, g.acts, st));
        cond2 = *cond;
        cond2.ids = g.acts;
        X.cond = &cond2;
    }
    // ---- the prompt fills cache slots 0 .. P-1
    for (int t = 0; t < P; ++t)
        GENIE_TRY(put_frame_ids(ids + (size_t)t * S, (long)T * S, g.idsP + (size_t)t * S, (long)P * S, S, B, 0, st, D.copies));
    GENIE_TRY(run_context(X, g, B, D.copies, P, ids, (long)T * S));
    return decode_slots(X, D, B, g, merge_commit, P, n_new, noise, uniforms, gen_out, (long)n_new * S, logits0_out,
                        teacher_force_time ? ids + (size_t)P * S : nullptr, (long)T * S, nullptr, 0, D.known);
}

extern "C" {

size_t genie_generate_workspace_bytes(const genie_cfg* cfg, int B, int P) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || P < 1 || P > cfg->T) return 0;
    return loop_bytes(carve_generate(*cfg, B, B, P, nullptr).end, carve(*cfg, B, nullptr).total);
}

size_t genie_generate_guided_workspace_bytes(const genie_cfg* cfg, int B, int P) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || B > 0x3fffffff || P < 1 || P > cfg->T) return 0;
    return loop_bytes(carve_generate(*cfg, B, 2 * B, P, nullptr).end, carve_guided_prompt(*cfg, 2 * B, nullptr).end);
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

int genie_generate_cached_guided(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                                 int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                 int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                                 size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                                 const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    return genie_generate_cached_known(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time,
                                       merge_commit, gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream, cond,
                                       sampling, guidance, nullptr);
}

int genie_generate_cached_ex(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int P, int n_new,
                             int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                             int teacher_force_time, int merge_commit, int64_t* gen_out, float* logits0_out, float* cache,
                             size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                             const genie_frame_cond* cond, const genie_sampling* sampling) {
    return genie_generate_cached_guided(cfg, wt, ids, B, P, n_new, steps, temperature, unmask_mode, noise, uniforms, teacher_force_time,
                                        merge_commit, gen_out, logits0_out, cache, cache_bytes, workspace, workspace_bytes, stream, cond,
                                        sampling, nullptr);
}

size_t genie_rollout_workspace_bytes(const genie_cfg* cfg, int B, int ctx_max, int guided) {
    if (check_cfg(cfg) != GENIE_OK || B < 1 || B > 0x3fffffff || ctx_max < 1 || ctx_max > cfg->T - 1) return 0;
    const int NB = guided ? 2 * B : B;
    return loop_bytes(carve_generate(*cfg, B, NB, ctx_max, nullptr, true).end,
                      guided ? carve_guided_prompt(*cfg, NB, nullptr).end : carve(*cfg, B, nullptr).total);
}

int genie_rollout_cached(const genie_cfg* cfg, const genie_weights* wt, int64_t* frames, int B, int P, int keep, int cap, int f0, int f1,
                         int resume, int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                         int merge_commit, float* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, void* stream,
                         const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    return genie_rollout_cached_known(cfg, wt, frames, B, P, keep, cap, f0, f1, resume, steps, temperature, unmask_mode, noise, uniforms,
                                      merge_commit, cache, cache_bytes, workspace, workspace_bytes, stream, cond, sampling, guidance, nullptr);
}

int genie_rollout_cached_known(const genie_cfg* cfg, const genie_weights* wt, int64_t* frames, int B, int P, int keep, int cap, int f0,
                               int f1, int resume, int steps, float temperature, int unmask_mode, const float* noise,
                               const float* uniforms, int merge_commit, float* cache, size_t cache_bytes, void* workspace,
                               size_t workspace_bytes, void* stream, const genie_frame_cond* cond, const genie_sampling* sampling,
                               const genie_guidance* guidance, const genie_known* known) {
    GENIE_TRY(check_cfg(cfg));
    const genie_cfg& c = *cfg;
    const int T = c.T, S = c.S;
    GENIE_CHECK_ARG(B >= 1 && steps >= 1, "rollout_cached: B=%d, steps %d", B, steps);
    GENIE_CHECK_ARG(P >= 1 && P <= T - 1, "rollout_cached: %d prompt frames outside [1, %d]", P, T - 1);
    GENIE_CHECK_ARG(keep >= 1 && keep <= T - 1, "rollout_cached: keep %d outside [1, %d]", keep, T - 1);
    GENIE_CHECK_ARG(P <= f0 && f0 < f1 && f1 <= cap, "rollout_cached: frames [%d, %d) must lie in [%d prompt frames, cap %d]", f0, f1, P, cap);
    GENIE_CHECK_ARG(resume == 0 || resume == 1, "rollout_cached: resume %d must be 0 or 1", resume);
    GENIE_TRY(check_known(known, (long)f1 - f0, S, "rollout_cached"));
    GENIE_TRY(check_frame_cond(cond, "rollout_cached"));
    Decode D;
    GENIE_TRY(make_decode(D, B, steps, temperature, unmask_mode, noise, uniforms, sampling, guidance, cond, "rollout_cached", known));
    GENIE_CHECK_ARG(wt && wt->layers_host && frames && cache, "rollout_cached: NULL pointer");
    const int NB = D.copies * B, hop = T - keep;
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
    const GenScratch g = carve_generate(c, B, NB, ctx_need, (char*)workspace, true);
    GENIE_CHECK_ARG(g.end <= workspace_bytes, "rollout_cached: workspace too small (%zu < %zu bytes: size it with "
                    "genie_rollout_workspace_bytes for a context of %d frames)", workspace_bytes, g.end, ctx_need);
    hipStream_t st = as_stream(stream);
    PassCtx X = pass_ctx(cfg, wt, NB, cond, cache, cache_bytes, workspace, workspace_bytes, stream);
    const bool acts = cond && cond->n_actions > 0;
    genie_frame_cond cond2;
    if (acts) {   // the passes read the window's actions, (NB, T) with the clip stride they expect
        cond2 = *cond;
        cond2.ids = g.acts;
        X.cond = &cond2;
    }
    const long stride = (long)cap * S;
    for (int f = f0; f < f1;) {
        const int start = start_of(f), end = start + T < f1 ? start + T : f1;
        const bool fresh = f != f0 || fresh0;   // the window's context is run from `frames`; else frame f - 1 is pending in the cache
        const int ctx = fresh ? f - start : 0;
        GENIE_TRY(put_rollout_window(frames, acts ? cond->ids : nullptr, g.idsP, acts ? g.acts : nullptr, B, D.copies, ctx, S, T, cap, start,
                                     D.guided ? guidance->null_action : 0, st));
        if (fresh) GENIE_TRY(run_context(X, g, B, D.copies, ctx, frames + (size_t)start * S, stride));
        GENIE_TRY(decode_slots(X, D, B, g, merge_commit, f - start, end - f, noise ? noise + (size_t)(f - f0) * (steps - 1) * B * S : nullptr,
                               uniforms ? uniforms + (size_t)(f - f0) * steps * c.num_factored * B * S : nullptr, frames + (size_t)f * S,
                               stride, nullptr, nullptr, 0, fresh ? nullptr : frames + (size_t)(f - 1) * S, stride,
                               D.known ? D.known + (size_t)(f - f0) * S : nullptr));
        f = end;
    }
    return GENIE_OK;
}

// ---- fan-out generation: K futures per clip over one shared context cache ------------------------------------------------
size_t genie_fanout_branch_bytes(const genie_cfg* cfg, int NB, int K, int n_new) {
    if (check_cfg(cfg) != GENIE_OK || !fanout_clips(NB, K, 1) || n_new < 1 || n_new > cfg->T - 1) return 0;
    return fanout_branch_bytes(*cfg, (size_t)NB * K, n_new);
}

size_t genie_fanout_workspace_bytes(const genie_cfg* cfg, int B, int K, int P, int guided) {
    if (check_cfg(cfg) != GENIE_OK || !fanout_clips(B, K, guided ? 2 : 1) || P < 1 || P > cfg->T - 1) return 0;
    const int NB = guided ? 2 * B : B;
    return loop_bytes(carve_fanout(*cfg, B, NB, K, P, nullptr).end, carve(*cfg, NB, nullptr).total);
}

int genie_generate_fanout(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int K, int P, int n_new, int steps,
                          float temperature, int unmask_mode, const float* noise, const float* uniforms, int merge_commit, int64_t* gen_out,
                          float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, const genie_frame_cond* cond, const genie_sampling* sampling, const genie_guidance* guidance) {
    return genie_generate_fanout_known(cfg, wt, ids, B, K, P, n_new, steps, temperature, unmask_mode, noise, uniforms, merge_commit, gen_out,
                                       trunk, trunk_bytes, branch, branch_bytes, workspace, workspace_bytes, stream, cond, sampling, guidance,
                                       nullptr);
}

int genie_generate_fanout_known(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int K, int P, int n_new,
                                int steps, float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                int merge_commit, int64_t* gen_out, float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes,
                                void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                const genie_sampling* sampling, const genie_guidance* guidance, const genie_known* known) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_TRY(check_known(known, n_new, cfg->S, "generate_fanout"));
    GENIE_TRY(check_frame_cond(cond, "generate_fanout"));
    GENIE_CHECK_ARG(B >= 1 && K >= 1 && P >= 1 && n_new >= 1 && P + n_new <= cfg->T && steps >= 1,
                    "generate_fanout: B=%d, K=%d, %d prompt + %d new frames of at most %d, steps %d", B, K, P, n_new, cfg->T, steps);
    Decode D;
    GENIE_TRY(make_decode(D, B, steps, temperature, unmask_mode, noise, uniforms, sampling, guidance, cond, "generate_fanout", known));
    FanCall F;
    GENIE_TRY(fanout_prologue("generate_fanout", "genie_fanout_workspace_bytes", cfg, wt, ids, (long)P * cfg->S, gen_out, B, K, P, n_new,
                              D.copies, D.guided ? guidance->null_action : 0, trunk, trunk_bytes, branch, branch_bytes, workspace,
                              workspace_bytes, stream, cond, F));
    // ... then the loop of genie_generate_cached decodes B * K clips over the split cache, starting at slot P with nothing pending
    return decode_slots(F.br, D, B * K, F.g, merge_commit, P, n_new, noise, uniforms, gen_out, (long)n_new * cfg->S, nullptr, nullptr, 0,
                        nullptr, 0, D.known);
}

// ---- scoring observed futures: per-(clip, branch, frame) NLL over the fan-out cache ----------------------------------------
size_t genie_score_workspace_bytes(const genie_cfg* cfg, int B, int K, int P) { return genie_fanout_workspace_bytes(cfg, B, K, P, 0); }

int genie_score_fanout(const genie_cfg* cfg, const genie_weights* wt, const int64_t* ids, int B, int K, int P, int n, int merge_commit,
                       double* nll, double* hits, float* token_nll, float* trunk, size_t trunk_bytes, float* branch, size_t branch_bytes,
                       void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond) {
    GENIE_TRY(check_cfg(cfg));
    GENIE_TRY(check_frame_cond(cond, "score_fanout"));
    GENIE_CHECK_ARG(B >= 1 && K >= 1 && P >= 1 && n >= 1 && P + n <= cfg->T, "score_fanout: B=%d, K=%d, %d prompt + %d scored frames of at most %d",
                    B, K, P, n, cfg->T);
    const long clip = (long)(P + n) * cfg->S;   // ids (B, P + n, S)
    FanCall F;
    GENIE_TRY(fanout_prologue("score_fanout", "genie_score_workspace_bytes", cfg, wt, ids, clip, nll, B, K, P, n, 1, 0, trunk, trunk_bytes,
                              branch, branch_bytes, workspace, workspace_bytes, stream, cond, F));
    return score_slots(F.br, F.g, merge_commit, P, n, ids + (size_t)P * cfg->S, clip, K, nll, hits, token_nll);
}

// ---- the full-forward MaskGIT loop -------------------------------------------------------------------------------------------
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

int genie_maskgit_generate_guided(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                                  float temperature, int unmask_mode, const float* noise, const float* uniforms,
                                  int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                                  void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                                  const genie_sampling* sampling, const genie_guidance* guidance) {
    return genie_maskgit_generate_known(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out, logits0_out,
                                        layout, status_flag, workspace, workspace_bytes, stream, cond, sampling, guidance, nullptr);
}

int genie_maskgit_generate_ex(const genie_cfg* cfg, const genie_weights* wt, int64_t* prompt, int B, int out_t, int steps,
                              float temperature, int unmask_mode, const float* noise, const float* uniforms,
                              int64_t* samples_out, float* logits0_out, int layout, int32_t* status_flag,
                              void* workspace, size_t workspace_bytes, void* stream, const genie_frame_cond* cond,
                              const genie_sampling* sampling) {
    return genie_maskgit_generate_guided(cfg, wt, prompt, B, out_t, steps, temperature, unmask_mode, noise, uniforms, samples_out, logits0_out,
                                         layout, status_flag, workspace, workspace_bytes, stream, cond, sampling, nullptr);
}

}  // extern "C"
