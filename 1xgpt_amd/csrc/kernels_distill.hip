// Distillation in the fused loss kernel (include/genie_hip.h, "Distillation"): the general objective of kernels_train.hip with a second,
// read-only row of TEACHER logits beside every student row.  Per counted token and factor, with mix alpha and temperature tau:
//   l_f = (1 - alpha) hard_f + alpha tau^2 KL(r || pt) + zeta lse^2,   r = softmax(u / tau), pt = softmax(z / tau)
//   d l_f / d z_k = (1 - alpha)(p_k - q_k) + 2 zeta lse p_k + alpha tau (pt_k - r_k)
//   sums = [sum w l, sum hits, W, sum plain nll, n, sum plain kd, sum teacher plain nll]; entries 1, 3, 5, 6 over ALL counted tokens
// count_frames_kernel (kernels_train.hip) runs first, as launched for the objective: it writes W and n.
//
// The mapping is ce_objective_kernel's: one wave per token, four tokens per 256-thread workgroup, lane l owns classes l + 64 j -- but a
// launch has at most DISTILL_MAX_GRID workgroups, each walking its share of the four-token groups and adding its sums up in registers.
// REG (vf <= 512): a factor's eight student and eight teacher values per lane are requested together, before the first use of either,
// and stay in registers: each row comes from memory once, 12 bytes per logit element (student read + write, teacher read).  Else three
// streaming passes (extrema; sums; elements), the teacher row riding in each.  TAU1 (tau == 1): pt = p and the teacher's tempered
// sum is its plain one, so the second exponential of both rows is never computed.
// log r_k and log pt_k are taken in log-softmax form, (u_k - max u) / tau - log sum: a probability that underflowed to 0 multiplies a
// finite number.  No atomics on d logits (the same bytes run to run); the five accumulated sums use double atomics, as the objective's.
#include "kernels.hpp"

namespace genie {

// a value every lane holds alike, moved to a scalar register: the per-token and per-factor constants (a wave is one token) otherwise
// take a vector register each (compiled without it: 104 / 117 / 71 / 79 VGPRs against 102 / 114 / 64 / 71, one wave per SIMD less in
// the streaming kernel at any tau)
__device__ __forceinline__ float uni(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

template <bool REG, bool TAU1>
__global__ __launch_bounds__(256) void ce_distill_kernel(float* __restrict__ logits, const float* __restrict__ teacher,
                                                         const int64_t* __restrict__ ids, const int64_t* __restrict__ labels,
                                                         long n_tok, int T, int S, int vf, int nfac, int64_t mask_id, float eps,
                                                         float zeta, float alpha, float tau, FrameWeights fw,
                                                         double* __restrict__ sums) {
    __shared__ double red[5][4];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double obj = 0, hit = 0, ce = 0, kd = 0, tce = 0;
    // a workgroup walks the groups of four tokens blockIdx.x, blockIdx.x + gridDim.x, ... and adds its sums up in registers: the five
    // double atomics at its end all land in one cache line, and with one set per FOUR-token group (the objective kernel's grid) this body
    // took 2.7 times as long at 32,768 tokens (profiles/train_distill.txt)
    for (long n = (long)blockIdx.x * 4 + wid; n < n_tok; n += (long)gridDim.x * 4) {
        float* lp = logits + (size_t)n * vf * nfac;
        const float* tp = teacher + (size_t)n * vf * nfac;
        const int t = (int)((n / S) % T);
        const bool counted = t >= 1 && ids[n] == mask_id;
        if (!counted) {
            for (int k = lane; k < vf * nfac; k += 64) lp[k] = 0.f;
        } else {
            const float wt = fw.at(t);
            const bool live = wt > 0.0f;   // a zero-weight frame: counted in hits, plain nll, kd and teacher nll; a zero row
            const float wgt = uni(live ? (float)((double)wt / sums[2]) : 0.0f);
            const float q_off = uni(eps / (float)vf), q_on = uni((1.0f - eps) + q_off), inv_vf = uni(1.0f / (float)vf);
            const float oma = uni(1.0f - alpha), at = uni(alpha * tau), inv_tau = uni(1.0f / tau);
            int64_t tgt = labels[n];
            float nll = 0.f, loss = 0.f, kdt = 0.f, tnll = 0.f;
            bool all_ok = true;
            for (int f = 0; f < nfac; ++f) {
                const int tf = (int)(tgt % vf);
                tgt /= vf;
                float* lf = lp + f * vf;
                const float* uf = tp + f * vf;
                // d: z - max, then (TAU1: the same) (z - max) / tau;  e: exp(z - max);  et: exp((z - max) / tau)
                // c: (u - max u) / tau, then c - d;  ru: exp((u - max u) / tau)
                float d[REG ? 8 : 1], e[REG ? 8 : 1], et[(REG && !TAU1) ? 8 : 1], c[REG ? 8 : 1], ru[REG ? 8 : 1];
                float mx = -INFINITY, mu = -INFINITY, sz = 0.f;
                int mi = 0;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {   // sixteen requests in flight before the first use
                        const int k = lane + 64 * j;
                        d[j] = k < vf ? lf[k] : -INFINITY;
                        c[j] = k < vf ? uf[k] : -INFINITY;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        if (k < vf) sz += d[j];
                        if (d[j] > mx) { mx = d[j]; mi = k; }
                        mu = fmaxf(mu, c[j]);
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float x = lf[k];
                        sz += x;
                        if (x > mx) { mx = x; mi = k; }
                        mu = fmaxf(mu, uf[k]);
                    }
                }
                wave_argmax(mx, mi);
                mx = uni(mx);
                mi = __builtin_amdgcn_readfirstlane(mi);
                mu = uni(wave_max(mu));
                const float zy = uni(lf[tf]), uy = uni(uf[tf]);   // z_y is read before any lane stores into the row
                float se = 0.f, st = 0.f, su = 0.f, su1 = 0.f;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (lane + 64 * j < vf) {
                            d[j] -= mx;
                            e[j] = expf(d[j]);
                            se += e[j];
                            c[j] -= mu;
                            if (!TAU1) {
                                su1 += expf(c[j]);
                                d[j] *= inv_tau;
                                c[j] *= inv_tau;
                                et[j] = expf(d[j]);
                                st += et[j];
                            }
                            ru[j] = expf(c[j]);
                            su += ru[j];
                            c[j] -= d[j];   // the KL term needs the difference alone
                        }
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float dz = lf[k] - mx, du = uf[k] - mu;
                        se += expf(dz);
                        if (!TAU1) {
                            su1 += expf(du);
                            st += expf(dz * inv_tau);
                            su += expf(du * inv_tau);
                        } else {
                            su += expf(du);
                        }
                    }
                }
                se = uni(wave_sum(se));
                su = uni(wave_sum(su));
                if (!TAU1) { st = uni(wave_sum(st)); su1 = uni(wave_sum(su1)); }
                sz = uni(wave_sum(sz));
                const float log_se = uni(logf(se)), log_su = uni(logf(su));
                const float log_st = TAU1 ? log_se : uni(logf(st));
                const float lse = uni(log_se + mx);
                const float nll_f = lse - zy;
                nll += nll_f;
                tnll += ((TAU1 ? log_su : logf(su1)) + mu) - uy;
                all_ok = all_ok && (mi == tf);
                const float inv = uni(1.0f / se), inv_st = TAU1 ? inv : uni(1.0f / st), inv_su = uni(1.0f / su),
                            zl2 = uni((2.0f * zeta) * lse), dlog = uni(log_su - log_st);
                float kl = 0.f;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        if (k < vf) {
                            const float p = e[j] * inv, pt = TAU1 ? p : et[j] * inv_st, r = ru[j] * inv_su;
                            kl += r * (c[j] - dlog);
                            const float g = (oma * (p - (k == tf ? q_on : q_off)) + zl2 * p) + at * (pt - r);
                            lf[k] = live ? g * wgt : 0.f;
                        }
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float dz = lf[k] - mx, du = uf[k] - mu;
                        const float p = expf(dz) * inv;
                        const float dzt = TAU1 ? dz : dz * inv_tau, dut = TAU1 ? du : du * inv_tau;
                        const float pt = TAU1 ? p : expf(dzt) * inv_st, r = expf(dut) * inv_su;
                        kl += r * ((dut - dzt) - dlog);
                        const float g = (oma * (p - (k == tf ? q_on : q_off)) + zl2 * p) + at * (pt - r);
                        lf[k] = live ? g * wgt : 0.f;
                    }
                }
                const float kd_f = uni((tau * tau) * wave_sum(kl));
                kdt += kd_f;
                const float hard_f = (1.0f - eps) * nll_f + eps * (lse - sz * inv_vf);
                loss += (oma * hard_f + alpha * kd_f) + zeta * (lse * lse);
            }
            if (lane == 0) {
                obj += (double)wt * (double)loss;
                hit += all_ok ? 1.0 : 0.0;
                ce += nll;
                kd += kdt;
                tce += tnll;
            }
        }
    }
    if (lane == 0) { red[0][wid] = obj; red[1][wid] = hit; red[2][wid] = ce; red[3][wid] = kd; red[4][wid] = tce; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a[5];
        for (int i = 0; i < 5; ++i) {
            a[i] = 0;
            for (int w = 0; w < 4; ++w) a[i] += red[i][w];
        }
        if (a[0] != 0.0) atomicAdd(&sums[0], a[0]);
        if (a[1] != 0.0) atomicAdd(&sums[1], a[1]);
        if (a[2] != 0.0) atomicAdd(&sums[3], a[2]);
        if (a[3] != 0.0) atomicAdd(&sums[5], a[3]);
        if (a[4] != 0.0) atomicAdd(&sums[6], a[4]);
    }
}

// workgroups of a launch at most: eight per CU of a 256-CU device, each walking its share of the token groups
constexpr long DISTILL_MAX_GRID = 2048;

int launch_ce_distill(float* logits, const float* teacher, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S,
                      int vf, int nfac, int64_t mask_id, const genie_objective& obj, float alpha, float tau, double* sums,
                      hipStream_t st) {
    const long n_tok = n_clips * T * (long)S;
    if (n_tok <= 0) return GENIE_OK;
    const FrameWeights fw = frame_weights_of(obj);
    GENIE_TRY(launch_count_frames(ids, n_clips, T, S, mask_id, fw, sums, st));
    // (an upper bound, as the objective kernel's 8: the host does not know how many tokens are counted, and an uncounted token's row is
    // only written -- 4 bytes per element, not 12)
    ProfScope prof(GENIE_KC_OTHER, 0.0, 12.0 * n_tok * vf * nfac, st, "ce_distill_kernel");
    const unsigned grid = (unsigned)std::min<long>((n_tok + 3) / 4, DISTILL_MAX_GRID);
#define GENIE_DISTILL_LAUNCH(REG, TAU1)                                                                                         \
    ce_distill_kernel<REG, TAU1><<<grid, 256, 0, st>>>(logits, teacher, ids, labels, n_tok, T, S, vf, nfac, mask_id,            \
                                                       obj.label_smoothing, obj.z_loss, alpha, tau, fw, sums)
    if (vf <= 512) {
        if (tau == 1.0f) GENIE_DISTILL_LAUNCH(true, true);
        else GENIE_DISTILL_LAUNCH(true, false);
    } else {
        if (tau == 1.0f) GENIE_DISTILL_LAUNCH(false, true);
        else GENIE_DISTILL_LAUNCH(false, false);
    }
#undef GENIE_DISTILL_LAUNCH
    GENIE_LAUNCH_CHECK("ce_distill");
    return GENIE_OK;
}

}  // namespace genie
