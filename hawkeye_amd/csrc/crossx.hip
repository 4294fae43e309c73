// CrossX head (one-squeeze multi-excitation blocks, the combined branch's upsample + add, the loss that ties the three
// classifiers together).  replaces model/methods/CrossX.py:109-119 and :225-226 (a clone, P broadcast multiplies, P + 1
// residual adds, P + 1 ReLUs and P pools as separate passes over [B,1024,28,28] and [B,2048,14,14] maps), :213-223 (a
// nearest-upsampled [B,1024,28,28] map per part, written only to be added to another) and model/loss/CrossX_loss.py:15-64
// (a P x P correlation matrix filled on the host, entry by entry: 3 P^2 device-to-host copies per step).
//
//   me     one wave per (sample, channel) row of HW elements, four rows per workgroup.  Lane l owns the elements 4 l .. 4 l + 3,
//          then + 256, ..: one 16-byte access per operand where HW % 4 == 0 and every pointer is 16-byte aligned, scalar
//          accesses with the same element-to-lane map otherwise - so both paths sum the mean in the same order and give the
//          same bits.  Forward: `out` and `res` are read once, the main map and the P part maps written once, and each
//          part's spatial max (lowest index on ties, as AdaptiveMaxPool2d) or mean leaves with a wave butterfly.  Backward:
//          every saved map and every map gradient is read once, d_out and d_res written once; the pooled gradient enters
//          per element (a broadcast, or a hit on the arg-max) and is never a map; d_gates leaves with a wave butterfly.
//          The products are not contracted into fmas: `out * gate + res` rounds the product as the reference's two ops do.
//   up_add a thread per four neighbouring outputs (one per output where Wo % 4 != 0 or a pointer is not aligned) forward;
//          a thread per source pixel backward, its children added row by row, left to right.
//   loss   one workgroup of 16 waves.  A wave per sample: the statistics of its four logit rows (the three classifiers and
//          their sum), the smoothed cross entropy, both KL terms and the three logit gradients.  A wave per feature row:
//          1 / norm.  A barrier.  A thread per feature column: s_i = sum_b u_i[b] for its P parts, the regulariser's
//          direction g_i, and its share of |s_i|^2 and s_i . s_j, which a fixed-order block sum collects.  A barrier.  A wave
//          per feature row: the gradient through the normalisation.  Wave 0 adds the terms.  One launch, no atomics.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int CX_MAX_P = 3;
constexpr int ME_THREADS = 256;
constexpr int ME_WAVES = ME_THREADS / WAVE;

__device__ __forceinline__ float cx_relu(float v) { return v > 0.f ? v : (v == v ? 0.f : v); }      // a NaN stays one, as torch's relu keeps it

template <int P, int MODE, bool VEC>
__global__ __launch_bounds__(ME_THREADS) void crossx_me_fwd_kernel(const float* __restrict__ out, const float* __restrict__ res,
                                                                   const float* __restrict__ gates, float* __restrict__ mainmap,
                                                                   float* __restrict__ parts, float* __restrict__ pooled,
                                                                   int32_t* __restrict__ argmax, long long rows, int HW) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * ME_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                               // wave-uniform; no barrier below
    const size_t base = (size_t)row * HW, pstride = (size_t)rows * HW;
    float g[P], acc[P];
    int idx[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        g[p] = gates[(size_t)p * rows + row];
        acc[p] = MODE == 0 ? -INFINITY : 0.f;
        idx[p] = 0x7fffffff;
    }
    for (int i = lane * 4; i < HW; i += ROW_STEP) {
        const f32x4 o = load4<VEC>(out + base, i, HW), r = load4<VEC>(res + base, i, HW);
        f32x4 m;
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = cx_relu(o[e] + r[e]);
        store4<VEC>(mainmap + base, i, HW, m);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = cx_relu(o[e] * g[p] + r[e]);
            store4<VEC>(parts + p * pstride + base, i, HW, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!VEC && i + e >= HW) continue;
                if (MODE == 0) {
                    if (v[e] > acc[p] || (v[e] != v[e] && acc[p] == acc[p])) { acc[p] = v[e]; idx[p] = i + e; }     // ascending: the lowest index
                } else {
                    acc[p] += v[e];
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (MODE == 0) {
            float a = acc[p];
            int k = idx[p];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float oa = __shfl_xor(a, s, 64);
                const int ok = __shfl_xor(k, s, 64);
                const bool an = a != a, on = oa != oa;
                const bool take = (on && !an) || (on == an && (oa > a || ((oa == a || on) && ok < k)));
                if (take) { a = oa; k = ok; }
            }
            if (lane == 0) {
                pooled[(size_t)p * rows + row] = a;
                argmax[(size_t)p * rows + row] = k;
            }
        } else {
            const float a = wave_sum(acc[p]);
            if (lane == 0) pooled[(size_t)p * rows + row] = a / (float)HW;
        }
    }
}

template <int P, int MODE, bool VEC>
__global__ __launch_bounds__(ME_THREADS) void crossx_me_bwd_kernel(const float* __restrict__ d_main, const float* __restrict__ d_parts,
                                                                   const float* __restrict__ d_pooled, const int32_t* __restrict__ argmax,
                                                                   const float* __restrict__ dz, const float* __restrict__ out,
                                                                   const float* __restrict__ gates, const float* __restrict__ mainmap,
                                                                   const float* __restrict__ parts, float* __restrict__ d_out,
                                                                   float* __restrict__ d_res, float* __restrict__ d_gates, long long rows,
                                                                   int HW) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * ME_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * HW, pstride = (size_t)rows * HW;
    float g[P], dp[P], dg[P];
    int am[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        g[p] = gates[(size_t)p * rows + row];
        dp[p] = d_pooled ? d_pooled[(size_t)p * rows + row] : 0.f;
        if (MODE == 1) dp[p] = dp[p] / (float)HW;
        am[p] = (MODE == 0 && d_pooled) ? argmax[(size_t)p * rows + row] : -1;
        dg[p] = 0.f;
    }
    const float zadd = dz ? dz[row] / (float)HW : 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane * 4; i < HW; i += ROW_STEP) {
        const f32x4 o = load4<VEC>(out + base, i, HW), m = load4<VEC>(mainmap + base, i, HW);
        const f32x4 dm = d_main ? load4<VEC>(d_main + base, i, HW) : zero;
        f32x4 dout, dres;
#pragma unroll
        for (int e = 0; e < 4; ++e) dout[e] = dres[e] = m[e] > 0.f ? dm[e] : 0.f;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const f32x4 v = load4<VEC>(parts + p * pstride + base, i, HW);
            const f32x4 dv = d_parts ? load4<VEC>(d_parts + p * pstride + base, i, HW) : zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pool = MODE == 1 ? dp[p] : (i + e == am[p] ? dp[p] : 0.f);
                const float gg = v[e] > 0.f ? dv[e] + pool : 0.f;
                dout[e] += g[p] * gg;
                dres[e] += gg;
                dg[p] += gg * o[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) dout[e] += zadd;
        store4<VEC>(d_out + base, i, HW, dout);
        store4<VEC>(d_res + base, i, HW, dres);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float s = wave_sum(dg[p]);
        if (lane == 0) d_gates[(size_t)p * rows + row] = s;
    }
}

// ------------------------------------------------------------------------------------------------- upsample + add
constexpr int UP_THREADS = 256;

template <int VEC>
__global__ __launch_bounds__(UP_THREADS) void crossx_up_add_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                       float* __restrict__ y, long long groups, int Hi, int Wi, int Ho,
                                                                       int Wo, int fh, int fw) {
    const long long q = (long long)blockIdx.x * UP_THREADS + threadIdx.x;
    if (q >= groups) return;
    const int qw = Wo / VEC;
    const int ox = (int)(q % qw) * VEC;
    const long long t = q / qw;
    const int oy = (int)(t % Ho);
    const long long plane = t / Ho;
    const float* src = b + ((size_t)plane * Hi + oy / fh) * Wi;
    const size_t at = ((size_t)plane * Ho + oy) * Wo + ox;
    if (VEC == 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(a + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += src[(ox + e) / fw];
        *reinterpret_cast<f32x4*>(y + at) = v;
    } else {
        y[at] = a[at] + src[ox / fw];
    }
}

__global__ __launch_bounds__(UP_THREADS) void crossx_up_add_bwd_kernel(const float* __restrict__ dy, float* __restrict__ db,
                                                                       long long total, int Hi, int Wi, int Wo, int fh, int fw) {
    const long long q = (long long)blockIdx.x * UP_THREADS + threadIdx.x;
    if (q >= total) return;
    const int ix = (int)(q % Wi);
    const long long t = q / Wi;                            // plane Hi + iy
    const float* g = dy + ((size_t)t * fh) * Wo + (size_t)ix * fw;
    float s = 0.f;
    for (int r = 0; r < fh; ++r)
        for (int c = 0; c < fw; ++c) s += g[(size_t)r * Wo + c];
    db[q] = s;
}

// ------------------------------------------------------------------------------------------------------------- loss
constexpr int CX_LOSS_THREADS = 1024;
constexpr int CX_LOSS_WAVES = CX_LOSS_THREADS / WAVE;
constexpr int CX_MAX_B = 1 << 16;
constexpr long long CX_MAX_WIDTH = 1 << 24;

struct CxLossArgs {
    const float* logits[3];        // ulti, plty, cmbn [B,K]
    const int64_t* labels;         // [B]
    const float* feat[3];          // [P,B,C_l]
    float gamma[3];
    float weight;
    float* loss;                   // [6]
    float* dlogits[3];
    float* dfeat[3];
    int B, K, P, C[3];
    // workspace
    float* sumrow;                 // [B,K]
    float* ce_rows;                // [B]
    float* kl_rows;                // [B]
    float* inv;                    // [3,P,B]
    float* g;                      // [P, C_0 + C_1 + C_2]: list l at column offset C_0 + .. + C_(l-1)
};

__global__ __launch_bounds__(CX_LOSS_THREADS) void crossx_loss_kernel(const CxLossArgs A) {
#pragma clang fp contract(off)
    __shared__ float red[CX_LOSS_WAVES];
    __shared__ float reg[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = A.B, K = A.K, P = A.P;
    const float smoothing = 0.1f;
    const int ctot = A.C[0] + A.C[1] + A.C[2];
    // ---- a wave per sample: cross entropy of the summed logits, both KL terms, the three logit gradients
    for (int b = wave; b < B; b += CX_LOSS_WAVES) {
        const float* u = A.logits[0] + (size_t)b * K;
        const float* p = A.logits[1] + (size_t)b * K;
        const float* c = A.logits[2] + (size_t)b * K;
        float* sum = A.sumrow + (size_t)b * K;
        for (int k = lane; k < K; k += WAVE) sum[k] = (u[k] + p[k]) + c[k];            // read back by the lane that wrote it
        const long long yl = A.labels[b];
        const int y = (yl >= 0 && yl < K) ? (int)yl : -1;
        const CeRow ss = ce_row_stats(sum, K, y, smoothing);
        const CeRow su = ce_row_stats(u, K, -1, 0.f), sp = ce_row_stats(p, K, -1, 0.f), sc = ce_row_stats(c, K, -1, 0.f);
        // t_k = 2 log pu_k - log pp_k - log pc_k ; kl_row = sum_k pu_k t_k = KL(pu | pp) + KL(pu | pc)
        float kl = 0.f;
        for (int k = lane; k < K; k += WAVE) {
            const float lu = (u[k] - su.mx) - su.ls, lp = (p[k] - sp.mx) - sp.ls, lc = (c[k] - sc.mx) - sc.ls;
            kl += expf(u[k] - su.mx) * su.inv * ((lu - lp) + (lu - lc));
        }
        kl = wave_sum(kl);
        const float wb = A.weight / (float)B, us = smoothing / (float)K;
        for (int k = lane; k < K; k += WAVE) {
            const float ps = expf(sum[k] - ss.mx) * ss.inv;
            const float ce = wb * (ps - us - (1.f - smoothing) * (k == y ? 1.f : 0.f));
            const float pu = expf(u[k] - su.mx) * su.inv, pp = expf(p[k] - sp.mx) * sp.inv, pc = expf(c[k] - sc.mx) * sc.inv;
            const float lu = (u[k] - su.mx) - su.ls, lp = (p[k] - sp.mx) - sp.ls, lc = (c[k] - sc.mx) - sc.ls;
            const float t = (lu - lp) + (lu - lc);
            A.dlogits[0][(size_t)b * K + k] = ce + wb * (pu * (t - kl));               // the target carries gradient too
            A.dlogits[1][(size_t)b * K + k] = ce + wb * (pp - pu);
            A.dlogits[2][(size_t)b * K + k] = ce + wb * (pc - pu);
        }
        if (lane == 0) {
            A.ce_rows[b] = ss.ce;
            A.kl_rows[b] = kl;
        }
    }
    // ---- a wave per feature row: 1 / |x_i[b]|
    const int frows = 3 * P * B;
    for (int r = wave; r < frows; r += CX_LOSS_WAVES) {
        const int l = r / (P * B), ib = r - l * P * B;
        const int C = A.C[l];
        const float* x = A.feat[l] + (size_t)ib * C;
        float q = 0.f;
        for (int k = lane; k < C; k += WAVE) q += x[k] * x[k];
        q = wave_sum(q);
        if (lane == 0) A.inv[r] = 1.f / sqrtf(q);
    }
    __syncthreads();
    // ---- a thread per feature column: s_i[c] = sum_b u_i[b][c], g_i[c] = gamma / B^2 (-2 s_i[c] + sum_{j != i} s_j[c])
    const float bb = (float)B * (float)B;
    int off = 0;
    for (int l = 0; l < 3; ++l) {
        const int C = A.C[l];
        float sq[CX_MAX_P] = {0.f, 0.f, 0.f}, cr[CX_MAX_P] = {0.f, 0.f, 0.f};          // |s_i|^2 ; s_0.s_1, s_0.s_2, s_1.s_2
        for (int c = threadIdx.x; c < C; c += CX_LOSS_THREADS) {
            float s[CX_MAX_P] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < CX_MAX_P; ++i) {
                if (i >= P) break;
                const float* x = A.feat[l] + (size_t)i * B * C + c;
                const float* inv = A.inv + (l * P + i) * B;
                float t = 0.f;
                for (int b = 0; b < B; ++b) t += x[(size_t)b * C] * inv[b];
                s[i] = t;
            }
            const float all = (s[0] + s[1]) + s[2];
#pragma unroll
            for (int i = 0; i < CX_MAX_P; ++i) {
                if (i >= P) break;
                A.g[(size_t)i * ctot + off + c] = A.gamma[l] / bb * (-2.f * s[i] + (all - s[i]));
                sq[i] += s[i] * s[i];
            }
            cr[0] += s[0] * s[1];
            cr[1] += s[0] * s[2];
            cr[2] += s[1] * s[2];
        }
        float corr = 0.f;                                  // sum of the upper triangle of the reference's matrix
#pragma unroll
        for (int i = 0; i < CX_MAX_P; ++i)
            if (i < P) corr += 1.f - block_sum<CX_LOSS_WAVES>(sq[i], red) / bb;              // P is uniform: every thread reaches the barriers
        if (P > 1) corr += block_sum<CX_LOSS_WAVES>(cr[0], red) / bb;
        if (P > 2) {
            corr += block_sum<CX_LOSS_WAVES>(cr[1], red) / bb;
            corr += block_sum<CX_LOSS_WAVES>(cr[2], red) / bb;
        }
        if (threadIdx.x == 0) reg[l] = corr * A.gamma[l];
        off += C;
    }
    __syncthreads();
    // ---- a wave per feature row: d x = (g_i - u (u . g_i)) / |x|
    for (int r = wave; r < frows; r += CX_LOSS_WAVES) {
        const int l = r / (P * B), ib = r - l * P * B, i = ib / B;
        const int C = A.C[l];
        const int lo = l == 0 ? 0 : (l == 1 ? A.C[0] : A.C[0] + A.C[1]);
        const float* x = A.feat[l] + (size_t)ib * C;
        const float* g = A.g + (size_t)i * ctot + lo;
        float* dx = A.dfeat[l] + (size_t)ib * C;
        const float inv = A.inv[r];
        float d = 0.f;
        for (int k = lane; k < C; k += WAVE) d += (x[k] * inv) * g[k];
        d = wave_sum(d);
        for (int k = lane; k < C; k += WAVE) dx[k] = A.weight * ((g[k] - (x[k] * inv) * d) * inv);
    }
    if (wave == 0) {
        const float ce = wave_total(A.ce_rows, B), kl = wave_total(A.kl_rows, B);
        if (lane == 0) {
            const float cls = ce / (float)B, klm = kl / (float)B;
            A.loss[0] = (((reg[0] + reg[1]) + reg[2]) + klm) + cls;                    // the reference's order of addition
            A.loss[1] = cls;
            A.loss[2] = klm;
            A.loss[3] = reg[0];
            A.loss[4] = reg[1];
            A.loss[5] = reg[2];
        }
    }
}

template <int P, int MODE>
static int me_fwd_launch(bool vec, unsigned blocks, hipStream_t st, const float* out, const float* res, const float* gates, float* mainmap,
                         float* parts, float* pooled, int32_t* argmax, long long rows, int HW) {
    if (vec)
        hipLaunchKernelGGL((crossx_me_fwd_kernel<P, MODE, true>), dim3(blocks), dim3(ME_THREADS), 0, st, out, res, gates, mainmap, parts,
                           pooled, argmax, rows, HW);
    else
        hipLaunchKernelGGL((crossx_me_fwd_kernel<P, MODE, false>), dim3(blocks), dim3(ME_THREADS), 0, st, out, res, gates, mainmap, parts,
                           pooled, argmax, rows, HW);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

template <int P, int MODE>
static int me_bwd_launch(bool vec, unsigned blocks, hipStream_t st, const float* d_main, const float* d_parts, const float* d_pooled,
                         const int32_t* argmax, const float* dz, const float* out, const float* gates, const float* mainmap,
                         const float* parts, float* d_out, float* d_res, float* d_gates, long long rows, int HW) {
    if (vec)
        hipLaunchKernelGGL((crossx_me_bwd_kernel<P, MODE, true>), dim3(blocks), dim3(ME_THREADS), 0, st, d_main, d_parts, d_pooled, argmax,
                           dz, out, gates, mainmap, parts, d_out, d_res, d_gates, rows, HW);
    else
        hipLaunchKernelGGL((crossx_me_bwd_kernel<P, MODE, false>), dim3(blocks), dim3(ME_THREADS), 0, st, d_main, d_parts, d_pooled, argmax,
                           dz, out, gates, mainmap, parts, d_out, d_res, d_gates, rows, HW);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

static bool me_sizes_ok(int P, int N, int C, int HW, long long& rows, unsigned& blocks) {
    rows = (long long)N * C;
    const long long nb = (rows + ME_WAVES - 1) / ME_WAVES;
    blocks = (unsigned)nb;
    return nb <= 0x7fffffff && HW <= 0x7fffffff - ROW_STEP && P * rows <= 0x7fffffffLL;
}

}  // namespace hk

using namespace hk;

#define CX_ME_DISPATCH(fn, ...)                                                                        \
    switch (P * 2 + mode) {                                                                            \
        case 2: return fn<1, 0>(__VA_ARGS__);                                                          \
        case 3: return fn<1, 1>(__VA_ARGS__);                                                          \
        case 4: return fn<2, 0>(__VA_ARGS__);                                                          \
        case 5: return fn<2, 1>(__VA_ARGS__);                                                          \
        case 6: return fn<3, 0>(__VA_ARGS__);                                                          \
        default: return fn<3, 1>(__VA_ARGS__);                                                         \
    }

extern "C" int hk_crossx_me_fwd(const float* out, const float* res, const float* gates, float* main_out, float* parts, float* pooled,
                                int32_t* argmax, int P, int N, int C, int HW, int mode, hk_stream_t stream) {
    if (!out || !res || !gates || !main_out || !parts || !pooled || N <= 0 || C <= 0 || HW <= 0 || (mode != 0 && mode != 1))
        return HK_ERR_BAD_ARG;
    if (mode == 0 && !argmax) return HK_ERR_BAD_ARG;
    if (P < 1 || P > CX_MAX_P) return HK_ERR_UNSUPPORTED;
    long long rows;
    unsigned blocks;
    if (!me_sizes_ok(P, N, C, HW, rows, blocks)) return HK_ERR_UNSUPPORTED;
    const bool vec = (HW & 3) == 0 && aligned16(out) && aligned16(res) && aligned16(main_out) && aligned16(parts);
    CX_ME_DISPATCH(me_fwd_launch, vec, blocks, (hipStream_t)stream, out, res, gates, main_out, parts, pooled, argmax, rows, HW)
}

extern "C" int hk_crossx_me_bwd(const float* d_main, const float* d_parts, const float* d_pooled, const int32_t* argmax, const float* dz,
                                const float* out, const float* gates, const float* main_saved, const float* parts, float* d_out,
                                float* d_res, float* d_gates, int P, int N, int C, int HW, int mode, hk_stream_t stream) {
    if (!out || !gates || !main_saved || !parts || !d_out || !d_res || !d_gates || N <= 0 || C <= 0 || HW <= 0 || (mode != 0 && mode != 1))
        return HK_ERR_BAD_ARG;
    if (mode == 0 && d_pooled && !argmax) return HK_ERR_BAD_ARG;
    if (P < 1 || P > CX_MAX_P) return HK_ERR_UNSUPPORTED;
    long long rows;
    unsigned blocks;
    if (!me_sizes_ok(P, N, C, HW, rows, blocks)) return HK_ERR_UNSUPPORTED;
    const bool vec = (HW & 3) == 0 && aligned16(out) && aligned16(main_saved) && aligned16(parts) && aligned16(d_out) && aligned16(d_res) &&
                     (!d_main || aligned16(d_main)) && (!d_parts || aligned16(d_parts));
    CX_ME_DISPATCH(me_bwd_launch, vec, blocks, (hipStream_t)stream, d_main, d_parts, d_pooled, argmax, dz, out, gates, main_saved, parts,
                   d_out, d_res, d_gates, rows, HW)
}

static int up_add_sizes(int N, int C, int Hi, int Wi, int Ho, int Wo, long long& planes) {
    if (N <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return HK_ERR_BAD_ARG;
    if (Ho % Hi != 0 || Wo % Wi != 0) return HK_ERR_UNSUPPORTED;
    planes = (long long)N * C;
    if (planes * Ho * (long long)Wo / UP_THREADS >= 0x7fffffffLL) return HK_ERR_UNSUPPORTED;
    return HK_OK;
}

extern "C" int hk_crossx_up_add_fwd(const float* a, const float* b, float* y, int N, int C, int Hi, int Wi, int Ho, int Wo,
                                    hk_stream_t stream) {
    if (!a || !b || !y) return HK_ERR_BAD_ARG;
    long long planes;
    const int rc = up_add_sizes(N, C, Hi, Wi, Ho, Wo, planes);
    if (rc != HK_OK) return rc;
    const bool vec = (Wo & 3) == 0 && aligned16(a) && aligned16(y);
    const long long groups = planes * Ho * (vec ? Wo / 4 : Wo);
    const dim3 grid((unsigned)((groups + UP_THREADS - 1) / UP_THREADS)), block(UP_THREADS);
    if (vec)
        hipLaunchKernelGGL((crossx_up_add_fwd_kernel<4>), grid, block, 0, (hipStream_t)stream, a, b, y, groups, Hi, Wi, Ho, Wo, Ho / Hi, Wo / Wi);
    else
        hipLaunchKernelGGL((crossx_up_add_fwd_kernel<1>), grid, block, 0, (hipStream_t)stream, a, b, y, groups, Hi, Wi, Ho, Wo, Ho / Hi, Wo / Wi);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_crossx_up_add_bwd(const float* dy, float* db, int N, int C, int Hi, int Wi, int Ho, int Wo, hk_stream_t stream) {
    if (!dy || !db) return HK_ERR_BAD_ARG;
    long long planes;
    const int rc = up_add_sizes(N, C, Hi, Wi, Ho, Wo, planes);
    if (rc != HK_OK) return rc;
    const long long total = planes * Hi * Wi;
    hipLaunchKernelGGL(crossx_up_add_bwd_kernel, dim3((unsigned)((total + UP_THREADS - 1) / UP_THREADS)), dim3(UP_THREADS), 0,
                       (hipStream_t)stream, dy, db, total, Hi, Wi, Wo, Ho / Hi, Wo / Wi);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

static bool cx_loss_sizes_ok(int B, int K, int P, int C0, int C1, int C2) {
    return B <= CX_MAX_B && K <= CX_MAX_WIDTH && C0 <= CX_MAX_WIDTH && C1 <= CX_MAX_WIDTH && C2 <= CX_MAX_WIDTH &&
           (long long)B * K <= 0x7fffffffLL && (long long)P * B * C0 <= 0x7fffffffLL && (long long)P * B * C1 <= 0x7fffffffLL &&
           (long long)P * B * C2 <= 0x7fffffffLL;
}

static size_t cx_loss_ws_need(int B, int K, int P, int C0, int C1, int C2) {
    const size_t ctot = (size_t)C0 + C1 + C2;
    return ((size_t)B * K + 2 * (size_t)B + 3 * (size_t)P * B + (size_t)P * ctot) * sizeof(float) + 256;
}

extern "C" size_t hk_crossx_loss_ws_bytes(int B, int K, int P, int C0, int C1, int C2) {
    if (B < 2 || K <= 0 || P < 1 || P > CX_MAX_P || C0 <= 0 || C1 <= 0 || C2 <= 0 || !cx_loss_sizes_ok(B, K, P, C0, C1, C2)) return 0;
    return cx_loss_ws_need(B, K, P, C0, C1, C2);
}

extern "C" int hk_crossx_loss(const float* ulti, const float* plty, const float* cmbn, const int64_t* labels, const float* f_ulti,
                              const float* f_plty, const float* f_cmbn, float gamma_ulti, float gamma_plty, float gamma_cmbn, float weight,
                              float* loss, float* d_ulti, float* d_plty, float* d_cmbn, float* df_ulti, float* df_plty, float* df_cmbn, int B,
                              int K, int P, int C_ulti, int C_plty, int C_cmbn, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!ulti || !plty || !cmbn || !labels || !f_ulti || !f_plty || !f_cmbn || !loss || !d_ulti || !d_plty || !d_cmbn || !df_ulti ||
        !df_plty || !df_cmbn || B <= 0 || K <= 0 || P <= 0 || C_ulti <= 0 || C_plty <= 0 || C_cmbn <= 0)
        return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < cx_loss_ws_need(B, K, P, C_ulti, C_plty, C_cmbn)) return HK_ERR_WORKSPACE;     // a short workspace first, like every entry point
    if (B < 2 || P > CX_MAX_P || !cx_loss_sizes_ok(B, K, P, C_ulti, C_plty, C_cmbn)) return HK_ERR_UNSUPPORTED;
    CxLossArgs A;
    A.logits[0] = ulti; A.logits[1] = plty; A.logits[2] = cmbn;
    A.labels = labels;
    A.feat[0] = f_ulti; A.feat[1] = f_plty; A.feat[2] = f_cmbn;
    A.gamma[0] = gamma_ulti; A.gamma[1] = gamma_plty; A.gamma[2] = gamma_cmbn;
    A.weight = weight;
    A.loss = loss;
    A.dlogits[0] = d_ulti; A.dlogits[1] = d_plty; A.dlogits[2] = d_cmbn;
    A.dfeat[0] = df_ulti; A.dfeat[1] = df_plty; A.dfeat[2] = df_cmbn;
    A.B = B; A.K = K; A.P = P;
    A.C[0] = C_ulti; A.C[1] = C_plty; A.C[2] = C_cmbn;
    A.sumrow = (float*)ws;
    A.ce_rows = A.sumrow + (size_t)B * K;
    A.kl_rows = A.ce_rows + B;
    A.inv = A.kl_rows + B;
    A.g = A.inv + (size_t)3 * P * B;
    hipLaunchKernelGGL(crossx_loss_kernel, dim3(1), dim3(CX_LOSS_THREADS), 0, (hipStream_t)stream, A);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
