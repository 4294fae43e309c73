// DCL head (Destruction and Construction Learning): the two readers of the last ResNet-50 map, the loss, and the swap law
// of the data pipeline.  replaces model/methods/DCL.py:33-39 (a 1 x 1 convolution to one channel, AvgPool2d(2), tanh and a
// view on one read of the [2B,2048,14,14] map, AdaptiveAvgPool2d(1) on another; backward: two full-size map gradients and an
// add), model/loss/DCL_loss.py:17-20 (two label-smoothed cross entropies and an L1 term: three reductions, their backward
// graphs and an add) and dataset/dataset_DCL.py:48-62 (per image 98 ImageStat means and a 49 x 49 nearest-mean search in
// Python, inside __getitem__).
//
//   head   a workgroup of four waves per (sample, 64 channels); a wave owns 16 (sample, channel) rows of HW elements.  Lane l
//          owns the elements 4 l .. 4 l + 3, then + 256, ..: one 16-byte access per row where HW % 4 == 0 and every map
//          pointer is 16-byte aligned, scalar accesses with the same element-to-lane map otherwise - both paths add in the
//          same order and give the same bits.  Forward: every row is read once; its mean leaves with a wave butterfly; its
//          share w[c] x of the 1 x 1 convolution is added over the wave's rows in a register, over the four waves through LDS
//          (wave 0 .. 3) and written as the workgroup's partial map; a second launch adds the partial maps chunk by chunk,
//          the bias, pools 2 x 2 (row by row, left to right) and takes the tanh.  Backward: g / 4 is formed per element from
//          d_mask and the saved mask, x is read once (for dw), dx written once; dw leaves as one partial per (sample,
//          channel) that a second launch adds sample by sample, together with dbias.  No atomics.
//          The products are not contracted into fmas: w[c] * x is rounded, then added, as the reference's two ops are.
//   loss   one workgroup of 16 waves, a wave per sample: both cross entropies (hk_rows.h), the row's share of the L1 term
//          and the three gradients; the waves' totals meet in LDS in wave order.  One launch, no workspace.
//   law    one workgroup per image.  A wave per patch: exact integer band totals of the unswapped and the swapped patch,
//          then in float64 ((0 + s_r / n) + s_g / n) + s_b / n - Python's sum() of ImageStat's means.  A thread per swapped
//          patch: the unswapped patch with the nearest value, the lowest index on ties.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int DH_THREADS = 256;
constexpr int DH_WAVES = DH_THREADS / WAVE;
constexpr int DH_CPW = 16;                             // rows (channels of one sample) that a wave owns
constexpr int DH_CHUNK = DH_WAVES * DH_CPW;            // channels per workgroup

template <bool VEC>
__global__ __launch_bounds__(DH_THREADS) void dcl_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  float* __restrict__ pooled, float* __restrict__ part, int C, int HW,
                                                                  int nchunk) {
#pragma clang fp contract(off)
    __shared__ float red[DH_WAVES][ROW_STEP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
    const int c0 = chunk * DH_CHUNK + wave * DH_CPW;
    const int left = C - c0;
    const int nc = left < 0 ? 0 : (left < DH_CPW ? left : DH_CPW);                  // wave-uniform
    float wc[DH_CPW], ps[DH_CPW];
#pragma unroll
    for (int k = 0; k < DH_CPW; ++k) {
        wc[k] = k < nc ? w[c0 + k] : 0.f;
        ps[k] = 0.f;
    }
    const float* xb = x + ((size_t)b * C + (nc ? c0 : 0)) * HW;
    float* pb = part + (size_t)blockIdx.x * HW;
    for (int t0 = 0; t0 < HW; t0 += ROW_STEP) {                                      // every thread makes every trip: barriers below
        const int i = t0 + lane * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (i < HW) {
#pragma unroll
            for (int k = 0; k < DH_CPW; ++k) {
                if (k < nc) {
                    const f32x4 v = load4<VEC>(xb + (size_t)k * HW, i, HW);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[e] += wc[k] * v[e];
                        ps[k] += v[e];                                              // past the end: + 0, which changes nothing
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][lane * 4 + e] = acc[e];
        __syncthreads();
        const int at = t0 + threadIdx.x;
        if (at < HW) pb[at] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < DH_CPW; ++k) {
        if (k < nc) {
            const float s = wave_sum(ps[k]);
            if (lane == 0) pooled[(size_t)b * C + c0 + k] = s / (float)HW;
        }
    }
}

// a thread per mask element: the four pixels of its window, each the sum of the partial maps in chunk order plus the bias
__global__ __launch_bounds__(DH_THREADS) void dcl_head_mask_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                   float* __restrict__ mask, long long total, int nchunk, int HW, int W,
                                                                   int Mh, int Mw) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * DH_THREADS + threadIdx.x;
    if (q >= total) return;
    const int M = Mh * Mw;
    const int m = (int)(q % M);
    const long long b = q / M;
    const int mi = m / Mw, mj = m - mi * Mw;
    const float bs = bias[0];
    float px[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pos = (2 * mi + (r >> 1)) * W + 2 * mj + (r & 1);
        const float* p = part + (size_t)b * nchunk * HW + pos;
        float s = 0.f;
        for (int ch = 0; ch < nchunk; ++ch) s += p[(size_t)ch * HW];
        px[r] = s + bs;
    }
    mask[q] = tanhf((((px[0] + px[1]) + px[2]) + px[3]) * 0.25f);
}

template <bool VEC>
__global__ __launch_bounds__(DH_THREADS) void dcl_head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ mask, const float* __restrict__ d_pooled,
                                                                  const float* __restrict__ d_mask, float* __restrict__ dx,
                                                                  float* __restrict__ dwpart, int C, int HW, int W, int Mh, int Mw,
                                                                  int nchunk) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
    const int c0 = chunk * DH_CHUNK + wave * DH_CPW;
    const int left = C - c0;
    const int nc = left < 0 ? 0 : (left < DH_CPW ? left : DH_CPW);
    if (nc == 0) return;                                                            // wave-uniform; no barrier below
    float wc[DH_CPW], dp[DH_CPW], da[DH_CPW];
#pragma unroll
    for (int k = 0; k < DH_CPW; ++k) {
        wc[k] = k < nc ? w[c0 + k] : 0.f;
        dp[k] = (k < nc && d_pooled) ? d_pooled[(size_t)b * C + c0 + k] / (float)HW : 0.f;
        da[k] = 0.f;
    }
    const size_t base = ((size_t)b * C + c0) * HW;
    const float* mk = mask + (size_t)b * Mh * Mw;
    const float* dm = d_mask ? d_mask + (size_t)b * Mh * Mw : nullptr;
    for (int i = lane * 4; i < HW; i += ROW_STEP) {
        f32x4 gq = {0.f, 0.f, 0.f, 0.f};                                            // g / 4 at the element's window; 0 outside the pooled area
        if (dm) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pos = i + e;
                if (pos < HW) {
                    const int h = pos / W, mi = h >> 1, mj = (pos - h * W) >> 1;
                    if (mi < Mh && mj < Mw) {
                        const float t = mk[mi * Mw + mj];
                        gq[e] = (dm[mi * Mw + mj] * (1.f - t * t)) * 0.25f;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < DH_CPW; ++k) {
            if (k < nc) {
                if (dwpart) {
                    const f32x4 v = load4<VEC>(x + base + (size_t)k * HW, i, HW);
#pragma unroll
                    for (int e = 0; e < 4; ++e) da[k] += v[e] * gq[e];
                }
                if (dx) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = dp[k] + wc[k] * gq[e];
                    store4<VEC>(dx + base + (size_t)k * HW, i, HW, o);
                }
            }
        }
    }
    if (dwpart) {
#pragma unroll
        for (int k = 0; k < DH_CPW; ++k) {
            if (k < nc) {
                const float s = wave_sum(da[k]);
                if (lane == 0) dwpart[(size_t)b * C + c0 + k] = s;
            }
        }
    }
}

// dw[c] = the partials of sample 0, 1, ..; block 0 also adds g = d_mask (1 - mask^2) over every sample for dbias.  d_mask
// NULL: zeros.
__global__ __launch_bounds__(DH_THREADS) void dcl_head_bwd_finish_kernel(const float* __restrict__ dwpart, const float* __restrict__ mask,
                                                                         const float* __restrict__ d_mask, float* __restrict__ dw,
                                                                         float* __restrict__ dbias, int B, int C, long long BM) {
#pragma clang fp contract(off)
    __shared__ float red[DH_WAVES];
    const int c = blockIdx.x * DH_THREADS + threadIdx.x;
    if (dw && c < C) {
        float s = 0.f;
        if (d_mask)
            for (int b = 0; b < B; ++b) s += dwpart[(size_t)b * C + c];
        dw[c] = s;
    }
    if (dbias && blockIdx.x == 0) {                                                 // block-uniform: every thread reaches the barriers
        float s = 0.f;
        if (d_mask)
            for (long long q = threadIdx.x; q < BM; q += DH_THREADS) {
                const float t = mask[q];
                s += d_mask[q] * (1.f - t * t);
            }
        s = block_sum<DH_WAVES>(s, red);
        if (threadIdx.x == 0) dbias[0] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------- loss
constexpr int DL_THREADS = 1024;
constexpr int DL_WAVES = DL_THREADS / WAVE;
constexpr int DL_MAX_N = 1 << 16;
constexpr long long DL_MAX_WIDTH = 1 << 24;

struct DclLossArgs {
    const float* logits;           // [N,K]
    const float* swap;             // [N,S]
    const float* mask;             // [N,M]
    const int64_t* labels;         // [N]
    const int64_t* labels_swap;    // [N]
    const float* law;              // [N,M]
    float alpha, beta, gamma, smoothing, weight;
    float* loss;                   // [4]
    float* d_logits;
    float* d_swap;
    float* d_mask;
    int N, K, S, M;
};

__global__ __launch_bounds__(DL_THREADS) void dcl_loss_kernel(const DclLossArgs A) {
#pragma clang fp contract(off)
    __shared__ float red[3][DL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = A.N, K = A.K, S = A.S, M = A.M;
    const float count = (float)N * (float)M;
    const float w_ce = A.alpha * A.weight / (float)N, w_sw = A.beta * A.weight / (float)N, w_law = A.gamma * A.weight / count;
    float ce = 0.f, sw = 0.f, lw = 0.f;
    for (int b = wave; b < N; b += DL_WAVES) {                                      // a wave per sample, in ascending order
        const long long yl = A.labels[b], zl = A.labels_swap[b];
        const int y = (yl >= 0 && yl < K) ? (int)yl : -1, z = (zl >= 0 && zl < S) ? (int)zl : -1;
        const float* row = A.logits + (size_t)b * K;
        const CeRow r = ce_row_stats(row, K, y, A.smoothing);
        ce_row_grad(row, A.d_logits + (size_t)b * K, K, y, A.smoothing, r, w_ce, 0.f);
        ce += r.ce;
        const float* srow = A.swap + (size_t)b * S;
        const CeRow q = ce_row_stats(srow, S, z, A.smoothing);
        ce_row_grad(srow, A.d_swap + (size_t)b * S, S, z, A.smoothing, q, w_sw, 0.f);
        sw += q.ce;
        float s = 0.f;
        for (int m = lane; m < M; m += WAVE) {
            const float d = A.mask[(size_t)b * M + m] - A.law[(size_t)b * M + m];
            s += fabsf(d);
            A.d_mask[(size_t)b * M + m] = d > 0.f ? w_law : (d < 0.f ? -w_law : (d == d ? 0.f : d));      // sign(0) = 0, as torch's
        }
        lw += wave_sum(s);
    }
    if (lane == 0) {
        red[0][wave] = ce;
        red[1][wave] = sw;
        red[2][wave] = lw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[3];
        for (int k = 0; k < 3; ++k) {
            float s = 0.f;
            for (int i = 0; i < DL_WAVES; ++i) s += red[k][i];
            t[k] = s;
        }
        const float cem = t[0] / (float)N, swm = t[1] / (float)N, lawm = t[2] / count;
        A.loss[0] = (A.alpha * cem + A.beta * swm) + A.gamma * lawm;                // the reference's order of addition
        A.loss[1] = cem;
        A.loss[2] = swm;
        A.loss[3] = lawm;
    }
}

// --------------------------------------------------------------------------------------------------------- swap law
constexpr int SL_THREADS = 1024;
constexpr int SL_WAVES = SL_THREADS / WAVE;
constexpr int SL_MAX_P = 2048;                         // patches per image: two float64 values each in LDS
constexpr long long SL_MAX_PIXELS = 1 << 24;           // 255 H W stays below 2^32: a band total fits 32 bits

__device__ __forceinline__ int sl_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(SL_THREADS) void dcl_swap_law_kernel(const uint8_t* __restrict__ un, const uint8_t* __restrict__ sw,
                                                                  const int32_t* __restrict__ bx, const int32_t* __restrict__ by,
                                                                  int32_t* __restrict__ index, float* __restrict__ law, int H, int W, int gx,
                                                                  int gy) {
#pragma clang fp contract(off)
    __shared__ double stat[2 * SL_MAX_P];              // [0, P): the unswapped patches, [P, 2 P): the swapped ones
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = gx * gy;
    const size_t image = (size_t)blockIdx.x * H * W * 3;
    for (int job = wave; job < 2 * P; job += SL_WAVES) {
        const int which = job / P, p = job - which * P;
        const int pj = p / gx, pi = p - pj * gx;
        // a table entry outside the image reads nothing: clamped here, because the table lives on the device
        const int x0 = sl_clamp(bx[pi], W), x1 = sl_clamp(bx[pi + 1], W), y0 = sl_clamp(by[pj], H), y1 = sl_clamp(by[pj + 1], H);
        const int pw = x1 > x0 ? x1 - x0 : 0, ph = y1 > y0 ? y1 - y0 : 0;
        const int cnt = pw * ph;
        const uint8_t* img = (which ? sw : un) + image;
        unsigned s0 = 0, s1 = 0, s2 = 0;
        for (int i = lane; i < cnt; i += WAVE) {
            const int r = i / pw, c = i - r * pw;
            const uint8_t* px = img + ((size_t)(y0 + r) * W + x0 + c) * 3;
            s0 += px[0];
            s1 += px[1];
            s2 += px[2];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o, 64);
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
        }
        if (lane == 0) {
            const double n = (double)cnt;              // an empty patch: 0 / 0, a NaN that no comparison picks
            stat[job] = ((0.0 + (double)s0 / n) + (double)s1 / n) + (double)s2 / n;
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += SL_THREADS) {
        const double v = stat[P + p];
        int best = 0;
        double bd = fabs(v - stat[0]);
        for (int q = 1; q < P; ++q) {
            const double d = fabs(v - stat[q]);
            if (d < bd) {                              // strictly nearer: the lowest index keeps a tie
                bd = d;
                best = q;
            }
        }
        index[(size_t)blockIdx.x * P + p] = best;
        law[(size_t)blockIdx.x * P + p] = (float)((double)(best - P / 2) / (double)P);
    }
}

static int head_sizes(int B, int C, int H, int W, int& nchunk) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return HK_ERR_BAD_ARG;
    nchunk = (C + DH_CHUNK - 1) / DH_CHUNK;
    if (H < 2 || W < 2) return HK_ERR_UNSUPPORTED;     // AvgPool2d(2) has no output there
    if ((long long)H * W > 0x7fffffffLL - ROW_STEP || (long long)B * nchunk > 0x7fffffffLL || (long long)B * C > 0x7fffffffLL ||
        (long long)B * (H / 2) * (W / 2) > 0x7fffffffLL)
        return HK_ERR_UNSUPPORTED;
    return HK_OK;
}

static size_t head_fwd_need(int B, int C, int H, int W) {
    return (size_t)B * ((C + DH_CHUNK - 1) / DH_CHUNK) * H * W * sizeof(float) + 256;
}

static size_t head_bwd_need(int B, int C) { return (size_t)B * C * sizeof(float) + 256; }

}  // namespace hk

using namespace hk;

extern "C" size_t hk_dcl_head_fwd_ws_bytes(int B, int C, int H, int W) {
    int nchunk;
    return head_sizes(B, C, H, W, nchunk) == HK_OK ? head_fwd_need(B, C, H, W) : 0;
}

extern "C" int hk_dcl_head_fwd(const float* x, const float* w, const float* bias, float* pooled, float* mask, int B, int C, int H, int W,
                               void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!x || !w || !bias || !pooled || !mask || B <= 0 || C <= 0 || H <= 0 || W <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < head_fwd_need(B, C, H, W)) return HK_ERR_WORKSPACE;       // a short workspace first, like every entry point
    int nchunk;
    const int rc = head_sizes(B, C, H, W, nchunk);
    if (rc != HK_OK) return rc;
    const int HW = H * W, Mh = H / 2, Mw = W / 2;
    float* part = (float*)ws;
    const dim3 grid((unsigned)(B * nchunk)), block(DH_THREADS);
    if ((HW & 3) == 0 && aligned16(x))
        hipLaunchKernelGGL((dcl_head_fwd_kernel<true>), grid, block, 0, (hipStream_t)stream, x, w, pooled, part, C, HW, nchunk);
    else
        hipLaunchKernelGGL((dcl_head_fwd_kernel<false>), grid, block, 0, (hipStream_t)stream, x, w, pooled, part, C, HW, nchunk);
    HK_LAUNCH_CHECK();
    const long long total = (long long)B * Mh * Mw;
    hipLaunchKernelGGL(dcl_head_mask_kernel, dim3((unsigned)((total + DH_THREADS - 1) / DH_THREADS)), block, 0, (hipStream_t)stream, part,
                       bias, mask, total, nchunk, HW, W, Mh, Mw);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" size_t hk_dcl_head_bwd_ws_bytes(int B, int C, int H, int W) {
    int nchunk;
    return head_sizes(B, C, H, W, nchunk) == HK_OK ? head_bwd_need(B, C) : 0;
}

extern "C" int hk_dcl_head_bwd(const float* x, const float* w, const float* mask, const float* d_pooled, const float* d_mask, float* dx,
                               float* dw, float* dbias, int B, int C, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!x || !w || !mask || B <= 0 || C <= 0 || H <= 0 || W <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < head_bwd_need(B, C)) return HK_ERR_WORKSPACE;
    int nchunk;
    const int rc = head_sizes(B, C, H, W, nchunk);
    if (rc != HK_OK) return rc;
    const int HW = H * W, Mh = H / 2, Mw = W / 2;
    float* dwpart = (dw && d_mask) ? (float*)ws : nullptr;
    const dim3 block(DH_THREADS);
    if (dx || dwpart) {
        const dim3 grid((unsigned)(B * nchunk));
        if ((HW & 3) == 0 && aligned16(x) && (!dx || aligned16(dx)))
            hipLaunchKernelGGL((dcl_head_bwd_kernel<true>), grid, block, 0, (hipStream_t)stream, x, w, mask, d_pooled, d_mask, dx, dwpart, C,
                               HW, W, Mh, Mw, nchunk);
        else
            hipLaunchKernelGGL((dcl_head_bwd_kernel<false>), grid, block, 0, (hipStream_t)stream, x, w, mask, d_pooled, d_mask, dx, dwpart, C,
                               HW, W, Mh, Mw, nchunk);
        HK_LAUNCH_CHECK();
    }
    if (dw || dbias) {
        const unsigned blocks = dw ? (unsigned)((C + DH_THREADS - 1) / DH_THREADS) : 1u;
        hipLaunchKernelGGL(dcl_head_bwd_finish_kernel, dim3(blocks), block, 0, (hipStream_t)stream, dwpart, mask, d_mask, dw, dbias, B, C,
                           (long long)B * Mh * Mw);
        HK_LAUNCH_CHECK();
    }
    return HK_OK;
}

extern "C" int hk_dcl_loss(const float* logits, const float* swap_logits, const float* mask, const int64_t* labels,
                           const int64_t* labels_swap, const float* law, float alpha, float beta, float gamma, float smoothing, float weight,
                           float* loss, float* d_logits, float* d_swap, float* d_mask, int N, int K, int S, int M, hk_stream_t stream) {
    if (!logits || !swap_logits || !mask || !labels || !labels_swap || !law || !loss || !d_logits || !d_swap || !d_mask || N <= 0 || K <= 0 ||
        S <= 0 || M <= 0)
        return HK_ERR_BAD_ARG;
    if (N > DL_MAX_N || K > DL_MAX_WIDTH || S > DL_MAX_WIDTH || M > DL_MAX_WIDTH || (long long)N * K > 0x7fffffffLL ||
        (long long)N * S > 0x7fffffffLL || (long long)N * M > 0x7fffffffLL)
        return HK_ERR_UNSUPPORTED;
    DclLossArgs A;
    A.logits = logits; A.swap = swap_logits; A.mask = mask;
    A.labels = labels; A.labels_swap = labels_swap; A.law = law;
    A.alpha = alpha; A.beta = beta; A.gamma = gamma; A.smoothing = smoothing; A.weight = weight;
    A.loss = loss; A.d_logits = d_logits; A.d_swap = d_swap; A.d_mask = d_mask;
    A.N = N; A.K = K; A.S = S; A.M = M;
    hipLaunchKernelGGL(dcl_loss_kernel, dim3(1), dim3(DL_THREADS), 0, (hipStream_t)stream, A);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_dcl_swap_law(const uint8_t* unswapped, const uint8_t* swapped, const int32_t* bounds_x, const int32_t* bounds_y,
                               int32_t* index, float* law, int N, int H, int W, int gx, int gy, hk_stream_t stream) {
    if (!unswapped || !swapped || !bounds_x || !bounds_y || !index || !law || N <= 0 || H <= 0 || W <= 0 || gx <= 0 || gy <= 0)
        return HK_ERR_BAD_ARG;
    if (W < gx || H < gy) return HK_ERR_UNSUPPORTED;                                // a patch would be empty: the reference divides by zero
    if ((long long)gx * gy > SL_MAX_P || (long long)H * W > SL_MAX_PIXELS || (long long)N * gx * gy > 0x7fffffffLL) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dcl_swap_law_kernel, dim3((unsigned)N), dim3(SL_THREADS), 0, (hipStream_t)stream, unswapped, swapped, bounds_x, bounds_y,
                       index, law, H, W, gx, gy);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
