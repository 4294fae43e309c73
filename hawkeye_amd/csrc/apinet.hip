// APINet head (attentive pairwise interaction): pair selection, pair gather, the gated interaction with its backward and
// the loss, with nothing leaving the device.  replaces model/methods/APINet.py:34-68,76-113 (a device-to-host copy of the
// distance matrix, a numpy argmin, a Python loop over the batch, four uploads, ~40 small launches) and
// model/loss/APINet_loss.py:29-39 (two softmaxes, two fancy-index gathers, a margin ranking loss and a smoothed CE).
//
//   pairs      partner[i]     = argmin_{j != i, y_j == y_i} sum_d (pool_i - pool_j)^2   (intra)      one workgroup per anchor
//              partner[B + i] = argmin_{y_j != y_i} ...                                 (inter)      lowest index among equal
//              distances; a row without a candidate gets 0 (numpy's argmin of an all-inf row).  The distance is the sum
//              of squared differences in a fixed order, NOT the reference's -2ab + |a|^2 + |b|^2, which cancels; a NaN
//              distance never compares below the running best, so it counts as +inf.
//   gather     mutual[r] = [pool[r mod B] | pool[partner[r]]]                           r < 2 B
//   interact   f1 = pool[r mod B], f2 = pool[partner[r]], g1 = sigmoid(m f1), g2 = sigmoid(m f2)
//              feats = [f1 (1 + g1) ; f2 (1 + g2) ; f1 (1 + g2) ; f2 (1 + g1)] (.) keep * scale       [8 B, D]
//   backward   every gradient that reaches pool is a scatter with a variable number of sources: row i is f1 of the rows i
//              and B + i and f2 of every row r with partner[r] == i.  api_collect() adds them for ONE target element in the
//              order i, B + i, then r = 0 .. 2B-1 - no atomics, the same bits on every run - and serves the gather's and
//              the interaction's backward (which recomputes the gates of the rows it collects from: one launch, no
//              workspace).
//   loss       one wave per row r of BOTH logit matrices: max, log-sum-exp, row sum, probability at the target; the
//              gradients need nothing from other rows and are written by the same wave.  A second one-wave launch adds the
//              per-row terms in a fixed order.
// A partner outside [0, B) (a caller's own index tensor) is never dereferenced: its f2 reads as zeros and it scatters nothing.
// These kernels are launch- and latency-bound (320 KB of pooled vectors at the yaml's batch), not roofline-bound.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int API_THREADS = 256;
constexpr int API_WAVES = API_THREADS / WAVE;

// One wave: sum_d (a[d] - b[d])^2.  The order depends on D alone (QUAD: D % 4 == 0, lane l owns the quads l, l + 64, ..;
// otherwise the elements l, l + 64, ..); alignment only decides how a quad is fetched.
template <bool QUAD, bool ALIGNED>
__device__ __forceinline__ float api_sqdist(const float* a, const float* b, int D) {
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    if (QUAD) {
        for (int q = lane; q < (D >> 2); q += WAVE) {
            const f32x4 va = load4a<ALIGNED>(a + 4 * q), vb = load4a<ALIGNED>(b + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = va[e] - vb[e];
                s += d * d;
            }
        }
    } else {
        for (int c = lane; c < D; c += WAVE) {
            const float d = a[c] - b[c];
            s += d * d;
        }
    }
    return wave_sum(s);
}

template <bool QUAD, bool ALIGNED>
__global__ __launch_bounds__(API_THREADS) void api_pairs_kernel(const float* __restrict__ pool, const int32_t* __restrict__ labels,
                                                                int32_t* __restrict__ partner, int B, int D) {
    __shared__ float sd[2][API_WAVES];
    __shared__ int si[2][API_WAVES];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int yi = labels[i];
    const float* a = pool + (size_t)i * D;
    float best[2] = {INFINITY, INFINITY};              // 0: same label, 1: another label
    int idx[2] = {0, 0};
    for (int j = wave; j < B; j += API_WAVES) {        // wave-uniform; increasing j and a strict <: the lowest index of a tie
        if (j == i) continue;
        const float d = api_sqdist<QUAD, ALIGNED>(a, pool + (size_t)j * D, D);
        const int k = labels[j] == yi ? 0 : 1;
        if (d < best[k]) { best[k] = d; idx[k] = j; }
    }
    if (lane == 0) {
        sd[0][wave] = best[0]; si[0][wave] = idx[0];
        sd[1][wave] = best[1]; si[1][wave] = idx[1];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        float b = sd[k][0];
        int bi = si[k][0];
        for (int w = 1; w < API_WAVES; ++w)
            if (sd[k][w] < b || (sd[k][w] == b && si[k][w] < bi)) { b = sd[k][w]; bi = si[k][w]; }
        partner[k * B + i] = bi;
    }
}

__device__ __forceinline__ bool api_valid(int p, int B) { return (unsigned)p < (unsigned)B; }

__global__ __launch_bounds__(API_THREADS) void api_gather_fwd_kernel(const float* __restrict__ pool, const int32_t* __restrict__ partner,
                                                                     float* __restrict__ mutual, int B, int D) {
    const int r = blockIdx.y, d = blockIdx.x * API_THREADS + threadIdx.x;
    if (d >= D) return;
    const int p = partner[r];
    float* out = mutual + (size_t)r * 2 * D;
    out[d] = pool[(size_t)(r % B) * D + d];
    out[D + d] = api_valid(p, B) ? pool[(size_t)p * D + d] : 0.f;
}

// The deterministic scatter, for ONE element d of target row i: what row i receives as f1 of the rows i and B + i, then as
// f2 of every row r with partner[r] == i, r ascending.  src.as_f1(r, d) / src.as_f2(r, d) give row r's two gradients.
template <class Src>
__device__ __forceinline__ float api_collect(Src& src, const int32_t* __restrict__ partner, int i, int d, int B) {
    float acc = src.as_f1(i, d);
    acc += src.as_f1(B + i, d);
    for (int r = 0; r < 2 * B; ++r)
        if (partner[r] == i) acc += src.as_f2(r, d);
    return acc;
}

struct GatherSrc {                                     // dmutual [2B, 2D]: the left half is f1's gradient, the right half f2's
    const float* dmutual;
    int D;
    __device__ __forceinline__ float as_f1(int r, int d) { return dmutual[(size_t)r * 2 * D + d]; }
    __device__ __forceinline__ float as_f2(int r, int d) { return dmutual[(size_t)r * 2 * D + D + d]; }
};

__global__ __launch_bounds__(API_THREADS) void api_gather_bwd_kernel(const float* __restrict__ dmutual, const int32_t* __restrict__ partner,
                                                                     float* __restrict__ dpool, int B, int D) {
    const int i = blockIdx.y, d = blockIdx.x * API_THREADS + threadIdx.x;
    if (d >= D) return;
    GatherSrc src{dmutual, D};
    dpool[(size_t)i * D + d] = api_collect(src, partner, i, d, B);
}

__device__ __forceinline__ float api_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// keep * scale of block k (0: 1-self, 1: 2-self, 2: 1-other, 3: 2-other), row r, element d
__device__ __forceinline__ float api_keep(const uint8_t* __restrict__ masks, float scale, int k, int r, int d, int B, int D) {
    if (!masks) return 1.f;
    return masks[((size_t)k * 2 * B + r) * D + d] ? scale : 0.f;
}

__global__ __launch_bounds__(API_THREADS) void api_interact_fwd_kernel(const float* __restrict__ pool, const int32_t* __restrict__ partner,
                                                                       const float* __restrict__ m, const uint8_t* __restrict__ masks,
                                                                       float scale, float* __restrict__ feats, int B, int D) {
    const int r = blockIdx.y, d = blockIdx.x * API_THREADS + threadIdx.x;
    if (d >= D) return;
    const int p = partner[r];
    const float f1 = pool[(size_t)(r % B) * D + d];
    const float f2 = api_valid(p, B) ? pool[(size_t)p * D + d] : 0.f;
    const float mv = m[(size_t)r * D + d];
    const float g1 = api_sigmoid(mv * f1), g2 = api_sigmoid(mv * f2);
    const size_t blk = (size_t)2 * B * D, at = (size_t)r * D + d;
    feats[at] = (f1 + f1 * g1) * api_keep(masks, scale, 0, r, d, B, D);
    feats[blk + at] = (f2 + f2 * g2) * api_keep(masks, scale, 1, r, d, B, D);
    feats[2 * blk + at] = (f1 + f1 * g2) * api_keep(masks, scale, 2, r, d, B, D);
    feats[3 * blk + at] = (f2 + f2 * g1) * api_keep(masks, scale, 3, r, d, B, D);
}

// Row r's gradients at element d, recomputed from the saved inputs: df1, df2 and (as_f1 only) dm.
struct InteractSrc {
    const float* pool;
    const int32_t* partner;
    const float* m;
    const uint8_t* masks;
    float scale;
    const float* dfeats;
    float* dm;
    int B, D;
    __device__ __forceinline__ void row(int r, int d, float& df1, float& df2, float& dmv) {
        const int p = partner[r];
        const bool ok = api_valid(p, B);
        const float f1 = pool[(size_t)(r % B) * D + d];
        const float f2 = ok ? pool[(size_t)p * D + d] : 0.f;
        const float mv = m[(size_t)r * D + d];
        const float g1 = api_sigmoid(mv * f1), g2 = api_sigmoid(mv * f2);
        const size_t blk = (size_t)2 * B * D, at = (size_t)r * D + d;
        const float a0 = dfeats[at] * api_keep(masks, scale, 0, r, d, B, D);
        const float a1 = dfeats[blk + at] * api_keep(masks, scale, 1, r, d, B, D);
        const float a2 = dfeats[2 * blk + at] * api_keep(masks, scale, 2, r, d, B, D);
        const float a3 = dfeats[3 * blk + at] * api_keep(masks, scale, 3, r, d, B, D);
        const float t1 = (a0 * f1 + a3 * f2) * (g1 * (1.f - g1));      // d / d(m f1)
        const float t2 = (a1 * f2 + a2 * f1) * (g2 * (1.f - g2));      // d / d(m f2)
        dmv = t1 * f1 + t2 * f2;
        df1 = a0 * (1.f + g1) + a2 * (1.f + g2) + t1 * mv;
        df2 = ok ? a1 * (1.f + g2) + a3 * (1.f + g1) + t2 * mv : 0.f;
    }
    __device__ __forceinline__ float as_f1(int r, int d) {             // called once per (r, d) over the grid: writes dm
        float df1, df2, dmv;
        row(r, d, df1, df2, dmv);
        dm[(size_t)r * D + d] = dmv;
        return df1;
    }
    __device__ __forceinline__ float as_f2(int r, int d) {
        float df1, df2, dmv;
        row(r, d, df1, df2, dmv);
        return df2;
    }
};

__global__ __launch_bounds__(API_THREADS) void api_interact_bwd_kernel(const float* __restrict__ pool, const int32_t* __restrict__ partner,
                                                                       const float* __restrict__ m, const uint8_t* __restrict__ masks,
                                                                       float scale, const float* __restrict__ dfeats,
                                                                       float* __restrict__ dm, float* __restrict__ dpool, int B, int D) {
    const int i = blockIdx.y, d = blockIdx.x * API_THREADS + threadIdx.x;
    if (d >= D) return;
    InteractSrc src{pool, partner, m, masks, scale, dfeats, dm, B, D};
    dpool[(size_t)i * D + d] = api_collect(src, partner, i, d, B);
}

// ------------------------------------------------------------------------------------------------------------- loss
__global__ __launch_bounds__(API_THREADS) void apinet_loss_rows_kernel(const float* __restrict__ ls_, const float* __restrict__ lo_,
                                                                       const int32_t* __restrict__ labels, float smoothing, float margin,
                                                                       float* __restrict__ dself, float* __restrict__ dother,
                                                                       float* __restrict__ ce_rows, float* __restrict__ rank_rows, int R,
                                                                       int C) {
    const int r = blockIdx.x * API_WAVES + (threadIdx.x >> 6);         // wave-uniform
    if (r >= R) return;
    const int y = labels[r];
    const float* rs = ls_ + (size_t)r * C;
    const float* ro = lo_ + (size_t)r * C;
    const CeRow s = ce_row_stats(rs, C, y, smoothing), o = ce_row_stats(ro, C, y, smoothing);
    const float hinge = (o.py - s.py) + margin;                        // MarginRankingLoss(self, other, +1)
    const bool active = hinge > 0.f;                                   // NaN: inactive here, the loss is NaN through ce
    const float w_ce = 0.5f / (float)R, w_rank = active ? 1.f / (float)R : 0.f;
    ce_row_grad(rs, dself + (size_t)r * C, C, y, smoothing, s, w_ce, -w_rank);
    ce_row_grad(ro, dother + (size_t)r * C, C, y, smoothing, o, w_ce, w_rank);
    if ((threadIdx.x & 63) == 0) {
        ce_rows[r] = s.ce + o.ce;
        rank_rows[r] = active ? hinge : (hinge != hinge ? hinge : 0.f);
    }
}

// loss [3] = total, CE, rank: one wave, lane partials over r = l, l + 64, .. then the butterfly - a fixed order
__global__ __launch_bounds__(WAVE) void apinet_loss_sum_kernel(const float* __restrict__ ce_rows, const float* __restrict__ rank_rows,
                                                               float* __restrict__ loss, int R) {
    const int lane = threadIdx.x;
    float a = 0.f, b = 0.f;
    for (int r = lane; r < R; r += WAVE) {
        a += ce_rows[r];
        b += rank_rows[r];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        const float ce = a / (2.f * (float)R), rank = b / (float)R;
        loss[0] = ce + rank;
        loss[1] = ce;
        loss[2] = rank;
    }
}

static bool api_grid_ok(long long rows, int D) { return rows <= 65535 && (long long)(D + API_THREADS - 1) / API_THREADS <= 0x7fffffff; }

}  // namespace hk

using namespace hk;

extern "C" int hk_api_pairs(const float* pool, const int32_t* labels, int32_t* partner, int B, int D, hk_stream_t stream) {
    if (!pool || !labels || !partner || B <= 0 || D <= 0) return HK_ERR_BAD_ARG;
    const bool quad = (D & 3) == 0, al = quad && aligned16(pool);
    const dim3 grid(B), block(API_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (!quad) hipLaunchKernelGGL((api_pairs_kernel<false, false>), grid, block, 0, st, pool, labels, partner, B, D);
    else if (al) hipLaunchKernelGGL((api_pairs_kernel<true, true>), grid, block, 0, st, pool, labels, partner, B, D);
    else hipLaunchKernelGGL((api_pairs_kernel<true, false>), grid, block, 0, st, pool, labels, partner, B, D);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_api_gather_fwd(const float* pool, const int32_t* partner, float* mutual, int B, int D, hk_stream_t stream) {
    if (!pool || !partner || !mutual || B <= 0 || D <= 0) return HK_ERR_BAD_ARG;
    if (!api_grid_ok(2LL * B, D)) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(api_gather_fwd_kernel, dim3((D + API_THREADS - 1) / API_THREADS, 2 * B), dim3(API_THREADS), 0, (hipStream_t)stream,
                       pool, partner, mutual, B, D);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_api_gather_bwd(const float* dmutual, const int32_t* partner, float* dpool, int B, int D, hk_stream_t stream) {
    if (!dmutual || !partner || !dpool || B <= 0 || D <= 0) return HK_ERR_BAD_ARG;
    if (!api_grid_ok(2LL * B, D)) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(api_gather_bwd_kernel, dim3((D + API_THREADS - 1) / API_THREADS, B), dim3(API_THREADS), 0, (hipStream_t)stream,
                       dmutual, partner, dpool, B, D);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_api_interact_fwd(const float* pool, const int32_t* partner, const float* m, const uint8_t* masks, float scale,
                                   float* feats, int B, int D, hk_stream_t stream) {
    if (!pool || !partner || !m || !feats || B <= 0 || D <= 0 || !(scale > 0.f) || std::isinf(scale)) return HK_ERR_BAD_ARG;
    if (!api_grid_ok(2LL * B, D)) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(api_interact_fwd_kernel, dim3((D + API_THREADS - 1) / API_THREADS, 2 * B), dim3(API_THREADS), 0,
                       (hipStream_t)stream, pool, partner, m, masks, scale, feats, B, D);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_api_interact_bwd(const float* pool, const int32_t* partner, const float* m, const uint8_t* masks, float scale,
                                   const float* dfeats, float* dm, float* dpool, int B, int D, hk_stream_t stream) {
    if (!pool || !partner || !m || !dfeats || !dm || !dpool || B <= 0 || D <= 0 || !(scale > 0.f) || std::isinf(scale))
        return HK_ERR_BAD_ARG;
    if (!api_grid_ok(2LL * B, D)) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(api_interact_bwd_kernel, dim3((D + API_THREADS - 1) / API_THREADS, B), dim3(API_THREADS), 0, (hipStream_t)stream,
                       pool, partner, m, masks, scale, dfeats, dm, dpool, B, D);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" size_t hk_apinet_loss_ws_bytes(int R, int C) {
    if (R <= 0 || C <= 0) return 0;
    return (size_t)2 * R * sizeof(float) + 256;
}

extern "C" int hk_apinet_loss(const float* self_logits, const float* other_logits, const int32_t* labels, float smoothing, float margin,
                              float* loss, float* dself, float* dother, int R, int C, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!self_logits || !other_logits || !labels || !loss || !dself || !dother || R <= 0 || C <= 0) return HK_ERR_BAD_ARG;
    if (!(smoothing >= 0.f && smoothing <= 1.f) || !(margin == margin) || std::isinf(margin)) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_apinet_loss_ws_bytes(R, C)) return HK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* ce_rows = (float*)ws;
    float* rank_rows = ce_rows + R;
    hipLaunchKernelGGL(apinet_loss_rows_kernel, dim3((R + API_WAVES - 1) / API_WAVES), dim3(API_THREADS), 0, st, self_logits, other_logits,
                       labels, smoothing, margin, dself, dother, ce_rows, rank_rows, R, C);
    HK_LAUNCH_CHECK();
    hipLaunchKernelGGL(apinet_loss_sum_kernel, dim3(1), dim3(WAVE), 0, st, (const float*)ce_rows, (const float*)rank_rows, loss, R);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
