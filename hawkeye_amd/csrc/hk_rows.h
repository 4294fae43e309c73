// What the plugin heads' kernels share when a wave walks a row of floats: the four-element accesses, a wave's total of an
// array, and the statistics and gradient of a label-smoothed cross entropy.  Users: peer.hip (load4a / store4a),
// apinet.hip (load4a, ce_row_*), nts.hip (wave_total, ce_row_*), crossx.hip (load4 / store4, wave_total, ce_row_stats) and
// dcl.hip (load4 / store4, ce_row_*).
#pragma once
#include <cmath>

#include "hk_common.h"

namespace hk {

constexpr int ROW_STEP = WAVE * 4;                     // elements of a row that one wave covers per trip of four per lane

// elements i .. i + 3 of a row of n floats; past the end: 0.  VEC: one 16-byte access (n % 4 == 0, an aligned row)
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* row, int i, int n) {
    if (VEC) return *reinterpret_cast<const f32x4*>(row + i);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? row[i + e] : 0.f;
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* row, int i, int n, f32x4 v) {
    if (VEC) {
        *reinterpret_cast<f32x4*>(row + i) = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i + e < n) row[i + e] = v[e];
}

// the four floats at p, all inside the row; ALIGNED: one 16-byte access
template <bool ALIGNED>
__device__ __forceinline__ f32x4 load4a(const float* p) {
    if (ALIGNED) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    return v;
}
template <bool ALIGNED>
__device__ __forceinline__ void store4a(float* p, f32x4 v) {
    if (ALIGNED) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// sum of v[0 .. n) by one wave: lane l adds l, l + 64, .. then the butterfly - a fixed order
__device__ __forceinline__ float wave_total(const float* v, int n) {
    float s = 0.f;
    for (int r = threadIdx.x & 63; r < n; r += WAVE) s += v[r];
    return wave_sum(s);
}

struct CeRow {
    float mx, ls, sum, py;       // max, log sum exp(l - mx), sum (l - mx), p[y]; ce: the smoothed cross entropy
    float ce, inv;               // inv = 1 / sum exp(l - mx): probabilities are exp(l - mx) inv (no log -> exp round trip, whose
                                 // absolute error in the logarithm would come back as a relative error of p)
};

// One wave, one row of C logits.  Element order: lane l owns l, l + 64, ..
__device__ __forceinline__ CeRow ce_row_stats(const float* row, int C, int y, float smoothing) {
    const int lane = threadIdx.x & 63;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += WAVE) mx = fmaxf(mx, row[c]);
    mx = wave_max(mx);
    float s = 0.f, t = 0.f;
    for (int c = lane; c < C; c += WAVE) {
        const float v = row[c] - mx;
        s += expf(v);
        t += v;
    }
    CeRow r;
    r.mx = mx;
    s = wave_sum(s);
    r.ls = logf(s);
    r.inv = 1.f / s;
    r.sum = wave_sum(t);
    if (y >= 0 && y < C) {                                             // a label out of range reads nothing
        const float vy = row[y] - mx;
        r.py = expf(vy) * r.inv;
        r.ce = (1.f - smoothing) * (r.ls - vy) + smoothing * (r.ls - r.sum / (float)C);
    } else {
        r.py = NAN;
        r.ce = NAN;
    }
    return r;
}

// dl[c] = w_ce (p[c] - smoothing / C - (1 - smoothing) [c == y]) + w_rank p[y] ([c == y] - p[c])
__device__ __forceinline__ void ce_row_grad(const float* row, float* out, int C, int y, float smoothing, const CeRow& r, float w_ce,
                                            float w_rank) {
    const int lane = threadIdx.x & 63;
    const float u = smoothing / (float)C, rk = w_rank != 0.f ? w_rank * r.py : 0.f;
    for (int c = lane; c < C; c += WAVE) {
        const float p = expf(row[c] - r.mx) * r.inv, hit = c == y ? 1.f : 0.f;
        out[c] = w_ce * (p - u - (1.f - smoothing) * hit) + rk * (hit - p);
    }
}

}  // namespace hk
