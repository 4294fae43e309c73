// One wave, one row of logits: the statistics of a label-smoothed cross entropy and the gradient of that row - shared by
// the losses that give one wave a row (apinet.hip, nts.hip).  Fixed element order: lane l owns l, l + 64, ..
#pragma once
#include <cmath>

#include "hk_common.h"

namespace hk {

struct ApiRow {
    float mx, ls, sum, py;       // max, log sum exp(l - mx), sum (l - mx), p[y]; ce: the smoothed cross entropy
    float ce, inv;               // inv = 1 / sum exp(l - mx): probabilities are exp(l - mx) inv (no log -> exp round trip, whose
                                 // absolute error in the logarithm would come back as a relative error of p)
};

// One wave, one row of C logits.  Element order: lane l owns l, l + 64, ..
__device__ __forceinline__ ApiRow api_row_stats(const float* row, int C, int y, float smoothing) {
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
    ApiRow r;
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
__device__ __forceinline__ void api_row_grad(const float* row, float* out, int C, int y, float smoothing, const ApiRow& r, float w_ce,
                                             float w_rank) {
    const int lane = threadIdx.x & 63;
    const float u = smoothing / (float)C, rk = w_rank != 0.f ? w_rank * r.py : 0.f;
    for (int c = lane; c < C; c += WAVE) {
        const float p = expf(row[c] - r.mx) * r.inv, hit = c == y ? 1.f : 0.f;
        out[c] = w_ce * (p - u - (1.f - smoothing) * hit) + rk * (hit - p);
    }
}

}  // namespace hk
