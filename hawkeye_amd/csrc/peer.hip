// Peer-learning loss (WebFG baseline): both losses and both logit gradients in one call, nothing leaves the device.
// replaces PeerLearningLoss, model/loss/peer_learning_loss.py:5-65 - there ~40 tiny launches (2 softmax, 2 topk, 2 nonzero,
// 6 boolean-index gathers, 2 argsort, 4 cat, 4 cross entropies) and two host synchronisations (nonzero).
//
//   per (row, net)   pred = argmax (lowest index among equal maxima), mx = max, ls = log sum exp(l - mx),
//                    ce = ls - (l[y] - mx)                                              "rows"    one wave64 each
//   selection        agree = pred_1 == pred_2, n = sum agree, m = (long long)((1 - drop_rate) n)  (double, on the device)
//                    rank_k[i] = #{agreeing j : (ce_k[j], j) < (ce_k[i], i)}            a count: no sort, deterministic
//                    keep_1 = !agree || rank_2 < m ; keep_2 = !agree || rank_1 < m      (crossed)
//                    loss_k = sum keep_k ce_k / count_k ; w_k = keep_k / count_k          "select"  one workgroup
//   gradient         dl_k[i][c] = w_k[i] (exp((l - mx) - ls) - [c == y])                  "grad"    one wave64 each
//
// Two forms behind hk_peer_loss: the general one (three launches, the per-row values in the workspace) and the resident
// one (one launch of one 1024-thread workgroup that stages both logit matrices in LDS and runs the three phases with
// barriers in between) for batches that fit a workgroup's LDS.  Both run the SAME device functions with the same lane
// order, so their results are bit-identical.  Element order inside a row depends on C alone: C % 4 == 0 -> lane l owns
// the quads l, l + 64, ...; otherwise the elements l, l + 64, ...  (alignment only decides how a quad is fetched).
// Every reduction runs in a fixed order: bit-reproducible.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int PEER_THREADS = 1024;                    // select kernel and resident form: 16 waves
constexpr int PEER_WAVES = PEER_THREADS / WAVE;
constexpr int PEER_ROW_WAVES = 4;                     // rows / grad kernels: 4 (row, net) items per 256-thread workgroup
constexpr int PEER_MAX_N = 2048;                      // select keeps 6 N + 32 words in LDS (48 KB at the bound)
constexpr size_t PEER_LDS_LIMIT = 160 * 1024;         // what one workgroup may hold on gfx950 (no static LDS in these kernels)

struct RowStat {
    int pred;
    float mx, ls, ce;
};

// One wave, one row of C logits (global memory or LDS).  QUAD: C % 4 == 0.
template <bool QUAD, bool ALIGNED>
__device__ __forceinline__ RowStat peer_row_stats(const float* row, int C, int y) {
    const int lane = threadIdx.x & 63;
    float m = -INFINITY;
    int idx = 0x7fffffff;
    if (QUAD) {
        for (int q = lane; q < (C >> 2); q += WAVE) {
            const f32x4 v = load4a<ALIGNED>(row + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v[e] > m) { m = v[e]; idx = 4 * q + e; }
        }
    } else {
        for (int c = lane; c < C; c += WAVE) {
            const float v = row[c];
            if (v > m) { m = v; idx = c; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
    }
    float s = 0.f;
    if (QUAD) {
        for (int q = lane; q < (C >> 2); q += WAVE) {
            const f32x4 v = load4a<ALIGNED>(row + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += expf(v[e] - m);
        }
    } else {
        for (int c = lane; c < C; c += WAVE) s += expf(row[c] - m);
    }
    s = wave_sum(s);
    RowStat r;
    r.pred = idx == 0x7fffffff ? 0 : idx;
    r.mx = m;
    r.ls = logf(s);
    r.ce = (y >= 0 && y < C) ? r.ls - (row[y] - m) : NAN;          // a label out of range reads nothing
    return r;
}

// One wave, one row of the gradient.  w == 0 (a dropped row): zeros, the logits are not read.
template <bool QUAD, bool ALIGNED_IN, bool ALIGNED_OUT>
__device__ __forceinline__ void peer_row_grad(const float* row, float* out, int C, int y, float w, float mx, float ls) {
    const int lane = threadIdx.x & 63;
    const bool live = w != 0.f;
    if (QUAD) {
        for (int q = lane; q < (C >> 2); q += WAVE) {
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (live) {
                const f32x4 v = load4a<ALIGNED_IN>(row + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = w * (expf((v[e] - mx) - ls) - (4 * q + e == y ? 1.f : 0.f));
            }
            store4a<ALIGNED_OUT>(out + 4 * q, g);
        }
    } else {
        for (int c = lane; c < C; c += WAVE)
            out[c] = live ? w * (expf((row[c] - mx) - ls) - (c == y ? 1.f : 0.f)) : 0.f;
    }
}

// The selection, by one workgroup of PEER_THREADS threads on LDS arrays: ce [2 N], pred [2 N] in; w [2 N] out
// (keep_k / count_k); red: 16 words of scratch.  Writes loss [2] and stats [4] = n, m, count_1, count_2.
__device__ __forceinline__ void peer_select(const float* ce, const int* pred, float* w, float* red, int N, double drop_rate,
                                            float* __restrict__ loss, int32_t* __restrict__ stats) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float c = 0.f;
    for (int i = tid; i < N; i += PEER_THREADS) c += (pred[i] == pred[N + i]) ? 1.f : 0.f;
    const int n = (int)block_sum<PEER_WAVES>(c, red);                   // counts up to 2048: exact in fp32
    const long long m = (long long)((1.0 - drop_rate) * (double)n);    // Python's int((1 - drop_rate) * n)
    for (int i = wave; i < N; i += PEER_WAVES) {
        float k1 = 1.f, k2 = 1.f;
        if (pred[i] == pred[N + i]) {
            const float a1 = ce[i], a2 = ce[N + i];
            float r1 = 0.f, r2 = 0.f;
            for (int j = lane; j < N; j += WAVE)
                if (pred[j] == pred[N + j]) {
                    const float b1 = ce[j], b2 = ce[N + j];
                    r1 += (b1 < a1 || (b1 == a1 && j < i)) ? 1.f : 0.f;
                    r2 += (b2 < a2 || (b2 == a2 && j < i)) ? 1.f : 0.f;
                }
            r1 = wave_sum(r1);
            r2 = wave_sum(r2);
            k1 = ((long long)r2 < m) ? 1.f : 0.f;                       // crossed: net 1 keeps what net 2 finds easy
            k2 = ((long long)r1 < m) ? 1.f : 0.f;
        }
        if (lane == 0) { w[i] = k1; w[N + i] = k2; }
    }
    __syncthreads();
    float c1 = 0.f, c2 = 0.f;
    for (int i = tid; i < N; i += PEER_THREADS) { c1 += w[i]; c2 += w[N + i]; }
    const float cnt1 = block_sum<PEER_WAVES>(c1, red);
    const float cnt2 = block_sum<PEER_WAVES>(c2, red);
    const float rw1 = 1.0f / cnt1, rw2 = 1.0f / cnt2;
    for (int i = tid; i < N; i += PEER_THREADS) {
        w[i] = w[i] != 0.f ? rw1 : 0.f;
        w[N + i] = w[N + i] != 0.f ? rw2 : 0.f;
    }
    __syncthreads();
    if (wave < 2) {                                                    // wave k sums net k: lane partials, then the butterfly
        const float* ck = ce + wave * N;
        const float* wk = w + wave * N;
        float s = 0.f;
        for (int i = lane; i < N; i += WAVE)
            if (wk[i] != 0.f) s += ck[i];
        s = wave_sum(s);
        if (lane == 0) loss[wave] = s / (wave == 0 ? cnt1 : cnt2);     // count 0: 0 / 0 = NaN, as the reference's empty mean
    }
    if (tid == 0) {
        stats[0] = n;
        stats[1] = (int32_t)m;
        stats[2] = (int32_t)cnt1;
        stats[3] = (int32_t)cnt2;
    }
}

// ---------------------------------------------------------------------------------------- general form: three launches
// workspace, N words each: pred [2], mx [2], ls [2], ce [2], w [2]   (index k N + i)
template <bool QUAD, bool ALIGNED>
__global__ __launch_bounds__(PEER_ROW_WAVES * WAVE) void peer_rows_kernel(const float* __restrict__ l1, const float* __restrict__ l2,
                                                                         const int32_t* __restrict__ labels, int* __restrict__ pred,
                                                                         float* __restrict__ mx, float* __restrict__ ls,
                                                                         float* __restrict__ ce, int N, int C) {
    const int item = blockIdx.x * PEER_ROW_WAVES + (threadIdx.x >> 6);         // wave-uniform
    if (item >= 2 * N) return;
    const int i = item >> 1, k = item & 1;
    const RowStat r = peer_row_stats<QUAD, ALIGNED>((k ? l2 : l1) + (size_t)i * C, C, labels[i]);
    if ((threadIdx.x & 63) == 0) {
        pred[k * N + i] = r.pred;
        mx[k * N + i] = r.mx;
        ls[k * N + i] = r.ls;
        ce[k * N + i] = r.ce;
    }
}

__global__ __launch_bounds__(PEER_THREADS) void peer_select_kernel(const int* __restrict__ pred_g, const float* __restrict__ ce_g,
                                                                  float* __restrict__ w_g, double drop_rate,
                                                                  float* __restrict__ loss, int32_t* __restrict__ stats, int N) {
    HK_DYN_LDS(sm);                                   // ce [2 N], pred [2 N], w [2 N], red [32]
    float* ce = sm;
    int* pred = reinterpret_cast<int*>(sm + 2 * N);
    float* w = sm + 4 * N;
    float* red = sm + 6 * N;
    for (int t = threadIdx.x; t < 2 * N; t += PEER_THREADS) {
        ce[t] = ce_g[t];
        pred[t] = pred_g[t];
    }
    __syncthreads();
    peer_select(ce, pred, w, red, N, drop_rate, loss, stats);
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * N; t += PEER_THREADS) w_g[t] = w[t];
}

template <bool QUAD, bool ALIGNED_IN, bool ALIGNED_OUT>
__global__ __launch_bounds__(PEER_ROW_WAVES * WAVE) void peer_grad_kernel(const float* __restrict__ l1, const float* __restrict__ l2,
                                                                         const int32_t* __restrict__ labels, const float* __restrict__ w,
                                                                         const float* __restrict__ mx, const float* __restrict__ ls,
                                                                         float* __restrict__ dl1, float* __restrict__ dl2, int N, int C) {
    const int item = blockIdx.x * PEER_ROW_WAVES + (threadIdx.x >> 6);
    if (item >= 2 * N) return;
    const int i = item >> 1, k = item & 1;
    peer_row_grad<QUAD, ALIGNED_IN, ALIGNED_OUT>((k ? l2 : l1) + (size_t)i * C, (k ? dl2 : dl1) + (size_t)i * C, C, labels[i],
                                                 w[k * N + i], mx[k * N + i], ls[k * N + i]);
}

// ------------------------------------------------------------------------------------------ resident form: one launch
// LDS: logits [2][N][C] (16-byte aligned rows when C % 4 == 0), then ce, pred, w, mx, ls [2 N] each, red [32]
template <bool QUAD, bool ALIGNED_IN, bool ALIGNED_OUT>
__global__ __launch_bounds__(PEER_THREADS) void peer_resident_kernel(const float* __restrict__ l1, const float* __restrict__ l2,
                                                                    const int32_t* __restrict__ labels, double drop_rate,
                                                                    float* __restrict__ loss, float* __restrict__ dl1,
                                                                    float* __restrict__ dl2, int32_t* __restrict__ stats, int N, int C) {
    HK_DYN_LDS16(sm);
    const int NC = N * C;
    float* lg = sm;
    float* ce = sm + 2 * (size_t)NC;
    int* pred = reinterpret_cast<int*>(ce + 2 * N);
    float* w = ce + 4 * N;
    float* mx = ce + 6 * N;
    float* ls = ce + 8 * N;
    float* red = ce + 10 * N;
    const int tid = threadIdx.x, wave = tid >> 6;
    if (QUAD && ALIGNED_IN) {                          // N C % 4 == 0 with C
        for (int q = tid; q < (NC >> 2); q += PEER_THREADS) {
            *reinterpret_cast<f32x4*>(lg + 4 * q) = *reinterpret_cast<const f32x4*>(l1 + 4 * q);
            *reinterpret_cast<f32x4*>(lg + NC + 4 * q) = *reinterpret_cast<const f32x4*>(l2 + 4 * q);
        }
    } else {
        for (int t = tid; t < NC; t += PEER_THREADS) {
            lg[t] = l1[t];
            lg[NC + t] = l2[t];
        }
    }
    __syncthreads();
    for (int item = wave; item < 2 * N; item += PEER_WAVES) {
        const int i = item >> 1, k = item & 1;
        const RowStat r = peer_row_stats<QUAD, true>(lg + (size_t)k * NC + (size_t)i * C, C, labels[i]);
        if ((tid & 63) == 0) {
            pred[k * N + i] = r.pred;
            mx[k * N + i] = r.mx;
            ls[k * N + i] = r.ls;
            ce[k * N + i] = r.ce;
        }
    }
    __syncthreads();
    peer_select(ce, pred, w, red, N, drop_rate, loss, stats);
    __syncthreads();
    for (int item = wave; item < 2 * N; item += PEER_WAVES) {
        const int i = item >> 1, k = item & 1;
        peer_row_grad<QUAD, true, ALIGNED_OUT>(lg + (size_t)k * NC + (size_t)i * C, (k ? dl2 : dl1) + (size_t)i * C, C, labels[i],
                                               w[k * N + i], mx[k * N + i], ls[k * N + i]);
    }
}

static size_t peer_resident_lds(int N, int C) { return ((size_t)2 * N * C + (size_t)10 * N + 32) * sizeof(float); }

template <bool QUAD, bool AI, bool AO>
static int peer_launch_resident(const float* l1, const float* l2, const int32_t* labels, double drop_rate, float* loss, float* dl1,
                                float* dl2, int32_t* stats, int N, int C, hipStream_t st) {
    const size_t lds = peer_resident_lds(N, C);
    HK_ALLOW_BIG_LDS((peer_resident_kernel<QUAD, AI, AO>), lds);
    hipLaunchKernelGGL((peer_resident_kernel<QUAD, AI, AO>), dim3(1), dim3(PEER_THREADS), lds, st, l1, l2, labels, drop_rate, loss,
                       dl1, dl2, stats, N, C);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

}  // namespace hk

using namespace hk;

extern "C" size_t hk_peer_loss_ws_bytes(int N, int C) {
    if (N <= 0 || C <= 0) return 0;
    return (size_t)10 * N * sizeof(float) + 256;
}

extern "C" int hk_peer_loss(const float* logits1, const float* logits2, const int32_t* labels, double drop_rate, float* loss,
                            float* dl1, float* dl2, int32_t* stats, int N, int C, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!logits1 || !logits2 || !labels || !loss || !dl1 || !dl2 || !stats || N <= 0 || C <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_peer_loss_ws_bytes(N, C)) return HK_ERR_WORKSPACE;
    if (!(drop_rate >= 0.0 && drop_rate <= 1.0)) return HK_ERR_BAD_ARG;                 // NaN fails both comparisons
    if (N > PEER_MAX_N) return HK_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool quad = (C & 3) == 0;
    const bool ai = quad && aligned16(logits1) && aligned16(logits2);
    const bool ao = quad && aligned16(dl1) && aligned16(dl2);
    const bool fits = peer_resident_lds(N, C) <= PEER_LDS_LIMIT;
    const int form = tuning().peer_form;
    if (form == 2 && !fits) return HK_ERR_UNSUPPORTED;
    // automatic: the resident form wherever it fits (one launch against three; not yet timed on the device - DESIGN.md 3.11)
    const bool resident = form == 2 || (form != 1 && fits);
    if (resident) {
#define HK_PEER_RES(Q, AI, AO) peer_launch_resident<Q, AI, AO>(logits1, logits2, labels, drop_rate, loss, dl1, dl2, stats, N, C, st)
        if (!quad) return HK_PEER_RES(false, false, false);
        if (ai) return ao ? HK_PEER_RES(true, true, true) : HK_PEER_RES(true, true, false);
        return ao ? HK_PEER_RES(true, false, true) : HK_PEER_RES(true, false, false);
#undef HK_PEER_RES
    }
    int* pred = (int*)ws;
    float* mx = (float*)ws + (size_t)2 * N;
    float* ls = mx + (size_t)2 * N;
    float* ce = ls + (size_t)2 * N;
    float* w = ce + (size_t)2 * N;
    const dim3 grid((2 * N + PEER_ROW_WAVES - 1) / PEER_ROW_WAVES), block(PEER_ROW_WAVES * WAVE);
#define HK_PEER_ROWS(Q, A) hipLaunchKernelGGL((peer_rows_kernel<Q, A>), grid, block, 0, st, logits1, logits2, labels, pred, mx, ls, ce, N, C)
    if (!quad) HK_PEER_ROWS(false, false);
    else if (ai) HK_PEER_ROWS(true, true);
    else HK_PEER_ROWS(true, false);
#undef HK_PEER_ROWS
    HK_LAUNCH_CHECK();
    hipLaunchKernelGGL(peer_select_kernel, dim3(1), dim3(PEER_THREADS), ((size_t)6 * N + 32) * sizeof(float), st, (const int*)pred,
                       (const float*)ce, w, drop_rate, loss, stats, N);
    HK_LAUNCH_CHECK();
#define HK_PEER_GRAD(Q, AI, AO)                                                                                                  \
    hipLaunchKernelGGL((peer_grad_kernel<Q, AI, AO>), grid, block, 0, st, logits1, logits2, labels, (const float*)w, (const float*)mx, \
                       (const float*)ls, dl1, dl2, N, C)
    if (!quad) HK_PEER_GRAD(false, false, false);
    else if (ai && ao) HK_PEER_GRAD(true, true, true);
    else if (ai) HK_PEER_GRAD(true, true, false);
    else if (ao) HK_PEER_GRAD(true, false, true);
    else HK_PEER_GRAD(true, false, false);
#undef HK_PEER_GRAD
    HK_LAUNCH_CHECK();
    return HK_OK;
}
