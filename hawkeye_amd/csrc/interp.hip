// Interpretable region grouping (InterpParts): the grouping unit on the layer-3 map and the criterion.  replaces
// model/methods/Interp_Parts.py:56-122 (GroupingUnit.forward: two contiguous().view round trips, bmm for C^T X, pow(2).sum(1),
// three expanded [N,K,H,W] temporaries, softmax, the permuted bmm, the residual coding and normalize - about six sweeps of the
// [N,C,H,W] map forward and as many backward through autograd) and model/loss/InterpParts_loss.py:24-138 (cross entropy, a
// Gaussian window built in Python loops, a depthwise conv2d, adaptive_max_pool2d, sort, and a Beta prior that goes through
// .cpu().numpy() and scipy on every call).
//
//   group  a workgroup of four waves owns one sample and a tile of IP_P = 32 pixels.  It stages the C x 32 tile into LDS once
//          (row stride 33 floats: a lane per pixel or a lane per channel, both conflict-free; 132 KiB at C = 1024 - more than
//          64 KiB, so the launch attribute is raised and its return code checked).  From that copy: <c_k, x_p> and |x_p|^2 over C
//          (a thread per (pixel, channel slice of 8), eight parts at a time against the centres transposed in chunks [KP / 8][C][8], the slices
//          added in slice order through LDS), the softmax over K per pixel, then the tile's share of q = a X^T [K x C] and of
//          sum_p a (a thread per channel, pixels in order).  The shares go to the workspace; a finish launch per (sample,
//          part) adds them tile by tile and applies the clamp, the residual, 1 / sigma and the normalisation.  X leaves HBM once.
//          Backward: a launch per (sample, part) turns d_outputs_t into dq, dS and the direct shares of d_centres / d_smooth
//          (K x C work); the main launch stages the tile again, recomputes the logits and the softmax from it, forms
//          da = d_assign + dq . x + dS, the softmax / clamp / (1 / beta) chain, writes dX once (built in place in the LDS tile)
//          and leaves the tile's shares of d_centres and d_smooth, which a last launch adds in tile order.  No atomics; every
//          sum has a fixed order; the 16-byte and the scalar paths differ in how the tile is copied only.
//          Every product-sum is an fp32 fma chain: l is a difference of large terms, no bf16 pass.
//   loss   launch one, a workgroup per (sample, part): zeroes the part's slice of d_assign, the "valid" correlation with the
//          window, its maximum and the lowest flat index that holds it.  Launch two, one workgroup: the mean cross entropy and
//          its gradient (hk_rows.h, a wave per sample), each maximum's rank among its part's N (the lower sample first on a
//          tie), |log(emp + 1e-5) - log(prior[rank] + 1e-5)|, and the gradient spread over the window at the argmax.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int IP_THREADS = 256;
constexpr int IP_WAVES = IP_THREADS / WAVE;
constexpr int IP_P = 32;                               // pixels of a tile
constexpr int IP_LD = IP_P + 1;                        // row stride of the tile in LDS
constexpr int IP_KC = 8;                               // parts handled at a time
constexpr int IP_MAXK = 32;
constexpr int IP_MAXC = 1024;                          // C x 33 floats and the small arrays fit 160 KiB up to here
constexpr int IP_SL = IP_THREADS / IP_P;               // channel slices of the dot products
constexpr float IP_S_MIN = 1e-5f;                      // the reference's clamp of sum_p a
constexpr float IP_N_MIN = 1e-12f;                     // F.normalize's eps

// LDS of the main kernels, in floats, behind the tile
constexpr int IP_RED = IP_SL * (IP_KC + 1) * IP_P;     // the slices' partial dot products (and |x|^2)
constexpr int IP_KP = IP_MAXK * IP_P;                  // one [K][P] or [P][K] array
constexpr int IP_FWD_EXTRA = IP_RED + 2 * IP_KP + IP_P;
constexpr int IP_BWD_EXTRA = IP_RED + 4 * IP_KP + 2 * IP_P;

__host__ __device__ __forceinline__ int ip_kpad(int K) { return (K + IP_KC - 1) / IP_KC * IP_KC; }

// the centres (and dq) transposed in chunks of eight parts, [KP / 8][C][8]: what a workgroup reads for a chunk is one
// contiguous C x 32-byte block, and the rows c and c + 1 of a chunk share a 64-byte line
__host__ __device__ __forceinline__ size_t ip_ct(int c, int k, int C) { return ((size_t)(k / IP_KC) * C + c) * IP_KC + k % IP_KC; }

__device__ __forceinline__ float ip_sigmoid(float s) { return 1.f / (1.f + expf(-s)); }

// centres [K][C] -> ct [KP / 8][C][8] (ip_ct; zero beyond K), csq [k] = |c_k|^2, beta [k] = sigmoid(s_k).  A workgroup per part.
__global__ __launch_bounds__(IP_THREADS) void ip_prep_kernel(const float* __restrict__ centres, const float* __restrict__ smooth,
                                                             float* __restrict__ ct, float* __restrict__ csq, float* __restrict__ beta,
                                                             int C, int K, int KP) {
#pragma clang fp contract(off)
    __shared__ float red[IP_WAVES];
    const int k = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += IP_THREADS) {
        const float v = centres[(size_t)k * C + c];
        ct[ip_ct(c, k, C)] = v;
        s = fmaf(v, v, s);
        if (k == 0)
            for (int j = K; j < KP; ++j) ct[ip_ct(c, j, C)] = 0.f;
    }
    s = block_sum<IP_WAVES>(s, red);
    if (threadIdx.x == 0) {
        csq[k] = s;
        beta[k] = ip_sigmoid(smooth[k]);
    }
}

// the tile: xs[c][p] = x[c][p0 + p], zero past the end of the row.  Thread t: four pixels (t & 7) of the rows t >> 3, + 32, ..
template <bool VEC>
__device__ __forceinline__ void ip_stage(float* xs, const float* __restrict__ xg, int C, int M, int p0) {
    constexpr int ROWS = IP_THREADS / 8, FLY = 8;          // eight 16-byte loads in flight per thread
    const int q = (threadIdx.x & 7) * 4;
    const bool in = p0 + q < M;
    for (int r0 = threadIdx.x >> 3; r0 < C; r0 += ROWS * FLY) {
        f32x4 v[FLY];
#pragma unroll
        for (int u = 0; u < FLY; ++u) {
            const int r = r0 + u * ROWS;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (in && r < C) v[u] = load4<VEC>(xg + (size_t)r * M, p0 + q, M);
        }
#pragma unroll
        for (int u = 0; u < FLY; ++u) {
            const int r = r0 + u * ROWS;
            if (r < C) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[r * IP_LD + q + e] = v[u][e];
            }
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void ip_unstage(const float* xs, float* __restrict__ xg, int C, int M, int p0) {
    const int q = (threadIdx.x & 7) * 4;
    for (int r = threadIdx.x >> 3; r < C; r += IP_THREADS / 8) {
        if (p0 + q < M) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = xs[r * IP_LD + q + e];
            store4<VEC>(xg + (size_t)r * M, p0 + q, M, v);
        }
    }
}

// out[(k0 + j)][p] = sum_c wt[c][k0 + j] xs[c][p] for j < 8 (and xsq[p] = sum_c xs[c][p]^2 with XSQ): thread (p, slice s) adds
// the channels s, s + 8, .. in order, the eight slices meet in LDS in slice order.  A row of a chunk of wt is 32 bytes that the
// 32 lanes of a slice share; a wave's two slices read one 64-byte line.  The loop is latency-bound (one wave per SIMD), so
// FLY iterations' loads are issued together.  Every thread calls it; ends on a barrier.
template <bool XSQ, int FLY>
__device__ __forceinline__ void ip_dots(const float* xs, const float* __restrict__ wt, int C, int KP, int k0, float* red, float* out,
                                        float* xsq) {
    const int p = threadIdx.x & (IP_P - 1), s = threadIdx.x / IP_P;
    float acc[IP_KC], xq = 0.f;
#pragma unroll
    for (int j = 0; j < IP_KC; ++j) acc[j] = 0.f;
#pragma unroll FLY
    for (int c = s; c < C; c += IP_SL) {                   // FLY rows' loads in flight: the registers of one wave per SIMD allow it
        const float* w = wt + ip_ct(c, k0, C);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(w), w1 = *reinterpret_cast<const f32x4*>(w + 4);
        const float xv = xs[c * IP_LD + p];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf(w0[j], xv, acc[j]);
            acc[4 + j] = fmaf(w1[j], xv, acc[4 + j]);
        }
        if (XSQ) xq = fmaf(xv, xv, xq);
    }
#pragma unroll
    for (int j = 0; j < IP_KC; ++j) red[(s * (IP_KC + 1) + j) * IP_P + p] = acc[j];
    if (XSQ) red[(s * (IP_KC + 1) + IP_KC) * IP_P + p] = xq;
    __syncthreads();
    {
        const int j = s;                                   // IP_SL == IP_KC: a thread per (part of the chunk, pixel)
        float t = 0.f, u = 0.f;
#pragma unroll
        for (int i = 0; i < IP_SL; ++i) {
            t += red[(i * (IP_KC + 1) + j) * IP_P + p];
            if (XSQ && j == 0) u += red[(i * (IP_KC + 1) + IP_KC) * IP_P + p];
        }
        out[(k0 + j) * IP_P + p] = t;
        if (XSQ && j == 0) xsq[p] = u;
    }
    __syncthreads();
}
static_assert(IP_SL == IP_KC, "ip_dots adds the slices with a thread per part of the chunk");

// out[k][c] = sum_p wl[p][k] xs[c][p]: a thread per channel, the pixels in order; its four channels share the reads of wl
__device__ __forceinline__ void ip_weighted(const float* xs, const float* wl, float* __restrict__ out, int C, int K) {
    constexpr int NCH = IP_MAXC / IP_THREADS;
    for (int k0 = 0; k0 < K; k0 += IP_KC) {
        float acc[NCH][IP_KC];
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int j = 0; j < IP_KC; ++j) acc[i][j] = 0.f;
#pragma unroll 4
        for (int p = 0; p < IP_P; ++p) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl + p * IP_MAXK + k0);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(wl + p * IP_MAXK + k0 + 4);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = threadIdx.x + i * IP_THREADS;
                const float xv = c < C ? xs[c * IP_LD + p] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = fmaf(w0[j], xv, acc[i][j]);
                    acc[i][4 + j] = fmaf(w1[j], xv, acc[i][4 + j]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = threadIdx.x + i * IP_THREADS;
#pragma unroll
            for (int j = 0; j < IP_KC; ++j)
                if (c < C && k0 + j < K) out[(size_t)(k0 + j) * C + c] = acc[i][j];
        }
    }
}

// the reference's logit: min(0, 2 <c, x> - |x|^2 - |c|^2) / beta, in its order of subtraction
__device__ __forceinline__ float ip_raw(float dot, float xsq, float csq) { return (2.f * dot - xsq) - csq; }

template <bool VEC>
__global__ __launch_bounds__(IP_THREADS) void ip_group_fwd_kernel(const float* __restrict__ x, const float* __restrict__ ct,
                                                                  const float* __restrict__ csq, const float* __restrict__ beta,
                                                                  float* __restrict__ assign, float* __restrict__ qpart,
                                                                  float* __restrict__ spart, int C, int K, int KP, int M, int T) {
#pragma clang fp contract(off)
    HK_DYN_LDS16(lds);
    float* xs = lds;
    float* red = xs + C * IP_LD;
    float* dots = red + IP_RED;
    float* at = dots + IP_KP;
    float* xsq = at + IP_KP;
    const int n = blockIdx.x / T, tile = blockIdx.x - n * T, p0 = tile * IP_P;
    ip_stage<VEC>(xs, x + (size_t)n * C * M, C, M, p0);
    __syncthreads();
    ip_dots<true, 16>(xs, ct, C, KP, 0, red, dots, xsq);
    for (int k0 = IP_KC; k0 < K; k0 += IP_KC) ip_dots<false, 16>(xs, ct, C, KP, k0, red, dots, xsq);
    {
        // the softmax over K: thread (p, s) owns the parts s, s + 8, ..; the maximum and the sum run over every part in order
        const int p = threadIdx.x & (IP_P - 1), s = threadIdx.x / IP_P;
        const bool valid = p0 + p < M;
        const float xq = xsq[p];
        float* ex = red;                                   // exp(l - max) [k][p]
        for (int k = s; k < K; k += IP_SL) dots[k * IP_P + p] = fminf(ip_raw(dots[k * IP_P + p], xq, csq[k]), 0.f) / beta[k];
        __syncthreads();
        float mx = -INFINITY, sum = 0.f;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, dots[k * IP_P + p]);
        for (int k = s; k < K; k += IP_SL) ex[k * IP_P + p] = expf(dots[k * IP_P + p] - mx);
        __syncthreads();
        for (int k = 0; k < K; ++k) sum += ex[k * IP_P + p];
        for (int k = s; k < KP; k += IP_SL) {
            float a = 0.f;
            if (valid && k < K) {
                a = ex[k * IP_P + p] / sum;
                assign[((size_t)n * K + k) * M + p0 + p] = a;
            }
            at[p * IP_MAXK + k] = a;
        }
    }
    __syncthreads();
    if (threadIdx.x < K) {
        float s = 0.f;
        for (int p = 0; p < IP_P; ++p) s += at[p * IP_MAXK + threadIdx.x];
        spart[(size_t)blockIdx.x * K + threadIdx.x] = s;
    }
    ip_weighted(xs, at, qpart + (size_t)blockIdx.x * K * C, C, K);
}

// a workgroup per (sample, part): q and S from the tiles' shares in tile order, then the clamp, the residual, 1 / sigma and
// the normalisation; outputs_t [N][C][K]
__global__ __launch_bounds__(IP_THREADS) void ip_group_fwd_finish_kernel(const float* __restrict__ qpart, const float* __restrict__ spart,
                                                                         const float* __restrict__ centres, const float* __restrict__ beta,
                                                                         float* __restrict__ outputs_t, float* __restrict__ S,
                                                                         float* __restrict__ nrm, int C, int K, int T) {
#pragma clang fp contract(off)
    __shared__ float red[IP_WAVES];
    const int n = blockIdx.x / K, k = blockIdx.x - n * K;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += spart[((size_t)n * T + t) * K + k];
    const float sc = fmaxf(s, IP_S_MIN), sigma = sqrtf(beta[k] / 2.f);
    float o[IP_MAXC / IP_THREADS], ss = 0.f;
#pragma unroll
    for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) o[i] = 0.f;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {                          // each channel's sum in tile order; the channels' loads in flight together
        const float* qp = qpart + (((size_t)n * T + t) * K + k) * C;
#pragma unroll
        for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) {
            const int c = threadIdx.x + i * IP_THREADS;
            if (c < C) o[i] += qp[c];
        }
    }
#pragma unroll
    for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) {
        const int c = threadIdx.x + i * IP_THREADS;
        if (c < C) {
            o[i] = (o[i] / sc - centres[(size_t)k * C + c]) / sigma;
            ss = fmaf(o[i], o[i], ss);
        }
    }
    ss = block_sum<IP_WAVES>(ss, red);
    const float nr = sqrtf(ss), den = fmaxf(nr, IP_N_MIN);
#pragma unroll
    for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) {
        const int c = threadIdx.x + i * IP_THREADS;
        if (c < C) outputs_t[((size_t)n * C + c) * K + k] = o[i] / den;
    }
    if (threadIdx.x == 0) {
        S[blockIdx.x] = s;
        nrm[blockIdx.x] = nr;
    }
}

// a workgroup per (sample, part): d_outputs_t -> dq (transposed per sample like the centres, zero beyond K), g = do / sigma [n][k][C] (the direct
// share of d_centres is - sum_n g), dS [n][k] (zero where the clamp of S is active) and dsig [n][k] = d loss / d sigma_k
__global__ __launch_bounds__(IP_THREADS) void ip_group_bwd_prep_kernel(const float* __restrict__ outputs_t, const float* __restrict__ dY,
                                                                       const float* __restrict__ centres, const float* __restrict__ smooth,
                                                                       const float* __restrict__ S, const float* __restrict__ nrm,
                                                                       float* __restrict__ dqt, float* __restrict__ gbuf,
                                                                       float* __restrict__ dS, float* __restrict__ dsig, int C, int K, int KP) {
#pragma clang fp contract(off)
    __shared__ float red[IP_WAVES];
    const int n = blockIdx.x / K, k = blockIdx.x - n * K;
    const float s = S[blockIdx.x], sc = fmaxf(s, IP_S_MIN), nr = nrm[blockIdx.x], den = fmaxf(nr, IP_N_MIN);
    const float sigma = sqrtf(ip_sigmoid(smooth[k]) / 2.f);
    float y[IP_MAXC / IP_THREADS], dy[IP_MAXC / IP_THREADS], dot = 0.f;
#pragma unroll
    for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) {
        const int c = threadIdx.x + i * IP_THREADS;
        y[i] = dy[i] = 0.f;
        if (c < C) {
            y[i] = outputs_t[((size_t)n * C + c) * K + k];
            dy[i] = dY ? dY[((size_t)n * C + c) * K + k] : 0.f;
            dot = fmaf(y[i], dy[i], dot);
        }
    }
    dot = block_sum<IP_WAVES>(dot, red);
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int i = 0; i < IP_MAXC / IP_THREADS; ++i) {
        const int c = threadIdx.x + i * IP_THREADS;
        if (c < C) {
            const float d_o = nr > IP_N_MIN ? (dy[i] - y[i] * dot) / den : dy[i] / den;
            const float o = y[i] * den, g = d_o / sigma;
            dqt[(size_t)n * C * KP + ip_ct(c, k, C)] = g / sc;
            gbuf[((size_t)n * K + k) * C + c] = g;
            t1 = fmaf(g, fmaf(o, sigma, centres[(size_t)k * C + c]), t1);       // q / S = o sigma + c
            t2 = fmaf(d_o, o, t2);
            if (k == 0)
                for (int j = K; j < KP; ++j) dqt[(size_t)n * C * KP + ip_ct(c, j, C)] = 0.f;
        }
    }
    t1 = block_sum<IP_WAVES>(t1, red);
    t2 = block_sum<IP_WAVES>(t2, red);
    if (threadIdx.x == 0) {
        dS[blockIdx.x] = s >= IP_S_MIN ? -t1 / sc : 0.f;
        dsig[blockIdx.x] = -t2 / sigma;
    }
}

template <bool VEC>
__global__ __launch_bounds__(IP_THREADS) void ip_group_bwd_kernel(const float* __restrict__ x, const float* __restrict__ ct,
                                                                  const float* __restrict__ csq, const float* __restrict__ beta,
                                                                  const float* __restrict__ dqt, const float* __restrict__ dS,
                                                                  const float* __restrict__ d_assign, float* __restrict__ dx,
                                                                  float* __restrict__ dcpart, float* __restrict__ dpart,
                                                                  float* __restrict__ bpart, int C, int K, int KP, int M, int T) {
#pragma clang fp contract(off)
    HK_DYN_LDS16(lds);
    float* xs = lds;
    float* red = xs + C * IP_LD;
    float* dots = red + IP_RED;                            // <c_k, x_p>
    float* dots2 = dots + IP_KP;                           // <dq_k, x_p>, later dl l / beta
    float* at = dots2 + IP_KP;                             // a [p][k]
    float* dt = at + IP_KP;                                // d raw [p][k]
    float* xsq = dt + IP_KP;
    float* rs = xsq + IP_P;                                // sum_k d raw [p]
    const int n = blockIdx.x / T, tile = blockIdx.x - n * T, p0 = tile * IP_P;
    const float* dqn = dqt + (size_t)n * C * KP;
    ip_stage<VEC>(xs, x + (size_t)n * C * M, C, M, p0);
    __syncthreads();
    ip_dots<true, 16>(xs, ct, C, KP, 0, red, dots, xsq);
    for (int k0 = IP_KC; k0 < K; k0 += IP_KC) ip_dots<false, 16>(xs, ct, C, KP, k0, red, dots, xsq);
    for (int k0 = 0; k0 < K; k0 += IP_KC) ip_dots<false, 16>(xs, dqn, C, KP, k0, red, dots2, xsq);
    {
        // the softmax and its gradient chain: thread (p, s) owns the parts s, s + 8, ..; every sum over K runs over all the
        // parts in order
        const int p = threadIdx.x & (IP_P - 1), s = threadIdx.x / IP_P;
        const bool valid = p0 + p < M;
        const float xq = xsq[p];
        float* lg = red;                                   // l [k][p]
        float* av = red + IP_KP;                           // exp(l - max), then a [k][p]
        for (int k = s; k < K; k += IP_SL) {
            const float raw = ip_raw(dots[k * IP_P + p], xq, csq[k]);
            dots[k * IP_P + p] = raw;                      // its sign is the clamp's mask
            lg[k * IP_P + p] = fminf(raw, 0.f) / beta[k];
        }
        __syncthreads();
        float mx = -INFINITY, sum = 0.f, inner = 0.f;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, lg[k * IP_P + p]);
        for (int k = s; k < K; k += IP_SL) av[k * IP_P + p] = expf(lg[k * IP_P + p] - mx);
        __syncthreads();
        for (int k = 0; k < K; ++k) sum += av[k * IP_P + p];
        __syncthreads();                                   // av is overwritten from here on
        for (int k = s; k < K; k += IP_SL) {               // da = d_assign + <dq_k, x_p> + dS_k, kept where <dq_k, x_p> was
            const float ext = (d_assign && valid) ? d_assign[((size_t)n * K + k) * M + p0 + p] : 0.f;
            dots2[k * IP_P + p] = (ext + dots2[k * IP_P + p]) + dS[(size_t)n * K + k];
            av[k * IP_P + p] = av[k * IP_P + p] / sum;
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) inner = fmaf(av[k * IP_P + p], dots2[k * IP_P + p], inner);
        __syncthreads();                                   // dots2 is overwritten from here on
        for (int k = s; k < KP; k += IP_SL) {
            float a = 0.f, dr = 0.f, bl = 0.f;
            if (valid && k < K) {
                const float raw = dots[k * IP_P + p], b = beta[k], l = lg[k * IP_P + p];
                a = av[k * IP_P + p];
                const float dl = a * (dots2[k * IP_P + p] - inner);
                dr = raw <= 0.f ? dl / b : 0.f;
                bl = dl * l / b;
            }
            at[p * IP_MAXK + k] = a;
            dt[p * IP_MAXK + k] = dr;
            if (k < K) dots2[k * IP_P + p] = bl;
        }
    }
    __syncthreads();
    if (threadIdx.x < IP_P) {
        float r = 0.f;
        for (int k = 0; k < KP; ++k) r += dt[threadIdx.x * IP_MAXK + k];
        rs[threadIdx.x] = r;
    }
    if (threadIdx.x < K) {
        float d = 0.f, b = 0.f;
        for (int p = 0; p < IP_P; ++p) {
            d += dt[p * IP_MAXK + threadIdx.x];
            b += dots2[threadIdx.x * IP_P + p];
        }
        dpart[(size_t)blockIdx.x * K + threadIdx.x] = d;
        bpart[(size_t)blockIdx.x * K + threadIdx.x] = -b;
    }
    if (dcpart) ip_weighted(xs, dt, dcpart + (size_t)blockIdx.x * K * C, C, K);
    if (!dx) return;                                       // block-uniform
    __syncthreads();                                       // the tile is overwritten from here on
    {
        // dX[c][p] = sum_k (2 draw[k][p] c_k[c] + a[k][p] dq[k][c]) - 2 x[c][p] sum_k draw[k][p], built in place: thread (p, s)
        // owns the channels s, s + 8, .. of pixel p
        const int p = threadIdx.x & (IP_P - 1), s = threadIdx.x / IP_P;
        const float r = rs[p];
        for (int k0 = 0; k0 < K; k0 += IP_KC) {
            float a8[IP_KC], d8[IP_KC];
#pragma unroll
            for (int j = 0; j < IP_KC; ++j) {
                a8[j] = at[p * IP_MAXK + k0 + j];
                d8[j] = 2.f * dt[p * IP_MAXK + k0 + j];
            }
#pragma unroll 8
            for (int c = s; c < C; c += IP_SL) {           // eight rows' loads in flight, as in ip_dots
                const float* wr = ct + ip_ct(c, k0, C);
                const float* gr = dqn + ip_ct(c, k0, C);
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(wr), w1 = *reinterpret_cast<const f32x4*>(wr + 4);
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(gr), g1 = *reinterpret_cast<const f32x4*>(gr + 4);
                float v = xs[c * IP_LD + p];
                if (k0 == 0) v = (-2.f * v) * r;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v = fmaf(d8[j], w0[j], v);
                    v = fmaf(a8[j], g0[j], v);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v = fmaf(d8[4 + j], w1[j], v);
                    v = fmaf(a8[4 + j], g1[j], v);
                }
                xs[c * IP_LD + p] = v;
            }
        }
    }
    __syncthreads();
    ip_unstage<VEC>(xs, dx + (size_t)n * C * M, C, M, p0);
}

// d_centres [k][c] = 2 sum_tiles dcpart - 2 c_k[c] sum_tiles dpart - sum_n g ; d_smooth [k] through beta.  Grid (K, C / 64):
// 64 channels per workgroup, the N T shares in four contiguous quarters (a wave each) that meet in LDS in quarter order.
__global__ __launch_bounds__(IP_THREADS) void ip_group_bwd_finish_kernel(const float* __restrict__ dcpart, const float* __restrict__ dpart,
                                                                         const float* __restrict__ bpart, const float* __restrict__ gbuf,
                                                                         const float* __restrict__ dsig, const float* __restrict__ centres,
                                                                         const float* __restrict__ smooth, float* __restrict__ d_centres,
                                                                         float* __restrict__ d_smooth, int N, int C, int K, int T) {
#pragma clang fp contract(off)
    __shared__ float part[IP_WAVES][WAVE];
    __shared__ float red[IP_WAVES];
    const int k = blockIdx.x, lane = threadIdx.x & 63, quarter = threadIdx.x >> 6, c = blockIdx.y * WAVE + lane;
    const int NT = N * T, per = (NT + IP_WAVES - 1) / IP_WAVES;
    const int lo = quarter * per, hi = lo + per < NT ? lo + per : NT;
    if (d_centres) {                                       // block-uniform
        float s = 0.f;
        if (dcpart)
            for (int i = lo; i < hi; ++i) s += dcpart[((size_t)i * K + k) * C + c];
        part[quarter][lane] = s;
        float d = 0.f;
        for (int i = threadIdx.x; i < NT; i += IP_THREADS) d += dpart[(size_t)i * K + k];
        d = block_sum<IP_WAVES>(d, red);                   // has the barriers that publish `part`
        if (quarter == 0) {
            const float tot = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
            float g = 0.f;
            for (int n = 0; n < N; ++n) g += gbuf[((size_t)n * K + k) * C + c];
            d_centres[(size_t)k * C + c] = (2.f * tot - (2.f * centres[(size_t)k * C + c]) * d) - g;
        }
    }
    if (d_smooth && blockIdx.y == 0) {                     // block-uniform
        float b = 0.f;
        for (int i = threadIdx.x; i < NT; i += IP_THREADS) b += bpart[(size_t)i * K + k];
        b = block_sum<IP_WAVES>(b, red);
        if (threadIdx.x == 0) {
            float sg = 0.f;
            for (int n = 0; n < N; ++n) sg += dsig[(size_t)n * K + k];
            const float be = ip_sigmoid(smooth[k]), sigma = sqrtf(be / 2.f);
            const float dbeta = b + sg / (4.f * sigma);    // sigma = sqrt(beta / 2): d sigma / d beta = 1 / (4 sigma)
            d_smooth[k] = dbeta * (be * (1.f - be));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- loss
constexpr int IL_THREADS = 1024;
constexpr int IL_WAVES = IL_THREADS / WAVE;
constexpr int IL_MAX_N = 4096;                         // the ranks take N comparisons per maximum
constexpr int IL_MAX_R = 15;
constexpr long long IL_MAX_WIDTH = 1 << 24;
constexpr float IL_EPS = 1e-5f;

// a workgroup per (sample, part): its slice of d_assign zeroed, the valid correlation with the window, the maximum and the
// lowest flat index that holds it
__global__ __launch_bounds__(IP_THREADS) void ip_loss_occ_kernel(const float* __restrict__ assign, const float* __restrict__ window,
                                                                 float* __restrict__ d_assign, float* __restrict__ occ,
                                                                 int* __restrict__ arg, int H, int W, int R) {
#pragma clang fp contract(off)
    __shared__ float bv[IP_WAVES];
    __shared__ int bi[IP_WAVES];
    const float* a = assign + (size_t)blockIdx.x * H * W;
    float* da = d_assign + (size_t)blockIdx.x * H * W;
    for (int i = threadIdx.x; i < H * W; i += IP_THREADS) da[i] = 0.f;
    const int D = 2 * R + 1, OH = H - 2 * R, OW = W - 2 * R;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int i = threadIdx.x; i < OH * OW; i += IP_THREADS) {
        const int oi = i / OW, oj = i - oi * OW;
        float v = 0.f;
        for (int u = 0; u < D; ++u)
            for (int w = 0; w < D; ++w) v = fmaf(window[u * D + w], a[(oi + u) * W + oj + w], v);
        if (v > best || at == 0x7fffffff) {                // ascending i: the first maximum is the lowest index
            best = v;
            at = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(at, o, 64);
        if (oi != 0x7fffffff && (at == 0x7fffffff || ov > best || (ov == best && oi < at))) {
            best = ov;
            at = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        bv[threadIdx.x >> 6] = best;
        bi[threadIdx.x >> 6] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < IP_WAVES; ++w)
            if (bi[w] != 0x7fffffff && (at == 0x7fffffff || bv[w] > best || (bv[w] == best && bi[w] < at))) {
                best = bv[w];
                at = bi[w];
            }
        occ[blockIdx.x] = best;
        arg[blockIdx.x] = at;
    }
}

struct IpLossArgs {
    const float* logits;           // [N,classes]
    const int64_t* labels;         // [N]
    const float* window;           // [(2R+1)^2]
    const float* prior;            // [N]
    const float* occ;              // [N,K]
    const int* arg;                // [N,K]
    float coeff;
    float* terms;                  // [3]
    float* d_logits;
    float* d_assign;
    int N, classes, K, H, W, R;
};

__global__ __launch_bounds__(IL_THREADS) void ip_loss_kernel(const IpLossArgs A) {
#pragma clang fp contract(off)
    __shared__ float red[IL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = A.N, K = A.K, D = 2 * A.R + 1, OW = A.W - 2 * A.R;
    float ce = 0.f;
    for (int b = wave; b < N; b += IL_WAVES) {                                      // a wave per sample, in ascending order
        const long long yl = A.labels[b];
        const int y = (yl >= 0 && yl < A.classes) ? (int)yl : -1;
        const float* row = A.logits + (size_t)b * A.classes;
        const CeRow r = ce_row_stats(row, A.classes, y, 0.f);
        ce_row_grad(row, A.d_logits + (size_t)b * A.classes, A.classes, y, 0.f, r, 1.f / (float)N, 0.f);
        ce += r.ce;
    }
    __syncthreads();
    if (lane == 0) red[wave] = ce;
    __syncthreads();
    float cet = 0.f;
    for (int i = 0; i < IL_WAVES; ++i) cet += red[i];
    const float count = (float)N * (float)K;
    float sh = 0.f;
    for (int i = threadIdx.x; i < N * K; i += IL_THREADS) {
        const int n = i / K, k = i - n * K;
        const float v = A.occ[i];
        int rank = 0;
        for (int m = 0; m < N; ++m) {
            const float o = A.occ[(size_t)m * K + k];
            rank += (o < v || (o == v && m < n)) ? 1 : 0;                           // the lower sample first on a tie
        }
        const float d = logf(v + IL_EPS) - logf(A.prior[rank] + IL_EPS);
        sh += fabsf(d);
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == d ? 0.f : d));
        const float g = ((A.coeff * sgn) / (v + IL_EPS)) / count;
        const int at = A.arg[i], oi = at / OW, oj = at - oi * OW;
        float* da = A.d_assign + (size_t)i * A.H * A.W;
        for (int u = 0; u < D; ++u)
            for (int w = 0; w < D; ++w) da[(oi + u) * A.W + oj + w] = g * A.window[u * D + w];
    }
    sh = block_sum<IL_WAVES>(sh, red);
    if (threadIdx.x == 0) {
        const float cem = cet / (float)N, shm = sh / count;
        A.terms[0] = cem + A.coeff * shm;
        A.terms[1] = cem;
        A.terms[2] = shm;
    }
}

// ------------------------------------------------------------------------------------------------------------- host
struct IpSizes {
    int KP, M, T;
    size_t lds_fwd, lds_bwd;
};

static int group_sizes(int N, int C, int K, int H, int W, IpSizes& z) {
    if (N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0) return HK_ERR_BAD_ARG;
    if (K > IP_MAXK || C % 64 != 0 || C > IP_MAXC) return HK_ERR_UNSUPPORTED;
    if ((long long)H * W > 0x7fffffffLL - IP_P) return HK_ERR_UNSUPPORTED;
    z.KP = ip_kpad(K);
    z.M = H * W;
    z.T = (z.M + IP_P - 1) / IP_P;
    if ((long long)N * z.T > 0x7fffffffLL / IP_MAXK || (long long)N * K > 0x7fffffffLL) return HK_ERR_UNSUPPORTED;
    z.lds_fwd = ((size_t)C * IP_LD + IP_FWD_EXTRA) * sizeof(float);
    z.lds_bwd = ((size_t)C * IP_LD + IP_BWD_EXTRA) * sizeof(float);
    return HK_OK;
}

static size_t al4(size_t floats) { return (floats + 3) & ~(size_t)3; }      // every piece of a workspace starts 16-byte aligned

static size_t group_fwd_need(int N, int C, int K, const IpSizes& z) {
    return (al4((size_t)C * z.KP) + 2 * al4(z.KP) + al4((size_t)N * z.T * K * C) + al4((size_t)N * z.T * K)) * sizeof(float) + 256;
}

static size_t group_bwd_need(int N, int C, int K, const IpSizes& z) {
    return (al4((size_t)C * z.KP) + 2 * al4(z.KP) + al4((size_t)N * C * z.KP) + al4((size_t)N * K * C) + 2 * al4((size_t)N * K) +
            al4((size_t)N * z.T * K * C) + 2 * al4((size_t)N * z.T * K)) * sizeof(float) + 256;
}

static size_t loss_need(int N, int K) { return 2 * al4((size_t)N * K) * sizeof(float) + 256; }

}  // namespace hk

using namespace hk;

extern "C" size_t hk_ip_group_fwd_ws_bytes(int N, int C, int K, int H, int W) {
    IpSizes z;
    return group_sizes(N, C, K, H, W, z) == HK_OK ? group_fwd_need(N, C, K, z) : 0;
}

extern "C" int hk_ip_group_fwd(const float* x, const float* centres, const float* smooth, float* outputs_t, float* assign, float* S,
                               float* nrm, int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!x || !centres || !smooth || !outputs_t || !assign || !S || !nrm || N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0)
        return HK_ERR_BAD_ARG;
    IpSizes z;
    const int rc = group_sizes(N, C, K, H, W, z);
    if (rc != HK_OK) return rc;
    if (!ws || !aligned16(ws) || ws_bytes < group_fwd_need(N, C, K, z)) return HK_ERR_WORKSPACE;
    float* ct = (float*)ws;
    float* csq = ct + al4((size_t)C * z.KP);
    float* beta = csq + al4(z.KP);
    float* qpart = beta + al4(z.KP);
    float* spart = qpart + al4((size_t)N * z.T * K * C);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ip_prep_kernel, dim3((unsigned)K), dim3(IP_THREADS), 0, st, centres, smooth, ct, csq, beta, C, K, z.KP);
    HK_LAUNCH_CHECK();
    const dim3 grid((unsigned)(N * z.T)), block(IP_THREADS);
    if ((z.M & 3) == 0 && aligned16(x)) {
        HK_ALLOW_BIG_LDS((&ip_group_fwd_kernel<true>), z.lds_fwd);
        hipLaunchKernelGGL((ip_group_fwd_kernel<true>), grid, block, z.lds_fwd, st, x, ct, csq, beta, assign, qpart, spart, C, K, z.KP, z.M,
                           z.T);
    } else {
        HK_ALLOW_BIG_LDS((&ip_group_fwd_kernel<false>), z.lds_fwd);
        hipLaunchKernelGGL((ip_group_fwd_kernel<false>), grid, block, z.lds_fwd, st, x, ct, csq, beta, assign, qpart, spart, C, K, z.KP, z.M,
                           z.T);
    }
    HK_LAUNCH_CHECK();
    hipLaunchKernelGGL(ip_group_fwd_finish_kernel, dim3((unsigned)(N * K)), block, 0, st, qpart, spart, centres, beta, outputs_t, S, nrm, C,
                       K, z.T);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" size_t hk_ip_group_bwd_ws_bytes(int N, int C, int K, int H, int W) {
    IpSizes z;
    return group_sizes(N, C, K, H, W, z) == HK_OK ? group_bwd_need(N, C, K, z) : 0;
}

extern "C" int hk_ip_group_bwd(const float* x, const float* centres, const float* smooth, const float* outputs_t, const float* S,
                               const float* nrm, const float* d_outputs_t, const float* d_assign, float* dx, float* d_centres,
                               float* d_smooth, int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!x || !centres || !smooth || !outputs_t || !S || !nrm || N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0) return HK_ERR_BAD_ARG;
    IpSizes z;
    const int rc = group_sizes(N, C, K, H, W, z);
    if (rc != HK_OK) return rc;
    if (!ws || !aligned16(ws) || ws_bytes < group_bwd_need(N, C, K, z)) return HK_ERR_WORKSPACE;
    if (!dx && !d_centres && !d_smooth) return HK_OK;
    float* ct = (float*)ws;
    float* csq = ct + al4((size_t)C * z.KP);
    float* beta = csq + al4(z.KP);
    float* dqt = beta + al4(z.KP);
    float* gbuf = dqt + al4((size_t)N * C * z.KP);
    float* dS = gbuf + al4((size_t)N * K * C);
    float* dsig = dS + al4((size_t)N * K);
    float* dcpart = dsig + al4((size_t)N * K);
    float* dpart = dcpart + al4((size_t)N * z.T * K * C);
    float* bpart = dpart + al4((size_t)N * z.T * K);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(IP_THREADS);
    hipLaunchKernelGGL(ip_prep_kernel, dim3((unsigned)K), block, 0, st, centres, smooth, ct, csq, beta, C, K, z.KP);
    HK_LAUNCH_CHECK();
    hipLaunchKernelGGL(ip_group_bwd_prep_kernel, dim3((unsigned)(N * K)), block, 0, st, outputs_t, d_outputs_t, centres, smooth, S, nrm, dqt,
                       gbuf, dS, dsig, C, K, z.KP);
    HK_LAUNCH_CHECK();
    const dim3 grid((unsigned)(N * z.T));
    float* dcp = d_centres ? dcpart : nullptr;
    if ((z.M & 3) == 0 && aligned16(x) && (!dx || aligned16(dx))) {
        HK_ALLOW_BIG_LDS((&ip_group_bwd_kernel<true>), z.lds_bwd);
        hipLaunchKernelGGL((ip_group_bwd_kernel<true>), grid, block, z.lds_bwd, st, x, ct, csq, beta, dqt, dS, d_assign, dx, dcp, dpart, bpart,
                           C, K, z.KP, z.M, z.T);
    } else {
        HK_ALLOW_BIG_LDS((&ip_group_bwd_kernel<false>), z.lds_bwd);
        hipLaunchKernelGGL((ip_group_bwd_kernel<false>), grid, block, z.lds_bwd, st, x, ct, csq, beta, dqt, dS, d_assign, dx, dcp, dpart, bpart,
                           C, K, z.KP, z.M, z.T);
    }
    HK_LAUNCH_CHECK();
    if (d_centres || d_smooth) {
        hipLaunchKernelGGL(ip_group_bwd_finish_kernel, dim3((unsigned)K, (unsigned)(d_centres ? C / WAVE : 1)), block, 0, st, dcp, dpart, bpart,
                           gbuf, dsig, centres, smooth, d_centres, d_smooth, N, C, K, z.T);
        HK_LAUNCH_CHECK();
    }
    return HK_OK;
}

extern "C" size_t hk_ip_loss_ws_bytes(int N, int K) { return (N > 0 && K > 0 && N <= IL_MAX_N && K <= IL_MAX_WIDTH) ? loss_need(N, K) : 0; }

extern "C" int hk_ip_loss(const float* logits, const int64_t* labels, const float* assign, const float* window, const float* prior,
                          float coeff, float* terms, float* d_logits, float* d_assign, int N, int classes, int K, int H, int W, int radius,
                          void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!logits || !labels || !assign || !window || !prior || !terms || !d_logits || !d_assign || N <= 0 || classes <= 0 || K <= 0 ||
        H <= 0 || W <= 0 || radius < 0)
        return HK_ERR_BAD_ARG;
    if (radius > IL_MAX_R) return HK_ERR_UNSUPPORTED;
    if (H < 2 * radius + 1 || W < 2 * radius + 1) return HK_ERR_BAD_ARG;           // the reference's conv2d raises there
    if (N > IL_MAX_N || classes > IL_MAX_WIDTH || K > IL_MAX_WIDTH || (long long)N * classes > 0x7fffffffLL ||
        (long long)N * K > 0x7fffffffLL || (long long)H * W > 0x7fffffffLL)
        return HK_ERR_UNSUPPORTED;
    if (!ws || !aligned16(ws) || ws_bytes < loss_need(N, K)) return HK_ERR_WORKSPACE;
    float* occ = (float*)ws;
    int* arg = (int*)(occ + al4((size_t)N * K));
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ip_loss_occ_kernel, dim3((unsigned)(N * K)), dim3(IP_THREADS), 0, st, assign, window, d_assign, occ, arg, H, W, radius);
    HK_LAUNCH_CHECK();
    IpLossArgs A;
    A.logits = logits; A.labels = labels; A.window = window; A.prior = prior; A.occ = occ; A.arg = arg;
    A.coeff = coeff; A.terms = terms; A.d_logits = d_logits; A.d_assign = d_assign;
    A.N = N; A.classes = classes; A.K = K; A.H = H; A.W = W; A.R = radius;
    hipLaunchKernelGGL(ip_loss_kernel, dim3(1), dim3(IL_THREADS), 0, st, A);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
