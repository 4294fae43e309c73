// MGE-CNN head (model/methods/MGE_CNN/MGE.py, grad_cam.py): the part pool behind conv6*, the Grad-CAM box and the criterion.
//
//   partpool fwd  replaces pool_max(relu(conv6(x))) with conv6 = Conv2d(Cin, Cout, 1, 1, padding = 1), MGE.py:135,166,197.  The padded
//                 map [B, Cout, H + 2, W + 2] is never written: its border ring is the bias alone, so
//                 pooled = relu(bias + max(0, max_p <w_o, x_p>)).  A batched GEMM W (Cout x Cin) by X_b (Cin x HW) on the fp32 MFMA
//                 (hk_bgemm.h) whose epilogue takes each row's maximum and first argmax over the tile's 64 columns - 32 lanes by
//                 butterfly, the two column halves through LDS - and writes one (value, pixel) pair per (image, row, column tile)
//                 to the workspace; a second launch walks the column tiles in ascending order.  Ties: the lowest pixel among
//                 interior ones, the border against the interior - the scan order of the reference's pool, whose first element is
//                 a border one.
//   partpool bwd  dW[o,:] = sum_b g[b,o] [pooled > 0] [argmax >= 0] x[b,:,argmax[b,o]], db[o] = sum_b g[b,o] [pooled > 0]: a gather, one
//                 workgroup per output channel, b in ascending order.  The reference runs a dense weight-gradient GEMM over a map of
//                 which one pixel per (image, channel) carries gradient.  No dx: the reference detaches the input.
//   cam_bbox      replaces GradCam.__call__ (an eval-mode forward and an autograd backward through layer4, grad_cam.py:65-90) and
//                 get_bbox's mask and box search (MGE.py:48-72: a [B,1,S,S] map, then per image nonzero(), four min / max and a
//                 tensor comparison in an `if`).  The target layer feeds AdaptiveAvgPool2d(1) and a Linear, so the CAM weight is
//                 relu(W[idx,c]) / (h w) in closed form.  One workgroup per image: the h x w CAM in LDS, the align-corners bilinear
//                 value at each of the S x S positions computed on the fly, twice - once for the map's minimum and range, once
//                 to flag in LDS the rows and columns with a normalised value >= rate -, the box read from the flags.
//   loss          K <= 16 label-smoothed cross entropies, their mean, and the K gradients of the mean: one workgroup, a wave per row
//                 (hk_rows.h), the terms added in a fixed order.  The reference trainer calls the criterion ten times.
// No atomics anywhere; every sum and every maximum in a fixed order.
#include <cmath>

#include "hk_bgemm.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

// ------------------------------------------------------------------------------------------------------- part pool
// is (vb, ib) the better candidate than (va, ia)?  The higher value, then the lower pixel index
__device__ __forceinline__ bool pool_better(float vb, int ib, float va, int ia) { return vb > va || (vb == va && ib < ia); }

struct EpRowMax {
    using Tile = void;
    float* pv;             // [B, M, tilesN] the tile's row maxima
    int32_t* pi;           // ... and the pixel that holds each
    __device__ __forceinline__ void operator()(int, int, int, float) const {}
    __device__ __forceinline__ void tile(int b, int tm, int tn, int tilesN, int M, int N, const f32x16& acc, float* lds) const {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
        float* sv = lds;                                   // [2][64]
        int* si = reinterpret_cast<int*>(lds + 128);       // [2][64]
        const int col = tn * 64 + wn * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = col < N ? acc[r] : -INFINITY;        // a column past the map never wins
            int i = col;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {             // the 32 lanes of a half wave hold one row
                const float ov = __shfl_xor(v, o, 64);
                const int oi = __shfl_xor(i, o, 64);
                if (pool_better(ov, oi, v, i)) { v = ov; i = oi; }
            }
            if (l31 == 0) {
                const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sv[wn * 64 + row] = v;
                si[wn * 64 + row] = i;
            }
        }
        __syncthreads();
        if (tid < 64 && tm * 64 + tid < M) {
            float v = sv[tid];
            int i = si[tid];
            if (pool_better(sv[64 + tid], si[64 + tid], v, i)) { v = sv[64 + tid]; i = si[64 + tid]; }
            const size_t at = ((size_t)b * M + tm * 64 + tid) * tilesN + tn;
            pv[at] = v;
            pi[at] = i;
        }
    }
};

__global__ __launch_bounds__(256) void mge_pool_finish_kernel(const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                              const float* __restrict__ bias, float* __restrict__ pooled,
                                                              int32_t* __restrict__ argmax, long long rows, int M, int tilesN) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;          // b M + o
    if (r >= rows) return;
    float v = pv[r * tilesN];
    int i = pi[r * tilesN];
    for (int t = 1; t < tilesN; ++t)                       // ascending pixels: a later tile wins only with a higher value
        if (pv[r * tilesN + t] > v) { v = pv[r * tilesN + t]; i = pi[r * tilesN + t]; }
    const bool inside = v > 0.f;                           // the border ring (response 0) comes first in the pool's scan
    const float z = bias[r % M] + (inside ? v : 0.f);
    pooled[r] = z > 0.f ? z : 0.f;
    argmax[r] = inside ? i : -1;
}

constexpr int POOL_BWD_THREADS = 256;

__global__ __launch_bounds__(POOL_BWD_THREADS) void mge_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                        const float* __restrict__ pooled, const int32_t* __restrict__ argmax,
                                                                        float* __restrict__ dw, float* __restrict__ db, int B, int Cin,
                                                                        int Cout, int HW) {
    const int o = blockIdx.x, tid = threadIdx.x;
    if (db && tid == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += pooled[(size_t)b * Cout + o] > 0.f ? g[(size_t)b * Cout + o] : 0.f;
        db[o] = s;
    }
    if (!dw) return;
    for (int c = tid; c < Cin; c += POOL_BWD_THREADS) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) {                      // (workgroup-uniform conditions)
            const size_t at = (size_t)b * Cout + o;
            const int p = argmax[at];
            if (!(pooled[at] > 0.f) || p < 0 || p >= HW) continue;
            s += g[at] * x[((size_t)b * Cin + c) * HW + p];
        }
        dw[(size_t)o * Cin + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------------- Grad-CAM box
constexpr int CAM_THREADS = 1024;
constexpr int CAM_WAVES = CAM_THREADS / WAVE;
constexpr int CAM_MAX_HW = 512;                            // the map in LDS with a share per wave: 17 x 2 KiB
constexpr int CAM_MAX_S = 2048;

__global__ __launch_bounds__(CAM_THREADS) void mge_cam_bbox_kernel(const float* __restrict__ conv5, const float* __restrict__ cls_weight,
                                                                   const int32_t* __restrict__ index, int32_t* __restrict__ boxes, int C,
                                                                   int h, int w, int classes, float rate, int S) {
    __shared__ float part[CAM_WAVES][CAM_MAX_HW];
    __shared__ float cam[CAM_MAX_HW];
    __shared__ float ext[4][CAM_WAVES];
    __shared__ int rowhit[CAM_MAX_S], colhit[CAM_MAX_S];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w;
    const int idx = index[b];
    const bool known = idx >= 0 && idx < classes;          // a class out of range reads nothing: the whole image
    const float* wrow = cls_weight + (size_t)(known ? idx : 0) * C;
    const float* x = conv5 + (size_t)b * C * hw;
    const float area = (float)hw;
    for (int p = lane; p < hw; p += WAVE) {
        float s = 0.f;
#pragma unroll 8
        for (int c = wave; c < C; c += CAM_WAVES) {
            const float a = wrow[c];
            s += ((a > 0.f ? a : 0.f) / area) * x[(size_t)c * hw + p];
        }
        part[wave][p] = s;
    }
    for (int i = tid; i < S; i += CAM_THREADS) { rowhit[i] = 0; colhit[i] = 0; }
    __syncthreads();
    for (int p = tid; p < hw; p += CAM_THREADS) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CAM_WAVES; ++k) s += part[k][p];
        cam[p] = s;
    }
    __syncthreads();
    // the minimum and range of the UPSAMPLED map, as the reference normalises: an interior cell is a sample only where S - 1 is a
    // multiple of h - 1, so these are not the CAM's own extremes (the corners alone are always sampled).  min / max: any order
    const float sy = S > 1 ? (float)(h - 1) / (float)(S - 1) : 0.f, sx = S > 1 ? (float)(w - 1) / (float)(S - 1) : 0.f;
    auto sample = [&](int q) {
        const int oy = q / S, ox = q % S;
        const float fy = sy * (float)oy, fx = sx * (float)ox;
        const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        return (1.f - ly) * ((1.f - lx) * cam[y0 * w + x0] + lx * cam[y0 * w + x1]) +
               ly * ((1.f - lx) * cam[y1 * w + x0] + lx * cam[y1 * w + x1]);
    };
    float mn = INFINITY, mx = -INFINITY;
    for (int q = tid; q < S * S; q += CAM_THREADS) {
        const float v = sample(q);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    // ... and the CAM's own: a constant CAM has no box, whatever the interpolation's rounding makes of it
    float cmn = INFINITY, cmx = -INFINITY;
    for (int p = tid; p < hw; p += CAM_THREADS) { cmn = fminf(cmn, cam[p]); cmx = fmaxf(cmx, cam[p]); }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    cmn = -wave_max(-cmn);
    cmx = wave_max(cmx);
    if (lane == 0) { ext[0][wave] = mn; ext[1][wave] = mx; ext[2][wave] = cmn; ext[3][wave] = cmx; }
    __syncthreads();
    mn = ext[0][0]; mx = ext[1][0]; cmn = ext[2][0]; cmx = ext[3][0];
#pragma unroll
    for (int k = 1; k < CAM_WAVES; ++k) {
        mn = fminf(mn, ext[0][k]); mx = fmaxf(mx, ext[1][k]);
        cmn = fminf(cmn, ext[2][k]); cmx = fmaxf(cmx, ext[3][k]);
    }
    const float range = mx - mn;
    const bool usable = known && cmx > cmn && range > 0.f && range < INFINITY;     // workgroup-uniform (a NaN or infinite map is not usable)
    if (usable)
        for (int q = tid; q < S * S; q += CAM_THREADS)
            if ((sample(q) - mn) / range >= rate) { rowhit[q / S] = 1; colhit[q % S] = 1; }      // every writer stores the same 1
    __syncthreads();
    if (tid == 0) {
        int ya = -1, yb = -1, xa = -1, xb = -1;
        if (usable)
            for (int i = 0; i < S; ++i) {
                if (rowhit[i]) { if (ya < 0) ya = i; yb = i; }
                if (colhit[i]) { if (xa < 0) xa = i; xb = i; }
            }
        // the reference slices [y1:y2, x1:x2] with the LAST hit as the exclusive end and takes the whole image when that is empty
        const bool whole = ya < 0 || ya == yb || xa == xb;
        int32_t* o = boxes + (size_t)b * 4;
        o[0] = whole ? 0 : ya;
        o[1] = whole ? 0 : xa;
        o[2] = whole ? S : yb;
        o[3] = whole ? S : xb;
    }
}

// ------------------------------------------------------------------------------------------------------- loss
constexpr int MGE_MAX_K = 16;
constexpr int MGE_LOSS_THREADS = 1024;
constexpr int MGE_LOSS_WAVES = MGE_LOSS_THREADS / WAVE;
constexpr long long MGE_MAX_ROWS = 1 << 22;

struct MgeLogits {
    const float* in[MGE_MAX_K];
    float* out[MGE_MAX_K];
};

__global__ __launch_bounds__(MGE_LOSS_THREADS) void mge_loss_kernel(MgeLogits t, const int32_t* __restrict__ labels, float smoothing,
                                                                    float* __restrict__ loss, float* ce_rows, int K, int B, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float wgt = 1.f / ((float)B * (float)K);
    for (int r = wave; r < K * B; r += MGE_LOSS_WAVES) {   // wave-uniform
        const int k = r / B, b = r % B, y = labels[b];
        const float* row = t.in[k] + (size_t)b * C;
        const CeRow s = ce_row_stats(row, C, y, smoothing);
        ce_row_grad(row, t.out[k] + (size_t)b * C, C, y, smoothing, s, wgt, 0.f);
        if (lane == 0) ce_rows[r] = s.ce;
    }
    __syncthreads();
    if (wave == 0) {
        float total = 0.f;
        for (int k = 0; k < K; ++k) {                      // the trainer's order: sum(losses) / len(losses)
            const float term = wave_total(ce_rows + (size_t)k * B, B) / (float)B;
            total += term;
            if (lane == 0) loss[1 + k] = term;
        }
        if (lane == 0) loss[0] = total / (float)K;
    }
}

}  // namespace hk

using namespace hk;

static bool pool_shape_ok(int B, int Cin, int Cout, int H, int W) {
    return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && Cin % 32 == 0 && (long long)H * W <= 0x3fffffff &&
           (long long)B * Cout * (((long long)H * W + 63) / 64) <= 0x3fffffff;
}

extern "C" size_t hk_mge_partpool_fwd_ws_bytes(int B, int Cin, int Cout, int H, int W) {
    if (!pool_shape_ok(B, Cin, Cout, H, W)) return 0;
    return (size_t)B * Cout * ((H * W + 63) / 64) * (sizeof(float) + sizeof(int32_t));
}

extern "C" int hk_mge_partpool_fwd(const float* x, const float* weight, const float* bias, float* pooled, int32_t* argmax, int B, int Cin,
                                   int Cout, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!x || !weight || !bias || !pooled || !argmax || !pool_shape_ok(B, Cin, Cout, H, W)) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_mge_partpool_fwd_ws_bytes(B, Cin, Cout, H, W)) return HK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, tilesN = (HW + 63) / 64;
    EpRowMax ep;
    ep.pv = (float*)ws;
    ep.pi = (int32_t*)(ep.pv + (size_t)B * Cout * tilesN);
    const LdPlain la = make_plain(weight, 0, Cin, Cout, Cin);
    const LdPlain lb = make_plain(x, (long long)Cin * HW, HW, Cin, HW);
    const int rc = bgemm_launch<true, false>(la, lb, ep, Cout, HW, Cin, B, st);
    if (rc != HK_OK) return rc;
    const long long rows = (long long)B * Cout;
    hipLaunchKernelGGL(mge_pool_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, ep.pv, ep.pi, bias, pooled, argmax,
                       rows, Cout, tilesN);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_mge_partpool_bwd(const float* x, const float* g, const float* pooled, const int32_t* argmax, float* dw, float* db, int B,
                                   int Cin, int Cout, int H, int W, hk_stream_t stream) {
    if (!x || !g || !pooled || !argmax || !pool_shape_ok(B, Cin, Cout, H, W)) return HK_ERR_BAD_ARG;
    if (!dw && !db) return HK_OK;
    hipLaunchKernelGGL(mge_pool_bwd_kernel, dim3(Cout), dim3(POOL_BWD_THREADS), 0, (hipStream_t)stream, x, g, pooled, argmax, dw, db, B, Cin,
                       Cout, H * W);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_mge_cam_bbox(const float* conv5, const float* cls_weight, const int32_t* index, int32_t* boxes, int B, int C, int h, int w,
                               int classes, float rate, int S, hk_stream_t stream) {
    if (!conv5 || !cls_weight || !index || !boxes || B <= 0 || C <= 0 || h <= 0 || w <= 0 || classes <= 0 || S <= 0 || !(rate == rate))
        return HK_ERR_BAD_ARG;
    if ((long long)h * w > CAM_MAX_HW || S > CAM_MAX_S) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mge_cam_bbox_kernel, dim3(B), dim3(CAM_THREADS), 0, (hipStream_t)stream, conv5, cls_weight, index, boxes, C, h, w,
                       classes, rate, S);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" size_t hk_mge_loss_ws_bytes(int K, int B) {
    if (K <= 0 || K > MGE_MAX_K || B <= 0 || (long long)K * B > MGE_MAX_ROWS) return 0;
    return (size_t)K * B * sizeof(float);
}

extern "C" int hk_mge_loss(const float* const* logits, const int32_t* labels, float smoothing, float* loss, float* const* d_logits, int K,
                           int B, int C, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!logits || !labels || !loss || !d_logits || K <= 0 || K > MGE_MAX_K || B <= 0 || C <= 0) return HK_ERR_BAD_ARG;
    if (!(smoothing >= 0.f && smoothing <= 1.f)) return HK_ERR_BAD_ARG;
    if ((long long)K * B > MGE_MAX_ROWS) return HK_ERR_UNSUPPORTED;
    MgeLogits t;
    for (int k = 0; k < MGE_MAX_K; ++k) {
        t.in[k] = k < K ? logits[k] : nullptr;
        t.out[k] = k < K ? d_logits[k] : nullptr;
        if (k < K && (!t.in[k] || !t.out[k])) return HK_ERR_BAD_ARG;
    }
    if (!ws || ws_bytes < hk_mge_loss_ws_bytes(K, B)) return HK_ERR_WORKSPACE;
    hipLaunchKernelGGL(mge_loss_kernel, dim3(1), dim3(MGE_LOSS_THREADS), 0, (hipStream_t)stream, t, labels, smoothing, loss, (float*)ws, K, B,
                       C);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
