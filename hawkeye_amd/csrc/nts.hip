// NTS-Net head (navigator - teacher - scrutinizer): proposal NMS, the part crops and the loss, with nothing leaving the
// device.  replaces model/methods/NTS_Net/NTSNet.py:29-47 with anchors.py:63-90 (a device-to-host copy of all proposal
// scores, a numpy greedy NMS per image, a zero-padded copy of the batch and B x topN separate F.interpolate calls) and
// model/loss/NTS_loss.py:15-47 (one .item() per part row, a Python loop over the proposals).
//
//   nms    one workgroup per image.  Thread t owns the anchors t, t + 256, .. (scores and boxes staged once, in registers);
//          topn rounds of: argmax over the live anchors (wave64 butterfly, then the four waves' winners through LDS), the
//          winner's box broadcast, every thread drops its anchors whose IoU with the winner is not < thresh.  The IoU is
//          hard_nms's: corner differences without + 1, intersection 0 when a side is negative - evaluated in float64 from
//          the integer corners, exactly the reference's arithmetic, so the decision is the reference's for every pair
//          (0 / 0 is NaN there and here: suppressed).  Equal scores: the highest index (a stable ascending sort read from
//          its end).  A NaN score counts as -inf.  A round without a live anchor repeats the last chosen one.
//   crop   out[b N + j] = bilinear resize (align_corners) of the box j of image b, cut out of the image as if it were
//          zero-padded by `pad` on every side; the padded tensor is never built.  One thread owns four neighbouring x of one
//          output row: its two source rows, eight source columns and the weights are computed once and serve every
//          channel; one 16-byte store per channel.  Write-bound: 14.4 MB at the yaml's batch against a source window that
//          stays in L2.
//   loss   one workgroup of 16 waves: a wave per row of the three logit matrices (statistics, gradient, the smoothed cross
//          entropy and, for part rows, the plain one), a barrier, a thread per (sample, proposal) for the gated ranking
//          hinge and its gradient, a barrier, wave 0 adds the per-row terms in a fixed order.  One launch, no atomics.
#include <cmath>

#include "hk_common.h"
#include "hk_rows.h"
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int NMS_THREADS = 256;
constexpr int NMS_WAVES = NMS_THREADS / WAVE;
constexpr int NMS_SLOTS = 8;
constexpr int NMS_MAX_A = NMS_THREADS * NMS_SLOTS;     // 2048; the default anchor set has 426 (224 x 224) or 1614 (448 x 448)

// (score, index) with index < 0 meaning "none": is `b` the better candidate?  Higher score, then the higher index.
__device__ __forceinline__ bool nms_better(float sb, int ib, float sa, int ia) {
    return ib >= 0 && (ia < 0 || sb > sa || (sb == sa && ib > ia));
}

__global__ __launch_bounds__(NMS_THREADS) void nts_nms_kernel(const float* __restrict__ scores, const int32_t* __restrict__ anchors,
                                                              int32_t* __restrict__ index, int32_t* __restrict__ boxes, int A, int topn,
                                                              double thresh) {
    __shared__ float sd[2][NMS_WAVES];
    __shared__ int si[2][NMS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float sc[NMS_SLOTS];
    int box[NMS_SLOTS][4];
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < NMS_SLOTS; ++k) {
        const int a = k * NMS_THREADS + tid;
        sc[k] = -INFINITY;
        box[k][0] = box[k][1] = box[k][2] = box[k][3] = 0;
        if (a < A) {
            const float s = scores[(size_t)b * A + a];
            sc[k] = s == s ? s : -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) box[k][e] = anchors[4 * a + e];
            live |= 1u << k;
        }
    }
    int last = 0;
    for (int r = 0; r < topn; ++r) {
        float best = -INFINITY;
        int bi = -1;
#pragma unroll
        for (int k = 0; k < NMS_SLOTS; ++k)                // ascending index and >=: the highest index of equal scores
            if (((live >> k) & 1u) && sc[k] >= best) { best = sc[k]; bi = k * NMS_THREADS + tid; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (nms_better(ob, oi, best, bi)) { best = ob; bi = oi; }
        }
        const int buf = r & 1;                             // two buffers: one barrier per round is enough
        if (lane == 0) { sd[buf][wave] = best; si[buf][wave] = bi; }
        __syncthreads();
        best = sd[buf][0];
        bi = si[buf][0];
#pragma unroll
        for (int w = 1; w < NMS_WAVES; ++w)
            if (nms_better(sd[buf][w], si[buf][w], best, bi)) { best = sd[buf][w]; bi = si[buf][w]; }
        const bool found = bi >= 0;                        // workgroup-uniform
        const int win = found ? bi : last;
        last = win;
        int wb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) wb[e] = anchors[4 * win + e];
        if (tid == 0) {
            index[(size_t)b * topn + r] = win;
#pragma unroll
            for (int e = 0; e < 4; ++e) boxes[((size_t)b * topn + r) * 4 + e] = wb[e];
        }
        if (!found) continue;
        const double wa = ((double)wb[2] - (double)wb[0]) * ((double)wb[3] - (double)wb[1]);
#pragma unroll
        for (int k = 0; k < NMS_SLOTS; ++k) {
            if (!((live >> k) & 1u)) continue;
            const double l0 = (double)min(box[k][2], wb[2]) - (double)max(box[k][0], wb[0]);
            const double l1 = (double)min(box[k][3], wb[3]) - (double)max(box[k][1], wb[1]);
            const double inter = (l0 < 0 || l1 < 0) ? 0.0 : l0 * l1;
            const double area = ((double)box[k][2] - (double)box[k][0]) * ((double)box[k][3] - (double)box[k][1]);
            const double iou = inter / (area + wa - inter);
            if (!(iou < thresh) || k * NMS_THREADS + tid == win) live &= ~(1u << k);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- crops
constexpr int CROP_THREADS = 256;

// source position of output index `o` on an axis of `len` source and `out` output pixels (align_corners): the two
// source pixels i0 <= i1 < len and the weight of i1
__device__ __forceinline__ void crop_axis(int o, int len, float step, int& i0, int& i1, float& w1) {
    const float f = step * (float)o;
    i0 = min((int)f, len - 1);
    i1 = i0 + (i0 < len - 1 ? 1 : 0);
    w1 = f - (float)i0;
}

template <int VEC>
__global__ __launch_bounds__(CROP_THREADS) void nts_crop_kernel(const float* __restrict__ images, const int32_t* __restrict__ boxes,
                                                                float* __restrict__ out, int N, int C, int H, int W, int pad, int oh,
                                                                int ow) {
    const int n = blockIdx.y;                              // b N + j
    const int qw = (ow + VEC - 1) / VEC;
    const long long q = (long long)blockIdx.x * CROP_THREADS + threadIdx.x;
    if (q >= (long long)qw * oh) return;
    const int oy = (int)(q / qw), ox = (int)(q % qw) * VEC;
    const int32_t* bx = boxes + (size_t)n * 4;
    const int y0 = max(bx[0], -pad), x0 = max(bx[1], -pad);                 // the slice of the padded image clips the box
    const int y1 = min(bx[2], H + pad), x1 = min(bx[3], W + pad);
    const int ly = y1 - y0, lx = x1 - x0;
    const size_t plane = (size_t)oh * ow;
    float* o = out + (size_t)n * C * plane + (size_t)oy * ow + ox;
    const bool empty = ly <= 0 || lx <= 0;
    int ya = 0, yb = 0, xa[VEC], xb[VEC];
    float wy = 0.f, wx[VEC];
    bool ya_in = false, yb_in = false, xa_in[VEC], xb_in[VEC];
    if (!empty) {
        int i0, i1;
        crop_axis(oy, ly, oh > 1 ? (float)(ly - 1) / (float)(oh - 1) : 0.f, i0, i1, wy);
        ya = y0 + i0;
        yb = y0 + i1;
        ya_in = ya >= 0 && ya < H;
        yb_in = yb >= 0 && yb < H;
        const float sx = ow > 1 ? (float)(lx - 1) / (float)(ow - 1) : 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            crop_axis(min(ox + e, ow - 1), lx, sx, i0, i1, wx[e]);
            xa[e] = x0 + i0;
            xb[e] = x0 + i1;
            xa_in[e] = xa[e] >= 0 && xa[e] < W;
            xb_in[e] = xb[e] >= 0 && xb[e] < W;
        }
    }
    const float* img = images + (size_t)(n / N) * C * H * W;
    for (int c = 0; c < C; ++c, img += (size_t)H * W, o += plane) {
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            v[e] = 0.f;
            if (empty) continue;
            const float* ra = img + (size_t)(ya_in ? ya : 0) * W;          // a row outside the image is never addressed
            const float* rb = img + (size_t)(yb_in ? yb : 0) * W;
            const float p00 = ya_in && xa_in[e] ? ra[xa[e]] : 0.f, p01 = ya_in && xb_in[e] ? ra[xb[e]] : 0.f;
            const float p10 = yb_in && xa_in[e] ? rb[xa[e]] : 0.f, p11 = yb_in && xb_in[e] ? rb[xb[e]] : 0.f;
            const float w0 = 1.f - wx[e];
            v[e] = (1.f - wy) * (w0 * p00 + wx[e] * p01) + wy * (w0 * p10 + wx[e] * p11);
        }
        if (VEC == 4) {
            f32x4 t;
            t[0] = v[0]; t[1] = v[VEC > 1 ? 1 : 0]; t[2] = v[VEC > 2 ? 2 : 0]; t[3] = v[VEC > 3 ? 3 : 0];
            *reinterpret_cast<f32x4*>(o) = t;
        } else {
            o[0] = v[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- loss
constexpr int NTS_LOSS_THREADS = 1024;
constexpr int NTS_LOSS_WAVES = NTS_LOSS_THREADS / WAVE;
constexpr long long NTS_MAX_ROWS = 1 << 22;            // B (N + 2): one workgroup walks the rows; far above any batch

__global__ __launch_bounds__(NTS_LOSS_THREADS) void nts_loss_kernel(const float* __restrict__ raw, const float* __restrict__ concat,
                                                                    const float* __restrict__ part, const float* __restrict__ prob,
                                                                    const int32_t* __restrict__ labels, float smoothing,
                                                                    float* __restrict__ loss, float* __restrict__ draw,
                                                                    float* __restrict__ dconcat, float* __restrict__ dpart,
                                                                    float* __restrict__ dprob, float* ce_rows, float* part_loss,
                                                                    float* rank_rows, int B, int N, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = B * N, R = 2 * B + P;
    for (int r = wave; r < R; r += NTS_LOSS_WAVES) {       // wave-uniform
        const float* row;
        float* out;
        int b;
        float w;
        if (r < 2 * B) {
            b = r < B ? r : r - B;
            row = (r < B ? raw : concat) + (size_t)b * C;
            out = (r < B ? draw : dconcat) + (size_t)b * C;
            w = 1.f / (float)B;
        } else {
            b = (r - 2 * B) / N;
            row = part + (size_t)(r - 2 * B) * C;
            out = dpart + (size_t)(r - 2 * B) * C;
            w = 1.f / (float)P;
        }
        const int y = labels[b];
        const CeRow s = ce_row_stats(row, C, y, smoothing);
        ce_row_grad(row, out, C, y, smoothing, s, w, 0.f);
        if (lane == 0) {
            ce_rows[r] = s.ce;
            if (r >= 2 * B) part_loss[r - 2 * B] = (y >= 0 && y < C) ? s.ls - (row[y] - s.mx) : NAN;     // no smoothing
        }
    }
    __syncthreads();
    // rank = (1 / B) sum_b sum_i sum_j relu(1 - s_bi + s_bj) [part_loss_bj > part_loss_bi]; thread (b, k) adds the terms
    // whose pivot i is k (j ascending) and counts how s_bk enters: -1 per active term as the pivot, +1 per active term as j
    for (int t = threadIdx.x; t < P; t += NTS_LOSS_THREADS) {
        const int base = (t / N) * N;
        const float pk = part_loss[t], sk = prob[t];
        float acc = 0.f;
        int cnt = 0;
        for (int j = 0; j < N; ++j) {
            const float pj = part_loss[base + j], sj = prob[base + j];
            if (pj > pk) {
                const float h = (1.f - sk) + sj;
                if (!(h <= 0.f)) { acc += h; --cnt; }      // a NaN hinge stays a NaN, as relu keeps it
            }
            if (pk > pj && !((1.f - sj) + sk <= 0.f)) ++cnt;
        }
        rank_rows[t] = acc;
        dprob[t] = (float)cnt / (float)B;
    }
    __syncthreads();
    if (wave == 0) {
        const float a = wave_total(ce_rows, B), c = wave_total(ce_rows + B, B);
        const float p = wave_total(ce_rows + 2 * B, P), k = wave_total(rank_rows, P);
        if (lane == 0) {
            const float l_raw = a / (float)B, l_cat = c / (float)B, l_part = p / (float)P, l_rank = k / (float)B;
            loss[0] = ((l_raw + l_rank) + l_cat) + l_part;                 // the reference's order of addition
            loss[1] = l_raw;
            loss[2] = l_cat;
            loss[3] = l_part;
            loss[4] = l_rank;
        }
    }
}

}  // namespace hk

using namespace hk;

extern "C" int hk_nts_nms(const float* scores, const int32_t* anchors, int32_t* index, int32_t* boxes, int B, int A, int topn,
                          double iou_thresh, hk_stream_t stream) {
    if (!scores || !anchors || !index || !boxes || B <= 0 || A <= 0 || topn <= 0 || !(iou_thresh == iou_thresh)) return HK_ERR_BAD_ARG;
    if (A > NMS_MAX_A) return HK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nts_nms_kernel, dim3(B), dim3(NMS_THREADS), 0, (hipStream_t)stream, scores, anchors, index, boxes, A, topn,
                       iou_thresh);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" int hk_nts_crop_resize(const float* images, const int32_t* boxes, float* out, int B, int N, int C, int H, int W, int pad,
                                  int out_h, int out_w, hk_stream_t stream) {
    if (!images || !boxes || !out || B <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || pad < 0 || out_h <= 0 || out_w <= 0)
        return HK_ERR_BAD_ARG;
    if ((long long)B * N > 65535 || (long long)H + pad > 0x3fffffff || (long long)W + pad > 0x3fffffff) return HK_ERR_UNSUPPORTED;
    const bool vec = (out_w & 3) == 0 && aligned16(out);
    const long long quads = (long long)(vec ? out_w / 4 : out_w) * out_h;
    const long long blocks = (quads + CROP_THREADS - 1) / CROP_THREADS;
    if (blocks > 0x7fffffff) return HK_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, (unsigned)(B * N)), block(CROP_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((nts_crop_kernel<4>), grid, block, 0, st, images, boxes, out, N, C, H, W, pad, out_h, out_w);
    else hipLaunchKernelGGL((nts_crop_kernel<1>), grid, block, 0, st, images, boxes, out, N, C, H, W, pad, out_h, out_w);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

extern "C" size_t hk_nts_loss_ws_bytes(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0 || (long long)B * (N + 2) > NTS_MAX_ROWS) return 0;
    return ((size_t)B * (N + 2) + (size_t)2 * B * N) * sizeof(float) + 256;
}

extern "C" int hk_nts_loss(const float* raw_logits, const float* concat_logits, const float* part_logits, const float* top_n_prob,
                           const int32_t* labels, float smoothing, float* loss, float* draw, float* dconcat, float* dpart, float* dprob,
                           int B, int N, int C, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!raw_logits || !concat_logits || !part_logits || !top_n_prob || !labels || !loss || !draw || !dconcat || !dpart || !dprob ||
        B <= 0 || N <= 0 || C <= 0)
        return HK_ERR_BAD_ARG;
    if (!(smoothing >= 0.f && smoothing <= 1.f)) return HK_ERR_BAD_ARG;
    if ((long long)B * (N + 2) > NTS_MAX_ROWS) return HK_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < hk_nts_loss_ws_bytes(B, N, C)) return HK_ERR_WORKSPACE;
    float* ce_rows = (float*)ws;
    float* part_loss = ce_rows + (size_t)B * (N + 2);
    float* rank_rows = part_loss + (size_t)B * N;
    hipLaunchKernelGGL(nts_loss_kernel, dim3(1), dim3(NTS_LOSS_THREADS), 0, (hipStream_t)stream, raw_logits, concat_logits, part_logits,
                       top_n_prob, labels, smoothing, loss, draw, dconcat, dpart, dprob, ce_rows, part_loss, rank_rows, B, N, C);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
