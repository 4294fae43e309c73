/* C ABI of the DCL plugin's kernels (hawkeye_amd/csrc/dcl.hip), part of libhawkeye_hip.so: six entry points next to the 98
 * of hawkeye_hip.h, which includes this header at its end.  Conventions as there: raw device pointers, an hk_stream_t, an
 * int status (0, HK_ERR_*, or a hipError_t). */
#ifndef HAWKEYE_DCL_H
#define HAWKEYE_DCL_H
#include "hawkeye_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ DCL head, loss and swap law ----
 * replaces model/methods/DCL.py:33-39 (Convmask, AvgPool2d(2), tanh and AdaptiveAvgPool2d(1) as two reads of the last map,
 * two full-size map gradients and an add), model/loss/DCL_loss.py:17-20 (two label-smoothed cross entropies, an L1 term
 * and their sum) and dataset/dataset_DCL.py:48-62 (98 ImageStat means and a 49 x 49 search per image, in Python).  Every
 * entry point: no host synchronisation, no allocation (capturable in a hipGraph), no atomics, fixed summation orders - the
 * same bits on every run, whatever the alignment.  HK_ERR_BAD_ARG: a null pointer that is not optional, a size <= 0;
 * HK_ERR_WORKSPACE: a short workspace (reported before an unsupported size); HK_ERR_UNSUPPORTED: H < 2 or W < 2 (head),
 * W < gx or H < gy, more than 2048 patches or more than 2^24 pixels per image (law), sizes past the index range.
 *   hk_dcl_head_fwd: x [B,C,H,W] dense NCHW ; w [C] (Convmask.weight) ; bias [1] on the DEVICE -> pooled [B,C] = the mean
 *     over H W ; mask [B,(H/2)(W/2)] = tanh(avgpool2x2(sum_c w[c] x[b,c] + bias)), floor semantics: the last row / column
 *     of an odd side enters pooled only.  x is read once; two launches.  16-byte accesses where H W % 4 == 0 and x is
 *     16-byte aligned.  ws: hk_dcl_head_fwd_ws_bytes(B, C, H, W) (0 for sizes the call refuses).
 *   hk_dcl_head_bwd: the saved mask, d_pooled [B,C] and d_mask [B,M] (each may be NULL, meaning zero) -> dx [B,C,H,W] =
 *     d_pooled / HW + w[c] g[b,h/2,w/2] / 4 with g = d_mask (1 - mask^2) (the second term only inside the pooled area) ;
 *     dw [C] = sum_b sum_hw x g / 4 ; dbias [1] = sum g.  Each output may be NULL; each one given is written in full.  x
 *     is read once (only when dw is wanted), dx written once; at most two launches.  ws: hk_dcl_head_bwd_ws_bytes.
 *   hk_dcl_loss: logits [N,K], swap_logits [N,S], mask [N,M] ; labels, labels_swap int64 [N] ; law [N,M] -> loss [4] =
 *     total, ce, swap, law with ce / swap the label-smoothed (`smoothing`) cross entropies (mean over N), law =
 *     mean |mask - law| and total = alpha ce + beta swap + gamma law ; d_logits, d_swap, d_mask = weight x d total (d_mask
 *     is exactly 0 where mask == law).  A label outside its range reads nothing and makes that term and total NaN.  One
 *     launch, no workspace.
 *   hk_dcl_swap_law: unswapped, swapped uint8 [N,H,W,3] ; bounds_x int32 [gx + 1], bounds_y int32 [gy + 1] (device; patch
 *     (i, j) spans columns [bounds_x[i], bounds_x[i+1]) and rows [bounds_y[j], bounds_y[j+1]), entries clamped to the image)
 *     -> index int32 [N, gx gy]: for each swapped patch (row-major) the unswapped patch whose value ((0 + s_r / n) + s_g / n)
 *     + s_b / n (exact integer band totals, float64 divisions and additions, as Python's sum() of ImageStat's means) is
 *     nearest, the lowest index on ties ; law float [N, gx gy] = (index - (gx gy) / 2) / (gx gy), divided in float64. */
size_t hk_dcl_head_fwd_ws_bytes(int B, int C, int H, int W);
int hk_dcl_head_fwd(const float* x, const float* w, const float* bias, float* pooled, float* mask, int B, int C, int H, int W,
                    void* ws, size_t ws_bytes, hk_stream_t stream);
size_t hk_dcl_head_bwd_ws_bytes(int B, int C, int H, int W);
int hk_dcl_head_bwd(const float* x, const float* w, const float* mask, const float* d_pooled, const float* d_mask, float* dx,
                    float* dw, float* dbias, int B, int C, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_dcl_loss(const float* logits, const float* swap_logits, const float* mask, const int64_t* labels,
                const int64_t* labels_swap, const float* law, float alpha, float beta, float gamma, float smoothing, float weight,
                float* loss, float* d_logits, float* d_swap, float* d_mask, int N, int K, int S, int M, hk_stream_t stream);
int hk_dcl_swap_law(const uint8_t* unswapped, const uint8_t* swapped, const int32_t* bounds_x, const int32_t* bounds_y,
                    int32_t* index, float* law, int N, int H, int W, int gx, int gy, hk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HAWKEYE_DCL_H */
