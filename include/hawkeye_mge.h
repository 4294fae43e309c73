/*
 * hawkeye_mge.h - the MGE-CNN plugin's entry points (csrc/mge.hip): the part pool behind conv6*, forward and backward, the
 * Grad-CAM box and the criterion; included by hawkeye_hip.h, whose conventions hold (raw device pointers, fp32, dense row-major
 * tensors, a workspace passed in, HK_ERR_* codes, everything enqueued on `stream`, no host synchronisation).  No atomics, every
 * reduction in a fixed order: two runs give the same bits.  Bound from hawkeye_amd/_lib.py: MGE_SIGNATURES.
 */
#ifndef HAWKEYE_MGE_H
#define HAWKEYE_MGE_H

#include "hawkeye_hip.h" /* hk_stream_t, HK_ERR_*; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* replaces pool_max(relu(conv6(x))), conv6 = Conv2d(Cin, Cout, 1, 1, padding = 1), model/methods/MGE_CNN/MGE.py:135,166,197.
 *   x [B,Cin,H,W] ; weight [Cout,Cin] ; bias [Cout] -> pooled [B,Cout] = relu(bias + max(0, max_p sum_c w[o,c] x[b,c,p])) and
 *   argmax [B,Cout] = the pixel p = y W + x that holds the maximum, or -1 where the padded map's border ring (the bias alone) wins.
 *   The border wins a tie with the interior, the lowest pixel wins among interior ties: the scan order of the reference's pool.
 *   The [B,Cout,H+2,W+2] map is never written.  A batched GEMM on the fp32 MFMA with a row-maximum epilogue; one (value, pixel)
 *   pair per 64-column tile goes through the workspace and the tiles are combined in ascending order.  Two launches.
 *   Cin a multiple of 32, anything else about the shape HK_ERR_BAD_ARG; ws: hk_mge_partpool_fwd_ws_bytes (0 for a refused shape),
 *   HK_ERR_WORKSPACE if short.
 * hk_mge_partpool_bwd: g [B,Cout] -> dw [Cout,Cin] = sum_b g[b,o] [pooled > 0] [argmax >= 0] x[b,:,argmax[b,o]] and
 *   db [Cout] = sum_b g[b,o] [pooled > 0], b in ascending order; either may be NULL: not wanted.  No dx (the reference detaches x). */
size_t hk_mge_partpool_fwd_ws_bytes(int B, int Cin, int Cout, int H, int W);
int hk_mge_partpool_fwd(const float* x, const float* weight, const float* bias, float* pooled, int32_t* argmax, int B, int Cin, int Cout,
                        int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_mge_partpool_bwd(const float* x, const float* g, const float* pooled, const int32_t* argmax, float* dw, float* db, int B, int Cin,
                        int Cout, int H, int W, hk_stream_t stream);

/* replaces GradCam.__call__ (grad_cam.py:65-90) and the mask and box search of get_bbox (MGE.py:48-72).
 *   conv5 [B,C,h,w] ; cls_weight [classes,C] ; index int32 [B] on the device ; rate ; S the image side
 *   -> boxes int32 [B,1,4] = y0, x0, y1, x1 with exclusive ends, the layout hk_nts_crop_resize reads.
 *   cam[p] = sum_c relu(W[index,c]) / (h w) conv5[c,p]; the align_corners bilinear value at each of the S x S positions (ATen's fp32
 *   coordinate arithmetic), normalised by the minimum and range of those S x S values (not the CAM's own: an interior cell is
 *   sampled only where S - 1 is a multiple of h - 1); y0 / x0 the first and y1 / x1 the LAST row / column that holds a
 *   value >= rate - the reference's slice drops that last one.  0, 0, S, S where y0 == y1 or x0 == x1 (the reference's own fall-back),
 *   where the CAM is constant or its range not finite, and where index is out of range (the reference raises there).  One launch.
 *   h w <= 512 and S <= 2048, else HK_ERR_UNSUPPORTED. */
int hk_mge_cam_bbox(const float* conv5, const float* cls_weight, const int32_t* index, int32_t* boxes, int B, int C, int h, int w,
                    int classes, float rate, int S, hk_stream_t stream);

/* replaces the K criterion calls and their mean of MGE_CNNTrainer.batch_training, Examples/MGE_CNN.py:43-45.
 *   logits, d_logits: HOST arrays of K device pointers, each [B,C] ; labels int32 [B]
 *   -> loss [1 + K] = {mean of the K label-smoothed cross entropies, the K terms}, d_logits[k] = the gradient of that mean.
 *   A label out of range: NaN, nothing read out of bounds.  1 <= K <= 16, else HK_ERR_BAD_ARG.  One launch.  ws: hk_mge_loss_ws_bytes. */
size_t hk_mge_loss_ws_bytes(int K, int B);
int hk_mge_loss(const float* const* logits, const int32_t* labels, float smoothing, float* loss, float* const* d_logits, int K, int B, int C,
                void* ws, size_t ws_bytes, hk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_MGE_H */
