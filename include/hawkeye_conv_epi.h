/*
 * hawkeye_conv_epi.h - the trunk's 3 x 3 forward and input gradient (hawkeye_conv.h) with the epilogue passes of the trunk
 * (hawkeye_hip.h, "VGG trunk epilogues") done on the accumulators, before anything is written (csrc/conv_fwd.hip, EPI); included by
 * hawkeye_hip.h, whose conventions hold.  Bound from hawkeye_amd/_lib.py: TRUNK_EPI_SIGNATURES.
 */
#ifndef HAWKEYE_CONV_EPI_H
#define HAWKEYE_CONV_EPI_H

#include "hawkeye_hip.h" /* hk_stream_t, HK_ERR_*; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* The forward and the input gradient of hawkeye_conv.h (same maps, same weight array, same checks, same split-bf16 kernel) with the
 * trunk's epilogue passes done on the accumulators, before anything is written (csrc/conv_fwd.hip, EPI):
 *   hk_conv3x3_bias_relu_fwd       y [N][H][W][Cout] = max(conv(x, w) + bias, 0) and `mask` (nullable, 8-byte aligned): the bits of the plain
 *                                  forward followed by hk_bias_relu_fwd, map and mask
 *   hk_conv3x3_bias_relu_pool_fwd  p [N][H/2][W/2][Cout], argmax [N][H/2][W/2][Cout/4] (8-byte aligned): the bits of the plain forward
 *                                  followed by hk_bias_relu_pool_fwd; H and W even; the full-resolution map is never written
 *   hk_conv3x3_masked_bwd_data     dx [N][H][W][Cin] = the plain input gradient where the bit of `mask` ([N][H][W][Cin/4], 16-byte aligned:
 *                                  the sign mask of the map x, written by the layer that produced it) is set, else 0 - the bits of the
 *                                  plain input gradient followed by hk_bias_relu_bwd - and dbias [Cin] = the column sums of dx, i.e. the
 *                                  PRODUCING layer's bias gradient: one partial row per 128-pixel tile (hawkeye_conv_tile.h), added in a fixed order in two
 *                                  stages (no atomics, the same bits every run; another order than hk_bias_relu_bwd's, so dbias agrees
 *                                  with it to rounding only).  Workspace hk_conv3x3_masked_ws_bytes(N, H, W, Cin, Cout): the split
 *                                  weights and the partial rows
 * Errors as in hawkeye_conv.h; HK_ERR_UNSUPPORTED also with the knob "conv_epi" below 1 (the two forwards) or 2 (the input gradient). */
int hk_conv3x3_bias_relu_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int N, int H, int W, int Cin,
                             int Cout, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_conv3x3_bias_relu_pool_fwd(const float* x, const float* w, const float* bias, float* p, uint8_t* argmax, int N, int H, int W, int Cin,
                                  int Cout, void* ws, size_t ws_bytes, hk_stream_t stream);
size_t hk_conv3x3_masked_ws_bytes(int N, int H, int W, int Cin, int Cout);
int hk_conv3x3_masked_bwd_data(const float* dy, const float* w, const uint8_t* mask, float* dx, float* dbias, int N, int H, int W, int Cin,
                               int Cout, void* ws, size_t ws_bytes, hk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_CONV_EPI_H */
