/*
 * hawkeye_conv.h - forward and input gradient of the trunk's 3 x 3 convolutions (csrc/conv_fwd.hip); included by hawkeye_hip.h,
 * whose conventions hold: fp32, device pointers, HK_OK or a negative HK_ERR_* or a positive hipError_t, no allocation and no
 * synchronisation inside (capturable), the same bits from run to run.  Bound from hawkeye_amd/_lib.py: TRUNK_SIGNATURES.
 */
#ifndef HAWKEYE_CONV_H
#define HAWKEYE_CONV_H

#include "hawkeye_hip.h" /* hk_stream_t, HK_ERR_*; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* y = conv2d(x, w, stride 1, padding 1, zeros outside the image), and its input gradient dx = conv2d(dy, w') with
 * w'[ci][kh][kw][co] = w[co][2 - kh][2 - kw][ci], on the bf16 matrix pipe with every fp32 value split into three bf16 pieces and
 * the six products of first and second order (fp32 accuracy: |y - exact| <= 1.5e-6 sum |x| |w|).
 *   x, dx  [N][H][W][Cin]    NHWC (the memory of a channels_last [N, Cin, H, W] map)
 *   y, dy  [N][H][W][Cout]
 *   w      [Cout][3][3][Cin] the memory of a channels_last Conv2d.weight - the SAME array for both calls
 *   ws     hk_conv3x3_ws_bytes(Cin, Cout) bytes: the split weights, rewritten by every call (nothing is kept between calls)
 * Cin and Cout multiples of 64, any N, H, W >= 1; every pointer 16-byte aligned.  The output is stored, never accumulated: no
 * zero-fill is needed, and nothing outside the three tensors and the workspace is read or written.
 * HK_ERR_BAD_ARG for a null pointer or a size < 1, then HK_ERR_WORKSPACE for a missing or short workspace, then
 * HK_ERR_UNSUPPORTED for other channel counts, a misaligned pointer, sizes the kernel's indices cannot address, or the knob
 * "conv_fwd" (hk_conv3x3_bwd_data: "conv_bwd_data") at 0.
 * The forms of these two calls that also do the trunk's bias / ReLU / pool / mask passes on the accumulators are declared with those
 * passes, in hawkeye_conv_epi.h (hk_conv3x3_bias_relu_fwd, hk_conv3x3_bias_relu_pool_fwd, hk_conv3x3_masked_bwd_data). */
size_t hk_conv3x3_ws_bytes(int Cin, int Cout);
int hk_conv3x3_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                   hk_stream_t stream);
int hk_conv3x3_bwd_data(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                        hk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_CONV_H */
