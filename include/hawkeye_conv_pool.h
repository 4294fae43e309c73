/*
 * hawkeye_conv_pool.h - the weight gradient of a 3 x 3 convolution whose output goes through bias, ReLU and a 2 x 2 max-pool, computed
 * from the POOLED gradient (csrc/conv_wrw.hip, "Pooled"; knob "wrw_pool"); included by hawkeye_hip.h, whose conventions hold.  Bound
 * from hawkeye_amd/_lib.py: TRUNK_POOL_SIGNATURES.
 */
#ifndef HAWKEYE_CONV_POOL_H
#define HAWKEYE_CONV_POOL_H

#include <stddef.h>
#include <stdint.h>

#include "hawkeye_hip.h" /* HK_ERR_*, hk_stream_t; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* dW of hk_conv3x3_wrw(g, x) for the full-resolution gradient g that hk_bias_relu_pool_bwd makes of (dp, p, argmax) - g[window
 * position named by the code] = !(p <= 0) ? dp : 0, zero elsewhere - without reading g: three of its four elements are zeros by
 * construction, and along a row every aligned group of four pixels holds at most two values, which is the 2:4 pattern of
 * v_smfmac_f32_16x16x64_bf16; the kernel issues half the matrix instructions of the dense one.
 *   dp, p   [N][H/2][W/2][Cout]     pooled gradient and pooled output        x   [N][H][W][Cin]
 *   argmax  [N][H/2][W/2][Cout/4]   hk_bias_relu_pool_fwd's codes            dw  [Cout][3][3][Cin]
 * H, W: the full-resolution sizes, both even.  Workspace hk_conv3x3_wrw_ws_bytes(Cin, Cout); per-workgroup partial results added in
 * a fixed order, no atomics: the same input gives the same bits.  Within 1e-6 S of float64, as hk_conv3x3_wrw's split form.
 * HK_ERR_BAD_ARG for a null pointer or a size < 1, HK_ERR_WORKSPACE, HK_ERR_UNSUPPORTED where hk_conv3x3_wrw's wide split form
 * refuses (Cin or Cout no multiple of 64, a pointer not 16-byte aligned, the knob "wrw_split" or "wrw_wide" at 0), for odd H or W,
 * and for a row of x (W Cin floats) or a window row of dp (W/2 Cout floats) of 2^31 bytes or more. */
int hk_conv3x3_wrw_pooled(const float* dp, const float* p, const uint8_t* argmax, const float* x, float* dw, int N, int H, int W, int Cin,
                          int Cout, void* ws, size_t ws_bytes, hk_stream_t stream);

/* 1 where a caller should take hk_conv3x3_wrw_pooled for this layer under the knob "wrw_pool" as it stands (0 = never, 1 = wherever the
 * entry point serves the shape, -1 = the library's measured rule), else 0.  A host-side query. */
int hk_conv3x3_wrw_pooled_served(int N, int H, int W, int Cin, int Cout);

/* (Not part of the product's path: it is exported so that a test without a GPU can see the even-row-block plan, as
 * hk_conv3x3_tile_plan shows the tiling.)  How that call splits into jobs under the knob "wrw_wgs" as it stands: out[0] = strips of 32 columns, out[1] = row blocks per image,
 * out[2] = rows per block (even: a step is one window row), out[3] = jobs, out[4] = workgroups per (Cout, Cin) slice.  A host-side
 * query: nothing is launched, `out` is 5 ints on the host.  HK_ERR_BAD_ARG for a null `out`, HK_ERR_UNSUPPORTED for an unserved shape. */
int hk_conv3x3_wrw_pooled_plan(int N, int H, int W, int Cin, int Cout, int* out);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_CONV_POOL_H */
