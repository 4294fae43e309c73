/*
 * hawkeye_conv_tile.h - how the kernels of hawkeye_conv.h and hawkeye_conv_epi.h tile a map (csrc/conv_fwd.hip: conv3x3_plan, knob
 * "conv_tile"); included by hawkeye_hip.h, whose conventions hold.  Bound from hawkeye_amd/_lib.py: TRUNK_TILE_SIGNATURES.
 */
#ifndef HAWKEYE_CONV_TILE_H
#define HAWKEYE_CONV_TILE_H

#include "hawkeye_hip.h" /* HK_ERR_*; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* The tiling of an H x W map on MFMA shape mf (0 = v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_16x16x32_bf16) under the knob "conv_tile" as it
 * stands: out[0] = tiles per image, out[1] = regions (1 or 2), then per region five ints (zeros for an absent second one): tile rows,
 * tile columns, row blocks, strips, first column.  A workgroup owns one tile of 128 pixels; a launch has N out[0] of them per 64 output
 * channels.  A host-side query: nothing is launched, `out` is 12 ints on the host.  HK_ERR_BAD_ARG for a null `out`, sizes < 1 or
 * another mf. */
int hk_conv3x3_tile_plan(int N, int H, int W, int mf, int* out);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_CONV_TILE_H */
