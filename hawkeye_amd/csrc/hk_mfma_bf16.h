// v_mfma_f32_16x16x32_bf16 (gfx950) for the kernels that use it (conv_fwd.hip, MF): lane l supplies the eight consecutive k at
// k = 8 (l / 16) of row (A) or column (B) l % 16; the lane's four results are rows 4 (l / 16) ..+3 of column l % 16.  A header of its
// own so that the CPU emulation of the tests can put its model of the instruction in this file's place (as for hk_isa.h)
#pragma once
#include "hk_split_bf16.h"

namespace hk {

__device__ __forceinline__ f32x4 mfma_f32_16x16x32_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

}  // namespace hk
