// v_smfmac_f32_16x16x64_bf16 (gfx950), the 2:4 sparse bf16 MFMA, for the kernel that uses it (conv_wrw.hip, the pooled layers' weight
// gradient): C[16][16] += A[16][64] B[64][16] where every aligned group of four k of a row of A holds at most two non-zeros, and A is
// passed without the zeros.  Layout as measured on the device (profiles/wrw_pool_probe.json), l = lane, g = l / 16:
//   A    row l % 16, k = 16 g .. 16 g + 15: the lane's eight values are the two kept ones of each of its four groups, in k order
//   idx  the low 16 bits: eight 2-bit positions, value j's at bits 2 j .. 2 j + 1 - value j sits at k = 16 g + 4 (j / 2) + position
//        (ABID 0; ABID 1 would take the high 16 bits)
//   B    column l % 16, sixteen values: elements 0 .. 7 are k = 8 g .. 8 g + 7, elements 8 .. 15 are k = 32 + 8 g .. 32 + 8 g + 7 - two
//        v_mfma_f32_16x16x32_bf16 B operands one after the other, NOT sixteen consecutive k
//   C    as the dense 16 x 16 forms: the lane's four results are rows 4 g ..+3 of column l % 16
// It issues at the rate of v_mfma_f32_16x16x32_bf16 (0.95 x its time per instruction), for twice the k.  A header of its own so that
// the CPU emulation of the tests can put its model of the instruction in this file's place (as for hk_mfma_bf16.h)
#pragma once
#include "hk_split_bf16.h"

namespace hk {

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

// the dense k of element e (0 .. 15) of the B operand of a lane of group g, and of the first k of the group of four that holds value
// j (0 .. 7) of the A operand
__host__ __device__ constexpr int smfmac_b_k(int g, int e) { return 32 * (e >> 3) + 8 * g + (e & 7); }
__host__ __device__ constexpr int smfmac_a_k4(int g, int j) { return 16 * g + 4 * (j >> 1); }

__device__ __forceinline__ f32x4 smfmac_f32_16x16x64_bf16(bf16x8 a, bf16x16 b, f32x4 c, int idx) {
    return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, c, idx, 0, 0);
}

}  // namespace hk
