// The three-way bf16 split of an fp32 value that the trunk's split-bf16 MFMA kernels share (conv_wrw.hip: weight gradient,
// conv_fwd.hip: forward and input gradient): a = hi + mid + lo, each piece a bf16, and the products of first and second order
// (hi hi, hi mid, mid hi, hi lo, lo hi, mid mid) on v_mfma_f32_32x32x16_bf16 keep fp32 accuracy (conv_wrw.hip header: "Split form").
#pragma once
#include "hk_common.h"

namespace hk {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// four bf16 as floats: the packed pairs' own bits (one shift or mask each; a vector conversion here is compiled to a second round of
// single conversions of the source)
__device__ __forceinline__ f32x4 wrs_widen(bf16x4 p) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x2 u = __builtin_bit_cast(u32x2, p);
    const u32x4 w = {u[0] << 16, u[0] & 0xffff0000u, u[1] << 16, u[1] & 0xffff0000u};
    return __builtin_bit_cast(f32x4, w);
}
// a = hi + mid + lo to 2^-27 |a|: round to nearest each time, the two differences are exact in fp32.  0 -> three zeros
__device__ __forceinline__ void wrs_split(f32x4 v, bf16x4 (&p)[3]) {
    p[0] = __builtin_convertvector(v, bf16x4);
    v -= wrs_widen(p[0]);
    p[1] = __builtin_convertvector(v, bf16x4);
    v -= wrs_widen(p[1]);
    p[2] = __builtin_convertvector(v, bf16x4);
}

}  // namespace hk
