// CPU-emulation counterpart of hawkeye_amd/csrc/hk_mfma_bf16.h (TEST INFRASTRUCTURE: tests/emu/build_emu.py puts this directory ahead
// of the kernel sources on the include path, so `#include <hk_mfma_bf16.h>` finds this file; the product build never sees it).
// v_mfma_f32_16x16x32_bf16 (gfx950): lane l supplies eight consecutive k of row / column l % 16, k = 8 (l / 16) + 0..7; the lane's
// four results are rows 4 (l / 16) + 0..3 of column l % 16, as the other 16x16 forms.  (The A/B layout is this model's assumption, as
// for mfma_f32_32x32x16_bf16 in hip/hip_runtime.h, until confirmed on the device.)  Piece products are exact in fp32; they are
// accumulated as an fp32 fma chain in k order.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "hk_split_bf16.h"

namespace hk {

inline f32x4 mfma_f32_16x16x32_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
    using namespace hipemu;
    Wave& w = B->waves[cur->wave];
    const unsigned p = cur->parity;
    cur->parity ^= 1u;
    const int l = cur->lane;
    memcpy(&w.slot[p][l][0], &a, 16);
    memcpy(&w.slot[p][l][2], &b, 16);
    wave_barrier();
    const int j = l % 16, g = l / 16;
    for (int v = 0; v < 4; ++v) {
        const int i = 4 * g + v;
        float acc = c[v];
        for (int kb = 0; kb < 4; ++kb) {
            uint16_t ai[8], bj[8];
            memcpy(ai, &w.slot[p][16 * kb + i][0], 16);
            memcpy(bj, &w.slot[p][16 * kb + j][2], 16);
            for (int t = 0; t < 8; ++t) {
                uint32_t ua = (uint32_t)ai[t] << 16, ub = (uint32_t)bj[t] << 16;
                float fa, fb;
                memcpy(&fa, &ua, 4);
                memcpy(&fb, &ub, 4);
                acc = fmaf(fa, fb, acc);
            }
        }
        c[v] = acc;
    }
    return c;
}

}  // namespace hk
