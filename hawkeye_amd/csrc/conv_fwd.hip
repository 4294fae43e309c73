// Forward and input gradient of the trunk's 3 x 3 convolutions whose channel counts are multiples of 64 (model/backbone/vgg.py:24-57;
// stride 1, padding 1, fp32, channels_last), on the bf16 matrix pipe with the three-way split of conv_wrw.hip ("Split form" there):
//   y[n][h][w][co] = sum over kh, kw, ci of x[n][h + kh - 1][w + kw - 1][ci] Wt[co][kh][kw][ci]
// - a GEMM with M = Cout, N = pixels, K = 9 Cin.  The library runs it on the fp32 matrix pipe at 131 - 136 TF/s of a practical 140
// (DESIGN 3.10); the split form's six bf16 products per fp32 product leave that pipe for one that is 16 x as fast.  The input
// gradient is the same sum over dy with W'[ci][kh][kw][co] = W[co][2 - kh][2 - kw][ci]: ONE main kernel behind ONE pre-pass
// kernel, which runs once per call and reads W' out of W when its `transposed` flag is set.
//
//   pre-pass = conv3x3_wsplit_kernel splits the weights (hk_split_bf16.h) once per call and writes them in the order the main kernel
//              stages them: [Cout tile of 64][Cin chunk of 32][tap][piece hi, mid, lo][64 co][40 bf16] - the 32 channels of a row and
//              8 of padding, the LDS image itself, so that staging is a 16-byte LDS-DMA per lane and piece.  `transposed` reads W'
//              out of W.  Not cached across calls: the weights change every step
//   tile     = a workgroup (four waves) owns 64 output channels x 4 rows x 32 columns of one image; wave r owns row r: two 32 x 32
//              MFMA blocks (co 0 - 31, 32 - 63) x 32 pixels.  The weights are the operand whose index is the accumulator ROW, so a
//              lane ends with 4 consecutive output channels of one pixel per accumulator quad: 16-byte stores, 128 contiguous
//              bytes per pixel and block.  Nothing is accumulated in memory: no atomics, no split-K, no zero-fill, same bits each run
//   tiles    = which 128 pixels a workgroup takes is a third template parameter (G, PLAN, documented at CfGeo and at the kernel; knob
//              `conv_tile`): 4 x 32 as described here, 8 x 16 (two rows a wave; halo tile 10 x 18) or, on CF_MF_16, 16 x 8 (four rows a wave;
//              halo tile 18 x 10 at a pitch of 16 pixels, 79872 B of LDS).  4 x 32 pads a 112-wide map to 128 columns and a 56-wide one
//              to 64 - one MFMA in eight on columns the store throws away; conv3x3_plan takes per map the tiling with the fewest tiles:
//              112 wide 98 tiles an image for 112 (8 x 16), 56 wide 25 for 28 (8 x 16 over three strips + 16 x 8 over the last eight
//              columns, one launch).  Every output element keeps its products, their order and its bits.  Measured at batch 64 (DESIGN
//              3.10, "Tile geometries"): matrix-pipe cycles x 0.875 and x 0.893 as the tile counts say, the clock gives 3 % back, the
//              twelve launches at those widths 0.17 - 0.60 ms faster each, the step 106.3 -> 102.1 ms
//   K        = the channel axis, contiguous in NHWC x and in [co][tap][ci] weights: a fragment (8 consecutive k of one row) is 16
//              contiguous bytes of a [pixel][32 channels] bf16 plane - a plain ds_read_b128.  Planes have a pitch of 80 bytes a
//              pixel (5 l mod 16 is a permutation of the 16-byte slots of a 256-byte bank row: the 16 lanes of a read phase do not meet)
//   x        = per Cin chunk of 32 the halo tile, 6 rows x 34 columns, is split on its way from registers to LDS (once per element
//              and workgroup) and used by all nine taps: a tap is an address offset.  Rows and columns outside the image and past a
//              ragged edge are zeros in LDS; the load itself is made from a clamped, in-bounds address, never skipped
//   pipeline = the weight tile of a (chunk, tap) is double-buffered (2 x 15360 B): tap t + 1 comes in by LDS-DMA (glds16: the
//              workspace is the LDS image, a wave's three or four pieces are 1 KiB each in both; no register, no ds_write) while
//              the MFMAs of tap t run.  A tap reads its 18 fragments, runs its MFMAs and ends with CF_TAP_BARRIER: a counted
//              s_waitcnt vmcnt(n) lgkmcnt(0) and a raw s_barrier - never __syncthreads(), whose fence would drain every request in
//              flight.  The next chunk's x tile is requested at tap 5 behind the weight pieces (vmcnt(7) there: it stays in flight
//              until tap 6's wait) and stored behind tap 8; one barrier per tap (24 MFMAs per wave), two at a chunk's end.
//              Measured against staging through registers + ds_write_b128 ("Weight tiles by LDS-DMA"): the step
//              3.2 ms of 112 faster at batch 64, every output of every instantiation bit-identical.  A third buffer (CF_MF_16:
//              76032 B, the tile two taps ahead, vmcnt(3)) measured 0.1 ms: inside the spread, not kept
//   chains   = the bf16 MFMA does not round its running sum as an fp32 fma does (conv_wrw.hip: "chains"): every CF_FLUSH = 3 chunks
//              (K = 864) the accumulators are added to a second fp32 set with ordinary additions and start again from zero
//              (one chain of 4608 at Cin = 512, measured on a build without the restart: 2.3 - 8.3e-7 S from float64, inside the 1.5e-6
//              bound but 2.5 - 4 x the restarted chains' 0.6 - 3.2e-7 and the library's 0.4 - 3.1e-7: DESIGN 3.10)
//   LDS      = 3 x 16320 + 2 x 15360 = 79680 B (dynamic): two workgroups per CU
//   grid     = xcd_map over (pixel tile, Cout tile): the Cout tiles of a pixel tile run one after the other on one XCD, so the x
//              tile comes out of that L2 for all but the first
//   measured = 175 - 202 TF/s stand-alone at batch 64 where the library's fp32 kernels give 108 - 139; in the training step the twelve
//              forwards 42.1 ms against 57.5 and the twelve input gradients 40.7 against 59.9, and no zero-fill of an output is left;
//              matrix pipe 56 - 64 % busy at 1.9 GHz, LDS bank conflicts 7 % of the LDS-active cycles
//   epilogue = the main kernel is a template (EPI, documented at the kernel): besides the plain store it leaves with bias + ReLU + sign
//              mask, with bias + ReLU + 2 x 2 max-pool + argmax (the full-resolution map is never written), or - the input gradient -
//              with the producing layer's ReLU mask applied and that layer's bias gradient summed (fp64 partial row per tile, then
//              conv3x3_colsum_kernel in two stages).  The same bits as the passes of trunk.hip they replace (the bias gradient: the
//              float next to the exact sum); in the training step those passes were 4.9 ms of 124.5, the four instantiations take
//              what the plain kernel took (80.4 against 80.5 ms), the reductions 0.07 ms
//   MFMA     = a second template parameter (MF, documented at the constants and at the kernel; knob `conv_mfma`): the same tile, chunk,
//              products, chains and pipeline on v_mfma_f32_16x16x32_bf16, whose fragment wants another LDS image (64-byte pitch, the
//              k-group pairs of every other four rows swapped: static_asserted conflict-free for all four ds_read_b128 lane groups at
//              every pixel offset, 63744 B).  Measured at batch 64 ("The MFMA shape"): 196 - 227 TF/s stand-alone where the
//              other shape gives 177 - 205; in the step the 24 launches 70.2 ms against 80.2 with every layer on it; per launch 9 - 11 %
//              fewer cycles (LDS bank conflicts 7 % -> 0, a fifth less weight traffic) at a 3 - 4 % higher clock, the matrix pipe
//              61 - 72 % busy.  Which shape a call runs on is decided here (conv3x3_mfma16_wins: every call on 16 x 16 x 32).  Registers
//              with the weight tiles by DMA and every fragment read in front of the MFMAs: 204 - 206 VGPRs (MF = 0: 190 - 192), no spill
//              (8 x 16: 200 - 202 and 184 - 188; the launch with both 8 x 16 and 16 x 8: 206 - 208)
#include "hk_common.h"
#include "hk_split_bf16.h"
#include <hk_mfma_bf16.h>   // the 16 x 16 x 32 bf16 MFMA (the emulation build finds its model of it first)
#include "../../include/hawkeye_hip.h"

namespace hk {

constexpr int CF_CO = 64;                                // output channels per workgroup
constexpr int CF_R = 4;                                  // output rows per workgroup: one per wave
constexpr int CF_SW = 32;                                // output columns per workgroup
constexpr int CF_CK = 32;                                // input channels per chunk
constexpr int CF_PIX = 80;                               // bytes of a pixel (or of a weight row) in a plane: 32 bf16 + 16 bytes
constexpr int CF_HW = CF_SW + 2;                         // columns of the halo tile
constexpr int CF_HPIX = (CF_R + 2) * CF_HW;              // 204 pixels
constexpr int CF_XPLANE = CF_HPIX * CF_PIX;              // 16320 B: one piece of the halo tile
constexpr int CF_WPLANE = CF_CO * CF_PIX;                // 5120 B: one piece of a (chunk, tap) weight tile
constexpr int CF_WTAP = 3 * CF_WPLANE;                   // 15360 B
constexpr int CF_LDS = 3 * CF_XPLANE + 2 * CF_WTAP;      // 79680 B
constexpr int CF_XF4 = CF_HPIX * (CF_CK / 4);            // 1632 float4 of a halo tile
constexpr int CF_XU = (CF_XF4 + 255) / 256;              // 7 loads per thread (the last one for 96 threads)
constexpr int CF_FLUSH = 3;                              // chunks (K = 864) an accumulator chain runs

// MF, the bf16 MFMA the main kernel runs on: CF_MF_32 = v_mfma_f32_32x32x16_bf16 (two 32 x 32 blocks a wave, two k steps a chunk) on
// the planes above; CF_MF_16 = v_mfma_f32_16x16x32_bf16 (four 16-channel x two 16-pixel blocks a wave, one k step a chunk) on the
// planes below.  Same tile, chunk, products, chains and pipeline; what differs is the fragment - lane l supplies the eight k at
// 8 (l / 16) of row or column l % 16 - and with it the image that ds_read_b128 reads without conflicts, and the accumulators' layout
constexpr int CF_MF_32 = 0, CF_MF_16 = 1;
constexpr int CF16_PIX = 64;                             // bytes of a pixel (or of a weight row) in a CF_MF_16 plane: 32 bf16, no padding
constexpr int CF16_XPLANE = CF_HPIX * CF16_PIX;          // 13056 B
constexpr int CF16_WPLANE = CF_CO * CF16_PIX;            // 4096 B
constexpr int CF16_WTAP = 3 * CF16_WPLANE;               // 12288 B: three 16-byte loads a thread
constexpr int CF16_LDS = 3 * CF16_XPLANE + 2 * CF16_WTAP;  // 63744 B

// G, which 128 pixels a workgroup takes ("Tile geometries"): the constants above are those of 4 rows x 32 columns, whose
// strips pad a 112-wide map to 128 columns and a 56-wide one to 64 - one MFMA in eight on zeros.  8 x 16 (halo tile 10 x 18, fewer
// pixels than 6 x 34) tiles 112 = 7 x 16 exactly; 16 x 8 takes the remainder strip of a 56-wide map (3 x 16 + 8).  Everything else is
// the same: 64 channels x 128 pixels a workgroup, 32 pixels a wave, the same chunks, taps, products and chains for every output
// element - only the lane that holds it differs
//   CF_MF_16: wave w, pixel block pb, lane l15 ->  4 x 32: row w, column 16 pb + l15;  8 x 16: row 2 w + pb, column l15;
//             16 x 8: row 4 w + 2 pb + l15 / 8, column l15 % 8 (halo rows at a pitch of 16 pixels: a tap's row step and the pixel blocks'
//             distance are then constant offsets in the image, and the lane pattern is conflict-free - it is 2-way conflicted at 10 .. 15)
//   CF_MF_32: wave w, lane l31 -> 4 x 32: row w, column l31;  8 x 16: row 2 w + l31 / 16, column l31 % 16 for the first row and
//             (l31 - 2) % 16 for the second: the halo pitch of 18 moves the second row's pixels 2 slots on, the rotation takes
//             them back, so a ds_read_b128 lane group (which mixes lanes of both halves) meets the slots of 4 x 32.  No 16 x 8
constexpr int CF_G_4x32 = 0, CF_G_8x16 = 1, CF_G_16x8 = 2;
template <int G>
struct CfGeo {
    static constexpr int TH = G == CF_G_4x32 ? 4 : (G == CF_G_8x16 ? 8 : 16), TW = 128 / TH;      // output rows and columns of a tile
    static constexpr int HR = TH + 2, HC = TW + 2;           // rows and columns of the halo tile
    static constexpr int HP = G == CF_G_16x8 ? 16 : HC;      // pixels from one halo row to the next in a plane
    static constexpr int LPIX = HR * HP;                     // pixels of a plane: 204, 180, 288
    static constexpr int XF4 = HR * HC * (CF_CK / 4);        // float4 of a halo tile: 1632, 1440, 1440
    static constexpr int XU = (XF4 + 255) / 256;             // loads per thread: 7, 6, 6
    static constexpr int PBD = G == CF_G_4x32 ? 16 : (G == CF_G_8x16 ? HP : 2 * HP);      // CF_MF_16: plane pixels from pixel block 0 to 1
    // a lane's pixel of the tile (CF_MF_16: l = lane % 16 of pixel block pb; CF_MF_32: l = lane % 32, pb = 0)
    __host__ __device__ static constexpr int trow(bool m32, int wave, int pb, int l) {
        return G == CF_G_4x32 ? wave : (G == CF_G_8x16 ? 2 * wave + (m32 ? l >> 4 : pb) : 4 * wave + 2 * pb + (l >> 3));
    }
    __host__ __device__ static constexpr int tcol(bool m32, int pb, int l) {
        return G == CF_G_4x32 ? (m32 ? l : 16 * pb + l) : (G == CF_G_8x16 ? (m32 ? (l < 16 ? l : (l - 2) & 15) : l) : l & 7);
    }
};
static_assert(CfGeo<CF_G_4x32>::LPIX == CF_HPIX && CfGeo<CF_G_4x32>::XU == CF_XU && CfGeo<CF_G_4x32>::HP == CF_HW, "4 x 32 is the tile above");
// PLAN, what a launch tiles a map with: one geometry, or - CF_MF_16 only - 8 x 16 over the whole strips of 16 columns and 16 x 8 over
// the remainder (a workgroup decodes its region from the tile index); the LDS of a launch is that of its largest geometry
constexpr int CF_PLAN_4x32 = 0, CF_PLAN_8x16 = 1, CF_PLAN_MIXED = 2;
template <int MF, int G>
constexpr int cf_xplane() { return CfGeo<G>::LPIX * (MF == CF_MF_32 ? CF_PIX : CF16_PIX); }
template <int MF, int PLAN>
constexpr int cf_lds() {
    return 3 * cf_xplane<MF, PLAN == CF_PLAN_MIXED ? CF_G_16x8 : PLAN>() + 2 * (MF == CF_MF_32 ? CF_WTAP : CF16_WTAP);
}
static_assert(cf_lds<CF_MF_32, CF_PLAN_4x32>() == CF_LDS && cf_lds<CF_MF_16, CF_PLAN_4x32>() == CF16_LDS, "4 x 32 keeps its LDS");
static_assert(cf_lds<CF_MF_32, CF_PLAN_8x16>() <= CF_LDS && cf_lds<CF_MF_16, CF_PLAN_MIXED>() == 79872 && 2 * 79872 <= 160 * 1024,
              "two workgroups per CU with every plan");
// The barrier that ends a tap: s_waitcnt vmcnt(n) lgkmcnt(0) + s_barrier.  HK_VM_BARRIER(n) with the LDS reads waited for as well: the
// DMA that another wave issues behind this barrier goes into the buffer this tap read, so no fragment read may still be on its way
// (the reads are issued in front of the MFMAs: the wait finds them done), and no __syncthreads(), whose fence drains vmcnt(0)
#define CF_TAP_BARRIER(n)                                                                                      \
    do {                                                                                                       \
        asm volatile("" ::: "memory");                 /* no LDS access moves across */                        \
        __builtin_amdgcn_s_waitcnt(HK_VMCNT_IMM(n) & ~(15 << 8));                                              \
        __builtin_amdgcn_s_barrier();                                                                          \
        asm volatile("" ::: "memory");                                                                         \
    } while (0)
// THE image of a CF_MF_16 plane, for the staging stores, the fragment reads and the weight pre-pass: byte offset of k-group kg
// (eight k, 16 bytes) of row `row` (a pixel of the halo tile, or a weight row).  The 80-byte pitch of the other shape puts rows 1
// and 4 of a ds_read_b128 lane group on one slot; no plain pitch separates the groups, and on the 80-byte pitch no XOR of period 16
// on the k-group does at every pixel offset (searched; the x fragment starts at any pixel: a tap is an address offset).  Rows 4 apart share their four
// slots at this pitch; of such rows a lane group reads r (k-group g), r + 4, r + 8 (g ^ 1) and r + 12 (g): swapping the k-group
// pairs of every other four rows gives them four different slots, whatever r is
__host__ __device__ constexpr int cf16_off(int row, int kg) { return row * CF16_PIX + ((kg ^ ((row >> 1) & 2)) << 4); }
// the 16-lane groups of ds_read_b128, one LDS cycle each: a group is conflict-free iff its lanes' 16-byte slots mod 256 B differ
constexpr int CF_B128_GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
// ... with the lane pattern of geometry G: lane l15 reads pixel base + (its row of the pixel block) HP + (its column); the weights'
// pattern - 16 consecutive rows - is that of 4 x 32
template <int G>
constexpr bool cf16_group_conflict_free(int g) {
    constexpr int LAST = CfGeo<G>::trow(false, 0, 0, 15) * CfGeo<G>::HP + CfGeo<G>::tcol(false, 0, 15);
    for (int base = 0; base + LAST < CfGeo<G>::LPIX; ++base) {    // the fragment's first pixel: any pixel of the halo tile (weights: multiples of 16)
        unsigned seen = 0;
        for (int i = 0; i < 16; ++i) {
            const int lane = CF_B128_GROUPS[g][i], l = lane & 15;
            const int pix = base + CfGeo<G>::trow(false, 0, 0, l) * CfGeo<G>::HP + CfGeo<G>::tcol(false, 0, l);
            const int slot = (cf16_off(pix, lane >> 4) >> 4) & 15;
            if ((seen >> slot) & 1u) return false;
            seen |= 1u << slot;
        }
    }
    return true;
}
template <int G>
constexpr bool cf16_conflict_free() {
    return cf16_group_conflict_free<G>(0) && cf16_group_conflict_free<G>(1) && cf16_group_conflict_free<G>(2) && cf16_group_conflict_free<G>(3);
}
static_assert(cf16_conflict_free<CF_G_4x32>() && cf16_conflict_free<CF_G_8x16>() && cf16_conflict_free<CF_G_16x8>(),
              "every ds_read_b128 lane group of a CF_MF_16 fragment reads 16 different slots, in every geometry at its pitch");
// the same for the pixel fragment of CF_MF_32 (80-byte pitch: slot 5 pixel + lane / 32 + 2 ks), whose 32 lanes are two tile rows in 8 x 16
template <int G>
constexpr bool cf32_conflict_free() {
    for (int g = 0; g < 4; ++g)
        for (int base = 0; base + CfGeo<G>::HP + 16 < CfGeo<G>::LPIX; ++base) {
            unsigned seen = 0;
            for (int i = 0; i < 16; ++i) {
                const int lane = CF_B128_GROUPS[g][i], l = lane & 31;
                const int pix = base + CfGeo<G>::trow(true, 0, 0, l) * CfGeo<G>::HP + CfGeo<G>::tcol(true, 0, l);
                const int slot = ((pix * CF_PIX + (lane >> 5) * 16) >> 4) & 15;
                if ((seen >> slot) & 1u) return false;
                seen |= 1u << slot;
            }
        }
    return true;
}
static_assert(cf32_conflict_free<CF_G_4x32>() && cf32_conflict_free<CF_G_8x16>(), "the CF_MF_32 pixel fragment, both geometries");
static_assert(cf16_off(16, 1) == cf16_off(0, 1) + 16 * CF16_PIX && cf16_off(35, 2) == cf16_off(3, 2) + 32 * CF16_PIX,
              "rows 16 and 32 further on are a constant offset away");
static_assert(CF16_WTAP <= CF_WTAP && CF16_WTAP == 3 * 256 * 16, "the workspace holds either image; a weight tile is three loads a thread");

// w [M][9][K] (transposed: w [K][9][M], read as W'[m][tap][k] = w[k][8 - tap][m]) -> ws [M / 64][K / 32][9][3][64][40] bf16.
// One thread per four k of a row, padding included (zeros).  MF = CF_MF_16: ws [M / 64][K / 32][9][3] planes of cf16_off, no padding
template <int MF>
__global__ __launch_bounds__(256) void conv3x3_wsplit_kernel(const float* __restrict__ w, char* __restrict__ ws, int M, int K,
                                                             int transposed, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int nchunk = K / CF_CK;
    constexpr int NQ = MF == CF_MF_32 ? 10 : 8;
    const int q = (int)(i % NQ);
    long long r = i / NQ;
    const int co = (int)(r % CF_CO);
    r /= CF_CO;                                          // r = (cot nchunk + chunk) 9 + tap: the tile
    const int tap = (int)(r % 9);
    const int chunk = (int)((r / 9) % nchunk), cot = (int)((r / 9) / nchunk);
    const long long m = (long long)cot * CF_CO + co, k0 = (long long)chunk * CF_CK + 4 * q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < 8) {
        if (!transposed) {
            v = *reinterpret_cast<const f32x4*>(w + (m * 9 + tap) * K + k0);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = w[((k0 + e) * 9 + (8 - tap)) * M + m];
        }
    }
    bf16x4 p[3];
    wrs_split(v, p);
    if (MF == CF_MF_32) {
        char* d = ws + (size_t)r * CF_WTAP + co * CF_PIX + q * 8;
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<bf16x4*>(d + s * CF_WPLANE) = p[s];
    } else {
        char* d = ws + (size_t)r * CF16_WTAP + cf16_off(co, q >> 1) + (q & 1) * 8;
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<bf16x4*>(d + s * CF16_WPLANE) = p[s];
    }
}

// one operand fragment of v_mfma_f32_32x32x16_bf16: 16 contiguous bytes of a plane in LDS
__device__ __forceinline__ bf16x8 cf_frag(const char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(3))) bf16x8*)p;
#else
    bf16x8 f;
    __builtin_memcpy(&f, p, 16);
    return f;
#endif
}

constexpr int CF_EPI_NONE = 0, CF_EPI_RELU = 1, CF_EPI_POOL = 2, CF_EPI_MASK = 3;
constexpr int CF_PARK = CF_CO + 4;                       // floats of a parked pixel (CF_EPI_POOL): 272 B, 16 lanes' float4 on 64 different banks
constexpr int CF_DB_RPG = 128;                           // partial rows a workgroup of the first reduction stage adds
static_assert(CF_R * CF_SW * CF_PARK * 4 <= CF_LDS, "the parked tile fits the LDS of the main loop");

__device__ __forceinline__ f32x4 cf_relu4(f32x4 v) {                 // relu4 of trunk.hip
    f32x4 r;
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = v[t] < 0.f ? 0.f : v[t];
    return r;
}
__device__ __forceinline__ unsigned cf_sign4(f32x4 r) {             // the mask byte of bias_relu_fwd_kernel<true>
    return (!(r[0] <= 0.f) ? 1u : 0u) | (!(r[1] <= 0.f) ? 2u : 0u) | (!(r[2] <= 0.f) ? 4u : 0u) | (!(r[3] <= 0.f) ? 8u : 0u);
}

// The way out of the CF_MF_16 main loop (the kernel's comment: EPI, MF).  C layout of the 16 x 16 MFMA: column = lane & 15 (pixel
// l15 of the wave's pixel block pb: CfGeo), row = 4 (lane >> 4) + e (channel 16 cb + 4 kg + e): v[cb][pb] is channel quad 4 cb + kg of pixel pb
template <int EPI, int G>
__device__ __forceinline__ void cf16_epilogue(const f32x4 (&acc4)[4][2], const f32x4 (&sum4)[4][2], float* ldsf, float* __restrict__ y, int H,
                                              int W, int Cout, long long n, int r0, int c0, int cot, int tile, int wave, int tid, int l15,
                                              int kg, const float* __restrict__ bias, uint8_t* __restrict__ mk,
                                              double* __restrict__ part) {
    typedef CfGeo<G> GE;
    const int c4 = Cout / 4;
    bool live[2];
    long long pix[2];                                                // (used where live)
    f32x4 v[4][2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
        const int row = r0 + GE::trow(false, wave, pb, l15), col = c0 + GE::tcol(false, pb, l15);
        live[pb] = row < H && col < W;
        pix[pb] = (n * H + row) * W + col;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) v[cb][pb] = sum4[cb][pb] + acc4[cb][pb];
    }
    if (EPI == CF_EPI_RELU || EPI == CF_EPI_POOL) {
        const f32x4* b4 = reinterpret_cast<const f32x4*>(bias + cot * CF_CO + 4 * kg);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const f32x4 b = b4[4 * cb];
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) v[cb][pb] = cf_relu4(v[cb][pb] + b);
        }
    }
    if (EPI == CF_EPI_MASK) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            u32x4 mb = {0u, 0u, 0u, 0u};                             // the 16 sign bytes of this pixel's quads; none past the image: zeros there
            if (live[pb]) mb = *reinterpret_cast<const u32x4*>(mk + pix[pb] * c4 + cot * (CF_CO / 4));
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const unsigned bits = mb[cb] >> (8 * kg);            // byte 4 cb + kg
#pragma unroll
                for (int e = 0; e < 4; ++e) v[cb][pb][e] = ((bits >> e) & 1u) != 0u ? v[cb][pb][e] : 0.f;      // (a select, not a product)
            }
        }
    }
    if (EPI != CF_EPI_POOL) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
            if (live[pb]) {
                float* yp = y + pix[pb] * Cout + cot * CF_CO + 4 * kg;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) *reinterpret_cast<f32x4*>(yp + 16 * cb) = v[cb][pb];
            }
    }
    if (EPI == CF_EPI_RELU) {
        if (mk) {                                                    // (the same for every thread of the launch)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                unsigned own = 0;                                    // byte cb: quad 4 cb + kg
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) own |= cf_sign4(v[cb][pb]) << (8 * cb);
                // lane kg of the pixel's four stores the bytes of quads 4 kg ..+3: byte kg of each of the four lanes, in lane order
                unsigned m4 = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) m4 |= ((__shfl(own, l15 + 16 * j) >> (8 * kg)) & 0xffu) << (8 * j);
                if (live[pb]) *reinterpret_cast<unsigned*>(mk + pix[pb] * c4 + cot * (CF_CO / 4) + 4 * kg) = m4;
            }
        }
    }
    if (EPI == CF_EPI_POOL) {
        float* park = ldsf;                                          // every wave is past the last tap's barrier
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float* mine = park + (GE::trow(false, wave, pb, l15) * GE::TW + GE::tcol(false, pb, l15)) * CF_PARK + 4 * kg;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) *reinterpret_cast<f32x4*>(mine + 16 * cb) = v[cb][pb];
        }
    }
    if (EPI == CF_EPI_MASK) {
        // column sums over the wave's 32 pixels: a lane's two pixels first, then the halving butterfly over its 16-lane group (at
        // distance d a lane keeps the half of its slots that matches its bit d); slot k = 4 cb + e of the 16 ends in lane l15 = k
        double s[16];                                                // (fp64 from here to db: see conv3x3_colsum_kernel)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[4 * cb + e] = (double)v[cb][0][e] + (double)v[cb][1][e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            const bool up = (l15 & d) != 0;
#pragma unroll
            for (int i = 0; i < d; ++i) {
                const double send = up ? s[i] : s[i + d], keep = up ? s[i + d] : s[i];
                s[i] = keep + __shfl_xor(send, d);
            }
        }
        double* red = reinterpret_cast<double*>(ldsf);               // [wave][64 channels]
        red[wave * CF_CO + 16 * (l15 >> 2) + 4 * kg + (l15 & 3)] = s[0];
        __syncthreads();
        if (tid < CF_CO)
            part[(long long)tile * Cout + cot * CF_CO + tid] = ((red[tid] + red[CF_CO + tid]) + red[2 * CF_CO + tid]) + red[3 * CF_CO + tid];
    }
}

// x [N][H][W][Cin], ws as conv3x3_wsplit_kernel leaves it -> y [N][H][W][Cout]: the work of one workgroup (the kernel, behind this
// function, decodes the tile; written for 4 x 32, the other geometries: CfGeo)
//
// EPI, what happens to the accumulators on their way out (the main loop is the same code in all four):
//   CF_EPI_NONE  y = the sums                                                                    (hk_conv3x3_fwd, hk_conv3x3_bwd_data)
//   CF_EPI_RELU  y = relu4(sums + bias) and, where mk is given, the sign byte of every channel quad in the [pixel][Cout / 4] layout of
//                bias_relu_fwd_kernel<true> (trunk.hip).  A lane holds the even (hf = 0) or the odd quads of its pixel: the two
//                lanes swap their eight bytes and each stores eight consecutive ones
//   CF_EPI_POOL  y = p [N][H / 2][W / 2][Cout] = maxpool2x2(relu4(sums + bias)), mk = the 2-bit argmax codes, both exactly as
//                bias_relu_pool_fwd_kernel forms them (H, W even: every geometry is anchored at even rows and columns: a tile holds whole windows).  The
//                full-resolution map is never written: every wave parks its row in the LDS the last tap has left free, and after one
//                barrier a thread forms two pooled float4; the 16 lanes of a pooled pixel gather their code bytes into two 8-byte stores
//   CF_EPI_MASK  y = sums where the bit of mk (read: the sign mask of the map this call produces the gradient of) is set, else 0 -
//                what bias_relu_bwd_kernel<true> writes - and part [tile][Cout] = this workgroup's column sums of those values:
//                a halving butterfly over the 32 pixels of a wave (31 cross-lane adds a lane, lane l ends with channel slot l), then
//                the four waves through LDS in wave order
// bias and mask are read behind the loop: nothing joins the loads its counted waits count
//
// MF = CF_MF_16 (dynamic LDS CF16_LDS): a tap is 48 MFMAs of 16 x 16 x 32 - the six products into each of eight accumulators (four
// 16-channel blocks cb x two 16-pixel blocks pb), product by product, so that an accumulator's next MFMA is eight behind its last and its
// own order of products is the other shape's - from the same 18 fragment reads (12 weight, 6 pixel).  A lane ends with channels
// 16 cb + 4 (lane / 16) ..+3 of pixels 16 pb + lane % 16: the sixteen channel quads of a pixel sit in FOUR lanes (16 apart), quad
// 4 cb + lane / 16 in each, and the epilogues gather accordingly: CF_EPI_RELU transposes the 4 x 4 sign bytes of those lanes (each
// stores four consecutive bytes a pixel), CF_EPI_POOL parks the same [row][column][channel] tile and leaves by the same code, CF_EPI_MASK
// adds a lane's two pixels and runs the halving butterfly over 16 lanes (all in fp64, a fixed order: db stays the float next to the
// exact sum)
//
// G, the tile's geometry (CfGeo): the body below is the kernel for one tile - rows [r0, r0 + TH), columns [c0, c0 + TW) of image n, tile
// number `tile` of the launch; the kernel itself (conv3x3_split_kernel, behind it) only decodes those from the block index
template <int EPI, int MF, int G>
__device__ __forceinline__ void conv3x3_split_tile(float* ldsf, const float* __restrict__ x, const char* __restrict__ ws, float* __restrict__ y,
                                                   int H, int W, int Cin, int Cout, long long n, int r0, int c0, int tile, int cot,
                                                   const float* __restrict__ bias, uint8_t* __restrict__ mk, double* __restrict__ part) {
    typedef CfGeo<G> GE;
    constexpr bool M32 = MF == CF_MF_32;
    static_assert(!(M32 && G == CF_G_16x8), "16 x 8 is a geometry of CF_MF_16 only");
    constexpr int XPLANE = cf_xplane<MF, G>(), WTAP = M32 ? CF_WTAP : CF16_WTAP;
    constexpr int XU = GE::XU, XF4 = GE::XF4, HC = GE::HC, HP = GE::HP;
    char* xs = reinterpret_cast<char*>(ldsf);            // the halo tile of the chunk: [piece][HR x HP pixels][80 B] (CF_MF_16: cf16_off)
    char* wb = xs + 3 * XPLANE;                          // two weight tiles: [buf][piece][64 co][80 B] (CF_MF_16: cf16_off)
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int l15 = lane & 15, kg = lane >> 4;           // (CF_MF_16: the lane's row or column of a block, and its k-group)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchunk = Cin / CF_CK, total = nchunk * 9;
    const float* xi = x + n * H * W * Cin;
    const char* wt = ws + (size_t)cot * total * WTAP + tid * 16;

    // this thread's float4 loads of a halo tile: float4 idx -> pixel idx / 8 (row r0 - 1 + pixel / HC, column c0 - 1 + pixel % HC),
    // channels 4 (idx % 8) ..+3 of the chunk; clamped into the image, and whether they count
    long long xoff[XU];
    unsigned xok = 0;
#pragma unroll
    for (int u = 0; u < XU; ++u) {
        const int idx = tid + 256 * u;
        const bool in = idx < XF4;
        const int p = in ? idx >> 3 : 0, hr = p / HC, hc = p - hr * HC;
        const int row = r0 - 1 + hr, col = c0 - 1 + hc;
        if (in && row >= 0 && row < H && col >= 0 && col < W) xok |= 1u << u;
        const int rc = row < 0 ? 0 : (row < H ? row : H - 1), cc = col < 0 ? 0 : (col < W ? col : W - 1);
        xoff[u] = ((long long)rc * W + cc) * Cin + 4 * (idx & 7);
    }
    // (CF_MF_16: pixel tid / 8 + 32 u, k-group (tid & 7) / 2, its first or second four k).  Where the plane's pitch is the halo tile's
    // width the pixel's place is its number; 16 x 8 works it out per load (xdst_of)
    const int xdst = M32 ? (tid >> 3) * CF_PIX + (tid & 7) * 8 : cf16_off(tid >> 3, (tid & 7) >> 1) + (tid & 1) * 8;      // + 32 u pixels
    auto xdst_of = [&](int u) {
        if constexpr (HP == HC) {
            return xdst + u * 32 * (M32 ? CF_PIX : CF16_PIX);
        } else {
            const int p = (tid >> 3) + 32 * u, hr = p / HC;
            return cf16_off(hr * HP + (p - hr * HC), (tid & 7) >> 1) + (tid & 1) * 8;
        }
    };

    f32x4 vx[XU];
    auto load_x = [&](int chunk) {
        const float* b = xi + chunk * CF_CK;
#pragma unroll
        for (int u = 0; u < XU; ++u) HK_LOAD16_ASYNC(vx[u], b + xoff[u]);
    };
    // tile `it` on its way into buffer `buf` by LDS-DMA, no register in between: the workspace IS the LDS image, and a wave's 64 lanes
    // x 16 bytes are 1 KiB contiguous in both - what one glds16 copies (LDS base wave-uniform, lane l lands at + 16 l).  CF_MF_32: the
    // fourth piece is 3072 B - waves 0 - 2 (wave 3 has one operation fewer in flight: the counted waits count from the youngest)
    auto load_w = [&](int it, int buf) {
        const char* b = wt + (size_t)it * WTAP;
        char* d = wb + buf * WTAP + wave * 1024;
#pragma unroll
        for (int u = 0; u < 3; ++u) glds16(reinterpret_cast<const float*>(b + 4096 * u), reinterpret_cast<float*>(d + 4096 * u));
        if constexpr (M32) {
            if (wave < 3) glds16(reinterpret_cast<const float*>(b + 3 * 4096), reinterpret_cast<float*>(d + 3 * 4096));
        }
    };
    auto store_x = [&]() {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            if (tid + 256 * u < XF4) {
                bf16x4 p[3];
                wrs_split(((xok >> u) & 1) ? vx[u] : zero, p);
                const int d = xdst_of(u);
#pragma unroll
                for (int s = 0; s < 3; ++s) *reinterpret_cast<bf16x4*>(xs + s * XPLANE + d) = p[s];
            }
        }
    };

    f32x16 acc[2], sum[2];                               // CF_MF_32: [channel block of 32]
    f32x4 acc4[4][2], sum4[4][2];                        // CF_MF_16: [channel block of 16][pixel block of 16]
    if constexpr (M32) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][i] = sum[cb][i] = 0.f;
    } else {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc4[cb][pb][e] = sum4[cb][pb][e] = 0.f;
    }

    load_w(0, 0);
    load_x(0);
    __builtin_amdgcn_s_waitcnt(HK_VMCNT_IMM(0));         // (this wave's pieces of tile 0 have landed, too)
#pragma unroll
    for (int u = 0; u < XU; ++u) HK_PIN_LOADED(vx[u]);
    store_x();
    HK_LDS_BARRIER();

    const int aoff = l31 * CF_PIX + hf * 16;                        // this lane's weight row (+ 32 rows for the second block)
    const int boff = (GE::trow(true, wave, 0, l31) * HP + GE::tcol(true, 0, l31)) * CF_PIX + hf * 16;      // this lane's pixel at tap (0, 0)
    const int bpix = GE::trow(false, wave, 0, l15) * HP + GE::tcol(false, 0, l15);      // CF_MF_16: the same, as a pixel of the plane, block 0
    int since = 0;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const bool more = chunk + 1 < nchunk;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int it = chunk * 9 + tap;
            // the next weight tile (the last step requests its own again: an unconditional, in-bounds request) into the buffer tap - 1
            // read - every wave is past the barrier that ended that tap, with its reads done - and, at tap 5, the next chunk's x tile:
            // in flight while this tap's MFMAs run
            load_w(it + 1 < total ? it + 1 : it, (it + 1) & 1);
            if (tap == 5) load_x(more ? chunk + 1 : chunk);
            if constexpr (M32) {
            const char* A = wb + (it & 1) * CF_WTAP + aoff;
            const char* B = xs + boff + ((tap / 3) * HP + tap % 3) * CF_PIX;
            bf16x8 a[2][2][3], b[2][3];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    b[ks][s] = cf_frag(B + s * XPLANE + ks * 32);
                    a[ks][0][s] = cf_frag(A + s * CF_WPLANE + ks * 32);
                    a[ks][1][s] = cf_frag(A + s * CF_WPLANE + 32 * CF_PIX + ks * 32);
                }
            __builtin_amdgcn_sched_barrier(0);           // every fragment read in front of the MFMAs (CF_TAP_BARRIER)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    // the six products of first and second order, small ones first (conv_wrw.hip)
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][1], b[ks][1], acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][0], b[ks][2], acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][2], b[ks][0], acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][0], b[ks][1], acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][1], b[ks][0], acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][cb][0], b[ks][0], acc[cb], 0, 0, 0);
                }
            } else {
                // the lane's pixels of this tap, one per pixel block; the image offset depends on the pixel (cf16_off): a constant
                // from block 0 to block 1 where they are a multiple of 16 pixels apart, worked out for both otherwise (8 x 16: 18 pixels)
                const char* A = wb + (it & 1) * CF16_WTAP + cf16_off(l15, kg);
                const int bp = bpix + (tap / 3) * HP + tap % 3;
                const char* Bp[2];
                Bp[0] = xs + cf16_off(bp, kg);
                Bp[1] = GE::PBD % 16 == 0 ? Bp[0] + GE::PBD * CF16_PIX : xs + cf16_off(bp + GE::PBD, kg);
                bf16x8 a[4][3], b[2][3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
#pragma unroll
                    for (int pb = 0; pb < 2; ++pb) b[pb][s] = cf_frag(Bp[pb] + s * XPLANE);
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) a[cb][s] = cf_frag(A + s * CF16_WPLANE + cb * 16 * CF16_PIX);
                }
                __builtin_amdgcn_sched_barrier(0);       // every fragment read in front of the MFMAs (CF_TAP_BARRIER)
                // the same six products in the same order, each into all eight accumulators before the next
                constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
                for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                        for (int pb = 0; pb < 2; ++pb) acc4[cb][pb] = mfma_f32_16x16x32_bf16(a[cb][PA[pr]], b[pb][PB[pr]], acc4[cb][pb]);
            }
            // The tap ends with a counted wait and a raw barrier: tile it + 1 has landed for every wave, and every wave has read this
            // tap's buffer.  Requests retire in order and the weight pieces were issued first: at tap 5 the XU x loads behind them
            // stay in flight, and tap 6's wait - its own pieces are behind them - covers them
            if (tap == 5) CF_TAP_BARRIER(XU);
            else CF_TAP_BARRIER(0);                      // (tap 8: and every wave is past its last read of the chunk's x tile)
            if (tap == 6) {
#pragma unroll
                for (int u = 0; u < XU; ++u) HK_PIN_LOADED(vx[u]);
            }
            if (tap == 8 && more) {
                store_x();
                HK_LDS_BARRIER();                        // (lgkmcnt(0): the x tile's writes have landed)
            }
        }
        if (++since == CF_FLUSH) {
            if constexpr (M32) {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    sum[cb] += acc[cb];
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
                }
            } else {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int pb = 0; pb < 2; ++pb) {
                        sum4[cb][pb] += acc4[cb][pb];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc4[cb][pb][e] = 0.f;
                    }
            }
            since = 0;
        }
    }
    if constexpr (!M32) {
        cf16_epilogue<EPI, G>(acc4, sum4, ldsf, y, H, W, Cout, n, r0, c0, cot, tile, wave, tid, l15, kg, bias, mk, part);
        if (EPI != CF_EPI_POOL) return;                  // (the pooled tile is parked: it leaves below, as the other shape's)
    }
    // C layout of the 32 x 32 MFMA: column = lane & 31 (pixel), row = 8 (i / 4) + 4 (lane >> 5) + i % 4 (output channel)
    const int trow = GE::trow(true, wave, 0, l31), tcol = GE::tcol(true, 0, l31);      // (CF_MF_32: this lane's pixel of the tile)
    const int row = r0 + trow, col = c0 + tcol;
    if (EPI == CF_EPI_NONE) {
        if (row < H && col < W) {
            float* yp = y + ((n * H + row) * W + col) * Cout + cot * CF_CO + 4 * hf;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = sum[cb][4 * j + e] + acc[cb][4 * j + e];
                    *reinterpret_cast<f32x4*>(yp + cb * 32 + 8 * j) = v;
                }
        }
        return;
    }
    // v[cb][j]: channel quad 8 cb + 2 j + hf of this workgroup's sixteen
    const bool live = row < H && col < W;
    const long long pix = (n * H + row) * W + col;                  // (used where live)
    const int c4 = Cout / 4;
    f32x4 v[2][4];
    if constexpr (M32) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[cb][j][e] = sum[cb][4 * j + e] + acc[cb][4 * j + e];
    }
    if (M32 && (EPI == CF_EPI_RELU || EPI == CF_EPI_POOL)) {
        const f32x4* b4 = reinterpret_cast<const f32x4*>(bias + cot * CF_CO + 4 * hf);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[cb][j] = cf_relu4(v[cb][j] + b4[8 * cb + 2 * j]);
    }
    if (EPI == CF_EPI_RELU) {
        if (live) {
            float* yp = y + pix * Cout + cot * CF_CO + 4 * hf;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(yp + cb * 32 + 8 * j) = v[cb][j];
        }
        if (mk) {                                                    // (the same for every thread of the launch)
            unsigned own[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                own[cb] = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) own[cb] |= cf_sign4(v[cb][j]) << (8 * j);
            }
            // hf = 0 stores the bytes of quads 0 - 7 (its own even ones, the partner's odd ones of cb = 0), hf = 1 those of 8 - 15
            const unsigned theirs0 = __shfl_xor(own[0], 32), theirs1 = __shfl_xor(own[1], 32);
            const unsigned ev = hf ? theirs1 : own[0], od = hf ? own[1] : theirs0;
            unsigned long long m8 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                m8 |= ((unsigned long long)((ev >> (8 * k)) & 0xffu) << (16 * k)) | ((unsigned long long)((od >> (8 * k)) & 0xffu) << (16 * k + 8));
            if (live) *reinterpret_cast<unsigned long long*>(mk + pix * c4 + cot * (CF_CO / 4) + 8 * hf) = m8;
        }
    }
    if (EPI == CF_EPI_POOL) {
        float* park = ldsf;                                          // [tile row][tile column][CF_PARK floats]: every wave is past the last tap's barrier
        if constexpr (M32) {
        float* mine = park + (trow * GE::TW + tcol) * CF_PARK + 4 * hf;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(mine + cb * 32 + 8 * j) = v[cb][j];
        }                                                            // (CF_MF_16: cf16_epilogue has parked the same tile)
        __syncthreads();
        // channel quad q of pooled pixels tid / 16 and tid / 16 + 16 of the tile's TH / 2 x TW / 2, row-major (4 x 32: column tid / 16 of
        // pooled rows u = 0, 1)
        constexpr int TW = GE::TW, PW = TW / 2;
        const int q = tid & 15;
        const int Ho = H / 2, Wo = W / 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pp = (tid >> 4) + 16 * u, pr = pp / PW, pc = pp % PW;
            const float* src = park + (2 * pr * TW + 2 * pc) * CF_PARK + 4 * q;
            f32x4 m = *reinterpret_cast<const f32x4*>(src);
            unsigned code = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(src + ((k >> 1) * TW + (k & 1)) * CF_PARK);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const bool take = (a[t] > m[t]) || (a[t] != a[t]);          // ATen max_pool2d: (val > max) || isnan(val)
                    m[t] = take ? a[t] : m[t];
                    code = take ? ((code & ~(3u << (2 * t))) | ((unsigned)k << (2 * t))) : code;
                }
            }
            // the code bytes of quads 8 (q / 8) ..+7 of this pooled pixel, gathered from their eight lanes, in every one of them
            unsigned t1 = __shfl_xor(code, 1);
            unsigned c2 = (q & 1) ? (t1 | (code << 8)) : (code | (t1 << 8));
            unsigned t2 = __shfl_xor(c2, 2);
            unsigned c4b = (q & 2) ? (t2 | (c2 << 16)) : (c2 | (t2 << 16));
            unsigned t4 = __shfl_xor(c4b, 4);
            const unsigned long long lo = (q & 4) ? t4 : c4b, hi = (q & 4) ? c4b : t4;
            const int ho = r0 / 2 + pr, wo = c0 / 2 + pc;
            if (ho < Ho && wo < Wo) {
                const long long opix = (n * Ho + ho) * Wo + wo;
                *reinterpret_cast<f32x4*>(y + opix * Cout + cot * CF_CO + 4 * q) = m;
                if ((q & 7) == 0) *reinterpret_cast<unsigned long long*>(mk + opix * c4 + cot * (CF_CO / 4) + q) = lo | (hi << 32);
            }
        }
    }
    if (EPI == CF_EPI_MASK) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        u32x4 mb = {0u, 0u, 0u, 0u};                                 // the 16 sign bytes of this pixel's quads; none past the image: zeros there
        if (live) mb = *reinterpret_cast<const u32x4*>(mk + pix * c4 + cot * (CF_CO / 4));
        double s[32];                                                // (fp64 from here to db: see conv3x3_colsum_kernel)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned bits = mb[2 * cb + (j >> 1)] >> (8 * (2 * (j & 1) + hf));          // byte 2 (4 cb + j) + hf
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[cb][j][e] = ((bits >> e) & 1u) != 0u ? v[cb][j][e] : 0.f;                   // (bias_relu_bwd_kernel: a select, not a product)
                    s[16 * cb + 4 * j + e] = v[cb][j][e];
                }
            }
        if (live) {
            float* yp = y + pix * Cout + cot * CF_CO + 4 * hf;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(yp + cb * 32 + 8 * j) = v[cb][j];
        }
        // column sums over the wave's 32 pixels: at distance d a lane keeps the half of its slots that matches its bit d and adds the
        // partner's values of that half; slot k of the 32 ends in lane l31 = k
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            const bool up = (l31 & d) != 0;
#pragma unroll
            for (int i = 0; i < d; ++i) {
                const double send = up ? s[i] : s[i + d], keep = up ? s[i + d] : s[i];
                s[i] = keep + __shfl_xor(send, d);
            }
        }
        // slot k = 16 cb + 4 j + e is channel 32 cb + 8 j + 4 hf + e of the 64
        double* red = reinterpret_cast<double*>(ldsf);               // [wave][64 channels]
        red[wave * CF_CO + 32 * (l31 >> 4) + 8 * ((l31 >> 2) & 3) + 4 * hf + (l31 & 3)] = s[0];
        __syncthreads();
        if (tid < CF_CO)
            part[(long long)tile * Cout + cot * CF_CO + tid] = ((red[tid] + red[CF_CO + tid]) + red[2 * CF_CO + tid]) + red[3 * CF_CO + tid];
    }
}

// The kernel: grid xcd_grid(ntiles, Cout / 64), dynamic LDS cf_lds<MF, PLAN>().  One geometry (PLAN = CF_PLAN_4x32, CF_PLAN_8x16):
// tile = ((n nrb + rb) nstrips + strip), rows [TH rb, ..), columns [TW strip, ..).  CF_PLAN_MIXED: tile = n tpi + t with tpi = nA + nrbB
// nstripsB tiles an image; t < nA = nrb nstrips is tile (rb, strip) of the 8 x 16 region, whose strips are whole (nstrips = W / 16, so it may
// be empty), the others are 16 x 8 tiles (rb, strip) of the region from column 16 nstrips on
template <int EPI, int MF, int PLAN>
__global__ __launch_bounds__(256, 2) void conv3x3_split_kernel(const float* __restrict__ x, const char* __restrict__ ws,
                                                               float* __restrict__ y, int H, int W, int Cin, int Cout, int nstrips,
                                                               int nrb, int ntiles, const float* __restrict__ bias,
                                                               uint8_t* __restrict__ mk, double* __restrict__ part, int nstripsB, int tpi) {
    HK_DYN_LDS16(ldsf);
    int tile, cot;
    if (!xcd_map(blockIdx.x, ntiles, Cout / CF_CO, tile, cot)) return;
    if constexpr (PLAN != CF_PLAN_MIXED) {
        typedef CfGeo<PLAN> GE;
        const int strip = tile % nstrips, tr = tile / nstrips;
        const int rb = tr % nrb;
        const long long n = tr / nrb;
        conv3x3_split_tile<EPI, MF, PLAN>(ldsf, x, ws, y, H, W, Cin, Cout, n, rb * GE::TH, strip * GE::TW, tile, cot, bias, mk, part);
    } else {
        const long long n = tile / tpi;
        const int t = tile % tpi, nA = nrb * nstrips;
        if (t < nA) {
            conv3x3_split_tile<EPI, MF, CF_G_8x16>(ldsf, x, ws, y, H, W, Cin, Cout, n, (t / nstrips) * 8, (t % nstrips) * 16, tile, cot, bias, mk,
                                                   part);
        } else {
            const int tb = t - nA;
            conv3x3_split_tile<EPI, MF, CF_G_16x8>(ldsf, x, ws, y, H, W, Cin, Cout, n, (tb / nstripsB) * 16, nstrips * 16 + (tb % nstripsB) * 8,
                                                   tile, cot, bias, mk, part);
        }
    }
}

// part [nrows][nel] -> out [gridDim.y][nel]: group g = blockIdx.y adds rows [g rpg, (g + 1) rpg) in a fixed order, as partial_sum_kernel
// (hk_partial_sum.h) does for all rows - the first stage (OUT = double) spreads up to 25088 partial rows (25.7 MB) over the chip, the
// second (OUT = float) adds the groups' rows.  The column sums stay fp64 from the wave's butterfly to here and are rounded ONCE, by the
// second stage's store: db is the float next to the exact sum whatever the order of the additions was (the two-kernel path's fp32
// chain of up to 12.8 M additions is one of the floats further away, or the same one)
template <int Q, typename OUT>
__global__ __launch_bounds__(64 * Q) void conv3x3_colsum_kernel(const double* __restrict__ part, int nrows, int nel, int rpg,
                                                                OUT* __restrict__ out) {
    __shared__ double red[Q][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + l;
    const int beg = blockIdx.y * rpg, end = beg + rpg < nrows ? beg + rpg : nrows;
    double s = 0.0;
    if (e < nel) {
        int k = beg + q;
        for (; k + 7 * Q < end; k += 8 * Q) {
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = part[(long long)(k + Q * u) * nel + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t[u];
        }
        for (; k < end; k += Q) s += part[(long long)k * nel + e];
    }
    red[q][l] = s;
    __syncthreads();
    if (q == 0 && e < nel) {
        double t = red[0][l];
        for (int k = 1; k < Q; ++k) t += red[k][l];
        out[(long long)blockIdx.y * nel + e] = (OUT)t;
    }
}

// The tiling of an H x W map on MFMA shape mf: the candidate with the fewest tiles - 4 x 32, then 8 x 16, then (CF_MF_16 only) 8 x 16 over
// the W / 16 whole strips with 16 x 8 over the remaining columns; a tie keeps the earlier one, so nothing changes where nothing is saved.
// Knob `conv_tile`: 0 is 4 x 32 everywhere, anything else this choice - so a launch never has more tiles than 4 x 32 gives it.
// VGG-16 at 448 x 448: 448, 224 and 28 wide keep 4 x 32 (1568, 392 and 7 tiles an image), 112 takes 8 x 16 (98 tiles for 112), 56 the
// mixed plan on CF_MF_16 (21 + 4 = 25 for 28) and nothing better than 28 on CF_MF_32
struct CfPlan {
    int plan;                                            // CF_PLAN_*
    long long tpi;                                       // tiles of an image
    int nrb, nstrips;                                    // the (first) region's row blocks and strips
    int nrbB, nstripsB;                                  // CF_PLAN_MIXED: the 16 x 8 region's, from column 16 nstrips on
};
static CfPlan conv3x3_plan(int H, int W, int mf, int knob) {
    auto cdiv = [](long long a, long long b) { return (int)((a + b - 1) / b); };
    CfPlan c[3];
    c[0] = {CF_PLAN_4x32, 0, cdiv(H, 4), cdiv(W, 32), 0, 0};
    c[1] = {CF_PLAN_8x16, 0, cdiv(H, 8), cdiv(W, 16), 0, 0};
    c[2] = {CF_PLAN_MIXED, 0, cdiv(H, 8), W / 16, cdiv(H, 16), cdiv(W % 16, 8)};
    for (CfPlan& p : c) p.tpi = (long long)p.nrb * p.nstrips + (long long)p.nrbB * p.nstripsB;
    const int ncand = mf == CF_MF_16 ? 3 : 2;
    if (knob == 0) return c[0];
    int best = 0;
    for (int i = 1; i < ncand; ++i)
        if (c[i].tpi < c[best].tpi) best = i;
    return c[best];
}

// x [N][H][W][K] (*) w -> y [N][H][W][M] (or what EPI makes of it): the pre-pass and the main kernel; M, K multiples of 64
template <int EPI, int MF, int PLAN>
static int conv3x3_run_on(const float* x, const float* w, float* y, int N, int H, int W, int K, int M, bool transposed, void* ws,
                          hipStream_t stream, const float* bias, uint8_t* mk, double* part, const CfPlan& pl) {
    constexpr int LDS = cf_lds<MF, PLAN>();
    const long long ntiles = N * pl.tpi;
    const int ncot = M / CF_CO;
    if ((ntiles + NXCD) * ncot > 0x7fffffffll) return HK_ERR_UNSUPPORTED;
    const long long total = (long long)ncot * (K / CF_CK) * 9 * CF_CO * (MF == CF_MF_32 ? 10 : 8);
    hipLaunchKernelGGL(conv3x3_wsplit_kernel<MF>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, (char*)ws, M, K,
                       transposed ? 1 : 0, total);
    HK_LAUNCH_CHECK();
    HK_ALLOW_BIG_LDS((conv3x3_split_kernel<EPI, MF, PLAN>), LDS);
    hipLaunchKernelGGL((conv3x3_split_kernel<EPI, MF, PLAN>), dim3((unsigned)xcd_grid((int)ntiles, ncot)), dim3(256), LDS, stream, x,
                       (const char*)ws, y, H, W, K, M, pl.nstrips, pl.nrb, (int)ntiles, bias, mk, part, pl.nstripsB, (int)pl.tpi);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
// Whether the GEMM of a call - x [N][H][W][K] (*) w -> [N][H][W][M], for the input gradient K = Cout and M = Cin: the forward of dy - is
// faster on v_mfma_f32_16x16x32_bf16: what knob `conv_mfma` runs at its default.  A function of the GEMM alone: the four epilogues of one
// GEMM run one main loop, and an input gradient runs the loop that the forward of dy with flipped weights runs.
// Rule: always.  Measured on an MI355X inside the training step (VGG-16 at 448 x 448, HK_CONV_MFMA=0 against the default, one kernel trace
// each: profiles/conv_mf16_step_layers.json): all 24 layer-directions are faster on 16 x 16 x 32 at batch 64 (0.16 - 1.21 ms a launch, the 24
// launches 75.3 -> 62.2 ms) and at batch 16 (19.0 -> 16.0), as all 48 were before the planned tiles (profiles/conv_wdma_mfma_step_layers.json);
// the stand-alone bar that functional.py's tables were made with decides by its own noise ("Weight tiles by LDS-DMA", last
// paragraph).  The arguments are what a finer rule would be written in
static bool conv3x3_mfma16_wins(int N, int H, int W, int K, int M) {
    (void)N, (void)H, (void)W, (void)K, (void)M;
    return true;
}
// THE MFMA shape of a call, for everything that follows it (the plan's geometries, the pre-pass, the main kernel, the partial rows of the
// masked input gradient): knob `conv_mfma` 1 = 16 x 16 x 32 everywhere, 0 = 32 x 32 x 16 everywhere, -1 (the default) = the rule above
static int conv3x3_mf(int N, int H, int W, int K, int M) {
    const int knob = tuning().conv_mfma;
    return knob == 1 || (knob < 0 && conv3x3_mfma16_wins(N, H, W, K, M)) ? CF_MF_16 : CF_MF_32;
}
// ... on that shape, tiled as conv3x3_plan says
template <int EPI>
static int conv3x3_run(const float* x, const float* w, float* y, int N, int H, int W, int K, int M, bool transposed, void* ws,
                       hipStream_t stream, const float* bias = nullptr, uint8_t* mk = nullptr, double* part = nullptr) {
    const int mf = conv3x3_mf(N, H, W, K, M);
    const CfPlan pl = conv3x3_plan(H, W, mf, tuning().conv_tile);
    if (pl.tpi > 0x7fffffffll) return HK_ERR_UNSUPPORTED;
    if (mf == CF_MF_16) {
        if (pl.plan == CF_PLAN_MIXED) return conv3x3_run_on<EPI, CF_MF_16, CF_PLAN_MIXED>(x, w, y, N, H, W, K, M, transposed, ws, stream, bias, mk, part, pl);
        if (pl.plan == CF_PLAN_8x16) return conv3x3_run_on<EPI, CF_MF_16, CF_PLAN_8x16>(x, w, y, N, H, W, K, M, transposed, ws, stream, bias, mk, part, pl);
        return conv3x3_run_on<EPI, CF_MF_16, CF_PLAN_4x32>(x, w, y, N, H, W, K, M, transposed, ws, stream, bias, mk, part, pl);
    }
    if (pl.plan == CF_PLAN_8x16) return conv3x3_run_on<EPI, CF_MF_32, CF_PLAN_8x16>(x, w, y, N, H, W, K, M, transposed, ws, stream, bias, mk, part, pl);
    return conv3x3_run_on<EPI, CF_MF_32, CF_PLAN_4x32>(x, w, y, N, H, W, K, M, transposed, ws, stream, bias, mk, part, pl);
}

static int conv3x3_check(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                         int knob) {
    if (!x || !w || !y || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_conv3x3_ws_bytes(Cin, Cout)) return HK_ERR_WORKSPACE;
    if (Cin % 64 != 0 || Cout % 64 != 0 || (long long)Cout * 9 * Cin > 0x7fffffffll || !aligned16(x) || !aligned16(w) || !aligned16(y) ||
        !aligned16(ws) || knob == 0)
        return HK_ERR_UNSUPPORTED;
    return HK_OK;
}

// tiles of a map (= partial rows of the masked input gradient) and the groups the first reduction stage makes of them
static long long conv3x3_tiles(int N, int H, int W) {
    return (long long)N * (((long long)H + CF_R - 1) / CF_R) * (((long long)W + CF_SW - 1) / CF_SW);
}
static long long conv3x3_groups(long long ntiles) { return ntiles > CF_DB_RPG ? (ntiles + CF_DB_RPG - 1) / CF_DB_RPG : 0; }

}  // namespace hk

using namespace hk;

extern "C" size_t hk_conv3x3_ws_bytes(int Cin, int Cout) {          // (for any sizes > 0: the workspace check comes before the shape check)
    if (Cin <= 0 || Cout <= 0) return 0;
    const size_t a = ((size_t)Cout + 63) / 64 * (((size_t)Cin + 31) / 32), b = ((size_t)Cin + 63) / 64 * (((size_t)Cout + 31) / 32);
    return (a > b ? a : b) * 9 * CF_WTAP;                            // the split weights, either way round
}

extern "C" int hk_conv3x3_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                              hk_stream_t stream) {
    const int rc = conv3x3_check(x, w, y, N, H, W, Cin, Cout, ws, ws_bytes, tuning().conv_fwd);
    return rc != HK_OK ? rc : conv3x3_run<CF_EPI_NONE>(x, w, y, N, H, W, Cin, Cout, false, ws, (hipStream_t)stream);
}

extern "C" int hk_conv3x3_bwd_data(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, void* ws,
                                   size_t ws_bytes, hk_stream_t stream) {
    const int rc = conv3x3_check(dy, w, dx, N, H, W, Cin, Cout, ws, ws_bytes, tuning().conv_bwd_data);
    return rc != HK_OK ? rc : conv3x3_run<CF_EPI_NONE>(dy, w, dx, N, H, W, Cout, Cin, true, ws, (hipStream_t)stream);
}

extern "C" int hk_conv3x3_bias_relu_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int N, int H, int W,
                                        int Cin, int Cout, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!bias) return HK_ERR_BAD_ARG;
    const int rc = conv3x3_check(x, w, y, N, H, W, Cin, Cout, ws, ws_bytes, tuning().conv_fwd);
    if (rc != HK_OK) return rc;
    if (!aligned16(bias) || (((uintptr_t)mask) & 7) != 0 || tuning().conv_epi < 1) return HK_ERR_UNSUPPORTED;
    return conv3x3_run<CF_EPI_RELU>(x, w, y, N, H, W, Cin, Cout, false, ws, (hipStream_t)stream, bias, mask);
}

extern "C" int hk_conv3x3_bias_relu_pool_fwd(const float* x, const float* w, const float* bias, float* p, uint8_t* argmax, int N, int H,
                                             int W, int Cin, int Cout, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!bias || !argmax) return HK_ERR_BAD_ARG;
    const int rc = conv3x3_check(x, w, p, N, H, W, Cin, Cout, ws, ws_bytes, tuning().conv_fwd);
    if (rc != HK_OK) return rc;
    if (H % 2 != 0 || W % 2 != 0 || !aligned16(bias) || (((uintptr_t)argmax) & 7) != 0 || tuning().conv_epi < 1) return HK_ERR_UNSUPPORTED;
    return conv3x3_run<CF_EPI_POOL>(x, w, p, N, H, W, Cin, Cout, false, ws, (hipStream_t)stream, bias, argmax);
}

extern "C" size_t hk_conv3x3_masked_ws_bytes(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    const long long ntiles = conv3x3_tiles(N, H, W);
    return hk_conv3x3_ws_bytes(Cin, Cout) + (size_t)(ntiles + conv3x3_groups(ntiles)) * Cin * sizeof(double);
}

extern "C" int hk_conv3x3_tile_plan(int N, int H, int W, int mf, int* out) {
    if (!out || N <= 0 || H <= 0 || W <= 0 || (mf != CF_MF_32 && mf != CF_MF_16)) return HK_ERR_BAD_ARG;
    const CfPlan pl = conv3x3_plan(H, W, mf, tuning().conv_tile);
    if (pl.tpi > 0x7fffffffll) return HK_ERR_UNSUPPORTED;
    const bool mixed = pl.plan == CF_PLAN_MIXED;
    const int th = pl.plan == CF_PLAN_4x32 ? 4 : 8;
    const bool a = pl.nstrips > 0;                                   // (the mixed plan of a map narrower than 16 has no 8 x 16 region)
    int r[2][5] = {{th, 128 / th, pl.nrb, pl.nstrips, 0}, {16, 8, pl.nrbB, pl.nstripsB, 16 * pl.nstrips}};
    const int first = mixed && !a ? 1 : 0, nreg = mixed && a && pl.nstripsB > 0 ? 2 : 1;
    out[0] = (int)pl.tpi;
    out[1] = nreg;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 5; ++k) out[2 + 5 * i + k] = i < nreg ? r[first + i][k] : 0;
    return HK_OK;
}

extern "C" int hk_conv3x3_masked_bwd_data(const float* dy, const float* w, const uint8_t* mask, float* dx, float* dbias, int N, int H, int W,
                                          int Cin, int Cout, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!mask || !dbias) return HK_ERR_BAD_ARG;
    const int rc = conv3x3_check(dy, w, dx, N, H, W, Cin, Cout, ws, ws_bytes, tuning().conv_bwd_data);
    if (rc != HK_OK) return rc;
    if (ws_bytes < hk_conv3x3_masked_ws_bytes(N, H, W, Cin, Cout)) return HK_ERR_WORKSPACE;
    if (!aligned16(mask) || tuning().conv_epi < 2) return HK_ERR_UNSUPPORTED;
    // the partial rows are those of the tiles the launch really has (the GEMM is the forward of dy: K = Cout, M = Cin): never more than the
    // 4 x 32 tiles the workspace is sized for
    const long long ntiles = N * conv3x3_plan(H, W, conv3x3_mf(N, H, W, Cout, Cin), tuning().conv_tile).tpi, ngroups = conv3x3_groups(ntiles);
    if (ntiles > conv3x3_tiles(N, H, W) || ntiles > 0x7fffffffll || ngroups > 65535) return HK_ERR_UNSUPPORTED;
    double* part = reinterpret_cast<double*>((char*)ws + hk_conv3x3_ws_bytes(Cin, Cout));    // [ntiles][Cin], then [ngroups][Cin]
    double* grp = part + ntiles * Cin;
    const int rc2 = conv3x3_run<CF_EPI_MASK>(dy, w, dx, N, H, W, Cout, Cin, true, ws, (hipStream_t)stream, nullptr, const_cast<uint8_t*>(mask), part);
    if (rc2 != HK_OK) return rc2;
    const dim3 cols((unsigned)(Cin / 64));
    if (ngroups > 0) {
        hipLaunchKernelGGL((conv3x3_colsum_kernel<16, double>), dim3(cols.x, (unsigned)ngroups), dim3(1024), 0, (hipStream_t)stream,
                           (const double*)part, (int)ntiles, Cin, CF_DB_RPG, grp);
        HK_LAUNCH_CHECK();
        hipLaunchKernelGGL((conv3x3_colsum_kernel<16, float>), cols, dim3(1024), 0, (hipStream_t)stream, (const double*)grp, (int)ngroups, Cin,
                           (int)ngroups, dbias);
    } else {
        hipLaunchKernelGGL((conv3x3_colsum_kernel<16, float>), cols, dim3(1024), 0, (hipStream_t)stream, (const double*)part, (int)ntiles, Cin,
                           (int)ntiles, dbias);
    }
    HK_LAUNCH_CHECK();
    return HK_OK;
}
