// Weight gradient of the trunk's 3 x 3 convolutions whose input channel count is a multiple of 64 (model/backbone/vgg.py:24-57; stride 1, padding 1, fp32,
// channels_last).  First the two layers with 64 input channels (conv1_2, 64 -> 64 at 448 x 448, and conv2_1, 64 -> 128 at 224 x 224),
// which both forms below serve; "Wide" at the end of this header: the ten layers with 128 - 512 input channels, split form only:
//   dW[o][kh][kw][ci] = sum over pixels of dy[pix][o] x[pix + (kh - 1, kw - 1)][ci]
// - a GEMM with M = Cout, N = 9 * 64 = 576 and K = N H W pixels (12.8 M at the metric shape).  The library runs these two
// layers on a 64 x 64 tile with one 32 x 32 MFMA block per wave (an LDS operand fetch for almost every MFMA) and splits K
// with float atomics behind a zero-fill: 112 - 122 TF/s where its other weight gradients reach 131
// (profiles/r6_step_BCNN_kernel_stats.csv).  Here a workgroup keeps a WHOLE 64 x 576 result in its accumulators (four
// waves x nine 32 x 32 blocks = 144 registers per lane) over all the pixels it is given, so that the matrix pipe is the only
// thing that is busy: per pixel pair a wave reads one A and nine B values from LDS for nine MFMAs.
//
//   NHWC is the MFMA's own operand layout: v_mfma_f32_32x32x2_f32 wants A[i = lane % 32][k = lane / 32] and
//   B[k = lane / 32][j = lane % 32]; with k = the pixel of a pair, i = output channel, j = input channel, a lane's A value is
//   dy[pix + lane / 32][o0 + lane % 32] and its B value x[pix + shift + lane / 32][c0 + lane % 32]: 32 consecutive floats per
//   half wave, conflict-free ds_read_b32 at any pitch.
//
//   job      = (image, strip of 32 columns, block of rows); a workgroup owns a fixed, contiguous list of jobs
//   row step = one image row of the strip: the dy segment (32 pixels x 64 channels of the workgroup's Cout slice) and the x
//              segment of the row below (34 pixels with the column halo x 64) come in through registers while the MFMAs of the
//              current row run - the three x rows a step needs stay in a four-slot LDS ring, dy is double-buffered; one barrier
//              per step (144 MFMAs per wave)
//   borders  = rows -1 and H, columns -1 and W, the pixels past a ragged last strip: zeros in LDS (the load is made from a
//              clamped, in-bounds address and replaced) - nothing outside the two tensors is read, rows of the neighbouring
//              image are never used
//   result   = every workgroup writes its 64 x 576 partial; partial_sum_kernel adds the partials of an element in a fixed order
//              (no atomics, no zero-fill: the same input gives the same bits)
//
// Split form (conv3x3_wrw_split_kernel, knob wrw_split): the fp32 form runs at 92 % of the fp32 matrix pipe, and the chip has no xf32,
// but its bf16 pipe is 16 x the fp32 one.  Every x and dy value is split, once per element per workgroup on its way from registers to
// LDS, into hi = bf16_rn(a), mid = bf16_rn(a - hi), lo = bf16_rn(a - hi - mid) (both differences exact in fp32; a = hi + mid + lo
// to 2^-27 |a|; zeros stay zeros), and a tap's product is the six bf16 MFMAs of first and second order - hi hi, hi mid, mid hi,
// hi lo, lo hi, mid mid - into the same nine fp32 accumulators: per 16 pixels and wave 9 x 6 v_mfma_f32_32x32x16_bf16 = 1728 pipe
// cycles where the fp32 form takes 9 x 8 v_mfma_f32_32x32x2_f32 = 4608.  Same jobs, ring, borders, partial results and finish.
//   numerics = the dropped products (mid lo, lo mid, lo lo) are below 2^-24 |x| |dy|: at most 3.9e-8 S from float64, S = sum |x| |dy|,
//              1.1 - 1.3e-7 S with the fp32 accumulation - what a plain fp32 evaluation gives (tests: the fp32 form's 1e-6 S bound).
//              Dropping the second order (three MFMAs) gives 1e-6 - 2e-5 S.  Domain: finite inputs, |a| < 2^127, zero or no smaller
//              than about 2^-100 (below, the low pieces reach bf16 subnormals; whether the bf16 MFMA flushes them is unmeasured).  A
//              non-finite input makes every dW element it touches non-finite: inf splits into (inf, NaN, NaN), so NaN where the fp32
//              form may give +-inf.
//   operands = the instruction wants 8 consecutive k (pixels) of one channel per lane, NHWC has the channel contiguous: LDS keeps
//              [pixel][channel] bf16 planes, one per piece and per 32-channel half (a wave's A or B tile is one half), 64 bytes a
//              pixel, written with 8-byte vector stores (a thread's float4 = 4 channels of one pixel, per piece), and read with the
//              transposing ds_read_b64_tr_b16: a 16-lane group fetches 4 pixels x 16 channels and each lane gets the 4 pixels of its
//              channel; two reads make a fragment.  A tap's shift kw is 64 bytes in the instruction's offset field.
//   banks    = a 32-lane half of a transposing read covers 4 consecutive pixels x 32 channels = 256 contiguous bytes of a plane - one
//              whole row of the 64 banks whatever pixel it starts at, so every operand read is conflict-free at any kw (with 64-channel
//              rows, 128 bytes a pixel, pixels q and q + 2 of a read would meet: 2-way).  The 8-byte stores of a half wave cover two
//              runs of 128 bytes (2 pixels x 64 B in each channel half): one pass over the 32 banks that writes use each.
//   LDS      = 4 x 34 x 64 x 6 B + 2 x 32 x 64 x 6 B = 76800 B (dynamic), 240 registers, no spill: two workgroups per CU - measured
//              against one (conv1_2 4.48 - 4.63 ms against 4.91 - 4.92)
//   chains   = the bf16 MFMA does not round into its accumulator as an fp32 fma does: one chain over a workgroup's whole share
//              (25088 pixels at conv1_2, batch 64) ended 2.7e-5 from the fp32 form, and the error grows with the chain and the size
//              of the running sum.  Every WRS_FLUSH = 32 row steps a wave adds its accumulators to its part of the workgroup's
//              partial with ordinary fp32 additions (the first time a store) and starts them from zero: 6.1e-6 there
//   schedule = per row step 18 rounds (2 chunks of 16 pixels x 9 taps) of six MFMAs; the six transposing reads of round i + 1 are
//              issued in front of the MFMAs of round i, held there by scheduling fences
//
// Wide (conv3x3_wrw_split_kernel<true>, knob wrw_wide): nothing in the method depends on Cin being 64.  With Cin a multiple of 64 a workgroup owns
// the 64 x 9 x 64 block of dW of one (Cout slice, Cin slice) pair and reads its 64 input channels out of the Cin-wide pixels of x the
// way dy's 64 channels have always been read out of Cout-wide pixels: a runtime pixel stride and a channel offset of 64 cslice in the
// image base, the row segment offsets and the loads; LDS layout, operand reads, ring, borders, chains and schedule are untouched (240
// registers, no spill, two workgroups per CU, as the 64-channel instantiation, whose code is the parent's but for scalar address
// arithmetic).  The partial result is [workgroup][Cout][9][Cin] - a row pitch of 9 Cin and a tap pitch of Cin at the flush - and
// partial_sum_kernel runs over Cout 9 Cin elements.
//   plan     = two workgroups per CU over ALL slices: max(1, 512 / slices) per slice (conv2_2: 4 slices x 128, conv3_2: 16 x 32,
//              conv4_2 / conv5_x: 64 x 8), which is also what the workspace holds: 75.5 MB whenever slices <= 512
//   grid     = (workgroups per slice, Cout slices, Cin slices): the workgroups of a slice are next to each other in the dispatch
//              order, so with a multiple of 8 workgroups per slice every slice of one pixel share lands on the same XCD and its x and dy rows are
//              in that L2 for the other slices (HBM: each x slab is needed by Cout / 64 slices, each dy slab by Cin / 64).  The other
//              order (the slices of a pixel share next to each other) was built, measured and dropped: no different
//              (profiles/wrw_wide_timing.json, rows `split_slices_adjacent`: within the repeats' spread on all twenty rows)
//   measured = 190 - 217 TF/s stand-alone at batch 64 where the library's fp32 kernels give 125 - 131, 26.8 ms for the ten layers in
//              the training step against the library's 48.5
//
// MFMA (template parameter MF, knob wrw_mfma): the split form on v_mfma_f32_16x16x32_bf16 (WRS_MF_16) beside v_mfma_f32_32x32x16_bf16
// (WRS_MF_32, the code above, instruction for instruction what it was).  Same wave tile (32 output x 32 input channels x 9 taps), same jobs,
// ring, borders, flush, partial results and order of the six products; per tap 2 x 2 blocks of 16 x 16, 36 f32x4 accumulators (the same
// 144 registers), one MFMA over the strip row's 32 pixels, 24 MFMAs of 16 cycles per (row, tap) = the 384 pipe cycles of two rounds above.
//   image    = planes [piece][16-channel quarter][35 pixels][16 channels], 32 B a pixel (wrs16_off), k permuted so that a 16-lane group
//              reads four consecutive pixels per transposing read (wrs16_kpix): reads and stores conflict-free, static_asserted there
//   limits   = 244 registers, no scratch, no spill, LDS 6 x 13440 = 80640 B (dynamic): two workgroups per CU (kernel-resource-usage)
//   measured = the same cycles (conv1_2: 7.79 M against 7.64 M, the matrix pipe 71 % busy either way) at a higher clock (1.69 against
//              1.55 GHz; conv4_2 1.79 against 1.66): every one of the twelve layers 1 - 4 % faster inside the training step at batch 64
//              and none slower at 16, 34.3 -> 33.1 ms per step for the twelve (profiles/wrw_mfma_step_layers.json), the step 108.9 ->
//              107.5 ms.  The rule behind the knob's default is therefore "always" (wrw_mfma16_wins).  The split and
//              the LDS stores moved in between the MFMAs (no serial tail) took 2.6 % of the cycles and gave most of it back in clock:
//              0.7 ms of the step, inside the bar - not kept
//
// Pooled (conv3x3_wrw_pooled_kernel, hk_conv3x3_wrw_pooled, knob wrw_pool): five of the twelve routed layers end in a 2 x 2 max-pool, and
// the dy that bias_relu_pool_bwd_kernel hands their weight gradient is three quarters zeros by construction: one value per window and
// channel, at the argmax.  Along a row every aligned group of four pixels is two window halves - at most two non-zeros, the first at
// position 0 or 1 and the second at 2 or 3: the 2:4 pattern of v_smfmac_f32_16x16x64_bf16 (hk_smfmac_bf16.h), which covers K = 64 in
// the time v_mfma_f32_16x16x32_bf16 covers 32.  The kernel takes the pooled gradient dp, the pooled output p (ReLU's mask) and the
// forward's argmax codes, never reads dy, and issues half the matrix instructions.
//   step     = one window row = two image rows; K = 64 is the strip's 32 pixels of row r, then of row r + 1 (wrp_krow, wrp_kpix), so
//              a B operand is the dense form's x fragments of two ring slots one after the other and a row's fragment serves two taps
//   dy       = per window row 16 windows x 64 channels of masked dp, split into the three pieces, and the codes as 16 bits a channel:
//              planes of [17 windows][16 channels] (wrp_aoff), 8704 B, ONE buffer - a lane's eight kept values are the eight windows
//              under its sixteen pixels (two transposing reads a plane), zeroed where the code's row bit is not the lane's row, at
//              position 2 (window % 2) + the code's column bit; fragments and index are formed once per step for its 216 MFMAs
//   ring     = FIVE x slots (67200 B): row r + 3 goes into the free slot half way through the step's MFMAs; row r + 4 and the next dy
//              behind a barrier after them: two barriers per two rows.  Row blocks start on even rows (wrw_plan, `even`)
//   limits   = LDS 75904 B (dynamic): two workgroups per CU.  The "no scratch, no spill" the dense kernels keep is MISSED (kernel-resource-usage):
//              wide 256 VGPRs, 16 bytes of scratch a lane, 3 VGPRs and 9 SGPRs spilled (the SGPRs into the lanes of v255); Cin 64 256 VGPRs, 12
//              bytes, 2 VGPRs, no SGPR.  The spill stores stand in front of the job loop, the reloads at the head of a job (no untracked load is
//              in flight there), none in the step loop.  Loads through a scalar base took it from 29 spilled VGPRs; five further attempts did
//              not improve it
//   measured = the sparse instruction issues in 0.95 x the dense one's time (profiles/wrw_pool_probe.json).  Inside the training step all five layers
//              0.65 - 0.68 x the dense kernel's time at batch 64 (16.07 -> 10.69 ms together) and 0.36 - 0.68 x at batch 16
//              (profiles/wrw_pool_step_layers.json); the step 98.99 -> 94.01 ms at batch 64, 27.03 -> 24.85 at 16
#include "hk_common.h"
#include "hk_partial_sum.h"
#include "hk_split_bf16.h"
#include <hk_mfma_bf16.h>   // the 16 x 16 x 32 bf16 MFMA (the emulation build finds its model of it first)
#include <hk_smfmac_bf16.h> // the 2:4 sparse 16 x 16 x 64 bf16 MFMA (likewise)
#include "../../include/hawkeye_hip.h"
#include "../../include/hawkeye_conv_pool.h"

namespace hk {

constexpr int WRW_CI = 64;                               // input channels per workgroup (all of them, or a 64-wide slice of Cin)
constexpr int WRW_OT = 64;                               // output channels per workgroup
constexpr int WRW_SW = 32;                               // strip width (pixels per row step)
constexpr int WRW_XROW = (WRW_SW + 2) * WRW_CI;          // floats of an x row segment (column halo on both sides)
constexpr int WRW_DYROW = WRW_SW * WRW_OT;               // floats of a dy row segment
constexpr int WRW_XF4 = WRW_XROW / 4;                    // 544 float4
constexpr int WRW_LDS = 4 * WRW_XROW + 2 * WRW_DYROW;    // 12800 floats = 50 KB
constexpr int WRW_MIN_ROWS = 4;                          // a row block is at least this high (each block re-reads two halo rows)
constexpr int WRW_MAX_WG = 512;                          // workgroups per Cout slice, at most (= partial results in the workspace)

// this thread's float4 loads of one row segment: where they come from (clamped into the tensor) and whether they count
struct WrwStage {
    long long xoff[3], doff[2];
    bool xok[3], dok[2];
};

// The loads are untracked (HK_LOAD16_ASYNC: they stay where they are written, in front of the step's MFMAs - left to the compiler,
// they end up behind the MFMAs, next to the LDS stores that use them), unconditional (clamped, in-bounds addresses), and waited for
// by wrw_loads_landed() behind the MFMAs; the zeros of the borders are put in on the way to LDS
// (cin = floats of an x pixel: the 64-channel slice that `xi` starts at is read out of wider pixels, as dy's is)
__device__ __forceinline__ bool wrw_load_x(const float* __restrict__ xi, const WrwStage& st, int r, int H, int W, int cin, f32x4 (&v)[3]) {
    const bool rok = r >= 0 && r < H;
    const float* row = xi + (long long)(r < 0 ? 0 : (r < H ? r : H - 1)) * W * cin;
#pragma unroll
    for (int u = 0; u < 3; ++u) HK_LOAD16_ASYNC(v[u], row + st.xoff[u]);
    return rok;
}
__device__ __forceinline__ void wrw_load_dy(const float* __restrict__ dyi, const WrwStage& st, int h, int H, int W, int Cout, f32x4 (&v)[2]) {
    const float* row = dyi + (long long)(h < H ? h : H - 1) * W * Cout;
#pragma unroll
    for (int u = 0; u < 2; ++u) HK_LOAD16_ASYNC(v[u], row + st.doff[u]);
}
__device__ __forceinline__ void wrw_loads_landed(f32x4 (&vx)[3], f32x4 (&vd)[2]) {
    __builtin_amdgcn_s_waitcnt(HK_VMCNT_IMM(0));
#pragma unroll
    for (int u = 0; u < 3; ++u) HK_PIN_LOADED(vx[u]);    // (no use of the registers moves in front of the wait)
#pragma unroll
    for (int u = 0; u < 2; ++u) HK_PIN_LOADED(vd[u]);
}
__device__ __forceinline__ void wrw_store_x(float* __restrict__ xs, int slot, const WrwStage& st, bool rok, const f32x4 (&v)[3]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4* d = reinterpret_cast<f32x4*>(xs + slot * WRW_XROW) + threadIdx.x;
    d[0] = (rok && st.xok[0]) ? v[0] : zero;
    d[256] = (rok && st.xok[1]) ? v[1] : zero;
    if (threadIdx.x + 512 < WRW_XF4) d[512] = (rok && st.xok[2]) ? v[2] : zero;
}
__device__ __forceinline__ void wrw_store_dy(float* __restrict__ ds, int buf, const WrwStage& st, const f32x4 (&v)[2]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4* d = reinterpret_cast<f32x4*>(ds + buf * WRW_DYROW) + threadIdx.x;
    d[0] = st.dok[0] ? v[0] : zero;
    d[256] = st.dok[1] ? v[1] : zero;
}

// dy [N][H][W][Cout], x [N][H][W][64] -> part [gridDim.x][Cout][9][64].  grid (workgroups per slice, Cout / 64).
// job j = ((n nrb + rb) nstrips + strip): rows [rb rpb, min(H, (rb + 1) rpb)), columns [32 strip, 32 strip + 32)
__global__ __launch_bounds__(256, 2) void conv3x3_wrw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          float* __restrict__ part, int H, int W, int Cout, int nstrips, int nrb,
                                                          int rpb, int njobs) {
    __shared__ __attribute__((aligned(16))) float lds[WRW_LDS];
    float* xs = lds;                                     // ring of four x row segments: [slot][34 pixels][64]
    float* ds = lds + 4 * WRW_XROW;                      // two dy row segments: [buf][32 pixels][64]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int oh = wave >> 1, ch = wave & 1;            // this wave's 32 output channels x 32 input channels, all nine taps
    const int slice = blockIdx.y;
    const int jb = (int)((long long)blockIdx.x * njobs / gridDim.x), je = (int)((long long)(blockIdx.x + 1) * njobs / gridDim.x);

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int aoff = hf * WRW_OT + oh * 32 + l31;        // + 64 (pixel of the strip): this lane's A value
    const int boff = hf * WRW_CI + ch * 32 + l31;        // + 64 (pixel of the strip + kw): this lane's B value

    for (int j = jb; j < je; ++j) {
        const int strip = j % nstrips, jr = j / nstrips;
        const int rb = jr % nrb;
        const long long n = jr / nrb;
        const int c0 = strip * WRW_SW, r0 = rb * rpb;
        const int nrows = (r0 + rpb < H ? r0 + rpb : H) - r0;
        const float* xi = x + n * H * W * WRW_CI;
        const float* dyi = dy + n * H * W * Cout + slice * WRW_OT;
        WrwStage st;
#pragma unroll
        for (int u = 0; u < 3; ++u) {                    // x: float4 idx of the segment -> pixel idx / 16 (column c0 - 1 + it), quad idx % 16
            const int idx = tid + 256 * u, col = c0 - 1 + (idx >> 4);
            st.xok[u] = idx < WRW_XF4 && col >= 0 && col < W;
            st.xoff[u] = (long long)(col < 0 ? 0 : (col < W ? col : W - 1)) * WRW_CI + 4 * (idx & 15);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {                    // dy: pixel idx / 16 (column c0 + it)
            const int idx = tid + 256 * u, col = c0 + (idx >> 4);
            st.dok[u] = col < W;
            st.doff[u] = (long long)(col < W ? col : W - 1) * Cout + 4 * (idx & 15);
        }
        // the first step's operands: x rows r0 - 1, r0, r0 + 1 into slots 0, 1, 2 and dy row r0 (the barrier that ended the
        // previous job's last step has every wave past its reads)
        f32x4 vx[3], vd[2];
        wrw_load_dy(dyi, st, r0, H, W, Cout, vd);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const bool rok = wrw_load_x(xi, st, r0 - 1 + t, H, W, WRW_CI, vx);
            wrw_loads_landed(vx, vd);
            wrw_store_x(xs, t, st, rok, vx);
        }
        wrw_store_dy(ds, 0, st, vd);
        __syncthreads();
        for (int k = 0; k < nrows; ++k) {                // output row r0 + k: x rows r0 + k - 1 .. + 1 are ring entries k, k + 1, k + 2
            // the next step's new segments: in flight while this step's MFMAs run.  (A job's last step loads and stores them for
            // nothing: ring entry and dy buffer are the ones the next job's first step does not use)
            const bool rok = wrw_load_x(xi, st, r0 + k + 2, H, W, WRW_CI, vx);
            wrw_load_dy(dyi, st, r0 + k + 1, H, W, Cout, vd);
            const float* A = ds + (k & 1) * WRW_DYROW + aoff;
            const float* B0 = xs + (k & 3) * WRW_XROW + boff;
            const float* B1 = xs + ((k + 1) & 3) * WRW_XROW + boff;
            const float* B2 = xs + ((k + 2) & 3) * WRW_XROW + boff;
            float a = *HK_LDS_CONST(A), b[9];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                b[kw] = *HK_LDS_CONST(B0 + kw * WRW_CI);
                b[3 + kw] = *HK_LDS_CONST(B1 + kw * WRW_CI);
                b[6 + kw] = *HK_LDS_CONST(B2 + kw * WRW_CI);
            }
#pragma unroll
            for (int p = 0; p < WRW_SW / 2; ++p) {       // pixel pair (2 p, 2 p + 1): the reads of pair p + 1 go out before the MFMAs of pair p
                float an = 0.f, bn[9];
                if (p + 1 < WRW_SW / 2) {
                    an = *HK_LDS_CONST(A + (2 * p + 2) * WRW_OT);
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        bn[kw] = *HK_LDS_CONST(B0 + (2 * p + 2 + kw) * WRW_CI);
                        bn[3 + kw] = *HK_LDS_CONST(B1 + (2 * p + 2 + kw) * WRW_CI);
                        bn[6 + kw] = *HK_LDS_CONST(B2 + (2 * p + 2 + kw) * WRW_CI);
                    }
                }
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], acc[t], 0, 0, 0);
                if (p + 1 < WRW_SW / 2) {
                    a = an;
#pragma unroll
                    for (int t = 0; t < 9; ++t) b[t] = bn[t];
                }
            }
            // ring entry k + 3 replaces entry k - 1, dy buffer (k + 1) & 1 row k - 1: last read a barrier ago
            wrw_loads_landed(vx, vd);
            wrw_store_x(xs, (k + 3) & 3, st, rok, vx);
            wrw_store_dy(ds, (k + 1) & 1, st, vd);
            __syncthreads();
        }
    }
    // C layout of the 32 x 32 MFMA: column = lane & 31 (input channel), row = 8 (i / 4) + 4 (lane >> 5) + i % 4 (output channel)
    float* pb = part + ((long long)blockIdx.x * Cout + slice * WRW_OT + oh * 32 + 4 * hf) * (9 * WRW_CI) + ch * 32 + l31;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) pb[(8 * (i >> 2) + (i & 3)) * (9 * WRW_CI) + t * WRW_CI] = acc[t][i];
}

// ---- the split form: the same walk on the bf16 matrix pipe (header: "Split form") ----
// (the split itself - wrs_split, wrs_widen, the bf16 vector types - is hk_split_bf16.h's: conv_fwd.hip uses it too)
constexpr int WRS_PIX = 32 * 2;                          // bytes of a pixel in a plane: 32 channels, bf16
constexpr int WRS_XPLANE = (WRW_SW + 2) * WRS_PIX;       // 2176 B: [34 pixels][32 channels] of one piece, one channel half
constexpr int WRS_DPLANE = WRW_SW * WRS_PIX;             // 2048 B
constexpr int WRS_XSLOT = 6 * WRS_XPLANE;                // [piece hi, mid, lo][channel half]: 13056 B
constexpr int WRS_DBUF = 6 * WRS_DPLANE;                 // 12288 B
constexpr int WRS_LDS = 4 * WRS_XSLOT + 2 * WRS_DBUF;    // 76800 B: two workgroups per CU in 160 KB
constexpr int WRS_FLUSH = 32;                            // row steps (1024 pixels) an accumulator chain runs before it is added to the partial

// float4 idx of a row segment (pixel idx / 16, channels 4 (idx % 16) ..+3) -> the three pieces, 8 bytes each, at
// [piece][channel half = (idx % 16) / 8][pixel][4 (idx % 8)] of the planes at `base` (piece = bytes from one piece to the next; WRS_MF_16:
// the image of wrs16_off, below)
__device__ __forceinline__ void wrs_store(char* base, int piece, f32x4 v) {
    bf16x4 p[3];
    wrs_split(v, p);
#pragma unroll
    for (int s = 0; s < 3; ++s) *reinterpret_cast<bf16x4*>(base + s * piece) = p[s];
}
__device__ __forceinline__ void wrs_store_x(char* xs, int slot, const WrwStage& st, bool rok, const f32x4 (&v)[3]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int tid = threadIdx.x;
    char* d = xs + slot * WRS_XSLOT + ((tid >> 3) & 1) * WRS_XPLANE + (tid >> 4) * WRS_PIX + (tid & 7) * 8;
    wrs_store(d, 2 * WRS_XPLANE, (rok && st.xok[0]) ? v[0] : zero);
    wrs_store(d + 16 * WRS_PIX, 2 * WRS_XPLANE, (rok && st.xok[1]) ? v[1] : zero);
    if (tid + 512 < WRW_XF4) wrs_store(d + 32 * WRS_PIX, 2 * WRS_XPLANE, (rok && st.xok[2]) ? v[2] : zero);
}
__device__ __forceinline__ void wrs_store_dy(char* ds, int buf, const WrwStage& st, const f32x4 (&v)[2]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int tid = threadIdx.x;
    char* d = ds + buf * WRS_DBUF + ((tid >> 3) & 1) * WRS_DPLANE + (tid >> 4) * WRS_PIX + (tid & 7) * 8;
    wrs_store(d, 2 * WRS_DPLANE, st.dok[0] ? v[0] : zero);
    wrs_store(d + 16 * WRS_PIX, 2 * WRS_DPLANE, st.dok[1] ? v[1] : zero);
}
// One operand fragment of v_mfma_f32_32x32x16_bf16: the eight pixels blk .. blk + 7 of this lane's channel.  `blk` = the plane's
// bytes at (first pixel + 8 (lane / 32), channel 16 ((lane / 16) % 2)): the 4 pixel x 16 channel block of the lane's 16-lane group;
// i = lane % 16.  On the device two transposing reads - lane 4 q + p of a group gives the address of pixel q, channels 4 p ..+3 and
// gets the four pixels of channel i -, elsewhere the same eight values one by one.
__device__ __forceinline__ bf16x8 wrs_frag(const char* blk, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) bf16x4* lds_b64;
    const char* a = blk + (i >> 2) * WRS_PIX + (i & 3) * 8;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)a);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)(a + 4 * WRS_PIX));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#else
    bf16x8 f;
    for (int q = 0; q < 8; ++q) {
        __bf16 e;
        __builtin_memcpy(&e, blk + q * WRS_PIX + i * 2, 2);
        f[q] = e;
    }
    return f;
#endif
}

// part (+)= acc; acc = 0.  The first time a plain store: the workspace is not zero-filled.  cin = floats of a tap in a row of the
// partial (a row = one output channel: 9 cin floats)
__device__ __forceinline__ void wrs_flush(float* __restrict__ pb, f32x16 (&acc)[9], bool add, int cin) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int o = t * cin;
        HK_PIN_LOADED(o);                                // (the addresses are made here: hoisted out of the row loop they are 288 registers;
        float* q = pb + o;                               //  the pointer itself stays a global one - a flat access makes every LDS wait a full one)
        f32x16 v = acc[t];
        if (add) {
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] += q[(8 * (i >> 2) + (i & 3)) * (9 * cin)];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            q[(8 * (i >> 2) + (i & 3)) * (9 * cin)] = v[i];
            acc[t][i] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);               // one tap at a time: sixteen loads in flight, not 144
    }
}

// ---- MF, the bf16 MFMA the split form runs on (knob wrw_mfma; header: "MFMA") ----
// WRS_MF_32 = v_mfma_f32_32x32x16_bf16 on the planes above, WRS_MF_16 = v_mfma_f32_16x16x32_bf16 on the image below.
constexpr int WRS_MF_32 = 0, WRS_MF_16 = 1;
constexpr int WRS16_PIX = 16 * 2;                        // bytes of a pixel in a plane: 16 channels, bf16
constexpr int WRS16_PITCH = WRW_SW + 3;                  // pixels of a plane: the 34 of an x row segment + 1 (dy uses 32), "banks" below
constexpr int WRS16_QPLANE = WRS16_PITCH * WRS16_PIX;    // 1120 B: [35 pixels][16 channels] of one piece, one 16-channel quarter
constexpr int WRS16_PIECE = 4 * WRS16_QPLANE;            // 4480 B
constexpr int WRS16_SLOT = 3 * WRS16_PIECE;              // 13440 B: an x ring slot and a dy buffer alike
constexpr int WRS16_LDS = 6 * WRS16_SLOT;                // 80640 B: two workgroups per CU in 160 KB

// THE image of a WRS_MF_16 row segment, for the staging stores, the fragment reads and the host twin of the reads: byte offset of
// channel `ch` (0 .. 15) of quarter `quarter` at pixel `pixel` in piece `piece`
__host__ __device__ constexpr int wrs16_off(int piece, int quarter, int pixel, int ch) {
    return piece * WRS16_PIECE + quarter * WRS16_QPLANE + pixel * WRS16_PIX + ch * 2;
}
// THE order of the GEMM's k inside a 16 x 16 x 32 MFMA: element e (0 .. 7) of the fragment of 16-lane group g is this pixel of the
// strip row (+ kw for x).  The instruction sums over all 32, and dy and x use the same order, so any permutation serves; this one
// gives a group four consecutive pixels per transposing read and a 32-lane half eight: 256 contiguous bytes of one plane
__host__ __device__ constexpr int wrs16_kpix(int g, int e) { return 16 * (e >> 2) + 4 * g + (e & 3); }
//   banks    = ds_read_b64_tr_b16 is serviced in two halves of 32 lanes, bank = (a / 4) % 64: a half's two groups read pixels
//              8 h ..+7 (+ 16 in the second read, + kw) of one quarter plane, 256 contiguous bytes from a multiple of 32 - every bank
//              once, at any kw and any plane pitch.  ds_write_b64 is serviced in four groups of 16 lanes, bank = (a / 4) % 32: a
//              group's lanes store one pixel's four quarters, 32 bytes each; with 35 pixels (280 dwords) to a plane the quarters
//              start 24 banks apart - 0, 24, 16, 8 - and the group covers the 32 banks once (with 34 pixels quarters 0 and 2
//              would meet: 2-way, what the WRS_MF_32 image's stores have always had).  Both static_asserted:
constexpr bool wrs16_reads_conflict_free() {
    for (int piece = 0; piece < 3; ++piece)
        for (int quarter = 0; quarter < 4; ++quarter)
            for (int kw = 0; kw < 3; ++kw)
                for (int rd = 0; rd < 2; ++rd)
                    for (int half = 0; half < 2; ++half) {
                        unsigned long long seen = 0;
                        for (int l = 32 * half; l < 32 * half + 32; ++l) {
                            const int g = l >> 4, i = l & 15;
                            const int a = wrs16_off(piece, quarter, kw + wrs16_kpix(g, 4 * rd) + (i >> 2), 4 * (i & 3));
                            if (a % 8 != 0 || kw + wrs16_kpix(g, 4 * rd + 3) >= WRS16_PITCH) return false;
                            for (int d = 0; d < 2; ++d) {
                                const int bank = (a / 4 + d) % 64;
                                if ((seen >> bank) & 1ull) return false;
                                seen |= 1ull << bank;
                            }
                        }
                    }
    return true;
}
constexpr bool wrs16_stores_conflict_free() {
    for (int u = 0; u < 3; ++u)                          // a thread's float4 idx = tid + 256 u of a row segment: pixel idx / 16, quarter (idx / 4) % 4
        for (int grp = 0; grp < 16; ++grp) {
            unsigned seen = 0;
            for (int tid = 16 * grp; tid < 16 * grp + 16; ++tid) {
                const int a = wrs16_off(0, (tid >> 2) & 3, (tid >> 4) + 16 * u, 4 * (tid & 3));
                for (int d = 0; d < 2; ++d) {
                    const int bank = (a / 4 + d) % 32;
                    if ((seen >> bank) & 1u) return false;
                    seen |= 1u << bank;
                }
            }
        }
    return true;
}
constexpr bool wrs16_k_is_a_permutation() {
    unsigned seen = 0;
    for (int g = 0; g < 4; ++g)
        for (int e = 0; e < 8; ++e) seen |= 1u << wrs16_kpix(g, e);
    return seen == 0xffffffffu;
}
static_assert(wrs16_reads_conflict_free(), "both 32-lane halves of both transposing reads of a WRS_MF_16 fragment cover the 64 banks once, at every kw");
static_assert(wrs16_stores_conflict_free(), "every 16-lane group of a WRS_MF_16 staging store covers the 32 banks once");
static_assert(wrs16_k_is_a_permutation(), "the four groups' fragments hold the strip row's 32 pixels once each");
static_assert(2 * WRS16_LDS <= 160 * 1024 && WRS16_PITCH >= WRW_SW + 2, "two workgroups per CU; a plane holds an x row segment");

// the staging stores of the WRS_MF_16 image: a thread's float4 (pixel tid / 16 + 16 u, channels 4 (tid % 16) ..+3) -> three 8-byte pieces
__device__ __forceinline__ void wrs16_store_x(char* xs, int slot, const WrwStage& st, bool rok, const f32x4 (&v)[3]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int tid = threadIdx.x;
    char* d = xs + slot * WRS16_SLOT + wrs16_off(0, (tid >> 2) & 3, tid >> 4, 4 * (tid & 3));
    wrs_store(d, WRS16_PIECE, (rok && st.xok[0]) ? v[0] : zero);
    wrs_store(d + 16 * WRS16_PIX, WRS16_PIECE, (rok && st.xok[1]) ? v[1] : zero);
    if (tid + 512 < WRW_XF4) wrs_store(d + 32 * WRS16_PIX, WRS16_PIECE, (rok && st.xok[2]) ? v[2] : zero);
}
__device__ __forceinline__ void wrs16_store_dy(char* ds, int buf, const WrwStage& st, const f32x4 (&v)[2]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int tid = threadIdx.x;
    char* d = ds + buf * WRS16_SLOT + wrs16_off(0, (tid >> 2) & 3, tid >> 4, 4 * (tid & 3));
    wrs_store(d, WRS16_PIECE, st.dok[0] ? v[0] : zero);
    wrs_store(d + 16 * WRS16_PIX, WRS16_PIECE, st.dok[1] ? v[1] : zero);
}
// One operand fragment of v_mfma_f32_16x16x32_bf16: the eight pixels wrs16_kpix(g, 0 .. 7) of channel i of a quarter plane.  `blk` =
// the plane's bytes at the strip row's first pixel (+ kw for x); g = lane / 16, i = lane % 16.  On the device two transposing reads,
// as wrs_frag; elsewhere the same eight values one by one.
__device__ __forceinline__ bf16x8 wrs16_frag(const char* blk, int g, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) bf16x4* lds_b64;
    const char* a = blk + wrs16_off(0, 0, wrs16_kpix(g, 0) + (i >> 2), 4 * (i & 3));
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)a);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)(a + (wrs16_kpix(0, 4) - wrs16_kpix(0, 0)) * WRS16_PIX));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#else
    bf16x8 f;
    for (int e = 0; e < 8; ++e) {
        __bf16 v;
        __builtin_memcpy(&v, blk + wrs16_off(0, 0, wrs16_kpix(g, e), i), 2);
        f[e] = v;
    }
    return f;
#endif
}
// wrs_flush for the accumulators of WRS_MF_16, [tap][block of 16 output channels][block of 16 input channels].  C layout of the
// 16 x 16 MFMA: column = lane % 16 (input channel), rows 4 (lane / 16) + e (output channel); pb = the lane's element of the first blocks
__device__ __forceinline__ void wrs16_flush(float* __restrict__ pb, f32x4 (&acc)[9][2][2], bool add, int cin) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int o = t * cin;
        HK_PIN_LOADED(o);                                // (as in wrs_flush)
        float* q = pb + o;
        f32x4 v[2][2];
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                v[ob][cb] = acc[t][ob][cb];
                if (add) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[ob][cb][e] += q[(16 * ob + e) * (9 * cin) + 16 * cb];
                }
            }
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    q[(16 * ob + e) * (9 * cin) + 16 * cb] = v[ob][cb][e];
                    acc[t][ob][cb][e] = 0.f;
                }
        __builtin_amdgcn_sched_barrier(0);               // one tap at a time: sixteen loads in flight, not 144
    }
}

// As conv3x3_wrw_kernel (same grid, jobs, ring, borders, result), with dynamic LDS of WRS_LDS bytes.  WIDE: x [N][H][W][Cin] with
// Cin a multiple of 64; a workgroup owns the 64 x 9 x 64 block (Cout slice blockIdx.y, Cin slice blockIdx.z) of dW and reads its 64
// input channels out of the Cin-wide pixels, part [gridDim.x][Cout][9][Cin].  Not WIDE: Cin = 64, as it was.
// MF = WRS_MF_16 (dynamic LDS WRS16_LDS): the wave's 32 x 32 x 9 tile as 2 x 2 blocks of 16 x 16 per tap (36 f32x4, the same 144
// registers); one MFMA sums over the strip row's 32 pixels, a (row, tap) is 4 blocks x 6 products = 24 MFMAs of 16 cycles.  The six
// dy fragments (2 blocks x 3 pieces) are read once per row step and serve all nine taps; the x fragments of a 16-channel block
// (3 pieces) serve 12 MFMAs, and those of the next (tap, block) are read in front of them.  Same jobs, ring, borders, flush and
// order of the six products; the two output blocks' chains alternate, so no MFMA waits for the one before it.
template <bool WIDE, int MF>
__global__ __launch_bounds__(256, 2) void conv3x3_wrw_split_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                float* __restrict__ part, int H, int W, int Cout, int nstrips,
                                                                int nrb, int rpb, int njobs, int Cin) {
    constexpr bool M32 = MF == WRS_MF_32;
    HK_DYN_LDS16(ldsf);
    char* xs = reinterpret_cast<char*>(ldsf);            // ring of four x row segments: [slot][piece][channel half][34 pixels][32]
    char* ds = xs + 4 * (M32 ? WRS_XSLOT : WRS16_SLOT);  // two dy row segments: [buf][piece][channel half][32 pixels][32]  (WRS_MF_16: wrs16_off)
    const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5, l15 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int oh = wave >> 1, ch = wave & 1;            // this wave's 32 output channels x 32 input channels, all nine taps
    const int cin = WIDE ? Cin : WRW_CI;                 // floats of an x pixel
    const int slice = blockIdx.y, cslice = WIDE ? blockIdx.z : 0;
    const int jb = (int)((long long)blockIdx.x * njobs / gridDim.x), je = (int)((long long)(blockIdx.x + 1) * njobs / gridDim.x);

    f32x16 acc[9];                                       // WRS_MF_32: [tap]
    f32x4 acc4[9][2][2];                                 // WRS_MF_16: [tap][block of 16 output channels][block of 16 input channels]
    if constexpr (M32) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    } else {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc4[t][q >> 1][q & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    const int blk = 8 * hf * WRS_PIX + ((lane >> 4) & 1) * 32;      // this lane's group block inside a plane, first pixel 0
    // (WRS_MF_16: the wave's first dy and x quarter planes; the lane's part of the address is wrs16_frag's)
    const int aoff = M32 ? oh * WRS_DPLANE + blk : wrs16_off(0, 2 * oh, 0, 0), boff = M32 ? ch * WRS_XPLANE + blk : wrs16_off(0, 2 * ch, 0, 0);
    // this wave's part of the workgroup's partial result (C layout of the 32 x 32 MFMA, as in conv3x3_wrw_kernel; WRS_MF_16: at
    // wrs16_flush).  Every WRS_FLUSH row steps the accumulators are added to it with ordinary fp32 additions and start again from
    // zero (header: "chains")
    auto mine = [&]() {                                  // (made anew at every flush: not two more registers through the row loop)
        const int l = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
        if constexpr (M32)
            return part + ((long long)blockIdx.x * Cout + slice * WRW_OT + (w >> 1) * 32 + 4 * (l >> 5)) * (9 * cin) + cslice * WRW_CI + (w & 1) * 32 + (l & 31);
        else
            return part + ((long long)blockIdx.x * Cout + slice * WRW_OT + (w >> 1) * 32 + 4 * (l >> 4)) * (9 * cin) + cslice * WRW_CI + (w & 1) * 32 + (l & 15);
    };
    int since = 0;
    bool stored = false;

    for (int j = jb; j < je; ++j) {
        const int strip = j % nstrips, jr = j / nstrips;
        const int rb = jr % nrb;
        const long long n = jr / nrb;
        const int c0 = strip * WRW_SW, r0 = rb * rpb;
        const int nrows = (r0 + rpb < H ? r0 + rpb : H) - r0;
        const float* xi = x + n * H * W * cin + cslice * WRW_CI;
        const float* dyi = dy + n * H * W * Cout + slice * WRW_OT;
        WrwStage st;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int idx = tid + 256 * u, col = c0 - 1 + (idx >> 4);
            st.xok[u] = idx < WRW_XF4 && col >= 0 && col < W;
            st.xoff[u] = (long long)(col < 0 ? 0 : (col < W ? col : W - 1)) * cin + 4 * (idx & 15);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, col = c0 + (idx >> 4);
            st.dok[u] = col < W;
            st.doff[u] = (long long)(col < W ? col : W - 1) * Cout + 4 * (idx & 15);
        }
        f32x4 vx[3], vd[2];
        wrw_load_dy(dyi, st, r0, H, W, Cout, vd);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const bool rok = wrw_load_x(xi, st, r0 - 1 + t, H, W, cin, vx);
            wrw_loads_landed(vx, vd);
            if constexpr (M32) wrs_store_x(xs, t, st, rok, vx);
            else wrs16_store_x(xs, t, st, rok, vx);
        }
        if constexpr (M32) wrs_store_dy(ds, 0, st, vd);
        else wrs16_store_dy(ds, 0, st, vd);
        __syncthreads();
        for (int k = 0; k < nrows; ++k) {
            const bool rok = wrw_load_x(xi, st, r0 + k + 2, H, W, cin, vx);
            wrw_load_dy(dyi, st, r0 + k + 1, H, W, Cout, vd);
            constexpr int DBUF = M32 ? WRS_DBUF : WRS16_SLOT, XSLOT = M32 ? WRS_XSLOT : WRS16_SLOT;
            const char* A = ds + (k & 1) * DBUF + aoff;
            const char* B[3] = {xs + (k & 3) * XSLOT + boff, xs + ((k + 1) & 3) * XSLOT + boff, xs + ((k + 2) & 3) * XSLOT + boff};
            if constexpr (!M32) {
                // 18 rounds of twelve MFMAs: (tap, block of 16 input channels); the x fragments of round i + 1 are read before the
                // MFMAs of round i.  The first reads in the order of their use: dy mid, x mid, dy hi, x lo, dy lo, x hi
                const int g = lane >> 4;
                constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
                bf16x8 a[2][3], b[3];
#pragma unroll
                for (int pr = 0; pr < 3; ++pr) {
#pragma unroll
                    for (int ob = 0; ob < 2; ++ob) a[ob][PA[pr]] = wrs16_frag(A + wrs16_off(PA[pr], ob, 0, 0), g, l15);
                    b[PB[pr]] = wrs16_frag(B[0] + wrs16_off(PB[pr], 0, 0, 0), g, l15);
                }
#pragma unroll
                for (int i = 0; i < 18; ++i) {
                    const int t = i / 2, cb = i % 2, tn = (i + 1) / 2, cbn = (i + 1) % 2;
                    bf16x8 bn[3];
                    if (i + 1 < 18) {
#pragma unroll
                        for (int s = 0; s < 3; ++s) bn[s] = wrs16_frag(B[tn / 3] + wrs16_off(s, cbn, tn % 3, 0), g, l15);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // (as below)
                    // the same six products in the same order, each into both output blocks before the next
#pragma unroll
                    for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                        for (int ob = 0; ob < 2; ++ob) acc4[t][ob][cb] = mfma_f32_16x16x32_bf16(a[ob][PA[pr]], b[PB[pr]], acc4[t][ob][cb]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (i + 1 < 18) {
#pragma unroll
                        for (int s = 0; s < 3; ++s) b[s] = bn[s];
                    }
                }
            } else {
                // 18 rounds of six MFMAs: (16-pixel chunk of the row, tap); the fragments of round i + 1 are read before the MFMAs of round i
                bf16x8 a[3], b[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    a[s] = wrs_frag(A + 2 * s * WRS_DPLANE, l15);
                    b[s] = wrs_frag(B[0] + 2 * s * WRS_XPLANE, l15);
                }
#pragma unroll
                for (int i = 0; i < 18; ++i) {
                    const int t = i % 9, cn = (i + 1) / 9, tn = (i + 1) % 9;
                    bf16x8 an[3], bn[3];
                    if (i + 1 < 18) {
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            bn[s] = wrs_frag(B[tn / 3] + 2 * s * WRS_XPLANE + (16 * cn + tn % 3) * WRS_PIX, l15);
                            if (tn == 0) an[s] = wrs_frag(A + 2 * s * WRS_DPLANE + 16 * cn * WRS_PIX, l15);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);       // (left alone, the scheduler sinks each read to the MFMA that needs it)
                    // the six products of first and second order, small ones first (they meet a running sum either way: the order
                    // costs nothing and matters only in a chain's first steps)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc[t], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (i + 1 < 18) {
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            b[s] = bn[s];
                            if (tn == 0) a[s] = an[s];
                        }
                    }
                }
            }
            wrw_loads_landed(vx, vd);
            if constexpr (M32) {
                wrs_store_x(xs, (k + 3) & 3, st, rok, vx);
                wrs_store_dy(ds, (k + 1) & 1, st, vd);
            } else {
                wrs16_store_x(xs, (k + 3) & 3, st, rok, vx);
                wrs16_store_dy(ds, (k + 1) & 1, st, vd);
            }
            __syncthreads();
            if (++since == WRS_FLUSH) {                  // (no load of the next step is in flight yet; each wave owns its part)
                if constexpr (M32) wrs_flush(mine(), acc, stored, cin);
                else wrs16_flush(mine(), acc4, stored, cin);
                since = 0;
                stored = true;
            }
        }
    }
    if (since > 0 || !stored) {
        if constexpr (M32) wrs_flush(mine(), acc, stored, cin);
        else wrs16_flush(mine(), acc4, stored, cin);
    }
}

// Which calls the split form serves by default (knob wrw_split at -1): the layers where it beat the fp32 form by more than three
// times the spread of the fp32 form's own repeats (profiles/wrw_split_timing.json), and nothing that was not measured.
// Two Cout slices: cleared at 3.2 M pixels (conv2_1, batch 64) and at 0.8 M (batch 16).  One slice: cleared at 12.8 M pixels
// (conv1_2, batch 64), missed at 3.2 M (batch 16: 0.72 ms faster against a bar of 0.75) - the line is drawn half way
static bool wrw_split_wins(int N, int H, int W, int Cout) {
    const long long pixels = (long long)N * H * W;
    return Cout >= 2 * WRW_OT ? pixels >= 16ll * 224 * 224 : pixels >= 32ll * 448 * 448;
}

// Which calls of the split form run on the 16 x 16 x 32 MFMA by default (knob wrw_mfma at -1).  A rule in N, H, W and Cout only: a
// wide call and the 64-channel call over the same map get the same shape (the tests compare them bit for bit).  Decided by the layers'
// times inside the training step (profiles/wrw_mfma_step_layers.json: HK_WRW_MFMA=1 against =0 on this build and against the build
// before): all twelve layers faster at batch 64 (0.02 - 0.38 ms each), none slower at batch 16 beyond the traces' spread - always.
// WRS_MF_32 stays reachable through the knob (tests: held to the bits of the commit before).
static bool wrw_mfma16_wins(int N, int H, int W, int Cout) {
    (void)N; (void)H; (void)W; (void)Cout;
    return true;
}

// The split of a problem into jobs and workgroups: the row-block height whose heaviest workgroup has the fewest row steps
// (a block costs its rows + the two rows that prime the ring), the lowest block count among equals
struct WrwPlan {
    int nstrips, nrb, rpb, njobs, nwg;
};
// Workgroups per slice that the workspace of a wide call (Cin > 64; slice = a 64 x 64 block of (Cout, Cin)) has room for: two
// workgroups per CU over all slices
static int wrw_wide_wgs(long long slices) { return slices < 512 ? (int)(512 / slices) : 1; }

// (even: row blocks start on even rows - the pooled form's two-row steps, "Pooled" below; H is even there)
static bool wrw_plan(int N, int H, int W, int slices, bool wide, WrwPlan& pl, bool even = false) {
    // two workgroups per CU over all slices (two waves per SIMD cover each other's LDS waits: conv1_2 6.54 ms against 6.72 with one)
    const int room = wide ? wrw_wide_wgs(slices) : WRW_MAX_WG;
    int wgmax = tuning().wrw_wgs > 0 ? tuning().wrw_wgs : (wide ? room : (slices <= 8 ? 512 / slices : 64));
    if (wgmax > room) wgmax = room;
    const long long nstrips = ((long long)W + WRW_SW - 1) / WRW_SW, base = (long long)N * nstrips;
    long long best = -1;
    for (int cand = 1; cand <= (H / WRW_MIN_ROWS > 1 ? H / WRW_MIN_ROWS : 1); ++cand) {
        const int rpb = (H + cand - 1) / cand + (even ? ((H + cand - 1) / cand) & 1 : 0), nrb = (H + rpb - 1) / rpb;
        if (nrb != cand) continue;
        const long long jobs = base * nrb;
        if (jobs > 0x7fffffffll) break;
        const long long wg = jobs < wgmax ? jobs : wgmax;
        const long long cost = ((jobs + wg - 1) / wg) * (rpb + 2);
        if (best < 0 || cost < best) {
            best = cost;
            pl.nstrips = (int)nstrips; pl.nrb = nrb; pl.rpb = rpb; pl.njobs = (int)jobs; pl.nwg = (int)wg;
        }
    }
    return best >= 0;
}

// one instantiation of the split form with its own LDS size (cin = Cin of a wide call, 64 otherwise)
template <bool WIDE, int MF>
static int wrw_split_launch(dim3 grid, const float* dy, const float* x, float* part, int H, int W, int Cout, const WrwPlan& pl, int cin,
                            hk_stream_t stream) {
    constexpr int LDS = MF == WRS_MF_32 ? WRS_LDS : WRS16_LDS;
    HK_ALLOW_BIG_LDS((conv3x3_wrw_split_kernel<WIDE, MF>), LDS);
    hipLaunchKernelGGL((conv3x3_wrw_split_kernel<WIDE, MF>), grid, dim3(256), LDS, (hipStream_t)stream, dy, x, part, H, W, Cout, pl.nstrips,
                       pl.nrb, pl.rpb, pl.njobs, cin);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

// ---- Pooled: the weight gradient of a layer that ends in a 2 x 2 max-pool, on the 2:4 sparse MFMA (header: "Pooled") ----
constexpr int WRP_SLOTS = 5;                             // x ring: the four rows a two-row step reads + the one that comes in meanwhile
constexpr int WRP_WPITCH = WRW_SW / 2 + 1;               // windows of a dy plane: the strip's 16 + 1 ("banks" below)
constexpr int WRP_QPLANE = WRP_WPITCH * WRS16_PIX;       // 544 B: [17 windows][16 channels] of one piece, one 16-channel quarter
constexpr int WRP_PLANE = 4 * WRP_QPLANE;                // 2176 B
constexpr int WRP_ABUF = 4 * WRP_PLANE;                  // 8704 B: hi, mid, lo and the argmax codes (16 bits a channel), one window row
constexpr int WRP_LDS = WRP_SLOTS * WRS16_SLOT + WRP_ABUF;   // 75904 B: two workgroups per CU in 160 KB
constexpr int WRP_FLUSH = WRS_FLUSH / 2;                 // two-row steps a chain runs: the same 1024 pixels

// THE image of a window row of dy: byte offset of channel `ch` (0 .. 15) of quarter `quarter` at window `window` of plane `plane`
// (0 .. 2 the pieces, 3 the codes)
__host__ __device__ constexpr int wrp_aoff(int plane, int quarter, int window, int ch) {
    return plane * WRP_PLANE + quarter * WRP_QPLANE + window * WRS16_PIX + ch * 2;
}
// THE order of the GEMM's 64 k inside a sparse MFMA: k < 32 is the strip's row r, k >= 32 its row r + 1, and within a row the pixel is
// the dense form's (a B operand is two of its fragments, hk_smfmac_bf16.h): aligned runs of four k are aligned runs of four pixels -
// two windows, so a group of four of dy holds at most two non-zeros, the first at position 0 or 1 and the second at 2 or 3
__host__ __device__ constexpr int wrp_krow(int k) { return k >> 5; }
__host__ __device__ constexpr int wrp_kpix(int k) { return wrs16_kpix((k & 31) >> 3, k & 7); }
// the window (0 .. 15) under value j of the A operand of a lane of group g: the lane's two transposing reads fetch windows
// 4 (g % 2) ..+3 and 8 + 4 (g % 2) ..+3, and the dwords are taken in the order 0, 2, 1, 3
__host__ __device__ constexpr int wrp_awin(int g, int j) { return 4 * (g & 1) + 8 * ((j >> 1) & 1) + 2 * (j >> 2) + (j & 1); }
//   banks    = a 32-lane half of a transposing read of dy covers windows 0 .. 7 or 8 .. 15 of one quarter plane: 256 contiguous bytes
//              from a multiple of 32, every bank once.  The 8-byte stores of a 16-lane group are one window's four quarters, 32 bytes
//              each: with 17 windows (136 dwords) to a plane they start 8 banks apart.  Both static_asserted, with the k order:
constexpr bool wrp_k_is_a_permutation() {
    unsigned long long seen = 0;
    for (int g = 0; g < 4; ++g)
        for (int e = 0; e < 16; ++e) {
            const int k = smfmac_b_k(g, e);
            seen |= 1ull << (32 * wrp_krow(k) + wrp_kpix(k));
        }
    return seen == ~0ull;
}
constexpr bool wrp_groups_are_window_pairs() {
    for (int k = 0; k < 64; k += 4)
        for (int d = 0; d < 4; ++d)
            if (wrp_kpix(k) % 4 != 0 || wrp_kpix(k + d) != wrp_kpix(k) + d || wrp_krow(k + d) != wrp_krow(k)) return false;
    for (int g = 0; g < 4; ++g)                          // ... and value j of the A operand is the window wrp_awin says
        for (int j = 0; j < 8; ++j)
            if (wrp_kpix(smfmac_a_k4(g, j) + 2 * (j & 1)) / 2 != wrp_awin(g, j) || wrp_krow(smfmac_a_k4(g, j)) != g >> 1) return false;
    return true;
}
constexpr bool wrp_a_reads_conflict_free() {
    for (int plane = 0; plane < 4; ++plane)
        for (int quarter = 0; quarter < 4; ++quarter)
            for (int rd = 0; rd < 2; ++rd)
                for (int half = 0; half < 2; ++half) {
                    unsigned long long seen = 0;
                    for (int l = 32 * half; l < 32 * half + 32; ++l) {
                        const int g = l >> 4, i = l & 15;
                        const int a = wrp_aoff(plane, quarter, 4 * (g & 1) + 8 * rd + (i >> 2), 4 * (i & 3));
                        if (a % 8 != 0) return false;
                        for (int d = 0; d < 2; ++d) {
                            const int bank = (a / 4 + d) % 64;
                            if ((seen >> bank) & 1ull) return false;
                            seen |= 1ull << bank;
                        }
                    }
                }
    return true;
}
constexpr bool wrp_a_stores_conflict_free() {
    for (int grp = 0; grp < 16; ++grp) {                 // a thread's float4: window tid / 16, quarter (tid / 4) % 4
        unsigned seen = 0;
        for (int tid = 16 * grp; tid < 16 * grp + 16; ++tid) {
            const int a = wrp_aoff(0, (tid >> 2) & 3, tid >> 4, 4 * (tid & 3));
            for (int d = 0; d < 2; ++d) {
                const int bank = (a / 4 + d) % 32;
                if ((seen >> bank) & 1u) return false;
                seen |= 1u << bank;
            }
        }
    }
    return true;
}
static_assert(wrp_k_is_a_permutation(), "the four groups' B operands hold the 32 pixels of both rows once each");
static_assert(wrp_groups_are_window_pairs(), "an aligned group of four k is two whole windows of one row");
static_assert(wrp_a_reads_conflict_free(), "both 32-lane halves of both transposing reads of a pooled dy fragment cover the 64 banks once");
static_assert(wrp_a_stores_conflict_free(), "every 16-lane group of a pooled dy staging store covers the 32 banks once");
static_assert(2 * WRP_LDS <= 160 * 1024, "two workgroups per CU");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// the eight 16-bit values of plane `pl` (its bytes at the lane's quarter) under this lane's eight kept positions, as four dwords in
// value order.  On the device two transposing reads, elsewhere the same values one by one.
__device__ __forceinline__ u32x4 wrp_read(const char* pl, int g, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) bf16x4* lds_b64;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const char* a = pl + wrp_aoff(0, 0, 4 * (g & 1) + (i >> 2), 4 * (i & 3));
    const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)a));
    const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64)(a + 8 * WRS16_PIX)));
    return (u32x4){lo[0], hi[0], lo[1], hi[1]};
#else
    unsigned short v[8];
    for (int j = 0; j < 8; ++j) __builtin_memcpy(&v[j], pl + wrp_aoff(0, 0, wrp_awin(g, j), i), 2);
    u32x4 r;
    for (int q = 0; q < 4; ++q) r[q] = (unsigned)v[2 * q] | ((unsigned)v[2 * q + 1] << 16);
    return r;
#endif
}
// One A operand: the three pieces of the eight windows under this lane's sixteen pixels, for output channel i of the quarter at `ab`,
// and their positions.  A window's value is kept where its code's row bit is the lane's row (g / 2), else it is a zero; its position is
// 2 (window % 2) + the code's column bit.
__device__ __forceinline__ void wrp_afrag(const char* ab, int g, int i, bf16x8 (&a)[3], int& idx) {
    const u32x4 c = wrp_read(ab + wrp_aoff(3, 0, 0, 0), g, i);
    const u32x4 keep = (((c >> 1) & 0x00010001u) ^ ((g >> 1) ? 0u : 0x00010001u)) * 0xffffu;
#pragma unroll
    for (int s = 0; s < 3; ++s) a[s] = __builtin_bit_cast(bf16x8, wrp_read(ab + wrp_aoff(s, 0, 0, 0), g, i) & keep);
    const u32x4 nib = 8u | (c & 1u) | ((c >> 14) & 4u);
    idx = (int)(nib[0] | (nib[1] << 4) | (nib[2] << 8) | (nib[3] << 12));
}
// HK_LOAD16_ASYNC / HK_LOAD4_ASYNC from a wave-uniform base (scalar registers) and a 32-bit byte offset per lane: the row's address is
// made once per wave, and no thread carries six 64-bit row pointers through the MFMAs (they were the kernel's spills)
#if defined(__HIP_DEVICE_COMPILE__)
#define WRP_LOAD16(dst, base, off) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(off), "s"(base) : "memory")
#define WRP_LOAD4(dst, base, off) asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(off), "s"(base) : "memory")
#else
#define WRP_LOAD16(dst, base, off) __builtin_memcpy(&(dst), reinterpret_cast<const char*>(base) + (off), 16)
#define WRP_LOAD4(dst, base, off) __builtin_memcpy(&(dst), reinterpret_cast<const char*>(base) + (off), 4)
#endif
// this thread's loads of a window row of dy: window tid / 16 of the strip, channels 4 (tid % 16) ..+3
struct WrpStage {
    int doff, coff;                                      // bytes into dp / p and into the codes (a dword's), from the window row's start
    int xoff[3];                                         // bytes into x from the row's start (WrwStage's, in 32 bits: a row is below 2^31)
    bool dok;
};
__device__ __forceinline__ bool wrp_load_x(const float* __restrict__ xi, const WrpStage& sa, int r, int H, int W, int cin, f32x4 (&v)[3]) {
    const bool rok = r >= 0 && r < H;
    const float* row = xi + (long long)(r < 0 ? 0 : (r < H ? r : H - 1)) * W * cin;
#pragma unroll
    for (int u = 0; u < 3; ++u) WRP_LOAD16(v[u], row, sa.xoff[u]);
    return rok;
}
__device__ __forceinline__ void wrp_load_a(const float* __restrict__ dpi, const float* __restrict__ pi, const uint8_t* __restrict__ ami,
                                           const WrpStage& sa, int ho, int Ho, int Wo, int Cout, f32x4& vd, f32x4& vp, unsigned& vc) {
    const long long row = (long long)(ho < Ho ? ho : Ho - 1) * Wo;
    WRP_LOAD16(vd, dpi + row * Cout, sa.doff);
    WRP_LOAD16(vp, pi + row * Cout, sa.doff);
    WRP_LOAD4(vc, ami + row * (Cout / 4), sa.coff);
}
// the rule of bias_relu_pool_bwd_kernel, applied before the split: a masked value is an exact zero
__device__ __forceinline__ f32x4 wrp_mask(const WrpStage& sa, const f32x4& vd, const f32x4& vp) {
    f32x4 d;
#pragma unroll
    for (int t = 0; t < 4; ++t) d[t] = (sa.dok && !(vp[t] <= 0.f)) ? vd[t] : 0.f;
    return d;
}
__device__ __forceinline__ void wrp_store_a(char* ab, const f32x4& d, unsigned vc) {
    const int tid = threadIdx.x;
    char* dst = ab + wrp_aoff(0, (tid >> 2) & 3, tid >> 4, 4 * (tid & 3));
    wrs_store(dst, WRP_PLANE, d);
    const unsigned code = (vc >> (8 * (tid & 3))) & 0xffu;
    *reinterpret_cast<u16x4*>(dst + 3 * WRP_PLANE) = (u16x4){(unsigned short)(code & 3u), (unsigned short)((code >> 2) & 3u),
                                                            (unsigned short)((code >> 4) & 3u), (unsigned short)(code >> 6)};
}

// dp, p [N][H/2][W/2][Cout], am [N][H/2][W/2][Cout/4], x [N][H][W][Cin] -> part [gridDim.x][Cout][9][Cin]: what
// conv3x3_wrw_split_kernel<WIDE, WRS_MF_16> gives for the dy that bias_relu_pool_bwd_kernel makes of (dp, p, am), which is never formed.
// Same grid, jobs (row blocks of an even height), x row image, borders, partial results and order of the six products.  A step is one
// window row = two image rows: per tap ONE sparse MFMA per 16 x 16 block and product sums over the strip's 32 pixels of both rows (12
// per (tap, block of input channels) where the dense form issues 24).  The B operand of tap (kh, kw) is the dense form's x fragment of
// row r + kh - 1 followed by that of row r + kh, so the fragment of a row serves two taps: per (kw, block) the four rows' fragments are
// read once for three taps.  The x ring has five slots: row r + 3 goes into the free one half way through the step's MFMAs, row r + 4
// and the next window row of dy (one buffer: its fragments are in registers from the step's start) behind a barrier after them -
// two barriers per two rows.
template <bool WIDE>
__global__ __launch_bounds__(256, 2) void conv3x3_wrw_pooled_kernel(const float* __restrict__ dp, const float* __restrict__ p,
                                                                 const uint8_t* __restrict__ am, const float* __restrict__ x,
                                                                 float* __restrict__ part, int H, int W, int Cout, int nstrips, int nrb,
                                                                 int rpb, int njobs, int Cin) {
    HK_DYN_LDS16(ldsf);
    char* xs = reinterpret_cast<char*>(ldsf);            // ring of five x row segments (wrs16_off)
    char* as = xs + WRP_SLOTS * WRS16_SLOT;              // one window row of dy (wrp_aoff)
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int oh = wave >> 1, ch = wave & 1;
    const int cin = WIDE ? Cin : WRW_CI;
    const int slice = blockIdx.y, cslice = WIDE ? blockIdx.z : 0;
    const int Ho = H / 2, Wo = W / 2;
    const int jb = (int)((long long)blockIdx.x * njobs / gridDim.x), je = (int)((long long)(blockIdx.x + 1) * njobs / gridDim.x);

    f32x4 acc4[9][2][2];                                 // [tap][block of 16 output channels][block of 16 input channels]
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc4[t][q >> 1][q & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int aoff = wrp_aoff(0, 2 * oh, 0, 0), boff = wrs16_off(0, 2 * ch, 0, 0);
    auto mine = [&]() {                                  // (as in conv3x3_wrw_split_kernel)
        const int l = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
        return part + ((long long)blockIdx.x * Cout + slice * WRW_OT + (w >> 1) * 32 + 4 * (l >> 4)) * (9 * cin) + cslice * WRW_CI + (w & 1) * 32 + (l & 15);
    };
    auto landed = [](f32x4 (&vx)[3]) {
        __builtin_amdgcn_s_waitcnt(HK_VMCNT_IMM(0));
#pragma unroll
        for (int u = 0; u < 3; ++u) HK_PIN_LOADED(vx[u]);
    };
    int since = 0;
    bool stored = false;

    for (int j = jb; j < je; ++j) {
        const int strip = j % nstrips, jr = j / nstrips;
        const int rb = jr % nrb;
        const long long n = jr / nrb;
        const int c0 = strip * WRW_SW, r0 = rb * rpb;
        const int nsteps = ((r0 + rpb < H ? r0 + rpb : H) - r0) / 2;
        const float* xi = x + n * H * W * cin + cslice * WRW_CI;
        const float* dpi = dp + n * Ho * Wo * Cout + slice * WRW_OT;
        const float* pi = p + n * Ho * Wo * Cout + slice * WRW_OT;
        const uint8_t* ami = am + n * Ho * Wo * (Cout / 4) + slice * (WRW_OT / 4);
        WrwStage st;                                     // (its xok alone: the staging stores')
        WrpStage sa;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int idx = tid + 256 * u, col = c0 - 1 + (idx >> 4);
            st.xok[u] = idx < WRW_XF4 && col >= 0 && col < W;
            sa.xoff[u] = 4 * ((col < 0 ? 0 : (col < W ? col : W - 1)) * cin + 4 * (idx & 15));
        }
        {
            const int wcol = c0 / 2 + (tid >> 4);
            sa.dok = wcol < Wo;
            sa.doff = 4 * ((wcol < Wo ? wcol : Wo - 1) * Cout + 4 * (tid & 15));
            sa.coff = (wcol < Wo ? wcol : Wo - 1) * (Cout / 4) + ((tid & 15) & ~3);
        }
        // the first step's operands: x rows r0 - 1 .. r0 + 2 into slots 0 .. 3 and window row r0 / 2 (the barrier that ended the previous
        // job's last step has every wave past its reads)
        f32x4 vx[3], vd, vp;
        unsigned vc;
        wrp_load_a(dpi, pi, ami, sa, r0 / 2, Ho, Wo, Cout, vd, vp, vc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool rok = wrp_load_x(xi, sa, r0 - 1 + t, H, W, cin, vx);
            landed(vx);
            wrs16_store_x(xs, t, st, rok, vx);
        }
        HK_PIN_LOADED(vd); HK_PIN_LOADED(vp); HK_PIN_LOADED(vc);
        wrp_store_a(as, wrp_mask(sa, vd, vp), vc);
        __syncthreads();
        int base = 0;                                    // slot of x row r - 1 of the step
        for (int s = 0; s < nsteps; ++s) {               // rows r = r0 + 2 s and r + 1: x rows r - 1 .. r + 2 are slots base .. base + 3 (mod 5)
            const int r = r0 + 2 * s;
            bool rok = wrp_load_x(xi, sa, r + 3, H, W, cin, vx);
            wrp_load_a(dpi, pi, ami, sa, r / 2 + 1, Ho, Wo, Cout, vd, vp, vc);
            const char* B[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) B[t] = xs + ((base + t) % WRP_SLOTS) * WRS16_SLOT + boff;
            constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
            bf16x8 a[2][3];
            int idx[2];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) wrp_afrag(as + aoff + wrp_aoff(0, ob, 0, 0), g, l15, a[ob], idx[ob]);
            // 18 rounds of twelve MFMAs: (kw, block of 16 input channels) x kh.  A piece's fragment of the next round is read as soon as the
            // piece has had its last product of this round: lo after the second, mid after the fourth, hi at the end
            bf16x16 b[3];
#pragma unroll
            for (int sp = 0; sp < 3; ++sp)
                b[sp] = __builtin_shufflevector(wrs16_frag(B[0] + wrs16_off(sp, 0, 0, 0), g, l15), wrs16_frag(B[1] + wrs16_off(sp, 0, 0, 0), g, l15),
                                                0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                const int kw = i / 6, cb = (i / 3) % 2, kh = i % 3, t = 3 * kh + kw;
                const int kwn = (i + 1) / 6, cbn = ((i + 1) / 3) % 2, khn = (i + 1) % 3;
                auto next = [&](int sp) {                // piece sp of round i + 1: the upper row moves down and row kh + 2 comes in, or two new rows
                    if (i + 1 == 18) return;
                    const bf16x8 up = wrs16_frag(B[khn + 1] + wrs16_off(sp, cbn, kwn, 0), g, l15);
                    if (khn > 0)
                        b[sp] = __builtin_shufflevector(b[sp], __builtin_shufflevector(up, up, 0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7),
                                                        8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23);
                    else
                        b[sp] = __builtin_shufflevector(wrs16_frag(B[0] + wrs16_off(sp, cbn, kwn, 0), g, l15), up,
                                                        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                };
#pragma unroll
                for (int pr = 0; pr < 6; ++pr) {
#pragma unroll
                    for (int ob = 0; ob < 2; ++ob)
                        acc4[t][ob][cb] = smfmac_f32_16x16x64_bf16(a[ob][PA[pr]], b[PB[pr]], acc4[t][ob][cb], idx[ob]);
                    if (pr == 1 || pr == 3 || pr == 5) {
                        __builtin_amdgcn_sched_barrier(0);
                        next(pr == 1 ? 2 : (pr == 3 ? 1 : 0));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (i == 8) {                            // row r + 3 into the free slot, row r + 4 on its way; dp and p become one value
                    landed(vx);
                    HK_PIN_LOADED(vd); HK_PIN_LOADED(vp); HK_PIN_LOADED(vc);
                    vd = wrp_mask(sa, vd, vp);
                    wrs16_store_x(xs, (base + 4) % WRP_SLOTS, st, rok, vx);
                    rok = wrp_load_x(xi, sa, r + 4, H, W, cin, vx);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();                             // every wave has read rows r - 1, r and - long ago - the dy buffer
            landed(vx);
            wrs16_store_x(xs, base, st, rok, vx);
            wrp_store_a(as, vd, vc);
            __syncthreads();
            base = (base + 2) % WRP_SLOTS;
            if (++since == WRP_FLUSH) {
                wrs16_flush(mine(), acc4, stored, cin);
                since = 0;
                stored = true;
            }
        }
    }
    if (since > 0 || !stored) wrs16_flush(mine(), acc4, stored, cin);
}

// Which calls the pooled form serves by default (knob wrw_pool at -1), decided by the layers' times inside the training step
// (profiles/wrw_pool_step_layers.json: HK_WRW_POOL=0 against the default on this build): all five pooled layers of VGG-16 at 448 x 448 are
// faster at batch 64 (0.65 - 0.68 x the dense kernel's time, the slowest repeat below the dense kernel's fastest) and at batch 16
// (0.36 - 0.68 x).  The rule is "always" from the smallest map that was measured (conv5_3 at batch 16: 16 x 28 x 28 pixels) and
// nothing below it, which nobody has timed; `wrw_pool` 1 reaches the kernel at every served shape (tests).
static bool wrw_pool_wins(int N, int H, int W, int Cin, int Cout) {
    (void)Cin; (void)Cout;
    return (long long)N * H * W >= 16ll * 28 * 28;
}

template <bool WIDE>
static int wrw_pooled_launch(dim3 grid, const float* dp, const float* p, const uint8_t* am, const float* x, float* part, int H, int W,
                             int Cout, const WrwPlan& pl, int cin, hk_stream_t stream) {
    HK_ALLOW_BIG_LDS((conv3x3_wrw_pooled_kernel<WIDE>), WRP_LDS);
    hipLaunchKernelGGL((conv3x3_wrw_pooled_kernel<WIDE>), grid, dim3(256), WRP_LDS, (hipStream_t)stream, dp, p, am, x, part, H, W, Cout,
                       pl.nstrips, pl.nrb, pl.rpb, pl.njobs, cin);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

// the shapes the pooled form runs on: hk_conv3x3_wrw's wide split form's, and whole windows
static bool wrw_pooled_shape_ok(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return false;
    if (Cin % WRW_CI != 0 || Cout % WRW_OT != 0 || Cout / WRW_OT > 65535 || Cin / WRW_CI > 65535 || (long long)Cout * 9 * Cin > 0x7fffffffll) return false;
    if ((long long)(Cout / WRW_OT) * (Cin / WRW_CI) > 0x7fffffffll) return false;
    // WrpStage's lane offsets are 32-bit bytes from a row's start: a row of x and a window row of dp / p stay below 2^31 bytes
    if ((long long)W * Cin * 4 > 0x7fffffffll || (long long)(W / 2) * Cout * 4 > 0x7fffffffll) return false;
    return H % 2 == 0 && W % 2 == 0;
}

}  // namespace hk

using namespace hk;

extern "C" size_t hk_conv3x3_wrw_ws_bytes(int Cin, int Cout) {      // (for any sizes > 0: the workspace check comes before the shape check)
    if (Cin <= 0 || Cout <= 0) return 0;
    const size_t one = (size_t)Cout * 9 * Cin * sizeof(float);       // one workgroup's share: a whole dW
    if (Cin <= WRW_CI) return WRW_MAX_WG * one;
    return wrw_wide_wgs(((long long)Cin + WRW_CI - 1) / WRW_CI * (((long long)Cout + WRW_OT - 1) / WRW_OT)) * one;
}

extern "C" int hk_conv3x3_wrw(const float* dy, const float* x, float* dw, int N, int H, int W, int Cin, int Cout, void* ws,
                              size_t ws_bytes, hk_stream_t stream) {
    if (!dy || !x || !dw || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_conv3x3_wrw_ws_bytes(Cin, Cout)) return HK_ERR_WORKSPACE;
    if (Cin % WRW_CI != 0 || Cout % WRW_OT != 0 || Cout / WRW_OT > 65535 || Cin / WRW_CI > 65535 || (long long)Cout * 9 * Cin > 0x7fffffffll ||
        !aligned16(dy) || !aligned16(x) || !aligned16(dw) || !aligned16(ws))
        return HK_ERR_UNSUPPORTED;
    const int split = tuning().wrw_split;
    const bool wide = Cin > WRW_CI;                      // only the split form reads a 64-channel slice out of wider x pixels
    if (wide && (split == 0 || tuning().wrw_wide == 0)) return HK_ERR_UNSUPPORTED;
    const int oslices = Cout / WRW_OT, cslices = Cin / WRW_CI;
    if ((long long)oslices * cslices > 0x7fffffffll) return HK_ERR_UNSUPPORTED;
    WrwPlan pl;
    if (!wrw_plan(N, H, W, oslices * cslices, wide, pl)) return HK_ERR_UNSUPPORTED;
    float* part = (float*)ws;
    const int mfma = tuning().wrw_mfma;
    const bool mf16 = mfma == 1 || (mfma < 0 && wrw_mfma16_wins(N, H, W, Cout));
    if (wide) {
        const dim3 grid((unsigned)pl.nwg, (unsigned)oslices, (unsigned)cslices);
        const int e = mf16 ? wrw_split_launch<true, WRS_MF_16>(grid, dy, x, part, H, W, Cout, pl, Cin, stream)
                           : wrw_split_launch<true, WRS_MF_32>(grid, dy, x, part, H, W, Cout, pl, Cin, stream);
        if (e != HK_OK) return e;
    } else if (split > 0 || (split < 0 && wrw_split_wins(N, H, W, Cout))) {
        const dim3 grid((unsigned)pl.nwg, (unsigned)(Cout / WRW_OT));
        const int e = mf16 ? wrw_split_launch<false, WRS_MF_16>(grid, dy, x, part, H, W, Cout, pl, WRW_CI, stream)
                           : wrw_split_launch<false, WRS_MF_32>(grid, dy, x, part, H, W, Cout, pl, WRW_CI, stream);
        if (e != HK_OK) return e;
    } else {
        hipLaunchKernelGGL(conv3x3_wrw_kernel, dim3((unsigned)pl.nwg, (unsigned)(Cout / WRW_OT)), dim3(256), 0, (hipStream_t)stream, dy, x,
                           part, H, W, Cout, pl.nstrips, pl.nrb, pl.rpb, pl.njobs);
    }
    HK_LAUNCH_CHECK();
    const int nel = Cout * 9 * Cin;
    hipLaunchKernelGGL(partial_sum_kernel<16>, dim3((nel + 63) / 64), dim3(1024), 0, (hipStream_t)stream, (const float*)part, pl.nwg, nel, nel,
                       dw, (float*)nullptr);
    HK_LAUNCH_CHECK();
    return HK_OK;
}

// ---- hawkeye_conv_pool.h ----
// the one reader of the knob wrw_pool and its rule
extern "C" int hk_conv3x3_wrw_pooled_served(int N, int H, int W, int Cin, int Cout) {
    const int pool = tuning().wrw_pool;
    if (pool == 0 || tuning().wrw_split == 0 || tuning().wrw_wide == 0 || !wrw_pooled_shape_ok(N, H, W, Cin, Cout)) return 0;
    return pool > 0 || wrw_pool_wins(N, H, W, Cin, Cout) ? 1 : 0;
}

extern "C" int hk_conv3x3_wrw_pooled_plan(int N, int H, int W, int Cin, int Cout, int* out) {
    if (!out) return HK_ERR_BAD_ARG;
    if (!wrw_pooled_shape_ok(N, H, W, Cin, Cout)) return HK_ERR_UNSUPPORTED;
    WrwPlan pl;
    if (!wrw_plan(N, H, W, (Cout / WRW_OT) * (Cin / WRW_CI), true, pl, true)) return HK_ERR_UNSUPPORTED;
    out[0] = pl.nstrips; out[1] = pl.nrb; out[2] = pl.rpb; out[3] = pl.njobs; out[4] = pl.nwg;
    return HK_OK;
}

extern "C" int hk_conv3x3_wrw_pooled(const float* dp, const float* p, const uint8_t* argmax, const float* x, float* dw, int N, int H, int W,
                                     int Cin, int Cout, void* ws, size_t ws_bytes, hk_stream_t stream) {
    if (!dp || !p || !argmax || !x || !dw || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return HK_ERR_BAD_ARG;
    if (!ws || ws_bytes < hk_conv3x3_wrw_ws_bytes(Cin, Cout)) return HK_ERR_WORKSPACE;
    if (!wrw_pooled_shape_ok(N, H, W, Cin, Cout) || !aligned16(dp) || !aligned16(p) || !aligned16(argmax) || !aligned16(x) || !aligned16(dw) ||
        !aligned16(ws) || tuning().wrw_split == 0 || tuning().wrw_wide == 0)
        return HK_ERR_UNSUPPORTED;
    // (the plan and the workspace of a WIDE call at every Cin: with one Cin slice that is wrw_wide_wgs(Cout slices) <= WRW_MAX_WG workgroups)
    const int oslices = Cout / WRW_OT, cslices = Cin / WRW_CI;
    WrwPlan pl;
    if (!wrw_plan(N, H, W, oslices * cslices, true, pl, true)) return HK_ERR_UNSUPPORTED;
    float* part = (float*)ws;
    const dim3 grid((unsigned)pl.nwg, (unsigned)oslices, (unsigned)cslices);
    const int e = Cin > WRW_CI ? wrw_pooled_launch<true>(grid, dp, p, argmax, x, part, H, W, Cout, pl, Cin, stream)
                               : wrw_pooled_launch<false>(grid, dp, p, argmax, x, part, H, W, Cout, pl, WRW_CI, stream);
    if (e != HK_OK) return e;
    const int nel = Cout * 9 * Cin;
    hipLaunchKernelGGL(partial_sum_kernel<16>, dim3((nel + 63) / 64), dim3(1024), 0, (hipStream_t)stream, (const float*)part, pl.nwg, nel, nel,
                       dw, (float*)nullptr);
    HK_LAUNCH_CHECK();
    return HK_OK;
}
