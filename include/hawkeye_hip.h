/* hawkeye_hip.h - C ABI of libhawkeye_hip.so (MI355X / gfx950 kernels for the
 * Hawkeye high-order pooling + attention-pooling hot path).
 *
 * The reference (Hawkeye-FineGrained/Hawkeye) is pure Python/PyTorch: it has no
 * FFI of its own.  Each entry point below therefore replaces a *sequence of ATen
 * calls* issued by one reference function; the function is cited as
 * "replaces <file>:<lines>" (paths relative to the reference checkout).  The
 * Python binding a maintainer adds on the reference side is a ctypes stub inside
 * a torch.autograd.Function - see INTEGRATION.md.
 *
 * Conventions
 *  - all pointers are DEVICE pointers to contiguous fp32 (or int32 where said)
 *    buffers owned by the caller; nothing is allocated or freed by the library;
 *  - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream);
 *    every call only enqueues kernels on it: no host synchronisation.  Process-wide
 *    state is limited to (a) the test-only hk_tuning_* knobs and (b) one helper HIP
 *    queue + event pair per device, owned by the library, created once
 *    (std::call_once) on the first batched Newton-Schulz call and used inside
 *    hk_ns_sqrtm_fwd / _bwd only: the two halves of the batch are forked onto it
 *    and joined back onto `stream` before the entry point returns - also on its
 *    error paths.  A per-device mutex is held from fork to join, so several host
 *    threads may drive one device (they take turns on the helper queue);
 *  - scratch memory is passed in (`ws`, `ws_bytes`); the matching
 *    hk_*_ws_bytes() tells how much is needed; contents need not be preserved
 *    between calls unless stated ("saved for backward" buffers are explicit
 *    arguments);
 *  - return value: 0 on success, a negative HK_ERR_* for bad arguments, or a
 *    positive hipError_t from the launch;
 *  - reductions use fixed orders (no float atomics): reruns are bit-identical.
 */
#ifndef HAWKEYE_HIP_H
#define HAWKEYE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hk_stream_t; /* hipStream_t */

#define HK_OK 0
#define HK_ERR_BAD_ARG (-1)
#define HK_ERR_WORKSPACE (-2)
#define HK_ERR_UNSUPPORTED (-3)

/* library / build identification: returns e.g. "hawkeye_hip 0.1 gfx950" */
const char* hk_version(void);

/* A/B levers for tests, benchmarks and profiling - never needed by a caller of the ops.  Each knob selects between
 * implementations that produce the same results (bit-identical or to rounding); the defaults are the measured winners.
 *   "bcnn_generic"  1 = generic GEMM path for the Gram / covariance / CBP kernels and the three-kernel CIN forward
 *   "bwd_v"         Gram backward (BCNN / signed-sqrt / covariance / CBP): 0 automatic (gram_bwd3_kernel / cbp_bwd3_kernel
 *                   where their row blocks fill the chip, else the 64-row panel kernel); 1 panel kernel
 *   "cbp_bin"       CBP forward: -1 automatic (the fused Gram + binning kernel where the plan allows it, else by batch
 *                   size), 0 row-sketch, 1 CSR gather, 2 row-scatter, 3 fused, 4 fused without paired tile steps
 *   "roi_bwd"       0 = LDS-staged ROI refinement kernels, 1 = the round-1 table kernels
 *   "linear_slabs"  split-K slabs of hk_linear_fwd (0 automatic, -1 generic tiles)
 *   "ns_tn"         tile width of the Newton-Schulz products (0 automatic, 64, 128)
 *   "ns_streams"    n: the batch runs the Newton-Schulz chain in n + 1 parts on n + 1 HIP queues (default 1, at most 3)
 *   "ns_sym"        1 (default): hk_ns_sqrtm_fwd_sym skips the tiles below the diagonal blocks; 0: it computes all
 *   "lin_walk"      classifier backward: 1 workgroup s walks the 64-feature chunks s, s + S, ..; 0 a contiguous slab per
 *                   workgroup; -1 (default) the measured winner per kernel
 *   "sched_b"       > 0: batch-size dependent work splits behave as if the batch were this (tests)
 *   "conv_wrw"      1 (default): the trunk routes the weight gradient of its 3 x 3 convolutions with a multiple of 64 input channels to
 *                   hk_conv3x3_wrw where that is the measured winner; 0: the library's weight gradient everywhere
 *   "wrw_wgs"       hk_conv3x3_wrw: workgroups per 64 x 64 slice of (Cout, Cin), at most (0 = two per CU over all slices; up to 512 with
 *                   64 input channels, up to what the workspace holds - max(1, 512 / slices) - with more)
 *   "wrw_split"     hk_conv3x3_wrw: 0 = the fp32-MFMA kernel (64 input channels only), 1 = the three-way split bf16-MFMA kernel wherever
 *                   the entry point serves the call, -1 (default) = per layer, the measured winner
 *   "wrw_wide"      hk_conv3x3_wrw with more than 64 input channels: 1 (default) = served (by the split form); 0 = refused with
 *                   HK_ERR_UNSUPPORTED, as before the split form read wider pixels
 *   "wrw_mfma"      the bf16 MFMA the split form of hk_conv3x3_wrw runs on: 1 = v_mfma_f32_16x16x32_bf16, 0 = v_mfma_f32_32x32x16_bf16,
 *                   -1 (default) = per call, the measured winner (a rule in N, H, W and Cout).  Same bound either way; the bits differ
 *   "wrw_pool"      weight gradient of a 3 x 3 layer that ends in a 2 x 2 max-pool, straight from the pooled gradient on the 2:4 sparse
 *                   bf16 MFMA (hawkeye_conv_pool.h): 0 = never, 1 = wherever served, -1 (default) = per layer, the measured winner
 *   "conv_fwd"      forward of the trunk's 3 x 3 convolutions with multiples of 64 channels (hawkeye_conv.h): -1 (default) = the split
 *                   bf16-MFMA kernel for the layers of the measured table, 0 = the library's everywhere (the entry point then refuses
 *                   with HK_ERR_UNSUPPORTED), 1 = the kernel wherever the entry point serves the call (tests)
 *   "conv_bwd_data" the same for the input gradient of those convolutions
 *   "conv_epi"      epilogues inside those kernels: 2 (default) = bias + ReLU (+ pool) in the forward and the producing layer's ReLU
 *                   mask + bias-gradient partials in the input gradient, 1 = the forward ones only, 0 = none (separate passes)
 *   "conv_mfma"     the bf16 MFMA those kernels run on: 1 = v_mfma_f32_16x16x32_bf16, 0 = v_mfma_f32_32x32x16_bf16, -1 (default) = per
 *                   call: 32x32x16 unless the caller has set 1 for the call, as the Python layer does for the layers of its
 *                   measured table.  Same results to the bound of hawkeye_conv.h either way; the bits differ
 *   "conv_tile"     which 128 pixels a workgroup of those kernels takes: -1 (default) = per map and MFMA shape the tiling with the fewest
 *                   tiles (hk_conv3x3_tile_plan), 0 = 4 rows x 32 columns everywhere.  The same bits either way
 * Values are seeded once from the environment (HK_<NAME>) when the library is first used; the launch paths never read
 * the environment.  Returns HK_ERR_BAD_ARG for an unknown name.  Process-wide: set them only while no other thread is
 * launching. */
int hk_tuning_set(const char* name, int value);
int hk_tuning_get(const char* name, int* value);

/* ---------------------------------------------------------------- BCNN ----
 * Bilinear pooling: G = X X^T / HW ; z = sqrt(G + 1e-5) ; y = z / max(|z|_2, 1e-12).
 * replaces model/methods/BCNN.py:13-27 (BilinearPooling.forward: view, transpose,
 * bmm, div, add, sqrt, F.normalize) and its autograd backward.
 *   x        [B, C, HW]   input feature map (NCHW contiguous, HW = H*W)
 *   y        [B, C*C]     output
 *   inv_norm [B]          1/max(|z|_2,1e-12)            (saved for backward)
 *   colsum   [B, HW]      sum_c x[b,c,hw]               (saved for backward)
 */
size_t hk_bcnn_pool_ws_bytes(int B, int C, int HW);
int hk_bcnn_pool_fwd(const float* x, float* y, float* inv_norm, float* colsum, int B, int C, int HW,
                     void* ws, size_t ws_bytes, hk_stream_t stream);
/* dx [B, C, HW] = d loss / d x given dy [B, C*C] */
int hk_bcnn_pool_bwd(const float* x, const float* y, const float* dy, const float* inv_norm,
                     const float* colsum, float* dx, int B, int C, int HW, void* ws, size_t ws_bytes,
                     hk_stream_t stream);
/* The same backward when dy is the input gradient of a linear layer ON y (BCNN.py:54: logits = classifier(y)), i.e.
 * dy = g W: the inner product t = <y, dy> the normalisation's backward needs (autograd of F.normalize, BCNN.py:26) is then
 *     t[b] = sum_k ta[b,k] * (tb[b,k] - tc[k])          ta = g [B,K], tb = logits [B,K], tc = bias [K] (nullable)
 * - B*K multiply-adds instead of a pass over the 2 x 4 C^2 bytes per image of y and dy: one launch, the rank-1 term applied
 * while dX is written.  Any (ta, tb, tc) with that property may be passed; with another it computes dX for THAT t. */
int hk_bcnn_pool_bwd_tdot(const float* x, const float* y, const float* dy, const float* inv_norm,
                          const float* colsum, const float* ta, const float* tb, const float* tc, int K,
                          float* dx, int B, int C, int HW, void* ws, size_t ws_bytes, hk_stream_t stream);

/* Signed-sqrt variant - the second normalisation the reference keeps (commented out) next to the one it runs:
 *     G = X X^T / HW ; u = sign(G) sqrt(|G| + 1e-10) ; y = u / max(|u|_2, 1e-12)
 * replaces model/methods/BCNN.py:18,23-26 (the `sign * sqrt(abs + 1e-10)` alternative; = CBCNN.py:132 on the 512x512
 * Gram) and its autograd backward.  Raw Gram on the panel kernel, then two elementwise passes (the norm of u has no
 * closed form from column sums); backward: t = <y, dy> partials, then the same GEMM-shaped launch as the default
 * variant with P = (dy + dy^T - 2 t y) / |y| * inv_norm^2 / (2 HW), zero where y = 0 (torch: sign'(0) = abs'(0) = 0).
 *   inv_norm [B]  saved for backward ;  ws: hk_bcnn_ssqrt_ws_bytes */
size_t hk_bcnn_ssqrt_ws_bytes(int B, int C, int HW);
int hk_bcnn_ssqrt_pool_fwd(const float* x, float* y, float* inv_norm, int B, int C, int HW, void* ws, size_t ws_bytes,
                           hk_stream_t stream);
int hk_bcnn_ssqrt_pool_bwd(const float* x, const float* y, const float* dy, const float* inv_norm, float* dx, int B, int C,
                           int HW, void* ws, size_t ws_bytes, hk_stream_t stream);
/* The same pooling with the l2 scale left to the consumer ("fold the per-sample 1 / |z| into the classifier's
 * epilogue"): _fwd_unscaled writes u = sign(G) sqrt(|G| + 1e-10) and inv_norm = 1 / max(|u|_2, 1e-12) - the scale pass over
 * the 4 C^2 bytes per image is not launched; hk_linear_fwd_scaled(u, ..., row_scale = inv_norm) applies it to the
 * [B, classes] logits.  _bwd_unscaled takes that u and dy = dL/d(inv_norm u) (what hk_linear_bwd_scaled returns).
 * (The default sqrt(G + 1e-5) variant needs none of this: its norm is known before the Gram is formed.) */
int hk_bcnn_ssqrt_pool_fwd_unscaled(const float* x, float* u, float* inv_norm, int B, int C, int HW, void* ws, size_t ws_bytes,
                                    hk_stream_t stream);
int hk_bcnn_ssqrt_pool_bwd_unscaled(const float* x, const float* u, const float* dy, const float* inv_norm, float* dx, int B,
                                    int C, int HW, void* ws, size_t ws_bytes, hk_stream_t stream);
/* ... and with the norm left entirely to the consumer: ONE launch that writes u and *nparts partial sums of u^2 per image
 * (ss_part [B, 64]); hk_linear_fwd_ssq (below) adds them up in its reduce launch, applies 1 / |u| to the logits and writes
 * inv_norm.  HK_ERR_UNSUPPORTED (nothing launched) outside the panel kernel's shapes. */
int hk_bcnn_ssqrt_pool_fwd_parts(const float* x, float* u, float* ss_part, int* nparts, int B, int C, int HW, hk_stream_t stream);
/* Either backward when dy = g W comes from a linear layer on the normalised pooled vector: the inner product <y, dy> of the
 * l2-normalisation's backward is then t[b] = sum_k ta[b,k] (tb[b,k] - tc[k]) (ta = g, tb = logits, tc = bias, nullable) and the
 * pass over y and dy that adds it up (2 x 4 C^2 bytes per image) is not launched.  unscaled = 0: y as hk_bcnn_ssqrt_pool_fwd
 * returned it; != 0: the u / dy of the _unscaled pair. */
int hk_bcnn_ssqrt_pool_bwd_tdot(const float* x, const float* y, const float* dy, const float* inv_norm, const float* ta,
                                const float* tb, const float* tc, int K, int unscaled, float* dx, int B, int C, int HW,
                                void* ws, size_t ws_bytes, hk_stream_t stream);

/* The two stages of each direction, individually callable (hk_bcnn_pool_fwd = colsum_norm + gram_norm,
 * hk_bcnn_pool_bwd = bwd_gemm + bwd_rank1); bench.py times them separately.
 *   tpart [B, ceil(C/64)] partial sums of <y,dy> written by bwd_gemm, consumed by bwd_rank1 */
/* ws (optional, hk_bcnn_pool_ws_bytes): enables the two-stage column sum (B*C/64 workgroups instead of B) */
int hk_bcnn_colsum_norm(const float* x, float* colsum, float* inv_norm, int B, int C, int HW, void* ws,
                        size_t ws_bytes, hk_stream_t stream);
int hk_bcnn_gram_norm(const float* x, const float* inv_norm, float* y, int B, int C, int HW, hk_stream_t stream);
int hk_bcnn_bwd_gemm(const float* x, const float* y, const float* dy, const float* inv_norm, float* dx,
                     float* tpart, int B, int C, int HW, hk_stream_t stream);
int hk_bcnn_bwd_rank1(float* dx, const float* tpart, const float* inv_norm, const float* colsum, int B, int C,
                      int HW, hk_stream_t stream);

/* ------------------------------------------------------------ Fast MPN-COV ----
 * Covariance pooling  cov = (1/M) (X - mu 1^T) X^T.
 * replaces model/methods/MPNCOV.py:105-119 (Covpool.forward) / :121-134 (backward).
 *   x [B, C, M] ; cov [B, C, C] ; mu [B, C] channel means (saved for backward)
 */
int hk_cov_pool_fwd(const float* x, float* cov, float* mu, int B, int C, int M, hk_stream_t stream);
int hk_cov_pool_bwd(const float* x, const float* mu, const float* dcov, float* dx, int B, int C, int M,
                    hk_stream_t stream);

/* Newton-Schulz matrix square root, iter_n coupled iterations with trace
 * pre-normalisation and sqrt(trace) post-compensation.
 * replaces model/methods/MPNCOV.py:137-164 (Sqrtm.forward) / :166-202 (backward,
 * including its per-sample python loop :198-201).
 *   a      [B, d, d]  input (covariance)
 *   out    [B, d, d]  sqrtm
 *   norm_a [B]        trace(a)                                  (saved)
 *   ysave, zsave [B, max(iter_n-1,1), d, d]  Y_i / Z_i iterates (saved; unused when iter_n < 2)
 */
size_t hk_ns_sqrtm_ws_bytes(int B, int d, int iter_n, int backward);
int hk_ns_sqrtm_fwd(const float* a, float* out, float* norm_a, float* ysave, float* zsave, int B, int d,
                    int iter_n, void* ws, size_t ws_bytes, hk_stream_t stream);
/* hk_ns_sqrtm_fwd_sym: the same, for a SYMMETRIC input `a` (what Covpool produces and all MPNCOV.forward ever feeds
 * Sqrtm, MPNCOV.py:73-76).  Every product of the chain is then a symmetric matrix (a polynomial in `a`): the launches
 * compute only the tiles that touch the 128 x 128 blocks on or above the diagonal (3 of 4 at d = 256) and write the
 * blocks right of the diagonal twice, transposed.  Results differ from hk_ns_sqrtm_fwd by the rounding asymmetry of a
 * product of commuting symmetric matrices (~1e-7 relative); with an input that is not symmetric the result is WRONG -
 * use hk_ns_sqrtm_fwd.  d % 128 != 0 falls back to the full schedule.  Saved iterates are interchangeable with
 * hk_ns_sqrtm_fwd's for either backward. */
int hk_ns_sqrtm_fwd_sym(const float* a, float* out, float* norm_a, float* ysave, float* zsave, int B, int d,
                        int iter_n, void* ws, size_t ws_bytes, hk_stream_t stream);
/* Sqrtm followed by Triuvec, as MPNCOV.forward applies them (MPNCOV.py:88-92): the chain's last product writes `out`
 * [B, d, d] (saved for the backward) AND its row-major packed upper triangle tv [B, d (d + 1) / 2] - what
 * hk_triu_vec_fwd(out) would return, bit for bit, without the extra pass.  symmetric != 0: the schedule of
 * hk_ns_sqrtm_fwd_sym (input must be symmetric), else that of hk_ns_sqrtm_fwd.  Backward: hk_triu_vec_bwd then
 * hk_ns_sqrtm_bwd. */
int hk_ns_sqrtm_triu_fwd(const float* a, float* out, float* tv, float* norm_a, float* ysave, float* zsave, int B, int d,
                         int iter_n, int symmetric, void* ws, size_t ws_bytes, hk_stream_t stream);
/* hk_ns_sqrtm_bwd executes 34 products instead of the reference's 38: Z_i Y_i is taken from the accumulator of Y_i Z_i.
 * That is exact for ANY input `a`, symmetric or not: every iterate is a polynomial in the one matrix A = a / tr(a)
 * (Y_0 = A (3I - A)/2, Z_0 = (3I - A)/2, and each step multiplies polynomials in A), and polynomials in one matrix
 * commute.  Measured on non-symmetric inputs: 6.7e-7 from the reference, the same as the 38-product form
 * (tests/test_gpu_kernels.py::test_ns_general_input_backward).  The upstream gradient `dout` may be anything.
 * hk_ns_sqrtm_bwd_general: same arguments, Z_i Y_i as its own product - all 38 of MPNCOV.py:174-194, literally; kept
 * for A/B checks (it costs four more products). */
int hk_ns_sqrtm_bwd(const float* a, const float* out, const float* norm_a, const float* ysave,
                    const float* zsave, const float* dout, float* da, int B, int d, int iter_n, void* ws,
                    size_t ws_bytes, hk_stream_t stream);
int hk_ns_sqrtm_bwd_general(const float* a, const float* out, const float* norm_a, const float* ysave,
                            const float* zsave, const float* dout, float* da, int B, int d, int iter_n, void* ws,
                            size_t ws_bytes, hk_stream_t stream);

/* Row-major upper-triangle (incl. diagonal) vectorisation, index in closed form.
 * replaces model/methods/MPNCOV.py:205-218 (Triuvec.forward; index built on the
 * CPU every call :213-214) / :220-230 (backward).
 *   x [B, d, d] -> y [B, d(d+1)/2]
 */
int hk_triu_vec_fwd(const float* x, float* y, int B, int d, hk_stream_t stream);
int hk_triu_vec_bwd(const float* dy, float* dx, int B, int d, hk_stream_t stream);

/* ------------------------------------------------------- Compact bilinear ----
 * Tensor-sketch compact bilinear pooling, evaluated through the exact identity
 *   c[b,k] = sum_{i,j : (h1[i]+h2[j]) mod D = k} s1[i] s2[j] (X X^T)[b,i,j]
 * (= ifft(fft(S1^T x) * fft(S2^T x)) summed over positions), then
 *   u = sign(c) sqrt(|c| + 1e-10) ; y = u / max(|u|_2, 1e-12).
 * replaces model/methods/CBCNN.py:96-135 (CompactBilinearPooling.forward) and its
 * autograd backward.
 * hk_cbp_plan_build: host+device one-time setup from the count-sketch hashes
 * (CBCNN.py:76-91): writes the hash tables, a CSR "bin -> (i*C+j, sign)" table and
 * (C % 64 == 0) the sorted per-tile gather lists of the fused forward into `plan`
 * (device memory, hk_cbp_plan_bytes(C, D) bytes).  h1,h2 int32 [C] in [0,D);
 * s1,s2 fp32 [C] of +-1; all four are HOST pointers.  The library remembers, per
 * plan ADDRESS, whether the fused lists could be built for these hashes (a host-side
 * directory under a mutex - the blob itself is device memory); hk_cbp_fwd on a blob
 * the caller has copied elsewhere takes the unfused kernels: same results to rounding.
 * hk_cbp_plan_destroy(plan) forgets the address: call it BEFORE freeing or reusing the
 * plan's memory, so that another blob placed there later cannot inherit the entry.
 * hk_cbp_fwd: Gram and binning in one kernel (the Gram matrix never reaches HBM),
 * then two small finishing launches; ws holds the per-workgroup partial bin vectors.
 */
size_t hk_cbp_plan_bytes(int C, int D);
int hk_cbp_plan_destroy(const void* plan);
int hk_cbp_plan_build(const int32_t* h1, const float* s1, const int32_t* h2, const float* s2, int C, int D,
                      void* plan, hk_stream_t stream);
size_t hk_cbp_ws_bytes(int B, int C, int HW, int D);
/* x [B,C,HW] -> y [B,D]; c_raw [B,D] pre-normalisation sums and inv_norm [B] saved for backward */
int hk_cbp_fwd(const float* x, const void* plan, float* y, float* c_raw, float* inv_norm, int B, int C, int HW,
               int D, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_cbp_bwd(const float* x, const void* plan, const float* y, const float* c_raw, const float* inv_norm,
               const float* dy, float* dx, int B, int C, int HW, int D, void* ws, size_t ws_bytes,
               hk_stream_t stream);

/* The two forms of CompactBilinearPooling.forward Hawkeye's own CBCNN never takes (it calls it with one input and
 * sum_pool = True, CBCNN.py:23,33): two DIFFERENT inputs (CBCNN.py:96-102) and sum_pool = False (:127-130), for any widths
 * C1, C2 (CompactBilinearPooling(C1, C2, D), CBCNN.py:68-94 builds one sketch matrix per input width; :104-105 asserts
 * bottom1 has C1 and bottom2 C2 channels).  The same identity over the C1 x C2 cross Gram G = X1 X2^T (hk_bgemm_f32):
 *   c[b,k] = sum_{(i,j) : (h1[i] + h2[j]) mod D = k} s1[i] s2[j] G[b,i,j].
 *   hk_cbp_rect_plan_build   hashes h1 [C1], h2 [C2] in [0,D), signs s1 [C1], s2 [C2] (HOST pointers) -> `plan` (DEVICE memory,
 *                            hk_cbp_rect_plan_bytes(C1, C2, D) bytes: the hashes, the signs and the CSR table bin -> (i*C2+j, sign))
 *   hk_cbp_rect_bin_matrix   G [B,C1,C2] -> c_raw [B,D]            hk_cbp_rect_unbin_matrix   dc [B,D] -> dG [B,C1,C2]
 *                            (then dX1 = dG X2, dX2 = dG^T X1)
 *   hk_cbp_rect_loc_fwd/bwd  sum_pool = False: x1 [B,C1,HW], x2 [B,C2,HW] <-> c [B,HW,D]   (C1, C2 <= 1024; either gradient nullable)
 * The four kernels' entry points take a plan from either builder: a hk_cbp_plan_build blob starts with the same bytes
 * (from offset 16 on) as the hk_cbp_rect_plan_build blob of its hashes, so pass it with C1 = C2 = C.  A rect plan holds no
 * host-side state (nothing to destroy).  The signed square root and F.normalize stay the caller's. */
size_t hk_cbp_rect_plan_bytes(int C1, int C2, int D);
int hk_cbp_rect_plan_build(const int32_t* h1, const float* s1, int C1, const int32_t* h2, const float* s2, int C2, int D,
                           void* plan, hk_stream_t stream);
int hk_cbp_rect_bin_matrix(const float* G, const void* plan, float* c_raw, int B, int C1, int C2, int D, hk_stream_t stream);
int hk_cbp_rect_unbin_matrix(const float* dc, const void* plan, float* dG, int B, int C1, int C2, int D, hk_stream_t stream);
int hk_cbp_rect_loc_fwd(const float* x1, const float* x2, const void* plan, float* c, int B, int C1, int C2, int HW, int D,
                        hk_stream_t stream);
int hk_cbp_rect_loc_bwd(const float* x1, const float* x2, const float* dc, const void* plan, float* dx1, float* dx2, int B,
                        int C1, int C2, int HW, int D, hk_stream_t stream);

/* ------------------------------------------------------- VGG trunk epilogues ----
 * What PyTorch-ROCm runs around every convolution of the VGG-16 trunk (model/backbone/vgg.py:24-57: Conv2d + bias, ReLU,
 * five MaxPool2d(2, 2); BCNN.py:38-39 / CBCNN.py:22 take all of `features`) as one full-tensor pass per elementwise op -
 * bias add, ReLU, pool; pool backward, ReLU backward, bias-gradient reduction - fused to ONE pass per convolution and
 * direction.  channels_last tensors: x [rows = N H W][C], C % 4 == 0.  Replaces, with the same arithmetic,
 *   hk_bias_relu_fwd        x = max(x + bias, 0) IN PLACE                 (nn.Conv2d's bias add + nn.ReLU(inplace=True)); `mask`
 *                           (nullable, [rows][C/4] bytes): bit t of a byte = channel t of the quad came out positive
 *   hk_bias_relu_bwd        dx = dy where y > 0 else 0 ; dbias = sum dx   (threshold_backward + the convolution's bias gradient;
 *                           dx may alias dy); the sign from `mask` when given (1/16 of the bytes of y), else from y
 *   hk_bias_relu_pool_fwd   p = maxpool2x2(max(x + bias, 0)), argmax [N][H/2][W/2][C/4] bytes (2 bits per channel: window position
 *                           2 dh + dw of the FIRST maximum, ATen's tie rule); the full-resolution activation is not written
 *   hk_bias_relu_pool_bwd   dx [N][H][W][C] = dp routed to the argmax where p > 0, zeros elsewhere ; dbias = sum dx
 * The backward kernels need C / 4 to divide 256 (C = 64 .. 512 in VGG) and a workspace of hk_trunk_ws_bytes(C) bytes (partial
 * column sums, added in a fixed order: deterministic).  HK_ERR_UNSUPPORTED (nothing launched) for other shapes / unaligned
 * pointers: the caller keeps the framework's own ops for those. */
size_t hk_trunk_ws_bytes(int C);
int hk_bias_relu_fwd(float* x, const float* bias, uint8_t* mask, long long rows, int C, hk_stream_t stream);
int hk_bias_relu_bwd(const float* dy, const float* y, const uint8_t* mask, float* dx, float* dbias, long long rows, int C, void* ws,
                     size_t ws_bytes, hk_stream_t stream);
int hk_bias_relu_pool_fwd(const float* x, const float* bias, float* p, uint8_t* argmax, int N, int H, int W, int C,
                          hk_stream_t stream);
int hk_bias_relu_pool_bwd(const float* dp, const float* p, const uint8_t* argmax, float* dx, float* dbias, int N, int H, int W,
                          int C, void* ws, size_t ws_bytes, hk_stream_t stream);
/* The end of a ResNet bottleneck, `out += identity; out = relu(out)` (model/backbone/resnet.py:89-136; the trunk of MPN, AP-CNN,
 * OSMENet, CIN): hk_add_relu_fwd  a = max(a + b, 0) IN PLACE on a, n elements of any dense layout the two share, n % 4 == 0;
 * hk_relu_mask_bwd  g = dy where y > 0 else 0 - the gradient of both operands. */
/* The trunk's FIRST convolution with its epilogue, Conv2d(Cin <= 3, 64, 3, padding=1) + bias + ReLU (model/backbone/vgg.py:24-57, layer 0
 * of `features`), as one kernel per direction: the layer is the write of its 3.29 GB output / the read of that output's gradient.
 *   hk_conv1_bias_relu_fwd   x [N][H][W][Cin] (channels_last), wt [9 Cin][64] = the layer's weight permuted to tap-major
 *                            (tap = (kh * 3 + kw) * Cin + c), bias [64] -> y [N][H][W][64] = max(conv + bias, 0), mask (nullable,
 *                            [N][H][W][16] bytes: the sign bits hk_bias_relu_fwd writes)
 *   hk_conv1_bias_relu_bwd   dy, mask, x -> dwt [9 Cin][64] (same layout as wt), dbias [64]; no input gradient (images need none);
 *                            workspace hk_conv1_ws_bytes(Cin) bytes; the masked gradient map is never written
 * Replaces the library convolution + hk_bias_relu_fwd and hk_bias_relu_bwd + the library's weight gradient for that layer. */
size_t hk_conv1_ws_bytes(int Cin);
int hk_conv1_bias_relu_fwd(const float* x, const float* wt, const float* bias, float* y, uint8_t* mask, int N, int H, int W, int Cin,
                           int Cout, hk_stream_t stream);
int hk_conv1_bias_relu_bwd(const float* dy, const uint8_t* mask, const float* x, float* dwt, float* dbias, int N, int H, int W, int Cin,
                           int Cout, void* ws, size_t ws_bytes, hk_stream_t stream);
/* Weight gradient of a 3 x 3 convolution whose input channel count is a multiple of 64 (stride 1, padding 1, dilation 1, fp32; every 3 x 3 layer of the trunk
 * but the first, model/backbone/vgg.py:24-57), on the matrix pipe with the whole 64 x 9 x 64 result of a (Cout slice, Cin slice) pair in
 * one workgroup's accumulators:
 *   x [N][H][W][Cin], dy [N][H][W][Cout] (channels_last maps) -> dw [Cout][3][3][Cin] (a channels_last [Cout, Cin, 3, 3] weight),
 *   dw[o][kh][kw][c] = sum over n, h, w of dy[n][h][w][o] x[n][h + kh - 1][w + kw - 1][c], zero outside the image.
 * Cin % 64 == 0, Cout % 64 == 0, Cout 9 Cin < 2^31, 16-byte aligned pointers, any N, H, W >= 1; HK_ERR_UNSUPPORTED (nothing launched)
 * otherwise, and for Cin > 64 with the knob "wrw_split" or "wrw_wide" at 0 (only the split form below reads a 64-channel slice out of
 * wider pixels).  Workspace hk_conv3x3_wrw_ws_bytes(Cin, Cout) bytes - a function of the two widths only: per-workgroup partial
 * results [workgroup][Cout][9][Cin], 512 of them for Cin = 64, max(1, 512 / slices) for more, 75.5 MB up to 512 slices -, added in
 * a fixed order: no atomics, no zero-fill, the same input gives the same bits.  Nothing outside the two maps is read.  Replaces the
 * library's weight gradient for the layers where it was measured faster (functional.conv3x3_wrw_route); the forward and the input
 * gradient stay the library's.
 * Two forms behind the one entry point (knob "wrw_split"; same workspace, same contract): the fp32-MFMA kernel, and a kernel that
 * splits every x and dy value into three bf16 pieces (hi + mid + lo = the value to 2^-27) and runs the six products of first and
 * second order on the bf16 matrix pipe with fp32 accumulation - within 3.9e-8 sum |x| |dy| of the exact result before accumulation,
 * the same 1e-6 sum |x| |dy| elementwise bound as the fp32 form after it, and 1.4 x faster at the trunk's shapes; by default the
 * layers where it was measured faster go to it.  Domain of that bound: finite inputs with |a| < 2^127 that are zero or no smaller
 * than about 2^-100 (below, the low pieces are bf16 subnormals and may be flushed).  A non-finite input makes every dw element it
 * touches non-finite in both forms - NaN in the split form where the fp32 form may give +-inf. */
size_t hk_conv3x3_wrw_ws_bytes(int Cin, int Cout);
int hk_conv3x3_wrw(const float* dy, const float* x, float* dw, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                   hk_stream_t stream);
int hk_add_relu_fwd(float* a, const float* b, long long n, hk_stream_t stream);
int hk_relu_mask_bwd(const float* dy, const float* y, float* g, long long n, hk_stream_t stream);

/* ------------------------------------------------------------------ AP-CNN ----
 * Attention pooling.  The reference materialises A = a_s*F + a_c*F and only ever
 * consumes its global average (cls3/4/5 start with AdaptiveAvgPool2d(1)), so
 *   gap [b,c] = mean_hw F[b,c,hw]              (also ChannelGate / Concate input)
 *   sgap[b,c] = mean_hw a_s[b,hw] F[b,c,hw]
 * and pooled = sgap + a_c * gap.  One pass over F.
 * replaces model/methods/APCNN.py:256,261,266 + :377-405 first layer + :533-538.
 *   f [B,C,HW] ; a_s [B,HW] (nullable: gap only) ; gap, sgap [B,C]
 */
int hk_att_pool_fwd(const float* f, const float* a_s, float* gap, float* sgap, int B, int C, int HW,
                    hk_stream_t stream);
/* df [B,C,HW] = (dsgap*a_s + dgap)/HW ; da_s [B,HW] = sum_c dsgap*F / HW (nullable with a_s).
 * a_s == NULL (plain GAP backward, df = dgap / HW): dsgap must be NULL too and f is not read (may be NULL). */
int hk_att_pool_bwd(const float* f, const float* a_s, const float* dgap, const float* dsgap, float* df,
                    float* da_s, int B, int C, int HW, hk_stream_t stream);

/* The three pyramid levels of PyramidAttentions.forward (APCNN.py:256-266) in one launch per direction: the levels'
 * poolings are independent (only the channel gates chain), and at 28 x 28 / 14 x 14 a launch per level is launch-bound.
 *   f_l [B,C,HW_l] ; a_l [B,HW_l] ; gap, sgap [3][B][C] (level-major) ; dgap, dsgap likewise ; df_l, da_l like f_l, a_l
 * Same arithmetic per row / column as hk_att_pool_fwd / _bwd: bit-identical results. */
int hk_att_pool3_fwd(const float* f0, const float* f1, const float* f2, const float* a0, const float* a1, const float* a2,
                     float* gap, float* sgap, int B, int C, int HW0, int HW1, int HW2, hk_stream_t stream);
int hk_att_pool3_bwd(const float* f0, const float* f1, const float* f2, const float* a0, const float* a1, const float* a2,
                     const float* dgap, const float* dsgap, float* df0, float* df1, float* df2, float* da0, float* da1,
                     float* da2, int B, int C, int HW0, int HW1, int HW2, hk_stream_t stream);

/* Attention -> ROI: border mask, one square anchor per cell, keep score > mean,
 * greedy NMS (IoU < thr keeps, area without +1, highest score first; ties:
 * highest cell index first), top-k, clamp to the image.  One workgroup per image,
 * no host synchronisation.
 * replaces model/methods/APCNN.py:444-476 (get_att_roi) + model/methods/nms.py:4-93.
 *   att   [B, h*w]      spatial attention (sigmoid output)
 *   rois  [B, topk, 5]  x1,y1,x2,y2,score (rows >= count are zero)
 *   count [B] int32     number of valid rows
 *   keep_r0..keep_c1: rows [r0,r1) x cols [c0,c1) that survive the border mask
 *       (= int(0.2*h), int(0.8*h), ... for 200 classes, 0.1/0.9 otherwise; the
 *       caller evaluates the reference's python expression, APCNN.py:451-455)
 */
int hk_att_roi_select(const float* att, float* rois, int32_t* count, int B, int h, int w,
                      int feature_stride, float anchor_size, int img_h, int img_w, int keep_r0, int keep_r1,
                      int keep_c0, int keep_c1, float iou_thr, int topk, hk_stream_t stream);

/* The three pyramid levels of one forward in ONE launch (grid B x 3): the reference calls get_att_roi once per level
 * (APCNN.py:256-266), each call a chain of top-k dependent rounds on one workgroup per image - side by side they take
 * as long as the longest.  Arrays of three (HOST arrays; the pointers in them are device pointers): att[i], rois[i],
 * count[i], h[i], w[i], feature_stride[i], anchor_size[i], topk[i]; keep[4 i .. 4 i + 3] = keep_r0, keep_r1, keep_c0,
 * keep_c1 of level i.  Results are those of three hk_att_roi_select calls, bit for bit. */
int hk_att_roi_select3(const float* const* att, float* const* rois, int32_t* const* count, int B, const int* h,
                       const int* w, const int* feature_stride, const float* anchor_size, int img_h, int img_w,
                       const int* keep, float iou_thr, const int* topk, hk_stream_t stream);

/* ROI-guided zoom-in (+ drop block): crop the union box of an image's ROIs,
 * zero one dropped ROI (training), rescale by c*h*w/sum(mask), bilinear resize
 * (align_corners=False) back to H x W.
 * replaces model/methods/APCNN.py:478-531 (get_roi_crop_feat).
 *   x    [B, C, H, W]
 *   box  [B, 4] fp32   x1,y1,x2,y2 of the union box in feature coordinates (already /scale)
 *   drop [B, 4] fp32   box to zero, or x2<=x1 for "no drop" (ignored when training == 0)
 *   y    [B, C, H, W]
 * Integer truncation of the box corners and the scale-rate rule follow the reference.
 */
int hk_roi_crop_resize_fwd(const float* x, const float* box, const float* drop, float* y, int B, int C, int H,
                           int W, int training, hk_stream_t stream);
int hk_roi_crop_resize_bwd(const float* dy, const float* box, const float* drop, float* dx, int B, int C, int H,
                           int W, int training, hk_stream_t stream);
/* Union / drop boxes from the fixed-layout ROI tables of hk_att_roi_select, on
 * device (no host read of the counts).
 *   rois_l [B,k_l,5], cnt_l [B] for the three pyramid levels; scale = 8 (coordinates are divided by it);
 *   u01 [B,2] uniforms in [0,1): u[.,0] picks the branch (<0.3 level-3 drop,
 *   <0.6 level-4 drop, else none), u[.,1] the ROI index floor(u*n).
 */
int hk_roi_boxes(const float* rois3, const int32_t* cnt3, int k3, const float* rois4, const int32_t* cnt4, int k4,
                 const float* rois5, const int32_t* cnt5, int k5, const float* u01, float scale, float* box,
                 float* drop, int B, hk_stream_t stream);

/* -------------------------------------------------------------------- OSME ----
 * One-squeeze multi-excitation: z = GAP(x) (one pass), and per attention p the
 * channel re-scaling s_p = m_p (.) x written for the following FC.
 * replaces model/methods/OSME.py:19-24 (avg_pool / broadcast mul).
 *   x [N,C,HW] ; z [N,C] ; m [P,N,C] sigmoid gates ; s [P,N,C,HW]
 */
int hk_osme_gap(const float* x, float* z, int N, int C, int HW, hk_stream_t stream);
int hk_osme_scale_fwd(const float* x, const float* m, float* s, int P, int N, int C, int HW, hk_stream_t stream);
/* dx [N,C,HW] = sum_p m_p * ds_p (+ dz/HW if dz != NULL) ; dm [P,N,C] = sum_hw ds_p * x */
int hk_osme_scale_bwd(const float* x, const float* m, const float* ds, const float* dz, float* dx, float* dm,
                      int P, int N, int C, int HW, hk_stream_t stream);

/* ------------------------------------------------------- classifier (8f-1) ----
 * out = y W^T + bias for the wide pooled vector and its backward.  Forward: the
 * feature axis is cut into slabs, partial results are added in slab order
 * (deterministic); wide classifiers (J % 32 == 0, enough work) stream y and W once
 * through LDS-DMA, other shapes take the generic f32-MFMA tiles.  Backward: streaming
 * kernels for up to 64 samples x 208 classes from 65536 features, plain tiles otherwise.
 * replaces nn.Linear at model/methods/BCNN.py:42,54 ; CBCNN.py:26,34 ; MPNCOV.py:31 ;
 * OSME.py:34,43 (same operand layouts: W is [K][J] as in nn.Linear.weight).
 *   y [B,J] ; w [K,J] ; bias [K] or NULL ; out [B,K] ; ws: hk_linear_ws_bytes(B,J,K)
 *   g [B,K] = dL/dout ; dy [B,J], dw [K,J], db [K]: each may be NULL (skipped)
 */
size_t hk_linear_ws_bytes(int B, int J, int K);
int hk_linear_fwd(const float* y, const float* w, const float* bias, float* out, int B, int J, int K, void* ws,
                  size_t ws_bytes, hk_stream_t stream);
int hk_linear_bwd(const float* y, const float* w, const float* g, float* dy, float* dw, float* db, int B, int J, int K,
                  hk_stream_t stream);
/* With a per-sample scale folded in (row_scale [B], e.g. the 1 / |z| of a pooled vector handed over unnormalised):
 *   out = row_scale[b] * (y W^T) + bias ;  dy = g W  (= dL/d(row_scale y)) ;  dW = (row_scale g)^T y ;  db = sum_b g.
 * hk_linear_bwd_scaled is served by the one-launch kernel only (up to 64 samples, up to 208 outputs, J % 4 == 0,
 * J >= 4096); HK_ERR_UNSUPPORTED - nothing launched - otherwise. */
int hk_linear_fwd_scaled(const float* y, const float* w, const float* bias, const float* row_scale, float* out, int B, int J,
                         int K, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_linear_bwd_scaled(const float* y, const float* w, const float* g, const float* row_scale, float* dy, float* dw, float* db,
                         int B, int J, int K, hk_stream_t stream);
/* hk_linear_fwd_scaled with the scale formed in the reduce launch: 1 / max(sqrt(sum of ss_part[b, 0 .. nparts)), 1e-12), written
 * to inv_norm [B] (the partial sums of |u|^2 of hk_bcnn_ssqrt_pool_fwd_parts: no launch in between). */
int hk_linear_fwd_ssq(const float* u, const float* w, const float* bias, const float* ss_part, int nparts, float* inv_norm,
                      float* out, int B, int J, int K, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------------ MAMC n-pairs loss (8f-4) ----
 * loss = NPairsLoss(parts, targets) and dx = d loss / d parts in one call.
 * replaces model/loss/MAMC_loss.py:34-90 (python loop over the b*p anchors).
 *   x [b*p, D] part features (row i = sample i / p, attention i % p) ; labels int32 [b]
 *   loss [1] ; dx [b*p, D] ; ws: hk_npairs_ws_bytes(b*p, D)
 */
size_t hk_npairs_ws_bytes(int n, int D);
int hk_npairs_loss(const float* x, const int32_t* labels, float* loss, float* dx, int b, int p, int D, void* ws,
                   size_t ws_bytes, hk_stream_t stream);

/* -------------------------------------------------- Peer-learning loss (WebFG baseline) ----
 * (loss_1, loss_2) = PeerLearningLoss(logits_1, logits_2, labels, drop_rate) and both logit gradients in one call.
 * replaces model/loss/peer_learning_loss.py:5-65 (about forty small launches and two host synchronisations).
 *   logits1, logits2 [N,C] ; labels int32 [N] ; drop_rate in [0, 1] (a host double)
 *   rows on which the two nets' argmax agree (n of them) are ranked by their cross entropy per net; net 1 keeps the
 *   m = (long long)((1 - drop_rate) n) rows net 2 finds easiest and the other way round; rows that disagree are always kept.
 *   loss [2]: mean cross entropy of each net over its kept rows (NaN when it keeps none) ;
 *   dl1, dl2 [N,C]: d loss_1 / d logits1, d loss_2 / d logits2 (zero rows where dropped; the selection is not differentiated) ;
 *   stats int32 [4]: n, m, count_1, count_2 - written on the device, nothing is read back ;
 *   a label outside [0, C) reads nothing and makes its row's cross entropy NaN.
 *   ws: hk_peer_loss_ws_bytes(N, C).  No host synchronisation, no allocation: capturable in a hipGraph.
 * One launch (both matrices resident in one workgroup's LDS) where 8 N C + 40 N + 128 bytes fit 160 KB, three launches
 * otherwise - bit-identical results (knob peer_form).  HK_ERR_BAD_ARG: null pointer, N or C <= 0, drop_rate outside [0, 1]
 * or NaN; HK_ERR_WORKSPACE: short workspace; HK_ERR_UNSUPPORTED: N > 2048 (what the selection kernel's LDS holds), or
 * peer_form 2 at a shape the resident form cannot hold. */
size_t hk_peer_loss_ws_bytes(int N, int C);
int hk_peer_loss(const float* logits1, const float* logits2, const int32_t* labels, double drop_rate, float* loss, float* dl1,
                 float* dl2, int32_t* stats, int N, int C, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------ APINet pairwise-interaction head ----
 * replaces model/methods/APINet.py:34-68,76-113 and model/loss/APINet_loss.py:29-39.  Every entry point: fp32, no host
 * synchronisation, no allocation (capturable in a hipGraph), no float atomics, fixed summation orders - the same bits on
 * every run.  HK_ERR_BAD_ARG: null pointer (masks may be NULL), B / D / R / C <= 0, scale not a positive finite number,
 * smoothing outside [0, 1], margin not finite; HK_ERR_UNSUPPORTED: 2 B > 65535 rows; HK_ERR_WORKSPACE: short workspace.
 *   pool [B,D] pooled vectors ; labels int32 [B] ; partner int32 [2B]
 *   hk_api_pairs: partner[i] = the nearest row j != i with labels[j] == labels[i], partner[B + i] = the nearest row with
 *     another label; squared Euclidean distance as sum (a - b)^2 in a fixed order (not the reference's cancelling
 *     -2ab + |a|^2 + |b|^2); ties go to the lowest index; a NaN distance counts as +inf; no candidate: 0.
 *   hk_api_gather_fwd: mutual [2B,2D], row r = [pool[r mod B] | pool[partner[r]]] ; hk_api_gather_bwd: dmutual -> dpool
 *     (row i gathers from the rows i, B + i and every r with partner[r] == i, r ascending).
 *   hk_api_interact_fwd: m [2B,D] ; f1 = pool[r mod B], f2 = pool[partner[r]], g1 = sigmoid(m f1), g2 = sigmoid(m f2) ;
 *     feats [8B,D] = [f1 (1 + g1) ; f2 (1 + g2) ; f1 (1 + g2) ; f2 (1 + g1)], each element times scale where
 *     masks uint8 [8B,D] is non-zero and 0 where it is zero (masks NULL: no dropout, scale ignored).
 *   hk_api_interact_bwd: dfeats [8B,D] -> dm [2B,D], dpool [B,D] (the same scatter order; one launch, gates recomputed).
 *   A partner outside [0, B) is never dereferenced: its f2 reads as zeros and it scatters nothing.
 *   hk_apinet_loss: self_logits, other_logits [R,C] (R = 4 x batch) ; labels int32 [R] = cat(labels1, labels2) ;
 *     loss [3] = total, CE, rank with CE = label-smoothed cross entropy averaged over the 2R rows of cat(self, other) and
 *     rank = mean_r max(0, p_other[r, y_r] - p_self[r, y_r] + margin) ; dself, dother [R,C] = d total / d logits.
 *     A label outside [0, C) reads nothing and makes the loss NaN.  ws: hk_apinet_loss_ws_bytes(R, C). */
int hk_api_pairs(const float* pool, const int32_t* labels, int32_t* partner, int B, int D, hk_stream_t stream);
int hk_api_gather_fwd(const float* pool, const int32_t* partner, float* mutual, int B, int D, hk_stream_t stream);
int hk_api_gather_bwd(const float* dmutual, const int32_t* partner, float* dpool, int B, int D, hk_stream_t stream);
int hk_api_interact_fwd(const float* pool, const int32_t* partner, const float* m, const uint8_t* masks, float scale,
                        float* feats, int B, int D, hk_stream_t stream);
int hk_api_interact_bwd(const float* pool, const int32_t* partner, const float* m, const uint8_t* masks, float scale,
                        const float* dfeats, float* dm, float* dpool, int B, int D, hk_stream_t stream);
size_t hk_apinet_loss_ws_bytes(int R, int C);
int hk_apinet_loss(const float* self_logits, const float* other_logits, const int32_t* labels, float smoothing, float margin,
                   float* loss, float* dself, float* dother, int R, int C, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------ NTS-Net head: proposal NMS, part crops, loss ----
 * replaces model/methods/NTS_Net/NTSNet.py:29-47 with anchors.py:63-90 (all scores copied to the host, a numpy greedy NMS
 * per image, a zero-padded copy of the batch, B x topN F.interpolate calls) and model/loss/NTS_loss.py:15-47 (an .item()
 * per part row, a Python loop over the proposals).  Every entry point: no host synchronisation, no allocation
 * (capturable in a hipGraph), no float atomics, fixed summation orders - the same bits on every run.
 * HK_ERR_BAD_ARG: null pointer, a size <= 0, pad < 0, iou_thresh NaN, smoothing outside [0, 1];
 * HK_ERR_UNSUPPORTED: A > 2048, B N > 65535 crops, B (N + 2) > 2^22 loss rows; HK_ERR_WORKSPACE: short workspace.
 *   hk_nts_nms: scores [B,A] ; anchors int32 [A,4] = y0, x0, y1, x1 -> index int32 [B,topn], boxes int32 [B,topn,4].
 *     hard_nms (anchors.py:63-90) per image: take the live anchor with the highest score, then keep a live anchor only if
 *     its IoU with it is < iou_thresh, strictly; IoU from corner differences without + 1, the intersection 0 when a side
 *     length is negative, evaluated in float64 as the reference evaluates it (0 / 0: suppressed).  Equal scores: the highest
 *     index.  A NaN score counts as -inf.  A slot that no live anchor can fill repeats the last chosen anchor (the
 *     reference returns a ragged array there); its `res.any()` stop is not reproduced.
 *   hk_nts_crop_resize: images [B,C,H,W] ; boxes int32 [B,N,4] in image coordinates (they may reach outside) ->
 *     out [B N,C,out_h,out_w]: the box clipped to [-pad, H + pad) x [-pad, W + pad), read from the image with zeros
 *     outside it, resized bilinearly with align_corners (src = dst (len - 1) / (out - 1), 0 when out == 1); an empty box
 *     gives zeros.  16-byte stores where out_w % 4 == 0 and out is 16-byte aligned.  No backward: the reference detaches.
 *   hk_nts_loss: raw_logits, concat_logits [B,C] ; part_logits [B,N,C] ; top_n_prob [B,N] ; labels int32 [B] ->
 *     loss [5] = total, raw CE, concat CE, part-class CE, rank ; draw, dconcat [B,C], dpart [B,N,C], dprob [B,N] = d total.
 *     The three CEs are label-smoothed means over their rows; part_loss[b,j] = -log_softmax(part_logits[b,j])[y_b] ;
 *     rank = (1 / B) sum_b sum_i sum_j relu(1 - s_bi + s_bj) [part_loss_bj > part_loss_bi] with s = top_n_prob; the
 *     indicator carries no gradient.  A label outside [0, C) reads nothing and makes the loss NaN.
 *     ws: hk_nts_loss_ws_bytes(B, N, C) (0 for sizes the call refuses). */
int hk_nts_nms(const float* scores, const int32_t* anchors, int32_t* index, int32_t* boxes, int B, int A, int topn,
               double iou_thresh, hk_stream_t stream);
int hk_nts_crop_resize(const float* images, const int32_t* boxes, float* out, int B, int N, int C, int H, int W, int pad,
                       int out_h, int out_w, hk_stream_t stream);
size_t hk_nts_loss_ws_bytes(int B, int N, int C);
int hk_nts_loss(const float* raw_logits, const float* concat_logits, const float* part_logits, const float* top_n_prob,
                const int32_t* labels, float smoothing, float* loss, float* draw, float* dconcat, float* dpart, float* dprob,
                int B, int N, int C, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------ CrossX head: multi-excitation block, upsample + add, loss ----
 * replaces model/methods/CrossX.py:109-119, :213-226 (a clone, P broadcast multiplies, P + 1 adds, P + 1 ReLUs, P pools and
 * a nearest-upsampled map per part as separate passes) and model/loss/CrossX_loss.py:15-64 (a P x P correlation matrix
 * filled on the host: 3 P^2 device-to-host copies).  Every entry point: no host synchronisation, no allocation (capturable
 * in a hipGraph), no float atomics, fixed summation orders - the same bits on every run, whatever the alignment.
 * HK_ERR_BAD_ARG: a null pointer that is not optional, a size <= 0, a mode other than 0 / 1; HK_ERR_UNSUPPORTED: P outside
 * [1, 3], sizes past the index range, an output size that is no multiple of the input's (up_add), B < 2 (loss).
 *   hk_crossx_me_fwd: out, res [N,C,HW] (the bottleneck's bn3 output and its residual) ; gates [P,N,C] (after the sigmoid)
 *     -> main_out [N,C,HW] = max(out + res, 0) ; parts [P,N,C,HW] = max(out * gates[p] + res, 0) (the product rounded, then
 *     the sum: no fma) ; pooled [P,N,C] = each part's spatial max (mode 0) or mean (mode 1) ; argmax int32 [P,N,C] (mode 0;
 *     may be NULL in mode 1): the lowest index of the maximum, as AdaptiveMaxPool2d.  HW is arbitrary; 16-byte accesses
 *     where HW % 4 == 0 and out, res, main_out and parts are 16-byte aligned.
 *   hk_crossx_me_bwd: d_main [N,C,HW], d_parts [P,N,C,HW], d_pooled [P,N,C], dz [N,C] (the gradient that reaches the
 *     squeeze GAP(out)) - each may be NULL, meaning zero - and the saved out, gates, main_out, parts, argmax ->
 *     g_p = [parts_p > 0] (d_parts_p + the pooled backward of d_pooled_p: d_pooled / HW everywhere (mode 1), d_pooled at the
 *     arg-max (mode 0); never a map) ;
 *     d_out = [main > 0] d_main + sum_p gates_p g_p + dz / HW ; d_res = [main > 0] d_main + sum_p g_p ;
 *     d_gates [P,N,C] = sum_hw g_p out.
 *   hk_crossx_up_add_fwd: y [N,C,Ho,Wo] = a + nearest_upsample(b [N,C,Hi,Wi]), Ho % Hi == 0 and Wo % Wi == 0 (source pixel
 *     = destination / factor, what F.interpolate(mode='nearest') takes for whole factors).
 *   hk_crossx_up_add_bwd: db [N,C,Hi,Wi] = the sum of dy over each source pixel's children (rows, then columns); the
 *     gradient of `a` is dy itself.
 *   hk_crossx_loss: ulti, plty, cmbn [B,K] ; labels int64 [B] ; f_ulti [P,B,C_ulti], f_plty [P,B,C_plty], f_cmbn [P,B,C_cmbn] ->
 *     loss [6] = total, cls, kl, reg_ulti, reg_plty, reg_cmbn ; d_* [B,K] and df_* (the features' shapes) = weight x d total.
 *     cls: the label-smoothed (0.1) cross entropy of ulti + plty + cmbn, mean over B ;
 *     kl = [KL(softmax(ulti) | softmax(plty)) + KL(softmax(ulti) | softmax(cmbn))] / B, with gradient into ulti through the
 *     target as well ; reg_l = gamma_l [sum_i (1 - |s_i|^2 / B^2) + sum_{i<j} s_i . s_j / B^2], s_i = sum_b x_i[b] / |x_i[b]| ;
 *     total = reg_ulti + reg_plty + reg_cmbn + kl + cls.  A zero feature row gives NaN; a label outside [0, K) reads
 *     nothing and makes cls and total NaN.  ws: hk_crossx_loss_ws_bytes(B, K, P, C_ulti, C_plty, C_cmbn) (0 for sizes the
 *     call refuses). */
int hk_crossx_me_fwd(const float* out, const float* res, const float* gates, float* main_out, float* parts, float* pooled,
                     int32_t* argmax, int P, int N, int C, int HW, int mode, hk_stream_t stream);
int hk_crossx_me_bwd(const float* d_main, const float* d_parts, const float* d_pooled, const int32_t* argmax, const float* dz,
                     const float* out, const float* gates, const float* main_saved, const float* parts, float* d_out,
                     float* d_res, float* d_gates, int P, int N, int C, int HW, int mode, hk_stream_t stream);
int hk_crossx_up_add_fwd(const float* a, const float* b, float* y, int N, int C, int Hi, int Wi, int Ho, int Wo,
                         hk_stream_t stream);
int hk_crossx_up_add_bwd(const float* dy, float* db, int N, int C, int Hi, int Wi, int Ho, int Wo, hk_stream_t stream);
size_t hk_crossx_loss_ws_bytes(int B, int K, int P, int C_ulti, int C_plty, int C_cmbn);
int hk_crossx_loss(const float* ulti, const float* plty, const float* cmbn, const int64_t* labels, const float* f_ulti,
                   const float* f_plty, const float* f_cmbn, float gamma_ulti, float gamma_plty, float gamma_cmbn, float weight,
                   float* loss, float* d_ulti, float* d_plty, float* d_cmbn, float* df_ulti, float* df_plty, float* df_cmbn, int B,
                   int K, int P, int C_ulti, int C_plty, int C_cmbn, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------ DCL head, loss and swap law ----
 * replaces model/methods/DCL.py:33-39 (Convmask, AvgPool2d(2), tanh and AdaptiveAvgPool2d(1) as two reads of the last map,
 * two full-size map gradients and an add), model/loss/DCL_loss.py:17-20 (two label-smoothed cross entropies, an L1 term
 * and their sum) and dataset/dataset_DCL.py:48-62 (98 ImageStat means and a 49 x 49 search per image, in Python).  Every
 * entry point: no host synchronisation, no allocation (capturable in a hipGraph), no atomics, fixed summation orders - the
 * same bits on every run, whatever the alignment.  HK_ERR_BAD_ARG: a null pointer that is not optional, a size <= 0;
 * HK_ERR_WORKSPACE: a short workspace (reported before an unsupported size); HK_ERR_UNSUPPORTED: H < 2 or W < 2 (head),
 * W < gx or H < gy, more than 2048 patches or more than 2^24 pixels per image (law), sizes past the index range.
 *   hk_dcl_head_fwd: x [B,C,H,W] dense NCHW ; w [C] (Convmask.weight) ; bias [1] on the DEVICE -> pooled [B,C] = the mean
 *     over H W ; mask [B,(H/2)(W/2)] = tanh(avgpool2x2(sum_c w[c] x[b,c] + bias)), floor semantics: the last row / column
 *     of an odd side enters pooled only.  x is read once; two launches.  16-byte accesses where H W % 4 == 0 and x is
 *     16-byte aligned.  ws: hk_dcl_head_fwd_ws_bytes(B, C, H, W) (0 for sizes the call refuses).
 *   hk_dcl_head_bwd: the saved mask, d_pooled [B,C] and d_mask [B,M] (each may be NULL, meaning zero) -> dx [B,C,H,W] =
 *     d_pooled / HW + w[c] g[b,h/2,w/2] / 4 with g = d_mask (1 - mask^2) (the second term only inside the pooled area) ;
 *     dw [C] = sum_b sum_hw x g / 4 ; dbias [1] = sum g.  Each output may be NULL; each one given is written in full.  x
 *     is read once (only when dw is wanted), dx written once; at most two launches.  ws: hk_dcl_head_bwd_ws_bytes.
 *   hk_dcl_loss: logits [N,K], swap_logits [N,S], mask [N,M] ; labels, labels_swap int64 [N] ; law [N,M] -> loss [4] =
 *     total, ce, swap, law with ce / swap the label-smoothed (`smoothing`) cross entropies (mean over N), law =
 *     mean |mask - law| and total = alpha ce + beta swap + gamma law ; d_logits, d_swap, d_mask = weight x d total (d_mask
 *     is exactly 0 where mask == law).  A label outside its range reads nothing and makes that term and total NaN.  One
 *     launch, no workspace.
 *   hk_dcl_swap_law: unswapped, swapped uint8 [N,H,W,3] ; bounds_x int32 [gx + 1], bounds_y int32 [gy + 1] (device; patch
 *     (i, j) spans columns [bounds_x[i], bounds_x[i+1]) and rows [bounds_y[j], bounds_y[j+1]), entries clamped to the image)
 *     -> index int32 [N, gx gy]: for each swapped patch (row-major) the unswapped patch whose value ((0 + s_r / n) + s_g / n)
 *     + s_b / n (exact integer band totals, float64 divisions and additions, as Python's sum() of ImageStat's means) is
 *     nearest, the lowest index on ties ; law float [N, gx gy] = (index - (gx gy) / 2) / (gx gy), divided in float64. */
size_t hk_dcl_head_fwd_ws_bytes(int B, int C, int H, int W);
int hk_dcl_head_fwd(const float* x, const float* w, const float* bias, float* pooled, float* mask, int B, int C, int H, int W,
                    void* ws, size_t ws_bytes, hk_stream_t stream);
size_t hk_dcl_head_bwd_ws_bytes(int B, int C, int H, int W);
int hk_dcl_head_bwd(const float* x, const float* w, const float* mask, const float* d_pooled, const float* d_mask, float* dx,
                    float* dw, float* dbias, int B, int C, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream);
int hk_dcl_loss(const float* logits, const float* swap_logits, const float* mask, const int64_t* labels,
                const int64_t* labels_swap, const float* law, float alpha, float beta, float gamma, float smoothing, float weight,
                float* loss, float* d_logits, float* d_swap, float* d_mask, int N, int K, int S, int M, hk_stream_t stream);
int hk_dcl_swap_law(const uint8_t* unswapped, const uint8_t* swapped, const int32_t* bounds_x, const int32_t* bounds_y,
                    int32_t* index, float* law, int N, int H, int W, int gx, int gy, hk_stream_t stream);

/* ------------------------------------------------ CIN channel interaction (8f-2) ----
 * SCI: W = softmax_rows(-X X^T / HW), Y = W X ; CCI: Yc[b] = |W[b] - w_b W[(b + B/2) % B]| X[b].
 * replaces the bmm / softmax / abs / bmm parts of ChannelInteractionModule.forward,
 * model/methods/CIN.py:24-60 (conv 3x3, residual and the 1-output fc stay on PyTorch).
 *   x, y, dy, dx [B,C,HW] ; w, dw [B,C,C] ; wt, dwt [B] ; B even for the CCI pair.
 *   hk_cin_sci_bwd: dwbuf [B,C,C] scratch; holds the gradient reaching W from the CCI
 *   branch on entry when has_extra != 0 (it is overwritten).
 *   hk_cin_sci_fwd, C % 64 == 0: ONE kernel at 7x7 / 8x8 / 6x6 maps (scores recomputed on the matrix pipe, W written
 *   once); at 14x14 / 12x12 / 10x10 maps and C % 128 == 0 three - Gram panel kernel, row statistics, softmax applied on the way into the
 *   second product (W written once, in place of the scores); any other shape: Gram, row softmax, product on the generic tile.
 *   hk_cin_sci_bwd at those larger maps: W^T dY and (dG + dG^T) X / HW each stream their C x C operand once through the
 *   forward's pipeline (the second as ONE product).
 */
int hk_cin_sci_fwd(const float* x, float* w, float* y, int B, int C, int HW, hk_stream_t stream);
int hk_cin_sci_bwd(const float* x, const float* w, const float* dy, float* dwbuf, int has_extra, float* dx, int B, int C,
                   int HW, hk_stream_t stream);
int hk_cin_cci_fwd(const float* x, const float* w, const float* wt, float* y, int B, int C, int HW, hk_stream_t stream);
size_t hk_cin_cci_ws_bytes(int B, int C);
int hk_cin_cci_bwd(const float* x, const float* w, const float* wt, const float* dy, float* dx, float* dw, float* dwt,
                   int B, int C, int HW, void* ws, size_t ws_bytes, hk_stream_t stream);

/* ------------------------------------------------------ input finalisation (8f-3) ----
 * uint8 HWC crops -> normalised fp32 images on the device, with the random-erasing
 * rectangle applied: PILToTensor + ConvertImageDtype + Normalize + RandomErasing(value 0)
 * of dataset/transforms.py:38-46 in one pass; bit-identical to the CPU order of operations.
 *   u8 [B,H,W,3] (device) ; mean3 / std3: HOST pointers to three floats ;
 *   erase int32 [B,4] = top, left, h, w (device; h or w <= 0: nothing erased; NULL: none)
 *   out fp32 [B,3,H,W], or the channels_last storage of the same tensor ([B,H,W,3]) if channels_last != 0
 */
int hk_image_finalize(const uint8_t* u8, const float* mean3, const float* std3, const int32_t* erase, float* out, int B,
                      int H, int W, int channels_last, hk_stream_t stream);

/* ------------------------------------------------------- generic primitive ----
 * Batched fp32 GEMM on the f32 MFMA path (exact fp32 fma chain):
 *   C[b] = alpha * op(A[b]) op(B[b]) + beta * C[b] + diag * I
 * row-major operands; trans_a: A stored K x M; trans_b: B stored N x K.
 * Exposed for the tests and for composing the Newton-Schulz chain.
 */
int hk_bgemm_f32(const float* a, int lda, long long stride_a, int trans_a, const float* b, int ldb,
                 long long stride_b, int trans_b, float* c, int ldc, long long stride_c, int M, int N, int K,
                 int batch, float alpha, float beta, float diag, hk_stream_t stream);

#ifdef __cplusplus
}
#endif

#include "hawkeye_conv.h" /* the trunk's forward and input gradient */
#include "hawkeye_conv_epi.h" /* ... with the trunk's epilogue passes done inside those kernels */
#include "hawkeye_conv_tile.h" /* ... and how those kernels tile a map */
#include "hawkeye_conv_pool.h" /* the weight gradient of the trunk's pooled layers from the pooled gradient */
#include "hawkeye_interp.h" /* the InterpParts plugin: region grouping and the shaping loss */
#include "hawkeye_mge.h" /* the MGE-CNN plugin: part pool, Grad-CAM box and the criterion */

#endif /* HAWKEYE_HIP_H */
