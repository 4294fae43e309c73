/*
 * hawkeye_interp.h - the InterpParts plugin's entry points (csrc/interp.hip): the grouping unit on the layer-3 map, forward and
 * backward, and the criterion; included by hawkeye_hip.h, whose conventions hold (raw device pointers, fp32, dense row-major
 * tensors, a workspace passed in, HK_ERR_* codes, everything enqueued on `stream`, no host synchronisation).  Bound from
 * hawkeye_amd/_lib.py: INTERP_SIGNATURES.
 */
#ifndef HAWKEYE_INTERP_H
#define HAWKEYE_INTERP_H

#include "hawkeye_hip.h" /* hk_stream_t, HK_ERR_*; that header includes this one at its end */

#ifdef __cplusplus
extern "C" {
#endif

/* replaces GroupingUnit.forward, model/methods/Interp_Parts.py:56-122, and its autograd graph.
 *   x [N,C,H,W] ; centres [K,C] (GroupingUnit.weight) ; smooth [K] (before the sigmoid).  beta = sigmoid(smooth), sigma = sqrt(beta / 2),
 *   l[k,p] = min(0, 2 <c_k, x_p> - |x_p|^2 - |c_k|^2) / beta_k, a = softmax_k(l), S_k = sum_p a[k,p], q = a X^T,
 *   o_k = (q_k / max(S_k, 1e-5) - c_k) / sigma_k, y_k = o_k / max(|o_k|, 1e-12).
 *   hk_ip_group_fwd -> outputs_t [N,C,K] = y transposed as the reference returns it, assign [N,K,H,W] = a, and for the backward
 *     S [N,K] (before the clamp) and nrm [N,K] = |o_k|.  x is read once; three launches (centres, the map, the finish).
 *   hk_ip_group_bwd: d_outputs_t [N,C,K] and d_assign [N,K,H,W], each may be NULL, meaning zeros (the same bits as passing zeros)
 *     -> dx [N,C,H,W], d_centres [K,C], d_smooth [K]; each may be NULL: not wanted.  x is read once, dx written once; at most four launches.
 *   1 <= K <= 32, C a multiple of 64 up to 1024, any N, H, W >= 1: anything else HK_ERR_UNSUPPORTED before any launch.  The 16-byte
 *   path (H W % 4 == 0 and 16-byte aligned maps) and the scalar one give the same bits; so do two runs: no atomics, every sum in a
 *   fixed order.  ws: hk_ip_group_*_ws_bytes (0 for sizes the call refuses), 16-byte aligned; HK_ERR_WORKSPACE if short.  The main
 *   launches use up to 158 KiB of LDS: a failure to raise the launch attribute is returned as the HIP error it is. */
size_t hk_ip_group_fwd_ws_bytes(int N, int C, int K, int H, int W);
int hk_ip_group_fwd(const float* x, const float* centres, const float* smooth, float* outputs_t, float* assign, float* S, float* nrm,
                    int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream);
size_t hk_ip_group_bwd_ws_bytes(int N, int C, int K, int H, int W);
int hk_ip_group_bwd(const float* x, const float* centres, const float* smooth, const float* outputs_t, const float* S, const float* nrm,
                    const float* d_outputs_t, const float* d_assign, float* dx, float* d_centres, float* d_smooth, int N, int C, int K,
                    int H, int W, void* ws, size_t ws_bytes, hk_stream_t stream);

/* replaces InterpPartsLoss.__call__ and ShapingLoss, model/loss/InterpParts_loss.py:24-138.
 *   logits [N,classes] ; labels int64 [N] ; assign [N,K,H,W] ; window [(2 radius + 1)^2] (radius 0: one weight) ; prior [N], ascending
 *   (the Beta prior's inverse CDF at the N grid points; it depends on N alone, so the caller keeps it on the device) ; coeff
 *   -> terms [3] = {cross entropy + coeff shaping, cross entropy, shaping}, d_logits [N,classes], d_assign [N,K,H,W] dense.
 *   shaping = mean over (rank, part) of |log(emp + 1e-5) - log(prior[rank] + 1e-5)|, emp = the N maxima of a part's "valid" correlation
 *   with the window, ascending.  Ties: the lowest flat index holds a tied maximum, the lower sample takes the lower rank.  d_assign is
 *   coeff sign(.) / (emp + 1e-5) / (N K) times the window at the argmax and exactly zero elsewhere.  A label out of range: NaN terms,
 *   nothing read out of bounds.  H or W below 2 radius + 1: HK_ERR_BAD_ARG.  Two launches.  ws: hk_ip_loss_ws_bytes(N, K). */
size_t hk_ip_loss_ws_bytes(int N, int K);
int hk_ip_loss(const float* logits, const int64_t* labels, const float* assign, const float* window, const float* prior, float coeff,
               float* terms, float* d_logits, float* d_assign, int N, int classes, int K, int H, int W, int radius, void* ws,
               size_t ws_bytes, hk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HAWKEYE_INTERP_H */
