"""ctypes binding of libhawkeye_hip.so (C ABI declared in include/hawkeye_hip.h).

The library is loaded AFTER torch so that its NEEDED libamdhip64.so.7 resolves to
the HIP runtime torch already mapped (one runtime => torch's stream handles are
valid inside the kernels' launches).  There is no CPU fallback: if the library
is missing or a tensor is not on a HIP device, the op raises.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported before the .so is dlopen'ed)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libhawkeye_hip.so')

c_f = ctypes.c_void_p       # device float*
c_i = ctypes.c_int
c_sz = ctypes.c_size_t
c_ll = ctypes.c_longlong
c_fl = ctypes.c_float

# name -> (restype, argtypes); mirrors include/hawkeye_hip.h one to one
SIGNATURES = {
    'hk_version': (ctypes.c_char_p, []),
    'hk_tuning_set': (c_i, [ctypes.c_char_p, c_i]),
    'hk_tuning_get': (c_i, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    'hk_bcnn_pool_ws_bytes': (c_sz, [c_i, c_i, c_i]),
    'hk_bcnn_pool_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_pool_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_pool_bwd_tdot': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_ws_bytes': (c_sz, [c_i, c_i, c_i]),
    'hk_bcnn_ssqrt_pool_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_pool_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_pool_fwd_parts': (c_i, [c_f, c_f, c_f, ctypes.c_void_p, c_i, c_i, c_i, c_f]),     # (4th: int* on the HOST - pass ctypes.byref)
    'hk_linear_fwd_ssq': (c_i, [c_f, c_f, c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_pool_bwd_tdot': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_pool_fwd_unscaled': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_ssqrt_pool_bwd_unscaled': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_colsum_norm': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_bcnn_gram_norm': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_bcnn_bwd_gemm': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_bcnn_bwd_rank1': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_cov_pool_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_cov_pool_bwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_ns_sqrtm_ws_bytes': (c_sz, [c_i, c_i, c_i, c_i]),
    'hk_ns_sqrtm_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_ns_sqrtm_fwd_sym': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_ns_sqrtm_triu_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_ns_sqrtm_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_ns_sqrtm_bwd_general': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_triu_vec_fwd': (c_i, [c_f, c_f, c_i, c_i, c_f]),
    'hk_triu_vec_bwd': (c_i, [c_f, c_f, c_i, c_i, c_f]),
    'hk_cbp_plan_bytes': (c_sz, [c_i, c_i]),
    'hk_cbp_plan_build': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f]),
    'hk_cbp_plan_destroy': (c_i, [c_f]),
    'hk_cbp_ws_bytes': (c_sz, [c_i, c_i, c_i, c_i]),
    'hk_cbp_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_cbp_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_trunk_ws_bytes': (c_sz, [c_i]),
    'hk_bias_relu_fwd': (c_i, [c_f, c_f, c_f, c_ll, c_i, c_f]),
    'hk_bias_relu_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_ll, c_i, c_f, c_sz, c_f]),
    'hk_bias_relu_pool_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_bias_relu_pool_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv1_ws_bytes': (c_sz, [c_i]),
    'hk_conv1_bias_relu_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    'hk_conv1_bias_relu_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv3x3_wrw_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_conv3x3_wrw': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_add_relu_fwd': (c_i, [c_f, c_f, c_ll, c_f]),
    'hk_relu_mask_bwd': (c_i, [c_f, c_f, c_f, c_ll, c_f]),
    'hk_cbp_rect_plan_bytes': (c_sz, [c_i, c_i, c_i]),
    'hk_cbp_rect_plan_build': (c_i, [c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_f, c_f]),
    'hk_cbp_rect_bin_matrix': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_cbp_rect_unbin_matrix': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_cbp_rect_loc_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    'hk_cbp_rect_loc_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    'hk_att_pool_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_att_pool_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_att_pool3_fwd': (c_i, [c_f] * 8 + [c_i] * 5 + [c_f]),
    'hk_att_pool3_bwd': (c_i, [c_f] * 14 + [c_i] * 5 + [c_f]),
    'hk_att_roi_select3': (c_i, [c_f, c_f, c_f, c_i, c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_fl, c_f, c_f]),     # host arrays passed as void*
    'hk_att_roi_select': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_i, c_i, c_i, c_i, c_i, c_i, c_fl, c_i, c_f]),
    'hk_roi_crop_resize_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    'hk_roi_crop_resize_bwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    'hk_roi_boxes': (c_i, [c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_f, c_i, c_f, c_fl, c_f, c_f, c_i, c_f]),
    'hk_osme_gap': (c_i, [c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_osme_scale_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_osme_scale_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_linear_ws_bytes': (c_sz, [c_i, c_i, c_i]),
    'hk_linear_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_linear_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_linear_fwd_scaled': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_linear_bwd_scaled': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_npairs_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_npairs_loss': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_peer_loss_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_peer_loss': (c_i, [c_f, c_f, c_f, ctypes.c_double, c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_sz, c_f]),
    'hk_api_pairs': (c_i, [c_f, c_f, c_f, c_i, c_i, c_f]),
    'hk_api_gather_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_f]),
    'hk_api_gather_bwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_f]),
    'hk_api_interact_fwd': (c_i, [c_f, c_f, c_f, c_f, c_fl, c_f, c_i, c_i, c_f]),
    'hk_api_interact_bwd': (c_i, [c_f, c_f, c_f, c_f, c_fl, c_f, c_f, c_f, c_i, c_i, c_f]),
    'hk_apinet_loss_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_apinet_loss': (c_i, [c_f, c_f, c_f, c_fl, c_fl, c_f, c_f, c_f, c_i, c_i, c_f, c_sz, c_f]),
    'hk_nts_nms': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, ctypes.c_double, c_f]),
    'hk_nts_crop_resize': (c_i, [c_f, c_f, c_f] + [c_i] * 8 + [c_f]),
    'hk_nts_loss_ws_bytes': (c_sz, [c_i, c_i, c_i]),
    'hk_nts_loss': (c_i, [c_f] * 5 + [c_fl] + [c_f] * 5 + [c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_crossx_me_fwd': (c_i, [c_f] * 7 + [c_i] * 5 + [c_f]),
    'hk_crossx_me_bwd': (c_i, [c_f] * 12 + [c_i] * 5 + [c_f]),
    'hk_crossx_up_add_fwd': (c_i, [c_f] * 3 + [c_i] * 6 + [c_f]),
    'hk_crossx_up_add_bwd': (c_i, [c_f] * 2 + [c_i] * 6 + [c_f]),
    'hk_crossx_loss_ws_bytes': (c_sz, [c_i] * 6),
    'hk_crossx_loss': (c_i, [c_f] * 7 + [c_fl] * 4 + [c_f] * 7 + [c_i] * 6 + [c_f, c_sz, c_f]),
    'hk_cin_sci_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_cin_sci_bwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_f]),
    'hk_cin_cci_fwd': (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    'hk_cin_cci_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_cin_cci_bwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_image_finalize': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    'hk_bgemm_f32': (c_i, [c_f, c_i, c_ll, c_i, c_f, c_i, c_ll, c_i, c_f, c_i, c_ll, c_i, c_i, c_i, c_i,
                           c_fl, c_fl, c_fl, c_f]),
    'hk_dcl_head_fwd_ws_bytes': (c_sz, [c_i] * 4),
    'hk_dcl_head_fwd': (c_i, [c_f] * 5 + [c_i] * 4 + [c_f, c_sz, c_f]),
    'hk_dcl_head_bwd_ws_bytes': (c_sz, [c_i] * 4),
    'hk_dcl_head_bwd': (c_i, [c_f] * 8 + [c_i] * 4 + [c_f, c_sz, c_f]),
    'hk_dcl_loss': (c_i, [c_f] * 6 + [c_fl] * 5 + [c_f] * 4 + [c_i] * 4 + [c_f]),
    'hk_dcl_swap_law': (c_i, [c_f] * 6 + [c_i] * 5 + [c_f]),
}

# the trunk's forward and input gradient; mirrors include/hawkeye_conv.h one to one (a table of its own, like the header)
TRUNK_SIGNATURES = {
    'hk_conv3x3_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_conv3x3_fwd': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv3x3_bwd_data': (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
}

# ... with the trunk's epilogue passes inside those kernels; mirrors include/hawkeye_conv_epi.h one to one
TRUNK_EPI_SIGNATURES = {
    'hk_conv3x3_bias_relu_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv3x3_bias_relu_pool_fwd': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv3x3_masked_ws_bytes': (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    'hk_conv3x3_masked_bwd_data': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
}

# ... and how those kernels tile a map (knob `conv_tile`); mirrors include/hawkeye_conv_tile.h one to one
TRUNK_TILE_SIGNATURES = {
    'hk_conv3x3_tile_plan': (c_i, [c_i, c_i, c_i, c_i, c_f]),     # (5th: int[12] on the HOST)
}

# ... and the weight gradient of the trunk's pooled layers from the pooled gradient (knob `wrw_pool`); mirrors include/hawkeye_conv_pool.h
TRUNK_POOL_SIGNATURES = {
    'hk_conv3x3_wrw_pooled': (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_sz, c_f]),
    'hk_conv3x3_wrw_pooled_served': (c_i, [c_i] * 5),
    'hk_conv3x3_wrw_pooled_plan': (c_i, [c_i] * 5 + [c_f]),     # (6th: int[5] on the HOST)
}

# the InterpParts plugin's grouping unit and criterion; mirrors include/hawkeye_interp.h one to one
INTERP_SIGNATURES = {
    'hk_ip_group_fwd_ws_bytes': (c_sz, [c_i] * 5),
    'hk_ip_group_fwd': (c_i, [c_f] * 7 + [c_i] * 5 + [c_f, c_sz, c_f]),
    'hk_ip_group_bwd_ws_bytes': (c_sz, [c_i] * 5),
    'hk_ip_group_bwd': (c_i, [c_f] * 11 + [c_i] * 5 + [c_f, c_sz, c_f]),
    'hk_ip_loss_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_ip_loss': (c_i, [c_f] * 5 + [c_fl] + [c_f] * 3 + [c_i] * 6 + [c_f, c_sz, c_f]),
}

# the MGE-CNN plugin's part pool, Grad-CAM box and criterion; mirrors include/hawkeye_mge.h one to one
MGE_SIGNATURES = {
    'hk_mge_partpool_fwd_ws_bytes': (c_sz, [c_i] * 5),
    'hk_mge_partpool_fwd': (c_i, [c_f] * 5 + [c_i] * 5 + [c_f, c_sz, c_f]),
    'hk_mge_partpool_bwd': (c_i, [c_f] * 6 + [c_i] * 5 + [c_f]),
    'hk_mge_cam_bbox': (c_i, [c_f] * 4 + [c_i] * 5 + [c_fl, c_i, c_f]),
    'hk_mge_loss_ws_bytes': (c_sz, [c_i, c_i]),
    'hk_mge_loss': (c_i, [c_f, c_f, c_fl, c_f, c_f, c_i, c_i, c_i, c_f, c_sz, c_f]),     # (1st and 5th: HOST arrays of K device pointers)
}


def attach(lib):
    """Give every function of SIGNATURES, TRUNK_SIGNATURES, TRUNK_EPI_SIGNATURES, TRUNK_TILE_SIGNATURES, TRUNK_POOL_SIGNATURES, INTERP_SIGNATURES and MGE_SIGNATURES its
    prototype on a library object (the gfx950 build, or whatever stands in for it).  Returns the library."""
    for name, (res, args) in list(SIGNATURES.items()) + list(TRUNK_SIGNATURES.items()) + list(TRUNK_EPI_SIGNATURES.items()) + \
            list(TRUNK_TILE_SIGNATURES.items()) + list(TRUNK_POOL_SIGNATURES.items()) + list(INTERP_SIGNATURES.items()) + list(MGE_SIGNATURES.items()):
        fn = getattr(lib, name)   # AttributeError => header/library drifted apart
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


HK_OK, HK_ERR_BAD_ARG, HK_ERR_WORKSPACE, HK_ERR_UNSUPPORTED = 0, -1, -2, -3      # hk_common.h


class HawkeyeHipError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library and attach prototypes.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HawkeyeHipError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C hawkeye_amd/csrc` (there is no CPU fallback for the HIP ops)')
    _lib = attach(ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL))
    return _lib


def check(rc, what):
    if rc != 0:
        raise HawkeyeHipError(f'{what} failed with code {rc} '
                              f'({"HK_ERR" if rc < 0 else "hipError_t"})')


def ptr(t):
    """Device pointer of a contiguous fp32/int32 HIP tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HawkeyeHipError('hawkeye_amd ops run on MI355X only: got a CPU tensor (no CPU fallback; '
                              'the CPU reference lives in oracle/ and is test infrastructure)')
    # dense memory: row-major, or NHWC behind a [N,C,H,W] view (the trunk epilogues take channels_last maps as they lie)
    if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
        raise HawkeyeHipError('internal error: non-contiguous tensor handed to the C ABI')
    if t.device.index != torch.cuda.current_device():
        # the library launches on the CURRENT device's stream (one process per GPU: Trainer / Tester / bench.py call
        # torch.cuda.set_device once); a tensor of another device would be touched from the wrong stream
        raise HawkeyeHipError(f'tensor lives on {t.device} but the current HIP device is cuda:{torch.cuda.current_device()}: '
                              f'call torch.cuda.set_device({t.device.index}) (one process per GPU) or wrap the call in '
                              f'`with torch.cuda.device(...)`')
    return ctypes.c_void_p(t.data_ptr())


class tuning:
    """`with tuning(ns_tn=64, bcnn_generic=1): ...` - flips A/B knobs of the library (hk_tuning_set) for tests and
    benchmarks and restores the previous values on exit.  The product path uses it for one knob only: `conv_mfma`, around a call of
    the trunk's 3 x 3 kernels that its measured table routes to the 16 x 16 x 32 MFMA (functional._conv3x3_mfma)."""

    def __init__(self, **knobs):
        self.knobs = knobs
        self.saved = {}

    def __enter__(self):
        lib = load()
        for name, value in self.knobs.items():
            old = ctypes.c_int(0)
            check(lib.hk_tuning_get(name.encode(), ctypes.byref(old)), f'hk_tuning_get({name})')
            self.saved[name] = old.value
            check(lib.hk_tuning_set(name.encode(), int(value)), f'hk_tuning_set({name})')
        return self

    def __exit__(self, *exc):
        lib = load()
        for name, value in self.saved.items():
            lib.hk_tuning_set(name.encode(), value)
        return False


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
