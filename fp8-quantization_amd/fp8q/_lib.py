"""ctypes binding of libfp8q_hip.so (include/fp8q.h).  There is NO fallback: if the library is
missing or fails to load, importing an op raises -- the product never runs on a CPU path."""
import ctypes
import os

from . import build as _build

_lib = None

_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_vp = ctypes.c_void_p
_f = ctypes.c_float
_i = ctypes.c_int



class MseState(ctypes.Structure):
    """fp8q_mse_state (include/fp8q.h): device pointers of one MSE estimator's persistent state"""
    _fields_ = [("cur_min", _vp), ("cur_max", _vp), ("absmax", _vp), ("grid", _vp), ("mses", _vp), ("maxval", _vp),
                ("xmin", _vp), ("mbits", _vp), ("vote", _vp)]


class MseRouteInfo(ctypes.Structure):
    """fp8q_mse_route_info (include/fp8q.h): the kernel a K4 call reaches and the choices its launcher takes from the shape"""
    _fields_ = [("kernel", _i), ("finish", _i), ("nsplit", _i64), ("tiles_per_wg", _i), ("part_wgs", _i), ("slice_min", _i),
                ("moments_threads", _i), ("n_superblocks", _i64), ("top_scan", _i), ("reserved", _i)]


class AffinePre(ctypes.Structure):
    """fp8q_affine_pre (include/fp8q.h): the BN + activation (+ residual) in front of a per-tensor MSE-calibrated quantizer"""
    _fields_ = [("x", _vp), ("residual", _vp), ("alpha_beta", _vp), ("N", _i64), ("C", _i64), ("HW", _i64), ("act", _i)]


class AffineRouteInfo(ctypes.Structure):
    """fp8q_affine_route_info (include/fp8q.h): the kernel the fused FP8 epilogue reaches for a shape and its launches"""
    _fields_ = [("kernel", _i), ("direct", _i), ("cpp", _i), ("launches", _i), ("grid_x", _i64), ("grid_y", _i64)]


class RowsRouteInfo(ctypes.Structure):
    """fp8q_rows_route_info (include/fp8q.h): the row kernel a quantize / min-max / fused call reaches and its launcher's choices"""
    _fields_ = [("kernel", _i), ("nontemporal", _i), ("small", _i), ("lut", _i), ("lanes", _i), ("slots", _i), ("group", _i),
                ("nch", _i), ("rows_per_block", _i), ("nsplit", _i), ("launches", _i), ("reserved", _i), ("grid_x", _i64),
                ("grid_y", _i64)]


class CodecRouteInfo(ctypes.Structure):
    """fp8q_codec_route_info (include/fp8q.h): the kernel a storage-code encode / decode reaches and its launcher's choices"""
    _fields_ = [("kernel", _i), ("nontemporal", _i), ("nch", _i), ("wide", _i), ("launches", _i), ("reserved", _i),
                ("grid_x", _i64), ("grid_y", _i64), ("steps", _i64)]


class ChunkRouteInfo(ctypes.Structure):
    """fp8q_chunk_route_info (include/fp8q.h): the launch geometry of a chunked INT / hardware-FP8 kernel"""
    _fields_ = [("per_channel", _i), ("rows_per_chunk", _i), ("two_row", _i), ("vec", _i), ("nontemporal", _i),
                ("sign_prepass", _i), ("magic", ctypes.c_uint32), ("reserved", _i), ("grid_x", _i64), ("lds_bytes", _i64),
                ("last_chunk", _i64)]


class H16LaunchInfo(ctypes.Structure):
    """fp8q_h16_launch_info (include/fp8q.h): one kernel of a half-lane call and its launcher's choices"""
    _fields_ = [("kernel", _i), ("u", _i), ("nontemporal", _i), ("lanes", _i), ("nsplit", _i), ("rows_per_chunk", _i),
                ("launches", _i), ("reserved", _i), ("head", _i64), ("groups", _i64), ("tail", _i64), ("lds_bytes", _i64),
                ("grid_x", _i64), ("grid_y", _i64)]


class H16RouteInfo(ctypes.Structure):
    """fp8q_h16_route_info (include/fp8q.h): the kernels a half-lane quantize / min-max / fused call launches, in order"""
    _fields_ = [("n_launches", _i), ("reserved", _i), ("launch", H16LaunchInfo * 2)]


class MxtRouteInfo(ctypes.Structure):
    """fp8q_mxt_route_info (include/fp8q.h): the kernel a transposed-MX call reaches and its tile"""
    _fields_ = [("kernel", _i), ("tile_rows", _i), ("tile_cols", _i), ("nontemporal", _i), ("code_store_bytes", _i),
                ("reserved", _i)]


class OcpbtRouteInfo(ctypes.Structure):
    """fp8q_ocpbt_route_info (include/fp8q.h): the kernel a transposed tile-scaled FP8 call reaches and its code stores"""
    _fields_ = [("kernel", _i), ("code_store_bytes", _i), ("nontemporal", _i), ("reserved", _i)]


class TensorDesc(ctypes.Structure):
    """fp8q_tensor_desc (include/fp8q.h)"""
    _fields_ = [("x", _vp), ("y", _vp), ("maxval", _vp), ("C", _i64), ("inner", _i64), ("n_maxval", _i64),
                ("mbits", _f), ("n_bits", _i), ("sign_bits", _i)]


SIGNATURES = {
    "fp8q_version": (_i, []),
    "fp8q_strerror": (ctypes.c_char_p, [_i]),
    "fp8q_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_minmax_workspace_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "fp8q_minmax_f32": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, _i, ctypes.c_double, _i, _vp,
                             ctypes.c_size_t, _vp]),
    "fp8q_minmax_packed_f32": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i, ctypes.c_double, _i, _vp,
                                    ctypes.c_size_t, _vp]),
    "fp8q_ranges_unpack_f32": (_i, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "fp8q_minmax_workspace_check": (_i, [_vp, ctypes.c_size_t, _i, _vp]),
    "fp8q_fused_max_inner": (_i64, []),
    "fp8q_minmax_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "fp8q_rows_route": (_i, [_i, _i64, _i64, _i, _f, _i, _i, _i, _i, _i, ctypes.POINTER(RowsRouteInfo)]),
    "fp8q_mse_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64, _i]),
    "fp8q_mse_grid_f32": (_i, [_vp, _i64, _i64, _vp, _i64, ctypes.POINTER(_f), _i, _i, _i, _vp, _vp,
                               ctypes.c_size_t, _vp]),
    "fp8q_mse_route": (_i, [_i64, _i64, _i64, ctypes.POINTER(_f), _i, _i, _i, ctypes.POINTER(MseRouteInfo)]),
    "fp8q_mse_linspace_f32": (_i, [_vp, _i64, _i, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "fp8q_minmax_linspace_f32": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i, ctypes.c_double, ctypes.c_double, _vp,
                                      ctypes.c_size_t, _vp]),
    "fp8q_mse_select_workspace_bytes": (ctypes.c_size_t, [_i64, _i]),
    "fp8q_mse_select_f32": (_i, [_vp, _vp, _i64, _i64, ctypes.POINTER(_f), _i, _i, _vp, _vp, _vp, _vp, _vp,
                                 ctypes.c_size_t, _vp]),
    "fp8q_quantize_dm_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i, _i, _vp]),
    "fp8q_quantize_ds_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _f, _i, _vp, _vp]),
    "fp8q_sign_fold_u8": (_i, [_vp, _i64, _vp, _vp]),
    "fp8q_quantize_dms_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i, _vp, _vp]),
    "fp8q_mse_calibrate_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64, _i, ctypes.POINTER(ctypes.c_size_t),
                                                             ctypes.POINTER(ctypes.c_size_t)]),
    "fp8q_mse_calibrate_f32": (_i, [_vp, _vp, _i64, _i64, ctypes.POINTER(MseState), _i, _i, ctypes.POINTER(_f), _i, _i, _i,
                                    ctypes.POINTER(AffinePre), _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "fp8q_quantize_f64": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_minmax_f64_workspace_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "fp8q_minmax_f64": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "fp8q_mse_f64_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64, _i]),
    "fp8q_mse_grid_f64": (_i, [_vp, _i64, _i64, _vp, _i64, ctypes.POINTER(_f), _i, _i, _i, _vp, _i, _vp,
                               ctypes.c_size_t, _vp]),
    "fp8q_affine_act_quantize_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i, _vp, _f, _i, _i,
                                          _vp]),
    "fp8q_bn_fold_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "fp8q_quantizer_prepare_f32": (_i, [_vp, _f, _i, _i, _vp, _vp]),
    "fp8q_affine_act_quantize_ab_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i, _vp, _vp, _f, _i, _i, _vp]),
    "fp8q_affine_act_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i, _vp]),
    "fp8q_affine_act_route": (_i, [_i64, _i64, _i64, _i, ctypes.POINTER(AffineRouteInfo)]),
    "fp8q_affine_act_minmax_linspace_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i, _vp, _vp, _vp, _vp, _i, ctypes.c_double,
                                                 ctypes.c_double, _vp, ctypes.c_size_t, _vp]),
    "fp8q_affine_act_minmax_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "fp8q_affine_act_minmax_f32": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i,
                                        ctypes.c_double, _i, _vp, ctypes.c_size_t, _vp]),
    "fp8q_affine_act_minmax_packed_f32": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                               _i, ctypes.c_double, _i, _vp, ctypes.c_size_t, _vp]),
    "fp8q_encode_u8": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_decode_u8": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_codec_route": (_i, [_i, _i64, _i64, _i64, _f, _i, _i, _i, _i, ctypes.POINTER(CodecRouteInfo)]),
    "fp8q_chunk_route": (_i, [_i64, _i64, _i64, _i, _i, _i, _i, _i, ctypes.POINTER(ChunkRouteInfo)]),
    "fp8q_multi_quantize_f32": (_i, [ctypes.POINTER(TensorDesc), _i, _vp]),
    "fp8q_multi_minmax_quantize_f32": (_i, [ctypes.POINTER(TensorDesc), ctypes.POINTER(_vp), _i, _vp]),
    "fp8q_multi_encode_u8": (_i, [ctypes.POINTER(TensorDesc), _i, _vp]),
    "fp8q_multi_minmax_encode_u8": (_i, [ctypes.POINTER(TensorDesc), ctypes.POINTER(_vp), _i, _vp]),
    "fp8q_multi_decode_u8": (_i, [ctypes.POINTER(TensorDesc), _i, _vp]),
    "fp8q_multi_plan_create": (_i, [ctypes.POINTER(TensorDesc), _i, ctypes.POINTER(_vp)]),
    "fp8q_multi_plan_launch": (_i, [_vp, _vp]),
    "fp8q_multi_plan_launches": (_i, [_vp]),
    "fp8q_multi_plan_destroy": (None, [_vp]),
    "fp8q_multi_route": (_i, [ctypes.POINTER(TensorDesc), _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "fp8q_copy_f32": (_i, [_vp, _vp, _i64, _vp]),
    "fp8q_int_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_int_set_range_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "fp8q_int_range_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "fp8q_int_minmax_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp,
                                          ctypes.c_size_t, _vp]),
    "fp8q_int_affine_act_quantize_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "fp8q_int_affine_act_range_quantize_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i,
                                                    _f, _vp]),
    "fp8q_int_sse_grid_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "fp8q_int_sse_grid_f32": (_i, [_vp, _i64, _i64, _vp, _i64, _i, _i, _i, _f, _vp, _vp, ctypes.c_size_t, _vp]),
    "fp8q_int_sse_grid_f64": (_i, [_vp, _i64, _i64, _vp, _i64, _i, _i, _i, _f, _vp, _vp, ctypes.c_size_t, _vp]),
    "fp8q_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_minmax_h16": (_i, [_vp, _i, _i64, _i64, _vp, _vp, _vp, _i, ctypes.c_double, _i, _vp, ctypes.c_size_t, _vp]),
    "fp8q_minmax_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "fp8q_h16_route": (_i, [_i, _i64, _i64, _i, _f, _i, _i, _i, _i, ctypes.POINTER(H16RouteInfo)]),
    "fp8q_int_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_int_range_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "fp8q_int_minmax_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp,
                                          ctypes.c_size_t, _vp]),
    "fp8q_encode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_decode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _f, _i, _i, _vp]),
    "fp8q_int_encode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_int_decode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_quantize_bwd_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _f, _vp, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "fp8q_quantize_bwd_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "fp8q_int_quantize_bwd_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _i64, _vp, _vp, _vp,
                                       ctypes.c_size_t, _vp]),
    "fp8q_int_quantize_bwd_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "fp8q_int_to_integer_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_int_encode": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_int_decode": (_i, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i, _i, _f, _vp]),
    "fp8q_percentile_resident_max_inner": (_i64, []),
    "fp8q_percentile_workspace_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "fp8q_percentile_f32": (_i, [_vp, _i64, _i64, ctypes.c_double, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "fp8q_ocp_encode_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _i, _f, _vp, _vp]),
    "fp8q_ocp_encode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _i, _f, _vp, _vp]),
    "fp8q_ocp_decode_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _i, _vp]),
    "fp8q_ocp_decode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _i, _vp]),
    "fp8q_ocp_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _i, _f, _vp]),
    "fp8q_ocp_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _i64, _i, _f, _vp]),
    "fp8q_ocp_scale_f32": (_i, [_vp, _i64, _i, _f, _vp, _vp]),
    "fp8q_ocpb_route": (_i, [_i64, _i64, _i, _i, _i, _i]),
    "fp8q_ocpb_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpb_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpb_decode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _vp]),
    "fp8q_ocpb_decode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _vp]),
    "fp8q_ocpb_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpb_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpbt_route": (_i, [_i64, _i64, _i, _i, _i, _i, ctypes.POINTER(OcpbtRouteInfo)]),
    "fp8q_ocpbt_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpbt_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpbt_encode_both_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_ocpbt_encode_both_h16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _vp]),
    "fp8q_mx_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _vp]),
    "fp8q_mx_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _vp]),
    "fp8q_mx_decode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "fp8q_mx_decode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _vp]),
    "fp8q_mx_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _vp]),
    "fp8q_mx_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_route": (_i, [_i64, _i64, _i, _i, _i, ctypes.POINTER(MxtRouteInfo)]),
    "fp8q_mxt_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_encode_both_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_encode_both_h16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _vp]),
    "fp8q_mxt_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _vp]),
    # the stochastic-rounding twins: (seed, offset) in front of the stream
    "fp8q_mxsr_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_encode_t_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_encode_t_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_encode_both_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_encode_both_h16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_quantize_t_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_mxsr_quantize_t_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _u64, _u64, _vp]),
    "fp8q_ocpsr_encode_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _i, _f, _vp, _u64, _u64, _vp]),
    "fp8q_ocpsr_encode_h16": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _i64, _i, _f, _vp, _u64, _u64, _vp]),
    "fp8q_ocpsr_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _vp, _i64, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpsr_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _i64, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbsr_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbsr_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbsr_quantize_f32": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbsr_quantize_h16": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbtsr_encode_f32": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbtsr_encode_h16": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbtsr_encode_both_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
    "fp8q_ocpbtsr_encode_both_h16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _f, _u64, _u64, _vp]),
}


class Fp8qError(RuntimeError):
    pass


def so_path():
    # FP8Q_SO: load an alternative build of the same library (kernel-tuning experiments only)
    return os.environ.get("FP8Q_SO") or _build.SO


def lib():
    """Load (once) the HIP library.  Raises if it has not been built: no silent fallback."""
    global _lib
    if _lib is None:
        path = so_path()
        if not os.path.exists(path):
            raise Fp8qError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  The FP8 engine has no CPU/eager fallback.")
        L = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().fp8q_strerror(rc).decode()
        raise Fp8qError(f"{what} failed: {msg} (code {rc})")
