"""ctypes binding of libvp_hip.so (C ABI: include/vp_hip.h).

There is NO CPU fallback: if the shared library is missing or no HIP device is visible every entry point
raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C autoware_vision_pilot_amd/csrc``.

Note for mixed processes (tests, bench): PyTorch-ROCm bundles its own ``libamdhip64.so``; import ``torch``
BEFORE this module in any process that uses both, so that a single HIP runtime is loaded.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvp_hip.so")

VP_SCENESEG, VP_SCENE3D, VP_DOMAINSEG, VP_EGOLANES, VP_AUTODRIVE, VP_AUTOSPEED, VP_AUTOSTEER = 0, 1, 2, 3, 4, 5, 6
VP_WEIGHTS_FP8 = 16
VP_PLAN_LATENCY = 32  # creation flag: this engine's kernel plan targets one network on one camera, one frame at a time (vp_hip.h)
VP_ACT_SCALE = 64  # creation flag: per-tensor power-of-two activation scale (AutoDrive, AutoSpeed, AutoSteer; parity mode; vp_hip.h)
VP_MFMA_FP8 = 128  # creation flag: the big plain 3x3 layers of a VP_FP16 scene network on the e4m3 MFMA kernel (vp_hip.h "FP8 MFMA ENGINES")
VP_FP16, VP_FP16X3 = 0, 1
VP_BGR8, VP_RGB8 = 0, 1
VP_PLANES_BGR, VP_PLANES_RGB = 0, 1
VP_DECODE_SEG_MASK, VP_DECODE_LANE_LABEL, VP_DECODE_CLASS_INDEX = 0, 1, 2
KINDS = {"sceneseg": VP_SCENESEG, "scene3d": VP_SCENE3D, "domainseg": VP_DOMAINSEG, "egolanes": VP_EGOLANES, "autodrive": VP_AUTODRIVE,
         "autospeed": VP_AUTOSPEED, "autosteer": VP_AUTOSTEER}
PRECISIONS = {"fp16": VP_FP16, "fp16x3": VP_FP16X3, "fp32": VP_FP16X3}

# every symbol include/vp_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_SIGS = {
    "vp_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_from_memory": (C.c_int, [C.POINTER(_P), C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_shared": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_shared_from_memory": (C.c_int, [C.POINTER(_P), _P, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_batched": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_batched_from_memory": (C.c_int, [C.POINTER(_P), C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_shared_frame": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_create_shared_frame_from_memory": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_frames": (C.c_int, [_P]),
    "vp_upload_frame_n": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "vp_shared_level": (C.c_int, [_P]),
    "vp_infer_shared": (C.c_int, [_P]),
    "vp_destroy": (None, [_P]),
    "vp_last_error": (C.c_char_p, [_P]),
    "vp_set_input_format": (C.c_int, [_P, C.c_int, C.c_int]),
    "vp_set_decode_mode": (C.c_int, [_P, C.c_int]),
    "vp_get_decode_mode": (C.c_int, [_P]),
    "vp_set_resize_mode": (C.c_int, [_P, C.c_int]),
    "vp_get_resize_mode": (C.c_int, [_P]),
    "vp_resample_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vp_gpu_id": (C.c_int, [_P]),
    "vp_device_count": (C.c_int, []),
    "vp_host_logits_current": (C.c_int, [_P]),
    "vp_input_hw": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_infer": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "vp_infer_tensor": (C.c_int, [_P, _P]),
    "vp_infer_pair": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "vp_logits": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int64)]),
    "vp_mask_u8": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_decode_logits_host": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "vp_mask_resized_u8": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "vp_depth_resized_f32": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "vp_visualize_mask_bgr8": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int]),
    "vp_frame_hw": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_set_outputs": (C.c_int, [_P, C.c_int]),
    "vp_set_pinned_staging": (C.c_int, [_P, C.c_int]),
    "vp_register_frames": (C.c_int, [C.c_void_p, C.c_size_t]),
    "vp_unregister_frames": (C.c_int, [C.c_void_p]),
    "vp_output_shape": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "vp_output_dims": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "vp_set_finite_check": (C.c_int, [_P, C.c_int]),
    "vp_infer_multi": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "vp_enqueue_multi": (C.c_int, [_P, C.POINTER(_P), C.c_int]),
    "vp_set_multi_fork": (C.c_int, [_P, C.c_int]),
    "vp_visualize_depth_bgr8": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "vp_input_tensor": (C.c_int, [_P, _P]),
    "vp_upload_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "vp_enqueue": (C.c_int, [_P]),
    "vp_sync": (C.c_int, [_P]),
    "vp_fetch_outputs": (C.c_int, [_P]),
    "vp_device_outputs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "vp_use_graph": (C.c_int, [_P, C.c_int]),
    "vp_timer_begin": (C.c_int, [_P]),
    "vp_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "vp_layer_count": (C.c_int, [_P]),
    "vp_layer_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vp_layer_kernel": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p)]),
    "vp_layer_launch": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p)]),
    "vp_autosteer_angle": (C.c_float, [_P, C.c_int]),
    "vp_copy_outputs_device": (C.c_int, [_P, _P, _P]),
    "vp_profile_layers": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "vp_layer_flops_executed": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "vp_tensor_count": (C.c_int, [_P]),
    "vp_tensor_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_tensor_read": (C.c_int, [_P, C.c_int, _P]),
    "vp_calibrate_range": (C.c_int, [_P, C.c_int]),
    "vp_reset_range": (C.c_int, [_P]),
    "vp_act_scales": (C.c_int, [_P, _P, C.c_int]),
    "vp_set_act_scales": (C.c_int, [_P, _P, C.c_int]),
    "vp_range_survey": (C.c_int, [_P, _P, C.c_int]),
    "vp_calibrate_fp8": (C.c_int, [_P, C.c_int]),
    "vp_reset_fp8": (C.c_int, [_P]),
    "vp_fp8_layers": (C.c_int, [_P, _P, C.c_int]),
    "vp_set_fp8_exps": (C.c_int, [_P, _P, C.c_int]),
    "vp_fp8_quantize_act": (C.c_int, [_P, C.c_size_t, C.c_int, _P]),
    "vp_op_conv3x3_f8": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "vp_op_fp8_quantize": (C.c_int, [C.c_int, _P, C.c_size_t, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "vp_op_exp_hist": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_char_p, C.c_size_t]),
    "vp_op_absmax": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]),
    "vp_op_conv2d_scaled": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_conv2d": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                               C.c_int, C.c_int, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "vp_compose_upconv": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_upconv": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                               C.c_char_p, C.c_size_t]),
    "vp_detect_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_detect_destroy": (None, [_P]),
    "vp_detect_last_error": (C.c_char_p, [_P]),
    "vp_detect_preprocess": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "vp_detect_input_device": (C.c_int, [_P, C.POINTER(_P)]),
    "vp_detect_letterbox": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_detect_set_letterbox": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_detect_postprocess": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "vp_detect_attach": (C.c_int, [_P, _P]),
    "vp_detect_infer": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "vp_detect_geometry_pil": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int)]),
    "vp_detect_preprocess_pil": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "vp_detect_postprocess_agnostic": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "vp_detect_infer_pil": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "vp_op_detect_head_decode": (C.c_int, [C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "vp_op_upsample2_cat": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_dwconv3x3": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_rowpair_conv": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_lane_rows_head": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, C.c_float, _P, C.c_float, _P, C.c_float, _P, C.c_char_p,
                                       C.c_size_t]),
    "vp_op_upsample2_cat_scaled": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                             C.c_char_p, C.c_size_t]),
    "vp_op_detect_head_decode_scaled": (C.c_int, [C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_rowpair_conv_scaled": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P,
                                            C.c_char_p, C.c_size_t]),
    "vp_op_lane_rows_head_scaled": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, C.c_float, _P, C.c_float, _P, C.c_float, C.c_int,
                                              _P, C.c_char_p, C.c_size_t]),
    "vp_op_conv2d_forms": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_version": (C.c_char_p, []),
    "vp_set_lane_ring": (C.c_int, [_P, C.c_int]),
    "vp_lane_ring_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int)]),
    "vp_lane_ring_fetch": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "vp_set_norm_form": (C.c_int, [_P, C.c_int]),
    "vp_get_norm_form": (C.c_int, [_P]),
    "vp_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "vp_get_option": (C.c_char_p, [C.c_char_p]),
    "vp_clear_options": (None, []),
    "vp_plan_hash": (C.c_ulonglong, [_P]),
    "vp_weight_bytes": (C.c_int, [_P, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "vp_split_weight_rows": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    "vp_fp8_encode_rows": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "vp_convert_onnx": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "vp_frame_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_size_t]),
    "vp_frame_destroy": (None, [_P]),
    "vp_frame_last_error": (C.c_char_p, [_P]),
    "vp_frame_upload": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]),
    "vp_frame_upload_device": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, _P]),
    "vp_frame_set_color": (C.c_int, [_P, C.c_int, C.c_int]),
    "vp_frame_get_color": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_frame_set_raw": (C.c_int, [_P, _P]),
    "vp_frame_get_raw": (C.c_int, [_P, _P]),
    "vp_frame_sync": (C.c_int, [_P]),
    "vp_frame_dims": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_frame_fetch_bgr8": (C.c_int, [_P, _P, C.c_int]),
    "vp_frame_set_rectify": (C.c_int, [_P, _P]),
    "vp_frame_get_rectify": (C.c_int, [_P, _P]),
    "vp_rectify_map": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "vp_rectify_homography": (C.c_int, [_P, _P, _P]),
    "vp_op_remap_bgr8": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_upload_from_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_infer_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_detect_infer_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "vp_canvas_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_size_t]),
    "vp_canvas_destroy": (None, [_P]),
    "vp_canvas_last_error": (C.c_char_p, [_P]),
    "vp_canvas_begin": (C.c_int, [_P, _P]),
    "vp_canvas_blend_mask": (C.c_int, [_P, _P, C.c_int]),
    "vp_canvas_blend_mask_u8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_canvas_paste_depth": (C.c_int, [_P, _P]),
    "vp_canvas_draw_detections": (C.c_int, [_P, _P, C.c_int]),
    "vp_canvas_sync": (C.c_int, [_P]),
    "vp_canvas_dims": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_canvas_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int)]),
    "vp_canvas_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_canvas_layout3": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_canvas_set_color": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "vp_canvas_get_color": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vp_canvas_fetch": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int), C.c_int]),
    "vp_canvas_add_planes_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_canvas_overlay_lanes": (C.c_int, [_P, _P, C.c_float]),
    "vp_canvas_draw_points": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "vp_canvas_draw_lane_rows": (C.c_int, [_P, _P]),
    "vp_canvas_fetch_resized": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int), C.c_int]),
    "vp_canvas_fetch_jpeg": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vp_canvas_fetch_jpeg_resized": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vp_jpeg_bound": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "vp_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "vp_op_jpeg_encode_bgr8": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "vp_metric_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_metric_destroy": (None, [_P]),
    "vp_metric_last_error": (C.c_char_p, [_P]),
    "vp_metric_reset": (C.c_int, [_P]),
    "vp_metric_add_seg": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vp_metric_add_depth": (C.c_int, [_P, _P, _P, C.c_int]),
    "vp_metric_add_seg_pair": (C.c_int, [_P, _P, _P]),
    "vp_metric_add_depth_pair": (C.c_int, [_P, _P, _P]),
    "vp_metric_frames": (C.c_int, [_P]),
    "vp_metric_fetch": (C.c_int, [_P, _P, C.c_int, _P]),
    "vp_metric_add_seg_logits": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "vp_metric_add_depth_plane": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "vp_op_select_f32": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_char_p, C.c_size_t]),
    "vp_metric_add_det": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int]),
    "vp_metric_add_det_pair": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, _P, C.c_int]),
    "vp_metric_add_det_raw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int]),
    "vp_metric_det_frames": (C.c_int, [_P]),
    "vp_metric_fetch_det": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P]),
    "vp_metric_det_ap": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "vp_op_detect_validate": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "vp_metric_add_lanes": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vp_metric_add_lanes_pair": (C.c_int, [_P, _P, _P]),
    "vp_metric_add_lanes_logits": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "vp_metric_lanes_frames": (C.c_int, [_P]),
    "vp_metric_fetch_lanes": (C.c_int, [_P, _P, C.c_int, _P]),
    "vp_metric_add_rows": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "vp_metric_add_rows_pair": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "vp_metric_add_rows_raw": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "vp_metric_rows_lines": (C.c_int, [_P]),
    "vp_metric_fetch_rows": (C.c_int, [_P, _P, C.c_int, _P]),
    "vp_metric_rows_ap": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P]),
    "vp_metric_add_seg_label": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vp_metric_add_depth_label": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_metric_add_seg_logits_label": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vp_metric_add_depth_plane_label": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vp_metric_label_frames": (C.c_int, [_P]),
    "vp_metric_fetch_labels": (C.c_int, [_P, _P, C.c_int]),
    "vp_op_label_gt": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_op_label_depth_gt": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_char_p, C.c_size_t]),
    "vp_lanes_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "vp_lanes_destroy": (None, [_P]),
    "vp_lanes_last_error": (C.c_char_p, [_P]),
    "vp_lanes_set_smoothing": (C.c_int, [_P, C.c_float]),
    "vp_lanes_reset": (C.c_int, [_P]),
    "vp_lanes_add": (C.c_int, [_P, _P, C.c_float]),
    "vp_lanes_add_logits": (C.c_int, [_P, _P, C.c_float]),
    "vp_lanes_pending": (C.c_int, [_P]),
    "vp_lanes_fetch": (C.c_int, [_P, _P, C.c_int, _P]),
    "vp_lanes_fetch_points": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "vp_lanes_fit": (C.c_int, [_P, _P, C.c_int, _P, _P]),
}
# multi-camera exchange (csrc/vp_comm.cpp): part of libvp_hip.so, absent from the CPU-emulated test build
_COMM_SIGS = {
    "vp_comm_unique_id": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "vp_comm_create": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_char_p, C.c_size_t]),
    "vp_comm_destroy": (None, [_P]),
    "vp_comm_last_error": (C.c_char_p, [_P]),
    "vp_comm_rank": (C.c_int, [_P]),
    "vp_comm_world": (C.c_int, [_P]),
    "vp_gather": (C.c_int, [_P, _P, C.c_int]),
    "vp_comm_device_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vp_comm_fetch": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
}
EXPORTED_SYMBOLS = tuple(_SIGS) + tuple(_COMM_SIGS)
VP_OUT_LOGITS, VP_OUT_MASK = 1, 2
VP_NORM_TORCHVISION, VP_NORM_OPENCV = 0, 1
VP_RESIZE_CV_LINEAR, VP_RESIZE_PIL_BILINEAR, VP_RESIZE_PIL_BICUBIC = 0, 1, 2
VP_GATHER_MASK, VP_GATHER_LOGITS = 0, 1
VP_COMM_ID_BYTES = 128

VP_RANGE_BINS, VP_RANGE_EXP_MIN = 40, -24
VP_VIZ_SCENE, VP_VIZ_DOMAIN, VP_VIZ_EGOLANES = 0, 1, 2
VP_FRAME_BGR8, VP_FRAME_RGB8, VP_FRAME_BGRA8, VP_FRAME_RGBA8, VP_FRAME_GRAY8, VP_FRAME_NV12, VP_FRAME_YUY2, VP_FRAME_UYVY = range(8)
VP_FRAME_I420, VP_FRAME_YV12, VP_FRAME_NV21 = 16, 17, 18
FRAME_FORMATS = {"bgr8": VP_FRAME_BGR8, "rgb8": VP_FRAME_RGB8, "bgra8": VP_FRAME_BGRA8, "rgba8": VP_FRAME_RGBA8, "gray8": VP_FRAME_GRAY8, "nv12": VP_FRAME_NV12,
                 "yuy2": VP_FRAME_YUY2, "uyvy": VP_FRAME_UYVY, "i420": VP_FRAME_I420, "yv12": VP_FRAME_YV12, "nv21": VP_FRAME_NV21}
# upload-only: 16-bit grey, P010, raw Bayer in 8-bit and 16-bit containers (little-endian words)
VP_FRAME_GRAY16, VP_FRAME_P010 = 20, 21
BAYER_ORDERS = ("rggb", "grbg", "gbrg", "bggr")
FRAME_FORMATS.update({"gray16": VP_FRAME_GRAY16, "p010": VP_FRAME_P010})
FRAME_FORMATS.update({f"bayer_{o}8": 32 + i for i, o in enumerate(BAYER_ORDERS)})
FRAME_FORMATS.update({f"bayer_{o}16": 36 + i for i, o in enumerate(BAYER_ORDERS)})
_FRAME_PX_BYTES = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1, 5: 1, 6: 2, 7: 2, 16: 1, 17: 1, 18: 1, 20: 2, 21: 2, 32: 1, 33: 1, 34: 1, 35: 1, 36: 2, 37: 2, 38: 2, 39: 2}   # bytes per pixel of plane 0
_FRAME_WORDS = frozenset((20, 21, 36, 37, 38, 39))                                          # formats of 16-bit samples
_FRAME_PLANES = {VP_FRAME_NV12: 2, VP_FRAME_NV21: 2, VP_FRAME_I420: 3, VP_FRAME_YV12: 3, VP_FRAME_P010: 2}    # every other format: 1
VP_COLOR_BT601, VP_COLOR_BT709 = 0, 1
VP_COLOR_RANGE_LIMITED, VP_COLOR_RANGE_FULL = 0, 1
VP_CHROMA_EVEN, VP_CHROMA_MEAN = 0, 1
COLOR_MATRICES = {"bt601": VP_COLOR_BT601, "bt709": VP_COLOR_BT709}
COLOR_RANGES = {"limited": VP_COLOR_RANGE_LIMITED, "full": VP_COLOR_RANGE_FULL}
CHROMA_MODES = {"even": VP_CHROMA_EVEN, "mean": VP_CHROMA_MEAN}
VP_RECTIFY_TWO_PASS, VP_RECTIFY_ONE_PASS = 0, 1
VP_BORDER_CONSTANT, VP_BORDER_REPLICATE = 0, 1
RECTIFY_MODES = {"two_pass": VP_RECTIFY_TWO_PASS, "one_pass": VP_RECTIFY_ONE_PASS}
RECTIFY_MAPS = {"undistort": 0, "warp": 1, "one_pass": 2}
BORDERS = {"constant": VP_BORDER_CONSTANT, "replicate": VP_BORDER_REPLICATE}
VP_GT_LABEL, VP_GT_BITS = 0, 1
GT_FORMS = {"label": VP_GT_LABEL, "bits": VP_GT_BITS}


def _named(table, v):
    return table[v.lower()] if isinstance(v, str) else int(v)


class Fp8Layer(C.Structure):
    """vp_fp8_layer (include/vp_hip.h): one conv3x3_f8 launch -- its launch index, its input tensor's index, its activation exponent"""
    _fields_ = [("launch", C.c_int), ("tensor", C.c_int), ("qexp", C.c_int)]


class RangeStats(C.Structure):
    """vp_range_stats (include/vp_hip.h)"""
    _fields_ = [("absmax", C.c_float), ("exp", C.c_int), ("count", C.c_ulonglong), ("nonfinite", C.c_ulonglong), ("zeros", C.c_ulonglong),
                ("bins", C.c_ulonglong * VP_RANGE_BINS)]


class Rectify(C.Structure):
    """vp_rectify (include/vp_hip.h)"""
    _fields_ = [("K", C.c_double * 9), ("dist", C.c_double * 5), ("H", C.c_double * 9), ("out_w", C.c_int), ("out_h", C.c_int), ("mode", C.c_int)]


class Raw(C.Structure):
    """vp_raw (include/vp_hip.h)"""
    _fields_ = [("bits", C.c_int), ("shift", C.c_int), ("black", C.c_int), ("gains", C.c_int * 3), ("ccm_on", C.c_int), ("ccm", C.c_int * 9),
                ("lut", C.c_void_p), ("lut_len", C.c_int)]


class MetricFrame(C.Structure):
    """vp_metric_frame (include/vp_hip.h)"""
    _fields_ = [("kind", C.c_int), ("I", C.c_uint32 * 3), ("P", C.c_uint32 * 3), ("G", C.c_uint32 * 3), ("nonfinite", C.c_uint32), ("n", C.c_uint32),
                ("kept", C.c_uint32), ("q_lo", C.c_float), ("q_hi", C.c_float), ("q", C.c_float), ("mae", C.c_float), ("mel", C.c_float)]


class MetricSummary(C.Structure):
    """vp_metric_summary (include/vp_hip.h)"""
    _fields_ = [("frames", C.c_int), ("sceneseg_frames", C.c_int), ("domainseg_frames", C.c_int), ("scene3d_frames", C.c_int), ("nan_frames", C.c_int),
                ("reserved", C.c_int), ("sceneseg_iou", C.c_double * 3), ("sceneseg_iou_full", C.c_double), ("domainseg_iou", C.c_double), ("mae", C.c_double),
                ("mel", C.c_double)]


METRIC_FRAME_DTYPE = np.dtype([("kind", "<i4"), ("I", "<u4", (3,)), ("P", "<u4", (3,)), ("G", "<u4", (3,)), ("nonfinite", "<u4"), ("n", "<u4"), ("kept", "<u4"),
                               ("q_lo", "<f4"), ("q_hi", "<f4"), ("q", "<f4"), ("mae", "<f4"), ("mel", "<f4")])


VP_DET_MAX_NMS, VP_DET_MAX_DET, VP_DET_MAX_CLASSES, VP_DET_MAX_IOU, VP_DET_MAX_LABELS = 30000, 300, 80, 16, 4096
DET_CONF, DET_IOU = 0.001, 0.65          # the trainer's validation thresholds (auto_speed_util.py:123)
# torch.linspace(0.5, 0.95, 10), from its bits
DET_IOU_V = np.array([0x3F000000, 0x3F0CCCCD, 0x3F19999A, 0x3F266666, 0x3F333333, 0x3F400000, 0x3F4CCCCD, 0x3F59999A, 0x3F666666, 0x3F733333], dtype="<u4").view("<f4")
METRIC_DET_FRAME_DTYPE = np.dtype([("candidates", "<u4"), ("ranked", "<u4"), ("kept", "<u4"), ("labels", "<u4"), ("first_row", "<u4")])
METRIC_DET_ROW_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("conf", "<f4"), ("cls", "<f4"), ("tp", "<u4")])


class MetricDetSummary(C.Structure):
    """vp_metric_det_summary (include/vp_hip.h)"""
    _fields_ = [("frames", C.c_int), ("rows", C.c_int), ("labels", C.c_int), ("classes", C.c_int), ("n_iou", C.c_int), ("grid_index", C.c_int),
                ("precision", C.c_double), ("recall", C.c_double), ("map50", C.c_double), ("map", C.c_double),
                ("class_id", C.c_float * VP_DET_MAX_CLASSES), ("class_labels", C.c_uint32 * VP_DET_MAX_CLASSES), ("ap50", C.c_double * VP_DET_MAX_CLASSES),
                ("ap", C.c_double * VP_DET_MAX_CLASSES), ("tp", C.c_double * VP_DET_MAX_CLASSES), ("fp", C.c_double * VP_DET_MAX_CLASSES)]


VP_LANES_GT_PLANES, VP_LANES_GT_BITS, VP_LANES_GT_BITS_4X = 0, 1, 2
LANES_GT_FORMS = {"planes": VP_LANES_GT_PLANES, "bits": VP_LANES_GT_BITS, "bits4x": VP_LANES_GT_BITS_4X}
VP_ROWS_MAX_THR, VP_ROWS_MAX_LINES, VP_ROWS_MAX_ROWS = 8, 8, 1024
ROWS_THR = (0.02, 0.05, 0.10)            # the trainer's thresholds (auto_steer_trainer.py:180)
METRIC_LANES_FRAME_DTYPE = np.dtype([("bce", "<f4", (3,)), ("edge", "<f4", (3, 5)), ("loss", "<f4", (3,)), ("score", "<f4"), ("n", "<u4"), ("nonfinite", "<u4")])
METRIC_ROWS_LINE_DTYPE = np.dtype([("dist", "<f4"), ("conf", "<f4"), ("tp", "<u4"), ("valid", "<u4"), ("target_valid", "<u4")])


class MetricLanesFrame(C.Structure):
    """vp_metric_lanes_frame (include/vp_hip.h)"""
    _fields_ = [("bce", C.c_float * 3), ("edge", (C.c_float * 5) * 3), ("loss", C.c_float * 3), ("score", C.c_float), ("n", C.c_uint32), ("nonfinite", C.c_uint32)]


class MetricLanesSummary(C.Structure):
    """vp_metric_lanes_summary (include/vp_hip.h)"""
    _fields_ = [("frames", C.c_int), ("nan_frames", C.c_int), ("score", C.c_double), ("loss", C.c_double * 3), ("bce", C.c_double * 3), ("edge", C.c_double * 3)]


class MetricRowsLine(C.Structure):
    """vp_metric_rows_line (include/vp_hip.h)"""
    _fields_ = [("dist", C.c_float), ("conf", C.c_float), ("tp", C.c_uint32), ("valid", C.c_uint32), ("target_valid", C.c_uint32)]


class MetricRowsSummary(C.Structure):
    """vp_metric_rows_summary (include/vp_hip.h)"""
    _fields_ = [("lines", C.c_int), ("n_thr", C.c_int), ("precision", C.c_double), ("recall", C.c_double), ("mean_ap", C.c_double), ("ap", C.c_double * VP_ROWS_MAX_THR),
                ("map50", C.c_double)]


VP_LANES_MAX_WINDOWS, VP_LANES_MAX_POINTS = 40, 1920
VP_LANES_SINGULAR, VP_LANES_SMOOTHED = 1, 2
# vp_lanes_lane / vp_lanes_result (include/vp_hip.h)
LANES_LANE_DTYPE = np.dtype([("start_x", "<i4"), ("start_y", "<i4"), ("n_windows_up", "<i4"), ("n_windows_down", "<i4"), ("n_points_up", "<i4"), ("n_points_down", "<i4"),
                             ("min_y", "<i4"), ("max_y", "<i4"), ("S", "<i8", (5,)), ("T", "<i8", (3,)), ("windows", "<i2", (VP_LANES_MAX_WINDOWS, 4)), ("order", "<i4"),
                             ("flags", "<i4"), ("coeffs_valid", "<i4"), ("reserved", "<i4"), ("raw_coeffs", "<f8", (6,)), ("coeffs", "<f8", (6,))])
LANES_RESULT_DTYPE = np.dtype([("lane", LANES_LANE_DTYPE, (2,))])
VP_LABEL_F32, VP_LABEL_F64 = 0, 1
LABEL_FRAME_DTYPE = np.dtype([("kind", "<i4"), ("n", "<u4"), ("freq", "<u4", (3,)), ("unmatched", "<u4"), ("outside", "<u4"), ("nonfinite", "<u4"), ("min", "<f8"),
                              ("max", "<f8")])
# VP_SCENESEG_COLOURS_INIT (include/vp_hip.h): rows r, g, b, class -- class 0 sky, background objects, road-edge delimiter, unlabelled; class 1 vulnerable
# living, small / large mobile vehicle, foreground objects; class 2 road
SCENESEG_COLOURS = np.array([(61, 184, 255, 0), (61, 93, 255, 0), (216, 255, 61, 0), (0, 0, 0, 0), (255, 61, 61, 1), (255, 190, 61, 1), (255, 116, 61, 1), (255, 28, 145, 1),
                             (0, 255, 220, 2)], dtype=np.uint8)
SCENESEG_WEIGHT_OFFSET = 5120


def sceneseg_roi(dataset, w, h):
    """the PIL box (l, t, r, b) the SceneSeg loader crops image and label of `dataset` with, for a w x h image; None: no crop (MAPILLARY, anything else)"""
    fixed = {"ACDC": (0, 0, 1919, 990), "BDD100K": (0, 0, 1000, 500), "IDDAW": (0, 476, 2047, 1500), "MUSES": (0, 0, 1919, 918)}
    name = str(dataset).upper()
    if name in fixed:
        return fixed[name]
    if name == "COMMA10K":
        return (0, 0, int(w) - 1, int(int(h) * 0.7))
    return None


def class_weights(record):
    """the loader's loss weights n / (freq[c] + 5120) of one colour-label record, in Python floats (double)"""
    return [int(record["n"]) / (int(f) + SCENESEG_WEIGHT_OFFSET) for f in record["freq"]]


def _label_u8(label):
    """(array kept alive, channels, h, w, stride in bytes): uint8 [h][w][3] or [h][w]; rows may be further apart than their bytes"""
    a = np.asarray(label)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError("label: a uint8 array [h][w][3] (colours) or [h][w] (a mask)")
    ch = 3 if a.ndim == 3 else 1
    if a.strides[-1] != 1 or (a.ndim == 3 and a.strides[1] != 3) or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    return a, ch, a.shape[0], a.shape[1], a.strides[0]


def _label_depth(label):
    """(array kept alive, dtype code, h, w, stride in elements): float32 or float64 [h][w]"""
    a = np.asarray(label)
    if a.dtype not in (np.float32, np.float64) or a.ndim != 2 or a.size == 0:
        raise ValueError("label: a float32 or float64 array [h][w]")
    if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
        a = np.ascontiguousarray(a)
    return a, (VP_LABEL_F64 if a.dtype == np.float64 else VP_LABEL_F32), a.shape[0], a.shape[1], a.strides[0] // a.itemsize


def _label_crop(crop):
    if crop is None:
        return None, None
    box = np.array([int(v) for v in crop], dtype=np.int32)
    if box.shape != (4,):
        raise ValueError("crop: (l, t, r, b)")
    return _ptr(box), box


def _label_colours(colours, channels):
    if channels != 3:
        return None, None, 0
    t = np.ascontiguousarray(SCENESEG_COLOURS if colours is None else colours, dtype=np.uint8)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("colours: rows r, g, b, class")
    return _ptr(t), t, t.shape[0]


def _rows_summary_dict(s):
    return {"lines": s.lines, "n_thr": s.n_thr, "precision": s.precision, "recall": s.recall, "mean_ap": s.mean_ap, "ap": np.array(s.ap[:s.n_thr]), "map50": s.map50}


def _rows_table(thr):
    t = np.ascontiguousarray(ROWS_THR if thr is None else thr, dtype=np.float64).reshape(-1)
    return t, _ptr(t), int(t.size)


def _det_summary_dict(s):
    n = min(s.classes, VP_DET_MAX_CLASSES)
    return {"frames": s.frames, "rows": s.rows, "labels": s.labels, "classes": s.classes, "n_iou": s.n_iou, "grid_index": s.grid_index, "precision": s.precision,
            "recall": s.recall, "map50": s.map50, "map": s.map, "class_id": np.array(s.class_id[:n], dtype=np.float32), "class_labels": np.array(s.class_labels[:n], dtype=np.uint32),
            "ap50": np.array(s.ap50[:n]), "ap": np.array(s.ap[:n]), "tp": np.array(s.tp[:n]), "fp": np.array(s.fp[:n])}


def _det_table(iou_v):
    t = np.ascontiguousarray(DET_IOU_V if iou_v is None else iou_v, dtype=np.float32).reshape(-1)
    return t, _ptr(t), int(t.size)


def _det_labels(labels):
    """(array [n][5] or None, pointer, n): rows cls, cx, cy, w, h normalised to the network input"""
    if labels is None or np.size(labels) == 0:
        return None, None, 0
    lb = np.ascontiguousarray(labels, dtype=np.float32)
    if lb.ndim != 2 or lb.shape[1] != 5:
        raise ValueError("labels: rows [cls, cx, cy, w, h]")
    return lb, _ptr(lb), int(lb.shape[0])


class CameraPose(C.Structure):
    """vp_camera_pose (include/vp_hip.h)"""
    _fields_ = [("pitch_deg", C.c_double), ("yaw_deg", C.c_double), ("roll_deg", C.c_double), ("camera_height", C.c_double), ("K", C.c_double * 9),
                ("img_w", C.c_int), ("img_h", C.c_int), ("hfov_deg", C.c_double)]


def _rectify(K, dist, H, out_hw, mode):
    r = Rectify()
    r.K[:] = [float(v) for v in np.asarray(K, dtype=np.float64).reshape(9)]
    r.dist[:] = [float(v) for v in np.asarray(dist, dtype=np.float64).reshape(5)]
    r.H[:] = [float(v) for v in np.asarray(H, dtype=np.float64).reshape(9)]
    r.out_h, r.out_w = int(out_hw[0]), int(out_hw[1])
    r.mode = _named(RECTIFY_MODES, mode)
    return r


_lib = None


class VpError(RuntimeError):
    pass


class VpRangeError(VpError):
    """VP_ERR_RANGE: a weight beyond the fp16 range at load, or inf / NaN in a network's output (an activation left the fp16 range)."""


def load():
    """dlopen libvp_hip.so and bind every symbol; raises (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VpError(f"{LIB_PATH} not built -- run __graft_entry__.build(); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    # the multi-camera exchange is bound where the build carries it (a single-camera host may build without the RCCL headers:
    # csrc/Makefile VP_NO_COMM=1); Comm raises on first use otherwise.  tests/test_host_cpu.py checks the shipped library has them all.
    for name, (res, args) in _COMM_SIGS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def set_option(key, value):
    """vp_set_option: a developer knob of the dispatch rules (process-wide, engines created afterwards); value None removes it.
    The library never reads the environment -- tools that want the old `VP_X=... python tool.py` spelling call options_from_env()."""
    rc = load().vp_set_option(key.encode(), None if value is None else str(value).encode())
    if rc != 0:
        raise ValueError(f"vp_set_option({key!r}): unknown key")


def get_option(key):
    v = load().vp_get_option(key.encode())
    return None if v is None else v.decode()


def clear_options():
    load().vp_clear_options()


def options_from_env(environ=None):
    """DEVELOPER TOOLS ONLY (tools/*.py call it explicitly): copy the VP_* variables the dispatch rules know from the environment into
    the library's option table.  Returns what was set."""
    environ = os.environ if environ is None else environ
    done = {}
    for k, v in environ.items():
        if k.startswith("VP_") and load().vp_set_option(k.encode(), v.encode()) == 0:
            done[k] = v
    return done


def register_frames(buf):
    """vp_register_frames: page-lock a host buffer (a C-contiguous uint8 ndarray that OUTLIVES the registration, e.g. a frame pool) so frames
    inside it go to the device by one DMA with no staging copy.  Keep the array alive and call unregister_frames(buf) before freeing it."""
    a = np.asarray(buf)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("frame pool must be C-contiguous")
    rc = load().vp_register_frames(a.ctypes.data_as(C.c_void_p), a.nbytes)
    if rc != 0:
        raise VpError(f"vp_register_frames failed (rc {rc})")
    return a


def unregister_frames(buf):
    rc = load().vp_unregister_frames(np.asarray(buf).ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise VpError(f"vp_unregister_frames failed (rc {rc})")


def version():
    return load().vp_version().decode()


def fp8_encode_rows(w):
    """vp_fp8_encode_rows (host only): fp32 [rows][per_row] -> (uint8 e4m3 codes, fp32 row scales)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, per = w.shape
    codes = np.empty((rows, per), np.uint8)
    scale = np.empty(rows, np.float32)
    if load().vp_fp8_encode_rows(_ptr(w), rows, per, _ptr(codes), _ptr(scale)) != 0:
        raise ValueError("vp_fp8_encode_rows failed")
    return codes, scale


def fp8_quantize_act(f16, qexp=0):
    """vp_fp8_quantize_act (host only): float16 array -> uint8 e4m3 codes of x * 2^-qexp under the rule of the e4m3 MFMA layers."""
    a = np.ascontiguousarray(f16, dtype=np.float16)
    codes = np.empty(a.shape, np.uint8)
    if load().vp_fp8_quantize_act(_ptr(a), a.size, int(qexp), _ptr(codes)) != 0:
        raise ValueError("vp_fp8_quantize_act failed (qexp: -24 .. 24)")
    return codes


def fp8_quantize(f16, qexp=0, gpu_id=0):
    """vp_op_fp8_quantize: the same codes from the kernel's device function."""
    a = np.ascontiguousarray(f16, dtype=np.float16)
    codes = np.empty(a.shape, np.uint8)
    err = C.create_string_buffer(512)
    rc = load().vp_op_fp8_quantize(gpu_id, _ptr(a), a.size, int(qexp), _ptr(codes), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_fp8_quantize failed ({rc}): {err.value.decode(errors='replace')}")
    return codes


def conv3x3_f8(x, weight, bias, act=0, qexp=0, gpu_id=0):
    """vp_op_conv3x3_f8: Conv2d 3x3 + bias + act (0 none, 1 GELU) on the e4m3 MFMA kernel under the activation exponent qexp.
    x [cin][h][w], weight [cout][cin][3][3], bias [cout] -> the stored float16 [cout][h][w]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    cin, h, w = x.shape
    cout = weight.shape[0]
    if weight.shape != (cout, cin, 3, 3) or bias.shape != (cout,):
        raise ValueError("weight [cout][cin][3][3], bias [cout]")
    out = np.empty((cout, h, w), np.float16)
    err = C.create_string_buffer(512)
    rc = load().vp_op_conv3x3_f8(gpu_id, _ptr(x), cin, h, w, _ptr(weight), _ptr(bias), cout, int(act), int(qexp), _ptr(out), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_conv3x3_f8 failed ({rc}): {err.value.decode(errors='replace')}")
    return out


def split_weight_rows(w):
    """vp_split_weight_rows (host only): fp32 [rows][per_row] -> (hi fp16, lo fp16, post_scale fp32 [rows])."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, per = w.shape
    hi = np.empty((rows, per), np.float16)
    lo = np.empty((rows, per), np.float16)
    post = np.empty(rows, np.float32)
    rc = load().vp_split_weight_rows(_ptr(w), rows, per, _ptr(hi), _ptr(lo), _ptr(post))
    if rc != 0:
        raise (VpRangeError if rc == -5 else ValueError)(f"vp_split_weight_rows failed ({rc})")
    return hi, lo, post


def convert_onnx(onnx_path, vpw_path):
    """ONNX file (reference exporter settings) -> VPW1 blob file with the library's native reader (csrc/onnx_reader.cpp;
    host only, no GPU needed).  `Engine(kind, "model.onnx")` does the same conversion in memory."""
    err = C.create_string_buffer(512)
    rc = load().vp_convert_onnx(os.fsencode(onnx_path), os.fsencode(vpw_path), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_convert_onnx failed ({rc}): {err.value.decode(errors='replace')}")
    return vpw_path


class Engine:
    """Thin RAII wrapper over a vp_engine handle."""

    def __init__(self, kind, weights, precision="fp16", gpu_id=0, base=None, weights_fp8=False, frames=1, frame_index=None, plan_latency=False, act_scale=False, mfma_fp8=False):
        """base: another Engine -> shared-prefix engine (vp_create_shared): reuses the base engine's backbone (and
        context + neck when their parameters are identical) on the frame the base last processed.
        frames > 1: batched encoder (vp_create_batched) -- preprocess + backbone of `frames` cameras per pass, no head;
        heads are Engine(kind, weights, base=encoder, frame_index=f) (vp_create_shared_frame)."""
        lib = load()
        self._lib = lib
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        k = KINDS[kind] if isinstance(kind, str) else int(kind)
        pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
        if weights_fp8:
            pr |= VP_WEIGHTS_FP8
        if plan_latency:
            pr |= VP_PLAN_LATENCY
        if act_scale:
            pr |= VP_ACT_SCALE
        if mfma_fp8:
            pr |= VP_MFMA_FP8
        self._base = base  # keeps the base engine alive as long as this one
        path = None if isinstance(weights, (bytes, bytearray, memoryview, np.ndarray)) else (os.fsencode(weights) if weights else b"")
        if frames != 1 or frame_index is not None:
            buf = None if path is not None else (np.frombuffer(weights, dtype=np.uint8) if not isinstance(weights, np.ndarray) else weights)
            if base is None:
                rc = (lib.vp_create_batched(C.byref(self._h), k, path, pr, gpu_id, frames, err, len(err)) if path is not None else
                      lib.vp_create_batched_from_memory(C.byref(self._h), k, _ptr(buf), buf.nbytes, pr, gpu_id, frames, err, len(err)))
            else:
                fi = int(frame_index or 0)
                rc = (lib.vp_create_shared_frame(C.byref(self._h), base._h, fi, k, path, pr, gpu_id, err, len(err)) if path is not None else
                      lib.vp_create_shared_frame_from_memory(C.byref(self._h), base._h, fi, k, _ptr(buf), buf.nbytes, pr, gpu_id, err, len(err)))
        elif isinstance(weights, (bytes, bytearray, memoryview, np.ndarray)):
            buf = np.frombuffer(weights, dtype=np.uint8) if not isinstance(weights, np.ndarray) else weights
            if base is not None:
                rc = lib.vp_create_shared_from_memory(C.byref(self._h), base._h, k, _ptr(buf), buf.nbytes, pr, gpu_id, err, len(err))
            else:
                rc = lib.vp_create_from_memory(C.byref(self._h), k, _ptr(buf), buf.nbytes, pr, gpu_id, err, len(err))
        elif base is not None:
            rc = lib.vp_create_shared(C.byref(self._h), base._h, k, os.fsencode(weights) if weights else b"", pr, gpu_id, err, len(err))
        else:
            rc = lib.vp_create(C.byref(self._h), k, os.fsencode(weights) if weights else b"", pr, gpu_id, err, len(err))
        if rc != 0:
            self._h = C.c_void_p()
            msg = err.value.decode(errors="replace")
            raise (ValueError if rc == -1 else VpRangeError if rc == -5 else VpError)(f"vp_create failed ({rc}): {msg}")
        self.kind = kind

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._h = None
            self._lib.vp_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: globals may already be gone
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpRangeError if rc == -5 else VpError)(f"libvp_hip error {rc}: {msg}")
        return rc

    def set_finite_check(self, on):
        """inf / NaN probe on the logits at the end of every pass (default on): VpRangeError from the synchronising call."""
        self._ck(self._lib.vp_set_finite_check(self._h, int(bool(on))))

    # ---- configuration
    def set_input_format(self, pixel_format, plane_order):
        self._ck(self._lib.vp_set_input_format(self._h, pixel_format, plane_order))

    def set_decode_mode(self, mode):
        self._ck(self._lib.vp_set_decode_mode(self._h, mode))

    def set_resize_mode(self, mode):
        """VP_RESIZE_CV_LINEAR (the C++ nodes' cv::resize model), VP_RESIZE_PIL_BILINEAR / _BICUBIC (the Python scripts' Image.resize)."""
        self._ck(self._lib.vp_set_resize_mode(self._h, mode))

    def resize_mode(self):
        return self._lib.vp_get_resize_mode(self._h)

    def set_norm_form(self, form):
        """VP_NORM_TORCHVISION: q / 255 (to_tensor; default), VP_NORM_OPENCV: q * fl(1/255) (cv::Mat::convertTo, the C++ front-ends)."""
        self._ck(self._lib.vp_set_norm_form(self._h, form))

    def norm_form(self):
        return self._lib.vp_get_norm_form(self._h)

    def plan_hash(self):
        return int(self._lib.vp_plan_hash(self._h))

    def set_lane_ring(self, on=True):
        """AutoSteer hand-over on an EgoLanes engine: keep [t-1 | t] of the raw logits (fp32 6 x 80 x 160) on the device (vp_set_lane_ring)."""
        self._ck(self._lib.vp_set_lane_ring(self._h, 1 if on else 0))

    def lane_ring(self):
        """(6 x 80 x 160 fp32 host copy of the ring, frames_valid)  -- frames_valid < 2: the reference skips AutoSteer (main.cpp:521)."""
        buf = np.empty((6, 80, 160), np.float32)
        n = C.c_int()
        self._ck(self._lib.vp_lane_ring_fetch(self._h, _ptr(buf), C.byref(n)))
        return buf, n.value

    def weight_bytes(self):
        """Device bytes of the weight tensors by storage class: {'fp8': e4m3 codes, 'fp16': fp16 planes, 'fp32': fp32 rows} (vp_weight_bytes)."""
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._ck(self._lib.vp_weight_bytes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"fp8": a.value, "fp16": b.value, "fp32": c.value}

    def input_hw(self):
        h, w = C.c_int(), C.c_int()
        self._ck(self._lib.vp_input_hw(self._h, C.byref(h), C.byref(w)))
        return h.value, w.value

    # ---- synchronous path
    def infer(self, frame_u8):
        f = np.ascontiguousarray(frame_u8, dtype=np.uint8)
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("frame must be HxWx3 uint8")
        self._ck(self._lib.vp_infer(self._h, _ptr(f), f.shape[0], f.shape[1], f.strides[0]))

    def infer_pair(self, prev_u8, curr_u8):
        """AutoDrive.forward(image_prev, image_curr): both HxWx3 uint8 frames of the same geometry."""
        a = np.ascontiguousarray(prev_u8, dtype=np.uint8)
        b = np.ascontiguousarray(curr_u8, dtype=np.uint8)
        if a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("frames must be two HxWx3 uint8 arrays of the same shape")
        self._ck(self._lib.vp_infer_pair(self._h, _ptr(a), _ptr(b), a.shape[0], a.shape[1], a.strides[0]))

    # ---- per-tensor activation scale (engines created with act_scale=True)
    def calibrate_range(self, target_log2=0):
        """vp_calibrate_range over the resident frame(s): the pair of the last infer_pair (whether or not it raised VpRangeError), or the uploaded frame."""
        self._ck(self._lib.vp_calibrate_range(self._h, int(target_log2)))

    def reset_range(self):
        self._ck(self._lib.vp_reset_range(self._h))

    def act_scales(self):
        """One exponent per tensors() entry: tensor t is stored as x * 2^-s_t."""
        n = self._ck(self._lib.vp_tensor_count(self._h))
        out = np.zeros(n, dtype=np.int32)
        self._ck(self._lib.vp_act_scales(self._h, _ptr(out), n))
        return out

    def set_act_scales(self, exps):
        e = np.ascontiguousarray(exps, dtype=np.int32)
        self._ck(self._lib.vp_set_act_scales(self._h, _ptr(e), int(e.size)))

    # ---- e4m3 MFMA layers (engines created with mfma_fp8=True)
    def calibrate_fp8(self, target_log2=0):
        """vp_calibrate_fp8 over the resident frame: every fp8 layer's qexp so that absmax(input) * 2^-qexp lies in [2^(t-1), 2^t); 0 = 8."""
        self._ck(self._lib.vp_calibrate_fp8(self._h, int(target_log2)))

    def reset_fp8(self):
        self._ck(self._lib.vp_reset_fp8(self._h))

    def fp8_layers(self):
        """[(launch index, input tensor index, qexp)] of the conv3x3_f8 launches, in plan order."""
        n = self._lib.vp_fp8_layers(self._h, None, 0)
        if n < 0:
            raise ValueError("vp_fp8_layers: the engine was not created with VP_MFMA_FP8")
        buf = (Fp8Layer * max(n, 1))()
        self._lib.vp_fp8_layers(self._h, buf, n)
        return [(buf[i].launch, buf[i].tensor, buf[i].qexp) for i in range(n)]

    def set_fp8_exps(self, exps):
        e = np.ascontiguousarray(exps, dtype=np.int32)
        self._ck(self._lib.vp_set_fp8_exps(self._h, _ptr(e), int(e.size)))

    def infer_shared(self):
        """Run this shared-prefix engine's own layers on the frame its base engine processed last."""
        self._ck(self._lib.vp_infer_shared(self._h))

    def shared_level(self):
        return self._lib.vp_shared_level(self._h)

    def infer_tensor(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        h, w = self.input_hw()
        if x.size != 3 * h * w:
            raise ValueError(f"tensor must be 1x3x{h}x{w}")
        self._ck(self._lib.vp_infer_tensor(self._h, _ptr(x)))

    def logits(self):
        p = C.POINTER(C.c_float)()
        shape = (C.c_int64 * 4)()
        self._ck(self._lib.vp_logits(self._h, C.byref(p), shape))
        n = int(shape[1] * shape[2] * shape[3])
        return np.ctypeslib.as_array(p, shape=(n,)).reshape(tuple(shape)[1:]).copy()

    def mask(self):
        p = C.POINTER(C.c_uint8)()
        h, w = C.c_int(), C.c_int()
        self._ck(self._lib.vp_mask_u8(self._h, C.byref(p), C.byref(h), C.byref(w)))
        return np.ctypeslib.as_array(p, shape=(h.value * w.value,)).reshape(h.value, w.value).copy()

    def mask_resized(self, h, w):
        out = np.empty((h, w), dtype=np.uint8)
        self._ck(self._lib.vp_mask_resized_u8(self._h, _ptr(out), h, w))
        return out

    def depth_resized(self, h, w):
        out = np.empty((h, w), dtype=np.float32)
        self._ck(self._lib.vp_depth_resized_f32(self._h, _ptr(out), h, w))
        return out

    def visualize_depth(self, h, w):
        """Colourised depth (depth_visualization_engine.cpp): plane 0 of the logits at h x w, min-max -> u8 -> VIRIDIS; BGR8."""
        out = np.empty((h, w, 3), dtype=np.uint8)
        self._ck(self._lib.vp_visualize_depth_bgr8(self._h, _ptr(out), h, w))
        return out

    def visualize_mask(self, viz_type, frame_hw):
        """Blended BGR visualisation (masks_visualization_engine.cpp) of the last inference at the last frame's size;
        ValueError if ``frame_hw`` is not the geometry of the frame that was inferred last."""
        out = np.empty((frame_hw[0], frame_hw[1], 3), dtype=np.uint8)
        self._ck(self._lib.vp_visualize_mask_bgr8(self._h, int(viz_type), _ptr(out), int(frame_hw[0]), int(frame_hw[1])))
        return out

    def frame_hw(self):
        h, w = C.c_int(), C.c_int()
        self._ck(self._lib.vp_frame_hw(self._h, C.byref(h), C.byref(w)))
        return h.value, w.value

    def set_outputs(self, logits=True, mask=True):
        """Which outputs infer() / infer_shared() / infer_multi() copy to the host; the rest is fetched on first use."""
        self._ck(self._lib.vp_set_outputs(self._h, (VP_OUT_LOGITS if logits else 0) | (VP_OUT_MASK if mask else 0)))

    def host_logits_current(self):
        """True when the pinned host copy of the logits belongs to the last pass (vp_host_logits_current)."""
        return bool(self._lib.vp_host_logits_current(self._h))

    def output_shape(self):
        """(1, C, H, W) of the output tensor without fetching it (vp_output_shape)."""
        sh = (C.c_int64 * 4)()
        self._ck(self._lib.vp_output_shape(self._h, sh))
        return tuple(int(v) for v in sh)

    def output_dims(self):
        """(1, C, H, W) of the output tensor as the plan fixes it: answered before the first inference too (vp_output_dims)."""
        sh = (C.c_int64 * 4)()
        self._ck(self._lib.vp_output_dims(self._h, sh))
        return tuple(int(v) for v in sh)

    def set_pinned_staging(self, on):
        self._ck(self._lib.vp_set_pinned_staging(self._h, int(bool(on))))

    def set_multi_fork(self, on):
        """Latency mode (default): enqueue_multi / infer_multi fork the backbone-only heads; off for several cameras in flight."""
        self._ck(self._lib.vp_set_multi_fork(self._h, 1 if on else 0))

    def enqueue_multi(self, heads):
        """Asynchronous: this base engine and its shared-prefix ``heads`` as one graph launch (level-1 heads forked behind the
        backbone, overlapping this engine's own decoder); same results and stream order as enqueue() on each."""
        arr = (C.c_void_p * max(1, len(heads)))(*[h._h for h in heads])
        self._ck(self._lib.vp_enqueue_multi(self._h, arr, len(heads)))

    def infer_multi(self, heads, frame_u8):
        """One frame through this base engine and its shared-prefix ``heads``: one H2D, one host synchronisation."""
        f = np.ascontiguousarray(frame_u8, dtype=np.uint8)
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("frame must be HxWx3 uint8")
        arr = (C.c_void_p * max(1, len(heads)))(*[h._h for h in heads])
        self._ck(self._lib.vp_infer_multi(self._h, arr, len(heads), _ptr(f), f.shape[0], f.shape[1], f.strides[0]))

    def input_tensor(self):
        h, w = self.input_hw()
        out = np.empty((1, 3, h, w), dtype=np.float32)
        self._ck(self._lib.vp_input_tensor(self._h, _ptr(out)))
        return out

    # ---- device-resident path
    def upload_frame(self, frame_u8, index=None):
        """index: slot of a batched encoder (vp_upload_frame_n); None = the single-frame call."""
        f = np.ascontiguousarray(frame_u8, dtype=np.uint8)
        if index is None:
            self._keep = f
            self._ck(self._lib.vp_upload_frame(self._h, _ptr(f), f.shape[0], f.shape[1], f.strides[0]))
        else:
            self._keep_n = getattr(self, "_keep_n", {})
            self._keep_n[index] = f
            self._ck(self._lib.vp_upload_frame_n(self._h, int(index), _ptr(f), f.shape[0], f.shape[1], f.strides[0]))

    def upload_from_frame(self, frame, region=None):
        """vp_upload_from_frame: asynchronous region copy out of a device-resident Frame into this engine's frame buffer (region = (x0, y0, w, h); None =
        the whole frame); enqueue() / sync() / fetch_outputs() follow as behind upload_frame."""
        x0, y0, w, h = (0, 0, 0, 0) if region is None else (int(v) for v in region)
        self._ck(self._lib.vp_upload_from_frame(self._h, frame._h, x0, y0, w, h))

    def infer_frame(self, frame, region=None):
        """vp_infer_frame: infer() on a region of a device-resident Frame (no staging copy, no H2D)."""
        x0, y0, w, h = (0, 0, 0, 0) if region is None else (int(v) for v in region)
        self._ck(self._lib.vp_infer_frame(self._h, frame._h, x0, y0, w, h))

    def frames(self):
        return self._lib.vp_frames(self._h)

    def enqueue(self):
        self._ck(self._lib.vp_enqueue(self._h))

    def sync(self):
        self._ck(self._lib.vp_sync(self._h))

    def fetch_outputs(self):
        self._ck(self._lib.vp_fetch_outputs(self._h))

    def device_outputs(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.vp_device_outputs(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def use_graph(self, on):
        self._ck(self._lib.vp_use_graph(self._h, int(bool(on))))

    def timer_begin(self):
        self._ck(self._lib.vp_timer_begin(self._h))

    def timer_end(self):
        ms = C.c_float()
        self._ck(self._lib.vp_timer_end(self._h, C.byref(ms)))
        return ms.value

    # ---- introspection
    def layers(self):
        out = []
        for i in range(self._ck(self._lib.vp_layer_count(self._h))):
            name, fl, by = C.c_char_p(), C.c_double(), C.c_double()
            self._ck(self._lib.vp_layer_info(self._h, i, C.byref(name), C.byref(fl), C.byref(by)))
            out.append((name.value.decode(), fl.value, by.value))
        return out

    def layer_flops_executed(self):
        """matrix work each launch EXECUTES (differs from layers()' reference-formulation count for the composed up-sampling stages)"""
        out = []
        for i in range(self._ck(self._lib.vp_layer_count(self._h))):
            fl = C.c_double()
            self._ck(self._lib.vp_layer_flops_executed(self._h, i, C.byref(fl)))
            out.append(fl.value)
        return out

    def layer_kernels(self):
        out = []
        for i in range(self._ck(self._lib.vp_layer_count(self._h))):
            k = C.c_char_p()
            self._ck(self._lib.vp_layer_kernel(self._h, i, C.byref(k)))
            out.append(k.value.decode())
        return out

    def layer_launches(self):
        """launch geometry beyond the kernel tag ("nsplit=4", "groups=32", ""), per launch"""
        out = []
        for i in range(self._ck(self._lib.vp_layer_count(self._h))):
            k = C.c_char_p()
            self._ck(self._lib.vp_layer_launch(self._h, i, C.byref(k)))
            out.append(k.value.decode())
        return out

    def copy_outputs_device(self, logits_ptr=None, mask_ptr=None):
        self._ck(self._lib.vp_copy_outputs_device(self._h, logits_ptr, mask_ptr))

    def profile_layers(self, iters=10):
        n = self._ck(self._lib.vp_layer_count(self._h))
        ms = np.zeros(n, dtype=np.float32)
        self._ck(self._lib.vp_profile_layers(self._h, iters, _ptr(ms), n))
        return ms

    def tensors(self):
        out = []
        for i in range(self._ck(self._lib.vp_tensor_count(self._h))):
            name, c, h, w = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
            self._ck(self._lib.vp_tensor_info(self._h, i, C.byref(name), C.byref(c), C.byref(h), C.byref(w)))
            out.append((name.value.decode(), c.value, h.value, w.value))
        return out

    def tensor_read(self, i):
        _, c, h, w = self.tensors()[i]
        out = np.empty((c, h, w), dtype=np.float32)
        self._ck(self._lib.vp_tensor_read(self._h, i, _ptr(out)))
        return out

    def range_survey(self):
        """vp_range_survey over the resident input: one record per tensors() entry -- name, c, h, w, exp, absmax, count, nonfinite, zeros, bins (int64
        [VP_RANGE_BINS], bins[k] = stored values with floor(log2 |x|) == VP_RANGE_EXP_MIN + k).  count == 0: the plan never stores that tensor.  Values
        are STORED ones (tensor_read(i) * 2^-exp on an act_scale engine).  range_summary() derives headroom and the subnormal shares from a record."""
        info = self.tensors()
        buf = (RangeStats * max(1, len(info)))()
        n = self._ck(self._lib.vp_range_survey(self._h, C.cast(buf, C.c_void_p), len(info)))
        if n != len(info):
            raise VpError(f"vp_range_survey answered {n} tensors, vp_tensor_count {len(info)}")
        return [{"name": name, "c": c, "h": h, "w": w, "exp": int(r.exp), "absmax": np.float32(r.absmax), "count": int(r.count), "nonfinite": int(r.nonfinite),
                 "zeros": int(r.zeros), "bins": np.array(r.bins[:], dtype=np.int64)} for (name, c, h, w), r in zip(info, buf)]


class Frame:
    """vp_frame: one camera frame, uploaded once in its native format, converted to BGR8 on the device and handed to any number of consumers
    (Engine.infer_frame / upload_from_frame, Detector.infer_frame).  One thread uploads, any number consume; ping-pong two Frames between capture
    and consumers (include/vp_hip.h)."""

    def __init__(self, gpu_id=0):
        self._lib = load()
        self._h = _P()
        err = C.create_string_buffer(512)
        rc = self._lib.vp_frame_create(C.byref(self._h), gpu_id, err, len(err))
        if rc != 0:
            self._h = None
            raise (ValueError if rc == -1 else VpError)(f"vp_frame_create failed ({rc}): {err.value.decode(errors='replace')}")
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_frame_destroy(self._h)
            self._h = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_frame_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpError)(f"libvp_hip frame error {rc}: {msg}")
        return rc

    @staticmethod
    def _fmt(fmt):
        return FRAME_FORMATS[fmt.lower()] if isinstance(fmt, str) else int(fmt)

    def upload(self, array_or_planes, fmt="bgr8", hw=None):
        """vp_frame_upload (asynchronous).  One uint8 array -- HxWx3 (bgr8 / rgb8), HxWx4 (bgra8 / rgba8), HxW (gray8), Hx(2W) or HxWx2 (yuy2 / uyvy) -- or,
        for nv12, the pair (Y [H][W], UV [H/2][W]) or one [H * 3 / 2][W] array; for nv21 the pair (Y, VU); for i420 / yv12 the three planes (Y [H][W],
        then U, V / V, U [H/2][W/2]); for those three also ONE flat contiguous buffer of H * W * 3 / 2 bytes, 1-D (with `hw`) or [H * 3 / 2][W].  The
        upload-only formats: HxW uint8 (bayer_*8), HxW uint16 (bayer_*16, gray16), for p010 the pair (Y [H][W], UV [H/2][W]) of uint16 arrays; a
        uint8 array is taken as the bytes of the little-endian words.  Row strides are taken from the arrays (the bytes of a row must be contiguous);
        `hw` overrides the (h, w) read off plane 0."""
        f = self._fmt(fmt)
        planes = list(array_or_planes) if isinstance(array_or_planes, (list, tuple)) else [array_or_planes]
        planes = [np.asarray(p) for p in planes]
        if f == VP_FRAME_NV12 and len(planes) == 1 and planes[0].ndim == 2 and planes[0].shape[0] % 3 == 0:
            a = planes[0]
            planes = [a[: a.shape[0] // 3 * 2], a[a.shape[0] // 3 * 2:]]
        if f in (VP_FRAME_I420, VP_FRAME_YV12, VP_FRAME_NV21) and len(planes) == 1:
            a = np.ascontiguousarray(planes[0], dtype=np.uint8)
            fh, fw = (int(hw[0]), int(hw[1])) if hw is not None else ((a.shape[0] // 3 * 2, a.shape[1]) if a.ndim == 2 else (0, 0))
            a = a.reshape(-1)
            if fh < 2 or fw < 2 or fh % 2 or fw % 2 or a.size != fh * fw * 3 // 2:
                pass   # not a flat frame of that size: one plane where the format has more, the library words the refusal
            elif f == VP_FRAME_NV21:
                planes = [a[:fh * fw].reshape(fh, fw), a[fh * fw:].reshape(fh // 2, fw)]
            else:
                q = fh * fw // 4
                planes = [a[:fh * fw].reshape(fh, fw), a[fh * fw:fh * fw + q].reshape(fh // 2, fw // 2), a[fh * fw + q:].reshape(fh // 2, fw // 2)]
        fixed = []
        for p in planes:
            # the 16-bit formats take uint16 arrays (little-endian words) as they are; their byte strides go to the library like any other
            dt = np.dtype("<u2") if f in _FRAME_WORDS and p.dtype.itemsize == 2 and p.dtype.kind == "u" else np.dtype(np.uint8)
            if p.dtype != dt or p.ndim < 2 or any(p.strides[i] != int(np.prod(p.shape[i + 1:])) * dt.itemsize for i in range(1, p.ndim)) or p.strides[0] < 0:
                p = np.ascontiguousarray(p, dtype=dt)
            fixed.append(p)
        p0 = fixed[0]
        h, w = (int(hw[0]), int(hw[1])) if hw is not None else (p0.shape[0], int(np.prod(p0.shape[1:])) * p0.dtype.itemsize // _FRAME_PX_BYTES[f] if f in _FRAME_PX_BYTES else 0)
        self._keep = fixed   # a registered pool is read by DMA after the call returns
        arr = (_P * len(fixed))(*[p.ctypes.data for p in fixed])
        strides = (C.c_int * len(fixed))(*[int(p.strides[0]) for p in fixed])
        self._ck(self._lib.vp_frame_upload(self._h, f, arr, strides, len(fixed), h, w))

    def upload_device(self, plane_ptrs, strides, fmt, h, w, producer_stream=None):
        """vp_frame_upload_device: device pointers (ints) of the planes on this frame's GPU and their row strides in bytes; producer_stream: the
        hipStream_t handle (int) the planes are ready on, None = ready now.  The planes stay valid and unmodified until sync() or a consumer's
        synchronising call."""
        arr = (_P * len(plane_ptrs))(*[int(p) for p in plane_ptrs])
        st = (C.c_int * len(strides))(*[int(s) for s in strides])
        self._ck(self._lib.vp_frame_upload_device(self._h, self._fmt(fmt), arr, st, len(plane_ptrs), int(h), int(w), _P(int(producer_stream)) if producer_stream else None))

    def set_color(self, matrix="bt601", range="limited"):  # noqa: A002 -- the C ABI's word
        """vp_frame_set_color: the colour standard of LATER YUV uploads -- matrix "bt601" / "bt709", range "limited" / "full" (or the VP_COLOR_* values)"""
        self._ck(self._lib.vp_frame_set_color(self._h, _named(COLOR_MATRICES, matrix), _named(COLOR_RANGES, range)))

    def get_color(self):
        """(matrix, range) as VP_COLOR_* values"""
        m, r = C.c_int(), C.c_int()
        self._ck(self._lib.vp_frame_get_color(self._h, C.byref(m), C.byref(r)))
        return m.value, r.value

    def set_raw(self, bits=0, shift=0, black=0, gains=(256, 256, 256), ccm=None, lut=None):
        """vp_frame_set_raw: the setting of LATER uploads of the Bayer formats -- bits: the significant bits (0: the container's width), shift: right
        shift of every sample, black: level subtracted behind it, gains: Q8 in R, G, B order, ccm: None or nine Q10 integers (rows and columns R, G, B),
        lut: None or 256 / 1024 / 4096 uint8 entries (copied at the call).  The arithmetic: include/vp_hip.h."""
        r = Raw()
        r.bits, r.shift, r.black = int(bits), int(shift), int(black)
        r.gains[:] = [int(g) for g in gains]
        r.ccm_on = 0 if ccm is None else 1
        r.ccm[:] = [0] * 9 if ccm is None else [int(v) for v in np.asarray(ccm).reshape(9)]
        table = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1)
        r.lut, r.lut_len = (None, 0) if table is None else (table.ctypes.data, int(table.size))
        self._ck(self._lib.vp_frame_set_raw(self._h, C.byref(r)))

    def get_raw(self):
        """the setting in force as a dict (bits, shift, black, gains, ccm: None when off, lut_len: 0 when no LUT is installed)"""
        r = Raw()
        self._ck(self._lib.vp_frame_get_raw(self._h, C.byref(r)))
        return {"bits": r.bits, "shift": r.shift, "black": r.black, "gains": tuple(r.gains[:]), "ccm": tuple(r.ccm[:]) if r.ccm_on else None, "lut_len": r.lut_len}

    def set_rectify(self, K, dist=None, H=None, out_hw=None, mode="two_pass"):
        """vp_frame_set_rectify: LATER uploads are undistorted (K 3x3, dist = (k1, k2, p1, p2, k3)) and warped by the homography H (source -> destination,
        3x3) to out_hw = (h, w) on the device; the frame then IS that picture (hw(), fetch_bgr8(), every consumer, Canvas.begin).  mode "two_pass" (the
        calibration protocol's pipeline) or "one_pass" (one resampling, not bit-equal).  K = None switches rectification off."""
        if K is None:
            self._ck(self._lib.vp_frame_set_rectify(self._h, None))
            return
        r = _rectify(K, dist, H, out_hw, mode)
        self._ck(self._lib.vp_frame_set_rectify(self._h, C.byref(r)))

    def get_rectify(self):
        """the setting in force as a dict (K, dist, H, out_hw, mode), None when rectification is off"""
        r = Rectify()
        rc = self._lib.vp_frame_get_rectify(self._h, C.byref(r))
        if rc == -4:
            return None
        self._ck(rc)
        return {"K": np.array(r.K[:]).reshape(3, 3), "dist": np.array(r.dist[:]), "H": np.array(r.H[:]).reshape(3, 3), "out_hw": (r.out_h, r.out_w), "mode": r.mode}

    def sync(self):
        self._ck(self._lib.vp_frame_sync(self._h))

    def hw(self):
        h, w = C.c_int(), C.c_int()
        rc = self._lib.vp_frame_dims(self._h, C.byref(h), C.byref(w))
        if rc != 0:
            raise VpError(f"vp_frame_dims failed ({rc}): nothing was uploaded yet")
        return h.value, w.value

    def fetch_bgr8(self):
        """the converted image, HxWx3 uint8 (synchronises the frame's stream)"""
        h, w = self.hw()
        out = np.empty((h, w, 3), np.uint8)
        self._ck(self._lib.vp_frame_fetch_bgr8(self._h, _ptr(out), out.strides[0]))
        return out


def rectify_map(K, dist, H, out_hw, src_hw, which, mode="two_pass"):
    """vp_rectify_map (host only): the map "undistort" (0), "warp" (1) or "one_pass" (2) of the setting for a src_hw = (h, w) source ->
    (xy int16 [rows][cols][2] = (ix, iy), frac uint16 [rows][cols] = fy << 5 | fx); rows x cols = src_hw for "undistort", out_hw otherwise.
    ValueError for a setting or a size the library refuses."""
    r = _rectify(K, dist, H, out_hw, mode)
    which = _named(RECTIFY_MAPS, which)
    rows, cols = (int(src_hw[0]), int(src_hw[1])) if which == 0 else (r.out_h, r.out_w)
    ok = 2 <= rows <= 16384 and 2 <= cols <= 16384
    xy = np.empty((rows, cols, 2) if ok else (1, 1, 2), np.int16)
    frac = np.empty((rows, cols) if ok else (1, 1), np.uint16)
    rc = load().vp_rectify_map(C.byref(r), int(src_hw[0]), int(src_hw[1]), which, _ptr(xy), _ptr(frac))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_rectify_map failed ({rc}): a setting, a source size or a map the library refuses")
    return xy, frac


def _camera_pose(d):
    p = CameraPose()
    p.pitch_deg, p.yaw_deg, p.roll_deg = float(d.get("pitch", 0.0)), float(d.get("yaw", 0.0)), float(d.get("roll", 0.0))
    p.camera_height = float(d.get("camera_height", 0.0))
    p.K[:] = [float(v) for v in np.asarray(d.get("intrinsic_matrix", np.eye(3)), dtype=np.float64).reshape(9)]
    p.img_w, p.img_h = int(d.get("img_width", 0)), int(d.get("img_height", 0))
    p.hfov_deg = float(d.get("hfov", 0.0))
    return p


def rectify_homography(inference_pose, standard_pose):
    """vp_rectify_homography (host only): the two config dicts of the calibration demo -- inference: pitch, yaw, roll (degrees), camera_height,
    intrinsic_matrix; standard: pitch, yaw, roll, camera_height, img_width, img_height, hfov (degrees) -> H 3x3 float64, source -> standard pose."""
    pi, ps = _camera_pose(inference_pose), _camera_pose(standard_pose)
    H = np.empty(9, np.float64)
    rc = load().vp_rectify_homography(C.byref(pi), C.byref(ps), _ptr(H))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_rectify_homography failed ({rc}): a pose the library refuses")
    return H.reshape(3, 3)


def op_remap_bgr8(src, xy, frac, border="replicate", dst_stride=None, gpu_id=0):
    """vp_op_remap_bgr8: frame_remap_kernel on src (uint8 [h][w][3]; a view with its own row stride is passed as it is) through the map (xy int16
    [oh][ow][2], frac uint16 [oh][ow]).  dst_stride None: the picture [oh][ow][3]; else the raw destination rows [oh][dst_stride], where bytes the
    entry does not write stay 0xAA."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3 or src.strides[2] != 1 or src.strides[1] != 3 or src.strides[0] < 0:
        src = np.ascontiguousarray(src, dtype=np.uint8)
    xy = np.ascontiguousarray(xy, dtype=np.int16)
    frac = np.ascontiguousarray(frac, dtype=np.uint16)
    oh, ow = frac.shape
    stride = 3 * ow if dst_stride is None else int(dst_stride)
    out = np.full((oh, max(stride, 1)), 0xAA, np.uint8)
    err = C.create_string_buffer(512)
    rc = load().vp_op_remap_bgr8(gpu_id, C.c_void_p(src.ctypes.data), src.shape[0], src.shape[1], int(src.strides[0]), _ptr(xy), _ptr(frac), oh, ow,
                                 _named(BORDERS, border), _ptr(out), stride, err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_remap_bgr8 failed ({rc}): {err.value.decode(errors='replace')}")
    return out.reshape(oh, ow, 3) if dst_stride is None else out


def canvas_layout(fmt, h, w):
    """vp_canvas_layout (host only): [(bytes per row, rows)] of each plane an h x w picture has in `fmt`; ValueError for a geometry the format refuses."""
    n = C.c_int()
    rb, rows = (C.c_int * 2)(), (C.c_int * 2)()
    if load().vp_canvas_layout(Frame._fmt(fmt), int(h), int(w), C.byref(n), rb, rows) != 0:
        raise ValueError(f"vp_canvas_layout: no {fmt} layout for a {w} x {h} picture")
    return [(rb[i], rows[i]) for i in range(n.value)]


def canvas_layout3(fmt, h, w):
    """vp_canvas_layout3 (host only): canvas_layout for every format, the three-plane ones (i420, yv12) included"""
    n = C.c_int()
    rb, rows = (C.c_int * 3)(), (C.c_int * 3)()
    if load().vp_canvas_layout3(Frame._fmt(fmt), int(h), int(w), C.byref(n), rb, rows) != 0:
        raise ValueError(f"vp_canvas_layout3: no {fmt} layout for a {w} x {h} picture")
    return [(rb[i], rows[i]) for i in range(n.value)]


def _op_raise(entry, rc, err):
    raise (ValueError if rc == -1 else VpError)(f"{entry} failed ({rc}): {err.value.decode(errors='replace')}")


def jpeg_bound(h, w, restart_mcus=0):
    """vp_jpeg_bound (host only): a buffer size that holds the JPEG of any h x w picture at `restart_mcus`"""
    n, err = C.c_size_t(), C.create_string_buffer(512)
    rc = load().vp_jpeg_bound(int(h), int(w), int(restart_mcus), C.byref(n), err, len(err))
    if rc != 0:
        _op_raise("vp_jpeg_bound", rc, err)
    return n.value


def jpeg_header(h, w, quality=90, restart_mcus=0):
    """vp_jpeg_header (host only): the stream's first 629 bytes, SOI through SOS"""
    buf, n, err = np.empty(1024, np.uint8), C.c_size_t(), C.create_string_buffer(512)
    rc = load().vp_jpeg_header(int(h), int(w), int(quality), int(restart_mcus), _ptr(buf), buf.size, C.byref(n), err, len(err))
    if rc != 0:
        _op_raise("vp_jpeg_header", rc, err)
    return buf[:n.value].tobytes()


def jpeg_encode(bgr, quality=90, restart_mcus=0, cap=None, gpu_id=0):
    """vp_op_jpeg_encode_bgr8: the baseline JPEG (bytes) of bgr (uint8 [h][w][3]; a view with its own row stride is passed as it is), encoded on the
    device.  cap: the size of the buffer offered (default: jpeg_bound)."""
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3 or bgr.strides[2] != 1 or bgr.strides[1] != 3 or bgr.strides[0] < 0:
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w = bgr.shape[:2]
    n, err = C.c_size_t(), C.create_string_buffer(512)
    buf = np.empty(max(1, jpeg_bound(h, w, restart_mcus) if cap is None else int(cap)), np.uint8)
    rc = load().vp_op_jpeg_encode_bgr8(gpu_id, C.c_void_p(bgr.ctypes.data), h, w, int(bgr.strides[0]), int(quality), int(restart_mcus), _ptr(buf), buf.size,
                                       C.byref(n), err, len(err))
    if rc != 0:
        _op_raise("vp_op_jpeg_encode_bgr8", rc, err)
    return buf[:n.value].tobytes()


class Canvas:
    """vp_canvas: one picture per camera frame, composed on the device.  begin(frame) copies the Frame's BGR8 picture; every Engine (heads included)
    blends its mask or pastes its depth map into the region its input came from; detections are drawn as boxes; overlay_lanes draws an EgoLanes
    engine's lanes in the production display's look and draw_lane_rows an AutoSteer engine's rows; fetch(fmt) returns the picture once, in any Frame
    format, at its own size or (size=) resized on the device.  One thread drives a canvas (include/vp_hip.h)."""

    def __init__(self, gpu_id=0):
        self._lib = load()
        self._h = _P()
        err = C.create_string_buffer(512)
        rc = self._lib.vp_canvas_create(C.byref(self._h), gpu_id, err, len(err))
        if rc != 0:
            self._h = None
            raise (ValueError if rc == -1 else VpError)(f"vp_canvas_create failed ({rc}): {err.value.decode(errors='replace')}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_canvas_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_canvas_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpError)(f"libvp_hip canvas error {rc}: {msg}")
        return rc

    def begin(self, frame):
        self._ck(self._lib.vp_canvas_begin(self._h, frame._h))

    def blend_mask(self, engine, viz_type=VP_VIZ_SCENE):
        self._ck(self._lib.vp_canvas_blend_mask(self._h, engine._h, int(viz_type)))

    def blend_mask_u8(self, mask, viz_type, region, device_hw=None):
        """mask: an HxW uint8 array, or (with device_hw = (mh, mw)) a device pointer (int); region: (x0, y0, w, h) of the canvas"""
        x0, y0, w, h = (int(v) for v in region)
        if device_hw is not None:
            self._ck(self._lib.vp_canvas_blend_mask_u8(self._h, _P(int(mask)), 1, int(device_hw[0]), int(device_hw[1]), int(viz_type), x0, y0, w, h))
            return
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != 2:
            raise ValueError("blend_mask_u8: the mask is an HxW uint8 array")
        self._ck(self._lib.vp_canvas_blend_mask_u8(self._h, _ptr(m), 0, m.shape[0], m.shape[1], int(viz_type), x0, y0, w, h))

    def paste_depth(self, engine):
        self._ck(self._lib.vp_canvas_paste_depth(self._h, engine._h))

    def draw_detections(self, rows):
        """rows: [n][6] x1, y1, x2, y2, confidence, class_id, as Detector.infer / postprocess return them"""
        r = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 6)
        rec = r.copy()
        rec[:, 5].view(np.int32)[:] = r[:, 5].astype(np.int32)   # vp_detection.class_id is an int
        self._ck(self._lib.vp_canvas_draw_detections(self._h, _ptr(rec) if len(rec) else None, len(rec)))

    def sync(self):
        self._ck(self._lib.vp_canvas_sync(self._h))

    def hw(self):
        h, w = C.c_int(), C.c_int()
        rc = self._lib.vp_canvas_dims(self._h, C.byref(h), C.byref(w))
        if rc != 0:
            raise VpError(f"vp_canvas_dims failed ({rc}): the canvas holds no picture yet")
        return h.value, w.value

    def device(self):
        """(device pointer of the BGR8 picture, row pitch in bytes): valid until the next begin() / close(), complete after sync()"""
        p, pitch = _P(), C.c_int()
        rc = self._lib.vp_canvas_device(self._h, C.byref(p), C.byref(pitch))
        if rc != 0:
            raise VpError(f"vp_canvas_device failed ({rc}): the canvas holds no picture yet")
        return p.value, pitch.value

    def set_color(self, matrix="bt601", range="limited", chroma_mode="even"):  # noqa: A002 -- the C ABI's word
        """vp_canvas_set_color: the colour standard and chroma rule ("even" / "mean") of LATER fetches into the YUV formats and gray8.  Not inherited from
        the frame the canvas is begun on."""
        self._ck(self._lib.vp_canvas_set_color(self._h, _named(COLOR_MATRICES, matrix), _named(COLOR_RANGES, range), _named(CHROMA_MODES, chroma_mode)))

    def get_color(self):
        """(matrix, range, chroma_mode) as VP_COLOR_* / VP_CHROMA_* values"""
        m, r, k = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._lib.vp_canvas_get_color(self._h, C.byref(m), C.byref(r), C.byref(k)))
        return m.value, r.value, k.value

    def add_planes(self, planes, threshold, add_bgr, region, device_shape=None):
        """vp_canvas_add_planes_f32.  planes: an [n][mh][mw] float32 array, or (with device_shape = (n, mh, mw)) a device pointer (int); add_bgr: [n][3]
        uint8 increments; region: (x0, y0, w, h) of the canvas"""
        x0, y0, w, h = (int(v) for v in region)
        add = np.ascontiguousarray(add_bgr, dtype=np.uint8).reshape(-1, 3)
        if device_shape is not None:
            n, mh, mw = (int(v) for v in device_shape)
            src, on_device = _P(int(planes)), 1
        else:
            p = np.ascontiguousarray(planes, dtype=np.float32)
            if p.ndim != 3:
                raise ValueError("add_planes: the planes are an [n][mh][mw] float32 array")
            (n, mh, mw), src, on_device = p.shape, _ptr(p), 0
        if len(add) != n:
            raise ValueError(f"add_planes: {n} planes but {len(add)} increments")
        self._ck(self._lib.vp_canvas_add_planes_f32(self._h, src, on_device, n, mh, mw, float(threshold), _ptr(add), x0, y0, w, h))

    def overlay_lanes(self, engine, threshold=0.0):
        """vp_canvas_overlay_lanes: the production display's three additive lane overlays, from an EgoLanes engine's device logits"""
        self._ck(self._lib.vp_canvas_overlay_lanes(self._h, engine._h, float(threshold)))

    def draw_points(self, xy, radius=3, bgr=(0, 255, 0)):
        """vp_canvas_draw_points: xy [n][2] integer (x, y) in canvas pixels, each a filled disc of `radius` in `bgr`"""
        pts = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        col = np.array(bgr, dtype=np.uint8).reshape(3)
        self._ck(self._lib.vp_canvas_draw_points(self._h, _ptr(pts) if len(pts) else None, len(pts), int(radius), _ptr(col)))

    def draw_lane_rows(self, engine):
        """vp_canvas_draw_lane_rows: the valid rows of an AutoSteer engine, read on the device"""
        self._ck(self._lib.vp_canvas_draw_lane_rows(self._h, engine._h))

    def fetch(self, fmt="bgr8", strides=None, size=None):
        """vp_canvas_fetch (synchronous): the picture as numpy planes -- bgr8 / rgb8 HxWx3, bgra8 / rgba8 HxWx4, gray8 HxW, yuy2 / uyvy Hx(2W), nv12 / nv21
        the pair (Y [H][W], UV / VU [H/2][W]), i420 / yv12 the three planes (Y [H][W], U, V / V, U [H/2][W/2]).  `strides`: row strides in bytes of the
        buffers fetched into (default: packed).  `size` = (out_h, out_w): vp_canvas_fetch_resized -- the picture resized on the device (the integer
        bilinear of the preprocess path), H x W above being the size asked for; the canvas keeps its full-size picture."""
        f = Frame._fmt(fmt)
        h, w = self.hw() if size is None else (int(size[0]), int(size[1]))
        n = C.c_int()
        rb, rows = (C.c_int * 3)(), (C.c_int * 3)()
        if self._lib.vp_canvas_layout3(f, h, w, C.byref(n), rb, rows) != 0:
            n.value = _FRAME_PLANES.get(f, 1)   # no layout: the library words the refusal
            for i in range(3):
                rb[i], rows[i] = 1, 1
            if size is not None and min(h, w) == 1 and max(h, w) <= 16384 and f <= VP_FRAME_GRAY8:   # a side of 1: layouts start at 2, the resized fetch at 1
                rb[0], rows[0] = _FRAME_PX_BYTES[f] * w, h
        st = [int(v) for v in strides] if strides is not None else [rb[i] for i in range(n.value)]
        bufs = [np.zeros((rows[min(i, 2)], max(st[i], 1)), np.uint8) for i in range(len(st))]
        arr = (_P * len(bufs))(*[b.ctypes.data for b in bufs])
        if size is None:
            self._ck(self._lib.vp_canvas_fetch(self._h, f, arr, (C.c_int * len(st))(*st), len(st)))
        else:
            self._ck(self._lib.vp_canvas_fetch_resized(self._h, f, h, w, arr, (C.c_int * len(st))(*st), len(st)))
        planes = [np.ascontiguousarray(b[:, :rb[min(i, 2)]]) for i, b in enumerate(bufs)]
        if f <= VP_FRAME_RGBA8:
            planes[0] = planes[0].reshape(h, w, _FRAME_PX_BYTES[f])
        return planes[0] if len(planes) == 1 else tuple(planes)

    def fetch_jpeg(self, quality=90, restart_mcus=0, size=None):
        """vp_canvas_fetch_jpeg (synchronous): the picture as a baseline JPEG (bytes; JFIF, 4:2:0), encoded on the device -- what
        cv2.VideoWriter(.., "MJPG").write(frame) makes on the host.  `size` = (out_h, out_w): vp_canvas_fetch_jpeg_resized, the picture resized on the
        device first.  Fetched into jpeg_bound bytes of fresh address space, of which only the stream's bytes are touched."""
        try:
            h, w = self.hw() if size is None else (int(size[0]), int(size[1]))
            cap = jpeg_bound(h, w, restart_mcus)
        except (ValueError, VpError):
            h, w, cap = 0, 0, 1024   # no picture or no such geometry: the library words the refusal
        buf, n = np.empty(cap, np.uint8), C.c_size_t()
        if size is None:
            self._ck(self._lib.vp_canvas_fetch_jpeg(self._h, int(quality), int(restart_mcus), _ptr(buf), buf.size, C.byref(n)))
        else:
            self._ck(self._lib.vp_canvas_fetch_jpeg_resized(self._h, int(size[0]), int(size[1]), int(quality), int(restart_mcus), _ptr(buf), buf.size, C.byref(n)))
        return buf[:n.value].tobytes()


class Metric:
    """vp_metric: the reference's validation scores (IoU of the segmentation trainers, mAE / mEL of the depth trainer) computed on the device, one record
    per frame.  add_* reads an Engine's device-resident logits behind its pass (or the caller's arrays) and returns without waiting; fetch() is the one
    synchronisation: (records, summary) -- a numpy array of METRIC_FRAME_DTYPE and a dict.  One thread drives a metric (include/vp_hip.h)."""

    def __init__(self, gpu_id=0, max_frames=4096):
        self._lib = load()
        self._h = _P()
        err = C.create_string_buffer(512)
        rc = self._lib.vp_metric_create(C.byref(self._h), gpu_id, int(max_frames), err, len(err))
        if rc != 0:
            self._h = None
            raise (ValueError if rc == -1 else VpError)(f"vp_metric_create failed ({rc}): {err.value.decode(errors='replace')}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_metric_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_metric_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpError)(f"libvp_hip metric error {rc}: {msg}")
        return rc

    @staticmethod
    def _arg(a, dtype, device):
        """(pointer, on_device, keep-alive): a numpy array (host) or, with device=True, a device pointer (int)"""
        if device:
            return _P(int(a)), 1, None
        arr = np.ascontiguousarray(a, dtype=dtype)
        return _ptr(arr), 0, arr

    def reset(self):
        self._ck(self._lib.vp_metric_reset(self._h))

    def frames(self):
        return self._ck(self._lib.vp_metric_frames(self._h))

    def add_seg(self, engine, gt, gt_form="label", gt_device=False):
        """gt: uint8 [h][w] of the engine's output size (or a device pointer with gt_device=True); gt_form: "label" or "bits" (VP_GT_LABEL, VP_GT_BITS)"""
        g, dev, keep = self._arg(gt, np.uint8, gt_device)
        if keep is not None and keep.size != int(np.prod(engine.output_dims()[-2:])):
            raise ValueError("add_seg: the ground truth has the engine's output size")
        self._ck(self._lib.vp_metric_add_seg(self._h, engine._h, g, dev, _named(GT_FORMS, gt_form)))

    def add_depth(self, engine, gt, gt_device=False):
        g, dev, keep = self._arg(gt, np.float32, gt_device)
        if keep is not None and keep.size != int(np.prod(engine.output_dims()[-2:])):
            raise ValueError("add_depth: the ground truth has the engine's output size")
        self._ck(self._lib.vp_metric_add_depth(self._h, engine._h, g, dev))

    def add_seg_pair(self, engine, ref):
        self._ck(self._lib.vp_metric_add_seg_pair(self._h, engine._h, ref._h))

    def add_depth_pair(self, engine, ref):
        self._ck(self._lib.vp_metric_add_depth_pair(self._h, engine._h, ref._h))

    def add_seg_logits(self, logits, gt, gt_form="label", device_chw=None):
        """logits fp32 [c][h][w] and gt uint8 [h][w]: numpy arrays, or (with device_chw = (c, h, w)) device pointers (ints)"""
        if device_chw is not None:
            c, h, w = (int(v) for v in device_chw)
            self._ck(self._lib.vp_metric_add_seg_logits(self._h, _P(int(logits)), 1, c, h, w, _P(int(gt)), 1, _named(GT_FORMS, gt_form)))
            return
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        g = np.ascontiguousarray(gt, dtype=np.uint8)
        if lg.ndim != 3 or g.shape != lg.shape[1:]:
            raise ValueError("add_seg_logits: logits [c][h][w] and a ground truth [h][w]")
        self._ck(self._lib.vp_metric_add_seg_logits(self._h, _ptr(lg), 0, lg.shape[0], lg.shape[1], lg.shape[2], _ptr(g), 0, _named(GT_FORMS, gt_form)))

    def add_depth_plane(self, pred, gt, device_hw=None):
        if device_hw is not None:
            self._ck(self._lib.vp_metric_add_depth_plane(self._h, _P(int(pred)), 1, _P(int(gt)), 1, int(device_hw[0]), int(device_hw[1])))
            return
        p = np.ascontiguousarray(pred, dtype=np.float32)
        g = np.ascontiguousarray(gt, dtype=np.float32)
        if p.ndim != 2 or g.shape != p.shape:
            raise ValueError("add_depth_plane: two planes [h][w] of one size")
        self._ck(self._lib.vp_metric_add_depth_plane(self._h, _ptr(p), 0, _ptr(g), 0, p.shape[0], p.shape[1]))

    def det_frames(self):
        return self._ck(self._lib.vp_metric_det_frames(self._h))

    def add_det(self, engine, labels, conf=DET_CONF, iou=DET_IOU, iou_v=None):
        """the detector's validation record of a VP_AUTOSPEED engine's last pass; labels: rows [cls, cx, cy, w, h] normalised to the network input (or None)"""
        lb, lp, n = _det_labels(labels)
        t, tp, nt = _det_table(iou_v)
        self._ck(self._lib.vp_metric_add_det(self._h, engine._h, lp, n, conf, iou, tp, nt))

    def add_det_pair(self, engine, ref, label_conf=0.25, conf=DET_CONF, iou=DET_IOU, iou_v=None):
        """ref's own kept rows with score > label_conf are the labels"""
        t, tp, nt = _det_table(iou_v)
        self._ck(self._lib.vp_metric_add_det_pair(self._h, engine._h, ref._h, label_conf, conf, iou, tp, nt))

    def add_det_raw(self, raw, labels, net_hw=(512, 1024), conf=DET_CONF, iou=DET_IOU, iou_v=None, device_shape=None):
        """raw fp32 [4 + nc][nb]: a numpy array, or (with device_shape = (nc, nb)) a device pointer (int)"""
        lb, lp, n = _det_labels(labels)
        t, tp, nt = _det_table(iou_v)
        if device_shape is not None:
            nc, nb = (int(v) for v in device_shape)
            self._ck(self._lib.vp_metric_add_det_raw(self._h, _P(int(raw)), 1, nc, nb, int(net_hw[0]), int(net_hw[1]), lp, n, conf, iou, tp, nt))
            return
        x = np.ascontiguousarray(raw, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] < 5:
            raise ValueError("add_det_raw: a tensor [4 + nc][nb]")
        self._ck(self._lib.vp_metric_add_det_raw(self._h, _ptr(x), 0, x.shape[0] - 4, x.shape[1], int(net_hw[0]), int(net_hw[1]), lp, n, conf, iou, tp, nt))

    def fetch_det(self):
        """(frames, rows, summary): numpy arrays of METRIC_DET_FRAME_DTYPE and METRIC_DET_ROW_DTYPE (frame f's rows: rows[first_row : first_row + kept]) and a dict"""
        n = self.det_frames()
        fr = np.zeros(n, dtype=METRIC_DET_FRAME_DTYPE)
        rows = np.zeros(n * VP_DET_MAX_DET, dtype=METRIC_DET_ROW_DTYPE)
        s = MetricDetSummary()
        self._ck(self._lib.vp_metric_fetch_det(self._h, _ptr(fr) if n else None, n, _ptr(rows) if n else None, rows.size, C.byref(s)))
        return fr, rows[:s.rows].copy(), _det_summary_dict(s)

    # ---- the lane part: EgoLanes frames and AutoSteer lines, counted apart
    @staticmethod
    def _lanes_gt(gt, gt_form, h, w, device):
        """(pointer, on_device, keep-alive, form): "planes" float32 [3][h][w], "bits" uint8 [h][w], "bits4x" uint8 [4h][4w]"""
        form = _named(LANES_GT_FORMS, gt_form)
        if form not in (0, 1, 2):
            raise ValueError("gt_form: 'planes', 'bits' or 'bits4x'")
        if device:
            return _P(int(gt)), 1, None, form
        arr = np.ascontiguousarray(gt, dtype=np.float32 if form == 0 else np.uint8)
        if arr.shape != ((3, h, w), (h, w), (4 * h, 4 * w))[form]:
            raise ValueError("lanes ground truth: float32 [3][h][w], uint8 [h][w] or uint8 [4h][4w] for an output of h x w")
        return _ptr(arr), 0, arr, form

    def lanes_frames(self):
        return self._ck(self._lib.vp_metric_lanes_frames(self._h))

    def add_lanes(self, engine, gt, gt_form="bits", gt_device=False):
        """the EgoLanes validation record of a VP_EGOLANES engine's last pass; gt: a numpy array in one of the three forms (or a device pointer with gt_device=True)"""
        h, w = engine.output_dims()[-2:]
        g, dev, keep, form = self._lanes_gt(gt, gt_form, h, w, gt_device)
        self._ck(self._lib.vp_metric_add_lanes(self._h, engine._h, g, dev, form))

    def add_lanes_pair(self, engine, ref):
        """ref's own prediction (1 where its logit > 0) is the ground truth"""
        self._ck(self._lib.vp_metric_add_lanes_pair(self._h, engine._h, ref._h))

    def add_lanes_logits(self, logits, gt, gt_form="bits", device_hw=None):
        """logits fp32 [3][h][w] and gt in one of the three forms: numpy arrays, or (with device_hw = (h, w)) device pointers (ints)"""
        if device_hw is not None:
            h, w = (int(v) for v in device_hw)
            self._ck(self._lib.vp_metric_add_lanes_logits(self._h, _P(int(logits)), 1, h, w, _P(int(gt)), 1, _named(LANES_GT_FORMS, gt_form)))
            return
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        if lg.ndim != 3 or lg.shape[0] != 3:
            raise ValueError("add_lanes_logits: logits [3][h][w]")
        g, dev, keep, form = self._lanes_gt(gt, gt_form, lg.shape[1], lg.shape[2], False)
        self._ck(self._lib.vp_metric_add_lanes_logits(self._h, _ptr(lg), 0, lg.shape[1], lg.shape[2], g, dev, form))

    def fetch_lanes(self):
        """(records, summary): a numpy array of METRIC_LANES_FRAME_DTYPE and a dict of the means over the frames without NaN"""
        n = self.lanes_frames()
        rec = np.zeros(n, dtype=METRIC_LANES_FRAME_DTYPE)
        s = MetricLanesSummary()
        self._ck(self._lib.vp_metric_fetch_lanes(self._h, _ptr(rec) if n else None, n, C.byref(s)))
        return rec, {"frames": s.frames, "nan_frames": s.nan_frames, "score": s.score, "loss": tuple(s.loss), "bce": tuple(s.bce), "edge": tuple(s.edge)}

    def rows_lines(self):
        return self._ck(self._lib.vp_metric_rows_lines(self._h))

    def add_rows(self, engine, target_xp, target_h, thr=None):
        """the line record of a VP_AUTOSTEER engine's last pass against host targets [rows]; thr: the run's threshold table (default: the trainer's)"""
        rows = engine.output_dims()[-2]
        tx = np.ascontiguousarray(target_xp, dtype=np.float32).reshape(-1)
        th = np.ascontiguousarray(target_h, dtype=np.float32).reshape(-1)
        if tx.size != rows or th.size != rows:
            raise ValueError("add_rows: target_xp and target_h have one value per row of the engine's output")
        t, tp, nt = _rows_table(thr)
        self._ck(self._lib.vp_metric_add_rows(self._h, engine._h, _ptr(tx), _ptr(th), tp, nt))

    def add_rows_pair(self, engine, ref, thr=None):
        """ref's own rows are the targets"""
        t, tp, nt = _rows_table(thr)
        self._ck(self._lib.vp_metric_add_rows_pair(self._h, engine._h, ref._h, tp, nt))

    def add_rows_raw(self, xp, h_vector, target_xp, target_h, thr=None):
        """the operator entry: four float32 arrays [n_lines][rows] (or [rows] for one line)"""
        a = [np.atleast_2d(np.ascontiguousarray(v, dtype=np.float32)) for v in (xp, h_vector, target_xp, target_h)]
        if a[0].ndim != 2 or any(v.shape != a[0].shape for v in a):
            raise ValueError("add_rows_raw: four arrays [n_lines][rows] of one shape")
        t, tp, nt = _rows_table(thr)
        self._ck(self._lib.vp_metric_add_rows_raw(self._h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), a[0].shape[0], a[0].shape[1], tp, nt))

    def fetch_rows(self):
        """(records, summary): a numpy array of METRIC_ROWS_LINE_DTYPE and the dict of rows_ap over all lines"""
        n = self.rows_lines()
        rec = np.zeros(n, dtype=METRIC_ROWS_LINE_DTYPE)
        s = MetricRowsSummary()
        self._ck(self._lib.vp_metric_fetch_rows(self._h, _ptr(rec) if n else None, n, C.byref(s)))
        return rec, _rows_summary_dict(s)

    def label_frames(self):
        return self._ck(self._lib.vp_metric_label_frames(self._h))

    def add_seg_label(self, engine, label, crop=None, colours=None):
        """vp_metric_add_seg_label.  label: the label file's decoded pixels, uint8 [h][w][3] (R, G, B) or [h][w] (a mask), rows possibly strided; crop: a
        PIL box (l, t, r, b) or None; colours: rows r, g, b, class (None: SCENESEG_COLOURS).  The label is copied before the call returns."""
        a, ch, h, w, stride = _label_u8(label)
        cp, keep_c = _label_crop(crop)
        tp, keep_t, nt = _label_colours(colours, ch)
        self._ck(self._lib.vp_metric_add_seg_label(self._h, engine._h, _P(a.ctypes.data), ch, h, w, stride, cp, tp, nt))

    def add_depth_label(self, engine, label):
        """vp_metric_add_depth_label.  label: the depth map as stored, float32 or float64 [h][w]"""
        a, dt, h, w, stride = _label_depth(label)
        self._ck(self._lib.vp_metric_add_depth_label(self._h, engine._h, _P(a.ctypes.data), dt, h, w, stride))

    def add_seg_logits_label(self, logits, label, crop=None, colours=None, device_chw=None):
        """vp_metric_add_seg_logits_label.  logits fp32 [c][oh][ow]: a numpy array, or (with device_chw = (c, oh, ow)) a device pointer (int)"""
        a, ch, h, w, stride = _label_u8(label)
        cp, keep_c = _label_crop(crop)
        tp, keep_t, nt = _label_colours(colours, ch)
        if device_chw is not None:
            c, oh, ow = (int(v) for v in device_chw)
            lp, dev, lg = _P(int(logits)), 1, None
        else:
            lg = np.ascontiguousarray(logits, dtype=np.float32)
            if lg.ndim != 3:
                raise ValueError("add_seg_logits_label: logits [c][oh][ow]")
            (c, oh, ow), lp, dev = lg.shape, _ptr(lg), 0
        self._ck(self._lib.vp_metric_add_seg_logits_label(self._h, lp, dev, c, oh, ow, _P(a.ctypes.data), ch, h, w, stride, cp, tp, nt))

    def add_depth_plane_label(self, pred, label, device_hw=None):
        """vp_metric_add_depth_plane_label.  pred fp32 [oh][ow]: a numpy array, or (with device_hw = (oh, ow)) a device pointer (int)"""
        a, dt, h, w, stride = _label_depth(label)
        if device_hw is not None:
            (oh, ow), pp, dev, p = (int(v) for v in device_hw), _P(int(pred)), 1, None
        else:
            p = np.ascontiguousarray(pred, dtype=np.float32)
            if p.ndim != 2:
                raise ValueError("add_depth_plane_label: a plane [oh][ow]")
            (oh, ow), pp, dev = p.shape, _ptr(p), 0
        self._ck(self._lib.vp_metric_add_depth_plane_label(self._h, pp, dev, oh, ow, _P(a.ctypes.data), dt, h, w, stride))

    def fetch_labels(self):
        """the label records in call order: a numpy array of LABEL_FRAME_DTYPE (synchronous)"""
        n = self.label_frames()
        rec = np.zeros(n, dtype=LABEL_FRAME_DTYPE)
        self._ck(self._lib.vp_metric_fetch_labels(self._h, _ptr(rec) if n else None, n))
        return rec

    def fetch(self):
        n = self.frames()
        rec = np.zeros(n, dtype=METRIC_FRAME_DTYPE)
        s = MetricSummary()
        self._ck(self._lib.vp_metric_fetch(self._h, _ptr(rec) if n else None, n, C.byref(s)))
        summary = {"frames": s.frames, "sceneseg_frames": s.sceneseg_frames, "domainseg_frames": s.domainseg_frames, "scene3d_frames": s.scene3d_frames,
                   "nan_frames": s.nan_frames, "sceneseg_iou": tuple(s.sceneseg_iou), "sceneseg_iou_full": s.sceneseg_iou_full, "domainseg_iou": s.domainseg_iou,
                   "mae": s.mae, "mel": s.mel}
        return rec, summary


class Lanes:
    """vp_lanes: the production app's LaneFilter::update on the device.  add() reads an EgoLanes Engine's device-resident logits behind its pass and
    returns without waiting; fetch() is the one synchronisation: a numpy array of LANES_RESULT_DTYPE, one record per add, oldest first -- start points,
    windows, point counts, moments, this frame's fit and the smoothed coefficients.  One thread drives a filter (include/vp_hip.h)."""

    def __init__(self, gpu_id=0, capacity=64):
        self._lib = load()
        self._h = _P()
        err = C.create_string_buffer(512)
        rc = self._lib.vp_lanes_create(C.byref(self._h), gpu_id, int(capacity), err, len(err))
        if rc != 0:
            self._h = None
            raise (ValueError if rc == -1 else VpError)(f"vp_lanes_create failed ({rc}): {err.value.decode(errors='replace')}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_lanes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_lanes_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpError)(f"libvp_hip lanes error {rc}: {msg}")
        return rc

    def set_smoothing(self, s):
        self._ck(self._lib.vp_lanes_set_smoothing(self._h, float(s)))

    def reset(self):
        self._ck(self._lib.vp_lanes_reset(self._h))

    def pending(self):
        return self._ck(self._lib.vp_lanes_pending(self._h))

    def add(self, engine, threshold=0.0):
        self._ck(self._lib.vp_lanes_add(self._h, engine._h if engine is not None else None, float(threshold)))

    def add_logits(self, logits, threshold=0.0):
        """logits: float32 [3][80][160] on the host (ego left, ego right, other lanes), copied before the call returns"""
        if logits is None:
            return self._ck(self._lib.vp_lanes_add_logits(self._h, None, float(threshold)))
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        if lg.shape != (3, 80, 160):
            raise ValueError("add_logits: logits of shape (3, 80, 160)")
        self._ck(self._lib.vp_lanes_add_logits(self._h, _ptr(lg), float(threshold)))

    def fetch(self, max_records=None):
        n = self.pending() if max_records is None else int(max_records)
        rec = np.zeros(max(n, 0), dtype=LANES_RESULT_DTYPE)
        got = C.c_int(0)
        self._ck(self._lib.vp_lanes_fetch(self._h, _ptr(rec) if n > 0 else None, n, C.byref(got)))
        return rec[:got.value]

    def fetch_points(self, record_index, lane):
        """the (x, y) points of one lane of a pending record, in collection order: uint8 [n][2]"""
        xy = np.zeros((VP_LANES_MAX_POINTS, 2), dtype=np.uint8)
        n = C.c_int(0)
        self._ck(self._lib.vp_lanes_fetch_points(self._h, int(record_index), int(lane), _ptr(xy), VP_LANES_MAX_POINTS, C.byref(n)))
        return xy[:n.value].copy()


def lanes_fit(S, T, order):
    """vp_lanes_fit: the exact least-squares line (order 1) or quadratic (order 2) from the integer moments -> ((a, b, c), singular); host only"""
    s = np.ascontiguousarray(S, dtype=np.int64).reshape(5)
    t = np.ascontiguousarray(T, dtype=np.int64).reshape(3)
    out = np.zeros(3, dtype=np.float64)
    sing = C.c_int(0)
    rc = load().vp_lanes_fit(_ptr(s), _ptr(t), int(order), _ptr(out), C.byref(sing))
    if rc != 0:
        raise ValueError(f"vp_lanes_fit failed ({rc}): order 1 or 2, moments below 2^40")
    return (tuple(float(v) for v in out), bool(sing.value))


def select_f32(values, k, gpu_id=0):
    """vp_op_select_f32: the k-th smallest (0-based) of non-negative finite float32 values, by the metric's radix select"""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    out = C.c_float()
    err = C.create_string_buffer(512)
    rc = load().vp_op_select_f32(gpu_id, _ptr(v), v.size, int(k), C.byref(out), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_select_f32 failed ({rc}): {err.value.decode(errors='replace')}")
    return np.float32(out.value)


def label_gt(label, out_hw, crop=None, colours=None, gpu_id=0):
    """vp_op_label_gt: the label kernels alone -> (ground truth uint8 [oh][ow], record: a LABEL_FRAME_DTYPE scalar).  Arguments as Metric.add_seg_label"""
    a, ch, h, w, stride = _label_u8(label)
    cp, keep_c = _label_crop(crop)
    tp, keep_t, nt = _label_colours(colours, ch)
    oh, ow = (int(v) for v in out_hw)
    gt = np.zeros((max(oh, 0), max(ow, 0)), dtype=np.uint8)
    rec = np.zeros(1, dtype=LABEL_FRAME_DTYPE)
    err = C.create_string_buffer(512)
    rc = load().vp_op_label_gt(gpu_id, _P(a.ctypes.data), ch, h, w, stride, cp, tp, nt, oh, ow, _ptr(gt), _ptr(rec), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_label_gt failed ({rc}): {err.value.decode(errors='replace')}")
    return gt, rec[0]


def label_depth_gt(label, out_hw, gpu_id=0):
    """vp_op_label_depth_gt: the depth label kernels alone -> (ground truth float32 [oh][ow], record).  label: float32 or float64 [h][w]"""
    a, dt, h, w, stride = _label_depth(label)
    oh, ow = (int(v) for v in out_hw)
    gt = np.zeros((max(oh, 0), max(ow, 0)), dtype=np.float32)
    rec = np.zeros(1, dtype=LABEL_FRAME_DTYPE)
    err = C.create_string_buffer(512)
    rc = load().vp_op_label_depth_gt(gpu_id, _P(a.ctypes.data), dt, h, w, stride, oh, ow, _ptr(gt), _ptr(rec), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_label_depth_gt failed ({rc}): {err.value.decode(errors='replace')}")
    return gt, rec[0]


def detect_validate(raw, conf=DET_CONF, iou=DET_IOU, gpu_id=0):
    """vp_op_detect_validate: the validation post-process's candidate / rank / suppression part on raw fp32 [4 + nc][nb] -> (rows [kept][6] x1, y1, x2, y2,
    score, cls; counts {candidates, ranked, kept})"""
    x = np.ascontiguousarray(raw, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] < 5:
        raise ValueError("detect_validate: a tensor [4 + nc][nb]")
    rows = np.zeros((VP_DET_MAX_DET, 6), dtype=np.float32)
    counts = np.zeros(3, dtype=np.uint32)
    err = C.create_string_buffer(512)
    rc = load().vp_op_detect_validate(gpu_id, _ptr(x), x.shape[0] - 4, x.shape[1], conf, iou, _ptr(rows), VP_DET_MAX_DET, _ptr(counts), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_detect_validate failed ({rc}): {err.value.decode(errors='replace')}")
    return rows[:int(counts[2])].copy(), {"candidates": int(counts[0]), "ranked": int(counts[1]), "kept": int(counts[2])}


def det_ap(tp, conf, det_cls, label_cls, n_iou=10):
    """vp_metric_det_ap: compute_ap on the host, no device -- tp words (bit t: correct at threshold t), conf and classes per kept row, the label classes"""
    tpw = np.ascontiguousarray(tp, dtype=np.uint32).reshape(-1)
    cf = np.ascontiguousarray(conf, dtype=np.float32).reshape(-1)
    dc = np.ascontiguousarray(det_cls, dtype=np.float32).reshape(-1)
    lc = np.ascontiguousarray(label_cls, dtype=np.float32).reshape(-1)
    if not (tpw.size == cf.size == dc.size):
        raise ValueError("det_ap: tp, conf and det_cls have one entry per kept row")
    s = MetricDetSummary()
    rc = load().vp_metric_det_ap(_ptr(tpw) if tpw.size else None, _ptr(cf) if cf.size else None, _ptr(dc) if dc.size else None, tpw.size, _ptr(lc) if lc.size else None, lc.size,
                                 int(n_iou), C.byref(s))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_metric_det_ap failed ({rc})")
    return _det_summary_dict(s)


def rows_ap(tp, conf, thr=None):
    """vp_metric_rows_ap: compute_vector_ap on the host, no device -- tp words (bit t: dist < thr[t]) and conf per line, the threshold table"""
    tpw = np.ascontiguousarray(tp, dtype=np.uint32).reshape(-1)
    cf = np.ascontiguousarray(conf, dtype=np.float32).reshape(-1)
    if tpw.size != cf.size:
        raise ValueError("rows_ap: tp and conf have one entry per line")
    t, tptr, nt = _rows_table(thr)
    s = MetricRowsSummary()
    rc = load().vp_metric_rows_ap(_ptr(tpw) if tpw.size else None, _ptr(cf) if cf.size else None, tpw.size, tptr, nt, C.byref(s))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_metric_rows_ap failed ({rc})")
    return _rows_summary_dict(s)


def decode_logits_host(logits_chw, decode_mode=VP_DECODE_SEG_MASK, gpu_id=0):
    """createMaskFromTensorHIP twin (vp_decode_logits_host): host CxHxW fp32 logits -> HxW u8 mask."""
    x = np.ascontiguousarray(logits_chw, dtype=np.float32)
    c, h, w = x.shape
    out = np.empty((h, w), dtype=np.uint8)
    rc = load().vp_decode_logits_host(gpu_id, _ptr(x), c, h, w, int(decode_mode), _ptr(out))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_decode_logits_host failed ({rc})")
    return out


def _comm_lib():
    lib = load()
    if not hasattr(lib, "vp_comm_create"):
        raise VpError("this libvp_hip.so was built without the multi-camera exchange (csrc/Makefile VP_NO_COMM=1)")
    return lib


class Comm:
    """RCCL communicator behind the C ABI (vp_comm_*): per-frame all-gather of the per-camera result records."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(VP_COMM_ID_BYTES)
        err = C.create_string_buffer(512)
        rc = _comm_lib().vp_comm_unique_id(buf, err, len(err))
        if rc != 0:
            raise VpError(f"vp_comm_unique_id failed ({rc}): {err.value.decode(errors='replace')}")
        return buf.raw

    def __init__(self, unique_id, rank, world, gpu_id, record_bytes_max):
        self._lib = _comm_lib()
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        idbuf = C.create_string_buffer(bytes(unique_id), VP_COMM_ID_BYTES)
        rc = self._lib.vp_comm_create(C.byref(self._h), idbuf, rank, world, gpu_id, record_bytes_max, err, len(err))
        if rc != 0:
            self._h = C.c_void_p()
            raise (ValueError if rc == -1 else VpError)(f"vp_comm_create failed ({rc}): {err.value.decode(errors='replace')}")
        self.rank, self.world = rank, world

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._h = None
            self._lib.vp_comm_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = self._lib.vp_comm_last_error(self._h).decode(errors="replace")
            raise (ValueError if rc == -1 else VpError)(f"libvp_hip comm error {rc}: {msg}")
        return rc

    def gather(self, engine, what=VP_GATHER_MASK):
        """Enqueue the all-gather of ``engine``'s last record on the engine's stream (no host sync)."""
        self._ck(self._lib.vp_gather(engine._h, self._h, int(what)))

    def fetch(self, engine, dtype=np.uint8):
        """[world][record] host copy of the last gather (synchronises the engine's stream)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.vp_comm_fetch(self._h, engine._h, C.byref(p), C.byref(n)))
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self.world * n.value,)).copy()
        return raw.view(dtype).reshape(self.world, -1)

    def device_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.vp_comm_device_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value


def op_conv2d(x, weight, bias, ks=3, mode=0, act=0, res=None, res_mode=0, precision=VP_FP16, tile=-1, bk=-1, nsplit=-1, gpu_id=0):
    """Single-operator entry for unit parity tests (vp_op_conv2d)."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    cin, h, w = x.shape
    cout = weight.shape[1] if mode == 1 else weight.shape[0]
    if mode == 2:  # (ConvTranspose weight [cin][cout][2][2], skip 1x1 weight [cout][cs]) and the two biases, concatenated
        cout = len(bias) // 2
    oh, ow = (2 * h, 2 * w) if mode in (1, 2) else (h, w)
    out = np.empty((cout, oh, ow), dtype=np.float32)
    r = np.ascontiguousarray(res, dtype=np.float32) if res is not None else None
    err = C.create_string_buffer(512)
    rc = lib.vp_op_conv2d(gpu_id, precision, mode, _ptr(x), cin, h, w, _ptr(weight), _ptr(bias), cout, ks, act, res_mode,
                          _ptr(r) if r is not None else None, tile, bk, nsplit, _ptr(out), err, len(err))
    if rc != 0:
        raise VpError(f"vp_op_conv2d failed ({rc}): {err.value.decode(errors='replace')}")
    return out


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def op_absmax(hi, lo, c, gpu_id=0):
    """vp_op_absmax: hi / lo float16 planes [h][w][c_pitch] (lo may be None) -> (max |hi + lo| over channels [0, c) as float32, count of non-finite elements)."""
    hi = np.ascontiguousarray(hi, dtype=np.float16)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float16)
    h, w, pitch = hi.shape
    amax, bad = C.c_float(), C.c_uint()
    err = C.create_string_buffer(512)
    rc = load().vp_op_absmax(gpu_id, _ptr(hi), None if lo is None else _ptr(lo), int(c), h, w, pitch, C.byref(amax), C.byref(bad), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_absmax failed ({rc}): {err.value.decode(errors='replace')}")
    return np.float32(amax.value), int(bad.value)


def op_exp_hist(hi, lo, c, gpu_id=0):
    """vp_op_exp_hist: hi / lo float16 planes [h][w][c_pitch] (lo may be None) -> (bins int64 [VP_RANGE_BINS], zeros, count) over channels [0, c)."""
    hi = np.ascontiguousarray(hi, dtype=np.float16)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float16)
    h, w, pitch = hi.shape
    bins = np.zeros(VP_RANGE_BINS, dtype=np.uint64)
    zeros, count = C.c_ulonglong(), C.c_ulonglong()
    err = C.create_string_buffer(512)
    rc = load().vp_op_exp_hist(gpu_id, _ptr(hi), None if lo is None else _ptr(lo), int(c), h, w, pitch, _ptr(bins), C.byref(zeros), C.byref(count), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_exp_hist failed ({rc}): {err.value.decode(errors='replace')}")
    return bins.astype(np.int64), int(zeros.value), int(count.value)


def range_summary(rec):
    """What a range_survey() record says about the fp16 exponent range: `headroom` = 15 - floor(log2 absmax), the binades left below the top one (None for
    an all-zero tensor), `below_lo_normal` = share of the non-zero finite values below 0.125 = 2^-3, where the quantum of the LOW plane (2^-11 of the
    value) is an fp16 subnormal (meaningful for two-plane engines), `below_hi_normal` = share below 2^-14, where the high plane itself is subnormal."""
    bins = np.asarray(rec["bins"], dtype=np.int64)
    nz = int(bins.sum())
    amax = float(rec["absmax"])
    share = lambda e: (float(bins[: e - VP_RANGE_EXP_MIN].sum()) / nz) if nz else 0.0
    return {"headroom": None if not amax > 0.0 else 15 - int(np.frexp(np.float32(amax))[1] - 1), "below_lo_normal": share(-3), "below_hi_normal": share(-14)}


def op_conv2d_scaled(x, weight, bias, ks=3, act=0, res=None, res_mode=0, in_exp=0, res_exp=0, out_exp=0, precision=VP_FP16X3, tile=-1, bk=-1, nsplit=-1, gpu_id=0):
    """vp_op_conv2d_scaled: op_conv2d with the input stored as x * 2^-in_exp, the residual as res * 2^-res_exp, the result as y * 2^-out_exp.
    x / res are true values; returns the STORED (hi, lo) float16 planes [cout][h][w]."""
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    cin, h, w = x.shape
    cout = weight.shape[0]
    r = _f32(res)
    hi = np.empty((cout, h, w), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    rc = load().vp_op_conv2d_scaled(gpu_id, int(precision), 0, _ptr(x), cin, h, w, _ptr(weight), _ptr(bias), cout, ks, act, res_mode, None if r is None else _ptr(r),
                                    tile, bk, nsplit, int(in_exp), int(res_exp), int(out_exp), _ptr(hi), _ptr(lo), err, len(err))
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"vp_op_conv2d_scaled failed ({rc}): {err.value.decode(errors='replace')}")
    return hi, lo


# vp_conv_form (include/vp_hip.h): its int fields in the header's order
_CONV_FORM_FIELDS = ("cin", "h", "w", "cout", "ks", "stride", "act", "post_act", "res_mode", "tile", "bk", "nsplit", "dst_c", "dst_off", "res_where", "res_off",
                     "res_h", "res_w", "in_c", "in_off", "in_exp", "res_exp", "out_exp")


def op_conv2d_forms(x, weight, bias, ks=3, stride=1, act=0, post_act=0, res_mode=0, res=None, res_off=None, dst=None, dst_off=0, in_c=0, in_off=0, in_exp=0,
                    res_exp=0, out_exp=0, precision=VP_FP16X3, tile=-1, bk=-1, nsplit=-1, gpu_id=0):
    """vp_op_conv2d_forms: Conv2d ks x ks (stride 1 or 2) + bias + act, the residual behind the activation (res_mode 1 add, 2 mul-add), then post_act,
    through the engine's own add_conv.  dst: None = a fresh output, else the destination's initial content [dst_c][oh][ow], into whose channels
    [dst_off, dst_off + cout) the launch stores through an alias view.  Residual: `res` [cout][rh][rw] = a fresh tensor (a map size other than the
    output's is refused), or res_off = channels [res_off, res_off + cout) of the destination itself.  in_c / in_off: the input as an alias view of a
    wider tensor (always refused).  Exponents: x, res and dst are true values stored as v * 2^-exp (a slice residual under out_exp); all 0 = an
    unflagged engine.  Returns the STORED (hi, lo) float16 planes of the whole destination [dst_c or cout][oh][ow]."""
    x, weight, bias, res, dst = _f32(x), _f32(weight), _f32(bias), _f32(res), _f32(dst)
    cin, h, w = x.shape
    cout = weight.shape[0]
    assert weight.shape == (cout, cin, ks, ks) and bias.shape == (cout,) and stride in (1, 2)
    oh, ow = h // stride, w // stride
    assert dst is None or dst.shape[1:] == (oh, ow)
    assert res is None or (res.ndim == 3 and res.shape[0] == cout and res_off is None)
    f = dict.fromkeys(_CONV_FORM_FIELDS, 0)
    f.update(cin=cin, h=h, w=w, cout=cout, ks=ks, stride=stride, act=act, post_act=post_act, res_mode=res_mode, tile=tile, bk=bk, nsplit=nsplit,
             dst_c=0 if dst is None else dst.shape[0], dst_off=dst_off, res_where=0 if res_off is None else 1, res_off=res_off or 0,
             res_h=0 if res is None else res.shape[1], res_w=0 if res is None else res.shape[2], in_c=in_c, in_off=in_off, in_exp=in_exp, res_exp=res_exp,
             out_exp=out_exp)
    form = np.array([int(f[k]) for k in _CONV_FORM_FIELDS], dtype=np.int32)
    hi = np.empty((cout if dst is None else dst.shape[0], oh, ow), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    _op_rc(load().vp_op_conv2d_forms(gpu_id, pr, _ptr(form), _ptr(x), _ptr(weight), _ptr(bias), None if res is None else _ptr(res),
                                     None if dst is None else _ptr(dst), _ptr(hi), _ptr(lo), err, len(err)), err, "vp_op_conv2d_forms")
    return hi, lo


def compose_upconv(wt, bt, w3, b3, ws=None, bs=None, gpu_id=0):
    """vp_compose_upconv: ConvTranspose2d(k2, s2) [+ 1x1 skip link] -> Conv3x3 multiplied out (fp64).  wt [cin][cm][2][2], w3 [cout][cm][3][3],
    ws [cm][cs] or [cm][cs][1][1].  Returns (wx [4][4][cout][cin], wsk [9][cout][cs] or None, bias [9][cout])."""
    lib = load()
    wt, bt, w3, b3, ws, bs = (_f32(v) for v in (wt, bt, w3, b3, ws, bs))
    cin, cm = wt.shape[:2]
    cout = w3.shape[0]
    cs = 0 if ws is None else ws.shape[1]
    wx = np.empty((4, 4, cout, cin), dtype=np.float64)
    wsk = np.empty((9, cout, cs), dtype=np.float64) if cs else None
    bias = np.empty((9, cout), dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = lib.vp_compose_upconv(gpu_id, _ptr(wt), _ptr(bt), _ptr(ws) if cs else None, _ptr(bs) if cs else None, _ptr(w3), _ptr(b3), cin, cm, cout, cs,
                               _ptr(wx), _ptr(wsk) if cs else None, _ptr(bias), err, len(err))
    if rc != 0:
        raise VpError(f"vp_compose_upconv failed ({rc}): {err.value.decode(errors='replace')}")
    return wx, wsk, bias


def op_upconv(x, wt, bt, w3, b3, skip=None, ws=None, bs=None, act=1, shape=-1, nsplit=0, gpu_id=0, precision="fp16x3"):
    """vp_op_upconv: one composed up-sampling stage through the engine's kernel (parity mode, or the fp16 engines' form of it): x [cin][h][w],
    skip [cs][2h][2w] -> [cout][2h][2w]."""
    lib = load()
    x, wt, bt, w3, b3, skip, ws, bs = (_f32(v) for v in (x, wt, bt, w3, b3, skip, ws, bs))
    cin, h, w = x.shape
    cm = wt.shape[1]
    cout = w3.shape[0]
    cs = 0 if skip is None else skip.shape[0]
    out = np.empty((cout, 2 * h, 2 * w), dtype=np.float32)
    err = C.create_string_buffer(512)
    rc = lib.vp_op_upconv(gpu_id, _ptr(x), cin, h, w, _ptr(skip) if cs else None, cs, _ptr(wt), _ptr(bt), _ptr(ws) if cs else None,
                          _ptr(bs) if cs else None, _ptr(w3), _ptr(b3), cm, cout, act, shape, nsplit, PRECISIONS[precision], _ptr(out), err, len(err))
    if rc != 0:
        raise VpError(f"vp_op_upconv failed ({rc}): {err.value.decode(errors='replace')}")
    return out


def _op_rc(rc, err, what):
    if rc != 0:
        raise (ValueError if rc == -1 else VpError)(f"{what} failed ({rc}): {err.value.decode(errors='replace')}")


def op_detect_head_decode(box, cls, h0, w0, precision="fp16x3", gpu_id=0, exps=None):
    """vp_op_detect_head_decode: box [64][sum h_l w_l] / cls [nc][sum h_l w_l] logits of the three levels one after the other (level l: (h0 >> l) x
    (w0 >> l), stride 8 << l) -> [4 + nc][sum h_l w_l] fp32 as AutoSpeedHead.forward gives in eval mode.  exps (vp_op_detect_head_decode_scaled): six
    exponents, (box, cls) per level -- the true-valued inputs are stored as x * 2^-exp and the kernel multiplies back."""
    box, cls = _f32(box), _f32(cls)
    nc, total = cls.shape[0], cls.shape[1]
    sizes = [(h0 >> l) * (w0 >> l) for l in range(3)]
    assert box.shape == (64, total) and sum(sizes) == total
    offs = np.cumsum([0] + sizes)
    bl = np.concatenate([box[:, offs[l]:offs[l + 1]].ravel() for l in range(3)])   # per level CHW, levels one after the other
    cl = np.concatenate([cls[:, offs[l]:offs[l + 1]].ravel() for l in range(3)])
    out = np.empty((4 + nc, total), np.float32)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    if exps is not None:
        e = np.ascontiguousarray(exps, dtype=np.int32).reshape(6)
        _op_rc(load().vp_op_detect_head_decode_scaled(gpu_id, pr, _ptr(bl), _ptr(cl), nc, h0, w0, _ptr(e), _ptr(out), err, len(err)), err,
               "vp_op_detect_head_decode_scaled")
        return out
    _op_rc(load().vp_op_detect_head_decode(gpu_id, pr, _ptr(bl), _ptr(cl), nc, h0, w0, _ptr(out), err, len(err)), err, "vp_op_detect_head_decode")
    return out


def op_upsample2_cat(a, b, precision="fp16x3", gpu_id=0):
    """vp_op_upsample2_cat: a [ca][h][w], b [cb][2h][2w] -> (hi, lo) float16 planes [ca + cb][2h][2w] of cat(nearest x2 of a, b) as the kernel stores them."""
    a, b = _f32(a), _f32(b)
    ca, h, w = a.shape
    cb = b.shape[0]
    hi = np.empty((ca + cb, 2 * h, 2 * w), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    _op_rc(load().vp_op_upsample2_cat(gpu_id, pr, _ptr(a), ca, _ptr(b), cb, h, w, _ptr(hi), _ptr(lo), err, len(err)), err, "vp_op_upsample2_cat")
    return hi, lo


def op_upsample2_cat_scaled(a, b, a_off=0, a_nch=None, b_off=0, b_nch=None, exp=0, precision="fp16x3", gpu_id=0):
    """vp_op_upsample2_cat_scaled: channels [a_off, a_off + a_nch) of a [ca][h][w] and [b_off, b_off + b_nch) of b [cb][2h][2w], true values stored as
    x * 2^-exp in a flagged engine that ties a, b and the result -> the STORED (hi, lo) float16 planes [a_nch + b_nch][2h][2w]."""
    a, b = _f32(a), _f32(b)
    ca, h, w = a.shape
    cb = b.shape[0]
    a_nch = ca - a_off if a_nch is None else int(a_nch)
    b_nch = cb - b_off if b_nch is None else int(b_nch)
    hi = np.empty((a_nch + b_nch, 2 * h, 2 * w), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    _op_rc(load().vp_op_upsample2_cat_scaled(gpu_id, pr, _ptr(a), ca, int(a_off), a_nch, _ptr(b), cb, int(b_off), b_nch, h, w, int(exp), _ptr(hi), _ptr(lo), err,
                                             len(err)), err, "vp_op_upsample2_cat_scaled")
    return hi, lo


def op_dwconv3x3(x, weight, bias, act=0, add=None, precision="fp16x3", gpu_id=0):
    """vp_op_dwconv3x3: depthwise 3x3 (pad 1) + bias + activation (0 none, 2 SiLU) [+ add] -> (hi, lo) float16 planes [c][h][w]."""
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    c, h, w = x.shape
    add = None if add is None else _f32(add)
    hi = np.empty((c, h, w), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    _op_rc(load().vp_op_dwconv3x3(gpu_id, pr, _ptr(x), c, h, w, _ptr(weight), _ptr(bias), int(act), None if add is None else _ptr(add), _ptr(hi), _ptr(lo), err,
                                  len(err)), err, "vp_op_dwconv3x3")
    return hi, lo


def op_rowpair_conv(x, weight, bias, replicate=False, dst=None, dst_off=0, precision="fp16x3", gpu_id=0, in_exp=None, out_exp=None):
    """vp_op_rowpair_conv: Conv2d(cin -> 32, kernel (2,1), stride (2,1)) + bias + SiLU of x [cin][h][w] (weight [32][cin][2][1]); with `replicate` every
    result pixel is stored 2 x 2.  dst: the destination's initial content [dst_c][h'][w'] (None: 32 channels of zeros); the result lands in its channels
    [dst_off, dst_off + 32).  Returns the whole destination as (hi, lo) float16 planes.  in_exp / out_exp (vp_op_rowpair_conv_scaled): x and dst are
    true values stored as x * 2^-in_exp / dst * 2^-out_exp, the planes returned are the STORED ones (true value = (hi + lo) * 2^out_exp)."""
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    cin, h, w = x.shape
    assert weight.shape == (32, cin, 2, 1) and bias.shape == (32,)
    f = 2 if replicate else 1
    ho, wo = (h // 2) * f, w * f
    dst = None if dst is None else _f32(dst)
    dst_c = 32 if dst is None else dst.shape[0]
    assert dst is None or dst.shape == (dst_c, ho, wo)
    hi = np.empty((dst_c, ho, wo), np.float16)
    lo = np.empty_like(hi)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    if in_exp is not None or out_exp is not None:
        _op_rc(load().vp_op_rowpair_conv_scaled(gpu_id, pr, _ptr(x), cin, h, w, _ptr(weight), _ptr(bias), int(bool(replicate)), dst_c, int(dst_off),
                                                None if dst is None else _ptr(dst), int(in_exp or 0), int(out_exp or 0), _ptr(hi), _ptr(lo), err, len(err)),
               err, "vp_op_rowpair_conv_scaled")
        return hi, lo
    _op_rc(load().vp_op_rowpair_conv(gpu_id, pr, _ptr(x), cin, h, w, _ptr(weight), _ptr(bias), int(bool(replicate)), dst_c, int(dst_off),
                                     None if dst is None else _ptr(dst), _ptr(hi), _ptr(lo), err, len(err)), err, "vp_op_rowpair_conv")
    return hi, lo


def op_lane_rows_head(features, c1_w, c1_b, c2_w, c2_b, h1_w, h1_b, h2_w, h2_b, precision="fp16x3", gpu_id=0, in_exp=None):
    """vp_op_lane_rows_head: features [cin][h][256] -> [2][h] fp32 (xp, h_vector) as AutoSteerPerceptHead.forward gives behind `features`; c1 / c2 are the
    3x3 convolutions [cin][3][3] with their BatchNorm folded in, h1 / h2 the 16-tap row convolutions.  in_exp (vp_op_lane_rows_head_scaled): the
    true-valued features are stored as x * 2^-in_exp and the kernel multiplies back."""
    features, c1_w, c2_w, h1_w, h2_w = _f32(features), _f32(c1_w).reshape(-1), _f32(c2_w).reshape(-1), _f32(h1_w).reshape(-1), _f32(h2_w).reshape(-1)
    cin, h, w = features.shape
    assert c1_w.size == cin * 9 and c2_w.size == cin * 9 and h1_w.size == 16 and h2_w.size == 16
    out = np.empty((2, h), np.float32)
    err = C.create_string_buffer(512)
    pr = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    if in_exp is not None:
        _op_rc(load().vp_op_lane_rows_head_scaled(gpu_id, pr, _ptr(features), cin, h, w, _ptr(c1_w), float(c1_b), _ptr(c2_w), float(c2_b), _ptr(h1_w),
                                                  float(h1_b), _ptr(h2_w), float(h2_b), int(in_exp), _ptr(out), err, len(err)), err,
               "vp_op_lane_rows_head_scaled")
        return out
    _op_rc(load().vp_op_lane_rows_head(gpu_id, pr, _ptr(features), cin, h, w, _ptr(c1_w), float(c1_b), _ptr(c2_w), float(c2_b), _ptr(h1_w), float(h1_b),
                                       _ptr(h2_w), float(h2_b), _ptr(out), err, len(err)), err, "vp_op_lane_rows_head")
    return out


def autosteer_angle(logits):
    """vp_autosteer_angle: AutoSteerOnnxEngine::postProcess -- first arg-max over the head's logits (61 classes) minus 30 degrees (host only)."""
    a = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    return float(load().vp_autosteer_angle(_ptr(a), int(a.size)))


def resample_coeffs(in_size, out_size, mode):
    """vp_resample_coeffs: (bounds [out][2], coefficients [out][ksize]) of a VP_RESIZE_PIL_* mode for one axis (host only)."""
    cap = out_size * (2 * int(np.ceil(2.0 * max(1.0, in_size / out_size))) + 1)
    b = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros(cap, dtype=np.int32)
    ks = load().vp_resample_coeffs(in_size, out_size, mode, _ptr(b), _ptr(k), cap)
    if ks <= 0:
        raise VpError(f"vp_resample_coeffs failed ({ks})")
    return b, k[: out_size * ks].reshape(out_size, ks)


class Detector:
    """AutoSpeed detector pre / post-processing on the device (vp_detect_*): the Python twin of AutoSpeedOnnxEngine's preprocessAutoSpeed and
    postProcess (VisionPilot/middleware_recipes/common/backends/autospeed/onnxruntime_engine.cpp:71-113, :170-290).  The detector network
    is either the caller's -- `preprocess(frame)` -> its input tensor, `postprocess(raw, conf, iou)` -> the kept detections -- or an
    Engine("autospeed", ...) of this library: `attach(engine)` once, then `infer(frame, conf, iou)` per frame (vp_detect_infer: nothing leaves the device).
    The network's input is 512 x 1024 with 10752 boxes: Detector(512, 1024, max_boxes=10752, max_attrs=4 + classes)."""

    def __init__(self, net_h=640, net_w=640, max_boxes=8400, max_attrs=84, gpu_id=0):
        self._lib = load()
        self._h = _P()
        self.net_h, self.net_w = net_h, net_w
        err = C.create_string_buffer(512)
        rc = self._lib.vp_detect_create(C.byref(self._h), gpu_id, net_h, net_w, max_boxes, max_attrs, err, len(err))
        if rc != 0:
            self._h = None
            raise VpError(f"vp_detect_create failed ({rc}): {err.value.decode(errors='replace')}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_detect_destroy(self._h)
            self._h = None
        self._net = None

    def attach(self, engine):
        """vp_detect_attach: borrow an Engine("autospeed", ...) as this detector's network (None detaches); ValueError if it does not fit."""
        rc = self._lib.vp_detect_attach(self._h, None if engine is None else engine._h)
        if rc == -1:
            raise ValueError(f"vp_detect_attach failed ({rc}): {self._lib.vp_detect_last_error(self._h).decode(errors='replace')}")
        self._check(rc, "vp_detect_attach")
        self._net = engine   # keeps the engine alive while it is attached

    def infer(self, frame_bgr_u8, conf_thresh, iou_thresh, cap=None):
        """vp_detect_infer: HxWx3 BGR uint8 frame -> ([n][6] float32 rows x1, y1, x2, y2, confidence, class_id; total kept) through the attached network."""
        f = self._frame(frame_bgr_u8)
        return self._rows("vp_detect_infer", (_ptr(f), f.shape[0], f.shape[1], f.strides[0]), conf_thresh, iou_thresh, 1024 if cap is None else cap, True, True)

    def infer_frame(self, frame, conf_thresh, iou_thresh, region=None, cap=None):
        """vp_detect_infer_frame: infer() on a region (x0, y0, w, h; None = the whole frame) of a device-resident Frame."""
        x0, y0, w, h = (0, 0, 0, 0) if region is None else (int(v) for v in region)
        return self._rows("vp_detect_infer_frame", (frame._h, x0, y0, w, h), conf_thresh, iou_thresh, 1024 if cap is None else cap, True, True)

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise VpError(f"{what} failed ({rc}): {self._lib.vp_detect_last_error(self._h).decode(errors='replace')}")

    @staticmethod
    def _frame(frame_u8):
        f = np.asarray(frame_u8)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.strides[2] != 1 or f.strides[1] != 3:
            f = np.ascontiguousarray(f, dtype=np.uint8)
        return f

    def _rows(self, entry, head, conf_thresh, iou_thresh, cap, int_class, range_error=False):
        """allocate `cap` rows, call `entry`(handle, *head, conf, iou, rows, cap, &count), slice: ([min(count, cap)][6] float32, count).  `int_class`: the
        entry writes vp_detection records, whose class_id is an int."""
        out = np.zeros((max(cap, 1), 6), np.float32)
        n = C.c_int()
        rc = getattr(self._lib, entry)(self._h, *head, float(conf_thresh), float(iou_thresh), _ptr(out), cap, C.byref(n))
        if range_error and rc == -5:
            raise VpRangeError(f"{entry} failed ({rc}): {self._lib.vp_detect_last_error(self._h).decode(errors='replace')}")
        self._check(rc, entry)
        rows = out[:min(n.value, cap)].copy()
        if int_class:
            rows[:, 5] = rows[:, 5].view(np.int32).astype(np.float32)
        return rows, n.value

    def preprocess(self, frame_bgr_u8):
        """HxWx3 BGR uint8 -> ([3][net_h][net_w] float32 planes R, G, B in [0, 1], (scale, pad_x, pad_y))."""
        f = self._frame(frame_bgr_u8)
        out = np.empty((3, self.net_h, self.net_w), np.float32)
        self._check(self._lib.vp_detect_preprocess(self._h, _ptr(f), f.shape[0], f.shape[1], f.strides[0], _ptr(out)), "vp_detect_preprocess")
        return out, self.letterbox()

    def letterbox(self):
        s, px, py = C.c_float(), C.c_int(), C.c_int()
        self._check(self._lib.vp_detect_letterbox(self._h, C.byref(s), C.byref(px), C.byref(py)), "vp_detect_letterbox")
        return np.float32(s.value), px.value, py.value

    def set_letterbox(self, scale, pad_x, pad_y, orig_w, orig_h):
        self._check(self._lib.vp_detect_set_letterbox(self._h, float(scale), pad_x, pad_y, orig_w, orig_h), "vp_detect_set_letterbox")

    def postprocess(self, raw, conf_thresh, iou_thresh, cap=None):
        """raw [num_attrs][num_boxes] float32 -> ([n][6] float32 rows x1, y1, x2, y2, confidence, class_id; total kept)."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        return self._rows("vp_detect_postprocess", (_ptr(raw), 0, raw.shape[0], raw.shape[1]), conf_thresh, iou_thresh, raw.shape[1] if cap is None else cap, True)

    # ---- the Python wrapper's arithmetic (Models/inference/auto_speed_infer.py; vp_hip.h vp_detect_*_pil / _agnostic)
    def preprocess_pil(self, frame_u8, pixel_format=VP_RGB8):
        """vp_detect_preprocess_pil: HxWx3 uint8 frame (RGB as a PIL image gives it, or VP_BGR8) -> ([3][net_h][net_w] float32 planes R, G, B, (scale, pad_x, pad_y)),
        Pillow's BILINEAR letterbox + ToTensor bit for bit."""
        f = self._frame(frame_u8)
        out = np.empty((3, self.net_h, self.net_w), np.float32)
        self._check(self._lib.vp_detect_preprocess_pil(self._h, _ptr(f), f.shape[0], f.shape[1], f.strides[0], int(pixel_format), _ptr(out)), "vp_detect_preprocess_pil")
        return out, self.letterbox()

    def postprocess_agnostic(self, raw, conf_thresh, iou_thresh, cap=None):
        """vp_detect_postprocess_agnostic: raw [num_attrs][num_boxes] float32 -> ([n][6] float32 rows x1, y1, x2, y2, score, class; total kept)."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        return self._rows("vp_detect_postprocess_agnostic", (_ptr(raw), 0, raw.shape[0], raw.shape[1]), conf_thresh, iou_thresh, raw.shape[1] if cap is None else cap, False)

    def infer_pil(self, frame_u8, conf_thresh, iou_thresh, cap=None, pixel_format=VP_RGB8):
        """vp_detect_infer_pil: frame -> ([n][6] float32 rows x1, y1, x2, y2, score, class; total kept) through the attached network."""
        f = self._frame(frame_u8)
        return self._rows("vp_detect_infer_pil", (_ptr(f), f.shape[0], f.shape[1], f.strides[0], int(pixel_format)), conf_thresh, iou_thresh, 1024 if cap is None else cap,
                          False, True)


def detect_geometry_pil(net_h, net_w, h, w):
    """vp_detect_geometry_pil: (scale, new_w, new_h, pad_x, pad_y) of the Python wrapper's resize_letterbox for an h x w frame (host only)."""
    s = C.c_double()
    v = [C.c_int() for _ in range(4)]
    rc = load().vp_detect_geometry_pil(net_h, net_w, h, w, C.byref(s), *[C.byref(x) for x in v])
    if rc != 0:
        raise ValueError(f"vp_detect_geometry_pil: a {h} x {w} frame has no letterbox in {net_h} x {net_w}")
    return (s.value,) + tuple(x.value for x in v)
