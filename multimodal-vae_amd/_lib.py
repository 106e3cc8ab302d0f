"""ctypes binding of libmmvae_hip.so (include/mmvae_hip.h).  No CPU fallback: if the library is missing or
no gfx950 device is usable, calls raise."""
import contextlib
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmvae_hip.so")


class MMVAEError(RuntimeError):
    pass


class StepIO(C.Structure):
    """mmvae_mm_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("text", C.c_void_p), ("eps", C.c_void_p),
        ("enc_mask1", C.c_void_p), ("enc_mask2", C.c_void_p), ("gru_keep", C.c_void_p),
        ("enc_dropout", C.c_int), ("gru_dropout", C.c_int),
        ("force_tokens", C.c_void_p),
        ("kl_lambda", C.c_float),
        ("lambda_xy", C.c_float * 3), ("lambda_yx", C.c_float * 3),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p), ("recon_text", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p), ("tokens", C.c_void_p),
        ("pass_skip", C.c_int * 3),
        ("defer_unpack", C.c_int),
        ("pack_first", C.c_int),
        ("dp_split", C.c_int),
        ("early_adam", C.c_void_p),
    ]


class EarlyAdam(C.Structure):
    """struct mmvae_early_adam"""
    _fields_ = [
        ("m", C.c_void_p), ("v", C.c_void_p), ("state", C.c_void_p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("grad_scale", C.c_float),
        ("gmap", C.c_void_p), ("ran", C.POINTER(C.c_int)),
    ]


class MnistStepIO(C.Structure):
    """mmvae_mnist_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("label", C.c_void_p), ("eps", C.c_void_p),
        ("lambda_xy", C.c_float * 3), ("lambda_yx", C.c_float * 3),
        ("kl_coef", C.c_float),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p), ("recon_text", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p),
        ("pass_skip", C.c_int * 3),
    ]


class CocoStepIO(C.Structure):
    """mmvae_coco_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("text", C.c_void_p), ("sos", C.c_void_p), ("eps", C.c_void_p),
        ("enc_mask1", C.c_void_p), ("enc_mask2", C.c_void_p), ("gru_keep", C.c_void_p),
        ("enc_dropout", C.c_int), ("gru_dropout", C.c_int),
        ("kl_lambda", C.c_float),
        ("lambda_xy", C.c_float * 3), ("lambda_yx", C.c_float * 3),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p), ("recon_text", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p),
        ("pass_skip", C.c_int * 3),
        ("defer_unpack", C.c_int),
        ("pack_first", C.c_int),
        ("optimizer_state", C.c_void_p),
    ]


class CelebaStepIO(C.Structure):
    """mmvae_celeba_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("attrs", C.c_void_p), ("eps", C.c_void_p),
        ("enc_mask", C.c_void_p), ("enc_dropout", C.c_int),
        ("kl_lambda", C.c_float),
        ("lambda_x", C.c_float * 3), ("lambda_y", C.c_float * 3),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p), ("recon_attrs", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p),
        ("pass_skip", C.c_int * 3),
        ("defer_unpack", C.c_int),
    ]


class ImageStepIO(C.Structure):
    """mmvae_image_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("eps", C.c_void_p),
        ("enc_mask1", C.c_void_p), ("enc_mask2", C.c_void_p),
        ("enc_dropout", C.c_int),
        ("kl_lambda", C.c_float), ("lambda_x", C.c_float),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p),
        ("defer_unpack", C.c_int),
    ]


class InfoVAEStepIO(C.Structure):
    """mmvae_infovae_step_io"""
    _fields_ = ImageStepIO._fields_ + [
        ("true_samples", C.c_void_p),
        ("lambda_mmd", C.c_float),
        ("z", C.c_void_p),
    ]


class MnistInfoVAEStepIO(C.Structure):
    """mmvae_mnist_infovae_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("image", C.c_void_p), ("true_samples", C.c_void_p),
        ("lambda_x", C.c_float), ("lambda_mmd", C.c_float),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_image", C.c_void_p), ("z", C.c_void_p),
    ]


class TextStepIO(C.Structure):
    """mmvae_text_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("text", C.c_void_p), ("sos", C.c_void_p), ("eps", C.c_void_p), ("gru_keep", C.c_void_p),
        ("gru_dropout", C.c_int),
        ("kl_lambda", C.c_float), ("lambda_y", C.c_float),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_text", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p),
        ("defer_unpack", C.c_int), ("pack_first", C.c_int),
        ("optimizer_state", C.c_void_p),
    ]


class MMTextStepIO(C.Structure):
    """mmvae_mm_text_step_io"""
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("step_counter", C.c_void_p),
        ("text", C.c_void_p), ("eps", C.c_void_p), ("gru_keep", C.c_void_p),
        ("gru_dropout", C.c_int),
        ("force_tokens", C.c_void_p),
        ("kl_lambda", C.c_float), ("lambda_y", C.c_float),
        ("seed", C.c_ulonglong),
        ("sums", C.c_void_p), ("recon_text", C.c_void_p),
        ("mu", C.c_void_p), ("logvar", C.c_void_p), ("tokens", C.c_void_p),
        ("defer_unpack", C.c_int), ("pack_first", C.c_int),
    ]


_P, _I, _F, _LL, _SZ, _ULL, _U = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t, C.c_ulonglong, C.c_uint

# name -> (restype, argtypes); restype int means "status code, raise on != 0"
SIGNATURES = {
    "mmvae_init": (_I, [_I]),
    "mmvae_last_error": (C.c_char_p, []),
    "mmvae_version": (C.c_char_p, []),
    "mmvae_set_stream_policy": (_I, [_I]),
    "mmvae_comm_unique_id": (_I, [_P]),
    "mmvae_comm_init": (_I, [C.POINTER(C.c_void_p), _I, _I, _P]),
    "mmvae_allreduce_grads": (_I, [_P, _P, C.c_size_t, _P]),
    "mmvae_comm_world": (_I, [_P]),
    "mmvae_comm_destroy": (_I, [_P]),
    "mmvae_mm_step": (_I, [_P, C.POINTER(StepIO), _I, _I, _P]),
    "mmvae_mm_wait_early_grads": (_I, [_P, _P]),
    "mmvae_mm_image_encoder_fwd": (_I, [_P, _P, _SZ, _P, _P, _P, _I, _P, _P]),
    "mmvae_mm_image_encoder_bwd": (_I, [_P, _P, _SZ, _P, _P, _P, _P]),
    "mmvae_mm_image_decoder_fwd": (_I, [_P, _P, _SZ, _P, _I, _P, _P]),
    "mmvae_mm_iw_workspace_bytes": (_SZ, [_P]),
    "mmvae_mm_iw_score": (_I, [_P, _P, _SZ, _P, _P, _I, _I, _P, _P, _P]),
    "mmvae_mm_image_decoder_bwd": (_I, [_P, _P, _SZ, _P, _P, _P, _P]),
    "mmvae_mm_text_encoder_fwd": (_I, [_P, _P, _SZ, _P, _P, _P]),
    "mmvae_mm_text_encoder_bwd": (_I, [_P, _P, _SZ, _P, _P, _P]),
    "mmvae_mm_text_decoder_fwd": (_I, [_P, _P, _SZ, _P, _I, _P, _P, _P, _P, _P]),
    "mmvae_mm_text_decoder_bwd": (_I, [_P, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mmvae_mm_bench_layer": (_I, [_P, _P, _SZ, C.c_char_p, _I, _P]),
    "mmvae_mm_layer_flops": (C.c_double, [_P, C.c_char_p]),
    "mmvae_mm_layer_algo_flops": (C.c_double, [_P, C.c_char_p]),
    "mmvae_mm_layer_algo_bytes": (C.c_double, [_P, C.c_char_p]),
    "mmvae_debug_flops": (C.c_double, [_I]),
    "mmvae_debug_set": (_I, [C.c_char_p, _I]),
    "mmvae_debug_get": (_I, [C.c_char_p, C.POINTER(_I), C.POINTER(_I)]),
    "mmvae_debug_reset": (_I, [C.c_char_p]),
    "mmvae_debug_knob_name": (C.c_char_p, [_I]),
    "mmvae_mm_debug_offset": (_LL, [_P, C.c_char_p]),
    "mmvae_poe_fwd": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "mmvae_poe_bwd": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mmvae_reparam_fwd": (_I, [_P, _P, _P, _I, _P, _P]),
    "mmvae_reparam_bwd": (_I, [_P, _P, _P, _I, _P, _P, _P]),
    "mmvae_kl_fwd": (_I, [_P, _P, _I, _P, _P]),
    "mmvae_kl_bwd": (_I, [_P, _P, _I, _F, _P, _P, _P, _P]),
    "mmvae_bce_fwd": (_I, [_P, _P, _LL, _P, _P]),
    "mmvae_bce_bwd": (_I, [_P, _P, _LL, _F, _P, _P, _P]),
    "mmvae_nll_fwd": (_I, [_P, _P, _I, _I, _P, _P]),
    "mmvae_nll_bwd": (_I, [_P, _I, _I, _F, _P, _P, _P]),
    "mmvae_iw_particles": (_I, [_P, _P, _I, _I, _I, _LL, _LL, _ULL, _P, _P, _P, _P]),
    "mmvae_iw_init": (_I, [_P, _I, _P]),
    "mmvae_iw_accumulate": (_I, [_P, _P, _P, _I, _I, _P, _I, _I, _P, _P, _P]),
    "mmvae_iw_finalize": (_I, [_P, _I, _LL, _P, _P]),
    "mmvae_normal": (_I, [_P, _LL, _ULL, _P, _U, _P]),
    "mmvae_keep_mask": (_I, [_P, _LL, _F, _ULL, _P, _U, _P]),
    "mmvae_mse_fwd": (_I, [_P, _P, _LL, _P, _P]),
    "mmvae_mse_bwd": (_I, [_P, _P, _LL, _F, _P, _P, _P]),
    "mmvae_u8_to_f32": (_I, [_P, _LL, _F, _P, _P]),
    "mmvae_u8_to_f32_after": (_I, [_P, _LL, _F, _P, _P, _P]),
    "mmvae_h2d_stage": (_I, [_P, _P, _SZ, _P, _P, _SZ, _P, _P]),
    "mmvae_gather_rows_u8_f32": (_I, [_P, _P, _LL, _LL, _F, _P, _P]),
    "mmvae_stream_wait_event": (_I, [_P, _P]),
    "mmvae_event_create": (_I, [C.POINTER(C.c_void_p)]),
    "mmvae_event_destroy": (_I, [_P]),
    "mmvae_event_record": (_I, [_P, _P]),
    "mmvae_event_synchronize": (_I, [_P]),
    "mmvae_stream_create": (_I, [_P]),
    "mmvae_stream_destroy": (_I, [_P]),
    "mmvae_gather_rows": (_I, [_P, _P, _LL, _LL, _P, _P]),
    "mmvae_step_status": (_I, [_P, _P]),
    "mmvae_step_losses": (_I, [_P, _P, _P, _P, _P, _P]),
    "mmvae_debug_probe": (_I, [_I]),
    "mmvae_debug_probe_read": (_I, [_P, _LL]),
    "mmvae_adam_step": (_I, [_P, _P, _P, _P, _LL, _P, _F, _F, _F, _F, _F, _P]),
    "mmvae_adam_step_packed": (_I, [_P, _P, _P, _P, _LL, _P, _F, _F, _F, _F, _F, _P, _P, _P, _P]),
    "mmvae_adam_step_packed_ranges": (_I, [_P, _P, _P, _P, _LL, C.POINTER(_LL), _I, _I, _P, _F, _F, _F, _F, _F, _P, _P, _P, _P]),
    "mmvae_mm_early_ranges": (_I, [_P, C.POINTER(_LL), _I]),
}


def _plan_api(pfx):
    """The plan/query/bind/pack entry points every model family exports under its own prefix."""
    return {
        "mmvae_%s_create" % pfx: (_P, [_I, _I]),
        "mmvae_%s_destroy" % pfx: (None, [_P]),
        "mmvae_%s_param_count" % pfx: (_LL, [_P]),
        "mmvae_%s_num_params" % pfx: (_I, [_P]),
        "mmvae_%s_param_info" % pfx: (_I, [_P, _I, C.c_char_p, C.POINTER(_I), C.POINTER(_I), C.POINTER(_LL)]),
        "mmvae_%s_bn_floats" % pfx: (_LL, [_P]),
        "mmvae_%s_num_bn" % pfx: (_I, [_P]),
        "mmvae_%s_bn_info" % pfx: (_I, [_P, _I, C.c_char_p, C.POINTER(_I), C.POINTER(_LL)]),
        "mmvae_%s_packed_elems" % pfx: (_LL, [_P]),
        "mmvae_%s_packed_vec_elems" % pfx: (_LL, [_P]),
        "mmvae_%s_gpk_elems" % pfx: (_LL, [_P]),
        "mmvae_%s_gpk_vec_elems" % pfx: (_LL, [_P]),
        "mmvae_%s_desc_bytes" % pfx: (_SZ, [_P, _I]),
        "mmvae_%s_desc_copy" % pfx: (_I, [_P, _I, _P]),
        "mmvae_%s_workspace_bytes" % pfx: (_SZ, [_P]),
        "mmvae_%s_module_workspace_bytes" % pfx: (_SZ, [_P]),
        "mmvae_%s_bind" % pfx: (_I, [_P] * 11),
        "mmvae_%s_pack_weights" % pfx: (_I, [_P, _P]),
        "mmvae_%s_grad_map" % pfx: (_I, [_P, _P, _P]),
        "mmvae_%s_debug_pack_as_grads" % pfx: (_I, [_P, _P, _P, _P, _P]),
    }


SIGNATURES.update(_plan_api("mm"))
SIGNATURES.update(_plan_api("mnist"))
SIGNATURES["mmvae_mnist_create_p"] = (_P, [_I, _I, _I])
SIGNATURES["mmvae_mnist_precision"] = (_I, [_P])
SIGNATURES["mmvae_mnist_step"] = (_I, [_P, C.POINTER(MnistStepIO), _I, _I, _P])
for _m in ("image_encoder", "image_decoder", "text_encoder", "text_decoder"):
    SIGNATURES["mmvae_mnist_%s_fwd" % _m] = (_I, [_P, _P, _SZ, _P, _I, _P, _P])
SIGNATURES["mmvae_mnist_image_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P])
SIGNATURES["mmvae_mnist_image_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_mnist_text_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_mnist_text_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_mnist_iw_score"] = (_I, [_P, _P, _P, _I, _I, _P, _P, _P])
SIGNATURES.update(_plan_api("celeba"))
SIGNATURES["mmvae_celeba_step"] = (_I, [_P, C.POINTER(CelebaStepIO), _I, _I, _P])
SIGNATURES["mmvae_celeba_bench_layer"] = (_I, [_P, _P, _SZ, C.c_char_p, _I, _P])
SIGNATURES["mmvae_celeba_debug_offset"] = (_LL, [_P, C.c_char_p])
SIGNATURES["mmvae_celeba_image_encoder_fwd"] = (_I, [_P, _P, _SZ, _P, _P, _I, _P, _P])
SIGNATURES["mmvae_celeba_image_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_celeba_image_decoder_fwd"] = (_I, [_P, _P, _SZ, _P, _I, _P, _P])
SIGNATURES["mmvae_celeba_image_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_celeba_attrs_encoder_fwd"] = (_I, [_P, _P, _SZ, _P, _I, _P, _P])
SIGNATURES["mmvae_celeba_attrs_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P])
SIGNATURES["mmvae_celeba_attrs_decoder_fwd"] = (_I, [_P, _P, _SZ, _P, _I, _P, _P])
SIGNATURES["mmvae_celeba_attrs_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_celeba_iw_workspace_bytes"] = (_SZ, [_P])
SIGNATURES["mmvae_celeba_iw_score"] = (_I, [_P, _P, _SZ, _P, _P, _I, _I, _P, _P, _P])
SIGNATURES["mmvae_celeba_iw_tail"] = (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _P, _P])
SIGNATURES["mmvae_celeba_iw_attrs"] = (_I, [_P, _P, _LL, _P, _P])
SIGNATURES.update(_plan_api("coco"))
SIGNATURES["mmvae_coco_create_t"] = (_P, [_I, _I, _I])
SIGNATURES["mmvae_coco_steps"] = (_I, [_P])
SIGNATURES["mmvae_coco_step"] = (_I, [_P, C.POINTER(CocoStepIO), _I, _I, _P])
SIGNATURES["mmvae_coco_image_encoder_fwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _I, _P, _P])
SIGNATURES["mmvae_coco_image_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_coco_image_decoder_fwd"] = (_I, [_P, _P, _SZ, _P, _I, _P, _P])
SIGNATURES["mmvae_coco_image_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P])
SIGNATURES["mmvae_coco_text_encoder_fwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_coco_text_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_coco_text_decoder_fwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _I, _P, _P])
SIGNATURES["mmvae_coco_text_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P, _P, _P, _P])
SIGNATURES["mmvae_coco_bench_layer"] = (_I, [_P, _P, _SZ, C.c_char_p, _I, _P])
SIGNATURES["mmvae_coco_debug_offset"] = (_LL, [_P, C.c_char_p])
SIGNATURES["mmvae_coco_iw_workspace_bytes"] = (_SZ, [_P])
SIGNATURES["mmvae_coco_iw_score"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P, _I, _I, _P, _P, _P])
SIGNATURES["mmvae_coco_iw_tail"] = (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _P, _P])
SIGNATURES["mmvae_coco_iw_text_sse"] = (_I, [_P, _P, _I, _I, _I, _P, _P])
for _f in ("celeba", "coco", "mm", "mnist"):
    SIGNATURES["mmvae_%s_image_step" % _f] = (_I, [_P, C.POINTER(ImageStepIO), _I, _I, _P])
    SIGNATURES["mmvae_%s_image_step_workspace_bytes" % _f] = (_SZ, [_P])
    SIGNATURES["mmvae_%s_iw_score_image" % _f] = (_I, [_P, _P, _SZ, _P, _P, _I, _I, _P, _P])
SIGNATURES["mmvae_coco_infovae_step"] = (_I, [_P, C.POINTER(InfoVAEStepIO), _I, _I, _P])
SIGNATURES["mmvae_coco_infovae_step_workspace_bytes"] = (_SZ, [_P])
SIGNATURES["mmvae_mnist_strip_max_rows"] = (_I, [])
SIGNATURES["mmvae_mnist_strip_route"] = (_I, [_I])
SIGNATURES["mmvae_mnist_lin_bn_act_fwd"] = (_I, [_I, _P, _I] + [_P] * 7 + [_I] * 4 + [_P] * 4)
SIGNATURES["mmvae_mnist_lin_dgrad_bn_bwd"] = (_I, [_I, _P, _I] + [_P] * 5 + [_I, _I] + [_P] * 4)
SIGNATURES["mmvae_coco_text_step"] = (_I, [_P, C.POINTER(TextStepIO), _I, _I, _P])
SIGNATURES["mmvae_coco_text_step_workspace_bytes"] = (_SZ, [_P])
SIGNATURES["mmvae_coco_iw_score_text"] = (_I, [_P, _P, _SZ, _P, _P, _P, _I, _I, _P, _P])
SIGNATURES.update(_plan_api("mmtext"))
SIGNATURES["mmvae_mmtext_create"] = (_P, [_I, _I, _I])
SIGNATURES["mmvae_mmtext_hidden"] = (_I, [_P])
SIGNATURES["mmvae_mmtext_step"] = (_I, [_P, C.POINTER(MMTextStepIO), _I, _I, _P])
SIGNATURES["mmvae_mmtext_encoder_fwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_mmtext_encoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P])
SIGNATURES["mmvae_mmtext_decoder_fwd"] = (_I, [_P, _P, _SZ, _P, _I, _P, _P, _P, _P, _P])
SIGNATURES["mmvae_mmtext_decoder_bwd"] = (_I, [_P, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P])
SIGNATURES["mmvae_mmtext_iw_score"] = (_I, [_P, _P, _SZ, _P, _I, _I, _P, _P])
SIGNATURES["mmvae_latent1_bwd_f32"] = (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _P, _I, _P])
SIGNATURES["mmvae_latent1_scratch_floats"] = (_SZ, [_I, _I])
SIGNATURES["mmvae_latent1_fwd"] = (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P])
SIGNATURES["mmvae_latent1_bwd"] = (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P])
SIGNATURES["mmvae_latent3_fwd"] = (_I, [_P] * 4 + [_I] * 3 + [_P] * 4 + [_I, _P, _P])
SIGNATURES["mmvae_latent3_bwd"] = (_I, [_P] * 8 + [_I] * 3 + [_F] * 3 + [_P, _I, _I] + [_P] * 8)
SIGNATURES["mmvae_sigmoid_bce"] = (_I, [_P, _I, _P] + [_I] * 5 + [C.POINTER(_F)] + [_P] * 4)
SIGNATURES["mmvae_logsoftmax_nll"] = (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _P, C.POINTER(_F), _P])
SIGNATURES["mmvae_bn_finalize"] = (_I, [_P, _I, _I, _F] + [_P] * 5 + [_I, _U, _P, _P, _F, _F, _I, _P])
SIGNATURES["mmvae_bn_act"] = (_I, [_P, _P] + [_I] * 6 + [_P, _F] + [_P] * 5 + [_I, _U, _P, _P, _F, _F, _I, _P])
SIGNATURES["mmvae_bn_bwd_apply"] = (_I, [_P] * 4 + [_I] * 5 + [_P] * 6)
SIGNATURES["mmvae_embed_gather_stats"] = (_I, [_P, _I, _P, _I, _I, _I, _P, _I, _P, _P])
SIGNATURES["mmvae_embed_scatter_add"] = (_I, [_P, _I, _I, _P, _I, _P, _P])
SIGNATURES["mmvae_colsum_f32"] = (_I, [_P, _I, _I, _P, _P])
SIGNATURES["mmvae_colsum_bf16"] = (_I, [_P, _I, _I, _I, _P, _P])
SIGNATURES["mmvae_nn_words_workspace_bytes"] = (_LL, [_I, _LL])
SIGNATURES["mmvae_nn_words_geometry"] = (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)])
SIGNATURES["mmvae_nn_words_norms"] = (_I, [_P, _LL, _I, _P, _P])
SIGNATURES["mmvae_nn_words_nearest"] = (_I, [_P, _I, _P, _P, _LL, _I, _P, _LL, _P, _P, _P])
SIGNATURES["mmvae_nn_words_dists"] = (_I, [_P, _I, _P, _LL, _I, _P, _P])
SIGNATURES["mmvae_mmd_geometry"] = (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)])
SIGNATURES["mmvae_mmd_workspace_bytes"] = (_LL, [_I, _I, _I])
SIGNATURES["mmvae_mmd"] = (_I, [_P, _I, _P, _I, _I, _P, _LL, _P, _P, _P, _P])
SIGNATURES["mmvae_mmd_kernel_matrix"] = (_I, [_P, _I, _P, _I, _I, _P, _P])
SIGNATURES["mmvae_mmd_dy_workspace_bytes"] = (_LL, [_I, _I, _I])
SIGNATURES["mmvae_mmd_dy"] = (_I, [_P, _I, _P, _I, _I, _P, _LL, _F, _P, _P, _I, _P])
SIGNATURES["mmvae_tsne_geometry"] = (_I, [C.POINTER(_I)] * 5)
SIGNATURES["mmvae_tsne_workspace_bytes"] = (_LL, [_I])
SIGNATURES["mmvae_tsne_affinities"] = (_I, [_P, _I, _I, _F, _P, _P, _P, _P, _LL, _P])
SIGNATURES["mmvae_tsne_grad"] = (_I, [_P, _F, _P, _I, _P, _LL, _P, _P, _P])
SIGNATURES["mmvae_tsne_run"] = (_I, [_P, _I, _P, _P, _P, _I, _I, _F, _F, _I, _P, _P, _LL, _P])
SIGNATURES["mmvae_pixelcnn_geometry"] = (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)])
SIGNATURES["mmvae_pixelcnn_param_elems"] = (_LL, [_I] * 5)
SIGNATURES["mmvae_pixelcnn_packed_elems"] = (_LL, [_I] * 5)
SIGNATURES["mmvae_pixelcnn_pack_weights"] = (_I, [_I] * 5 + [_P, _LL, _P, _P])
SIGNATURES["mmvae_pixelcnn_workspace_bytes"] = (_LL, [_I] * 8)
SIGNATURES["mmvae_pixelcnn_sample"] = (_I, [_I] * 5 + [_P, _P, _LL, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P])
SIGNATURES["mmvae_causal_conv_geometry"] = (_I, [C.POINTER(_I)] * 6)
SIGNATURES["mmvae_causal_conv_workspace_bytes"] = (_LL, [_I] * 8)
SIGNATURES["mmvae_causal_conv_forward"] = (_I, [_P, _P, _P, _P, C.POINTER(_I), _I] + [_I] * 7 + [_P, _LL, _P])
SIGNATURES["mmvae_causal_conv_backward_data"] = (_I, [_P, _P, _P, C.POINTER(_I), _I] + [_I] * 7 + [_P, _LL, _P])
SIGNATURES["mmvae_causal_conv_backward_weight"] = (_I, [_P, _P, _P, _P, C.POINTER(_I), _I] + [_I] * 7 + [_P, _LL, _P])
SIGNATURES["mmvae_head_nll_geometry"] = (_I, [C.POINTER(_I)] * 6)
SIGNATURES["mmvae_head_nll_workspace_bytes"] = (_LL, [_I] * 6)
SIGNATURES["mmvae_head_nll_forward"] = (_I, [_P] * 6 + [_I] * 6 + [_P, _LL, _P])
SIGNATURES["mmvae_head_nll_backward"] = (_I, [_P] * 9 + [_I] * 6 + [_P, _LL, _P])
SIGNATURES["mmvae_conv4s2_geometry"] = (_I, [C.POINTER(_I)] * 6)
SIGNATURES["mmvae_conv4s2_workspace_bytes"] = (_LL, [_I] * 5)
SIGNATURES["mmvae_conv4s2_down"] = (_I, [_P] * 4 + [_I, _I, _F] + [_I] * 5 + [_P, _LL, _P])
SIGNATURES["mmvae_conv4s2_up"] = (_I, [_P] * 4 + [_I, _I, _F] + [_I] * 5 + [_P, _LL, _P])
SIGNATURES["mmvae_conv4s2_wgrad"] = (_I, [_P] * 4 + [_I, _F, _P] + [_I] * 5 + [_P, _LL, _P])
SIGNATURES["mmvae_mmgen_geometry"] = (_I, [C.POINTER(_I)] * 6)
SIGNATURES["mmvae_lin_act_workspace_bytes"] = (_LL, [_I] * 4)
SIGNATURES["mmvae_lin_act_fwd"] = (_I, [_P] * 4 + [_I, _I, _I, _I, _F, _I] + [_P, _LL, _P])
SIGNATURES["mmvae_lin_act_dgrad"] = (_I, [_P] * 4 + [_I, _I, _I, _I, _F, _I] + [_P, _LL, _P])
SIGNATURES["mmvae_lin_act_wgrad"] = (_I, [_P] * 5 + [_I, _I, _I, _I, _F, _I] + [_P])
SIGNATURES["mmvae_mnist_infovae_create"] = (_P, [_I, _I])
SIGNATURES["mmvae_mnist_infovae_destroy"] = (None, [_P])
SIGNATURES["mmvae_mnist_infovae_param_count"] = (_LL, [_P])
SIGNATURES["mmvae_mnist_infovae_num_params"] = (_I, [_P])
SIGNATURES["mmvae_mnist_infovae_param_info"] = (_I, [_P, _I, C.c_char_p, C.POINTER(_I), C.POINTER(_I), C.POINTER(_LL)])
SIGNATURES["mmvae_mnist_infovae_bind"] = (_I, [_P, _P, _P])
SIGNATURES["mmvae_mnist_infovae_step_workspace_bytes"] = (_SZ, [_P])
SIGNATURES["mmvae_mnist_infovae_step"] = (_I, [_P, C.POINTER(MnistInfoVAEStepIO), _I, _I, _P])
SIGNATURES["mmvae_mmgen_table_bytes"] = (_LL, [])
SIGNATURES["mmvae_mmgen_build_tables"] = (_I, [_P])
SIGNATURES["mmvae_mmgen_generate"] = (_I, [_P, _P, _I, _P, _I, _I, _I, _ULL, _ULL, _I] + [_P] * 7)
SIGNATURES["mmvae_mmgen_render"] = (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P])
SIGNATURES["mmvae_imgprep_geometry"] = (_I, [C.POINTER(_I)] * 3)
SIGNATURES["mmvae_imgprep_layout"] = (_I, [_I, _I, _I] + [C.POINTER(_I)] * 4)
SIGNATURES["mmvae_imgprep_coeffs"] = (_I, [_I] * 5 + [_P] * 3)
SIGNATURES["mmvae_imgprep_scale_crop"] = (_I, [_P, _LL, _P, _P, _P, _I, _I, _P, _P, _P, _P])
_STATUS = {n for n, (r, _) in SIGNATURES.items() if r is _I and not n.endswith(("_num_params", "_num_bn", "_precision", "_mmtext_hidden", "_coco_steps", "_comm_world", "_probe_read", "_early_ranges", "_strip_max_rows", "_strip_route"))}

_lib = None
_inited = set()


def load():
    """dlopen the library and declare every prototype (works without a GPU)."""
    global _lib
    if _lib is None:
        # PyTorch ships its own libamdhip64: it must be mapped first so that this library's NEEDED entry binds to the
        # same HIP runtime (two runtimes in one process see no devices)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise MMVAEError("%s not found: run `python multimodal-vae_amd/build.py` (hipcc, gfx950). "
                             "There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in _STATUS and rc != 0:
        raise MMVAEError("%s failed (%d): %s" % (name, rc, lib.mmvae_last_error().decode()))
    return rc


@contextlib.contextmanager
def knobs(**kw):
    """Sets the named library knobs (csrc/knobs.h) for the block; behind it, also on an exception, exactly those are back at
    the table's defaults.  A name the table lacks raises."""
    try:
        for k, v in kw.items():
            call("mmvae_debug_set", k.encode(), int(v))
        yield
    finally:
        for k in kw:
            load().mmvae_debug_reset(k.encode())


def knob_default(name):
    """the table's default of one knob"""
    d = C.c_int()
    call("mmvae_debug_get", name.encode(), None, C.byref(d))
    return d.value


def knob_ptr(prefix, t):
    """{prefix_lo: .., prefix_hi: ..} for ``knobs(**...)``: the device pointer of tensor ``t`` (None: null) as the two int halves of
    an ADDR pair (convres_ts, wr_ts, txt_ts)"""
    p = 0 if t is None else t.data_ptr()
    return {prefix + "_lo": C.c_int(p & 0xffffffff).value, prefix + "_hi": C.c_int(p >> 32).value}


def init_device(index):
    if index not in _inited:
        call("mmvae_init", int(index))
        _inited.add(index)


class OwnedEvent:
    """One HIP event created by the library (mmvae_event_create: no timing, no system-scope fence), with the three methods a
    host-side pipeline needs.  ``torch.cuda.Event()`` performs a system-scope release when it completes -- a cache write-back per
    record on the compute stream (include/mmvae_hip.h)."""

    def __init__(self):
        h = C.c_void_p()
        call("mmvae_event_create", C.byref(h))
        self.handle = h.value
        self._h = C.c_void_p(h.value)

    def record(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        call("mmvae_event_record", self._h, C.c_void_p(s.cuda_stream))

    def synchronize(self):
        call("mmvae_event_synchronize", self._h)

    def __del__(self):
        try:
            if self.handle:
                call("mmvae_event_destroy", self._h)
        except Exception:
            pass


class OwnedStream:
    """One HIP stream created by the library (mmvae_stream_create), usable wherever torch takes a stream.  NOT from torch's pool:
    the first ``torch.cuda.Stream()`` of a process creates 32 pool streams, more than the hardware queues the HIP runtime maps
    streams onto, and every kernel of the process slows down (include/mmvae_hip.h)."""

    def __init__(self, device):
        import torch
        h = C.c_void_p()
        with torch.cuda.device(device):
            call("mmvae_stream_create", C.byref(h))
        self.handle = h.value
        self.stream = torch.cuda.ExternalStream(self.handle, device=device)

    def __del__(self):
        try:
            if self.handle:
                load().mmvae_stream_destroy(C.c_void_p(self.handle))
        except Exception:
            pass


def ptr(t):
    """data pointer of a tensor (None -> NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())
