"""ctypes binding of libyvhip.so (include/yv_hip.h) + thin tensor-level wrappers.

PyTorch-ROCm is used only as plumbing: device memory (`tensor.data_ptr()`),
the current HIP stream and `torch.distributed`.  Every op below enqueues
hand-written gfx950 kernels through the C ABI; there is NO fallback path: if the
library is missing or a call fails, a `YvError` is raised.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

# multi-stream schedules (yvhip.pipeline.PipelinedRunner) need more hardware queues than HIP's default 4; only effective
# when set before the process's first HIP call, harmless otherwise
_HWQ_PRESET = os.environ.get("GPU_MAX_HW_QUEUES")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import re
from typing import List, Optional, Tuple

import torch

# hardware queues this process will really have: the variable only counts if HIP was not initialised yet
HW_QUEUES = int(_HWQ_PRESET) if _HWQ_PRESET else (4 if torch.cuda.is_initialized() else 8)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libyvhip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "yv_hip.h"))


class YvError(RuntimeError):
    pass


from .extent import n_anchors, net_hw          # noqa: E402  (host helpers; the module imports YvError from here)


def _load():
    if not os.path.exists(LIB_PATH):
        raise YvError(f"{LIB_PATH} is missing: build it with `make -C yolov8-vit_amd/csrc` "
                      "(or __graft_entry__.build()); there is no CPU fallback")
    return C.CDLL(LIB_PATH)


lib = _load()

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class yv_view(C.Structure):
    _fields_ = [("ptr", _vp), ("ld", _i), ("c", _i), ("up", _i)]


class yv_mx_view(C.Structure):
    _fields_ = [("q", _vp), ("s", _vp), ("ld", _i), ("c", _i), ("up", _i)]


class yv_conv2d_desc(C.Structure):
    _fields_ = [("in0", yv_view), ("in1", yv_view), ("B", _i), ("Hout", _i), ("Wout", _i), ("ksize", _i), ("stride", _i),
                ("weight", _vp), ("bias", _vp), ("Cout", _i), ("out", _vp), ("out_ld", _i), ("res", _vp), ("res_ld", _i),
                ("flags", _i)]


class yv_conv2d_shape(C.Structure):
    _fields_ = [(n, _i) for n in ("B", "Hout", "Wout", "ksize", "stride", "c0", "c1", "Cout", "out_ld", "res_ld", "flags")]


class yv_conv2d_group_plan_t(C.Structure):
    _fields_ = [(n, _i) for n in ("launch", "instance", "first_wg", "position", "work")]


_SIGS = {
    "yv_version": (_i, []),
    "yv_error_string": (C.c_char_p, [_i]),
    "yv_device_is_gfx950": (_i, []),
    "yv_set_option": (_i, [C.c_char_p, _i]),
    "yv_get_option": (_i, [C.c_char_p, _vp]),
    "yv_set_workspace": (_i, [_vp, _vp, _sz]),
    "yv_set_launch_timing": (_i, [_vp, _vp]),
    "yv_linear_mxfp8_q": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _vp, _vp, C.c_longlong, _vp, _i, _i, _i, _i, _vp, _i, _vp,
                               C.c_longlong, _vp, C.c_longlong, _vp]),
    "yv_attention_mxfp8": (_i, [_vp, _i, _i, _i, _f, _vp, C.c_longlong, _vp, C.c_longlong, _vp, _vp]),
    "yv_layernorm_mxfp8": (_i, [_vp, _sz, _vp, _vp, _i, _i, _f, _vp, _sz, _vp, C.c_longlong, _vp, _i, _vp]),
    "yv_mx_probe": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "yv_mx_probe32": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "yv_attention_fp8": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _i, _i, _i, _f, _vp, _vp, _vp, C.c_longlong, _vp,
                              C.c_longlong, _vp]),
    "yv_attention_fp8_dequant": (_i, [_vp, C.c_longlong, _i, _vp, _vp]),
    "yv_quant_mxfp8": (_i, [_vp, C.c_longlong, C.c_longlong, _i, _vp, C.c_longlong, _vp, C.c_longlong, _vp]),
    "yv_quant_mxfp8_map": (_i, [_vp, C.c_longlong, C.c_longlong, _i, _vp, C.c_longlong, _vp, _vp]),
    "yv_conv2d_mxfp8": (_i, [C.POINTER(yv_mx_view), C.POINTER(yv_mx_view), _i, _i, _i, _i, _i, _vp, _vp, C.c_longlong, _vp, _i,
                             _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "yv_conv2d_mxfp8_instance": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "yv_linear_mxfp8": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _vp, _vp, C.c_longlong, _vp, _i, _i, _i, _vp, _i, _i, _vp,
                             _i, _vp]),
    "yv_quant_mxfp8_2d": (_i, [_vp, C.c_longlong, C.c_longlong, _i, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _vp,
                               C.c_longlong, C.c_longlong, _vp]),
    "yv_linear_mxfp8_ex": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _vp, _vp, C.c_longlong, _vp, _i, _i, _i, _vp, _i, _i, _vp,
                                _vp, _i, _vp]),
    "yv_linear_mxfp8_instance": (_i, [_i, _i, _i, _i]),
    "yv_linear_route": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _sz, _i, _vp]),
    "yv_linear_ln": (_i, [_vp, _sz, _vp, _vp, _f, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "yv_linear_ln_route": (_i, [_i, _i, _i, _i, _i, _vp]),
    "yv_linear_mxfp8_q_route": (_i, [_i, _i, _i, _i, _i, _vp]),
    "yv_wgrad_mxfp8": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _i, _i, _i, _vp, _i, _vp]),
    "yv_custom_nms_ws_bytes": (_sz, [_i, _i]),
    "yv_custom_nms": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "yv_efficient_nms": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "yv_efficient_nms_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "yv_efficient_nms_ws": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yv_postprocess_dets": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _i, _i,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yv_compact_crops": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "yv_compact_crops_split": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "yv_crop_resize_norm": (_i, [_vp, _i, _i, _i, _sz, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "yv_pack_results": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "yv_letterbox": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "yv_letterbox_hw": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "yv_augment_patchify": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "yv_train_crops": (_i, [_vp, _sz, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "yv_mosaic_augment": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "yv_mosaic_augment_ex": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yv_detect_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "yv_detect_tail": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "yv_detect_decode_hw": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "yv_detect_tail_hw": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "yv_c2f_debug": (_i, [_vp]),
    "yv_crop_debug": (_i, [_i]),
    "yv_c2f_fused": (_i, [_vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _vp]),
    "yv_optim_step": (_i, [_i, _vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _f, _i, _vp, _vp]),
    "yv_optim_step_rec": (_i, [_i, _vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _vp, _i, _vp, _vp]),
    "yv_grad_clip_ws_bytes": (_sz, [_sz]),
    "yv_grad_clip_record": (_i, [_vp, _sz, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "yv_ema_update": (_i, [_vp, _vp, _sz, _f, _vp]),
    "yv_axpby": (_i, [_vp, _vp, _sz, _f, _f, _vp]),
    "yv_detect_loss_ws_bytes": (_sz, [_i, _i, _i]),
    "yv_detect_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _sz, _vp]),
    "yv_blob_nhwc8": (_i, [_vp, C.c_longlong, _vp, _vp]),
    "yv_bn_ws_floats": (_sz, [C.c_longlong, _i]),
    "yv_bn_stats": (_i, [_vp, C.c_longlong, C.c_longlong, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yv_bn_stats_finish": (_i, [_vp, C.c_longlong, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "yv_conv_stats_ws_floats": (_sz, [C.c_longlong, _i]),
    "yv_conv2d_stats": (_i, [C.POINTER(yv_view), _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "yv_conv2d_bnbwd": (_i, [C.POINTER(yv_view), _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp,
                             _i, _vp, _sz, _vp, _sz, _vp]),
    "yv_conv_bnbwd_ws_floats": (_sz, [C.c_longlong, _i]),
    "yv_conv2d_bnbwd_route": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _sz, _vp]),
    "yv_bn_act_bwd_finish": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, C.c_longlong, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp,
                                  _vp, C.c_longlong, _vp, _vp]),
    "yv_bn_act_fwd": (_i, [_vp, C.c_longlong, C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _vp, C.c_longlong,
                           _i, _vp]),
    "yv_bn_act_bwd": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, C.c_longlong, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp,
                           _vp, C.c_longlong, _vp, _sz, _vp]),
    "yv_view_op": (_i, [_i, _vp, C.c_longlong, _vp, C.c_longlong, _i, _i, _i, _i, _vp]),
    "yv_maxpool5_bwd": (_i, [_vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _i, _i, _i, _i, _vp, _sz, _vp]),
    "yv_im2col3": (_i, [_vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp]),
    "yv_conv_weight_dgrad": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "yv_conv2d": (_i, [C.POINTER(yv_view), C.POINTER(yv_view), _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i,
                       _i, _vp]),
    "yv_conv2d_instance": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _sz]),
    "yv_conv2d_group": (_i, [C.POINTER(yv_conv2d_desc), _i, _vp]),
    "yv_conv2d_group_plan": (_i, [C.POINTER(yv_conv2d_shape), _i, C.POINTER(yv_conv2d_group_plan_t), C.POINTER(_i)]),
    "yv_conv2d_dgrad_s2": (_i, [C.POINTER(yv_view), _i, _i, _i, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "yv_conv2d_dgrad_s2_route": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "yv_conv2d_ws": (_i, [C.POINTER(yv_view), C.POINTER(yv_view), _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i,
                          _i, _vp, _sz, _vp]),
    "yv_linear": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp]),
    "yv_layernorm": (_i, [_vp, _sz, _vp, _vp, _i, _i, _f, _vp, _sz, _vp, _i, _vp]),
    "yv_linear_res_ln": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _vp, _i, _vp]),
    "yv_attention": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_cls": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_long": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp]),
    "yv_attention_debug": (_i, [_i]),
    "yv_cls_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "yv_wrapper_head": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "yv_sppf_pool": (_i, [_vp, _i, _i, _i, _i, _i, _vp]),
    "yv_stem_conv": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "yv_linear_ex": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "yv_attention_train": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_bwd_long": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_bwd_short": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_cls_train": (_i, [_vp, C.c_longlong, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "yv_attention_cls_bwd": (_i, [_vp, C.c_longlong, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "yv_linear_nn": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp]),
    "yv_wgrad": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "yv_wgrad_conv3": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "yv_wgrad_tiled": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "yv_wgrad_conv3_tiled": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "yv_wgrad_conv3_gather": (_i, [_vp, _i, _vp, C.c_longlong, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "yv_wgrad_conv3_gather_route": (_i, [_i, _i, _i, _i, _i, _i, _i, _sz, _i, _vp, _vp]),
    "yv_wgrad_conv3_gather_src": (_i, [_i, _i, _i, _i, _i, _i, _vp]),
    "yv_wgrad_route": (_i, [_i, _i, _i, _i, _sz, _i, _vp]),
    "yv_wgrad_wide": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "yv_wgrad_wide_route": (_i, [_i, _i, _i, _i, _sz, _i, _vp]),
    "yv_transpose_bf16": (_i, [_vp, _i, _i, C.c_longlong, _vp, C.c_longlong, _vp]),
    "yv_cast_weights": (_i, [_vp, _i, _i, _vp, _vp, C.c_longlong, _vp]),
    "yv_colsum_ws_floats": (_sz, [_i, _i]),
    "yv_cast_colsum": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "yv_colsum_bf16": (_i, [_vp, _i, _i, C.c_longlong, _vp, _i, _vp, _vp]),
    "yv_layernorm_bwd_ws_floats": (_sz, [_i, _i]),
    "yv_layernorm_bwd": (_i, [_vp, C.c_longlong, _vp, _vp, C.c_longlong, _i, _i, _f, _vp, C.c_longlong, _vp, _vp, _vp, _vp]),
    "yv_token_reduce": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "yv_head_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "yv_loss_fwd_bwd": (_i, [_vp, _vp, _i, _i, _f, _f, _vp, _vp, _vp]),
    "yv_sgd_step": (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _f, _i, _vp, _vp]),
    "yv_sgd_step_rec": (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _vp, _i, _vp, _vp]),
    "yv_transpose_bf16_batched": (_i, [_vp, _vp, _i, _i, _i, C.c_longlong, C.c_longlong, _vp]),
}


def header_symbols() -> List[str]:
    """Every function include/yv_hip.h declares (used by the CPU symbol test)."""
    txt = open(HEADER_PATH, encoding="utf-8").read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(yv_[a-z0-9_]+)\s*\(", txt)))


MISSING: List[str] = []


def _bind():
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:           # header/library mismatch: recorded, and calling it raises
            MISSING.append(name)
            continue
        fn.restype = res
        fn.argtypes = args


_bind()


def set_option(key: str, value: int):
    check(lib.yv_set_option(key.encode(), int(value)), "yv_set_option")


def get_option(key: str) -> int:
    v = C.c_int(0)
    check(lib.yv_get_option(key.encode(), C.byref(v)), "yv_get_option")
    return int(v.value)


def check(code: int, what: str = ""):
    if code != 0:
        raise YvError(f"{what or 'libyvhip'}: {lib.yv_error_string(code).decode()} ({code})")


def _apply_env_options():
    """YV_OPTIONS="key=value,key=value": yv_set_option pairs applied at import (A/B runs of bench.py / tools without editing
    them); unknown keys fail loudly."""
    spec = os.environ.get("YV_OPTIONS", "")
    for item in filter(None, (x.strip() for x in spec.split(","))):
        k, _, v = item.partition("=")
        set_option(k.strip(), int(v))


_apply_env_options()


def require_gpu():
    if not torch.cuda.is_available():
        raise YvError("no HIP device visible: the hot path has no CPU fallback")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_STREAM_WS = {}


def _st():
    """Current HIP stream handle; the first use of a stream registers its split-K workspace (64 MB)."""
    h = torch.cuda.current_stream().cuda_stream
    key = (torch.cuda.current_device(), h)
    if key not in _STREAM_WS:
        ws = torch.empty((16 * 1024 * 1024,), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        _STREAM_WS[key] = ws
        lib.yv_set_workspace(C.c_void_p(h), C.c_void_p(ws.data_ptr()), ws.numel() * 4)
    return C.c_void_p(h)


def _chk_dev(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise YvError("expected a device tensor")
            if not t.is_contiguous():
                raise YvError("expected a contiguous tensor")


def _chk_rows(t):
    """A 2-D device operand read with a row stride (t.stride(0)): only its rows must be contiguous."""
    if not t.is_cuda:
        raise YvError("expected a device tensor")
    if t.dim() != 2 or t.stride(1) != 1:
        raise YvError("expected a 2-D tensor with contiguous rows")


# ------------------------------------------------------------------ boxes
def custom_nms_batched(boxes: torch.Tensor, scores: torch.Tensor, counts: Optional[torch.Tensor],
                       iou_threshold: float = 0.45):
    """boxes (S,n,4) f32, scores (S,n) f32, counts (S) i32|None -> keep (S,n) i32 (-1 padded), num (S) i32."""
    _chk_dev(boxes, scores, counts)
    S, n = scores.shape
    keep = torch.empty((S, n), dtype=torch.int32, device=boxes.device)
    num = torch.empty((S,), dtype=torch.int32, device=boxes.device)
    wsb = lib.yv_custom_nms_ws_bytes(S, n)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=boxes.device)
    check(lib.yv_custom_nms(_p(boxes), _p(scores), _p(counts), S, n, float(iou_threshold), _p(keep), _p(num),
                            _p(ws), wsb, _st()), "yv_custom_nms")
    return keep, num


def custom_nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float = 0.45) -> List[int]:
    """Reference signature (README.md:62): returns a Python list of kept ORIGINAL indices."""
    require_gpu()
    n = int(scores.shape[0])
    if n == 0:
        return []
    dev = torch.device("cuda", torch.cuda.current_device())
    b = boxes.to(device=dev, dtype=torch.float32).reshape(1, n, 4).contiguous()
    s = scores.to(device=dev, dtype=torch.float32).reshape(1, n).contiguous()
    keep, num = custom_nms_batched(b, s, None, iou_threshold)
    k = int(num[0])
    return keep[0, :k].tolist()


def efficient_nms(boxes: torch.Tensor, scores: torch.Tensor, score_threshold: float = 0.25,
                  iou_threshold: float = 0.65, max_output_boxes: int = 100, pre_nms_topk: int = 4096,
                  single_kernel: bool = False):
    """boxes (B,A,4), scores (B,A,nc) f32 -> (num_dets (B,1) i32, bboxes (B,K,4), scores (B,K), labels (B,K) i32).
    Default: the multi-workgroup form (yv_efficient_nms_ws; scratch from torch's caching allocator, allocated on the current
    stream like the outputs); single_kernel=True runs the one-workgroup-per-image form.  Both give identical outputs."""
    _chk_dev(boxes, scores)
    B, A, nc = scores.shape
    K = max_output_boxes
    dev = boxes.device
    num = torch.empty((B, 1), dtype=torch.int32, device=dev)
    ob = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    osc = torch.empty((B, K), dtype=torch.float32, device=dev)
    ol = torch.empty((B, K), dtype=torch.int32, device=dev)
    if single_kernel:
        check(lib.yv_efficient_nms(_p(boxes), _p(scores), B, A, nc, float(score_threshold), float(iou_threshold), K,
                                   int(pre_nms_topk), _p(num), _p(ob), _p(osc), _p(ol), _st()), "yv_efficient_nms")
        return num, ob, osc, ol
    wsb = int(lib.yv_efficient_nms_ws_bytes(B, A, nc, K, int(pre_nms_topk)))
    if B > 0 and wsb == 0:
        raise YvError("yv_efficient_nms_ws_bytes: arguments out of range")
    ws = torch.empty((max(wsb, 256),), dtype=torch.uint8, device=dev)
    check(lib.yv_efficient_nms_ws(_p(boxes), _p(scores), B, A, nc, float(score_threshold), float(iou_threshold), K,
                                  int(pre_nms_topk), _p(num), _p(ob), _p(osc), _p(ol), _p(ws), wsb, _st()),
          "yv_efficient_nms_ws")
    return num, ob, osc, ol


def postprocess_dets(num_dets, bboxes, scores, labels, ratio, dwdh, img_wh, conf=0.35, dedupe_iou=0.45,
                     coord_mode: str = "trunc", max_crops: int = 0):
    _chk_dev(num_dets, bboxes, scores, labels, ratio, dwdh, img_wh)
    B, slots = scores.shape
    dev = scores.device
    out = {
        "det_count": torch.empty((B,), dtype=torch.int32, device=dev),
        "det_box": torch.empty((B, slots, 4), dtype=torch.int32, device=dev),
        "det_score": torch.empty((B, slots), dtype=torch.float32, device=dev),
        "det_label": torch.empty((B, slots), dtype=torch.int32, device=dev),
        "crop_rect": torch.empty((B, slots, 4), dtype=torch.int32, device=dev),
        "crop_ok": torch.empty((B, slots), dtype=torch.int32, device=dev),
    }
    check(lib.yv_postprocess_dets(_p(num_dets), _p(bboxes), _p(scores), _p(labels), B, slots, _p(ratio), _p(dwdh),
                                  _p(img_wh), float(conf), float(dedupe_iou), 1 if coord_mode == "round" else 0,
                                  int(max_crops), _p(out["det_count"]), _p(out["det_box"]), _p(out["det_score"]),
                                  _p(out["det_label"]), _p(out["crop_rect"]), _p(out["crop_ok"]), _st()),
          "yv_postprocess_dets")
    return out


def compact_crops(det_count, crop_rect, crop_ok, cap: int, parts: int = 0):
    """-> crop_list (cap, 6) i32, total (1,) i32.  parts > 0: total is (1 + parts,) = {total, crops in each of `parts` equal
    slices of ceil(cap / parts) entries} (device-side: the classifier's concurrent half-batches read their counts from it)."""
    _chk_dev(det_count, crop_rect, crop_ok)
    B, slots = crop_ok.shape
    dev = crop_ok.device
    crop_list = torch.empty((max(cap, 1), 6), dtype=torch.int32, device=dev)
    total = torch.empty((1 + max(parts, 0),), dtype=torch.int32, device=dev)
    if parts > 0:
        check(lib.yv_compact_crops_split(_p(det_count), _p(crop_rect), _p(crop_ok), B, slots, cap, parts, _p(crop_list),
                                         _p(total), _st()), "yv_compact_crops_split")
    else:
        check(lib.yv_compact_crops(_p(det_count), _p(crop_rect), _p(crop_ok), B, slots, cap, _p(crop_list), _p(total),
                                   _st()), "yv_compact_crops")
    return crop_list, total


def crop_resize_norm(images: torch.Tensor, crop_list: torch.Tensor, crop_total: Optional[torch.Tensor], cap: int,
                     out_size: int = 224, patch: int = 16, layout: int = 2, out: Optional[torch.Tensor] = None):
    """images (B,H,W,3) u8 -> layout 0: (cap,3,S,S) f32 | 1: same bf16 | 2: (cap*(S/P)^2, 3*P*P) bf16."""
    _chk_dev(images, crop_list, crop_total)
    B, H, W, _ = images.shape
    dev = images.device
    if out is None:
        if layout == 0:
            out = torch.zeros((cap, 3, out_size, out_size), dtype=torch.float32, device=dev)
        elif layout == 1:
            out = torch.zeros((cap, 3, out_size, out_size), dtype=torch.bfloat16, device=dev)
        else:
            g = out_size // patch
            out = torch.zeros((cap * g * g, 3 * patch * patch), dtype=torch.bfloat16, device=dev)
    check(lib.yv_crop_resize_norm(_p(images), B, H, W, H * W * 3, _p(crop_list), _p(crop_total), cap, out_size,
                                  patch, layout, _p(out), _st()), "yv_crop_resize_norm")
    return out


def pack_results(det: dict, cls_label: torch.Tensor, cls_logits: torch.Tensor, cap: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """det: the detect stage's dict (crop_list, crop_total, det_box, det_score, det_label); cls_label (>= cap) i32 and cls_logits
    (>= cap, nc) f32 the classifier's -> (1 + cap, 9 + nc) i32 records (yv_pack_results; yvhip.request.unpack_results reads
    them).  One launch and nothing else, so it can be captured; out: a buffer of that shape to write instead of a new one."""
    cl, ct, box, sc, lab = det["crop_list"], det["crop_total"], det["det_box"], det["det_score"], det["det_label"]
    _chk_dev(cl, ct, box, sc, lab, cls_label, cls_logits, out)
    cap = int(cap)
    if cls_logits.dim() != 2 or sc.dim() != 2:
        raise YvError("pack_results: det_score is (B, slots) and cls_logits (cap, nc)")
    (B, slots), nc = sc.shape, cls_logits.shape[1]
    if cap < 0 or cap > cl.shape[0] or cap > cls_logits.shape[0] or cap > cls_label.shape[0]:
        raise YvError("pack_results: cap exceeds the crop list or the classifier's outputs")
    if (cl.dtype, ct.dtype, box.dtype, lab.dtype, cls_label.dtype) != (torch.int32,) * 5 or \
            (sc.dtype, cls_logits.dtype) != (torch.float32,) * 2 or tuple(box.shape) != (B, slots, 4) or tuple(lab.shape) != (B, slots):
        raise YvError("pack_results: operands do not have the detect stage's types and shapes")
    if out is None:
        out = torch.empty((1 + cap, 9 + nc), dtype=torch.int32, device=sc.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (1 + cap, 9 + nc):
        raise YvError(f"pack_results: out must be ({1 + cap}, {9 + nc}) int32")
    check(lib.yv_pack_results(_p(cl), _p(ct), _p(box), _p(sc), _p(lab), _p(cls_label), _p(cls_logits), B, slots, cap, nc,
                              _p(out), _st()), "yv_pack_results")
    return out


def letterbox(src: torch.Tensor, geom: torch.Tensor, size) -> torch.Tensor:
    """src (B,Hc,Wc,3) u8 canvas, geom (B,6) i32 {w,h,nw,nh,left,top} -> (B,size,size,3) u8; size an (H, W) pair of multiples
    of 32: (B,H,W,3)."""
    _chk_dev(src, geom)
    B, Hc, Wc, _ = src.shape
    if isinstance(size, (tuple, list)):
        H, W = net_hw(size)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=src.device)
        check(lib.yv_letterbox_hw(_p(src), B, Hc, Wc, _p(geom), H, W, _p(out), _st()), "yv_letterbox_hw")
        return out
    out = torch.empty((B, size, size, 3), dtype=torch.uint8, device=src.device)
    check(lib.yv_letterbox(_p(src), B, Hc, Wc, _p(geom), size, _p(out), _st()), "yv_letterbox")
    return out


def augment_patchify(x: torch.Tensor, geo: torch.Tensor, idx: torch.Tensor, patch: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B,3,S,S) f32 normalised crops + one augmentation record per sample (yvhip.augment) ->
    (B*(S/P)^2, 3*P*P) bf16 patch-major rows."""
    _chk_dev(x, geo, idx)
    B, C, S, S2 = x.shape
    if C != 3 or S != S2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise YvError("augment_patchify: x must be a contiguous (B,3,S,S) f32 tensor")
    if tuple(geo.shape) != (B, 6 + 2 * S) or geo.dtype != torch.float32 or not geo.is_contiguous():
        raise YvError("augment_patchify: geo must be (B, 6 + 2S) f32")
    if tuple(idx.shape) != (B, 36 + 2 * S) or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise YvError("augment_patchify: idx must be (B, 36 + 2S) i32")
    g = S // patch
    if out is None:
        out = torch.empty((B * g * g, 3 * patch * patch), dtype=torch.bfloat16, device=x.device)
    check(lib.yv_augment_patchify(_p(x), B, S, patch, _p(geo), _p(idx), _p(out), _st()), "yv_augment_patchify")
    return out


def train_crops(pool: torch.Tensor, table: torch.Tensor, plan: torch.Tensor, geo: torch.Tensor, idx: torch.Tensor,
                size: int, patch: int, layout: int = 2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pool (bytes,) u8 decoded source images, table (n,3) i64 {offset, width, height}, plan (B,5) i32 {image, x0, y0, x1, y1}
    + one augmentation record per sample (yvhip.augment) -> layout 2: (B*(S/P)^2, 3*P*P) bf16 patch-major rows |
    layout 0: (B,3,S,S) f32.  Crop + nearest resize + normalise + the record in one pass (yvhip.crop_loader feeds it)."""
    _chk_dev(pool, table, plan, geo, idx)
    S = int(size)
    if pool.dim() != 1 or pool.dtype != torch.uint8 or pool.numel() < 3:
        raise YvError("train_crops: pool must be a flat u8 tensor of at least 3 bytes")
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or table.dtype != torch.int64:
        raise YvError("train_crops: table must be (n_images, 3) i64 {offset, width, height}")
    B = plan.shape[0]
    if tuple(plan.shape) != (B, 5) or plan.dtype != torch.int32:
        raise YvError("train_crops: plan must be (B, 5) i32 {image, x0, y0, x1, y1}")
    if S <= 0 or S % 8:
        raise YvError("train_crops: size must be a positive multiple of 8")
    if tuple(geo.shape) != (B, 6 + 2 * S) or geo.dtype != torch.float32:
        raise YvError("train_crops: geo must be (B, 6 + 2S) f32")
    if tuple(idx.shape) != (B, 36 + 2 * S) or idx.dtype != torch.int32:
        raise YvError("train_crops: idx must be (B, 36 + 2S) i32")
    if layout not in (0, 2):
        raise YvError("train_crops: layout is 0 (f32 CHW) or 2 (bf16 patch-major rows)")
    if layout == 2:
        if patch < 8 or patch % 8 or S % patch:
            raise YvError("train_crops: patch must be a multiple of 8 dividing size")
        g = S // patch
        shape, dtype = (B * g * g, 3 * patch * patch), torch.bfloat16
    else:
        shape, dtype = (B, 3, S, S), torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=pool.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_cuda or not out.is_contiguous():
        raise YvError(f"train_crops: out must be a contiguous device tensor {shape} {dtype}")
    check(lib.yv_train_crops(_p(pool), pool.numel(), _p(table), table.shape[0], _p(plan), B, S, int(patch), _p(geo), _p(idx),
                             int(layout), _p(out), _st()), "yv_train_crops")
    return out


def mosaic_augment(tiles: torch.Tensor, rec_f: torch.Tensor, rec_i: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """tiles (N,S,S,3) u8 + one record per output image (yvhip.yolo_augment) -> (B,S,S,3) u8 augmented detector inputs."""
    _chk_dev(tiles, rec_f, rec_i, lut)
    N, S, S2, C = tiles.shape
    B = rec_f.shape[0]
    if C != 3 or S != S2 or tiles.dtype != torch.uint8 or not tiles.is_contiguous():
        raise YvError("mosaic_augment: tiles must be a contiguous (N,S,S,3) u8 tensor")
    if tuple(rec_f.shape) != (B, 6) or rec_f.dtype != torch.float32 or not rec_f.is_contiguous():
        raise YvError("mosaic_augment: rec_f must be (B,6) f32")
    if tuple(rec_i.shape) != (B, 34) or rec_i.dtype != torch.int32 or not rec_i.is_contiguous():
        raise YvError("mosaic_augment: rec_i must be (B,34) i32")
    if tuple(lut.shape) != (B, 3, 256) or lut.dtype != torch.uint8 or not lut.is_contiguous():
        raise YvError("mosaic_augment: lut must be (B,3,256) u8")
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=tiles.device)
    check(lib.yv_mosaic_augment(_p(tiles), N, B, S, _p(rec_f), _p(rec_i), _p(lut), _p(out), _st()), "yv_mosaic_augment")
    return out


def mosaic_augment_ex(tiles: torch.Tensor, rec_h: torch.Tensor, rec_i: torch.Tensor, mix: Optional[torch.Tensor],
                      lut: torch.Tensor) -> torch.Tensor:
    """tiles (N,S,S,3) u8 + per output image `layers` (1 or 2) records: rec_h (B,layers,9) f32 inverse homographies,
    rec_i (B,layers,34) i32, mix (B) f32 weight of layer 0 (None allowed with one layer), lut (B,3,256) u8
    -> (B,S,S,3) u8: rotation / shear / perspective / flipud / mixup of the detector trainer (yvhip.yolo_augment)."""
    _chk_dev(tiles, rec_h, rec_i, mix, lut)
    if tiles.dim() != 4 or tiles.shape[3] != 3 or tiles.shape[1] != tiles.shape[2] or tiles.shape[0] < 1 \
            or tiles.dtype != torch.uint8:
        raise YvError("mosaic_augment_ex: tiles must be a contiguous (N,S,S,3) u8 tensor")
    N, S = tiles.shape[0], tiles.shape[1]
    if rec_h.dim() != 3 or rec_h.shape[1] not in (1, 2) or rec_h.shape[2] != 9 or rec_h.dtype != torch.float32:
        raise YvError("mosaic_augment_ex: rec_h must be (B,layers,9) f32 with layers 1 or 2")
    B, layers = rec_h.shape[0], rec_h.shape[1]
    if tuple(rec_i.shape) != (B, layers, 34) or rec_i.dtype != torch.int32:
        raise YvError("mosaic_augment_ex: rec_i must be (B,layers,34) i32")
    if mix is None:
        if layers == 2:
            raise YvError("mosaic_augment_ex: mix is required with two layers")
    elif tuple(mix.shape) != (B,) or mix.dtype != torch.float32:
        raise YvError("mosaic_augment_ex: mix must be (B) f32")
    if tuple(lut.shape) != (B, 3, 256) or lut.dtype != torch.uint8:
        raise YvError("mosaic_augment_ex: lut must be (B,3,256) u8")
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=tiles.device)
    check(lib.yv_mosaic_augment_ex(_p(tiles), N, B, S, layers, _p(rec_h), _p(rec_i), _p(mix), _p(lut), _p(out), _st()),
          "yv_mosaic_augment_ex")
    return out


def detect_decode(box_logits, cls_logits, size, nc: int):
    """box_logits: 3 x (B,Hs,Ws,64) f32; cls_logits: 3 x (B,Hs,Ws,ld) f32 -> boxes (B,A,4), scores (B,A,nc).  size: the network
    input's side, or its (H, W)."""
    _chk_dev(*box_logits, *cls_logits)
    B = box_logits[0].shape[0]
    ld = cls_logits[0].shape[-1]
    dev = box_logits[0].device
    if isinstance(size, (tuple, list)):
        H, W = net_hw(size)
        A = n_anchors(H, W)
        boxes = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((B, A, nc), dtype=torch.float32, device=dev)
        check(lib.yv_detect_decode_hw(_p(box_logits[0]), _p(box_logits[1]), _p(box_logits[2]), _p(cls_logits[0]),
                                      _p(cls_logits[1]), _p(cls_logits[2]), ld, B, H, W, nc, _p(boxes), _p(scores), _st()),
              "yv_detect_decode_hw")
        return boxes, scores
    A = sum((size // s) ** 2 for s in (8, 16, 32))
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, A, nc), dtype=torch.float32, device=dev)
    check(lib.yv_detect_decode(_p(box_logits[0]), _p(box_logits[1]), _p(box_logits[2]), _p(cls_logits[0]),
                               _p(cls_logits[1]), _p(cls_logits[2]), ld, B, size, nc, _p(boxes), _p(scores), _st()),
          "yv_detect_decode")
    return boxes, scores


def detect_tail(feats, c3: int, w2, b2, w3, b3, size, nc: int):
    """Fused Detect tail: feats 3 x (B,Hs,Ws,ld) bf16 (box-branch features in channels 0..63, class-branch features behind them);
    w2 3 x (64,64) bf16, b2 3 x (64) f32, w3 3 x (16,c3) bf16 (rows >= nc zero), b3 3 x (16) f32 -> boxes (B,A,4), scores (B,A,nc),
    bit-identical to the two 1 x 1 convolutions + detect_decode.  size: the network input's side, or its (H, W)."""
    _chk_dev(*feats, *w2, *b2, *w3, *b3)
    B, ld = feats[0].shape[0], feats[0].shape[-1]
    dev = feats[0].device
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    if isinstance(size, (tuple, list)):
        H, W = net_hw(size)
        A = n_anchors(H, W)
        boxes = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((B, A, nc), dtype=torch.float32, device=dev)
        check(lib.yv_detect_tail_hw(_p(feats[0]), _p(feats[1]), _p(feats[2]), ld, c3, arr(w2), arr(b2), arr(w3), arr(b3), B, H, W,
                                    nc, _p(boxes), _p(scores), _st()), "yv_detect_tail_hw")
        return boxes, scores
    A = sum((size // s) ** 2 for s in (8, 16, 32))
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, A, nc), dtype=torch.float32, device=dev)
    check(lib.yv_detect_tail(_p(feats[0]), _p(feats[1]), _p(feats[2]), ld, c3, arr(w2), arr(b2), arr(w3), arr(b3), B, size, nc,
                             _p(boxes), _p(scores), _st()), "yv_detect_tail")
    return boxes, scores


def c2f_fused(x: torch.Tensor, c: int, n: int, w_cv1, b_cv1, w_m, b_m, w_cv2, b_cv2, out: torch.Tensor):
    """One launch for a backbone C2f block (cv1, n bottlenecks with shortcut, cv2; SiLU everywhere): x (B,H,W,2c) bf16 ->
    out (B,H,W,2c) bf16; weights (Cout, k*k*Cin) bf16 / biases f32 as conv2d takes them, w_m / b_m = [m0.cv1, m0.cv2, ...]."""
    _chk_dev(x, out, w_cv1, b_cv1, w_cv2, b_cv2, *w_m, *b_m)
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    check(lib.yv_c2f_fused(_p(x), x.stride(2), B, H, W, c, n, _p(w_cv1), _p(b_cv1), arr(w_m), arr(b_m), _p(w_cv2), _p(b_cv2),
                           _p(out), out.stride(2), _st()), "yv_c2f_fused")
    return out


# --------------------------------------------------------------- training
def loss_fwd_bwd(logits: torch.Tensor, labels: torch.Tensor, w_lsce: float = 1.0 / 6.0, w_focal: float = 5.0 / 6.0):
    _chk_dev(logits, labels)
    B, nc = logits.shape
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits)
    check(lib.yv_loss_fwd_bwd(_p(logits), _p(labels), B, nc, float(w_lsce), float(w_focal), _p(loss), _p(grad), _st()),
          "yv_loss_fwd_bwd")
    return loss, grad


def sgd_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, lr: float, momentum: float = 0.9,
             weight_decay: float = 1e-3, first: bool = False, grad_scale: float = 1.0,
             mirror: Optional[torch.Tensor] = None, scale_rec: Optional[torch.Tensor] = None):
    """scale_rec: the record of grad_clip_record in place of grad_scale (yv_sgd_step_rec); None: yv_sgd_step."""
    _chk_dev(p, g, m, mirror)
    if scale_rec is not None:
        _chk_rec(scale_rec, grad_scale)
        check(lib.yv_sgd_step_rec(_p(p), _p(g), _p(m), p.numel(), float(lr), float(momentum), float(weight_decay), _p(scale_rec),
                                  1 if first else 0, _p(mirror), _st()), "yv_sgd_step_rec")
        return
    check(lib.yv_sgd_step(_p(p), _p(g), _p(m), p.numel(), float(lr), float(momentum), float(weight_decay),
                          float(grad_scale), 1 if first else 0, _p(mirror), _st()), "yv_sgd_step")


def transpose_bf16_batched(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, batch: int = 1, src_stride: int = 0,
                           dst_stride: int = 0):
    """dst[b] (cols, rows) = src[b] (rows, cols)^T for b < batch; strides in elements between consecutive matrices."""
    _chk_dev(src, dst)
    check(lib.yv_transpose_bf16_batched(_p(src), _p(dst), rows, cols, batch, src_stride, dst_stride, _st()),
          "yv_transpose_bf16_batched")


# ------------------------------------------------------------- dense math
EPI_BIAS, EPI_SILU, EPI_GELU, EPI_RES_F32, EPI_RES_BF16, EPI_OUT_F32, EPI_POSEMB = 1, 2, 4, 8, 16, 32, 64
LINEAR_HOOK = None      # callable(M, N, K, start_event, end_event) or None
CONV_HOOK = None        # the same for conv2d (tools/conv_small_bench.py, tools/conv_dma32_bench.py): every bf16 convolution kernel attaches
                        # the events to its launch (a split-K launch to its main kernel, not to the reduce pass)


_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        _HIP.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        _HIP.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _HIP.hipEventDestroy.argtypes = [C.c_void_p]
        _HIP.hipEventSynchronize.argtypes = [C.c_void_p]
    return _HIP


_EVENT_POOL: list = []


def reserve_events(n: int):
    """Create n HipEvents ahead of a timed region (hipEventCreate inside it would be host time on the measured path)."""
    while len(_EVENT_POOL) < n:
        _EVENT_POOL.append(HipEvent())


def _timing_event() -> "HipEvent":
    return _EVENT_POOL.pop() if _EVENT_POOL else HipEvent()


class HipEvent:
    """Plain hipEvent_t (timing enabled) for launch-attached timestamps; elapsed_time() in ms like torch.cuda.Event."""

    def __init__(self):
        self.handle = C.c_void_p()
        if _hip().hipEventCreate(C.byref(self.handle)) != 0:
            raise YvError("hipEventCreate failed")

    def record(self, stream: Optional[int] = None):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if _hip().hipEventRecord(self.handle, C.c_void_p(st)) != 0:
            raise YvError("hipEventRecord failed")

    def elapsed_time(self, other: "HipEvent") -> float:
        ms = C.c_float()
        rc = _hip().hipEventElapsedTime(C.byref(ms), self.handle, other.handle)
        if rc != 0:
            raise YvError(f"hipEventElapsedTime failed ({rc})")
        return float(ms.value)

    def __del__(self):
        try:
            if self.handle:
                _hip().hipEventDestroy(self.handle)
        except Exception:
            pass


def view(t: torch.Tensor, c_off: int, c: int, up: int = 0) -> "yv_view":
    """NHWC bf16 tensor (B,H,W,ld) -> operand view of channels [c_off, c_off+c)."""
    assert t.dtype == torch.bfloat16 and t.is_cuda and t.is_contiguous()
    return yv_view(C.c_void_p(t.data_ptr() + 2 * c_off), t.shape[-1], c, up)


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, flags: int = 0,
           pos: Optional[torch.Tensor] = None, tok: int = 0, m_dev: Optional[torch.Tensor] = None, m_mul: int = 1,
           M: Optional[int] = None):
    """out[M,N] (+)= a[M,K] @ w[N,K]^T with the fused epilogue selected by `flags`."""
    _chk_dev(w, bias, pos, m_dev)
    for t in (a, out):                       # row-strided 2-D views (every N-th row, a column range) are operands as they are
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise YvError("expected a device matrix with unit column stride")
    Mr = a.shape[0] if M is None else M
    K = a.shape[1]
    N = w.shape[0]
    assert w.shape[1] == K and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    if bias is not None:
        flags |= EPI_BIAS
    hook = LINEAR_HOOK
    if hook is not None:                     # bench.py: HIP events attached to the launch itself (hipExtLaunchKernel)
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_linear(_p(a), a.stride(0), _p(w), _p(bias), Mr, N, K, _p(out), out.stride(0), _p(pos), tok, flags,
                        _p(m_dev), m_mul, _st()), "yv_linear")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)             # not consumed when the call took a non-DMA kernel path
        hook(Mr, N, K, e0, e1)
    return out


def linear_ln(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, h: torch.Tensor, w: torch.Tensor,
              bias: Optional[torch.Tensor], out: torch.Tensor, flags: int = 0, eps: float = 1e-6,
              m_dev: Optional[torch.Tensor] = None, m_mul: int = 1, M: Optional[int] = None):
    """out[M,N] = LayerNorm(x[M,K] f32; gamma, beta, eps) @ w[N,K]^T with the epilogue `flags` select: one launch where
    linear_ln_route answers fused (h is then not written), else layernorm into h followed by linear.  See yv_linear_ln."""
    _chk_dev(w, bias, gamma, beta, m_dev)
    for t in (x, h, out):                    # row-strided 2-D views are operands as they are
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise YvError("expected a device matrix with unit column stride")
    Mr = x.shape[0] if M is None else M
    K = x.shape[1]
    N = w.shape[0]
    assert w.shape[1] == K and h.shape[1] == K and out.shape[1] == N
    assert x.dtype == torch.float32 and h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == K
    assert out.dtype == (torch.float32 if flags & EPI_OUT_F32 else torch.bfloat16)
    assert min(x.shape[0], h.shape[0], out.shape[0]) >= Mr
    if bias is not None:
        flags |= EPI_BIAS
    hook = LINEAR_HOOK
    if hook is not None:                     # HIP events attached to the launch itself (the linear's, where the pair runs)
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_linear_ln(_p(x), x.stride(0), _p(gamma), _p(beta), float(eps), _p(h), h.stride(0), _p(w), _p(bias), _p(out),
                           out.stride(0), Mr, N, K, flags, _p(m_dev), m_mul, _st()), "yv_linear_ln")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)
        hook(Mr, N, K, e0, e1)
    return out


LinearLnRoute = collections.namedtuple("LinearLnRoute", "fused tiles_m tiles_n workgroups")


def linear_ln_route(M: int, N: int, K: int, flags: int = 0, n_cu: int = 0) -> LinearLnRoute:
    """What linear_ln does for this shape under the current options (host only): see yv_linear_ln_route in include/yv_hip.h.
    `flags` as the C entry takes them (EPI_BIAS is NOT added); n_cu = 0: the current device's CU count (needs a GPU)."""
    out = (C.c_int * len(LinearLnRoute._fields))()
    check(lib.yv_linear_ln_route(M, N, K, flags, n_cu, out), "yv_linear_ln_route")
    return LinearLnRoute(*out)


RES_LN_WIDTHS = (128, 768, 1024)          # output widths yv_linear_res_ln has an instance for (a tile spans the row)


def linear_res_ln(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor,
                  beta: torch.Tensor, h: torch.Tensor, eps: float = 1e-6, m_dev: Optional[torch.Tensor] = None, m_mul: int = 1,
                  M: Optional[int] = None):
    """x[M,N] (f32) += a[M,K] @ w[N,K]^T + bias and h[M,N] (bf16) = LayerNorm(x; gamma, beta, eps) in one launch."""
    _chk_dev(w, bias, gamma, beta, m_dev)
    for t in (a, x, h):                      # row-strided 2-D views are operands as they are
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise YvError("expected a device matrix with unit column stride")
    Mr = a.shape[0] if M is None else M
    K = a.shape[1]
    N = w.shape[0]
    assert w.shape[1] == K and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    assert x.dtype == torch.float32 and h.dtype == torch.bfloat16 and x.shape[1] == N and h.shape[1] == N
    assert bias.dtype == gamma.dtype == beta.dtype == torch.float32 and bias.numel() == gamma.numel() == beta.numel() == N
    hook = LINEAR_HOOK
    if hook is not None:                     # bench.py: HIP events attached to the launch itself (hipExtLaunchKernel)
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_linear_res_ln(_p(a), a.stride(0), _p(w), _p(bias), Mr, N, K, _p(x), x.stride(0), _p(gamma), _p(beta),
                               float(eps), _p(h), h.stride(0), _p(m_dev), m_mul, _st()), "yv_linear_res_ln")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)
        hook(Mr, N, K, e0, e1)
    return x, h


_CONV_WS = {}


def _conv_workspace(device) -> torch.Tensor:
    """Split-K partial-sum workspace (64 MB f32 per device, allocated once; launches on one stream serialise on it)."""
    key = str(device)
    if key not in _CONV_WS:
        _CONV_WS[key] = torch.empty((CONV_WS_BYTES // 4,), dtype=torch.float32, device=device)
    return _CONV_WS[key]


def conv2d(in0: "yv_view", in1: Optional["yv_view"], B: int, Hout: int, Wout: int, ksize: int, stride: int,
           weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, out_c_off: int, flags: int,
           res: Optional[torch.Tensor] = None, res_c_off: int = 0):
    """Conv2d + bias (+SiLU ...) ; `out` is a (B,Hout,Wout,ld) tensor, written at channel offset out_c_off."""
    Cout = weight.shape[0]
    esz = 4 if (flags & EPI_OUT_F32) else 2
    optr = C.c_void_p(out.data_ptr() + esz * out_c_off)
    rptr = None if res is None else C.c_void_p(res.data_ptr() + 2 * res_c_off)
    ws = _conv_workspace(out.device)
    hook = CONV_HOOK
    if hook is not None:
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_conv2d_ws(C.byref(in0), C.byref(in1) if in1 is not None else None, B, Hout, Wout, ksize, stride,
                           _p(weight), _p(bias), Cout, optr, out.shape[-1], rptr,
                           0 if res is None else res.shape[-1], flags | EPI_BIAS, _p(ws), ws.numel() * 4, _st()),
          "yv_conv2d_ws")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)             # (nothing stays armed for a later launch)
        hook(B * Hout * Wout, Cout, e0, e1)
    return out


CONV_WS_BYTES = 16 * 1024 * 1024 * 4      # the workspace conv2d passes (what conv2d_instance assumes by default)
# conv2d_instance codes: kernel instance in the low four bits ...
CONV_IGEMM_16, CONV_IGEMM_32, CONV_IGEMM_64, CONV_IGEMM_128 = 0, 1, 2, 3
CONV_DMA_64_2, CONV_DMA_64_3, CONV_DMA_64_4, CONV_DMA_128_2, CONV_DMA_128_3 = 4, 5, 6, 7, 8
CONV_SMALL_64, CONV_SMALL_32 = 9, 10      # cgemm_small_kernel<64, 2> / <32, 4>: only under the option "conv_small"
# cgemm_dma32_kernel<64, ..> / <128, ..>: only under the option "conv_dma32" (12: the 96-wide instance, measured and not built)
CONV_DMA32_64, CONV_DMA32_96, CONV_DMA32_128 = 11, 12, 13
# ... and flag bits: the staged epilogue runs, split-K, the two-source igemm instantiation
CONV_STAGED, CONV_SPLITK, CONV_TWO = 16, 32, 64


def conv2d_instance(B: int, Hout: int, Wout: int, ksize: int, stride: int, c0: int, c1: int, Cout: int, out_ld: int,
                    res_ld: int = 0, flags: int = 0, ws_bytes: int = CONV_WS_BYTES) -> int:
    """Route conv2d takes for this shape under the current options (host only, no GPU needed): kernel instance | CONV_STAGED |
    CONV_SPLITK | CONV_TWO, see yv_conv2d_instance in include/yv_hip.h.  `flags` as conv2d takes them (EPI_BIAS is added);
    16-byte aligned bases are assumed."""
    r = lib.yv_conv2d_instance(B, Hout, Wout, ksize, stride, c0, c1, Cout, out_ld, res_ld, flags | EPI_BIAS, ws_bytes)
    check(min(r, 0), "yv_conv2d_instance")
    return r


CONV_GROUP_MAX = 8                        # YV_CONV_GROUP_MAX: members of one grouped launch
CONV_GROUP_INSTANCES = (CONV_DMA_64_3, CONV_SMALL_64, CONV_SMALL_32)     # the instances that have a grouped form


def conv2d_group(members):
    """Independent convolutions as one call (yv_conv2d_group): `members` is a sequence of conv2d's argument lists,
    (in0, in1, B, Hout, Wout, ksize, stride, weight, bias, out, out_c_off, flags[, res[, res_c_off]]).  The members on one of
    CONV_GROUP_INSTANCES run as one grid per instance (CONV_GROUP_MAX at most), the others alone; every member's output is, bit
    for bit, what conv2d without split-K writes for it alone.  No member may read what another writes: they run concurrently.
    With CONV_HOOK set, the events are armed for the call's FIRST launch only and the hook gets them with M = N = 0:
    time a call whose members are exactly one launch of conv2d_group_plan (tools/conv_group_bench.py)."""
    d = (yv_conv2d_desc * max(len(members), 1))()
    for x, m in zip(d, members):
        in0, in1, B, Hout, Wout, ksize, stride, weight, bias, out, out_c_off, flags = m[:12]
        res = m[12] if len(m) > 12 else None
        res_c_off = m[13] if len(m) > 13 else 0
        esz = 4 if (flags & EPI_OUT_F32) else 2
        x.in0 = in0
        if in1 is not None:
            x.in1 = in1
        x.B, x.Hout, x.Wout, x.ksize, x.stride = B, Hout, Wout, ksize, stride
        x.weight, x.bias, x.Cout = weight.data_ptr(), bias.data_ptr(), weight.shape[0]
        x.out, x.out_ld = out.data_ptr() + esz * out_c_off, out.shape[-1]
        if res is not None:
            x.res, x.res_ld = res.data_ptr() + 2 * res_c_off, res.shape[-1]
        x.flags = flags | EPI_BIAS
    hook = CONV_HOOK
    if hook is not None:
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    try:
        check(lib.yv_conv2d_group(d, len(members), _st()), "yv_conv2d_group")
    finally:
        if hook is not None:
            lib.yv_set_launch_timing(None, None)         # (also where the call failed: nothing stays armed for a later launch)
    if hook is not None:
        hook(0, 0, e0, e1)


def conv2d_group_plan(shapes):
    """The partition conv2d_group makes of members of these shapes under the current options (host only, no GPU needed; see
    yv_conv2d_group_plan in include/yv_hip.h).  `shapes`: (B, Hout, Wout, ksize, stride, c0, c1, Cout, out_ld[, res_ld[, flags]])
    per member, flags as conv2d takes them (EPI_BIAS is added).  Returns (number of launches, [per member: dict(launch, instance,
    first_wg, position, work)]); `instance` is conv2d_instance(..., ws_bytes=0) of the member alone."""
    n = len(shapes)
    sh = (yv_conv2d_shape * max(n, 1))()
    for x, s in zip(sh, shapes):
        s = tuple(s) + (0, 0)[len(s) - 9:]
        x.B, x.Hout, x.Wout, x.ksize, x.stride, x.c0, x.c1, x.Cout, x.out_ld, x.res_ld = s[:10]
        x.flags = s[10] | EPI_BIAS
    out = (yv_conv2d_group_plan_t * max(n, 1))()
    launches = C.c_int(0)
    check(lib.yv_conv2d_group_plan(sh, n, out, C.byref(launches)), "yv_conv2d_group_plan")
    return int(launches.value), [{f: int(getattr(o, f)) for f, _ in yv_conv2d_group_plan_t._fields_} for o in out[:n]]


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y: torch.Tensor, rows: int, D: int,
              ldx: int, ldy: int, eps: float = 1e-6, count_dev: Optional[torch.Tensor] = None,
              rows_per_count: int = 1):
    check(lib.yv_layernorm(_p(x), ldx, _p(gamma), _p(beta), rows, D, float(eps), _p(y), ldy, _p(count_dev),
                           rows_per_count, _st()), "yv_layernorm")
    return y


def attention(qkv: torch.Tensor, R: int, N: int, H: int, out: torch.Tensor, scale: Optional[float] = None,
              r_dev: Optional[torch.Tensor] = None):
    _chk_dev(qkv, out, r_dev)
    check(lib.yv_attention(_p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale), _p(out), _p(r_dev),
                           _st()), "yv_attention")
    return out


def attention_long(qkv: torch.Tensor, R: int, N: int, H: int, out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                   r_dev: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                   out_q: Optional[torch.Tensor] = None, out_scale: Optional[torch.Tensor] = None):
    """The attention forward for sequences longer than one K/V tile (yv_attention_long; any N >= 1 is accepted).  Outputs, any
    combination with at least one of out / out_q: out (R*N, H*64) bf16; lse (R, H, N) f32 for attention_bwd; out_q / out_scale,
    the MXFP8 operand image of attention_mxfp8 (bytes (rows, >= H*64) + scales (H*64 // 128, rows_pad, 4)); r_dev: crop count."""
    _chk_dev(qkv, out, r_dev, lse, out_q, out_scale)
    if (out_q is None) != (out_scale is None):
        raise YvError("attention_long: out_q and out_scale come together")
    check(lib.yv_attention_long(_p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale), _p(out), _p(r_dev), _p(lse),
                                _p(out_q), 0 if out_q is None else out_q.stride(0), _p(out_scale),
                                0 if out_scale is None else out_scale.shape[1], _st()), "yv_attention_long")
    return out


def attention_cls(q: torch.Tensor, qkv: torch.Tensor, R: int, N: int, H: int, out: torch.Tensor,
                  scale: Optional[float] = None, r_dev: Optional[torch.Tensor] = None):
    """Attention of the cls query of each crop: q (R, H*64) compact, K | V from the qkv buffer (R*N, 3*H*64), out (R, H*64)."""
    _chk_dev(q, qkv, out, r_dev)
    check(lib.yv_attention_cls(_p(q), _p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale), _p(out), _p(r_dev),
                               _st()), "yv_attention_cls")
    return out


def cls_rows(cls: torch.Tensor, pos: torch.Tensor, R: int, tok: int, D: int, x: torch.Tensor):
    check(lib.yv_cls_rows(_p(cls), _p(pos), R, tok, D, _p(x), _st()), "yv_cls_rows")


def wrapper_head(feats: torch.Tensor, w1, b1, w2, b2, R: int, nc: int, logits: torch.Tensor, labels: torch.Tensor,
                 scale: float = 1.0, accumulate: bool = False, r_dev: Optional[torch.Tensor] = None):
    check(lib.yv_wrapper_head(_p(feats), feats.stride(0), _p(w1), _p(b1), _p(w2), _p(b2), R, nc, float(scale),
                              1 if accumulate else 0, _p(logits), _p(labels), _p(r_dev), _st()), "yv_wrapper_head")


def sppf_pool(buf: torch.Tensor, c: int):
    B, H, W, ld = buf.shape
    check(lib.yv_sppf_pool(_p(buf), B, H, W, ld, c, _st()), "yv_sppf_pool")


def stem_conv(images: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor):
    B, H, W, _ = images.shape
    check(lib.yv_stem_conv(_p(images), B, H, W, _p(weight), _p(bias), weight.shape[1], _p(out), out.shape[-1],
                           _st()), "yv_stem_conv")


# ------------------------------------------------------------ training ops
EPI_SAVE_PRE, EPI_GELU_BWD = 128, 256


def linear_ex(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, flags: int = 0,
              res_f32: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None, M: Optional[int] = None):
    """Training form of `linear` (separate f32 residual source, saved pre-activation, GELU backward)."""
    _chk_dev(a, w, bias, out, res_f32, aux)
    Mr = a.shape[0] if M is None else M
    K, N = a.shape[1], w.shape[0]
    if bias is not None:
        flags |= EPI_BIAS
    check(lib.yv_linear_ex(_p(a), a.stride(0), _p(w), _p(bias), Mr, N, K, _p(out), out.stride(0), flags, _p(res_f32),
                           _p(aux), 0 if aux is None else aux.stride(0), _st()), "yv_linear_ex")
    return out


def attention_train(qkv, R, N, H, out, lse, scale=None):
    check(lib.yv_attention_train(_p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale), _p(out), _p(lse),
                                 _st()), "yv_attention_train")


def attention_bwd(qkv, out, dout, lse, R, N, H, dqkv, delta_ws, scale=None):
    check(lib.yv_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), R, N, H, float(64 ** -0.5 if scale is None else scale),
                               _p(dqkv), _p(delta_ws), _st()), "yv_attention_bwd")


def attention_bwd_long(qkv, out, dout, lse, R, N, H, dqkv, delta_ws, scale=None):
    """attention_bwd for sequences longer than one tile (yv_attention_bwd_long; any N >= 1 is accepted): the same operands and,
    on finite inputs, the same bits in dqkv and delta_ws."""
    check(lib.yv_attention_bwd_long(_p(qkv), _p(out), _p(dout), _p(lse), R, N, H, float(64 ** -0.5 if scale is None else scale),
                                    _p(dqkv), _p(delta_ws), _st()), "yv_attention_bwd_long")


def attention_bwd_short(qkv, out, dout, lse, R, N, H, dqkv, delta_ws, scale=None):
    """attention_bwd in one launch for sequences of up to 224 tokens (yv_attention_bwd_short; N > 224 is refused): the same
    operands and, on finite inputs, the same bits in dqkv and delta_ws."""
    check(lib.yv_attention_bwd_short(_p(qkv), _p(out), _p(dout), _p(lse), R, N, H, float(64 ** -0.5 if scale is None else scale),
                                     _p(dqkv), _p(delta_ws), _st()), "yv_attention_bwd_short")


def attention_cls_train(q, qkv, R, N, H, out, lse, scale=None):
    """attention_cls for the trainer (yv_attention_cls_train): q (R, H*64) bf16 with any row stride (a view of the qkv buffer's
    cls rows needs no copy), out (R, H*64) bf16 compact with the bits of attention_cls, lse (R*H) f32 in the log2 domain."""
    _chk_dev(qkv, out, lse)
    _chk_rows(q)
    check(lib.yv_attention_cls_train(_p(q), q.stride(0), _p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale),
                                     _p(out), _p(lse), _st()), "yv_attention_cls_train")
    return out


def attention_cls_bwd(q, qkv, dout, lse, R, N, H, dqkv, scale=None):
    """Backward of attention_cls_train (yv_attention_cls_bwd): dout (R, H*64) bf16 compact, lse from the forward; writes every
    element of rows [0, R*N) of dqkv (R*N, 3*H*64) bf16: dK and dV of every key, dQ in the cls rows and zeros in the others."""
    _chk_dev(qkv, dout, lse, dqkv)
    _chk_rows(q)
    check(lib.yv_attention_cls_bwd(_p(q), q.stride(0), _p(qkv), _p(dout), _p(lse), R, N, H,
                                   float(64 ** -0.5 if scale is None else scale), _p(dqkv), _st()), "yv_attention_cls_bwd")
    return dqkv


def transpose_bf16(x: torch.Tensor, out_t: torch.Tensor, rows: Optional[int] = None):
    """x (rows, cols) bf16 -> out_t (cols, ld >= round64(rows)) with zero padding."""
    r = x.shape[0] if rows is None else rows
    check(lib.yv_transpose_bf16(_p(x), r, x.shape[1], x.stride(0), _p(out_t), out_t.stride(0), _st()), "yv_transpose_bf16")
    return out_t


def cast_weights(w: torch.Tensor, w_bf16: torch.Tensor, wt_bf16: torch.Tensor):
    N, K = w.shape
    check(lib.yv_cast_weights(_p(w), N, K, _p(w_bf16), _p(wt_bf16), wt_bf16.stride(0), _st()), "yv_cast_weights")


def colsum_ws_floats(rows: int, cols: int) -> int:
    return int(lib.yv_colsum_ws_floats(rows, cols))


def cast_colsum(x: torch.Tensor, y_bf16: Optional[torch.Tensor], colsum: Optional[torch.Tensor], ws: torch.Tensor,
                accumulate: bool = False):
    rows, cols = x.shape
    check(lib.yv_cast_colsum(_p(x), rows, cols, _p(y_bf16), _p(colsum), 1 if accumulate else 0, _p(ws), _st()),
          "yv_cast_colsum")


def colsum_bf16(x: torch.Tensor, colsum: torch.Tensor, ws: torch.Tensor, rows: Optional[int] = None,
                accumulate: bool = False):
    r = x.shape[0] if rows is None else rows
    check(lib.yv_colsum_bf16(_p(x), r, x.shape[1], x.stride(0), _p(colsum), 1 if accumulate else 0, _p(ws), _st()),
          "yv_colsum_bf16")


def layernorm_bwd(x, ldx, gamma, dy, lddy, rows, D, dx, lddx, dgamma, dbeta, ws, eps=1e-6):
    check(lib.yv_layernorm_bwd(_p(x), ldx, _p(gamma), _p(dy), lddy, rows, D, float(eps), _p(dx), lddx, _p(dgamma),
                               _p(dbeta), _p(ws), _st()), "yv_layernorm_bwd")


def token_reduce(dx, R, N, D, out):
    check(lib.yv_token_reduce(_p(dx), R, N, D, _p(out), _st()), "yv_token_reduce")


def head_bwd(feats, w1t, b1, w2, dlogits, R, nc, dw1, db1, dw2, db2, dfeats, ws):
    check(lib.yv_head_bwd(_p(feats), feats.stride(0), _p(w1t), _p(b1), _p(w2), _p(dlogits), R, nc, _p(dw1), _p(db1),
                          _p(dw2), _p(db2), _p(dfeats), dfeats.stride(0), _p(ws), _st()), "yv_head_bwd")


def wgrad(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, T: Optional[int] = None, tile_n: Optional[int] = None):
    """dw (N,K) f32 = dy[:T]^T @ x[:T]; dy (>=T,N), x (>=T,K) bf16, T a multiple of 64 with zero tail rows.
    tile_n: None = yv_wgrad (128 x 128 tiles); 128 / 64 / 32 = that N tile, 0 = the one wgrad_route picks (yv_wgrad_tiled)."""
    for t_ in (dy, x, dw):
        if not t_.is_cuda or t_.stride(-1) != 1:
            raise YvError("wgrad operands must be device tensors with unit column stride")
    t = dy.shape[0] if T is None else T
    if tile_n is None:
        check(lib.yv_wgrad(_p(dy), dy.stride(0), _p(x), x.stride(0), t, dy.shape[1], x.shape[1], _p(dw), dw.stride(0), _st()),
              "yv_wgrad")
    else:
        check(lib.yv_wgrad_tiled(_p(dy), dy.stride(0), _p(x), x.stride(0), t, dy.shape[1], x.shape[1], _p(dw), dw.stride(0),
                                 int(tile_n), _st()), "yv_wgrad_tiled")
    return dw


def wgrad_wide(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, T: Optional[int] = None, routed: bool = False):
    """wgrad on 256 (n) x 128 (k) output tiles (yv_wgrad_wide); operands as wgrad takes them.  routed=False: always the wide tile;
    routed=True: the wide tile where wgrad_wide_route picks it, otherwise exactly what wgrad launches."""
    for t_ in (dy, x, dw):
        if not t_.is_cuda or t_.stride(-1) != 1:
            raise YvError("wgrad operands must be device tensors with unit column stride")
    t = dy.shape[0] if T is None else T
    check(lib.yv_wgrad_wide(_p(dy), dy.stride(0), _p(x), x.stride(0), t, dy.shape[1], x.shape[1], _p(dw), dw.stride(0),
                            0 if routed else 1, _st()), "yv_wgrad_wide")
    return dw


def wgrad_conv3(dyp: torch.Tensor, xp: torch.Tensor, dw: torch.Tensor, T: int, pitch: int, tile_n: Optional[int] = None):
    """dw (N, 9*Cin) f32 = 3x3 / stride 1 weight gradient from operands over the zero-padded pixel grid (view_op VIEW_PAD):
    dyp (>=T, N) bf16 with zero ring / tail, xp (T, Cin) bf16 DENSE view inside a buffer that has pitch + 1 rows of finite
    values on both sides (see yv_wgrad_conv3).  tile_n as wgrad takes it (yv_wgrad_conv3_tiled)."""
    for t_ in (dyp, xp, dw):
        if not t_.is_cuda or t_.stride(-1) != 1:
            raise YvError("wgrad_conv3 operands must be device tensors with unit column stride")
    cin = xp.shape[1]
    if xp.stride(0) != cin or dw.shape[1] != 9 * cin:
        raise YvError("wgrad_conv3: xp must be dense (row stride Cin) and dw (N, 9*Cin)")
    if tile_n is None:
        check(lib.yv_wgrad_conv3(_p(dyp), dyp.stride(0), _p(xp), cin, pitch, T, dyp.shape[1], _p(dw), dw.stride(0), _st()),
              "yv_wgrad_conv3")
    else:
        check(lib.yv_wgrad_conv3_tiled(_p(dyp), dyp.stride(0), _p(xp), cin, pitch, T, dyp.shape[1], _p(dw), dw.stride(0),
                                       int(tile_n), _st()), "yv_wgrad_conv3_tiled")
    return dw


def wgrad_conv3_gather(dy: torch.Tensor, x: "yv_view", dw: torch.Tensor, B: int, Hin: int, Win: int, stride: int,
                       tile_n: Optional[int] = None):
    """dw (N, 9*Cin) f32 = 3x3 / pad 1 / stride 1 or 2 weight gradient with no operand copy (yv_wgrad_conv3_gather): dy
    (r64(B*Hout*Wout), N) bf16 with a zero tail, x the convolution's input (B, Hin, Win, Cin) as a view (mview), read in place.
    tile_n as wgrad takes it; the bits are those of im2col3 + wgrad(tile_n=...) on the same operands."""
    for t_ in (dy, dw):
        if not t_.is_cuda or t_.stride(-1) != 1:
            raise YvError("wgrad_conv3_gather operands must be device tensors with unit column stride")
    hout, wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    if dy.shape[0] < (B * hout * wout + 63) // 64 * 64 or dw.shape != (dy.shape[1], 9 * x.c) or x.up:
        raise YvError("wgrad_conv3_gather: dy must have r64(B*Hout*Wout) rows, dw be (N, 9*Cin) and x a plain view")
    check(lib.yv_wgrad_conv3_gather(_p(dy), dy.stride(0), x.ptr, x.ld, B, Hin, Win, stride, x.c, dy.shape[1], _p(dw), dw.stride(0),
                                    128 if tile_n is None else int(tile_n), _st()), "yv_wgrad_conv3_gather")
    return dw


def linear_nn(a: torch.Tensor, w_kn: torch.Tensor, out: torch.Tensor, flags: int = 0, aux: Optional[torch.Tensor] = None,
              M: Optional[int] = None):
    """out[M,N] = a[M,K] @ w_kn[K,N] (weight read reduction-major: dgrad on the master layout)."""
    _chk_dev(a, out, aux)
    Mr = a.shape[0] if M is None else M
    K, N = w_kn.shape
    check(lib.yv_linear_nn(_p(a), a.stride(0), _p(w_kn), w_kn.stride(0), None, Mr, N, K, _p(out), out.stride(0), flags,
                           _p(aux), 0 if aux is None else aux.stride(0), _st()), "yv_linear_nn")
    return out


# ------------------------------------------------------------- detector training (row C4)
VIEW_COPY, VIEW_ADD, VIEW_UP2, VIEW_UP2_BWD, VIEW_ZERO_INSERT, VIEW_ZERO, VIEW_PAD = 0, 1, 2, 3, 4, 5, 6


def blob_nhwc8(images: torch.Tensor, out: torch.Tensor):
    """(B,H,W,3) u8 -> (B,H,W,8) bf16 /255 with zero pad channels."""
    _chk_dev(images, out)
    check(lib.yv_blob_nhwc8(_p(images), images.numel() // 3, _p(out), _st()), "yv_blob_nhwc8")


def bn_ws_floats(T: int, Cn: int) -> int:
    return int(lib.yv_bn_ws_floats(T, Cn))


def bn_stats(z: "yv_view", T: int, mean, rstd, run_mean, run_var, ws, eps: float = 1e-3, momentum: float = 0.03):
    check(lib.yv_bn_stats(z.ptr, z.ld, T, z.c, eps, momentum, _p(mean), _p(rstd), _p(run_mean), _p(run_var), _p(ws),
                          ws.numel(), _st()), "yv_bn_stats")


def conv_stats_ws_floats(T: int, Cout: int) -> int:
    """Floats of conv_view_stats' `stats_ws` for T output rows (tile partials + what bn_stats_finish folds them into)."""
    return int(lib.yv_conv_stats_ws_floats(T, Cout))


def bn_stats_finish(stats_ws, T: int, mean, rstd, run_mean, run_var, eps: float = 1e-3, momentum: float = 0.03):
    """bn_stats' second half on the tile partials conv_view_stats left in `stats_ws` (C = mean.numel())."""
    check(lib.yv_bn_stats_finish(_p(stats_ws), T, mean.numel(), eps, momentum, _p(mean), _p(rstd), _p(run_mean), _p(run_var),
                                 _st()), "yv_bn_stats_finish")


def bn_act_fwd(z: "yv_view", T: int, mean, rstd, gamma, beta, out: "yv_view", res: Optional["yv_view"] = None, act: int = 1):
    check(lib.yv_bn_act_fwd(z.ptr, z.ld, T, z.c, _p(mean), _p(rstd), _p(gamma), _p(beta), res.ptr if res else None,
                            res.ld if res else 0, out.ptr, out.ld, act, _st()), "yv_bn_act_fwd")


def bn_act_bwd(da: "yv_view", z: "yv_view", T: int, mean, rstd, gamma, beta, dgamma, dbeta, dz: "yv_view", ws,
               act: int = 1, batch_stats: bool = True):
    check(lib.yv_bn_act_bwd(da.ptr, da.ld, z.ptr, z.ld, T, z.c, _p(mean), _p(rstd), _p(gamma), _p(beta), act,
                            1 if batch_stats else 0, _p(dgamma), _p(dbeta), dz.ptr, dz.ld, _p(ws), ws.numel(), _st()),
          "yv_bn_act_bwd")


def view_op(mode: int, src: Optional["yv_view"], dst: "yv_view", B: int, H: int, W: int, Cn: Optional[int] = None):
    """H, W are the dims of the SMALLER grid for the up / zero-insert modes (see include/yv_hip.h)."""
    check(lib.yv_view_op(mode, src.ptr if src is not None else None, src.ld if src is not None else 0, dst.ptr, dst.ld, B, H,
                         W, Cn if Cn is not None else dst.c, _st()), "yv_view_op")


_POOL_WS = {}


def maxpool5_bwd(x: "yv_view", dout: "yv_view", din: "yv_view", B: int, H: int, W: int):
    need = B * H * W * x.c
    dev = torch.cuda.current_device()
    ws = _POOL_WS.get(dev)
    if ws is None or ws.numel() < need:
        ws = _POOL_WS[dev] = torch.empty(need, dtype=torch.uint8, device=f"cuda:{dev}")
    check(lib.yv_maxpool5_bwd(x.ptr, x.ld, dout.ptr, dout.ld, din.ptr, din.ld, B, H, W, x.c, _p(ws), ws.numel(), _st()),
          "yv_maxpool5_bwd")


def im2col3(x: "yv_view", B: int, Hin: int, Win: int, stride: int, col: torch.Tensor):
    check(lib.yv_im2col3(x.ptr, x.ld, B, Hin, Win, x.c, stride, _p(col), _st()), "yv_im2col3")


def conv_weight_dgrad(w: torch.Tensor, Cout: int, taps: int, Cin: int, wd: torch.Tensor):
    _chk_dev(w, wd)
    check(lib.yv_conv_weight_dgrad(_p(w), Cout, taps, Cin, _p(wd), _st()), "yv_conv_weight_dgrad")


def conv_view(in0: "yv_view", B: int, Hout: int, Wout: int, ksize: int, stride: int, weight: torch.Tensor, Cout: int,
              out: "yv_view", flags: int = 0, res: Optional["yv_view"] = None, bias: Optional[torch.Tensor] = None,
              out_f32: bool = False):
    """yv_conv2d on views: out (B,Hout,Wout) rows of `out.ld` elements (bf16, or f32 with out_f32); optional bias and
    bf16 residual view (EPI_RES_BF16 accumulates gradients into a slice)."""
    if bias is not None:
        flags |= EPI_BIAS
    if out_f32:
        flags |= EPI_OUT_F32
    if res is not None:
        flags |= EPI_RES_BF16
    ws = _conv_workspace(weight.device)
    check(lib.yv_conv2d_ws(C.byref(in0), None, B, Hout, Wout, ksize, stride, _p(weight), _p(bias), Cout, out.ptr, out.ld,
                           res.ptr if res is not None else None, res.ld if res is not None else 0, flags, _p(ws),
                           ws.numel() * 4, _st()), "yv_conv2d_ws")


def dgrad_s2_taps(py: int, px: int) -> List[Tuple[int, int, int]]:
    """The taps of parity phase (py, px) of a 3 x 3 / stride 2 / pad 1 data gradient, as (wd slot, dy, dx) in ascending slot
    order: dx[b, 2i + py, 2j + px, :] = sum over the list of wd[:, slot, :] @ dz[b, i + dy, j + dx, :] (zero past the last row /
    column), wd (Cin, 9, Cout) being conv_weight_dgrad's flipped weight.  Per axis parity 0 takes slot row 1 at displacement
    0; parity 1 takes slot row 0 at displacement 0 and slot row 2 at displacement + 1.  1 / 2 / 2 / 4 taps: yv_conv2d_dgrad_s2
    walks exactly this list."""
    axis = lambda p: ((0, 0), (2, 1)) if p else ((1, 0),)
    return [(3 * r + c, dy, dx) for r, dy in axis(py) for c, dx in axis(px)]


DgradS2Route = collections.namedtuple("DgradS2Route", "kernel ksteps staged tiles workgroups use")


def conv_dgrad_s2_route(B: int, Hin: int, Win: int, ksize: int, Cin: int, Cout: int, dz_ld: Optional[int] = None,
                        dx_ld: Optional[int] = None, res_ld: Optional[int] = None) -> DgradS2Route:
    """Route conv_dgrad_s2 takes for the data gradient of a ksize x ksize / stride 2 layer (B, Hin, Win, Cin) -> Cout under the
    current options (host only): see yv_conv2d_dgrad_s2_route in include/yv_hip.h.  kernel is a CONV_IGEMM_* / CONV_DMA_* code;
    dense rows and a residual of dx's stride by default (res_ld = 0: none); raises YvError where the entry rejects the layer;
    use = False: the route keeps this shape on zero insertion."""
    out = (C.c_int * 9)()
    dx_ld = Cin if dx_ld is None else dx_ld
    check(lib.yv_conv2d_dgrad_s2_route(B, Hin, Win, ksize, Cin, Cout, Cout if dz_ld is None else dz_ld, dx_ld,
                                       dx_ld if res_ld is None else res_ld, out), "yv_conv2d_dgrad_s2_route")
    return DgradS2Route(out[0], tuple(out[1:5]), bool(out[5]), out[6], out[7], bool(out[8]))


def conv_dgrad_s2(dz: "yv_view", B: int, Hout: int, Wout: int, wd: torch.Tensor, Cin: int, Cout: int, dx: "yv_view",
                  res: Optional["yv_view"] = None):
    """dx (B, 2*Hout, 2*Wout) view = [res +] data gradient of a 3 x 3 / stride 2 convolution at dz (B, Hout, Wout) with
    wd = conv_weight_dgrad(w), no zero-inserted copy: yv_conv2d_dgrad_s2.  res may be dx (accumulate into a slice)."""
    _chk_dev(wd)
    check(lib.yv_conv2d_dgrad_s2(C.byref(dz), B, Hout, Wout, _p(wd), Cin, Cout, dx.ptr, dx.ld,
                                 res.ptr if res is not None else None, res.ld if res is not None else 0, None, 0, _st()),
          "yv_conv2d_dgrad_s2")


def conv_view_stats(in0: "yv_view", B: int, Hout: int, Wout: int, ksize: int, stride: int, weight: torch.Tensor, Cout: int,
                    out: "yv_view", stats_ws: torch.Tensor, bias: Optional[torch.Tensor] = None, flags: int = 0):
    """conv_view (bf16 out, optional bias, nothing else) that also leaves the per-tile column sums of what it stored in
    `stats_ws` (f32, >= conv_stats_ws_floats(B*Hout*Wout, Cout) floats) for bn_stats_finish: yv_conv2d_stats."""
    if bias is not None:
        flags |= EPI_BIAS
    ws = _conv_workspace(weight.device)
    check(lib.yv_conv2d_stats(C.byref(in0), B, Hout, Wout, ksize, stride, _p(weight), _p(bias), Cout, out.ptr, out.ld, flags,
                              _p(stats_ws), stats_ws.numel(), _p(ws), ws.numel() * 4, _st()), "yv_conv2d_stats")


def conv_bnbwd_ws_floats(T: int, Cout: int) -> int:
    """Floats of conv_view_bnbwd's `stats_ws` for T output rows: conv_stats_ws_floats + the 2 * Cout coefficients of the apply pass."""
    return int(lib.yv_conv_bnbwd_ws_floats(T, Cout))


ConvBnBwdRoute = collections.namedtuple("ConvBnBwdRoute", "kernel staged tiles workgroups splitk use")


def conv_bnbwd_route(B: int, Hout: int, Wout: int, ksize: int, stride: int, Cin: int, Cout: int, in_ld: Optional[int] = None,
                     out_ld: Optional[int] = None, res_ld: Optional[int] = None, ldz: Optional[int] = None,
                     flags: Optional[int] = None, ws_bytes: int = CONV_WS_BYTES) -> ConvBnBwdRoute:
    """Route conv_view_bnbwd takes for this data gradient under the current options (host only): see yv_conv2d_bnbwd_route in
    include/yv_hip.h.  Dense rows, a residual of the output's stride (EPI_RES_BF16, as the trainer accumulates) and conv_view's
    split-K workspace by default; raises YvError where the entry rejects the call; use = False: keep conv_view + bn_act_bwd."""
    out = (C.c_int * 6)()
    out_ld = Cout if out_ld is None else out_ld
    check(lib.yv_conv2d_bnbwd_route(B, Hout, Wout, ksize, stride, Cin, Cin if in_ld is None else in_ld, Cout, out_ld,
                                    out_ld if res_ld is None else res_ld, Cout if ldz is None else ldz,
                                    EPI_RES_BF16 if flags is None else flags, ws_bytes, out), "yv_conv2d_bnbwd_route")
    return ConvBnBwdRoute(out[0], bool(out[1]), out[2], out[3], bool(out[4]), bool(out[5]))


def conv_view_bnbwd(in0: "yv_view", B: int, Hout: int, Wout: int, ksize: int, stride: int, weight: torch.Tensor, Cout: int,
                    out: "yv_view", z: "yv_view", mean, rstd, gamma, beta, stats_ws: torch.Tensor, act: int = 1,
                    res: Optional["yv_view"] = None, bias: Optional[torch.Tensor] = None, flags: int = 0):
    """conv_view (bf16 out, optional bias and bf16 residual) as the data gradient that writes the gradient of a BatchNorm block's
    output, leaving that block's backward sums per tile in `stats_ws` (f32, >= conv_bnbwd_ws_floats(B*Hout*Wout, Cout) floats)
    for bn_act_bwd_finish: yv_conv2d_bnbwd.  z, mean, rstd, gamma, beta, act: the producer's, as bn_act_bwd takes them."""
    if bias is not None:
        flags |= EPI_BIAS
    if res is not None:
        flags |= EPI_RES_BF16
    ws = _conv_workspace(weight.device)
    check(lib.yv_conv2d_bnbwd(C.byref(in0), B, Hout, Wout, ksize, stride, _p(weight), _p(bias), Cout, out.ptr, out.ld,
                              res.ptr if res is not None else None, res.ld if res is not None else 0, flags, z.ptr, z.ld,
                              _p(mean), _p(rstd), _p(gamma), _p(beta), act, _p(stats_ws), stats_ws.numel(), _p(ws), ws.numel() * 4,
                              _st()), "yv_conv2d_bnbwd")


def bn_act_bwd_finish(da: "yv_view", z: "yv_view", T: int, mean, rstd, gamma, beta, dgamma, dbeta, dz: "yv_view", stats_ws,
                      act: int = 1, batch_stats: bool = True):
    """bn_act_bwd's finaliser and apply pass on the tile partials conv_view_bnbwd left in `stats_ws`: yv_bn_act_bwd_finish."""
    if stats_ws.numel() < conv_bnbwd_ws_floats(T, z.c):
        raise YvError("yv_bn_act_bwd_finish: stats_ws is smaller than conv_bnbwd_ws_floats(T, C)")
    check(lib.yv_bn_act_bwd_finish(da.ptr, da.ld, z.ptr, z.ld, T, z.c, _p(mean), _p(rstd), _p(gamma), _p(beta), act,
                                   1 if batch_stats else 0, _p(dgamma), _p(dbeta), dz.ptr, dz.ld, _p(stats_ws), _st()),
          "yv_bn_act_bwd_finish")


def mview(t: torch.Tensor, c_off: int = 0, c: Optional[int] = None) -> "yv_view":
    """(rows, ld) or (B,H,W,ld) bf16/f32 tensor -> view of channels [c_off, c_off + c)."""
    assert t.is_cuda and t.is_contiguous()
    c = t.shape[-1] - c_off if c is None else c
    return yv_view(C.c_void_p(t.data_ptr() + t.element_size() * c_off), t.shape[-1], c, 0)


def detect_loss_ws_bytes(B: int, A: int, G: int) -> int:
    return int(lib.yv_detect_loss_ws_bytes(B, A, G))


def detect_loss(box, cls, dbox, dcls, B: int, size: int, nc: int, ncp: int, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                gt_counts: torch.Tensor, loss: torch.Tensor, ws: torch.Tensor, gains=(7.5, 0.5, 1.5)):
    """v8 detection loss + gradient; box/cls/dbox/dcls: lists of the three scales' (rows, 64) / (rows, ncp) f32 tensors."""
    _chk_dev(*box, *cls, *dbox, *dcls, gt_boxes, gt_labels, gt_counts, loss, ws)
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    G = gt_boxes.shape[1]
    assert gt_boxes.dtype == torch.float32 and gt_labels.dtype == torch.int32 and gt_counts.dtype == torch.int32
    check(lib.yv_detect_loss(arr(box), arr(cls), arr(dbox), arr(dcls), B, size, nc, ncp, _p(gt_boxes), _p(gt_labels),
                             _p(gt_counts), G, gains[0], gains[1], gains[2], _p(loss), _p(ws), ws.numel() * ws.element_size(),
                             _st()), "yv_detect_loss")


OPT_SGD_NESTEROV, OPT_ADAMW = 1, 2


def optim_step(kind: int, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor], lr: float, step: int,
               beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
               mirror: Optional[torch.Tensor] = None, scale_rec: Optional[torch.Tensor] = None):
    """torch.optim.SGD(nesterov=True) (kind 1) / torch.optim.AdamW (kind 2) on flat fp32 buffers; step counts from 1.
    scale_rec: the record of grad_clip_record in place of grad_scale (yv_optim_step_rec); None: yv_optim_step."""
    _chk_dev(p, g, m, v, mirror)
    if scale_rec is not None:
        _chk_rec(scale_rec, grad_scale)
        check(lib.yv_optim_step_rec(kind, _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                    float(weight_decay), _p(scale_rec), int(step), _p(mirror), _st()), "yv_optim_step_rec")
        return
    check(lib.yv_optim_step(kind, _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                            float(weight_decay), float(grad_scale), int(step), _p(mirror), _st()), "yv_optim_step")


def _chk_rec(rec: torch.Tensor, grad_scale: float = 1.0):
    """A clip record: four f32 on the device; it carries the gradient scale, so a grad_scale next to it is a mistake."""
    _chk_dev(rec)
    if rec.dtype != torch.float32 or rec.numel() != 4:
        raise YvError("a clip record is four float32 values")
    if float(grad_scale) != 1.0:
        raise YvError("scale_rec already holds grad_scale (grad_clip_record): pass one of the two")


def grad_clip_ws_bytes(n: int) -> int:
    return int(lib.yv_grad_clip_ws_bytes(int(n)))


def grad_clip_record(g: torch.Tensor, grad_scale: float, max_norm: float, ws: torch.Tensor, rec: torch.Tensor,
                     skipped: Optional[torch.Tensor] = None):
    """torch.nn.utils.clip_grad_norm_(max_norm) over the flat f32 gradient g, on the device: rec (4 f32) = sum of squares, norm of
    g * grad_scale, clip coefficient, grad_scale * coefficient; skipped (1 i32) counts the records whose norm is not finite.
    ws: grad_clip_ws_bytes(g.numel()) bytes.  The record goes to sgd_step / optim_step as scale_rec."""
    _chk_dev(g, ws, skipped)
    _chk_rec(rec)
    if g.dtype != torch.float32 or (skipped is not None and (skipped.dtype != torch.int32 or skipped.numel() != 1)):
        raise YvError("grad_clip_record: g is float32, skipped one int32")
    check(lib.yv_grad_clip_record(_p(g), g.numel(), float(grad_scale), float(max_norm), _p(ws), ws.numel() * ws.element_size(),
                                  _p(rec), _p(skipped), _st()), "yv_grad_clip_record")


def ema_update(ema: torch.Tensor, src: torch.Tensor, decay: float):
    _chk_dev(ema, src)
    check(lib.yv_ema_update(_p(ema), _p(src), ema.numel(), float(decay), _st()), "yv_ema_update")


def axpby(dst: torch.Tensor, src: torch.Tensor, a: float, b: float):
    _chk_dev(dst, src)
    check(lib.yv_axpby(_p(dst), _p(src), dst.numel(), float(a), float(b), _st()), "yv_axpby")


# ------------------------------------------------------------- MXFP8 linears (BASELINE configs[4])
def quant_mxfp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None):
    """x (rows, K) bf16 -> (q (rows, K) uint8 e4m3 bytes, scales (K/128, rows_pad, 4) uint8 E8M0, rows_pad = rows up to 256)."""
    _chk_dev(x, q, scales)
    rows, K = x.shape
    rp = (rows + 255) // 256 * 256
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device) if q is None else q
    scales = torch.zeros((K // 128, rp, 4), dtype=torch.uint8, device=x.device) if scales is None else scales
    check(lib.yv_quant_mxfp8(_p(x), x.stride(0), rows, K, _p(q), q.stride(0), _p(scales), scales.shape[1], _st()),
          "yv_quant_mxfp8")
    return q, scales


def linear_mxfp8(aq: torch.Tensor, a_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor,
                 bias: Optional[torch.Tensor], out: torch.Tensor, flags: int = 0, m_dev: Optional[torch.Tensor] = None,
                 m_mul: int = 1):
    """aq (M, K) e4m3 bytes, read with its row stride (a view of a wider buffer is fine); the other tensors contiguous."""
    _chk_rows(aq)
    _chk_dev(a_scale, wq, w_scale, bias, out, m_dev)
    M, K = aq.shape
    N = wq.shape[0]
    if bias is not None:
        flags |= EPI_BIAS
    hook = LINEAR_HOOK
    if hook is not None:
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_linear_mxfp8(_p(aq), aq.stride(0), _p(a_scale), a_scale.shape[1], _p(wq), _p(w_scale), w_scale.shape[1],
                              _p(bias), M, N, K, _p(out), out.stride(0), flags, _p(m_dev), m_mul, _st()), "yv_linear_mxfp8")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)
        hook(M, N, K, e0, e1)
    return out


# ------------------------------------------------------------- MXFP8 training (VitTrainer(dtype="mxfp8"))
def r128(n: int) -> int:
    return (n + 127) // 128 * 128


def _mx_shape_check(what: str, t: Optional[torch.Tensor], dtype, rows: int, cols: int, exact_cols: bool = False):
    """Host-side size check of a caller-provided buffer (the C ABI sees pointers and strides only): a 2-D tensor of `dtype`
    with at least `rows` rows and `cols` (exactly `cols` with exact_cols) columns."""
    if t is None:
        return
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] < rows or (t.shape[1] != cols if exact_cols else t.shape[1] < cols):
        raise YvError(f"{what}: expected {dtype} ({'>=' if rows else ''}{rows}, {'' if exact_cols else '>='}{cols}), "
                      f"got {t.dtype} {tuple(t.shape)}")


def _mx_scale_check(what: str, s: Optional[torch.Tensor], ksteps: int, rows: int):
    """K-step-major E8M0 scales: uint8 (ksteps, >= rows, 4), contiguous (the C ABI takes shape[1] as the padded row count)."""
    if s is None:
        return
    if s.dtype != torch.uint8 or s.dim() != 3 or s.shape[0] != ksteps or s.shape[1] < rows or s.shape[2] != 4 or \
            not s.is_contiguous():
        raise YvError(f"{what}: expected contiguous uint8 ({ksteps}, >={rows}, 4) scales, got {s.dtype} {tuple(s.shape)}")


def _mx_device_check(what: str, *ts):
    for t_ in ts:
        if t_ is not None and (not t_.is_cuda or t_.stride(-1) != 1):
            raise YvError(f"{what}: operands must be device tensors with unit column stride")


def quant_mxfp8_2d(x: torch.Tensor, q: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                   qt: Optional[torch.Tensor] = None, scales_t: Optional[torch.Tensor] = None, rows: Optional[int] = None,
                   row_form: bool = True, col_form: bool = True):
    """x (T, C) bf16 (unit column stride; any row stride) read once -> the row form (q (T, C) uint8, scales (C/128, T_pad', 4)),
    bytes and scales of quant_mxfp8(x), and / or the column form (qt (C, T_pad) uint8, scales_t (T_pad/128, C_pad, 4)), those of
    quant_mxfp8 applied to x^T zero-padded to T_pad = T rounded up to 128 (the column form's width: qt.shape[1]).
    Returns (q, scales, qt, scales_t) with None for a form not written."""
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise YvError("quant_mxfp8_2d: x must be a 2-D bf16 tensor")
    T = x.shape[0] if rows is None else rows
    Cc = x.shape[1]
    if T > x.shape[0] or T <= 0 or Cc % 128:
        raise YvError(f"quant_mxfp8_2d: {T} rows of a {tuple(x.shape)} tensor (C a multiple of 128)")
    dev = x.device
    if row_form:
        q = torch.empty((T, Cc), dtype=torch.uint8, device=dev) if q is None else q
        scales = torch.zeros((Cc // 128, r128(T), 4), dtype=torch.uint8, device=dev) if scales is None else scales
        _mx_shape_check("quant_mxfp8_2d row form", q, torch.uint8, T, Cc)
        _mx_scale_check("quant_mxfp8_2d row form", scales, Cc // 128, T)
    else:
        q = scales = None
    if col_form:
        qt = torch.empty((Cc, r128(T)), dtype=torch.uint8, device=dev) if qt is None else qt
        _mx_shape_check("quant_mxfp8_2d column form", qt, torch.uint8, Cc, r128(T))
        if qt.shape[1] % 128:
            raise YvError(f"quant_mxfp8_2d column form: width {qt.shape[1]} is not a multiple of 128")
        scales_t = torch.zeros((qt.shape[1] // 128, r128(Cc), 4), dtype=torch.uint8, device=dev) if scales_t is None else scales_t
        _mx_scale_check("quant_mxfp8_2d column form", scales_t, qt.shape[1] // 128, Cc)
    else:
        qt = scales_t = None
    _mx_device_check("quant_mxfp8_2d", x, q, scales, qt, scales_t)
    check(lib.yv_quant_mxfp8_2d(_p(x), x.stride(0), T, Cc, _p(q), 0 if q is None else q.stride(0), _p(scales),
                                0 if scales is None else scales.shape[1], _p(qt), 0 if qt is None else qt.stride(0), _p(scales_t),
                                0 if scales_t is None else scales_t.shape[1], 0 if qt is None else qt.shape[1], _st()),
          "yv_quant_mxfp8_2d")
    return q, scales, qt, scales_t


def linear_mxfp8_ex(aq: torch.Tensor, a_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor,
                    bias: Optional[torch.Tensor], out: torch.Tensor, flags: int = 0, res_f32: Optional[torch.Tensor] = None,
                    aux: Optional[torch.Tensor] = None, M: Optional[int] = None):
    """Training form of linear_mxfp8 (the MX counterpart of linear_ex): separate f32 residual source, saved pre-activation,
    GELU backward.  aq (>=M, K) / wq (N, K) e4m3 bytes with their K-step-major scales; out (>=M, >=N) bf16, or f32 with
    EPI_OUT_F32 / EPI_RES_F32; res_f32 f32 with the row stride of out; aux bf16 (>=M, >=N)."""
    if aq.dim() != 2 or wq.dim() != 2:
        raise YvError("linear_mxfp8_ex: aq and wq must be 2-D")
    Mr = aq.shape[0] if M is None else M
    K, N = aq.shape[1], wq.shape[0]
    if Mr > aq.shape[0] or Mr < 0:
        raise YvError(f"linear_mxfp8_ex: M = {Mr} rows of a {tuple(aq.shape)} operand")
    _mx_shape_check("linear_mxfp8_ex aq", aq, torch.uint8, Mr, K)
    _mx_shape_check("linear_mxfp8_ex wq", wq, torch.uint8, N, K, exact_cols=True)
    _mx_scale_check("linear_mxfp8_ex a_scale", a_scale, K // 128, Mr)
    _mx_scale_check("linear_mxfp8_ex w_scale", w_scale, K // 128, N)
    f32o = bool(flags & (EPI_OUT_F32 | EPI_RES_F32))
    _mx_shape_check("linear_mxfp8_ex out", out, torch.float32 if f32o else torch.bfloat16, Mr, N)
    _mx_shape_check("linear_mxfp8_ex res_f32", res_f32, torch.float32, Mr, N)
    _mx_shape_check("linear_mxfp8_ex aux", aux, torch.bfloat16, Mr, N)
    if res_f32 is not None and res_f32.stride(0) != out.stride(0):
        raise YvError("linear_mxfp8_ex: res_f32 must have the row stride of out")
    if bias is not None and (bias.dtype != torch.float32 or bias.dim() != 1 or bias.numel() < N):
        raise YvError(f"linear_mxfp8_ex: bias must be f32 with >= {N} entries")
    _mx_device_check("linear_mxfp8_ex", aq, a_scale, wq, w_scale, bias, out, res_f32, aux)
    if bias is not None:
        flags |= EPI_BIAS
    check(lib.yv_linear_mxfp8_ex(_p(aq), aq.stride(0), _p(a_scale), a_scale.shape[1], _p(wq), _p(w_scale), w_scale.shape[1],
                                 _p(bias), Mr, N, K, _p(out), out.stride(0), flags, _p(res_f32), _p(aux),
                                 0 if aux is None else aux.stride(0), _st()), "yv_linear_mxfp8_ex")
    return out


def linear_mxfp8_instance(M: int, N: int, K: int, flags: int = 0) -> int:
    """Kernel instance an MX linear launches for this shape (0: gemm_mx_kernel 128 x 128, 1: the persistent kernel)."""
    r = lib.yv_linear_mxfp8_instance(M, N, K, flags)
    check(min(r, 0), "yv_linear_mxfp8_instance")
    return r


STREAM_WS_BYTES = 16 * 1024 * 1024 * 4      # the split-K workspace _st() registers per stream (what linear_route assumes by default)
# linear_route: kernel families (yv_linear_route_t.kernel, include/yv_hip.h)
LIN_SKINNY, LIN_IGEMM, LIN_DMA, LIN_P8, LIN_P9, LIN_MX, LIN_MID, LIN_MX_MID = 0, 1, 2, 3, 4, 5, 6, 7
ROUTE_M_DEV = 0x40000000                     # linear_route flag: the launch passes a device row count
LinearRoute = collections.namedtuple("LinearRoute", "kernel tile_rows tile_cols f32out ext abl mx splitk staged grid")


def linear_route(M: int, N: int, K: int, flags: int = 0, lda: Optional[int] = None, ldo: Optional[int] = None,
                 res_f32: bool = False, ldaux: int = 0, mx: bool = False, ws_bytes: int = STREAM_WS_BYTES,
                 n_cu: int = 0, m_dev: bool = False) -> LinearRoute:
    """Route linear / linear_ex (mx: linear_mxfp8 / linear_mxfp8_ex) take for this shape under the current options (host only):
    see yv_linear_route in include/yv_hip.h.  `flags` as the C entry takes them (EPI_BIAS is NOT added); dense rows by
    default; m_dev: the launch passes a device row count; n_cu = 0: the current device's CU count (needs a GPU)."""
    out = (C.c_int * len(LinearRoute._fields))()
    check(lib.yv_linear_route(M, N, K, K if lda is None else lda, N if ldo is None else ldo, flags | (ROUTE_M_DEV if m_dev else 0),
                              int(res_f32), ldaux, int(mx),
                              ws_bytes, n_cu, out), "yv_linear_route")
    return LinearRoute(*out)


def linear_mxfp8_q_route(M: int, N: int, K: int, flags: int = 0, n_cu: int = 0, m_dev: bool = False) -> LinearRoute:
    """Route linear_mxfp8_q takes for this shape under the current options (host only; linear_route rejects its output form):
    see yv_linear_mxfp8_q_route in include/yv_hip.h.  `flags` within EPI_BIAS | EPI_GELU, as the C entry takes them."""
    out = (C.c_int * len(LinearRoute._fields))()
    check(lib.yv_linear_mxfp8_q_route(M, N, K, flags | (ROUTE_M_DEV if m_dev else 0), n_cu, out), "yv_linear_mxfp8_q_route")
    return LinearRoute(*out)


WgradRoute = collections.namedtuple("WgradRoute", "tile_n tile_k tiles slices workgroups")


def wgrad_route(T: int, N: int, K: int, tile_n: int = 0, ws_bytes: int = STREAM_WS_BYTES, n_cu: int = 256) -> WgradRoute:
    """Route wgrad / wgrad_conv3 (K = 9 * Cin) take for this shape and tile_n under the current options (host only): see
    yv_wgrad_route in include/yv_hip.h.  tile_n = 128 is what tile_n=None launches."""
    out = (C.c_int * len(WgradRoute._fields))()
    check(lib.yv_wgrad_route(T, N, K, tile_n, ws_bytes, n_cu, out), "yv_wgrad_route")
    return WgradRoute(*out)


def wgrad_wide_route(T: int, N: int, K: int, routed: bool = False, ws_bytes: int = STREAM_WS_BYTES, n_cu: int = 256) -> WgradRoute:
    """Route wgrad_wide takes for this shape under the current options (host only): see yv_wgrad_wide_route in
    include/yv_hip.h.  tile_n = 256 is the wide tile; routed=True may answer wgrad_route(T, N, K, 128)."""
    out = (C.c_int * len(WgradRoute._fields))()
    check(lib.yv_wgrad_wide_route(T, N, K, 0 if routed else 1, ws_bytes, n_cu, out), "yv_wgrad_wide_route")
    return WgradRoute(*out)


def wgrad_conv3_gather_route(B: int, Hin: int, Win: int, stride: int, Cin: int, N: int, tile_n: int = 0,
                             ws_bytes: int = STREAM_WS_BYTES, n_cu: int = 256) -> Tuple[WgradRoute, bool]:
    """(route, use) of wgrad_conv3_gather for this layer (host only): see yv_wgrad_conv3_gather_route in include/yv_hip.h.  The
    route is wgrad_route(r64(B*Hout*Wout), N, 9*Cin, tile_n); use is False where the gather form was measured slower than
    im2col3 + wgrad."""
    out, use = (C.c_int * len(WgradRoute._fields))(), C.c_int(0)
    check(lib.yv_wgrad_conv3_gather_route(B, Hin, Win, stride, Cin, N, tile_n, ws_bytes, n_cu, out, C.byref(use)),
          "yv_wgrad_conv3_gather_route")
    return WgradRoute(*out), bool(use.value)


def wgrad_conv3_gather_src(B: int, Hin: int, Win: int, stride: int, m: int, tap: int) -> int:
    """Input pixel index (b*Hin + iy)*Win + ix that tap (0..8) of output pixel m reads in wgrad_conv3_gather's kernels, -1 for
    zero (host only: the kernels' own index function, yv_wgrad_conv3_gather_src)."""
    pixel = C.c_longlong(0)
    check(lib.yv_wgrad_conv3_gather_src(B, Hin, Win, stride, m, tap, C.byref(pixel)), "yv_wgrad_conv3_gather_src")
    return int(pixel.value)


def wgrad_mxfp8(dyt: torch.Tensor, dy_scale: torch.Tensor, xt: torch.Tensor, x_scale: torch.Tensor, dw: torch.Tensor):
    """dw (N, K) f32 (any row stride) = dY^T . X over T_pad tokens from the column forms of quant_mxfp8_2d: dyt (N, T_pad),
    xt (K, T_pad) uint8 with their token-block scales (T_pad/128, >= N / K, 4)."""
    if dyt.dim() != 2 or xt.dim() != 2:
        raise YvError("wgrad_mxfp8: dyt and xt must be 2-D")
    N, K, Tp = dyt.shape[0], xt.shape[0], dyt.shape[1]
    _mx_shape_check("wgrad_mxfp8 dyt", dyt, torch.uint8, N, Tp, exact_cols=True)
    _mx_shape_check("wgrad_mxfp8 xt", xt, torch.uint8, K, Tp, exact_cols=True)
    _mx_scale_check("wgrad_mxfp8 dy_scale", dy_scale, Tp // 128, N)
    _mx_scale_check("wgrad_mxfp8 x_scale", x_scale, Tp // 128, K)
    if dw.dtype != torch.float32 or tuple(dw.shape) != (N, K):
        raise YvError(f"wgrad_mxfp8: dw must be f32 ({N}, {K}), got {dw.dtype} {tuple(dw.shape)}")
    _mx_device_check("wgrad_mxfp8", dyt, dy_scale, xt, x_scale, dw)
    check(lib.yv_wgrad_mxfp8(_p(dyt), dyt.stride(0), _p(dy_scale), dy_scale.shape[1], _p(xt), xt.stride(0), _p(x_scale),
                             x_scale.shape[1], Tp, N, K, _p(dw), dw.stride(0), _st()), "yv_wgrad_mxfp8")
    return dw


# ------------------------------------------------------------- MXFP8 convolutions (YoloEngine(dtype="mxfp8"))
def mx_map(B: int, H: int, W: int, C: int, device) -> tuple:
    """An MX map: e4m3 bytes (B,H,W,C) uint8 + E8M0 scales (B,H,W,C/32) uint8 (C a multiple of 32)."""
    assert C % 32 == 0
    return (torch.zeros((B, H, W, C), dtype=torch.uint8, device=device),
            torch.zeros((B, H, W, C // 32), dtype=torch.uint8, device=device))


def mx_view(m: tuple, c_off: int, c: int, up: int = 0) -> "yv_mx_view":
    """MX map (q, s) -> operand view of channels [c_off, c_off+c) (multiples of 32)."""
    q, s = m
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.is_cuda and q.is_contiguous() and s.is_contiguous()
    assert c_off % 32 == 0 and c % 32 == 0 and q.shape[-1] == 32 * s.shape[-1]
    return yv_mx_view(C.c_void_p(q.data_ptr() + c_off), C.c_void_p(s.data_ptr() + c_off // 32), q.shape[-1], c, up)


def quant_mxfp8_map(x: torch.Tensor, out: tuple, c_off: int = 0, c: Optional[int] = None, out_c_off: int = 0):
    """bf16 NHWC x, channels [c_off, c_off+c) -> channels [out_c_off, ...) of the MX map `out` (rule of quant_mxfp8)."""
    q, s = out
    _chk_dev(x, q, s)
    c = x.shape[-1] - c_off if c is None else c
    assert x.dtype == torch.bfloat16 and c_off % 8 == 0 and out_c_off % 32 == 0
    pixels = x.numel() // x.shape[-1]
    assert q.numel() // q.shape[-1] == pixels
    check(lib.yv_quant_mxfp8_map(C.c_void_p(x.data_ptr() + 2 * c_off), x.shape[-1], pixels, c,
                                 C.c_void_p(q.data_ptr() + out_c_off), q.shape[-1], C.c_void_p(s.data_ptr() + out_c_off // 32),
                                 _st()), "yv_quant_mxfp8_map")
    return out


def pad_k128(w: torch.Tensor) -> torch.Tensor:
    """(Cout, K) -> (Cout, Kpad) with K zero-padded to a multiple of 128 (the MX convolution's weight depth)."""
    K = w.shape[1]
    kp = (K + 127) // 128 * 128
    return w if kp == K else torch.cat([w, w.new_zeros(w.shape[0], kp - K)], 1).contiguous()


def quant_conv_weight_mxfp8(w: torch.Tensor):
    """Convolution weight (Cout, k*k*Cin) bf16, K order (ky,kx,cin) -> (wq (Cout, Kpad) e4m3, scales (Kpad/128, rows_pad, 4))."""
    return quant_mxfp8(pad_k128(w.to(torch.bfloat16)).contiguous())


def conv2d_mxfp8(in0: "yv_mx_view", in1: Optional["yv_mx_view"], B: int, Hout: int, Wout: int, ksize: int, stride: int,
                 wq: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                 out_c_off: int = 0, flags: int = 0, res: Optional[torch.Tensor] = None, res_c_off: int = 0,
                 out_mx: Optional[tuple] = None, outq_c_off: int = 0):
    """MXFP8 conv2d + bias (+SiLU, + bf16 residual): writes the bf16 (f32 with EPI_OUT_F32) view of `out` at channel offset
    out_c_off and / or the MX map `out_mx` at channel offset outq_c_off (the bf16-rounded result, quantised)."""
    _chk_dev(wq, wscale, bias, out, res)
    Cout = wq.shape[0]
    if bias is not None:
        flags |= EPI_BIAS
    esz = 4 if (flags & EPI_OUT_F32) else 2
    optr = None if out is None else C.c_void_p(out.data_ptr() + esz * out_c_off)
    rptr = None if res is None else C.c_void_p(res.data_ptr() + 2 * res_c_off)
    qptr = sptr = None
    qld = 0
    if out_mx is not None:
        q, s = out_mx
        _chk_dev(q, s)
        assert outq_c_off % 32 == 0
        qptr, sptr, qld = C.c_void_p(q.data_ptr() + outq_c_off), C.c_void_p(s.data_ptr() + outq_c_off // 32), q.shape[-1]
    check(lib.yv_conv2d_mxfp8(C.byref(in0), C.byref(in1) if in1 is not None else None, B, Hout, Wout, ksize, stride,
                              _p(wq), _p(wscale), wscale.shape[1], _p(bias), Cout, optr, 0 if out is None else out.shape[-1],
                              qptr, sptr, qld, rptr, 0 if res is None else res.shape[-1], flags, _st()), "yv_conv2d_mxfp8")
    return out


def conv2d_mxfp8_instance(B: int, Hout: int, Wout: int, ksize: int, stride: int, Cin: int, Cout: int) -> int:
    """Kernel instance yv_conv2d_mxfp8 launches for this shape (0: 128 x 64 tiles, 1: 128 x 128 tiles)."""
    r = lib.yv_conv2d_mxfp8_instance(B, Hout, Wout, ksize, stride, Cin, Cout)
    check(min(r, 0), "yv_conv2d_mxfp8_instance")
    return r


def layernorm_mxfp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, rows: int,
                    D: int, ldx: int, eps: float = 1e-6, count_dev: Optional[torch.Tensor] = None, rows_per_count: int = 1):
    """LayerNorm -> MXFP8 operand (q (rows, D) e4m3 bytes, scales (D/128, rows_pad, 4) E8M0) in one pass."""
    check(lib.yv_layernorm_mxfp8(_p(x), ldx, _p(gamma), _p(beta), rows, D, float(eps), _p(q), q.stride(0), _p(scales),
                                 scales.shape[1], _p(count_dev), rows_per_count, _st()), "yv_layernorm_mxfp8")


def linear_mxfp8_q(aq: torch.Tensor, a_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor,
                   bias: Optional[torch.Tensor], out_q: torch.Tensor, out_scale: torch.Tensor, flags: int = 0,
                   m_dev: Optional[torch.Tensor] = None, m_mul: int = 1):
    """MXFP8 linear whose output is again an MXFP8 operand (bias / GELU -> bf16 rounding -> e4m3 + E8M0).  aq is read with its
    row stride, as in linear_mxfp8."""
    _chk_rows(aq)
    _chk_dev(a_scale, wq, w_scale, bias, out_q, out_scale, m_dev)
    M, K = aq.shape
    N = wq.shape[0]
    if bias is not None:
        flags |= EPI_BIAS
    hook = LINEAR_HOOK
    if hook is not None:
        e0, e1 = _timing_event(), _timing_event()
        check(lib.yv_set_launch_timing(e0.handle, e1.handle), "yv_set_launch_timing")
    check(lib.yv_linear_mxfp8_q(_p(aq), aq.stride(0), _p(a_scale), a_scale.shape[1], _p(wq), _p(w_scale), w_scale.shape[1],
                                _p(bias), M, N, K, flags, _p(m_dev), m_mul, _p(out_q), out_q.stride(0), _p(out_scale),
                                out_scale.shape[1], _st()), "yv_linear_mxfp8_q")
    if hook is not None:
        lib.yv_set_launch_timing(None, None)
        hook(M, N, K, e0, e1)


def attention_mxfp8(qkv: torch.Tensor, R: int, N: int, H: int, out_q: torch.Tensor, out_scale: torch.Tensor,
                    scale: Optional[float] = None, r_dev: Optional[torch.Tensor] = None):
    _chk_dev(qkv, out_q, out_scale, r_dev)
    check(lib.yv_attention_mxfp8(_p(qkv), R, N, H, float(64 ** -0.5 if scale is None else scale), _p(out_q), out_q.stride(0),
                                 _p(out_scale), out_scale.shape[1], _p(r_dev), _st()), "yv_attention_mxfp8")


def attention_fp8(qkv_q: torch.Tensor, qkv_scale: torch.Tensor, R: int, N: int, H: int, out: Optional[torch.Tensor] = None,
                  scale: Optional[float] = None, r_dev: Optional[torch.Tensor] = None, out_q: Optional[torch.Tensor] = None,
                  out_scale: Optional[torch.Tensor] = None):
    """attention_long on an MXFP8 qkv operand (yv_attention_fp8; any N >= 1, inference only): qkv_q (>= R*N, 3*H*64) e4m3 bytes read
    with its row stride, qkv_scale (3*H*64 // 128, rows_pad, 4) E8M0 - what linear_mxfp8_q(flags=0) writes for the qkv product.  QK^T
    runs on the block-scaled FP8 MFMA, V is dequantised to bf16 in the kernel, P stays bf16.  Outputs as attention_long: out
    (R*N, H*64) bf16 and / or the proj operand out_q / out_scale; r_dev: crop count."""
    _chk_rows(qkv_q)
    _chk_dev(qkv_scale, out, r_dev, out_q, out_scale)
    if (out_q is None) != (out_scale is None):
        raise YvError("attention_fp8: out_q and out_scale come together")
    if out is None and out_q is None:
        raise YvError("attention_fp8: one of out / out_q is required")
    if H <= 0 or H % 2:
        raise YvError("attention_fp8: the MXFP8 qkv operand has whole 128-column K steps per tensor (H even)")
    _mx_shape_check("attention_fp8 qkv_q", qkv_q, torch.uint8, R * N, 3 * H * 64)
    _mx_scale_check("attention_fp8 qkv_scale", qkv_scale, 3 * H * 64 // 128, R * N)
    _mx_shape_check("attention_fp8 out", out, torch.bfloat16, R * N, H * 64, exact_cols=True)
    _mx_shape_check("attention_fp8 out_q", out_q, torch.uint8, R * N, H * 64)
    _mx_scale_check("attention_fp8 out_scale", out_scale, H * 64 // 128, R * N)
    check(lib.yv_attention_fp8(_p(qkv_q), qkv_q.stride(0), _p(qkv_scale), qkv_scale.shape[1], R, N, H,
                               float(64 ** -0.5 if scale is None else scale), _p(out), _p(r_dev), _p(out_q),
                               0 if out_q is None else out_q.stride(0), _p(out_scale),
                               0 if out_scale is None else out_scale.shape[1], _st()), "yv_attention_fp8")
    return out


def mx_probe32(a: torch.Tensor, b: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, opsel: int = 0) -> torch.Tensor:
    """ONE v_mfma_scale_f32_32x32x64_f8f6f4 on register images (yv_mx_probe32): a, b (64, 32) uint8, sa, sb (64,) int32 -> (64, 16)
    f32, lane-major."""
    _chk_dev(a, b, sa, sb)
    for t, shape, dt in ((a, (64, 32), torch.uint8), (b, (64, 32), torch.uint8), (sa, (64,), torch.int32), (sb, (64,), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt:
            raise YvError(f"mx_probe32: expected {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    d = torch.zeros((64, 16), dtype=torch.float32, device=a.device)
    check(lib.yv_mx_probe32(_p(a), _p(b), _p(sa), _p(sb), int(opsel), _p(d), _st()), "yv_mx_probe32")
    return d


def attention_fp8_dequant(q: torch.Tensor, scale_byte: int) -> torch.Tensor:
    """The V dequantisation of attention_fp8 on its own (yv_attention_fp8_dequant): e4m3 bytes at one E8M0 scale byte -> bf16."""
    _chk_dev(q)
    if q.dtype != torch.uint8:
        raise YvError("attention_fp8_dequant: expected uint8 bytes")
    out = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
    check(lib.yv_attention_fp8_dequant(_p(q), q.numel(), int(scale_byte), _p(out), _st()), "yv_attention_fp8_dequant")
    return out
