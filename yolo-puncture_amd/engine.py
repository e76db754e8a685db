"""ctypes binding of libyolop.so (include/yolop.h). Tensors in / tensors out; PyTorch is only the owner of device
memory and streams. There is NO fallback: if the HIP library is missing or no GPU is present, calls raise.

Replaces what `ultralytics.YOLO(path)` builds and what `.predict` runs (reference yolo_seg/app.py:45,91).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .weights import fold_state

_LIB: Optional[C.CDLL] = None
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YOLOP_LIB") or os.path.join(_HERE, "libyolop.so")     # YOLOP_LIB: another build of the same ABI (A/B runs)

YP_BF16, YP_F32 = 0, 1
TASK_DETECT, TASK_SEGMENT = 0, 1
OP_KINDS = {0: "stem", 1: "conv", 2: "dwconv", 3: "pool5", 4: "upsample", 5: "attn", 6: "head", 7: "convT", 8: "pool3", 9: "amax"}
FORMS = ("plain", "dwpw", "dwpw_tail", "s2pw", "frontend", "c2f", "scdown", "pwsp", "cls_out")   # enum Form of csrc/common.h


class ModelDesc(C.Structure):
    _fields_ = [("variant", C.c_int), ("nc", C.c_int), ("task", C.c_int), ("dtype", C.c_int), ("max_det", C.c_int), ("family", C.c_int)]


class YolopError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libyolop.so and declare the prototypes of include/yolop.h. Raises if it was not built."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.isfile(p):
        raise YolopError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path.")
    lib = C.CDLL(p)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    lib.yp_last_error.restype = C.c_char_p
    lib.yp_create.argtypes = [C.POINTER(ModelDesc), C.c_int, C.POINTER(vp)]
    lib.yp_destroy.argtypes = [vp]
    lib.yp_weight_count.argtypes = [vp]
    lib.yp_weight_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), ip]
    lib.yp_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), C.c_int]
    lib.yp_finalize.argtypes = [vp]
    lib.yp_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.yp_proto.argtypes = [vp, C.POINTER(vp), ip, ip]
    lib.yp_masks.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.yp_id_mask_resized.argtypes = [vp, C.c_int, vp, vp] + [C.c_int] * 5 + [vp, vp, C.c_int, C.c_int, vp]
    lib.yp_id_mask_resized.restype = C.c_int
    lib.yp_mask_contours.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.yp_mask_contours.restype = C.c_int
    lib.yp_mask_contours_scaled.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp]
    lib.yp_mask_contours_scaled.restype = C.c_int
    lib.yp_mask_contours_large_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.yp_mask_contours_large_workspace.restype = C.c_size_t
    lib.yp_mask_contours_large.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp,
                                           C.c_size_t, vp]
    lib.yp_mask_contours_large.restype = C.c_int
    lib.yp_mask_contours_merge_workspace.argtypes = [C.c_int, C.c_int]
    lib.yp_mask_contours_merge_workspace.restype = C.c_size_t
    lib.yp_mask_contours_merge_tiles.argtypes = [C.POINTER(C.c_int32), C.c_int]
    lib.yp_mask_contours_merge_tiles.restype = C.c_ulonglong
    lib.yp_mask_contours_merge.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_size_t, vp]
    lib.yp_mask_contours_merge.restype = C.c_int
    lib.yp_mask_contours_merge_sizes.argtypes = [ip, ip]
    lib.yp_mask_contours_merge_sizes.restype = None
    lib.yp_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.yp_max_batch.argtypes = [vp, C.c_int, C.c_int]
    lib.yp_max_batch.restype = C.c_int
    lib.yp_debug_topk_anchors.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.c_int, vp, vp, vp]
    lib.yp_debug_topk_anchors.restype = C.c_int
    lib.yp_debug_attention.argtypes = [vp, vp] + [C.c_int] * 11 + [ip, vp]
    lib.yp_debug_attention.restype = C.c_int
    lib.yp_debug_attention_form.argtypes = [vp, vp] + [C.c_int] * 12 + [ip, vp]
    lib.yp_debug_attention_form.restype = C.c_int
    lib.yp_debug_conv_s2.argtypes = [vp, vp, vp, vp, vp] + [C.c_int] * 9 + [C.POINTER(C.c_int64), C.c_char_p, C.c_int, vp]
    lib.yp_debug_conv_s2.restype = C.c_int
    lib.yp_set_attention_form.argtypes = [vp, C.c_int]
    lib.yp_set_attention_form.restype = C.c_int
    lib.yp_debug_attention_f32.argtypes = [vp, vp] + [C.c_int] * 11 + [ip, vp]
    lib.yp_debug_attention_f32.restype = C.c_int
    lib.yp_set_attention_f32_stream.argtypes = [vp, C.c_int]
    lib.yp_set_attention_f32_stream.restype = C.c_int
    lib.yp_op_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.yp_op_output.argtypes = [vp, C.c_int, ip, ip, ip]
    lib.yp_op_kernel.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    lib.yp_op_fusion.argtypes = [vp, C.c_int, ip, ip]
    lib.yp_op_fusion.restype = C.c_int
    lib.yp_debug_op_form.argtypes = [vp, C.c_int, ip, ip, C.c_int]
    lib.yp_debug_op_form.restype = C.c_int
    lib.yp_run_op.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.yp_tensor_write.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.yp_tensor_count.argtypes = [vp]
    lib.yp_tensor_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, ip, ip]
    lib.yp_tensor_read.argtypes = [vp, C.c_int, vp]
    lib.yp_profile.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.yp_set_graph.argtypes = [vp, C.c_int]
    lib.yp_set_autotune.argtypes = [vp, C.c_int]
    lib.yp_set_nms.argtypes = [vp, C.c_float, C.c_float]
    lib.yp_set_nms.restype = C.c_int
    lib.yp_set_nms_options.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int]
    lib.yp_set_nms_options.restype = C.c_int
    lib.yp_debug_host_selftest.argtypes = [vp]
    lib.yp_debug_host_selftest.restype = C.c_int
    lib.yp_tuning_source.argtypes = [vp]
    lib.yp_tuning_source.restype = C.c_int
    lib.yp_debug_graph_info.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.yp_debug_graph_info.restype = C.c_int
    lib.yp_debug_head_positions.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.yp_debug_head_positions.restype = C.c_int
    lib.yp_debug_marker.argtypes = [vp]
    lib.yp_debug_marker.restype = C.c_int
    lib.yp_debug_force_conv_cfg.argtypes = [C.c_int]
    lib.yp_debug_op_cfg.argtypes = [vp, C.c_int, ip]
    lib.yp_debug_op_cfg.restype = C.c_int
    lib.yp_debug_last_store_form.argtypes = []
    lib.yp_debug_last_store_form.restype = C.c_int
    lib.yp_debug_max_workgroups.argtypes = [C.c_int]
    lib.yp_debug_max_workgroups.restype = C.c_int
    lib.yp_debug_conv_families.argtypes = [ip, ip, C.c_int]
    lib.yp_debug_conv_families.restype = C.c_int
    lib.yp_debug_ablation.argtypes = [C.c_int]
    lib.yp_debug_head_clocks.argtypes = [C.POINTER(C.c_uint64)]
    lib.yp_debug_head_branch_clocks.argtypes = [C.POINTER(C.c_uint64)]
    lib.yp_debug_contour_clocks.argtypes = [C.POINTER(C.c_uint64)]
    lib.yp_debug_pwsp_clocks.argtypes = [C.POINTER(C.c_uint64)]
    lib.yp_letterbox.argtypes = [vp, C.c_int, C.c_int, vp] + [C.c_int] * 7 + [vp]
    lib.yp_letterbox.restype = C.c_int
    lib.yp_letterbox_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp] + [C.c_int] * 7 + [vp]
    lib.yp_letterbox_batch.restype = C.c_int
    lib.yp_overlay_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]
    lib.yp_overlay_frames.restype = C.c_int
    lib.yp_masks_frames.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp, C.c_int, C.c_int, vp, vp]
    lib.yp_masks_frames.restype = C.c_int
    lib.yp_masks_frames_input.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp, C.c_int, C.c_int, vp, vp]
    lib.yp_masks_frames_input.restype = C.c_int
    lib.yp_id_masks_frames.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
    lib.yp_id_masks_frames.restype = C.c_int
    lib.yp_id_masks_frames_workspace.argtypes = [vp] + [C.c_int] * 6
    lib.yp_id_masks_frames_workspace.restype = C.c_size_t
    lib.yp_comm_unique_id.argtypes = [vp]
    lib.yp_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.yp_allgather.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.yp_comm_destroy.argtypes = [vp]
    for fn in ("yp_comm_unique_id", "yp_comm_create", "yp_allgather", "yp_comm_destroy"):
        getattr(lib, fn).restype = C.c_int
    for fn in ("yp_create", "yp_destroy", "yp_weight_count", "yp_weight_info", "yp_set_weight", "yp_finalize",
               "yp_forward", "yp_proto", "yp_masks", "yp_plan", "yp_op_info", "yp_op_output", "yp_op_input", "yp_tensor_count",
               "yp_tensor_info", "yp_tensor_read", "yp_profile", "yp_set_graph", "yp_run_op", "yp_tensor_write",
               "yp_op_kernel", "yp_set_autotune", "yp_debug_force_conv_cfg", "yp_debug_ablation"):
        getattr(lib, fn).restype = C.c_int
    if path is None:
        _LIB = lib
    return lib


EXPORTS = ["yp_last_error", "yp_create", "yp_destroy", "yp_weight_count", "yp_weight_info", "yp_set_weight",
           "yp_finalize", "yp_forward", "yp_proto", "yp_masks", "yp_id_mask_resized", "yp_plan", "yp_op_info", "yp_op_output", "yp_op_input", "yp_op_fusion",
           "yp_tensor_count", "yp_tensor_info", "yp_tensor_read", "yp_profile", "yp_set_graph", "yp_run_op",
           "yp_tensor_write", "yp_op_kernel", "yp_set_autotune", "yp_tuning_export", "yp_tuning_import", "yp_set_nms", "yp_set_nms_options", "yp_debug_force_conv_cfg", "yp_debug_op_cfg", "yp_debug_op_form", "yp_debug_last_store_form", "yp_debug_max_workgroups", "yp_debug_conv_families", "yp_debug_ablation", "yp_debug_head_clocks", "yp_debug_head_branch_clocks", "yp_debug_head_winners", "yp_debug_contour_clocks", "yp_debug_pwsp_clocks", "yp_debug_host_selftest", "yp_debug_graph_info", "yp_tuning_source", "yp_debug_head_positions", "yp_debug_marker", "yp_max_batch", "yp_debug_topk_anchors", "yp_debug_attention", "yp_debug_attention_form", "yp_debug_attention_f32", "yp_debug_conv_s2", "yp_set_attention_form", "yp_set_attention_f32_stream", "yp_letterbox", "yp_letterbox_batch", "yp_overlay_frames", "yp_masks_frames", "yp_masks_frames_input", "yp_id_masks_frames", "yp_id_masks_frames_workspace", "yp_mask_contours",
           "yp_mask_contours_scaled", "yp_mask_contours_large_workspace", "yp_mask_contours_large", "yp_mask_contours_merge_workspace",
           "yp_mask_contours_merge_tiles", "yp_mask_contours_merge", "yp_mask_contours_merge_sizes", "yp_comm_unique_id", "yp_comm_create", "yp_allgather", "yp_comm_destroy",
           "yp_u2net_create", "yp_u2net_destroy", "yp_u2net_weight_count", "yp_u2net_weight_info", "yp_u2net_set_weight", "yp_u2net_finalize",
           "yp_u2net_forward", "yp_u2net_forward_crops", "yp_u2net_set_graph", "yp_u2net_tensor_count", "yp_u2net_tensor_info", "yp_u2net_tensor_read",
           "yp_u2net_op_count", "yp_u2net_op_info",
           "yp_cls_create", "yp_cls_destroy", "yp_cls_weight_count", "yp_cls_weight_info", "yp_cls_set_weight", "yp_cls_finalize",
           "yp_cls_forward", "yp_cls_set_graph", "yp_cls_tensor_count", "yp_cls_tensor_info", "yp_cls_tensor_read"]


MAX_ANCHORS = 294912      # YP_MAX_ANCHORS
MAX_MASKS = 480           # YP_MAX_MASKS
ID_MASKS_FRAMES_BUDGET = 1 << 30      # YP_ID_MASKS_FRAMES_BUDGET: workspace bytes of one yp_id_masks_frames call before the facade splits a chunk
ATTENTION_FORMS = {"auto": 0, "stream": 1, "stream_wide": 3}      # yp_set_attention_form (bit 0: 32/64 streaming kernel, bit 1: 36/72)


ATTENTION_F32 = {"generic": 0, "stream": 1}      # yp_set_attention_f32_stream: a switch of its own beside the form
ATTENTION_F32_WIDE = {"stream_wide": 3}          # ... read as a bit set: bit 0 the 32/64 fp32 streaming kernel, bit 1 the 36/72 one (2 is no value)


def _attention_f32(value) -> int:
    if value in ATTENTION_F32:
        return ATTENTION_F32[value]
    if value in ATTENTION_F32_WIDE:
        return ATTENTION_F32_WIDE[value]
    raise ValueError(f"attention_f32 {value!r}: one of {sorted(ATTENTION_F32) + sorted(ATTENTION_F32_WIDE)}")


def _attention_form(form) -> int:
    if form not in ATTENTION_FORMS:
        raise ValueError(f"attention form {form!r}: one of {sorted(ATTENTION_FORMS)}")
    return ATTENTION_FORMS[form]


def topk_anchors(mk: List[torch.Tensor], hw, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Debug: stage 1 of the top-k head alone (yp_debug_topk_anchors) on caller-made class-max keys. mk[l]: device uint32-as-int32 [B, H_l * W_l]
    (bits of non-negative float scores), hw: three (H_l, W_l). Returns (winners int32 [B, 512] - anchor ids by rank in the first
    min(k, anchors) slots - and the threshold's score bits int32 [B]), on the device. Runs the kernels an engine takes for that anchor count."""
    lib = load_library()
    if len(mk) != 3 or len(hw) != 3:
        raise ValueError("three levels")
    B = int(mk[0].shape[0])
    dev = mk[0].device
    for t, (h, w) in zip(mk, hw):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev or tuple(t.shape) != (B, int(h) * int(w)):
            raise ValueError("mk[l] must be contiguous int32 [B, H_l * W_l] on one device")
    sel = torch.full((B, 512), -1, dtype=torch.int32, device=dev)
    thr = torch.zeros((B,), dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in mk])
    hwa = (C.c_int * 6)(*[int(v) for pair in hw for v in pair])
    rc = lib.yp_debug_topk_anchors(ptrs, B, hwa, int(k), C.c_void_p(sel.data_ptr()), C.c_void_p(thr.data_ptr()), C.c_void_p(_stream_ptr(dev)))
    if rc < 0:
        raise YolopError(lib.yp_last_error().decode())
    return sel, thr


def attention(qkv: torch.Tensor, nh: int, kd: int, hd: int, q_coff: int = 0, out: Optional[torch.Tensor] = None, o_coff: int = 0,
              wgs: int = 0, form: str = "auto") -> Tuple[torch.Tensor, int]:
    """Debug: the PSA attention core alone (yp_debug_attention_form) through the launcher an engine's attention op takes. qkv: device bf16 or
    float32 [B, N, q_stride], head h of a token at channels q_coff + h * (2 kd + hd) as q(kd) | k(kd) | v(hd). out: device [B, N, o_stride]
    of the same dtype (default: a new [B, N, nh * hd]); head h lands at channels o_coff + h * hd, nothing else is written. wgs > 0
    replaces the matrix-core kernels' workgroup target for this call. form "stream": bf16 calls with kd 32, hd 64 and more than 400 tokens
    take the streaming kernel; form "stream_wide": those too, and bf16 calls with kd 36, hd 72 take the wide-head streaming kernel at every token
    count. Returns (out, kernel): 3 the wide-head streaming kernel ran, 2 the streaming kernel, 1 the resident matrix-core kernel, 0 the generic one. Whatever the host check refuses raises YolopError before anything launches."""
    lib = load_library()
    if qkv.dim() != 3 or qkv.dtype not in (torch.bfloat16, torch.float32) or not qkv.is_contiguous() or not qkv.is_cuda:
        raise ValueError("qkv must be a contiguous device bf16 / float32 [B, N, q_stride]")
    B, N, q_stride = (int(v) for v in qkv.shape)
    if out is None:
        out = torch.empty((B, N, int(nh) * int(hd)), dtype=qkv.dtype, device=qkv.device)
    if out.dim() != 3 or out.dtype != qkv.dtype or not out.is_contiguous() or out.device != qkv.device or tuple(out.shape[:2]) != (B, N):
        raise ValueError("out must be a contiguous [B, N, o_stride] of qkv's dtype on its device")
    kernel = C.c_int(-1)
    rc = lib.yp_debug_attention_form(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), YP_BF16 if qkv.dtype == torch.bfloat16 else YP_F32, B, N,
                                int(nh), int(kd), int(hd), q_stride, int(q_coff), int(out.shape[2]), int(o_coff), int(wgs), _attention_form(form), C.byref(kernel),
                                C.c_void_p(_stream_ptr(qkv.device)))
    if rc < 0:
        raise YolopError(lib.yp_last_error().decode())
    return out, kernel.value


def attention_f32(qkv: torch.Tensor, nh: int, kd: int, hd: int, q_coff: int = 0, out: Optional[torch.Tensor] = None, o_coff: int = 0,
                  wgs: int = 0, f32: str = "generic") -> Tuple[torch.Tensor, int]:
    """Debug: `attention` on a float32 qkv under the fp32 switch (yp_debug_attention_f32). f32 "stream": calls with kd 32, hd 64 and more
    than 400 tokens take the fp32 streaming kernel, and wgs sets the query groups its workgroups walk; "stream_wide": those too, and calls
    with kd 36, hd 72 and more than 400 tokens take the wide-head fp32 streaming kernel; "generic": what `attention` does.
    Returns (out, kernel): 5 the wide-head fp32 streaming kernel ran, 4 the fp32 streaming kernel, 0 the generic one. Whatever the host
    check refuses raises YolopError before anything launches."""
    lib = load_library()
    if qkv.dim() != 3 or qkv.dtype != torch.float32 or not qkv.is_contiguous() or not qkv.is_cuda:
        raise ValueError("qkv must be a contiguous device float32 [B, N, q_stride]")
    B, N, q_stride = (int(v) for v in qkv.shape)
    if out is None:
        out = torch.empty((B, N, int(nh) * int(hd)), dtype=qkv.dtype, device=qkv.device)
    if out.dim() != 3 or out.dtype != qkv.dtype or not out.is_contiguous() or out.device != qkv.device or tuple(out.shape[:2]) != (B, N):
        raise ValueError("out must be a contiguous float32 [B, N, o_stride] on qkv's device")
    kernel = C.c_int(-1)
    rc = lib.yp_debug_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), B, N, int(nh), int(kd), int(hd), q_stride, int(q_coff),
                                    int(out.shape[2]), int(o_coff), int(wgs), _attention_f32(f32), C.byref(kernel), C.c_void_p(_stream_ptr(qkv.device)))
    if rc < 0:
        raise YolopError(lib.yp_last_error().decode())
    return out, kernel.value


def conv_s2(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, cfg: int, res: Optional[torch.Tensor] = None, out_f32: bool = False,
            silu: bool = True, lds_weights: bool = False) -> torch.Tensor:
    """Debug: one 3x3 / stride-2 / pad-1 bf16 conv alone (yp_debug_conv_s2) under configuration id `cfg` of the stride-2 halo family.
    x: device bf16 [B, H, W, Cin]; w: device bf16 [Cout, 3, 3, Cin]; bias: device float32 [Cout]; res: device bf16 [B, H/2, W/2, Cout] or None.
    lds_weights: keep the weights in LDS where the launcher would take the register-weights instance (ids 500 / 501, Cin 32 / 64).
    Returns y [B, H/2, W/2, Cout], float32 when out_f32, else bf16. A shape the id does not admit raises YolopError before anything launches."""
    lib = load_library()
    if x.dim() != 4 or w.dim() != 4 or x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or bias.dtype != torch.float32:
        raise ValueError("x: bf16 [B, H, W, Cin], w: bf16 [Cout, 3, 3, Cin], bias: float32 [Cout]")
    B, H, W, Cin = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    if tuple(w.shape) != (Cout, 3, 3, Cin) or tuple(bias.shape) != (Cout,) or not (x.is_cuda and w.is_cuda and bias.is_cuda):
        raise ValueError("w must be [Cout, 3, 3, Cin] and bias [Cout], all on the device")
    if not (x.is_contiguous() and w.is_contiguous() and bias.is_contiguous()):
        raise ValueError("contiguous tensors")
    if res is not None and (res.dtype != torch.bfloat16 or tuple(res.shape) != (B, H // 2, W // 2, Cout) or not res.is_contiguous() or res.device != x.device):
        raise ValueError("res must be a contiguous bf16 [B, H/2, W/2, Cout] on x's device")
    y = torch.zeros((B, H // 2, W // 2, Cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    rc = lib.yp_debug_conv_s2(C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(bias.data_ptr()),
                              C.c_void_p(res.data_ptr()) if res is not None else None, C.c_void_p(y.data_ptr()), int(bool(out_f32)), B, H, W, Cin, Cout,
                              int(bool(silu)), int(cfg), int(bool(lds_weights)), None, None, 0, C.c_void_p(_stream_ptr(x.device)))
    if rc < 0:
        raise YolopError(lib.yp_last_error().decode())
    return y


def conv_s2_admits(cfg: int, B: int, H: int, W: int, Cin: int, Cout: int, res: bool = False, out_f32: bool = False,
                   lds_weights: bool = False) -> Tuple[bool, int, str]:
    """Host only (yp_debug_conv_s2 without buffers): does id `cfg` of the stride-2 halo family admit the shape, the dynamic LDS bytes of its
    launch (0 when the id is not of the family) and the kernel symbol it would launch ("" when refused)."""
    lib = load_library()
    lds = C.c_int64(0)
    name = C.create_string_buffer(160)
    rc = lib.yp_debug_conv_s2(None, None, None, C.c_void_p(1) if res else None, None, int(bool(out_f32)), int(B), int(H), int(W), int(Cin), int(Cout),
                              1, int(cfg), int(bool(lds_weights)), C.byref(lds), name, 160, None)
    return rc >= 0, int(lds.value), name.value.decode()


def conv_families() -> List[Tuple[int, int]]:
    """(base, number of configurations) of every conv tile family: configuration ids [base, base + n), in the autotuner's order."""
    lib = load_library()
    n = lib.yp_debug_conv_families(None, None, 0)
    base, num = (C.c_int * n)(), (C.c_int * n)()
    lib.yp_debug_conv_families(base, num, n)
    return list(zip(base, num))


def _stream_ptr(device: torch.device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def letterbox_device(src: torch.Tensor, geo: dict, out: Optional[torch.Tensor] = None, pad_value: int = 114) -> torch.Tensor:
    """LetterBox on the GPU (yp_letterbox): `src` uint8 cuda [h0,w0,3], `geo` from hostops.letterbox_geometry ->
    uint8 cuda [out_h,out_w,3] (written into `out` when given, e.g. a row of the batch tensor)."""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 3 and src.is_contiguous()):
        raise ValueError("letterbox_device needs a contiguous uint8 CUDA tensor [H,W,3]")
    oh, ow = int(geo["out_h"]), int(geo["out_w"])
    if out is None:
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=src.device)
    if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (oh, ow, 3) and out.is_contiguous()):
        raise ValueError(f"letterbox_device: output must be a contiguous uint8 CUDA tensor [{oh},{ow},3]")
    lib = load_library()
    with torch.cuda.device(src.device):
        rc = lib.yp_letterbox(C.c_void_p(src.data_ptr()), int(src.shape[0]), int(src.shape[1]), C.c_void_p(out.data_ptr()), oh, ow,
                              int(geo["new_h"]), int(geo["new_w"]), int(geo["top"]), int(geo["left"]), int(pad_value),
                              C.c_void_p(_stream_ptr(src.device)))
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    return out


def letterbox_batch_device(frames: torch.Tensor, geo: dict, out: torch.Tensor, pad_value: int = 114) -> torch.Tensor:
    """yp_letterbox_batch: `frames` uint8 cuda [n,h0,w0,3] of one shape, `geo` from hostops.letterbox_geometry -> written into `out`
    uint8 cuda [n,out_h,out_w,3] in one launch (byte-equal to letterbox_device per frame)."""
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()):
        raise ValueError("letterbox_batch_device needs a contiguous uint8 CUDA tensor [n,H,W,3]")
    n = int(frames.shape[0])
    oh, ow = int(geo["out_h"]), int(geo["out_w"])
    if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, oh, ow, 3) and out.is_contiguous()):
        raise ValueError(f"letterbox_batch_device: output must be a contiguous uint8 CUDA tensor [{n},{oh},{ow},3]")
    if out.device != frames.device:
        raise ValueError(f"letterbox_batch_device: frames on {frames.device}, output on {out.device}")
    lib = load_library()
    with torch.cuda.device(frames.device):
        rc = lib.yp_letterbox_batch(C.c_void_p(frames.data_ptr()), n, int(frames.shape[1]), int(frames.shape[2]), C.c_void_p(out.data_ptr()),
                                    oh, ow, int(geo["new_h"]), int(geo["new_w"]), int(geo["top"]), int(geo["left"]), int(pad_value),
                                    C.c_void_p(_stream_ptr(frames.device)))
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    return out


CONTOUR_STRATEGIES = {"largest": 0, "all": 1}      # include/yolop.h YP_CONTOURS_*
_PARTS_CAP = 65                                     # [count | up to 64 contour lengths] (csrc/contour.hip CT_NLMAX)


def mask_contours_device(masks: torch.Tensor, max_pts: Optional[int] = None, want_rect: bool = True, strategy: str = "all", want_parts: bool = False,
                         orig_hw: Optional[Tuple[int, int]] = None):
    """yp_mask_contours: uint8 cuda [n,H,W] -> (list of int32 [m,2] numpy polygons (None where the device path declined), rect float64 [n,2]
    numpy (long side, short side) or None[, list of per-mask contour lengths when `want_parts`]). `strategy` as ultralytics' masks2segments:
    "all" (every external contour, concatenated bottom-up), "largest", or "all_merged" (the "all" list bridged at the closest points as the
    later 8.3.x releases do, hostops.merge_contours - traced and bridged on the device, yp_mask_contours_merge; with `want_parts` the third
    value is None per mask, except for a list the device bridge declined: that polygon comes unbridged with its contour lengths). The
    masks stay on the device; counts, contour lengths, rectangles
    and the heads of the point lists share one allocation so that a single mask (what the reference's loop asks for per frame) costs ONE
    device-to-host copy. `max_pts` also sizes the kernel's per-candidate lists (1024 points each behind the result): the default is
    generous for one mask, 16384 per mask otherwise.
    orig_hw = (H0, W0): masks at the letterboxed input size of an (H0, W0) frame (yp_mask_contours_scaled). The polygons are the same; each
    rectangle is of the polygon after hostops.scale_coords((H, W) -> orig_hw) and int32 truncation, (-1, -1) where the device declined it
    (W0 >= 2048)."""
    if not (masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3):
        raise ValueError("mask_contours_device needs a uint8 CUDA tensor [n,H,W]")
    if strategy not in CONTOUR_STRATEGIES and strategy != MERGED:
        raise ValueError(f"strategy must be 'all', 'largest' or 'all_merged', got {strategy!r}")
    if orig_hw is not None and not (int(orig_hw[0]) > 0 and int(orig_hw[1]) > 0):
        raise ValueError(f"orig_hw must be a positive (H0, W0), got {orig_hw!r}")
    masks = masks.contiguous()
    n, H, W = (int(v) for v in masks.shape)
    if max_pts is None:
        max_pts = 131072 if n <= 2 else 16384
    dev = masks.device
    if strategy == MERGED:
        h0, w0 = (int(orig_hw[0]), int(orig_hw[1])) if orig_hw is not None else (0, 0)

        def trace(lib, pts, count, parts, rect):
            args = (C.c_void_p(masks.data_ptr()), n, H, W, CONTOUR_STRATEGIES["all"], int(max_pts), pts, count, parts, _PARTS_CAP, rect)
            if orig_hw is None:
                return lib.yp_mask_contours(*args, C.c_void_p(_stream_ptr(dev)))
            return lib.yp_mask_contours_scaled(*args, h0, w0, C.c_void_p(_stream_ptr(dev)))
        return _trace_and_bridge(trace, dev, n, int(max_pts), _PARTS_CAP, want_rect, want_parts)
    # int32 words: [count (n) | pad | parts (n x _PARTS_CAP, padded to even) | rect (n x 2 float64) | points (n x max_pts x 2)]
    o_parts = (n + 1) // 2 * 2
    o_rect = o_parts + (n * _PARTS_CAP + 1) // 2 * 2
    o_pts = o_rect + 4 * n
    buf = torch.empty((o_pts + n * max_pts * 2,), dtype=torch.int32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        base = buf.data_ptr()
        args = (C.c_void_p(masks.data_ptr()), n, H, W, CONTOUR_STRATEGIES[strategy], int(max_pts), C.c_void_p(base + 4 * o_pts), C.c_void_p(base),
                C.c_void_p(base + 4 * o_parts), _PARTS_CAP, C.c_void_p(base + 4 * o_rect if want_rect else None))
        if orig_hw is None:
            rc = lib.yp_mask_contours(*args, C.c_void_p(_stream_ptr(dev)))
        else:
            rc = lib.yp_mask_contours_scaled(*args, int(orig_hw[0]), int(orig_hw[1]), C.c_void_p(_stream_ptr(dev)))
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    return _read_contours(buf, n, int(max_pts), _PARTS_CAP, o_parts, o_rect, o_pts, want_rect, want_parts)


class ContourList(list):
    """The polygons of one device contour call (a plain list to its users) with what a follow-up call on the declined ones needs:
    `max_pts`, the per-mask point capacity the call ran with."""
    max_pts: Optional[int] = None


def _read_contours(buf: torch.Tensor, n: int, max_pts: int, parts_cap: int, o_parts: int, o_rect: int, o_pts: int, want_rect: bool, want_parts: bool):
    """The host side of a contour call's one allocation ([count | parts | rect | points], int32 words): counts, contour lengths, rectangles
    and the heads of the point lists in ONE device-to-host copy for a single mask, two otherwise."""
    if n == 0:
        polys = ContourList()
        polys.max_pts = max_pts
        return (polys, (np.zeros((0, 2)) if want_rect else None), []) if want_parts else (polys, (np.zeros((0, 2)) if want_rect else None))
    head_pts = min(max_pts, 1024)
    if n == 1:
        h = buf[:o_pts + 2 * head_pts].cpu().numpy()
        c = h[:1]
        if c[0] > head_pts:
            host = buf[o_pts:o_pts + 2 * int(c[0])].cpu().numpy().reshape(1, -1, 2)
        else:
            host = h[o_pts:].reshape(1, -1, 2)
    else:
        h = buf[:o_pts].cpu().numpy()
        c = h[:n]
        top = int(max(1, c.max()))
        host = buf[o_pts:].view(n, max_pts, 2)[:, :top].cpu().numpy()
    rect = h[o_rect:o_rect + 4 * n].view(np.float64).reshape(n, 2).copy() if want_rect else None
    polys = ContourList(host[i, :c[i]].copy() if c[i] >= 0 else None for i in range(n))
    polys.max_pts = max_pts
    if not want_parts:
        return polys, rect
    pr = h[o_parts:o_parts + n * parts_cap].reshape(n, parts_cap)
    parts = [[int(v) for v in pr[i, 1:1 + min(int(pr[i, 0]), parts_cap - 1)]] if c[i] >= 0 else None for i in range(n)]
    return polys, rect, parts


MERGED = "all_merged"                               # hostops.POLYGON_STRATEGIES' third: the "all" list, bridged on the device (yp_mask_contours_merge)
MERGE_MAX_PTS = 1 << 19                             # include/yolop.h YP_CONTOURS_MERGE_MAX_PTS


def merge_sizes() -> Tuple[int, int]:
    """(tile, scan block) of yp_mask_contours_merge as the loaded library was built: points a side of a closest-pair tile, contours per
    step of the per-mask scans."""
    tile, scan = C.c_int(0), C.c_int(0)
    load_library().yp_mask_contours_merge_sizes(C.byref(tile), C.byref(scan))
    return int(tile.value), int(scan.value)


def merge_tiles(lengths) -> int:
    """yp_mask_contours_merge_tiles: work tiles the device derives for one mask whose contours have these lengths (host arithmetic)."""
    arr = (C.c_int32 * max(1, len(lengths)))(*[int(v) for v in lengths])
    return int(load_library().yp_mask_contours_merge_tiles(arr, len(lengths)))


def _merge_call(lib, dev, pts_ptr: int, count_ptr: int, parts_ptr: int, n: int, max_pts: int, parts_cap: int, out_ptr: int, out_count_ptr: int,
                out_cap: int) -> int:
    """yp_mask_contours_merge on the current stream of `dev`, its workspace allocated for the call (stream-ordered: free to go afterwards)."""
    ws_bytes = int(lib.yp_mask_contours_merge_workspace(n, parts_cap))
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.int32, device=dev)
    return lib.yp_mask_contours_merge(C.c_void_p(pts_ptr), C.c_void_p(count_ptr), C.c_void_p(parts_ptr), n, max_pts, parts_cap, C.c_void_p(out_ptr),
                                      C.c_void_p(out_count_ptr), out_cap, C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(_stream_ptr(dev)))


def contours_merge_device(pts: torch.Tensor, count: torch.Tensor, parts: torch.Tensor, out_cap: Optional[int] = None,
                          out: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None):
    """yp_mask_contours_merge on device tensors as the contour calls fill them: pts int32 [n,max_pts,2], count int32 [n], parts int32
    [n,parts_cap] ([0] = contours, then their lengths) -> (merged int32 [n,out_cap,2], merged_count int32 [n]) on the device:
    hostops.merge_contours of every mask's list; count <= 0 passed on, -1 where the bridge declines (more than `out_cap` points - default:
    room for every list the inputs can hold -, a parts row that does not list every contour). `out` / `out_count`: tensors to write into
    (int32, contiguous, [n,out_cap,2] and [n]) instead of fresh ones."""
    ok = all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (pts, count, parts))
    if not (ok and pts.dim() == 3 and pts.shape[2] == 2 and count.dim() == 1 and parts.dim() == 2 and pts.shape[0] == count.shape[0] == parts.shape[0]):
        raise ValueError("contours_merge_device needs contiguous int32 CUDA tensors pts [n,max_pts,2], count [n], parts [n,parts_cap]")
    n, max_pts, parts_cap = int(pts.shape[0]), int(pts.shape[1]), int(parts.shape[1])
    if out_cap is None:
        out_cap = max_pts + 2 * min(parts_cap - 1, max_pts)
    out_cap = int(out_cap)
    dev = pts.device
    if out is None:
        out = torch.empty((n, out_cap, 2), dtype=torch.int32, device=dev)
    if out_count is None:
        out_count = torch.empty((n,), dtype=torch.int32, device=dev)
    if not all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.device == dev for t in (out, out_count)) or \
            tuple(out.shape) != (n, out_cap, 2) or tuple(out_count.shape) != (n,):
        raise ValueError(f"contours_merge_device: out must be int32 [{n},{out_cap},2] and out_count int32 [{n}] on {dev}")
    lib = load_library()
    with torch.cuda.device(dev):
        rc = _merge_call(lib, dev, pts.data_ptr(), count.data_ptr(), parts.data_ptr(), n, max_pts, parts_cap, out.data_ptr(), out_count.data_ptr(), out_cap)
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    return out, out_count


def _trace_and_bridge(trace, dev, n: int, max_pts: int, parts_cap: int, want_rect: bool, want_parts: bool):
    """strategy "all_merged" of the two contour calls: `trace(lib, pts, count, parts, rect)` lists every contour ("all") into the tail of
    the call's one allocation, yp_mask_contours_merge bridges them into its head on the same stream - nothing is read back in between -
    and the head is read as for the other strategies. -> (polys, rect[, parts]): parts[i] is None where the device bridged (or the trace
    declined); where only the bridge declined, polys[i] is the unbridged list and parts[i] its contour lengths when `want_parts`
    (predictor._finish_contour bridges it), else it is bridged here."""
    from . import hostops
    if max_pts > MERGE_MAX_PTS:
        raise ValueError(f"'all_merged' on the device: max_pts <= {MERGE_MAX_PTS}, got {max_pts}")
    out_cap = max_pts + 2 * (parts_cap - 1)               # two more points per listable contour: every list the trace can write fits bridged
    # int32 words: [bridged count (n) | traced count (n) | parts | rect | bridged points (n x out_cap x 2) | traced points (n x max_pts x 2)]
    o_parts = 2 * n
    o_rect = o_parts + (n * parts_cap + 1) // 2 * 2
    o_pts = o_rect + 4 * n
    o_raw = o_pts + n * out_cap * 2
    buf = torch.empty((o_raw + n * max_pts * 2,), dtype=torch.int32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        base = buf.data_ptr()
        rc = trace(lib, C.c_void_p(base + 4 * o_raw), C.c_void_p(base + 4 * n), C.c_void_p(base + 4 * o_parts),
                   C.c_void_p(base + 4 * o_rect if want_rect else None))
        if rc == 0:
            rc = _merge_call(lib, dev, base + 4 * o_raw, base + 4 * n, base + 4 * o_parts, n, max_pts, parts_cap, base + 4 * o_pts, base, out_cap)
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    polys, rect = _read_contours(buf[:o_raw], n, out_cap, parts_cap, o_parts, o_rect, o_pts, want_rect, False)
    polys.max_pts = max_pts
    parts = [None] * n
    if any(p is None for p in polys):                   # which of them did the trace list? (a second, small copy: only when something declined)
        head = buf[n:o_rect].cpu().numpy()
        for i in range(n):
            row = head[o_parts - n + i * parts_cap:o_parts - n + (i + 1) * parts_cap]
            if polys[i] is not None or head[i] <= 0 or not 1 <= row[0] <= parts_cap - 1:
                continue
            raw = buf[o_raw + i * max_pts * 2:o_raw + (i * max_pts + int(head[i])) * 2].cpu().numpy().reshape(-1, 2)
            lens = [int(v) for v in row[1:1 + int(row[0])]]
            if want_parts:
                polys[i], parts[i] = raw, lens
            else:
                polys[i] = hostops.merge_contours(np.split(raw, np.cumsum(lens)[:-1])).astype(np.int32)
    return (polys, rect, parts) if want_parts else (polys, rect)


LARGE_MAX_DIM = 4096                                # include/yolop.h YP_CONTOURS_LARGE_MAX_DIM
_LARGE_MAX_BORDERS = 65536                          # ... YP_CONTOURS_LARGE_MAX_STARTS: a mask has at most as many outer borders
YP_CONTOURS_ONLY_DECLINED = 1


def mask_contours_large_device(masks: torch.Tensor, max_pts: Optional[int] = None, want_rect: bool = True, strategy: str = "all",
                               want_parts: bool = False, orig_hw: Optional[Tuple[int, int]] = None):
    """yp_mask_contours_large: arguments and return values of mask_contours_device, every mask through the large path (tables in a device
    workspace instead of LDS; csrc/contour_large.hip): masks up to 4096 x 4096, up to 65536 border starts and outer borders each, the
    scaled rectangle (`orig_hw`) for a frame of any width. `parts` lists every contour of the mask. None where it declines (more starts, or
    more than `max_pts` points); masks higher or wider than 4096 raise YolopError. The workspace lives for the call only."""
    if not (masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3):
        raise ValueError("mask_contours_large_device needs a uint8 CUDA tensor [n,H,W]")
    if strategy not in CONTOUR_STRATEGIES and strategy != MERGED:
        raise ValueError(f"strategy must be 'all', 'largest' or 'all_merged', got {strategy!r}")
    if orig_hw is not None and not (int(orig_hw[0]) > 0 and int(orig_hw[1]) > 0):
        raise ValueError(f"orig_hw must be a positive (H0, W0), got {orig_hw!r}")
    masks = masks.contiguous()
    n, H, W = (int(v) for v in masks.shape)
    if max_pts is None:
        max_pts = 131072 if n <= 2 else 16384
    max_pts = int(max_pts)
    dev = masks.device
    # parts rows: every length the mask can have (a contour has at least one point, so at most max_pts of them are ever listed)
    parts_cap = 1 + min(_LARGE_MAX_BORDERS, max_pts, max(1, H * ((W + 1) // 2))) if want_parts or strategy == MERGED else 2
    lib = load_library()
    ws_bytes = int(lib.yp_mask_contours_large_workspace(n, H, W))
    h0, w0 = (int(orig_hw[0]), int(orig_hw[1])) if orig_hw is not None else (0, 0)
    if strategy == MERGED:
        ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.int32, device=dev)

        def trace(lib, pts, count, parts, rect):
            return lib.yp_mask_contours_large(C.c_void_p(masks.data_ptr()), n, H, W, CONTOUR_STRATEGIES["all"], max_pts, pts, count, parts, parts_cap,
                                              rect, h0, w0, 0, C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(_stream_ptr(dev)))
        return _trace_and_bridge(trace, dev, n, max_pts, parts_cap, want_rect, want_parts)
    o_parts = (n + 1) // 2 * 2
    o_rect = o_parts + (n * parts_cap + 1) // 2 * 2
    o_pts = o_rect + 4 * n
    buf = torch.empty((o_pts + n * max_pts * 2,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        base = buf.data_ptr()
        rc = lib.yp_mask_contours_large(C.c_void_p(masks.data_ptr()), n, H, W, CONTOUR_STRATEGIES[strategy], max_pts, C.c_void_p(base + 4 * o_pts),
                                        C.c_void_p(base), C.c_void_p(base + 4 * o_parts if want_parts else None), parts_cap,
                                        C.c_void_p(base + 4 * o_rect if want_rect else None), h0, w0, 0, C.c_void_p(ws.data_ptr()), ws_bytes,
                                        C.c_void_p(_stream_ptr(dev)))
    if rc != 0:
        raise YolopError(lib.yp_last_error().decode())
    return _read_contours(buf, n, max_pts, parts_cap, o_parts, o_rect, o_pts, want_rect, want_parts)


class Engine:
    """One engine per GPU. `state` is an (unfused) ultralytics-layout state dict; see weights.py."""

    def __init__(self, variant: str = "s", nc: int = 80, seg: bool = False, dtype: str = "bf16",
                 device: int = 0, max_det: int = 300, state: Optional[Dict[str, torch.Tensor]] = None,
                 finalize: bool = True, family: str = "v10", attention: Optional[str] = None, attention_f32: Optional[str] = None):
        self.lib = load_library()
        self.variant, self.nc, self.seg, self.max_det = variant, nc, seg, max_det
        self.family = family
        if family != "v10" and not seg:
            raise ValueError("the v8 / 11 families are built as segmentation models (the checkpoints the reference ships)")
        self.dtype = {"bf16": YP_BF16, "fp32": YP_F32, "f32": YP_F32}[dtype]
        self.device_index = int(device)
        self._h = C.c_void_p()
        desc = ModelDesc(ord(variant), nc, TASK_SEGMENT if seg else TASK_DETECT, self.dtype, max_det, {"v10": 0, "v8": 8, "11": 11}[family])
        self._chk(self.lib.yp_create(C.byref(desc), self.device_index, C.byref(self._h)))
        self._keep: List[torch.Tensor] = []
        self.finalized = False
        if attention is not None:           # (None: what YOLOP_ATTN_FORM said when the engine was created, "auto" without it)
            self.set_attention_form(attention)
        if attention_f32 is not None:       # (None: what YOLOP_ATTN_F32 said when the engine was created, "generic" without it)
            self.set_attention_f32(attention_f32)
        if state is not None:
            self.load_state(state)
            if finalize:
                self.finalize()

    # -- errors ------------------------------------------------------------------------------------------------
    def _chk(self, rc: int) -> int:
        if rc < 0:
            raise YolopError(f"libyolop error {rc}: {self.lib.yp_last_error().decode()}")
        return rc

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.yp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -----------------------------------------------------------------------------------------------
    def expected_weights(self) -> List[Tuple[str, Tuple[int, ...]]]:
        out = []
        n = self._chk(self.lib.yp_weight_count(self._h))
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            self._chk(self.lib.yp_weight_info(self._h, i, name, 256, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[j]) for j in range(nd.value))))
        return out

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        """Fold Conv+BN (and merge RepVGGDW) on the host, hand every folded fp32 tensor to the engine."""
        folded = fold_state(state)
        for name, (w, b) in folded.items():
            for suffix, t in ((".weight", w), (".bias", b)):
                t = t.detach().to(torch.float32).contiguous().cpu()
                shp = (C.c_int64 * t.dim())(*t.shape)
                self._chk(self.lib.yp_set_weight(self._h, (name + suffix).encode(), C.c_void_p(t.data_ptr()), shp, t.dim()))

    def finalize(self) -> None:
        self._chk(self.lib.yp_finalize(self._h))
        self.finalized = True

    def set_attention_form(self, form: str) -> None:
        """"auto": the PSA block's resident matrix-core kernel up to 400 tokens, the generic kernel up to 2368, refusal beyond (the default).
        "stream": bf16 engines with 32-wide keys run attention_stream_kernel above 400 tokens, without a token bound. "stream_wide": that, and
        bf16 engines with 36-wide keys and 72-wide heads (YOLOv10-M) run attention_stream_wide_kernel at every token count. Drops the current plan."""
        self._chk(self.lib.yp_set_attention_form(self._h, _attention_form(form)))

    def set_attention_f32(self, value: str) -> None:
        """"generic": an fp32 engine's PSA block runs the generic kernel up to 2368 tokens and is refused beyond (the default). "stream": fp32
        engines with 32-wide keys and 64-wide heads run attention_stream_f32_kernel above 400 tokens, without a token bound; bf16 engines
        and YOLOv10-M are as before. "stream_wide": that, and fp32 engines with 36-wide keys and 72-wide heads (YOLOv10-M) run
        attention_stream_wide_f32_kernel above 400 tokens. Independent of set_attention_form. Drops the current plan."""
        self._chk(self.lib.yp_set_attention_f32_stream(self._h, _attention_f32(value)))

    def set_autotune(self, enable: bool) -> None:
        self._chk(self.lib.yp_set_autotune(self._h, 1 if enable else 0))

    def tuning_export(self) -> List[int]:
        """Tile configuration id per op of the current plan (after a forward): what `tuning_import` takes on another engine / rank."""
        n = self._chk(self.lib.yp_tuning_export(self._h, None, 0))
        buf = (C.c_int32 * n)()
        self._chk(self.lib.yp_tuning_export(self._h, buf, n))
        return list(buf)

    def tuning_import(self, B: int, H: int, W: int, cfgs) -> None:
        """Install another engine's tile configurations for shape (B,H,W): the next forward of that shape does not tune, and its bf16
        results equal the exporting engine's bit for bit (same build)."""
        cfgs = [int(c) for c in cfgs]
        buf = (C.c_int32 * len(cfgs))(*cfgs)
        self._chk(self.lib.yp_tuning_import(self._h, int(B), int(H), int(W), buf, len(cfgs)))

    def set_nms(self, conf: float = 0.25, iou: float = 0.7) -> None:
        """families v8 / 11: thresholds of the NMS inside the forward (`.predict(conf=, iou=)`)."""
        self._chk(self.lib.yp_set_nms(self._h, float(conf), float(iou)))

    def set_nms_options(self, classes=None, agnostic: bool = False, max_nms: int = 16384) -> None:
        """families v8 / 11: `.predict(classes=, agnostic_nms=, max_nms=)` of the NMS inside the forward. `classes`: None (all), an int or
        a sequence of class ids; they are filtered before NMS and before the max_nms cut. `max_nms=30000` is ultralytics' value (the
        default keeps this engine's 16384). A v10 engine refuses (it has no NMS)."""
        if classes is None:
            ids = []
        elif isinstance(classes, (int, np.integer)):
            ids = [int(classes)]
        else:
            ids = [int(c) for c in classes]
        buf = (C.c_int32 * len(ids))(*ids) if ids else None
        self._chk(self.lib.yp_set_nms_options(self._h, buf, len(ids), int(bool(agnostic)), int(max_nms)))

    def set_graph(self, enable) -> None:
        """False / 0: eager launches; True / 1: hipGraph replay with head lanes; 2: replay without lanes; "auto" / 3: per input shape
        whichever of eager and replay a one-off timing finds faster (include/yolop.h yp_set_graph)."""
        mode = 3 if enable == "auto" else int(enable)
        self._chk(self.lib.yp_set_graph(self._h, mode))

    # -- hot path ------------------------------------------------------------------------------------------------
    def forward(self, im: torch.Tensor, out: Optional[dict] = None) -> dict:
        """im: uint8 cuda tensor [B,H,W,3] BGR, letterboxed (H,W multiples of 32).
        -> dict(det [B,max_det,6] f32, idx [B,max_det] i32, coeff [B,max_det,32] f32 | None)."""
        if not im.is_cuda or im.dtype != torch.uint8 or im.dim() != 4 or im.shape[-1] != 3:
            raise TypeError("forward expects a uint8 CUDA tensor [B,H,W,3]")
        if im.device.index != self.device_index:
            raise ValueError(f"input is on cuda:{im.device.index}, engine on cuda:{self.device_index}")
        im = im.contiguous()
        B, H, W, _ = im.shape
        dev = im.device
        if out is None:
            out = dict(det=torch.empty((B, self.max_det, 6), dtype=torch.float32, device=dev),
                       idx=torch.empty((B, self.max_det), dtype=torch.int32, device=dev),
                       coeff=torch.empty((B, self.max_det, 32), dtype=torch.float32, device=dev) if self.seg else None)
        cf = out["coeff"].data_ptr() if out.get("coeff") is not None else None
        self._chk(self.lib.yp_forward(self._h, C.c_void_p(im.data_ptr()), B, H, W, C.c_void_p(out["det"].data_ptr()),
                                      C.c_void_p(out["idx"].data_ptr()), C.c_void_p(cf), C.c_void_p(_stream_ptr(dev))))
        self._last_im = im    # keep the input alive until the stream has consumed it
        return out

    def proto(self) -> torch.Tensor:
        """Engine-owned prototypes of the last forward as fp32 [B,Hp,Wp,32] (a copy; test/debug helper)."""
        for t in self.tensors():
            if t["name"].endswith(".proto.cv3"):
                return self.read_tensor(t["index"])
        raise KeyError("proto.cv3")

    def masks(self, b: int, coeff: torch.Tensor, boxes: torch.Tensor, out_hw: Tuple[int, int], retina: bool = True,
              want_masks: bool = True, want_ids: bool = False, suppress_small: bool = False, min_area: int = 100):
        """-> (masks uint8 [n,oh,ow] | None, ids int64 [oh,ow] | None, kept int32 [n] | None)"""
        n = int(coeff.shape[0])
        dev = coeff.device
        oh, ow = int(out_hw[0]), int(out_hw[1])
        coeff = coeff.to(torch.float32).contiguous()
        boxes = boxes.to(torch.float32).contiguous()
        m = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev) if want_masks else None
        ids = torch.empty((oh, ow), dtype=torch.int64, device=dev) if want_ids else None
        kept = torch.empty((n,), dtype=torch.int32, device=dev) if want_ids else None
        self._chk(self.lib.yp_masks(self._h, b, C.c_void_p(coeff.data_ptr()), C.c_void_p(boxes.data_ptr()), n, oh, ow,
                                    1 if retina else 0, C.c_void_p(m.data_ptr() if m is not None else None),
                                    C.c_void_p(ids.data_ptr() if ids is not None else None),
                                    C.c_void_p(kept.data_ptr() if kept is not None else None),
                                    1 if suppress_small else 0, int(min_area), C.c_void_p(_stream_ptr(dev))))
        self._keep = [coeff, boxes]
        return m, ids, kept

    def masks_frames(self, frame_idx, coeff: torch.Tensor, boxes: torch.Tensor, out_hw: Tuple[int, int],
                     out: Optional[torch.Tensor] = None, retina: bool = True) -> torch.Tensor:
        """yp_masks_frames: one retina mask per entry of `frame_idx` (images of the last forward; gaps and repeats allowed). `coeff` is the
        forward's float32 cuda [B,max_det,32] (row 0 of image frame_idx[j] is used), `boxes` float32 cuda [k,4] in original-image pixels.
        -> uint8 cuda [k,oh,ow] {0,1}, mask j equal to masks(frame_idx[j], coeff[frame_idx[j], :1], boxes[j:j+1], out_hw, retina=True)[0].
        retina=False: yp_masks_frames_input - boxes in letterboxed-input pixels, out_hw the forward's input size (H, W), mask j equal to
        masks(..., out_hw, retina=False)[0]."""
        fidx = np.ascontiguousarray(np.asarray(frame_idx, dtype=np.int64).reshape(-1)).astype(np.int32)
        k = int(fidx.shape[0])
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if not (coeff.is_cuda and coeff.dtype == torch.float32 and coeff.dim() == 3 and coeff.shape[2] == 32 and coeff.is_contiguous()):
            raise ValueError("masks_frames: coeff must be a contiguous float32 CUDA tensor [B,max_det,32]")
        if not (boxes.is_cuda and boxes.dtype == torch.float32 and tuple(boxes.shape) == (k, 4) and boxes.device == coeff.device):
            raise ValueError(f"masks_frames: boxes must be a float32 CUDA tensor [{k},4] on {coeff.device}")
        if k and (fidx.min() < 0 or fidx.max() >= coeff.shape[0]):
            raise ValueError(f"masks_frames: frame indices must lie in [0,{int(coeff.shape[0])})")
        dev = coeff.device
        boxes = boxes.contiguous()
        if out is None:
            out = torch.empty((k, oh, ow), dtype=torch.uint8, device=dev)
        if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (k, oh, ow) and out.is_contiguous() and out.device == dev):
            raise ValueError(f"masks_frames: output must be a contiguous uint8 CUDA tensor [{k},{oh},{ow}] on {dev}")
        fn = self.lib.yp_masks_frames if retina else self.lib.yp_masks_frames_input
        self._chk(fn(self._h, fidx.ctypes.data_as(C.c_void_p), k, C.c_void_p(coeff.data_ptr()), int(coeff.stride(0)), C.c_void_p(boxes.data_ptr()),
                     oh, ow, C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(dev))))
        self._keep = [coeff, boxes]
        return out

    def id_mask_resized(self, b: int, coeff: torch.Tensor, boxes: torch.Tensor, mask_hw: Tuple[int, int], out_hw: Tuple[int, int],
                        suppress_small: bool = False, min_area: int = 100):
        """`auto_segment` with min_side > 0 (yp_id_mask_resized): masks at `mask_hw` (the shrunk frame), antialiased bilinear to
        `out_hw`, float-area test, paint. -> (ids int64 [out_hw] cuda, kept int32 [n] cuda)"""
        n = int(coeff.shape[0])
        dev = coeff.device
        coeff = coeff.to(torch.float32).contiguous()
        boxes = boxes.to(torch.float32).contiguous()
        ids = torch.empty((int(out_hw[0]), int(out_hw[1])), dtype=torch.int64, device=dev)
        kept = torch.empty((n,), dtype=torch.int32, device=dev)
        self._chk(self.lib.yp_id_mask_resized(self._h, b, C.c_void_p(coeff.data_ptr()), C.c_void_p(boxes.data_ptr()), n, int(mask_hw[0]),
                                              int(mask_hw[1]), int(out_hw[0]), int(out_hw[1]), C.c_void_p(ids.data_ptr()),
                                              C.c_void_p(kept.data_ptr()), 1 if suppress_small else 0, int(min_area),
                                              C.c_void_p(_stream_ptr(dev))))
        self._keep = [coeff, boxes]
        return ids, kept

    def id_masks_frames_workspace(self, n_total: int, k: int, mask_hw: Tuple[int, int], out_hw: Optional[Tuple[int, int]] = None) -> int:
        """yp_id_masks_frames_workspace: bytes of engine workspace id_masks_frames needs for `k` frames with `n_total` masks in all at the
        engine's current plan (host arithmetic). 0: no plan yet, or sizes the call refuses."""
        oh, ow = int(mask_hw[0]), int(mask_hw[1])
        rh, rw = (oh, ow) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        return int(self.lib.yp_id_masks_frames_workspace(self._h, int(n_total), int(k), oh, ow, rh, rw))

    def id_masks_frames(self, frame_idx, counts, coeff: torch.Tensor, boxes: torch.Tensor, mask_hw: Tuple[int, int],
                        out_hw: Optional[Tuple[int, int]] = None, suppress_small: bool = False, min_area: int = 100):
        """yp_id_masks_frames: the id image of every frame of `frame_idx` (images of the last forward; gaps and repeats allowed) from ALL its
        masks. Frame j owns the next counts[j] rows of `coeff` float32 cuda [n_total,32] and `boxes` float32 cuda [n_total,4] (pixels of
        `mask_hw`, the size the masks are made at); `out_hw` is the size of the id images (antialiased second resize when it differs).
        -> (ids int64 cuda [k,rh,rw], kept int32 cuda [n_total]); frame j's part equals masks(frame_idx[j], its rows, mask_hw, want_ids=True)
        or id_mask_resized(frame_idx[j], its rows, mask_hw, out_hw) byte for byte."""
        fidx = np.ascontiguousarray(np.asarray(frame_idx, dtype=np.int64).reshape(-1)).astype(np.int32)
        cnt = np.asarray(counts, dtype=np.int64).reshape(-1)
        k = int(fidx.shape[0])
        if cnt.shape[0] != k:
            raise ValueError(f"id_masks_frames: {k} frames but {cnt.shape[0]} counts")
        if k and cnt.min() < 0:
            raise ValueError("id_masks_frames: negative count")
        n_total = int(cnt.sum())
        if n_total >= 2 ** 31:
            raise ValueError("id_masks_frames: too many rows")
        row_off = np.zeros(k + 1, dtype=np.int32)
        row_off[1:] = np.cumsum(cnt)
        oh, ow = int(mask_hw[0]), int(mask_hw[1])
        rh, rw = (oh, ow) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if not (coeff.is_cuda and coeff.dtype == torch.float32 and tuple(coeff.shape) == (n_total, 32)):
            raise ValueError(f"id_masks_frames: coeff must be a float32 CUDA tensor [{n_total},32]")
        if not (boxes.is_cuda and boxes.dtype == torch.float32 and tuple(boxes.shape) == (n_total, 4) and boxes.device == coeff.device):
            raise ValueError(f"id_masks_frames: boxes must be a float32 CUDA tensor [{n_total},4] on {coeff.device}")
        dev = coeff.device
        coeff, boxes = coeff.contiguous(), boxes.contiguous()
        ids = torch.empty((k, max(rh, 0), max(rw, 0)), dtype=torch.int64, device=dev)
        kept = torch.empty((n_total,), dtype=torch.int32, device=dev)
        self._chk(self.lib.yp_id_masks_frames(self._h, fidx.ctypes.data_as(C.c_void_p), row_off.ctypes.data_as(C.c_void_p), k,
                                              C.c_void_p(coeff.data_ptr()), C.c_void_p(boxes.data_ptr()), oh, ow, rh, rw,
                                              C.c_void_p(ids.data_ptr()), C.c_void_p(kept.data_ptr()), 1 if suppress_small else 0, int(min_area),
                                              C.c_void_p(_stream_ptr(dev))))
        self._keep = [coeff, boxes]
        return ids, kept

    # -- introspection ---------------------------------------------------------------------------------------------
    def plan(self, B: int, H: int, W: int) -> List[dict]:
        n = self._chk(self.lib.yp_plan(self._h, B, H, W))
        ops = []
        name = C.create_string_buffer(256)
        kind, fl, by = C.c_int(), C.c_double(), C.c_double()
        t, co, cc = C.c_int(), C.c_int(), C.c_int()
        for i in range(n):
            self._chk(self.lib.yp_op_info(self._h, i, name, 256, C.byref(kind), C.byref(fl), C.byref(by)))
            self._chk(self.lib.yp_op_output(self._h, i, C.byref(t), C.byref(co), C.byref(cc)))
            rec = dict(name=name.value.decode(), kind=OP_KINDS[kind.value], flops=fl.value, bytes=by.value,
                       out=(t.value, co.value, cc.value))
            self._chk(self.lib.yp_op_kernel(self._h, i, name, 256))
            rec["kernel"] = name.value.decode()
            cr = C.c_int()
            self._chk(self.lib.yp_op_input(self._h, i, C.byref(t), C.byref(co), C.byref(cc), C.byref(cr)))
            rec["in"] = (t.value, co.value, cc.value)
            rec["c_read"] = cr.value
            pre, stored = C.c_int(), C.c_int()
            self._chk(self.lib.yp_op_fusion(self._h, i, C.byref(pre), C.byref(stored)))
            rec["pre"], rec["pre_stored"] = pre.value, bool(stored.value)     # pwsp_kernel: the 1x1 conv fused in front (or -1), and whether its output is written too
            self._chk(self.lib.yp_debug_op_cfg(self._h, i, C.byref(pre)))
            rec["cfg"] = pre.value          # the tile configuration id run_op launches it with under the forced id (-1: a heuristic picks)
            absorbed = (C.c_int * 3)()
            n_abs = self._chk(self.lib.yp_debug_op_form(self._h, i, C.byref(pre), absorbed, 3))
            rec["form"], rec["absorbed"] = FORMS[pre.value], list(absorbed[:n_abs])   # the fused launch form and the ops whose work it takes over
            ops.append(rec)
        return ops

    def max_batch(self, H: int, W: int) -> int:
        """The largest batch that plans at HxW (every activation below 2^31 bytes); callers split larger groups to it."""
        return self._chk(self.lib.yp_max_batch(self._h, int(H), int(W)))

    def tensors(self) -> List[dict]:
        n = self._chk(self.lib.yp_tensor_count(self._h))
        name = C.create_string_buffer(256)
        dims = (C.c_int * 4)()
        f32 = C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.yp_tensor_info(self._h, i, name, 256, dims, C.byref(f32)))
            out.append(dict(index=i, name=name.value.decode(), shape=tuple(dims), f32=bool(f32.value)))
        return out

    def find_tensor(self, name: str) -> int:
        for t in self.tensors():
            if t["name"] == name:
                return t["index"]
        raise KeyError(name)

    def read_tensor(self, index: int) -> torch.Tensor:
        """Debug tap: NHWC fp32 host copy of an engine-owned activation of the last forward."""
        info = self.tensors()[index]
        out = torch.empty(info["shape"], dtype=torch.float32)
        self._chk(self.lib.yp_tensor_read(self._h, index, C.c_void_p(out.data_ptr())))
        return out

    def run_op(self, i: int, im: torch.Tensor, out: dict) -> None:
        """Debug stepping: launch op i of the current plan (inputs are whatever the engine tensors hold)."""
        cf = out["coeff"].data_ptr() if out.get("coeff") is not None else None
        self._chk(self.lib.yp_run_op(self._h, i, C.c_void_p(im.data_ptr()), C.c_void_p(out["det"].data_ptr()),
                                     C.c_void_p(out["idx"].data_ptr()), C.c_void_p(cf), C.c_void_p(_stream_ptr(im.device))))

    def write_tensor(self, index: int, coff: int, data_nhwc: torch.Tensor) -> None:
        """Debug: overwrite channels [coff, coff+C) of an engine tensor from an fp32 host tensor [B,H,W,C]."""
        d = data_nhwc.detach().to(torch.float32).contiguous().cpu()
        self._chk(self.lib.yp_tensor_write(self._h, index, coff, int(d.shape[-1]), C.c_void_p(d.data_ptr())))

    def head_winners(self, B: int):
        """Debug: what the winners-only head left behind the last forward - (mode bits, sel [B,512] int32, box rows [B,max_det,64],
        coefficient rows [B,max_det,32]); mode 0 = dense head (arrays are then zeros)."""
        sel = torch.zeros((B, 512), dtype=torch.int32)
        box = torch.zeros((B, self.max_det, 64), dtype=torch.float32)
        cf = torch.zeros((B, self.max_det, 32), dtype=torch.float32)
        mode = self._chk(self.lib.yp_debug_head_winners(self._h, C.c_void_p(sel.data_ptr()), C.c_void_p(box.data_ptr()), C.c_void_p(cf.data_ptr())))
        return mode, sel, box, cf

    def tuning_source(self) -> str:
        """Where the current plan's tile configurations came from: "tuner", "cache file" (YOLOP_TUNE_CACHE) or "packaged table"."""
        r = self.lib.yp_tuning_source(self._h)
        if r < 0:
            self._chk(r)
        return ("tuner", "cache file", "packaged table")[r]

    def graph_info(self) -> dict:
        """What the last hipGraph capture built (yp_debug_graph_info): captures so far, nodes, edges, the lane schedule's edge count."""
        v = (C.c_int64 * 6)()
        self._chk(self.lib.yp_debug_graph_info(self._h, v))
        return dict(captures=int(v[0]), nodes=int(v[1]), edges=int(v[2]), schedule_edges=int(v[3]), lanes=int(v[4]), live=bool(v[5]))

    def head_positions(self) -> Optional[dict]:
        """Winners-only head, last forward: distinct 3x3-neighbourhood positions and winners per level (P3, P4, P5); None = dense head."""
        v = (C.c_int64 * 6)()
        if self._chk(self.lib.yp_debug_head_positions(self._h, v)) == 0:
            return None
        return dict(positions=[int(v[i]) for i in range(3)], winners=[int(v[3 + i]) for i in range(3)])

    def profile(self, im: torch.Tensor, iters: int = 5) -> List[dict]:
        """Per-op HIP-event timing (eager, one event pair per launch) on the current stream."""
        B, H, W, _ = im.shape
        ops = self.plan(B, H, W)
        dev = im.device
        det = torch.empty((B, self.max_det, 6), dtype=torch.float32, device=dev)
        idx = torch.empty((B, self.max_det), dtype=torch.int32, device=dev)
        cf = torch.empty((B, self.max_det, 32), dtype=torch.float32, device=dev) if self.seg else None
        ms = (C.c_float * len(ops))()
        self._chk(self.lib.yp_profile(self._h, C.c_void_p(im.data_ptr()), B, H, W, C.c_void_p(det.data_ptr()),
                                      C.c_void_p(idx.data_ptr()), C.c_void_p(cf.data_ptr() if cf is not None else None),
                                      ms, iters, C.c_void_p(_stream_ptr(dev))))
        for o, m in zip(ops, ms):
            o["ms"] = float(m)
        return ops
