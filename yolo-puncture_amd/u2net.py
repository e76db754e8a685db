"""U^2-Net-P on the MI355X engine: host mirror of the reference's `load_unet` / `unet_predict`
(yolo_seg/tasks/unet_segment.py:32-73, called per frame at yolo_seg/app.py:46,184) over libyolop.so's yp_u2net_* entry points.

The network itself (yolo_seg/tasks/models/U2Net.py:424-526: six RSU encoder stages, five decoder stages, six side outputs, 1x1
fusion, sigmoid) runs only through the HIP library: dilated 3x3 convolutions with the folded BatchNorm + ReLU (+ the block
residual) in the epilogue on the matrix cores, ceil-mode 2x2 max-pool, bilinear resize-to-size written straight into the concat
buffer, and one tail kernel for side maps -> fusion -> sigmoid -> min-max normalisation -> mask. There is no CPU fallback.

`unet_predict_clip` is the clip form of the app's per-frame `crop_frame` + `unet_predict` + paste (yolo_seg/app.py:127,183-186): the
crops are cut from the uint8 frames on the device and run in batches, with normPRED per frame as the per-frame call has it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .engine import YolopError, load_library

BN_EPS = 1e-5

# (kind, in, mid, out) per stage - U2NETP (U2Net.py:429-448), U2NET (:323-342)
_CFG = {
    "p": dict(enc=[("RSU7", 3, 16, 64), ("RSU6", 64, 16, 64), ("RSU5", 64, 16, 64), ("RSU4", 64, 16, 64), ("RSU4F", 64, 16, 64), ("RSU4F", 64, 16, 64)],
              dec=[("RSU4F", 128, 16, 64), ("RSU4", 128, 16, 64), ("RSU5", 128, 16, 64), ("RSU6", 128, 16, 64), ("RSU7", 128, 16, 64)],
              side=[64, 64, 64, 64, 64, 64]),
    "f": dict(enc=[("RSU7", 3, 32, 64), ("RSU6", 64, 32, 128), ("RSU5", 128, 64, 256), ("RSU4", 256, 128, 512), ("RSU4F", 512, 256, 512), ("RSU4F", 512, 256, 512)],
              dec=[("RSU4F", 1024, 256, 512), ("RSU4", 1024, 128, 256), ("RSU5", 512, 64, 128), ("RSU6", 256, 32, 64), ("RSU7", 128, 16, 64)],
              side=[64, 64, 128, 256, 512, 512]),
}


def conv_specs(variant: str = "p") -> List[Tuple[str, int, int, bool]]:
    """(module name, cin, cout, has_bn) of every convolution, in state-dict order of the reference modules."""
    cfg = _CFG[variant]
    out: List[Tuple[str, int, int, bool]] = []

    def rsu(p, kind, cin, mid, co):
        out.append((f"{p}.rebnconvin", cin, co, True))
        out.append((f"{p}.rebnconv1", co, mid, True))
        n = 4 if kind == "RSU4F" else int(kind[3:])
        for i in range(2, n + 1):
            out.append((f"{p}.rebnconv{i}", mid, mid, True))
        for i in range(n - 1, 1, -1):
            out.append((f"{p}.rebnconv{i}d", 2 * mid, mid, True))
        out.append((f"{p}.rebnconv1d", 2 * mid, co, True))

    for i, (kind, cin, mid, co) in enumerate(cfg["enc"]):
        rsu(f"stage{i + 1}", kind, cin, mid, co)
    for j, (kind, cin, mid, co) in enumerate(cfg["dec"]):
        rsu(f"stage{5 - j}d", kind, cin, mid, co)
    for k, c in enumerate(cfg["side"]):
        out.append((f"side{k + 1}", c, 1, False))
    out.append(("outconv", 6, 1, False))
    return out


def synthetic_state(variant: str = "p", seed: int = 0, gain: float = 1.25, side_gain: float = 8.0) -> Dict[str, torch.Tensor]:
    """Seeded state dict in the reference's layout (no checkpoint exists offline): scaled-normal conv weights, small conv biases,
    BatchNorm statistics away from the identity so that the fold is exercised. The gains keep the activations O(1) through the
    ~110 convolutions and spread the fused logit over about +-5 (neither dead nor saturated)."""
    g = torch.Generator().manual_seed(seed)
    st: Dict[str, torch.Tensor] = {}
    for name, cin, cout, bn in conv_specs(variant):
        k = 1 if name == "outconv" else 3
        fan = cin * k * k
        if bn:
            st[f"{name}.conv_s1.weight"] = torch.randn(cout, cin, k, k, generator=g) * (gain / fan) ** 0.5
            st[f"{name}.conv_s1.bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
            st[f"{name}.bn_s1.weight"] = 0.6 + 0.8 * torch.rand(cout, generator=g)
            st[f"{name}.bn_s1.bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.4
            st[f"{name}.bn_s1.running_mean"] = torch.randn(cout, generator=g) * 0.1
            st[f"{name}.bn_s1.running_var"] = 0.5 + torch.rand(cout, generator=g)
            st[f"{name}.bn_s1.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
        else:
            st[f"{name}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (side_gain / fan) ** 0.5
            st[f"{name}.bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
    return st


def fold_state(state: Dict[str, torch.Tensor], variant: str = "p") -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Conv + eval-mode BatchNorm -> one (weight, bias) per convolution (fp64 fold, fp32 out); plain convs pass through."""
    out = {}
    for name, cin, cout, bn in conv_specs(variant):
        if bn:
            w = state[f"{name}.conv_s1.weight"].double()
            b = state[f"{name}.conv_s1.bias"].double()
            s = state[f"{name}.bn_s1.weight"].double() / torch.sqrt(state[f"{name}.bn_s1.running_var"].double() + BN_EPS)
            out[name] = ((w * s[:, None, None, None]).float(), ((b - state[f"{name}.bn_s1.running_mean"].double()) * s + state[f"{name}.bn_s1.bias"].double()).float())
        else:
            out[name] = (state[f"{name}.weight"].float(), state[f"{name}.bias"].float())
    return out


def _declare(lib: C.CDLL) -> None:
    if getattr(lib, "_u2_declared", False):
        return
    vp = C.c_void_p
    lib.yp_u2net_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.yp_u2net_destroy.argtypes = [vp]
    lib.yp_u2net_weight_count.argtypes = [vp]
    lib.yp_u2net_weight_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    lib.yp_u2net_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), C.c_int]
    lib.yp_u2net_finalize.argtypes = [vp]
    lib.yp_u2net_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.yp_u2net_forward_crops.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.yp_u2net_set_graph.argtypes = [vp, C.c_int]
    lib.yp_u2net_set_graph.restype = C.c_int
    lib.yp_u2net_tensor_count.argtypes = [vp]
    lib.yp_u2net_tensor_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.yp_u2net_tensor_read.argtypes = [vp, C.c_int, vp]
    lib.yp_u2net_op_count.argtypes = [vp]
    lib.yp_u2net_op_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.c_int]
    for fn in ("yp_u2net_create", "yp_u2net_destroy", "yp_u2net_weight_count", "yp_u2net_weight_info", "yp_u2net_set_weight",
               "yp_u2net_finalize", "yp_u2net_forward", "yp_u2net_forward_crops", "yp_u2net_tensor_count", "yp_u2net_tensor_info", "yp_u2net_tensor_read",
               "yp_u2net_op_count", "yp_u2net_op_info"):
        getattr(lib, fn).restype = C.c_int
    lib._u2_declared = True


class U2NetEngine:
    """One engine per GPU. dtype 'fp32' = exact fp32 FMA chains on the matrix cores (parity mode, the default: the reference runs
    this network in fp32, unet_segment.py:53-60), 'bf16' = bf16 storage with fp32 accumulation."""

    def __init__(self, variant: str = "p", dtype: str = "fp32", device: int = 0, state: Optional[Dict[str, torch.Tensor]] = None):
        self.lib = load_library()
        _declare(self.lib)
        self.variant, self.device_index = variant, int(device)
        self._h = C.c_void_p()
        self._chk(self.lib.yp_u2net_create(ord(variant), {"bf16": 0, "fp32": 1, "f32": 1}[dtype], self.device_index, C.byref(self._h)))
        if state is not None:
            self.load_state(state)
            self.finalize()

    def _chk(self, rc: int) -> int:
        if rc < 0:
            raise YolopError(f"libyolop error {rc}: {self.lib.yp_last_error().decode()}")
        return rc

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.yp_u2net_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def expected_weights(self) -> List[Tuple[str, Tuple[int, ...]]]:
        n = self._chk(self.lib.yp_u2net_weight_count(self._h))
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.yp_u2net_weight_info(self._h, i, name, 256, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[j]) for j in range(nd.value))))
        return out

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        for name, (w, b) in fold_state(state, self.variant).items():
            for suffix, t in ((".weight", w), (".bias", b)):
                t = t.detach().to(torch.float32).contiguous().cpu()
                shp = (C.c_int64 * t.dim())(*t.shape)
                self._chk(self.lib.yp_u2net_set_weight(self._h, (name + suffix).encode(), C.c_void_p(t.data_ptr()), shp, t.dim()))

    def finalize(self) -> None:
        self._chk(self.lib.yp_u2net_finalize(self._h))

    def set_graph(self, enable: bool) -> None:
        self._chk(self.lib.yp_u2net_set_graph(self._h, 1 if enable else 0))

    def forward(self, im_bgr: torch.Tensor, want_mask: bool = True):
        """im_bgr uint8 cuda [B,H,W,3] (BGR, as cv2 frames are) -> (prob float32 [B,H,W] = sigmoid(d0), norm float32 [B,H,W] = normPRED(prob)
        over the whole call, mask uint8 [B,H,W] in {0,255} = norm > 0.5)."""
        if not (im_bgr.is_cuda and im_bgr.dtype == torch.uint8 and im_bgr.dim() == 4 and im_bgr.shape[-1] == 3):
            raise TypeError("forward expects a uint8 CUDA tensor [B,H,W,3]")
        im_bgr = im_bgr.contiguous()
        B, H, W, _ = im_bgr.shape
        dev = im_bgr.device
        prob = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        norm = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_mask else None
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
        self._chk(self.lib.yp_u2net_forward(self._h, C.c_void_p(im_bgr.data_ptr()), B, H, W, C.c_void_p(prob.data_ptr()),
                                            C.c_void_p(norm.data_ptr() if norm is not None else None),
                                            C.c_void_p(mask.data_ptr() if mask is not None else None),
                                            C.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream))))
        self._last = im_bgr
        return prob, norm, mask

    def forward_crops(self, frames: torch.Tensor, windows, frame_idx, crop_hw: Tuple[int, int], *, want_prob: bool = True,
                      want_crop_mask: bool = True, frame_mask: Union[None, bool, torch.Tensor] = None):
        """Crops of uint8 cuda frames [N,H,W,3] (BGR) -> (prob float32 [B,ch,cw], crop mask uint8 [B,ch,cw], frame mask uint8 [N,H,W]),
        each None unless asked for. `windows` int [B,4] are clipped (x1,y1,x2,y2) windows (crop_window), `frame_idx` int [B] the frame of
        each; every window fits in crop_hw = (ch, cw) and sits at its top-left, the rest of the crop is zero. normPRED runs per crop. The
        frame mask (True = allocate, or a uint8 cuda [N,H,W] tensor to write into) gets every pixel of each named frame written: the crop
        mask inside the window, 0 outside; frames no crop names are left as they are. Launches on the caller's current stream."""
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise TypeError("forward_crops expects uint8 CUDA frames [N,H,W,3]")
        frames = frames.contiguous()
        N, H, W, _ = frames.shape
        win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 4))
        fidx = np.ascontiguousarray(np.asarray(frame_idx, dtype=np.int32).reshape(-1))
        if win.shape[0] != fidx.shape[0]:
            raise ValueError(f"{win.shape[0]} windows but {fidx.shape[0]} frame indices")
        B = win.shape[0]
        ch, cw = (int(v) for v in crop_hw)
        dev = frames.device
        prob = torch.empty((B, ch, cw), dtype=torch.float32, device=dev) if want_prob else None
        cmask = torch.empty((B, ch, cw), dtype=torch.uint8, device=dev) if want_crop_mask else None
        if frame_mask is True:
            frame_mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        elif frame_mask is False:
            frame_mask = None
        if frame_mask is not None and not (frame_mask.device == dev and frame_mask.dtype == torch.uint8 and tuple(frame_mask.shape) == (N, H, W)
                                           and frame_mask.is_contiguous()):
            raise TypeError(f"frame_mask must be a contiguous uint8 tensor [{N},{H},{W}] on {dev}")

        def ptr(t):
            return C.c_void_p(t.data_ptr() if t is not None else None)
        self._chk(self.lib.yp_u2net_forward_crops(self._h, ptr(frames), N, H, W, win.ctypes.data_as(C.c_void_p), fidx.ctypes.data_as(C.c_void_p),
                                                  B, ch, cw, ptr(prob), ptr(cmask), ptr(frame_mask),
                                                  C.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream))))
        return prob, cmask, frame_mask

    def tensors(self) -> List[dict]:
        n = self._chk(self.lib.yp_u2net_tensor_count(self._h))
        name = C.create_string_buffer(256)
        dims = (C.c_int * 4)()
        return [dict(index=i, name=(self._chk(self.lib.yp_u2net_tensor_info(self._h, i, name, 256, dims)), name.value.decode())[1], shape=tuple(dims))
                for i in range(n)]

    def ops(self) -> List[dict]:
        """The ops of the current plan, in launch order (read-only): kind 'input' | 'conv' | 'pool' | 'up'; `in`, `out`, `res` = (tensor index,
        first channel, channels), res[0] < 0 when there is none; dil, act (0 none, 2 ReLU), cin (logical), impl (-1 not chosen yet,
        0 conv_igemm, 1 conv_small, 2 conv_small taking its pool / up-sample while loading, 3 conv_halo_f32: final after a forward of the
        shape), pool_op / up_op (convs) and consumer (pools / up-samples): op indices or -1. A pool / up-sample whose consumer has impl 2
        does not launch."""
        n = self._chk(self.lib.yp_u2net_op_count(self._h))
        name = C.create_string_buffer(256)
        f = (C.c_int32 * 17)()
        out = []
        for i in range(n):
            if self._chk(self.lib.yp_u2net_op_info(self._h, i, name, 256, f, 17)) != 17:
                raise YolopError("yp_u2net_op_info: this library reports another field count than 17")
            v = [int(x) for x in f]
            out.append({"index": i, "name": name.value.decode(), "kind": ("input", "conv", "pool", "up")[v[0]], "in": tuple(v[1:4]),
                        "out": tuple(v[4:7]), "res": tuple(v[7:10]), "dil": v[10], "act": v[11], "cin": v[12], "impl": v[13],
                        "pool_op": v[14], "up_op": v[15], "consumer": v[16]})
        return out

    def read_tensor(self, name: str) -> torch.Tensor:
        """Debug tap: NHWC fp32 host copy of an activation of the last forward."""
        for t in self.tensors():
            if t["name"] == name:
                out = torch.empty(t["shape"], dtype=torch.float32)
                self._chk(self.lib.yp_u2net_tensor_read(self._h, t["index"], C.c_void_p(out.data_ptr())))
                return out
        raise KeyError(name)


# ---- the reference's two entry points (yolo_seg/tasks/unet_segment.py:32-73) ------------------------------------------------------------
def load_unet(model_name: str = "u2netp", model_dir: str = "", device="cuda", dtype: str = "fp32") -> U2NetEngine:
    """`load_unet(model_name, model_dir, device)`: model_dir is the path of the `.pth` state dict (as in the reference, :43-46)."""
    variant = {"u2netp": "p", "u2net": "f"}.get(model_name)
    if variant is None:
        raise ValueError(f"unknown model_name {model_name!r} (u2net | u2netp)")
    if not os.path.isfile(model_dir):
        raise FileNotFoundError(f"{model_dir}: no such state dict (nothing is downloaded)")
    state = torch.load(model_dir, map_location="cpu", weights_only=True)
    d = torch.device(device if device != "cuda" else "cuda:0")
    if d.type != "cuda":
        raise ValueError("this engine runs on MI355X GPUs only")
    return U2NetEngine(variant, dtype, d.index or 0, state=state)


def unet_predict(model: U2NetEngine, image: np.ndarray, device="cuda") -> np.ndarray:
    """`unet_predict(model, image)` (:53-73): BGR uint8 HWC frame -> uint8 mask {0,255} [H,W] (numpy, as the reference returns)."""
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise TypeError("unet_predict expects a BGR uint8 HWC frame")
    x = torch.from_numpy(np.ascontiguousarray(image)).to(torch.device("cuda", model.device_index))[None]
    _, _, mask = model.forward(x)
    return mask[0].cpu().numpy()


# ---- the app's crop + predict + paste over a whole clip (yolo_seg/app.py:127,183-186) ---------------------------------------------------
U2_OFFSET_LIMIT = 1 << 31          # plan_u2 (u2net.hip): B x H x W x 128 channels x 4 bytes must stay below 2^31


def crop_window(box: Sequence[int], height: int, width: int, crop_size: int = 380) -> Tuple[Tuple[int, int, int, int], Tuple[int, int]]:
    """crop_frame(frame, box, crop_size, need_padding=False) (yolo_seg/utils/transform.py:22-50) as geometry: ((x1, y1, x2, y2), (ch, cw)).

    The centre is int((x1+x2)/2), int((y1+y2)/2); the window [c - crop_size//2, c + crop_size//2) is clipped to the frame and returned as
    crop_frame returns it. Its padding test reads `if need_padding and h < crop_size or w < crop_size`, which Python groups as
    `(need_padding and h < crop_size) or (w < crop_size)`: with need_padding=False only a window narrower than crop_size is padded, to
    crop_size x crop_size with the window at the top-left. A full-width window stays unpadded, (y2-y1) x crop_size, also when it is short.
    classify.crop_geometry is the need_padding=True sibling (the classifier's crops are always crop_size^2)."""
    x1, y1, x2, y2 = (int(v) for v in box)
    cx, cy = int((x1 + x2) / 2), int((y1 + y2) / 2)
    half = crop_size // 2
    wx1, wy1 = max(0, cx - half), max(0, cy - half)
    wx2, wy2 = min(int(width), cx + half), min(int(height), cy + half)
    if max(0, wx2 - wx1) < crop_size:
        shape = (crop_size, crop_size)
    else:
        shape = (wy2 - wy1, wx2 - wx1)
    return (wx1, wy1, wx2, wy2), shape


def max_crops_per_call(ch: int, cw: int) -> int:
    """The most ch x cw crops one yp_u2net_forward_crops call takes (the engine's 32-bit offset guard)."""
    return (U2_OFFSET_LIMIT - 1) // (int(ch) * int(cw) * 128 * 4)


def clip_chunks(shapes: Sequence[Tuple[int, int]], batch_size: int = 16) -> List[Tuple[Tuple[int, int], List[int]]]:
    """Group frame indices by crop shape (first appearance order) and split each group into chunks whose sizes are powers of two, the
    largest first, capped by batch_size and by max_crops_per_call: each shape meets at most log2(batch_size)+1 batch sizes, so at most
    that many engine plans (and tuning passes)."""
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, s in enumerate(shapes):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    out: List[Tuple[Tuple[int, int], List[int]]] = []
    for shape, idx in groups.items():
        cap = min(int(batch_size), max_crops_per_call(*shape))
        if cap < 1:
            raise ValueError(f"a {shape[0]}x{shape[1]} crop is too large for the engine")
        top = 1 << (cap.bit_length() - 1)
        k = 0
        while k < len(idx):
            n = top
            while n > len(idx) - k:
                n >>= 1
            out.append((shape, idx[k:k + n]))
            k += n
    return out


def unet_predict_clip(model: U2NetEngine, frames, boxes, device="cuda", *, batch_size: int = 16, full_frame: bool = False):
    """The app's loop body `crop_frame(frame, box)` -> `unet_predict(model, crop)` -> paste into a full-frame mask, for a whole clip.

    frames: a list of same-shape BGR uint8 HWC ndarrays, or a uint8 CUDA tensor [N,H,W,3]; boxes: one integer xyxy per frame (the app's
    yolo_pred_xyxy). Returns [(mask, (x1, y1, x2, y2)), ...] in input order, mask being the uint8 {0,255} ndarray
    unet_predict(model, crop_frame(frame, box)[0]) returns (normPRED per frame, the zero pad included); with full_frame=True a uint8 CUDA
    tensor [N,H,W] instead: each frame's crop mask pasted at its window, 0 elsewhere (the app's paste, which raises in the reference when
    the crop is padded). Frames are grouped by crop shape and run batch_size at a time (clip_chunks); host frames go
    up one chunk at a time. `device` is accepted for the reference's signature; the engine's device is used."""
    on_dev = isinstance(frames, torch.Tensor)
    if on_dev:
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise TypeError("unet_predict_clip expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
        N, H, W = (int(v) for v in frames.shape[:3])
    else:
        frames = list(frames)
        N = len(frames)
        for f in frames:
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise TypeError("unet_predict_clip expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
            if f.shape != frames[0].shape:
                raise ValueError(f"frames differ in shape: {f.shape} vs {frames[0].shape}")
        H, W = (int(v) for v in frames[0].shape[:2]) if N else (0, 0)
    boxes = list(boxes)
    if len(boxes) != N:
        raise ValueError(f"{N} frames but {len(boxes)} boxes")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    if N == 0:
        return []
    geo = [crop_window(b, H, W) for b in boxes]
    for i, ((x1, y1, x2, y2), _) in enumerate(geo):
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"frame {i}: box {tuple(boxes[i])} has its centre outside the {W}x{H} frame")
    chunks = clip_chunks([g[1] for g in geo], batch_size)

    dev = torch.device("cuda", model.device_index)
    if on_dev:
        if frames.device != dev:
            raise ValueError(f"frames are on {frames.device}, the engine on {dev}")
        frames = frames.contiguous()
    full = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if full_frame else None
    pending = []
    for shape, idx in chunks:
        win = np.array([geo[i][0] for i in idx], dtype=np.int32)
        if on_dev:
            _, cm, _ = model.forward_crops(frames, win, np.array(idx, dtype=np.int32), shape, want_prob=False, want_crop_mask=not full_frame,
                                           frame_mask=full)
        else:
            up = torch.from_numpy(np.stack([frames[i] for i in idx])).to(dev)
            _, cm, fm = model.forward_crops(up, win, np.arange(len(idx), dtype=np.int32), shape, want_prob=False,
                                            want_crop_mask=not full_frame, frame_mask=full_frame)
            if full_frame:
                full.index_copy_(0, torch.tensor(idx, dtype=torch.long, device=dev), fm)
        if not full_frame:
            pending.append((idx, cm))
    if full_frame:
        return full
    out: List = [None] * N
    for idx, cm in pending:
        host = cm.cpu().numpy()
        for j, i in enumerate(idx):
            out[i] = (host[j], geo[i][0])
    return out
