"""`YOLO(...).predict(...)` facade over the MI355X engine: the exact Python surface the reference's callers use.

Call sites mirrored (reference = /root/reference):
    YOLO(path)                                         yolo_seg/app.py:45, yolo_seg/yolo_with_deva.py:226,
                                                       dev_tools/auto_speed_calc.py:40, dev_tools/classify/cls_bbox_dataset_generate.py:66
    .predict(source=, conf=, retina_masks=, device=)   yolo_seg/app.py:49,91 ; yolo_seg/yolo_with_deva.py:51 (positional source) ;
                                                       dev_tools/auto_speed_calc.py:62 ; dev_tools/classify/cls_bbox_dataset_generate.py:48
    results[0].boxes.cpu().numpy() / .xyxy .conf .cls  yolo_seg/app.py:92-98 ; .xywhn cls_bbox_dataset_generate.py:52
    results[0].masks.xy[i] / .data[i] / len(masks)     yolo_seg/app.py:50,101 ; yolo_seg/yolo_with_deva.py:61-68
    yolo.model.parameters() / yolo.model.to(device)    yolo_seg/yolo_with_deva.py:42,130
Semantics follow SURVEY.md Appendix A.5-A.7 [U] (ultralytics is not vendored in the reference).
The network itself runs only through libyolop.so (engine.py); there is no CPU fallback.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import hostops
from .engine import ATTENTION_F32, ATTENTION_F32_WIDE, ATTENTION_FORMS, ID_MASKS_FRAMES_BUDGET, LARGE_MAX_DIM, Engine, letterbox_batch_device, letterbox_device, mask_contours_device, mask_contours_large_device
from .weights import read_ultralytics_pt, synthetic_state

_ENGINE_CACHE: Dict[tuple, Engine] = {}


def shutdown() -> None:
    """Destroy every cached engine now (device memory, streams, graphs). Registered with atexit so that it runs while the HIP
    runtime and torch are still alive - not from `Engine.__del__` during interpreter teardown."""
    while _ENGINE_CACHE:
        _, eng = _ENGINE_CACHE.popitem()
        try:
            eng.close()
        except Exception:
            pass


import atexit  # noqa: E402

atexit.register(shutdown)


class Boxes:
    """[n,6] rows = x1,y1,x2,y2 (original-image pixels), conf, cls; sorted by conf descending."""

    def __init__(self, data, orig_shape: Tuple[int, int]):
        self.data = data
        self.orig_shape = tuple(orig_shape)

    def _new(self, data):
        return Boxes(data, self.orig_shape)

    def cpu(self):
        return self._new(self.data.cpu() if isinstance(self.data, torch.Tensor) else self.data)

    def numpy(self):
        return self._new(self.data.detach().cpu().numpy() if isinstance(self.data, torch.Tensor) else self.data)

    def to(self, *a, **k):
        return self._new(self.data.to(*a, **k) if isinstance(self.data, torch.Tensor) else self.data)

    def __len__(self):
        return int(self.data.shape[0])

    def __getitem__(self, i):
        d = self.data[i]
        return self._new(d.reshape(-1, 6) if d.ndim == 1 else d)

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, 4]

    @property
    def cls(self):
        return self.data[:, 5]

    @property
    def xywh(self):
        x = self.xyxy
        cat = torch.stack if isinstance(x, torch.Tensor) else np.stack
        return cat(((x[:, 0] + x[:, 2]) / 2, (x[:, 1] + x[:, 3]) / 2, x[:, 2] - x[:, 0], x[:, 3] - x[:, 1]), -1)

    @property
    def xyxyn(self):
        h, w = self.orig_shape
        x = self.xyxy
        s = x.new_tensor([w, h, w, h]) if isinstance(x, torch.Tensor) else np.asarray([w, h, w, h], dtype=x.dtype)
        return x / s

    @property
    def xywhn(self):
        h, w = self.orig_shape
        x = self.xywh
        s = x.new_tensor([w, h, w, h]) if isinstance(x, torch.Tensor) else np.asarray([w, h, w, h], dtype=x.dtype)
        return x / s


MASK_POLYGON_STRATEGY = "all"     # ultralytics masks2segments(strategy=...) [U]: "all" is the default of the 8.3.x line the app's YOLO11 weights
                                  # need - every external contour, laid end to end (8.1 ... early 8.3) or, "all_merged", bridged at their closest
                                  # points with merge_multi_segment (later 8.3.x); "largest" is the default of 8.0. All three give the same
                                  # minimum-area rectangle whenever a mask has one contour, and "all" / "all_merged" always (same point set).
                                  # SURVEY A.7; set before predicting.


class Masks:
    """.data: float {0,1} [n,H,W] (H,W = original image when retina_masks else the letterboxed input);
    .xy: one float32 [m,2] polygon per mask - cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) + masks2segments(MASK_POLYGON_STRATEGY)
    as hostops defines them, in pixels of the original image.
    When the masks live on the GPU the contour, its convex hull and the minimum-area rectangle are computed there
    (yp_mask_contours) and only the polygon's few hundred points travel to the host; `.min_rect` is the rectangle
    `get_coord_min_rect_len` would derive from `.xy[i]` (reference yolo_seg/app.py:101-103)."""

    def __init__(self, data: Optional[torch.Tensor], orig_shape: Tuple[int, int], u8: Optional[torch.Tensor] = None, strategy: Optional[str] = None):
        if data is None and u8 is None:
            raise ValueError("Masks needs data or u8")
        self.strategy = strategy or MASK_POLYGON_STRATEGY
        self._data = data                 # float {0,1}; made from the uint8 masks on first use (the engine produces uint8)
        self.orig_shape = tuple(orig_shape)
        self._u8 = u8                     # the engine's uint8 masks (same pixels as data), kept for the device contour pass
        self._polys: Dict[int, np.ndarray] = {}
        self._rects: Dict[int, Tuple[float, float]] = {}

    @property
    def data(self):
        if self._data is None:
            self._data = self._u8.to(torch.float32)
        return self._data

    @property
    def shape(self):
        return tuple((self._data if self._data is not None else self._u8).shape)

    def cpu(self):
        m = Masks(self.data.cpu(), self.orig_shape, self._u8, self.strategy)
        m._polys, m._rects = self._polys, self._rects
        return m

    def numpy(self):
        d = self.data
        m = Masks(d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else d, self.orig_shape, self._u8, self.strategy)
        m._polys, m._rects = self._polys, self._rects
        return m

    def __len__(self):
        return int(self.shape[0])

    def __getitem__(self, i):
        u = self._u8[i] if self._u8 is not None else None
        if u is not None and u.dim() == 2:
            u = u[None]
        d = None
        if self._data is not None:
            d = self._data[i]
            d = d[None] if d.ndim == 2 else d
        return Masks(d, self.orig_shape, u, self.strategy)

    def _contour(self, i: int) -> np.ndarray:
        """polygon of mask i (float32 [m,2], original-image pixels), computed on first use: the reference's loop touches ONE mask per
        frame (`masks.xy[best]`, yolo_seg/app.py:101), so nothing is traced for the others."""
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        if i in self._polys:
            return self._polys[i]
        mh, mw = self.shape[1:]
        poly, rect, parts = None, None, None
        u8 = self._u8
        one = None
        if u8 is None and isinstance(self._data, torch.Tensor) and self._data.is_cuda:
            one = (self._data[i:i + 1] > 0.5).to(torch.uint8)
        elif u8 is not None and u8.is_cuda:
            one = u8[i:i + 1]
        if one is not None:                               # "all_merged": traced AND bridged on the device (yp_mask_contours_merge); parts
            merged = self.strategy == "all_merged"        # only where that bridge declined: bridged on the host then
            polys, rects, all_parts = _device_contours(one, None, self.strategy, merged)
            poly, rect, parts = polys[0], rects[0], (all_parts[0] if merged else None)

        def host_mask():
            d = self.data[i]
            host = d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
            return host > 0.5

        poly, rect = _finish_contour(poly, rect, parts, self.strategy, host_mask, (mh, mw), self.orig_shape)
        if rect is not None:
            self._rects[i] = rect
        self._polys[i] = poly
        return poly

    @property
    def xy(self) -> "_LazyPolygons":
        return _LazyPolygons(self)

    def min_rect_len(self, i: int):
        """(length, length / width) exactly as `get_coord_min_rect_len(self.xy[i])` returns them (yolo_seg/utils/mask_tools.py:12-22),
        from the device rectangle when there is one."""
        poly = self._contour(i)
        if i < 0:
            i += len(self)
        return _rect_len(poly, self._rects.get(i))


def _device_contours(masks: torch.Tensor, max_pts: Optional[int], strategy: str, want_parts: bool, orig_hw: Optional[Tuple[int, int]] = None):
    """The device trace of Masks.xy and predict_clip: the LDS pass (mask_contours_device) over all masks, then whatever it declined - a
    polygon, or with `orig_hw` a rectangle left at (-1, -1) - through the large path (mask_contours_large_device) in ONE further call,
    with the point capacity the first call ran with. Nothing more is launched when nothing was declined. -> (polys, rects, parts or
    None); what is still None goes to the host trace. Under "all_merged" both calls bridge the contours on the device as well, and
    parts[t] is None wherever they did: lengths come back only with a list the device bridge declined (_finish_contour bridges it)."""
    got = mask_contours_device(masks, max_pts=max_pts, strategy=strategy, want_parts=want_parts, orig_hw=orig_hw)
    polys, rects = got[0], got[1]
    parts = got[2] if want_parts else None
    need = [t for t in range(len(polys)) if polys[t] is None or (orig_hw is not None and rects is not None and rects[t][0] < 0)]
    if not need or int(masks.shape[1]) > LARGE_MAX_DIM or int(masks.shape[2]) > LARGE_MAX_DIM:
        return polys, rects, parts
    sub = masks if len(need) == len(polys) else masks[torch.as_tensor(need, device=masks.device)]
    big = mask_contours_large_device(sub, max_pts=getattr(polys, "max_pts", None) or max_pts, strategy=strategy, want_parts=want_parts, orig_hw=orig_hw)
    for q, t in enumerate(need):
        if big[0][q] is None:
            continue
        polys[t] = big[0][q]
        rects[t] = big[1][q]
        if want_parts:
            parts[t] = big[2][q]
    return polys, rects, parts


def _finish_contour(poly, rect, parts, strategy: str, host_mask, mask_hw: Tuple[int, int], orig_shape: Tuple[int, int], rect_in_orig: bool = False):
    """What follows the device trace of one mask (Masks.xy and YOLO.predict_clip): poly / rect / parts as mask_contours_device gives them
    for that mask (poly None: no device pass, or the device declined), the "all_merged" bridge, the host trace of `host_mask()` (bool
    [mh,mw]) where there is no device polygon, and the scale to original-image pixels. -> (float32 [m,2] polygon, (long, short) device
    rectangle or None; the device rectangle is of the polygon in mask pixels, so it is kept only when those are the original's - or when
    `rect_in_orig`: it was measured on the polygon already scaled to original-image pixels (mask_contours_device(orig_hw=...)); a declined
    one, (-1, -1), is dropped)."""
    if poly is not None and strategy == "all_merged" and parts is not None and len(parts) > 1:
        cuts = np.cumsum(parts)[:-1]
        poly = hostops.merge_contours(np.split(poly, cuts)).astype(np.int32)
    if poly is None:
        poly = hostops.mask_polygon(host_mask(), strategy)
        rect = None
    if rect_in_orig:
        rect = (float(rect[0]), float(rect[1])) if rect is not None and rect[0] >= 0 else None
    else:
        rect = (float(rect[0]), float(rect[1])) if rect is not None and tuple(mask_hw) == tuple(orig_shape) else None
    if poly.shape[0] and tuple(mask_hw) != tuple(orig_shape):
        poly = hostops.scale_coords(tuple(mask_hw), poly, orig_shape)
    return poly.astype(np.float32), rect


def _rect_len(poly: np.ndarray, rect) -> Tuple[float, float]:
    """get_coord_min_rect_len(poly), from the device rectangle `rect` = (long, short) when there is one and the polygon has >= 3 points."""
    if rect is None or len(poly) < 3:
        return hostops.get_coord_min_rect_len(poly)
    length, width = rect
    if width == 0:
        width = 1
    return length, length / width


class _LazyPolygons:
    """What `Masks.xy` returns: behaves like the list of polygons ultralytics builds (len, indexing, slicing, iteration), but a
    polygon is traced only when it is asked for."""

    def __init__(self, masks: Masks):
        self._m = masks

    def __len__(self):
        return len(self._m)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._m._contour(j) for j in range(*i.indices(len(self._m)))]
        return self._m._contour(int(i))

    def __iter__(self):
        return (self._m._contour(j) for j in range(len(self._m)))


class Results:
    def __init__(self, orig_img: np.ndarray, boxes: Boxes, masks: Optional[Masks], names: Dict[int, str], path: str = ""):
        self.orig_img = orig_img
        self.orig_shape = tuple(orig_img.shape[:2])
        self.boxes = boxes
        self.masks = masks
        self.names = names
        self.path = path

    def __len__(self):
        return len(self.boxes)

    def cpu(self):
        return Results(self.orig_img, self.boxes.cpu(), self.masks.cpu() if self.masks is not None else None, self.names, self.path)

    def numpy(self):
        return Results(self.orig_img, self.boxes.numpy(), self.masks.numpy() if self.masks is not None else None, self.names, self.path)


class ClipResults(tuple):
    """What YOLO.predict_clip returns: unpacks as `boxes, coords, lens` - the app's yolo_pred_xyxy, coord_xys and lens (yolo_seg/app.py:93-113)
    - and also carries, per frame, `detected` (a row above conf), `conf` (its score, or None) and `xyxy` (its float32 [4] box in original-image
    pixels, or None)."""

    def __new__(cls, boxes, coords, lens, detected, conf, xyxy):
        self = super().__new__(cls, (boxes, coords, lens))
        self.detected, self.conf, self.xyxy = detected, conf, xyxy
        return self

    @property
    def boxes(self):
        return self[0]

    @property
    def coords(self):
        return self[1]

    @property
    def lens(self):
        return self[2]


def _clip_frames(frames, dev: torch.device, what: str):
    """The clip argument of YOLO.predict_id_mask_clip, checked as predict_clip checks its own and in its words: a list of BGR uint8 HWC
    ndarrays of one shape, or a uint8 CUDA tensor [N,H,W,3] on `dev`. -> (on_dev, frames (a list, or the tensor), N, H, W); raises before
    any engine is built."""
    on_dev = isinstance(frames, torch.Tensor)
    if on_dev:
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise TypeError(f"{what} expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
        if frames.device != dev:
            raise ValueError(f"frames are on {frames.device}, the engine on {dev}")
        N, H, W = (int(v) for v in frames.shape[:3])
    else:
        frames = list(frames)
        N = len(frames)
        for f in frames:
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise TypeError(f"{what} expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
            if f.shape != frames[0].shape:
                raise ValueError(f"frames differ in shape: {f.shape} vs {frames[0].shape}")
        H, W = (int(v) for v in frames[0].shape[:2]) if N else (0, 0)
    return on_dev, frames, N, H, W


class _ModelHandle:
    """What callers touch through `yolo.model`: `.parameters()` for the device and an idempotent `.to()`
    (reference yolo_seg/yolo_with_deva.py:42,129-130 moves the model every frame)."""

    def __init__(self, owner: "YOLO"):
        self._owner = owner
        self.names = owner.names

    def parameters(self):
        yield self._owner._device_token()

    def to(self, device=None, *a, **k):
        self._owner._set_device(device)
        return self

    def eval(self):
        return self

    def fuse(self, *a, **k):
        return self


class YOLO:
    """Drop-in for `ultralytics.YOLO` on the predict path (reference yolo_seg/app.py:45-50,91; yolo_seg/yolo_with_deva.py:51,226) of YOLOv10
    detect / v10-seg checkpoints and of the YOLOv8-seg / YOLO11-seg checkpoints the reference's UI offers (yolo_seg/app.py:218-223); family,
    variant, class count and task are read from the checkpoint's state dict.

    model: path to an ultralytics-layout `.pt` (read without ultralytics, weights.py), or "synthetic:<n|s|m|b|l|x>[-seg]"
    (seeded weights, for tests/benchmarks: no checkpoint exists offline)."""

    def __init__(self, model: Union[str, os.PathLike] = "yolov10s.pt", task: Optional[str] = None, dtype: str = "bf16",
                 device: Optional[Union[int, str, torch.device]] = None, nc: int = 80, seed: int = 0, attention: str = "auto",
                 attention_f32: Optional[str] = None):
        self.ckpt_path = str(model)
        self.dtype = dtype
        if attention not in ATTENTION_FORMS:
            raise ValueError(f"attention={attention!r}: one of {sorted(ATTENTION_FORMS)}")
        self.attention = attention          # "stream" / "stream_wide": the PSA block's streaming kernels (Engine.set_attention_form)
        if attention_f32 is not None and attention_f32 not in ATTENTION_F32 and attention_f32 not in ATTENTION_F32_WIDE:
            raise ValueError(f"attention_f32={attention_f32!r}: one of {sorted(ATTENTION_F32) + sorted(ATTENTION_F32_WIDE)}")
        self.attention_f32 = attention_f32  # "stream" / "stream_wide": fp32 engines' streaming attention kernels past 400 tokens (Engine.set_attention_f32); None: the engine's default
        self.family = "v10"
        if self.ckpt_path.startswith("synthetic:"):
            spec = self.ckpt_path.split(":", 1)[1]              # "s", "s-seg" (YOLOv10) ; "v8n-seg", "11x-seg" (the app's families)
            base = spec.split("-")[0]
            self.seg = spec.endswith("-seg")
            self.nc = nc
            if base[:2] in ("v8", "11"):
                from .weights import synthetic_state_family
                self.family, self.variant = base[:2], base[2:]
                if not self.seg:
                    raise ValueError("the v8 / 11 families are built as segmentation models")
                self._state = synthetic_state_family(self.family, self.variant, nc, seed=seed)
            else:
                self.variant = base
                self._state = synthetic_state(self.variant, nc, self.seg, seed=seed)
            self.names = {i: str(i) for i in range(nc)}
        else:
            if not os.path.isfile(self.ckpt_path):
                raise FileNotFoundError(f"{self.ckpt_path}: no such checkpoint (nothing is downloaded)")
            st, meta = read_ultralytics_pt(self.ckpt_path)
            if meta.get("family") is None or meta.get("variant") is None or meta.get("nc") is None:
                raise ValueError(f"{self.ckpt_path}: not a checkpoint this engine understands (YOLOv10 detect / v10-seg, "
                                 "YOLOv8-seg, YOLO11-seg)")
            if meta["family"] != "v10" and not meta["seg"]:
                raise ValueError(f"{self.ckpt_path}: YOLOv8 / YOLO11 detect-only checkpoints are not built; the reference uses the -seg models")
            self.family = meta["family"]
            self.variant, self.seg, self.nc = meta["variant"], bool(meta["seg"]), int(meta["nc"])
            self._state = st
            names = meta.get("names")
            self.names = dict(names) if isinstance(names, dict) else {i: str(i) for i in range(self.nc)}
        if task == "segment" and not self.seg:
            raise ValueError("task='segment' but the checkpoint has no Proto/cv4 head")
        self.task = "segment" if self.seg else "detect"
        self._dev_index: Optional[int] = None
        self._set_device(device)
        self.model = _ModelHandle(self)

    # -- device / engine -----------------------------------------------------------------------------------------
    def _set_device(self, device) -> None:
        if device is None or device == "":
            idx = self._dev_index if self._dev_index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
        else:
            d = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            if d.type != "cuda":
                raise ValueError(f"device={device!r}: this engine runs on MI355X GPUs only (device='cuda' / 'cuda:N' / N)")
            idx = d.index if d.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._dev_index = int(idx)

    def _device_token(self) -> torch.Tensor:
        return torch.empty(0, device=torch.device("cuda", self._dev_index))

    def _engine(self) -> Engine:
        # the reference rebuilds the model on every request (yolo_seg/app.py:45): keep engines per (ckpt, mtime, ...)
        try:
            mt = os.path.getmtime(self.ckpt_path)
        except OSError:
            mt = 0.0
        key = (self.ckpt_path, mt, self.family, self.variant, self.nc, self.seg, self.dtype, self._dev_index, self.attention, self.attention_f32)
        eng = _ENGINE_CACHE.get(key)
        if eng is None:
            eng = Engine(self.variant, self.nc, self.seg, self.dtype, self._dev_index, state=self._state, family=self.family, attention=self.attention,
                         attention_f32=self.attention_f32)
            _ENGINE_CACHE[key] = eng
        return eng

    # -- predict ---------------------------------------------------------------------------------------------------
    def _class_ids(self, classes) -> Optional[List[int]]:
        """predict(classes=): None, an int or a sequence of ints -> None or a list of class ids, checked against the model's classes"""
        if classes is None:
            return None
        seq = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
        nc = self.nc
        ids = []
        for c in seq:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
                raise TypeError(f"classes must be an int or a sequence of ints (got {c!r})")
            if not 0 <= int(c) < nc:
                raise ValueError(f"classes: {int(c)} is not a class of this model (it has {nc}: 0..{nc - 1})")
            ids.append(int(c))
        return ids or None                                            # (ultralytics treats an empty list as no filter)

    @staticmethod
    def _max_nms(max_nms) -> int:
        if max_nms is None:
            return 16384
        if isinstance(max_nms, bool) or not isinstance(max_nms, (int, np.integer)) or int(max_nms) < 1:
            raise ValueError(f"max_nms must be a positive int (got {max_nms!r}); ultralytics' value is 30000")
        return int(max_nms)

    def __call__(self, source=None, **kw):
        return self.predict(source, **kw)

    def predict(self, source=None, conf: float = 0.25, retina_masks: bool = False, device=None, imgsz: int = 640,
                max_det: int = 300, stream: bool = False, verbose: bool = False, iou: float = 0.7, classes=None,
                agnostic_nms: bool = False, max_nms: Optional[int] = None, **ignored) -> List[Results]:
        """classes / agnostic_nms / max_nms: ultralytics' arguments of the same names. v8 / 11: they steer the NMS inside the forward
        (Engine.set_nms_options; max_nms None keeps this engine's 16384, 30000 is ultralytics' value). v10 has no NMS: `classes` filters
        the rows that pass `conf` on the host, before masks are made (ultralytics' end-to-end branch); the other two have no effect."""
        if source is None:
            raise ValueError("predict() needs a source (ndarray BGR HWC uint8, PIL.Image, path or a list of them)")
        class_ids = self._class_ids(classes)
        if device is not None:
            self._set_device(device)
        imgs, paths = hostops.load_sources(source)                    # list of BGR uint8 HWC (ndarray => taken as BGR)
        eng = self._engine()
        if self.family != "v10":
            eng.set_nms(conf, iou)                                    # v8 / 11: conf filter + NMS run inside the forward
            eng.set_nms_options(class_ids, agnostic_nms, self._max_nms(max_nms))
        wanted = torch.tensor(class_ids, dtype=torch.float32) if (self.family == "v10" and class_ids is not None) else None
        dev = torch.device("cuda", self._dev_index)
        results: List[Results] = []
        # frames that letterbox to the same shape run as one batch
        groups: Dict[Tuple[int, int], List[int]] = {}
        geos = []
        for i, im in enumerate(imgs):
            geo = hostops.letterbox_geometry(im.shape[0], im.shape[1], imgsz)
            geos.append(geo)
            groups.setdefault((geo["out_h"], geo["out_w"]), []).append(i)
        out_by_index: Dict[int, Results] = {}
        # ... in runs of at most the engine's largest batch at that shape (Engine.max_batch: large inputs reach the kernels' 32-bit byte offsets)
        runs: List[Tuple[Tuple[int, int], List[int]]] = []
        for (H, W), idxs in groups.items():
            mb = eng.max_batch(H, W)
            runs += [((H, W), idxs[s0:s0 + mb]) for s0 in range(0, len(idxs), mb)]
        for (H, W), idxs in runs:
            # the raw frame goes up once; resize + pad-114 run on the device straight into the batch tensor (yp_letterbox)
            # (one persistent batch buffer per shape: the engine's hipGraph is specialised on the input pointer)
            bcache = self.__dict__.setdefault("_batch_cache", {})
            bkey = (self._dev_index, len(idxs), H, W)
            batch = bcache.get(bkey)
            if batch is None:
                batch = bcache[bkey] = torch.empty((len(idxs), H, W, 3), dtype=torch.uint8, device=dev)
            for bi, i in enumerate(idxs):
                raw = torch.from_numpy(np.ascontiguousarray(imgs[i])).to(dev, non_blocking=True)
                letterbox_device(raw, geos[i], out=batch[bi])
            # one output set per batch size (no allocation per call); everything handed to the caller below is copied out of it
            cache = self.__dict__.setdefault("_out_cache", {})
            okey = (self._dev_index, len(idxs))
            # launch mode "auto": per input shape the engine times eager launches against hipGraph replay once and keeps the faster - the
            # reference's one-frame calls (yolo_seg/app.py:85-91) run eagerly (~80 kernels of a few microseconds: the graph executor's
            # per-node cost loses), batches replay. YOLOP_PREDICT_GRAPH=0 / 1 forces one mode.
            mode = os.environ.get("YOLOP_PREDICT_GRAPH", "auto")
            eng.set_graph("auto" if mode == "auto" else int(mode))
            out = eng.forward(batch, cache.get(okey))
            cache[okey] = out
            # ONE device-to-host copy of the [B,300,6] rows ends the forward; the conf filter and scale_boxes are a few dozen floats of
            # host arithmetic (a chain of tiny device ops with two boolean gathers - each a device sync - cost ~0.1 ms per frame).
            # Both heads emit their rows best first, so the rows above `conf` are a prefix and the coefficients are sliced, not gathered.
            det_host = out["det"][:len(idxs)].cpu()
            for bi, i in enumerate(idxs):
                oh, ow = imgs[i].shape[:2]
                dh = det_host[bi]
                keep = dh[:, 4] > conf                                  # strict, A.6 step 2
                if wanted is not None:                                  # v10: the class set acts on the rows above conf
                    keep &= torch.isin(dh[:, 5], wanted)
                n = int(keep.sum())
                prefix = bool(keep[:n].all())
                d = (dh[:n] if prefix else dh[keep])[:max_det].clone()
                n = int(d.shape[0])
                boxes_in = d[:, :4].clone()                              # letterboxed-input pixels
                d[:, :4] = hostops.scale_boxes_t((H, W), d[:, :4], (oh, ow))
                masks = None
                if self.seg and n > 0:
                    cf = out["coeff"][bi][:n] if prefix else out["coeff"][bi][keep.to(dev)][:max_det]
                    if retina_masks:
                        m, _, _ = eng.masks(bi, cf, d[:, :4].to(dev, non_blocking=True), (oh, ow), retina=True)
                    else:
                        m, _, _ = eng.masks(bi, cf, boxes_in.to(dev, non_blocking=True), (H, W), retina=False)
                    masks = Masks(None, (oh, ow), u8=m)
                out_by_index[i] = Results(imgs[i], Boxes(d, (oh, ow)), masks, self.names, paths[i])
        for i in range(len(imgs)):
            results.append(out_by_index[i])
        return results

    def predict_clip(self, frames, conf: float = 0.25, iou: float = 0.7, imgsz: int = 640, batch_size: int = 32, device=None,
                     retina_masks: bool = True, classes=None, agnostic_nms: bool = False, max_nms: Optional[int] = None) -> ClipResults:
        """The app's first video loop (yolo_seg/app.py:85-113: predict(frame, conf, retina_masks=True) -> best row -> masks.xy[best] ->
        get_coord_min_rect_len, with the carry-forward of the last box and length) for a whole clip of same-shape frames.
        retina_masks=False: the same loop as the speed-evaluation script runs it (dev_tools/auto_speed_calc.py:56-84: predict(frame, conf)
        without retina masks): masks at the letterboxed input size from the boxes in its pixels (yp_masks_frames_input), polygons scaled to
        the frame by hostops.scale_coords, rectangles of the scaled polygons (yp_mask_contours_scaled).

        frames: a list of BGR uint8 HWC ndarrays of one shape, or a uint8 CUDA tensor [N,H,W,3] on the engine's device. Frames run in
        contiguous chunks of B = min(batch_size, N), the last one padded to B by repeating its last frame (hostops.clip_plan), so each chunk
        is the computation predict() does on that padded chunk. Per chunk: one upload (host frames), one letterbox launch, the forward, ONE
        copy of each frame's row 0 (rows are best first: np.argmax of the scores), the strict `> conf` test and scale_boxes on the host, one
        mask per detected frame (yp_masks_frames) and one contour pass over them (MASK_POLYGON_STRATEGY; what the LDS kernel declines -
        4K masks, many blobs - goes through the large path in one further call, host trace where that declines too). -> ClipResults: `boxes, coords, lens = model.predict_clip(frames)`."""
        if not self.seg:
            raise ValueError("predict_clip needs a segmentation checkpoint (-seg): the app reads masks.xy of the best row")
        class_ids = self._class_ids(classes)
        if self.family == "v10" and class_ids is not None:
            raise ValueError("predict_clip(classes=) needs a v8 / 11 checkpoint: the v10 head picks each frame's best row on the device, before "
                             "a class set could act (use predict(classes=) per frame)")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
        retina = bool(retina_masks)
        strategy = MASK_POLYGON_STRATEGY
        if strategy not in hostops.POLYGON_STRATEGIES:
            raise ValueError(f"MASK_POLYGON_STRATEGY must be one of {hostops.POLYGON_STRATEGIES}, got {strategy!r}")
        if device is not None:
            self._set_device(device)
        dev = torch.device("cuda", self._dev_index)
        on_dev = isinstance(frames, torch.Tensor)
        if on_dev:
            if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
                raise TypeError("predict_clip expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
            if frames.device != dev:
                raise ValueError(f"frames are on {frames.device}, the engine on {dev}")
            N, H, W = (int(v) for v in frames.shape[:3])
        else:
            frames = list(frames)
            N = len(frames)
            for f in frames:
                if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                    raise TypeError("predict_clip expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
                if f.shape != frames[0].shape:
                    raise ValueError(f"frames differ in shape: {f.shape} vs {frames[0].shape}")
            H, W = (int(v) for v in frames[0].shape[:2]) if N else (0, 0)
        if N == 0:
            return ClipResults([], [], [], [], [], [])
        if H <= 0 or W <= 0:
            raise ValueError(f"empty frames ({H}x{W})")
        geo = hostops.letterbox_geometry(H, W, imgsz)
        Hl, Wl = geo["out_h"], geo["out_w"]
        eng = self._engine()
        B, chunks = hostops.clip_plan(N, min(int(batch_size), eng.max_batch(Hl, Wl)))      # (no chunk larger than the engine plans at this shape)
        if self.family != "v10":
            eng.set_nms(conf, iou)
            eng.set_nms_options(class_ids, agnostic_nms, self._max_nms(max_nms))
        mode = os.environ.get("YOLOP_PREDICT_GRAPH", "auto")
        bcache = self.__dict__.setdefault("_batch_cache", {})          # the buffer predict() uses for this shape: one hipGraph per shape
        batch = bcache.get((self._dev_index, B, Hl, Wl))
        if batch is None:
            batch = bcache[(self._dev_index, B, Hl, Wl)] = torch.empty((B, Hl, Wl, 3), dtype=torch.uint8, device=dev)
        stage = None
        if on_dev:
            frames = frames.contiguous()
        else:
            scache = self.__dict__.setdefault("_clip_stage", {})
            stage = scache.get((self._dev_index, B, H, W))
            if stage is None:
                stage = scache[(self._dev_index, B, H, W)] = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        cache = self.__dict__.setdefault("_out_cache", {})
        okey = (self._dev_index, B)

        detected: List[bool] = [False] * N
        confs: List[Optional[float]] = [None] * N
        xyxy: List[Optional[np.ndarray]] = [None] * N
        polys: List[Optional[np.ndarray]] = [None] * N
        rect_lens: List[float] = [0] * N
        for s0, c in chunks:
            if on_dev:
                src = frames[s0:s0 + c]
            else:
                for q in range(c):                                      # straight into the device staging rows: no host-side stack
                    stage[q].copy_(torch.from_numpy(np.ascontiguousarray(frames[s0 + q])), non_blocking=True)
                src = stage[:c]
            letterbox_batch_device(src, geo, out=batch[:c])
            if c < B:                                                   # pad rows: the chunk's last frame again (their results are dropped)
                batch[c:].copy_(batch[c - 1:c].expand(B - c, Hl, Wl, 3))
            eng.set_graph("auto" if mode == "auto" else int(mode))
            out = eng.forward(batch, cache.get(okey))
            cache[okey] = out
            rows = out["det"][:, 0].cpu()[:c]                           # ONE copy: row 0 of every frame (best first)
            keep = rows[:, 4] > conf                                    # strict, as predict()
            sel = [int(j) for j in torch.nonzero(keep).flatten()]
            if not sel:
                continue
            boxes = hostops.scale_boxes_t((Hl, Wl), rows[sel, :4], (H, W))
            if retina:
                m = eng.masks_frames(sel, out["coeff"], boxes.to(dev, non_blocking=True), (H, W))
                mask_hw, orig_hw = (H, W), None
            else:                                                       # process_mask from the boxes in letterboxed-input pixels
                m = eng.masks_frames(sel, out["coeff"], rows[sel, :4].to(dev, non_blocking=True), (Hl, Wl), retina=False)
                mask_hw, orig_hw = (Hl, Wl), (H, W)
            dpolys, drects, dparts = _device_contours(m, 131072, strategy, strategy == "all_merged", orig_hw)
            bnp = boxes.numpy()
            for t, j in enumerate(sel):
                i = s0 + j
                parts = dparts[t] if dparts is not None else None
                poly, rect = _finish_contour(dpolys[t], drects[t], parts, strategy, lambda t=t: m[t].cpu().numpy() > 0, mask_hw, (H, W),
                                             rect_in_orig=not retina)
                detected[i], confs[i], xyxy[i] = True, float(rows[j, 4]), bnp[t].copy()
                polys[i] = poly
                rect_lens[i] = _rect_len(poly, rect)[0]
        boxes_l, coords, lens = hostops.clip_track(detected, xyxy, polys, rect_lens, W, H)
        return ClipResults(boxes_l, coords, lens, detected, confs, xyxy)

    def predict_id_mask(self, image: np.ndarray, conf: float = 0.9, out_hw: Optional[Tuple[int, int]] = None,
                        suppress_small: bool = False, min_area: int = 100, imgsz: int = 640,
                        pre_resize: Optional[Tuple[int, int]] = None):
        """The fused body of `auto_segment` (reference yolo_seg/yolo_with_deva.py:45-86): (cv2.resize to `pre_resize` = (w,h), :45-48)
        -> predict(retina_masks=True, conf) -> masks at the fed frame's size -> (antialiased bilinear to `out_hw` if it differs,
        :71-72) -> area test -> id paint, all on the GPU: the raw frame is uploaded once.
        -> (ids int64 [h,w] cuda, kept int32 [n] cpu (id per detection, 0 = suppressed), conf [n] cpu, cls [n] cpu)"""
        if not self.seg:
            raise ValueError("auto_segment needs a segmentation checkpoint")
        imgs, _ = hostops.load_sources(image)
        im = imgs[0]
        eng = self._engine()
        dev = torch.device("cuda", self._dev_index)
        raw = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
        if pre_resize is not None and (int(pre_resize[1]), int(pre_resize[0])) != tuple(im.shape[:2]):
            nw, nh = int(pre_resize[0]), int(pre_resize[1])
            raw = letterbox_device(raw, dict(out_h=nh, out_w=nw, new_h=nh, new_w=nw, top=0, left=0))   # cv2.resize(INTER_LINEAR) on the device
        oh, ow = int(raw.shape[0]), int(raw.shape[1])
        out_hw = (oh, ow) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        geo = hostops.letterbox_geometry(oh, ow, imgsz)
        H, W = geo["out_h"], geo["out_w"]
        bcache = self.__dict__.setdefault("_batch_cache", {})
        batch = bcache.get((self._dev_index, 1, H, W))
        if batch is None:
            batch = bcache[(self._dev_index, 1, H, W)] = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        letterbox_device(raw, geo, out=batch[0])
        if self.family != "v10":
            eng.set_nms(conf, 0.7)
            eng.set_nms_options()                                     # (fixed arguments: whatever a predict(classes=...) left on the engine goes)
        mode = os.environ.get("YOLOP_PREDICT_GRAPH", "auto")             # (explicit: not whatever the last predict() left; one frame resolves to eager)
        eng.set_graph("auto" if mode == "auto" else int(mode))
        out = eng.forward(batch)
        dh = out["det"][0].cpu()                                        # (one copy; see predict())
        keep = dh[:, 4] > conf
        n = int(keep.sum())
        prefix = bool(keep[:n].all())
        d = dh[:n] if prefix else dh[keep]
        if n == 0:
            z = torch.zeros(out_hw, dtype=torch.int64, device=dev)
            e = torch.zeros(0)
            return z, torch.zeros(0, dtype=torch.int32), e, e
        boxes = hostops.scale_boxes_t((H, W), d[:, :4], (oh, ow)).to(dev, non_blocking=True)
        cf = out["coeff"][0][:n] if prefix else out["coeff"][0][keep.to(dev)]
        if out_hw == (oh, ow):
            _, ids, kept = eng.masks(0, cf, boxes, (oh, ow), retina=True, want_masks=False, want_ids=True,
                                     suppress_small=suppress_small, min_area=min_area)
        else:
            # the reference resizes each float mask to (h,w) (torchvision F.resize: antialiased bilinear), tests the float area and
            # thresholds at 0.5 (:71-79): one GPU pass (yp_id_mask_resized)
            ids, kept = eng.id_mask_resized(0, cf, boxes, (oh, ow), out_hw, suppress_small=suppress_small, min_area=min_area)
        return ids, kept.cpu(), d[:, 4].clone(), d[:, 5].clone()

    def predict_id_mask_clip(self, images, conf: float = 0.9, out_hw: Optional[Tuple[int, int]] = None, suppress_small: bool = False,
                             min_area: int = 100, imgsz: int = 640, pre_resize: Optional[Tuple[int, int]] = None, batch_size: int = 32):
        """predict_id_mask for a whole clip of same-shape frames - the detection frames of a DEVA run, which are known in advance
        (yolo_seg/yolo_with_deva.py:140,197). -> a list with predict_id_mask's 4-tuple for every frame.

        images: a list of uint8 HWC ndarrays of one shape, or a uint8 CUDA tensor [N,H,W,3] on the engine's device. Chunks and padding are
        predict_clip's (hostops.clip_plan). Per chunk: one upload (host frames), one letterbox launch per resize (`pre_resize`, then the
        model input), the forward, ONE copy of the [c,max_det,6] rows, the strict `> conf` test and scale_boxes on the host, one gather of
        the kept coefficient rows by an index built from that host copy, one upload of all boxes, and the id-mask tail of all frames
        (Engine.id_masks_frames) - in as many calls as keep each call's workspace within ID_MASKS_FRAMES_BUDGET
        (hostops.group_frames_by_workspace); a frame that exceeds it alone takes the one-frame call."""
        if not self.seg:
            raise ValueError("auto_segment needs a segmentation checkpoint")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
        dev = torch.device("cuda", self._dev_index)
        on_dev, frames, N, H, W = _clip_frames(images, dev, "predict_id_mask_clip")
        if N == 0:
            return []
        if H <= 0 or W <= 0:
            raise ValueError(f"empty frames ({H}x{W})")
        pre_geo = None
        oh, ow = H, W
        if pre_resize is not None and (int(pre_resize[1]), int(pre_resize[0])) != (H, W):
            ow, oh = int(pre_resize[0]), int(pre_resize[1])
            pre_geo = dict(out_h=oh, out_w=ow, new_h=oh, new_w=ow, top=0, left=0)          # cv2.resize(INTER_LINEAR) on the device
        out_hw = (oh, ow) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        geo = hostops.letterbox_geometry(oh, ow, imgsz)
        Hl, Wl = geo["out_h"], geo["out_w"]
        eng = self._engine()
        B, chunks = hostops.clip_plan(N, min(int(batch_size), eng.max_batch(Hl, Wl)))
        if self.family != "v10":
            eng.set_nms(conf, 0.7)
            eng.set_nms_options()                                     # (fixed arguments: whatever a predict(classes=...) left on the engine goes)
        mode = os.environ.get("YOLOP_PREDICT_GRAPH", "auto")

        def buffer(name, shape):
            cache = self.__dict__.setdefault(name, {})
            key = (self._dev_index,) + shape
            if key not in cache:
                cache[key] = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
            return cache[key]

        batch = buffer("_batch_cache", (B, Hl, Wl))                     # the buffer predict() uses for this shape: one hipGraph per shape
        stage = None if on_dev else buffer("_clip_stage", (B, H, W))
        shrunk = buffer("_clip_pre", (B, oh, ow)) if pre_geo is not None else None
        if on_dev:
            frames = frames.contiguous()
        cache = self.__dict__.setdefault("_out_cache", {})
        okey = (self._dev_index, B)
        same = out_hw == (oh, ow)
        results = []
        for s0, c in chunks:
            if on_dev:
                src = frames[s0:s0 + c]
            else:
                for q in range(c):
                    stage[q].copy_(torch.from_numpy(np.ascontiguousarray(frames[s0 + q])), non_blocking=True)
                src = stage[:c]
            if pre_geo is not None:
                src = letterbox_batch_device(src, pre_geo, out=shrunk[:c])
            letterbox_batch_device(src, geo, out=batch[:c])
            if c < B:                                                   # pad rows: the chunk's last frame again (their results are dropped)
                batch[c:].copy_(batch[c - 1:c].expand(B - c, Hl, Wl, 3))
            eng.set_graph("auto" if mode == "auto" else int(mode))
            out = eng.forward(batch, cache.get(okey))
            cache[okey] = out
            det_host = out["det"][:c].cpu()                             # ONE copy: every row of the chunk's frames
            max_det = int(det_host.shape[1])
            rows, gather, counts = [], [], []
            for j in range(c):
                dh = det_host[j]
                keep = torch.nonzero(dh[:, 4] > conf).flatten()         # strict, as predict_id_mask
                rows.append(dh[keep])
                gather.append(keep + j * max_det)
                counts.append(int(keep.shape[0]))
            d_all = torch.cat(rows)
            n_all = int(d_all.shape[0])
            boxes = hostops.scale_boxes_t((Hl, Wl), d_all[:, :4], (oh, ow)).to(dev, non_blocking=True)
            coeff = out["coeff"].view(-1, 32).index_select(0, torch.cat(gather).to(dev, non_blocking=True)) if n_all else \
                torch.empty((0, 32), dtype=torch.float32, device=dev)
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            ids_of, kept_of = [None] * c, [None] * c
            groups = hostops.group_frames_by_workspace(counts, lambda n, k: eng.id_masks_frames_workspace(n, k, (oh, ow), out_hw),
                                                       ID_MASKS_FRAMES_BUDGET)
            for batched, js in groups:
                r0, r1 = int(off[js[0]]), int(off[js[-1] + 1])
                if batched:
                    ids, kept = eng.id_masks_frames(js, [counts[j] for j in js], coeff[r0:r1], boxes[r0:r1], (oh, ow), out_hw,
                                                    suppress_small=suppress_small, min_area=min_area)
                    kept = kept.cpu()
                    for t, j in enumerate(js):
                        ids_of[j], kept_of[j] = ids[t], kept[int(off[j]) - r0:int(off[j + 1]) - r0].clone()
                else:                                                   # alone beyond the budget: the one-frame call
                    j = js[0]
                    if same:
                        _, ids, kept = eng.masks(j, coeff[r0:r1], boxes[r0:r1], (oh, ow), retina=True, want_masks=False, want_ids=True,
                                                 suppress_small=suppress_small, min_area=min_area)
                    else:
                        ids, kept = eng.id_mask_resized(j, coeff[r0:r1], boxes[r0:r1], (oh, ow), out_hw, suppress_small=suppress_small,
                                                        min_area=min_area)
                    ids_of[j], kept_of[j] = ids, kept.cpu()
            for j in range(c):
                d = rows[j]
                results.append((ids_of[j], kept_of[j], d[:, 4].clone(), d[:, 5].clone()))
        return results
