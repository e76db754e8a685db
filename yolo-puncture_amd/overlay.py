"""The app's output frames on the device (yp_overlay_frames): loop #2 of the reference's video path (yolo_seg/app.py:131-191) pastes the
U^2-Net crop mask, draws the ROI rectangle and the label (create_roi_mask, yolo_seg/utils/mask_tools.py:100-129) and adds both to the frame
with two saturating cv2.addWeighted calls. `overlay_clip` is that arithmetic for a clip whose frames and masks are already on the GPU,
`render_labels` makes the label bitmaps with Pillow, `render_clip` is the loop body for a whole clip: U^2-Net chunk by chunk, the overlay
straight from the crop masks, and the finished frames handed to the host while the next chunk runs. hostops.overlay_frame is the numpy
statement of the same frame. The ROI / label state machine of the loop (app.py:134-176) is scalar work and stays with the caller.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .engine import YolopError, load_library
from .u2net import U2NetEngine, clip_chunks, crop_window

OVERLAY_PARAMS = 13       # YP_OVERLAY_PARAMS: x_lt, y_lt, x_rd, y_rd, x1, y1, x2, y2, lx, ly, lw, lh, crop


def _is_frames(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[-1] == 3 and t.is_contiguous()


def overlay_clip(frames: torch.Tensor, masks: Optional[torch.Tensor], windows, rois, labels: Optional[torch.Tensor] = None, label_xy=None, *,
                 crop_index=None, out: Optional[torch.Tensor] = None, inplace: bool = False, color: Sequence[int] = (0, 0, 255)) -> torch.Tensor:
    """out[n] = hostops.overlay_frame(frames[n], masks[crop_index[n]], windows[n], rois[n], labels[n], label_xy[n], color), on the device, in
    one launch.

    frames: contiguous uint8 CUDA [N,H,W,3] (BGR). masks: uint8 CUDA [B,ch,cw] crop masks (U2NetEngine.forward_crops; the window at the
    top-left, ch x cw at least its size) with `windows` int [N,4] = (x_lt, y_lt, x_rd, y_rd) per frame and `crop_index` int [N] (default
    0..N-1); or a full-frame mask [N,H,W] with windows=None; or None (no mask). rois int [N,4] = (x1, y1, x2, y2), both corners on the
    outline. labels: uint8 CUDA [N,LH,LW] coverage bitmaps (render_labels) with label_xy int [N,2] = (lx, ly), the top-left of each, or
    [N,4] = (lx, ly, lw, lh) when a frame uses only the top-left lw x lh of its bitmap (0: that frame has no label).
    inplace=True writes into `frames` (only the bytes the mask window, the rectangle or the label meet are touched) and returns it;
    otherwise the result goes to `out` (same shape, no overlap with frames) or a new tensor, and every byte is read and written once."""
    if not _is_frames(frames):
        raise TypeError("overlay_clip expects contiguous uint8 CUDA frames [N,H,W,3]")
    N, H, W, _ = (int(v) for v in frames.shape)
    dev = frames.device
    rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
    if rois.shape[0] != N:
        raise ValueError(f"{N} frames but {rois.shape[0]} rois")
    par = np.zeros((N, OVERLAY_PARAMS), dtype=np.int32)
    par[:, 4:8] = rois
    if masks is None:
        B = ch = cw = 0
    else:
        if not (isinstance(masks, torch.Tensor) and masks.device == dev and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous()):
            raise TypeError(f"masks must be a contiguous uint8 tensor [B,ch,cw] or [N,H,W] on {dev}")
        B, ch, cw = (int(v) for v in masks.shape)
        if windows is None:
            if (B, ch, cw) != (N, H, W):
                raise ValueError(f"masks without windows must be [{N},{H},{W}], got {tuple(masks.shape)}")
            par[:, 0:4] = (0, 0, W, H)
        else:
            win = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
            if win.shape[0] != N:
                raise ValueError(f"{N} frames but {win.shape[0]} windows")
            par[:, 0:4] = win
        idx = np.arange(N) if crop_index is None else np.asarray(crop_index, dtype=np.int64).reshape(-1)
        if idx.shape[0] != N:
            raise ValueError(f"{N} frames but {idx.shape[0]} crop indices")
        par[:, 12] = idx
    if labels is None:
        LH = LW = 0
    else:
        if not (isinstance(labels, torch.Tensor) and labels.device == dev and labels.dtype == torch.uint8 and labels.dim() == 3
                and labels.shape[0] == N and labels.is_contiguous()):
            raise TypeError(f"labels must be a contiguous uint8 tensor [{N},LH,LW] on {dev}")
        LH, LW = int(labels.shape[1]), int(labels.shape[2])
        xy = np.asarray(label_xy, dtype=np.int64).reshape(N, -1) if label_xy is not None else None
        if xy is None or xy.shape[1] not in (2, 4):
            raise ValueError("labels need label_xy [N,2] = (lx, ly) or [N,4] = (lx, ly, lw, lh)")
        par[:, 8:10] = xy[:, :2]
        par[:, 10:12] = xy[:, 2:4] if xy.shape[1] == 4 else (LW, LH)
    if inplace:
        if out is not None and out.data_ptr() != frames.data_ptr():
            raise ValueError("inplace=True writes into frames: pass no other out")
        out = frames
    elif out is None:
        out = torch.empty_like(frames)
    elif not (_is_frames(out) and out.shape == frames.shape and out.device == dev):
        raise TypeError(f"out must be a contiguous uint8 tensor {tuple(frames.shape)} on {dev}")
    elif out.data_ptr() == frames.data_ptr():
        raise ValueError("out is frames: say inplace=True")
    col = (C.c_uint8 * 3)(*[int(v) for v in color])
    lib = load_library()
    with torch.cuda.device(dev):
        rc = lib.yp_overlay_frames(C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()), N, H, W,
                                   C.c_void_p(masks.data_ptr() if B else None), B, ch, cw, par.ctypes.data_as(C.c_void_p),
                                   C.c_void_p(labels.data_ptr() if LH * LW else None), LH, LW, C.cast(col, C.c_void_p),
                                   C.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream)))
    if rc < 0:
        raise YolopError(f"libyolop error {rc}: {lib.yp_last_error().decode()}")
    return out


def _default_font():
    from PIL import ImageFont
    try:
        return ImageFont.load_default(size=28)         # about the cap height of FONT_HERSHEY_COMPLEX at scale 1
    except (TypeError, OSError):                       # a Pillow without FreeType has only its bitmap font
        return ImageFont.load_default()


def label_origin(x1: int, y1: int, text_h: int) -> Tuple[int, int]:
    """create_roi_mask's placement (mask_tools.py:124-125): the text starts at x1; its baseline is y1 - 10 if that is > 10, else
    y1 + 10 + text_h, text_h being the height of the text above its baseline."""
    return int(x1), (int(y1) - 10 if int(y1) - 10 > 10 else int(y1) + 10 + int(text_h))


def render_labels(texts: Sequence[Optional[str]], rois, font=None) -> Tuple[np.ndarray, np.ndarray]:
    """The labels of a clip as coverage bitmaps -> (bitmaps uint8 [N,LH,LW], label_xy int32 [N,4] = (lx, ly, lw, lh)), what overlay_clip and
    render_clip take. Text n is drawn with Pillow (`font`: a PIL ImageFont, default Pillow's own at 28 px) with its left end at x1 and its
    baseline where create_roi_mask puts it (label_origin); lw x lh is the ink box of the text, (lx, ly) its top-left in the frame, and an
    empty or None text has lw = lh = 0. The glyphs are Pillow's, not cv2's Hershey font: a caller who has cv2 gets the reference's look by
    drawing `cv2.putText(canvas, label, (0, text_h), cv2.FONT_HERSHEY_COMPLEX, 1, (0, 0, 255), 2, cv2.LINE_AA)` on a small zero canvas and
    passing its red channel as the bitmap, with (lx, ly) = (text_x, text_y - text_h)."""
    from PIL import Image, ImageDraw
    font = font or _default_font()
    rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
    texts = list(texts)
    if len(texts) != rois.shape[0]:
        raise ValueError(f"{len(texts)} texts but {rois.shape[0]} rois")
    try:                                               # FreeType fonts know their baseline; Pillow's bitmap font is drawn from its top
        ascent = int(font.getmetrics()[0])
    except AttributeError:
        ascent = None
    tiles: List[Optional[np.ndarray]] = []
    xy = np.zeros((len(texts), 4), dtype=np.int32)
    for n, (text, roi) in enumerate(zip(texts, rois)):
        if not text:
            tiles.append(None)
            continue
        l, t, r, b = (int(v) for v in font.getbbox(text))           # ink box with the pen at (0, 0), top-anchored
        base = ascent if ascent is not None else b                  # the baseline's y in that box
        if r <= l or b <= t:
            tiles.append(None)
            continue
        im = Image.new("L", (r - l, b - t), 0)
        ImageDraw.Draw(im).text((-l, -t), text, fill=255, font=font)
        tiles.append(np.asarray(im, dtype=np.uint8))
        tx, ty = label_origin(roi[0], roi[1], base - t)
        xy[n] = (tx + l, ty - (base - t), r - l, b - t)
    LH = max([t.shape[0] for t in tiles if t is not None], default=0)
    LW = max([t.shape[1] for t in tiles if t is not None], default=0)
    bitmaps = np.zeros((len(texts), LH, LW), dtype=np.uint8)
    for n, t in enumerate(tiles):
        if t is not None:
            bitmaps[n, :t.shape[0], :t.shape[1]] = t
    return bitmaps, xy


def frame_runs(shapes: Sequence[Tuple[int, int]], batch_size: int = 16) -> List[Tuple[Tuple[int, int], int, int]]:
    """Chunks of a clip in frame order -> [((ch, cw), first, end), ...]: every maximal run of consecutive frames with one crop shape, split
    by clip_chunks (power-of-two sizes, the largest first), so that the chunks' frames are contiguous and ascending."""
    out = []
    s = 0
    while s < len(shapes):
        e = s
        while e < len(shapes) and tuple(shapes[e]) == tuple(shapes[s]):
            e += 1
        for shape, idx in clip_chunks(shapes[s:e], batch_size):
            out.append((shape, s + idx[0], s + idx[-1] + 1))
        s = e
    return out


def render_clip(unet_model: U2NetEngine, frames, boxes, rois, labels=None, *, batch_size: int = 16, to_host: bool = True,
                color: Sequence[int] = (0, 0, 255)) -> Union[Iterator[Tuple[int, np.ndarray]], torch.Tensor]:
    """The body of the app's loop #2 for a clip: crop_frame + unet_predict per frame (U2NetEngine.forward_crops, chunk by chunk), then the
    mask paste, create_roi_mask and the two addWeighted calls as one overlay launch per chunk, straight from the crop masks (no full-frame
    mask is written).

    frames: a list of same-shape BGR uint8 HWC ndarrays (uploaded one chunk at a time and overlaid in place there) or a uint8 CUDA tensor
    [N,H,W,3] (left as it is); boxes: the app's yolo_pred_xyxy, one per frame; rois: (x1, y1, x2, y2) per frame; labels: None, one text per
    frame (render_labels) or render_labels' own (bitmaps, label_xy) pair. Frames the app skips are left out by the caller.
    to_host=True: a generator of (index, ndarray [H,W,3]) in frame order. The ndarray is a view of one of two pinned staging buffers and
    stays valid until the next frame is asked for (write or copy it first); the download of a chunk runs on a side stream while the next
    chunk's network runs. to_host=False: the uint8 CUDA tensor [N,H,W,3]."""
    on_dev = isinstance(frames, torch.Tensor)
    if on_dev:
        if not _is_frames(frames):
            raise TypeError("render_clip expects BGR uint8 HWC ndarrays or a contiguous uint8 CUDA tensor [N,H,W,3]")
        N, H, W = (int(v) for v in frames.shape[:3])
    else:
        frames = list(frames)
        N = len(frames)
        for f in frames:
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise TypeError("render_clip expects BGR uint8 HWC ndarrays or a contiguous uint8 CUDA tensor [N,H,W,3]")
            if f.shape != frames[0].shape:
                raise ValueError(f"frames differ in shape: {f.shape} vs {frames[0].shape}")
        H, W = (int(v) for v in frames[0].shape[:2]) if N else (0, 0)
    boxes = list(boxes)
    rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
    if len(boxes) != N or rois.shape[0] != N:
        raise ValueError(f"{N} frames but {len(boxes)} boxes and {rois.shape[0]} rois")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    dev = torch.device("cuda", unet_model.device_index)
    if on_dev and frames.device != dev:
        raise ValueError(f"frames are on {frames.device}, the engine on {dev}")
    geo = [crop_window(b, H, W) for b in boxes]
    for i, ((x1, y1, x2, y2), _) in enumerate(geo):
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"frame {i}: box {tuple(boxes[i])} has its centre outside the {W}x{H} frame")
    bitmaps = label_xy = None
    if labels is not None:
        if isinstance(labels, tuple) and len(labels) == 2 and not isinstance(labels[0], str):
            bitmaps, label_xy = labels
        else:
            bitmaps, label_xy = render_labels(labels, rois)
        label_xy = np.asarray(label_xy).reshape(N, -1)
        if not isinstance(bitmaps, torch.Tensor):
            bitmaps = torch.from_numpy(np.ascontiguousarray(bitmaps))
        bitmaps = bitmaps.to(dev)
        if bitmaps.shape[0] != N:
            raise ValueError(f"{N} frames but {bitmaps.shape[0]} label bitmaps")
        if bitmaps.shape[1] * bitmaps.shape[2] == 0:
            bitmaps = label_xy = None
    chunks = frame_runs([g[1] for g in geo], batch_size)

    def overlay_chunk(shape, s, e, out):
        """network + overlay of frames [s, e) on the current stream, into `out` or (out=None, host frames) in place in the uploaded chunk
        -> the uint8 CUDA tensor [e-s,H,W,3] that holds the result"""
        win = np.array([geo[i][0] for i in range(s, e)], dtype=np.int32)
        if on_dev:
            src, fidx = frames, np.arange(s, e, dtype=np.int32)
        else:
            src, fidx = torch.from_numpy(np.stack(frames[s:e])).to(dev), np.arange(e - s, dtype=np.int32)
        _, cm, _ = unet_model.forward_crops(src, win, fidx, shape, want_prob=False)
        lab = dict(labels=bitmaps[s:e], label_xy=label_xy[s:e]) if bitmaps is not None else {}
        if on_dev:
            src = frames[s:e]
        if out is None:                                 # an uploaded chunk is ours to write into
            return overlay_clip(src, cm, win, rois[s:e], inplace=True, color=color, **lab)
        return overlay_clip(src, cm, win, rois[s:e], out=out, color=color, **lab)

    if not to_host:
        result = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for shape, s, e in chunks:
                overlay_chunk(shape, s, e, result[s:e])
        return result
    return _stream_to_host(chunks, overlay_chunk, on_dev, dev, H, W)


def _stream_to_host(chunks, overlay_chunk, on_dev: bool, dev, H: int, W: int) -> Iterator[Tuple[int, np.ndarray]]:
    """Two slots (device result, pinned host buffer, event): chunk k's download runs on the side stream while chunk k+1's network and
    overlay are enqueued and run on the main one; chunk k's frames are handed out once its event has passed."""
    if not chunks:
        return
    cap = max(e - s for _, s, e in chunks)
    with torch.cuda.device(dev):
        main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        pinned = [torch.empty((cap, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        held = [torch.empty((cap, H, W, 3), dtype=torch.uint8, device=dev) if on_dev else None for _ in range(2)]
        copied = [torch.cuda.Event() for _ in range(2)]
        busy = [False, False]

        def enqueue(k):
            shape, s, e = chunks[k]
            slot = k % 2
            if busy[slot]:
                main.wait_event(copied[slot])           # the slot's device buffer is written again only after its download
            done = overlay_chunk(shape, s, e, held[slot][:e - s] if on_dev else None)
            if not on_dev:
                held[slot] = done                       # keeps the chunk alive until its download has run
            side.wait_stream(main)
            with torch.cuda.stream(side):
                pinned[slot][:e - s].copy_(done, non_blocking=True)
                copied[slot].record(side)
            busy[slot] = True

        enqueue(0)
        for k, (_, s, e) in enumerate(chunks):
            if k + 1 < len(chunks):
                enqueue(k + 1)
            copied[k % 2].synchronize()
            host = pinned[k % 2].numpy()
            for i in range(s, e):
                yield i, host[i - s]
