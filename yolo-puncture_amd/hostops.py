"""Host-side steps around the engine: source loading, LetterBox, box rescale, mask -> polygon.

These sit on the CPU in the reference too (cv2 / numpy inside ultralytics' predictor; SURVEY.md A.5-A.7 [U]) and are
"next" rows of the scope table for a GPU version. cv2 is not available offline, so the 8-bit
INTER_LINEAR resize and the external-contour trace are restated here from the public OpenCV algorithms.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import torch


# ---- sources (A.5 step 1) --------------------------------------------------------------------------------------------
def _one_source(src) -> Tuple[np.ndarray, str]:
    if isinstance(src, np.ndarray):
        if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8:
            raise TypeError(f"ndarray source must be HxWx3 uint8 (BGR), got {src.shape} {src.dtype}")
        return src, ""                                    # ndarray => taken as BGR, never auto-corrected (SURVEY C-6)
    if isinstance(src, (str, os.PathLike)):
        from PIL import Image
        p = os.fspath(src)
        if not os.path.isfile(p):
            raise FileNotFoundError(p)
        with Image.open(p) as im:
            rgb = np.asarray(im.convert("RGB"))
        return np.ascontiguousarray(rgb[:, :, ::-1]), p
    if hasattr(src, "convert") and hasattr(src, "size"):   # PIL.Image -> RGB -> BGR (yolo_seg/app.py:49)
        rgb = np.asarray(src.convert("RGB"))
        return np.ascontiguousarray(rgb[:, :, ::-1]), ""
    if isinstance(src, torch.Tensor):
        raise TypeError("tensor sources are not part of the reference's call sites; pass ndarray / PIL / path")
    raise TypeError(f"unsupported source type {type(src)}")


def load_sources(source) -> Tuple[List[np.ndarray], List[str]]:
    items = list(source) if isinstance(source, (list, tuple)) else [source]
    if not items:
        raise ValueError("empty source list")
    pairs = [_one_source(s) for s in items]
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ---- LetterBox (A.5 step 2) ------------------------------------------------------------------------------------------
def letterbox_geometry(h0: int, w0: int, new_shape: int = 640, stride: int = 32, auto: bool = True) -> dict:
    r = min(new_shape / h0, new_shape / w0)
    nw, nh = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = new_shape - nw, new_shape - nh
    if auto:
        dw, dh = dw % stride, dh % stride
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return dict(r=r, new_w=nw, new_h=nh, top=top, bottom=bottom, left=left, right=right,
                out_h=nh + top + bottom, out_w=nw + left + right)


def _axis_coeffs(n_dst: int, n_src: int):
    scale = n_src / n_dst
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_src - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = n_src - 1, 0
    a1 = np.rint(f * 2048).astype(np.int64)
    a0 = np.rint((np.float32(1.0) - f) * 2048).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), a0, a1


def resize_linear_u8(img: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    """8-bit bilinear resize in OpenCV's fixed-point form (11-bit coefficients; vertical pass
    ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2)>>2). Restated, not verified against cv2 (absent offline)."""
    h0, w0 = img.shape[:2]
    if (h0, w0) == (new_h, new_w):
        return img
    x0, x1, ax0, ax1 = _axis_coeffs(new_w, w0)
    y0, y1, ay0, ay1 = _axis_coeffs(new_h, h0)
    src = img.astype(np.int64)
    hrow = src[:, x0, :] * ax0[None, :, None] + src[:, x1, :] * ax1[None, :, None]
    out = (((ay0[:, None, None] * (hrow[y0] >> 4)) >> 16) + ((ay1[:, None, None] * (hrow[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def letterbox(img_bgr: np.ndarray, new_shape: int = 640, stride: int = 32, auto: bool = True):
    g = letterbox_geometry(img_bgr.shape[0], img_bgr.shape[1], new_shape, stride, auto)
    im = resize_linear_u8(img_bgr, g["new_w"], g["new_h"])
    out = np.full((g["out_h"], g["out_w"], 3), 114, dtype=np.uint8)
    out[g["top"]:g["top"] + g["new_h"], g["left"]:g["left"] + g["new_w"]] = im
    return out, g


# ---- boxes (A.6 step 3) ----------------------------------------------------------------------------------------------
def scale_boxes_t(img1_hw: Sequence[int], boxes: torch.Tensor, img0_hw: Sequence[int]) -> torch.Tensor:
    """undo letterbox pad/gain, clamp to the original image (ops.scale_boxes + clip_boxes)."""
    gain = min(img1_hw[0] / img0_hw[0], img1_hw[1] / img0_hw[1])
    padx = round((img1_hw[1] - img0_hw[1] * gain) / 2 - 0.1)
    pady = round((img1_hw[0] - img0_hw[0] * gain) / 2 - 0.1)
    b = boxes.clone()
    b[:, 0] -= padx
    b[:, 2] -= padx
    b[:, 1] -= pady
    b[:, 3] -= pady
    b /= gain
    b[:, 0].clamp_(0, img0_hw[1])
    b[:, 2].clamp_(0, img0_hw[1])
    b[:, 1].clamp_(0, img0_hw[0])
    b[:, 3].clamp_(0, img0_hw[0])
    return b


def scale_coords(img1_hw: Sequence[int], coords: np.ndarray, img0_hw: Sequence[int]) -> np.ndarray:
    """polygon points from the letterboxed frame to the original image (ops.scale_coords)."""
    gain = min(img1_hw[0] / img0_hw[0], img1_hw[1] / img0_hw[1])
    padx = (img1_hw[1] - img0_hw[1] * gain) / 2
    pady = (img1_hw[0] - img0_hw[0] * gain) / 2
    c = coords.astype(np.float32).copy()
    c[:, 0] = np.clip((c[:, 0] - padx) / gain, 0, img0_hw[1])
    c[:, 1] = np.clip((c[:, 1] - pady) / gain, 0, img0_hw[0])
    return c


def scale_coords_f32_geometry(img1_hw: Sequence[int], img0_hw: Sequence[int]) -> Tuple[np.float32, np.float32, np.float32]:
    """(gain, padx, pady) of scale_coords as numpy meets them on a float32 polygon: computed in double (Python floats), rounded to float32.
    yp_mask_contours_scaled derives the same three constants on the host (csrc/contour.hip launch_contours_scaled)."""
    gain = min(img1_hw[0] / img0_hw[0], img1_hw[1] / img0_hw[1])
    padx = (img1_hw[1] - img0_hw[1] * gain) / 2
    pady = (img1_hw[0] - img0_hw[0] * gain) / 2
    return np.float32(gain), np.float32(padx), np.float32(pady)


def scale_coords_int(img1_hw: Sequence[int], points: np.ndarray, img0_hw: Sequence[int]) -> np.ndarray:
    """np.array(scale_coords(img1_hw, points, img0_hw), np.int32) - the integer points get_coord_min_rect_len measures on the polygon of a
    non-retina mask - stated as the device evaluates it per point (csrc/contour.hip scale_coord): float32 (v - pad) / gain, clipped to
    [0, W0] / [0, H0], truncated to int32."""
    gain, padx, pady = scale_coords_f32_geometry(img1_hw, img0_hw)
    p = np.asarray(points).reshape(-1, 2).astype(np.float32)
    x = np.minimum(np.maximum((p[:, 0] - padx) / gain, np.float32(0)), np.float32(img0_hw[1]))
    y = np.minimum(np.maximum((p[:, 1] - pady) / gain, np.float32(0)), np.float32(img0_hw[0]))
    return np.stack([x, y], 1).astype(np.int32)


# ---- Masks.xy (A.7): cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) + masks2segments, restated ----------------------------
# Definitions this module and the device kernel (csrc/contour.hip) both implement - cv2 is absent here, so they are stated, not pinned:
#   * foreground 8-connected, background 4-connected (the pairing of Suzuki & Abe's border following, which cv2.findContours implements);
#   * an OUTER border belongs to one 8-connected blob; it is EXTERNAL (what RETR_EXTERNAL keeps) iff the blob is not enclosed by another
#     blob, i.e. iff the background pixel west of the blob's raster-first pixel is 4-connected to the image frame. A blob inside a hole of
#     another blob is NOT external and is skipped, as cv2 skips it;
#   * a contour starts at its blob's raster-first pixel and runs DOWN first (counter-clockwise on screen: for a filled rectangle top-left,
#     bottom-left, bottom-right, top-right - the order cv2 returns); CHAIN_APPROX_SIMPLE keeps a pixel iff the move into it differs from
#     the move out of it (the start pixel included, judged on the closed chain);
#   * contours are listed bottom-up: descending raster order of their start pixels (cv2 returns the last contour it found first);
#   * masks2segments [U]: strategy "largest" = the contour with the most points (first in list order on a tie), "all" (the default of the
#     8.3.x line that YOLO11 weights need) = all contours concatenated in list order.
_DIRS = [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]   # (dy,dx), clockwise from east


def _trace_outer(mask: np.ndarray, sy: int, sx: int) -> List[Tuple[int, int]]:
    """Moore-neighbour boundary trace (8-connectivity) of the blob containing (sy,sx), which must be its first pixel
    in raster order; Jacob's stopping criterion. Clockwise on screen (east first); `_cv_order` turns the chain round."""
    H, W = mask.shape

    def on(y, x):
        return 0 <= y < H and 0 <= x < W and mask[y, x]

    pts = [(sx, sy)]
    cy, cx, d = sy, sx, 6            # we "arrived" from the north-west side: start searching at north
    start_d = None
    for _ in range(4 * H * W + 8):
        found = False
        for k in range(8):
            nd = (d + k) % 8
            ny, nx = cy + _DIRS[nd][0], cx + _DIRS[nd][1]
            if on(ny, nx):
                if start_d is None:
                    start_d = nd
                elif (cy, cx) == (sy, sx) and nd == start_d:
                    return pts[:-1] if len(pts) > 1 else pts
                cy, cx = ny, nx
                pts.append((cx, cy))
                d = (nd + 6) % 8 if (nd % 2 == 0) else (nd + 5) % 8   # restart at the background pixel examined last
                found = True
                break
        if not found:
            return pts                  # isolated pixel
    return pts


def _compress(pts: List[Tuple[int, int]]) -> np.ndarray:
    """CHAIN_APPROX_SIMPLE on a closed chain in the order given: keep only the end points of horizontal / vertical / diagonal runs."""
    n = len(pts)
    if n <= 2:
        return np.asarray(pts, dtype=np.int32).reshape(-1, 2)
    keep = []
    for i in range(n):
        px, py = pts[i - 1]
        cx, cy = pts[i]
        nx, ny = pts[(i + 1) % n]
        if (cx - px, cy - py) != (nx - cx, ny - cy):
            keep.append((cx, cy))
    if not keep:
        keep = [pts[0]]
    return np.asarray(keep, dtype=np.int32)


def _cv_order(pts: List[Tuple[int, int]]) -> np.ndarray:
    """The clockwise chain of `_trace_outer` walked the other way round from the same start pixel (the direction cv2 follows an outer
    border in), then CHAIN_APPROX_SIMPLE. The kept pixels are the same set - a pixel is a run end in either direction."""
    if len(pts) <= 2:
        return _compress(pts)
    return _compress([pts[0]] + pts[:0:-1])


def external_contours(mask: np.ndarray) -> List[np.ndarray]:
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0] as defined at the top of this section: list of int32 [m,2] (x,y)."""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    if n == 0:
        return []
    holes = ndimage.binary_fill_holes(mask) & ~mask          # (default structure: the background is invaded 4-connectedly from the frame)
    found = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        sub = lab[sl] == k
        ys, xs = np.nonzero(sub)
        sy = ys.min()
        sx = xs[ys == sy].min()
        gy, gx = int(sy) + sl[0].start, int(sx) + sl[1].start
        if gx > 0 and holes[gy, gx - 1]:
            continue                                         # the blob sits in a hole of another blob: not an external contour
        poly = _cv_order(_trace_outer(sub, int(sy), int(sx))) + np.asarray([sl[1].start, sl[0].start], dtype=np.int32)
        found.append((gy * mask.shape[1] + gx, poly))
    found.sort(key=lambda t: -t[0])
    return [p for _, p in found]


POLYGON_STRATEGIES = ("all", "largest", "all_merged")


_MERGE_BLOCK_CELLS = 1 << 20      # cells of the squared-distance table held at a time (8 MB of int64 per temporary)


def _closest_pair(a: np.ndarray, b: np.ndarray) -> Tuple[int, int]:
    """(index in a, index in b) of the first minimum, in row-major order, of the |a| x |b| table of squared integer distances - the
    argmin of the whole table, computed over blocks of rows: a later block replaces the best so far only when strictly smaller."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    rows = max(1, _MERGE_BLOCK_CELLS // max(1, b.shape[0]))
    best, at = None, (0, 0)
    for r0 in range(0, a.shape[0], rows):
        blk = a[r0:r0 + rows]
        d = (blk[:, None, 0] - b[None, :, 0]) ** 2 + (blk[:, None, 1] - b[None, :, 1]) ** 2
        j = int(d.argmin())
        v = int(d.flat[j])
        if best is None or v < best:
            best, at = v, (r0 + j // d.shape[1], j % d.shape[1])
    return at


def merge_contours(contours: List[np.ndarray]) -> np.ndarray:
    """"all" of the LATER 8.3.x releases [U]: `masks2segments` there joins several contours with `merge_multi_segment` (the COCO converter's
    routine) instead of laying them end to end - consecutive contours of the list are bridged at their closest pair of points (first
    minimum in row-major order of the squared-distance table), the first and the last contour are walked whole and closed, a middle one
    from its entry point to its exit point on the way out and the rest of it on the way back. Same point set as the concatenation (hence
    the same hull and minimum-area rectangle), another vertex order."""
    segs = [np.asarray(c).reshape(-1, 2) for c in contours]
    n = len(segs)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if n == 1:
        return segs[0]
    near = [[] for _ in range(n)]
    for i in range(1, n):
        ia, ib = _closest_pair(segs[i - 1], segs[i])
        near[i - 1].append(ia)
        near[i].append(ib)
    out, back = [], []
    for i in range(n):
        idx = near[i]
        seg = segs[i]
        if len(idx) == 2 and idx[0] > idx[1]:
            idx, seg = idx[::-1], seg[::-1]
        seg = np.roll(seg, -idx[0], axis=0)
        seg = np.concatenate([seg, seg[:1]])
        if i == 0 or i == n - 1:
            out.append(seg)
        else:
            out.append(seg[:idx[1] - idx[0] + 1])
            back.append(seg[abs(near[i][1] - near[i][0]):])
    return np.concatenate(out + back[::-1], axis=0)


def mask_polygon(mask: np.ndarray, strategy: str = "all") -> np.ndarray:
    """ultralytics `masks2segments(mask, strategy)` for one mask [U]: int32 [m,2] (x,y); [0,2] for an empty mask. "all" = every external
    contour laid end to end, "all_merged" = the same contours bridged at their closest points (later 8.3.x, merge_contours)."""
    if strategy not in POLYGON_STRATEGIES:
        raise ValueError(f"strategy must be one of {POLYGON_STRATEGIES}, got {strategy!r}")
    c = external_contours(mask)
    if not c:
        return np.zeros((0, 2), dtype=np.int32)
    if strategy == "all":
        return np.concatenate(c, axis=0)
    if strategy == "all_merged":
        return merge_contours(c).astype(np.int32)
    return c[int(np.argmax([len(x) for x in c]))]


def largest_external_contour(mask: np.ndarray) -> np.ndarray:
    """[m,2] (x,y) int32 polygon: the external contour with the most points (ultralytics masks2segments 'largest')."""
    return mask_polygon(mask, "largest")


# ---- shaft length from a polygon (reference yolo_seg/utils/mask_tools.py:12-22, which calls cv2.minAreaRect) ---------------------
def _convex_hull(pts: np.ndarray) -> np.ndarray:
    """Andrew's monotone chain on integer points; counter-clockwise, no collinear points, float64 out."""
    p = np.unique(pts.astype(np.int64), axis=0)            # sorted by x, then y
    if p.shape[0] <= 2:
        return p.astype(np.float64)

    def half(seq):
        h = []
        for q in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (q[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (q[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(q)
        return h

    lo, up = half(list(map(tuple, p))), half(list(map(tuple, p[::-1])))
    return np.asarray(lo[:-1] + up[:-1], dtype=np.float64)


def min_area_rect_size(points) -> Tuple[float, float]:
    """(long side, short side) of the minimum-area enclosing rectangle of integer points: one side of that rectangle is collinear
    with an edge of the convex hull (rotating calipers; the public algorithm behind cv2.minAreaRect, here in float64)."""
    hull = _convex_hull(np.asarray(points).reshape(-1, 2))
    n = hull.shape[0]
    if n == 0 or n == 1:
        return 0.0, 0.0
    if n == 2:
        return float(np.hypot(*(hull[1] - hull[0]))), 0.0
    best = None
    for i in range(n):
        e = hull[(i + 1) % n] - hull[i]
        u = e / np.hypot(e[0], e[1])
        v = np.array([-u[1], u[0]])
        a, b = hull @ u, hull @ v
        w, h = a.max() - a.min(), b.max() - b.min()
        if best is None or w * h < best[0]:
            best = (w * h, w, h)
    return float(max(best[1], best[2])), float(min(best[1], best[2]))


def get_coord_min_rect_len(coord_xy) -> Tuple[float, float]:
    """Drop-in for the reference's `get_coord_min_rect_len(results[0].masks.xy[i])` (yolo_seg/app.py:101-103): the polygon is
    truncated to int32 like there; -> (length of the longer side in pixels, length / shorter side, with a zero width counted as 1);
    (0, 0) for fewer than 3 points."""
    points = np.array(coord_xy, dtype=np.int32).reshape((-1, 2))
    if len(points) < 3:
        return 0, 0
    length, width = min_area_rect_size(points)
    if width == 0:
        width = 1
    return length, length / width


# ---- the app's first video loop over a whole clip (YOLO.predict_clip) -------------------------------------------------------
def clip_plan(n: int, batch_size: int) -> Tuple[int, List[Tuple[int, int]]]:
    """Chunks of YOLO.predict_clip for an n-frame clip: -> (B, [(start, count), ...]) with B = min(batch_size, n), contiguous chunks of
    B frames; the last one (count < B) is padded to B by repeating its last frame, so a clip meets one engine plan."""
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    n = int(n)
    if n <= 0:
        return 0, []
    B = min(int(batch_size), n)
    return B, [(s, min(B, n - s)) for s in range(0, n, B)]


def clip_track(detected: Sequence[bool], xyxy: Sequence, polygons: Sequence, rect_lens: Sequence, width: int, height: int):
    """The carry-forward of the reference's first video loop (yolo_seg/app.py:93-113) over per-frame results of the best detection:
    detected[i], its float xyxy box, polygon (masks.xy[best]) and rectangle length (get_coord_min_rect_len(polygon)[0]).
    -> (yolo_pred_xyxy, coord_xys, lens): a detection gives list(map(int, xyxy)), its polygon and its length; a frame without one repeats
    the last box ((0, 0, width, height) before the first detection), gets None and repeats the last length (0 before the first)."""
    boxes, coords, lens = [], [], []
    last_box, last_rect_len = None, 0
    for det, box, poly, rect_len in zip(detected, xyxy, polygons, rect_lens):
        if det:
            xyxy_box = list(map(int, box))
            last_box = xyxy_box
            coords.append(poly)
            last_rect_len = rect_len
            lens.append(rect_len)
        else:
            xyxy_box = (0, 0, width, height) if last_box is None else last_box
            coords.append(None)
            lens.append(last_rect_len)
        boxes.append(xyxy_box)
    return boxes, coords, lens


# ---- `auto_segment` over a clip (YOLO.predict_id_mask_clip) -----------------------------------------------------------------
def group_frames_by_workspace(counts: Sequence[int], workspace_bytes, budget: int, max_rows: int = 65535):
    """Calls of Engine.id_masks_frames for a chunk whose frame j has counts[j] masks: frames are taken greedily, in order, into one call
    while `workspace_bytes(n_total, k)` (the engine's query for k frames with n_total masks in all) stays within `budget` bytes and the
    call has at most `max_rows` masks. -> [(batched, [frame, ...]), ...] covering every frame once, in order; batched=False is ONE frame
    whose own workspace exceeds the budget (or that the query declines with 0): it goes through the one-frame call. Frames without
    masks are grouped like any other (their id image comes out of the same launches)."""
    groups: List[Tuple[bool, List[int]]] = []
    cur: List[int] = []
    rows = 0

    def fits(n_total, k):
        need = int(workspace_bytes(n_total, k))
        return 0 < need <= budget and n_total <= max_rows

    for j, n in enumerate(int(c) for c in counts):
        if n < 0:
            raise ValueError(f"negative mask count {n} for frame {j}")
        if cur and fits(rows + n, len(cur) + 1):
            cur.append(j)
            rows += n
            continue
        if cur:
            groups.append((True, cur))
            cur, rows = [], 0
        if fits(n, 1):
            cur, rows = [j], n
        else:
            groups.append((False, [j]))
    if cur:
        groups.append((True, cur))
    return groups


# ---- the app's output frame (loop #2 of the video path: yolo_seg/app.py:179-190, create_roi_mask at utils/mask_tools.py:100-129) ------
def roi_band(height: int, width: int, x1: int, y1: int, x2: int, y2: int) -> np.ndarray:
    """The pixel set of `cv2.rectangle(img, (x1, y1), (x2, y2), color, thickness=2)` as this project states it -> bool [height, width]:
    every in-frame pixel at Chebyshev distance <= 1 from the one-pixel outline through the two corners, i.e. the rectangle
    [x1-1, x2+1] x [y1-1, y2+1] without the pixels that are at least 2 away from all four sides. x2 == width and y2 == height (the app
    clamps to them, app.py:142-143) clip to the frame. Stated, not pinned: cv2 is not available to compare against, and its round line
    caps may leave out the four outer corner pixels (x1-1, y1-1), (x2+1, y1-1), (x1-1, y2+1), (x2+1, y2+1)."""
    if x2 < x1 or y2 < y1:
        raise ValueError(f"roi ({x1},{y1},{x2},{y2}) has x2 < x1 or y2 < y1")
    ys, xs = np.arange(int(height))[:, None], np.arange(int(width))[None, :]
    outer = (xs >= x1 - 1) & (xs <= x2 + 1) & (ys >= y1 - 1) & (ys <= y2 + 1)
    inner = (xs >= x1 + 2) & (xs <= x2 - 2) & (ys >= y1 + 2) & (ys <= y2 - 2)
    return outer & ~inner


def overlay_frame(frame: np.ndarray, crop_mask, window, roi, label=None, label_xy=None, col: Sequence[int] = (0, 0, 255)) -> np.ndarray:
    """One output frame of the app's loop #2, built the way the reference builds it: a zero image with the crop mask pasted at its window
    (with fix U-1 of INTEGRATION.md: `crop[:y_rd-y_lt, :x_rd-x_lt, None]`, the byte as it is on all three channels), a zero `roi_mask`
    with the rectangle (roi_band) and the label drawn into it in `col` (BGR), and two saturating adds (`cv2.addWeighted(a, 1, b, 1, 0)`).

    frame uint8 [H,W,3]; crop_mask uint8 [ch,cw] or None; window (x_lt, y_lt, x_rd, y_rd); roi (x1, y1, x2, y2); label a uint8 coverage
    bitmap [lh,lw] (0 = background, 255 = full colour) or None, its top-left at label_xy = (lx, ly), clipped to the frame. Where label
    and rectangle meet the larger value stays: a pixel of the label is max(what is there, (cov * col + 127) // 255) per channel."""
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise TypeError("overlay_frame expects a BGR uint8 HWC frame")
    H, W = frame.shape[:2]
    colour = np.asarray(col, dtype=np.uint8).reshape(3)
    mask = np.zeros(frame.shape, dtype=np.uint8)
    x_lt, y_lt, x_rd, y_rd = (int(v) for v in window)
    if crop_mask is not None and x_rd > x_lt and y_rd > y_lt:
        mask[y_lt:y_rd, x_lt:x_rd] = np.asarray(crop_mask, dtype=np.uint8)[:y_rd - y_lt, :x_rd - x_lt, None]
    roi_mask = np.zeros(frame.shape, dtype=np.uint8)
    roi_mask[roi_band(H, W, *(int(v) for v in roi))] = colour
    if label is not None and label.size:
        lx, ly = (int(v) for v in label_xy)
        lh, lw = label.shape
        xa, ya, xb, yb = max(lx, 0), max(ly, 0), min(lx + lw, W), min(ly + lh, H)
        if xa < xb and ya < yb:
            cov = label[ya - ly:yb - ly, xa - lx:xb - lx].astype(np.uint16)[:, :, None]
            drawn = ((cov * colour.astype(np.uint16) + 127) // 255).astype(np.uint8)
            roi_mask[ya:yb, xa:xb] = np.maximum(roi_mask[ya:yb, xa:xb], drawn)
    combined = np.minimum(frame.astype(np.uint16) + mask, 255).astype(np.uint8)
    return np.minimum(combined.astype(np.uint16) + roi_mask, 255).astype(np.uint8)
