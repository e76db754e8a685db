"""Inputs and a second, per-pixel statement of the app's output frame (hostops.overlay_frame / yp_overlay_frames), shared by
test_overlay_host.py and test_gpu_overlay.py."""
import numpy as np

SHAPES = [(3, 37, 53),      # W*3 = 159 and H*W*3 = 5883 are no multiples of 16: frames 1 and 2 start misaligned
          (2, 16, 16),      # everything aligned
          (2, 9, 5)]        # a row (15 bytes) is shorter than one vector
VARIANTS = 4
COLOURS = [(0, 0, 255), (10, 200, 77)]
LH, LW = 7, 11


def band_by_distance(H, W, x1, y1, x2, y2):
    """Chebyshev distance <= 1 from the one-pixel outline through (x1,y1)-(x2,y2), pixel by pixel (the outline itself may lie outside
    the frame: x2 == W, y2 == H)."""
    outline = [(x, y) for y in range(y1, y2 + 1) for x in range(x1, x2 + 1) if x in (x1, x2) or y in (y1, y2)]
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            out[y, x] = any(max(abs(x - ox), abs(y - oy)) <= 1 for ox, oy in outline)
    return out


def overlay_by_loops(frame, crop, window, roi, label, label_xy, col):
    """out = min(255, frame + M + R[c]) per pixel and channel, as the issue states it."""
    H, W = frame.shape[:2]
    x_lt, y_lt, x_rd, y_rd = window
    band = band_by_distance(H, W, *roi)
    out = np.zeros_like(frame)
    for y in range(H):
        for x in range(W):
            m = int(crop[y - y_lt, x - x_lt]) if (crop is not None and x_lt <= x < x_rd and y_lt <= y < y_rd) else 0
            cov = 0
            if label is not None:
                u, v = x - label_xy[0], y - label_xy[1]
                if 0 <= u < label.shape[1] and 0 <= v < label.shape[0]:
                    cov = int(label[v, u])
            for c in range(3):
                r = max(int(col[c]) if band[y, x] else 0, (cov * int(col[c]) + 127) // 255)
                out[y, x, c] = min(255, int(frame[y, x, c]) + m + r)
    return out


def windows_of(H, W):
    return [(0, 0, min(W, 7), min(H, 5)),                          # the four corners
            (W - min(W, 6), 0, W, min(H, 4)),
            (0, H - min(H, 6), min(W, 4), H),
            (W - min(W, 9), H - min(H, 7), W, H),
            (W // 2, 1, W // 2 + 1, H - 1),                        # one pixel wide
            (0, 0, W, H),                                          # the full frame
            (W // 3, H // 3, W // 3 + max(1, W // 2), H // 3 + max(1, H // 2))]   # inside, narrower than cw


def rois_of(H, W):
    return [(0, 0, W, H),                                          # the fallback box: touches every edge, x2 == W and y2 == H
            (W // 4, H // 4, W // 2, H // 2),
            (W // 2, 2, W // 2, H - 3),                            # one pixel wide
            (W - 3, H - 3, W, H),
            (0, 1, W - 1, H - 1),                                  # x1 == 0, the right side on the last column
            (1, 0, 2, 1)]


def labels_of(H, W, roi, window):
    """(lx, ly, lw, lh): hanging off each edge, past the frame, over the band and the window, absent."""
    return [(-4, -3, LW, LH), (W - 5, H - 3, LW, LH), (W + 2, 3, LW, LH), (3, H + 1, LW, LH), (roi[0] - 2, roi[1] - 2, LW, LH),
            (0, 0, 0, 0), (window[0] - 1, window[1] + 1, LW - 3, LH - 2), (-LW, 2, LW, LH), (W - 1, -LH + 1, LW, LH)]


def make_case(N, H, W, variant, seed=0):
    """One call's inputs as numpy: frames [N,H,W,3] (0 and 255 among the bytes), crop masks [B,ch,cw] = [N+1,H,W+2] with random bytes,
    per-frame windows, rois, label bitmaps and (lx, ly, lw, lh), and a crop index that is a permutation against the frame index."""
    rng = np.random.default_rng(1000 * seed + 17 * variant + H * W + N)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    frames[rng.random((N, H, W, 3)) < 0.15] = 255
    frames[rng.random((N, H, W, 3)) < 0.15] = 0
    masks = rng.integers(0, 256, (N + 1, H, W + 2), dtype=np.uint8)
    labels = rng.integers(0, 256, (N, LH, LW), dtype=np.uint8)
    labels[rng.random(labels.shape) < 0.3] = 0
    labels[rng.random(labels.shape) < 0.2] = 255
    crop_index = (np.arange(N)[::-1] + variant) % (N + 1)          # N + 1 crops, taken in reversed order from a moving start
    wins, rois, lxy = [], [], []
    for n in range(N):
        k = variant * N + n
        w = windows_of(H, W)[k % 7]
        r = rois_of(H, W)[k % 6]
        wins.append(w)
        rois.append(r)
        lxy.append(labels_of(H, W, r, w)[k % 9])
    return dict(frames=frames, masks=masks, labels=labels, windows=np.array(wins, np.int32), rois=np.array(rois, np.int32),
                label_xy=np.array(lxy, np.int32), crop_index=crop_index.astype(np.int32), col=COLOURS[variant % 2])


def reference(case, overlay_frame):
    """overlay_frame over the case's frames -> [N,H,W,3]"""
    out = []
    for n in range(case["frames"].shape[0]):
        lx, ly, lw, lh = (int(v) for v in case["label_xy"][n])
        label = case["labels"][n][:lh, :lw] if lw and lh else None
        out.append(overlay_frame(case["frames"][n], case["masks"][case["crop_index"][n]], case["windows"][n], case["rois"][n], label,
                                 (lx, ly), case["col"]))
    return np.stack(out)


def region_mask(case):
    """bool [N,H,W]: pixels of the mask window, the band or the label rectangle"""
    N, H, W = case["frames"].shape[:3]
    out = np.zeros((N, H, W), bool)
    for n in range(N):
        x_lt, y_lt, x_rd, y_rd = case["windows"][n]
        out[n, y_lt:y_rd, x_lt:x_rd] = True
        out[n] |= band_by_distance(H, W, *(int(v) for v in case["rois"][n]))
        lx, ly, lw, lh = (int(v) for v in case["label_xy"][n])
        out[n, max(ly, 0):max(ly + lh, 0), max(lx, 0):max(lx + lw, 0)] = True
    return out
