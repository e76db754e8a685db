"""The app's output frame on the host (hostops.overlay_frame, hostops.roi_band), label placement (overlay.render_labels) and the argument
checks of yp_overlay_frames, none of which needs a device."""
import ctypes as C

import numpy as np
import pytest

from overlay_cases import COLOURS, LH, LW, SHAPES, VARIANTS, band_by_distance, make_case, overlay_by_loops, reference
from yolo_puncture_amd import hostops
from yolo_puncture_amd.engine import load_library
from yolo_puncture_amd.overlay import OVERLAY_PARAMS, frame_runs, label_origin, render_labels


def test_overlay_frame_equals_the_per_pixel_statement():
    rng = np.random.default_rng(5)
    H, W = 11, 13
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frame[2:5, 3:9] = 255
    frame[7:9, 0:4] = 0
    crop = rng.integers(0, 256, (8, 9), dtype=np.uint8)
    label = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    for window, roi, xy, col in (((2, 3, 9, 10), (1, 2, 9, 8), (0, 0), (0, 0, 255)),
                                 ((5, 0, 13, 8), (0, 0, 13, 11), (10, 9), (10, 200, 77)),       # the label hangs off the right and bottom
                                 ((0, 4, 1, 11), (6, 1, 6, 9), (-3, -2), (255, 1, 128)),         # off the left and top
                                 ((4, 4, 4, 4), (3, 3, 12, 10), (2, 2), (0, 0, 255))):           # no window; label over the band
        want = overlay_by_loops(frame, crop, window, roi, label, xy, col)
        got = hostops.overlay_frame(frame, crop, window, roi, label, xy, col)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (window, roi, xy)
    assert np.array_equal(hostops.overlay_frame(frame, None, (0, 0, 0, 0), (1, 2, 9, 8)),
                          overlay_by_loops(frame, None, (0, 0, 0, 0), (1, 2, 9, 8), None, None, (0, 0, 255)))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", range(VARIANTS))
def test_gpu_cases_on_the_host(shape, variant):
    """the inputs of test_gpu_overlay.py: overlay_frame equals the per-pixel statement on every one of them"""
    case = make_case(*shape, variant)
    want = reference(case, lambda f, m, w, r, l, xy, c: overlay_by_loops(f, m, tuple(w), tuple(int(v) for v in r), l, xy, c))
    assert np.array_equal(reference(case, hostops.overlay_frame), want)


@pytest.mark.parametrize("roi", [(3, 2, 13, 11),        # x2 == W, y2 == H
                                 (0, 0, 6, 5),          # x1 == 0, y1 == 0
                                 (5, 1, 5, 9),          # one pixel wide
                                 (0, 0, 13, 11),        # the fallback box (0, 0, W, H)
                                 (4, 3, 5, 4), (2, 2, 6, 6)])
def test_roi_band(roi):
    H, W = 11, 13
    band = hostops.roi_band(H, W, *roi)
    assert band.dtype == bool and band.shape == (H, W)
    assert np.array_equal(band, band_by_distance(H, W, *roi))
    x1, y1, x2, y2 = roi
    for y in range(max(y1, 0), min(y2, H - 1) + 1):     # the outline itself, where it is in the frame
        for x in (x1, x2):
            if 0 <= x < W:
                assert band[y, x]


def test_roi_band_of_the_fallback_box_is_the_frame_border():
    band = hostops.roi_band(11, 13, 0, 0, 13, 11)
    want = np.zeros((11, 13), bool)
    want[:2], want[:, :2] = True, True                  # the outline on row / column 0 and its inner neighbour
    want[10], want[:, 12] = True, True                  # the outline on row 11 / column 13 is outside: only its neighbour inside
    assert np.array_equal(band, want)
    with pytest.raises(ValueError):
        hostops.roi_band(11, 13, 5, 0, 4, 3)


@pytest.mark.parametrize("value,mask,want", [(254, 0, 254), (254, 1, 255), (254, 2, 255), (255, 0, 255), (255, 255, 255), (1, 255, 255),
                                             (0, 254, 254), (128, 127, 255), (128, 128, 255)])
def test_saturation(value, mask, want):
    """frame + M at 254, 255 and 256 and beyond, away from the rectangle; then with the rectangle's 255 on top"""
    frame = np.full((9, 9, 3), value, np.uint8)
    crop = np.full((3, 3), mask, np.uint8)
    out = hostops.overlay_frame(frame, crop, (4, 4, 7, 7), (0, 0, 1, 1))
    assert (out[4:7, 4:7] == want).all() and (out[3, 3:] == value).all()
    out = hostops.overlay_frame(frame, crop, (0, 0, 3, 3), (0, 0, 1, 1))
    assert (out[0, 0] == (want, want, 255)).all()       # red on top of frame + M


def test_label_and_band_keep_the_larger_value():
    frame = np.zeros((12, 12, 3), np.uint8)
    label = np.array([[0, 64, 255]], np.uint8)
    col = (10, 200, 77)
    out = hostops.overlay_frame(frame, None, (0, 0, 0, 0), (3, 3, 8, 8), label, (2, 3), col)      # label pixels on the band's row 3
    assert tuple(out[3, 2]) == col and tuple(out[3, 3]) == col and tuple(out[3, 4]) == col          # max(col, anything <= col) = col
    out = hostops.overlay_frame(frame, None, (0, 0, 0, 0), (3, 3, 8, 8), label, (5, 5), col)      # label inside the rectangle
    assert tuple(out[5, 5]) == (0, 0, 0)
    assert tuple(out[5, 6]) == tuple((64 * c + 127) // 255 for c in col)
    assert tuple(out[5, 7]) == col


def test_render_labels_placement():
    rois = [(40, 60, 200, 220), (40, 21, 200, 220), (40, 20, 200, 220), (7, 0, 50, 50), (5, 5, 9, 9)]
    texts = ["12 0 0.98 30.00 17.50", "g", "0 1 0.50 2.00mm/s", "Ag", ""]
    bitmaps, xy = render_labels(texts, rois)
    assert bitmaps.dtype == np.uint8 and bitmaps.ndim == 3 and bitmaps.shape[0] == 5 and xy.shape == (5, 4)
    from yolo_puncture_amd.overlay import _default_font
    font = _default_font()
    ascent = font.getmetrics()[0]
    for n, (text, roi) in enumerate(zip(texts, rois)):
        lx, ly, lw, lh = (int(v) for v in xy[n])
        if not text:
            assert (lw, lh) == (0, 0) and not bitmaps[n].any()
            continue
        l, t, r, b = font.getbbox(text)
        text_h = ascent - t                                 # height above the baseline
        assert (lw, lh) == (r - l, b - t) and lw <= bitmaps.shape[2] and lh <= bitmaps.shape[1]
        baseline = ly + text_h
        assert lx - l == roi[0]                             # text_x = x1
        assert baseline == (roi[1] - 10 if roi[1] - 10 > 10 else roi[1] + 10 + text_h)
        assert bitmaps[n, :lh, :lw].max() == 255 and not bitmaps[n, lh:].any() and not bitmaps[n, :, lw:].any()
        assert bitmaps[n, 0, :lw].any() and bitmaps[n, lh - 1, :lw].any()       # the ink box is tight
    # both sides of the `> 10` rule: y1 = 21 is above the box (baseline 11), y1 = 20 goes below it
    assert label_origin(40, 21, 9) == (40, 11) and label_origin(40, 20, 9) == (40, 39)
    assert xy[1][1] + (ascent - font.getbbox("g")[1]) == 11
    assert xy[2][1] + (ascent - font.getbbox(texts[2])[1]) == 20 + 10 + (ascent - font.getbbox(texts[2])[1])
    with pytest.raises(ValueError):
        render_labels(["a"], rois)


def test_frame_runs_are_in_frame_order():
    shapes = [(380, 380)] * 5 + [(200, 380)] * 3 + [(380, 380)] * 9
    runs = frame_runs(shapes, 4)
    assert [(s, e) for _, s, e in runs] == [(0, 4), (4, 5), (5, 7), (7, 8), (8, 12), (12, 16), (16, 17)]
    assert all(shape == shapes[s] for shape, s, _ in runs)
    assert frame_runs([], 4) == []


def _call(lib, par, *, src=0x1000, dst=0x100000, n=None, H=16, W=20, masks=0x2000, B=2, ch=8, cw=10, labels=0x3000, lh=LH, lw=LW, params=True):
    par = np.ascontiguousarray(np.asarray(par, np.int32).reshape(-1, OVERLAY_PARAMS))
    n = par.shape[0] if n is None else n
    return lib.yp_overlay_frames(C.c_void_p(src), C.c_void_p(dst), n, H, W, C.c_void_p(masks), B, ch, cw,
                                 par.ctypes.data_as(C.c_void_p) if params else None, C.c_void_p(labels), lh, lw, None, None)


def test_abi_refuses_bad_arguments():
    """every check runs before the device is touched: the pointers here are never dereferenced"""
    lib = load_library()
    ok = [2, 3, 12, 11, 1, 1, 19, 15, 0, 0, LW, LH, 1]

    def bad(i, v):
        row = list(ok)
        row[i] = v
        return row
    for what, rc in (("null src", _call(lib, ok, src=None)), ("null dst", _call(lib, ok, dst=None)), ("null params", _call(lib, ok, params=False)),
                     ("null masks", _call(lib, ok, masks=None)), ("null labels", _call(lib, ok, labels=None)),
                     ("window wider than cw", _call(lib, bad(2, 13))), ("window taller than ch", _call(lib, bad(3, 12))),
                     ("window past W", _call(lib, bad(2, 21), cw=30)), ("window past H", _call(lib, bad(3, 17), ch=30)),
                     ("negative window", _call(lib, bad(0, -1))), ("x_rd < x_lt", _call(lib, bad(2, 1))),
                     ("x2 < x1", _call(lib, bad(6, 0))), ("y2 < y1", _call(lib, bad(7, 0))),
                     ("crop index == B", _call(lib, bad(12, 2))), ("negative crop index", _call(lib, bad(12, -1))),
                     ("label wider than LW", _call(lib, bad(10, LW + 1))), ("negative n", _call(lib, ok, n=-1)),
                     ("H == 0", _call(lib, ok, H=0)), ("overlapping src and dst", _call(lib, ok, dst=0x1010)),
                     ("second row bad", _call(lib, [ok, bad(12, 5)]))):
        assert rc == -1, what                               # YP_ERR_ARG
        assert b"yp_overlay_frames" in lib.yp_last_error(), what
    assert _call(lib, ok, n=0) == 0                         # nothing to do
    assert COLOURS[0] == (0, 0, 255)
