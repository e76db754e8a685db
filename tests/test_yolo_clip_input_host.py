"""YOLO.predict_clip(retina_masks=False) without a GPU: the float32 scale geometry yp_mask_contours_scaled evaluates per point
(hostops.scale_coords_int) against hostops.scale_coords + the int32 truncation of get_coord_min_rect_len, its clip and truncation rules,
_finish_contour keeping a rectangle measured in original-image pixels, and argument errors raised before any engine is built."""
import numpy as np
import pytest

from yolo_puncture_amd import hostops
from yolo_puncture_amd.predictor import YOLO, ClipResults, _finish_contour

# (frame h0, w0): 720p, 1080p, portrait, odd sizes (non-integer pads and gains), a frame too wide for the device's hull tables
GEOMETRIES = [(720, 1280), (1080, 1920), (1280, 720), (333, 517), (517, 333), (1000, 1500), (480, 640), (1152, 2048), (1, 7)]


def _letterboxed(h0, w0):
    g = hostops.letterbox_geometry(h0, w0, 640)
    return g["out_h"], g["out_w"]


@pytest.mark.parametrize("h0,w0", GEOMETRIES)
def test_scale_coords_int_matches_numpy(h0, w0):
    H, W = _letterboxed(h0, w0)
    rng = np.random.RandomState(h0 * 7 + w0)
    pts = np.stack([rng.randint(0, W, 20000), rng.randint(0, H, 20000)], 1).astype(np.int32)
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W, H]], np.int32)
    pts = np.concatenate([pts, corners])
    want = np.array(hostops.scale_coords((H, W), pts, (h0, w0)), dtype=np.int32)
    assert np.array_equal(hostops.scale_coords_int((H, W), pts, (h0, w0)), want)


def test_scale_geometry_is_float32_of_the_double_values():
    gain, padx, pady = hostops.scale_coords_f32_geometry((416, 640), (333, 517))
    g = min(416 / 333, 640 / 517)
    assert gain.dtype == padx.dtype == pady.dtype == np.float32
    assert gain == np.float32(g) and padx == np.float32((640 - 517 * g) / 2) and pady == np.float32((416 - 333 * g) / 2)
    assert float(pady) != 0.0 and float(pady) != round(float(pady))          # a non-integer pad: the float32 rounding of it matters


def test_scale_coords_is_evaluated_in_float32():
    """scale_coords computes in float32 (the Python-float pad and gain are cast to float32): on a 1000x1500 frame (letterboxed 448x640, gain
    0.4267, pad 10.67) a float64 evaluation truncates some coordinates differently, and the device statement follows float32."""
    h0, w0 = 1000, 1500
    H, W = _letterboxed(h0, w0)
    xs, ys = np.meshgrid(np.arange(W + 1), np.arange(H + 1))
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    f = hostops.scale_coords((H, W), pts, (h0, w0))
    assert f.dtype == np.float32
    want = np.array(f, dtype=np.int32)
    assert np.array_equal(hostops.scale_coords_int((H, W), pts, (h0, w0)), want)
    g = min(H / h0, W / w0)
    x64 = np.clip((pts[:, 0] - (W - w0 * g) / 2) / g, 0, w0).astype(np.int32)
    y64 = np.clip((pts[:, 1] - (H - h0 * g) / 2) / g, 0, h0).astype(np.int32)
    assert int((x64 != want[:, 0]).sum()) > 0 and int((y64 != want[:, 1]).sum()) > 0


def test_scale_coords_int_clip_and_truncation():
    # 720p: letterboxed 384x640, gain 0.5, pads (0, 12): rows 0..11 are padding above the frame, 372.. below it
    H, W = _letterboxed(720, 1280)
    assert (H, W) == (384, 640)
    pts = np.array([[0, 0], [0, 11], [0, 12], [0, 13], [639, 371], [639, 372], [639, 383], [640, 384]], np.int32)
    got = hostops.scale_coords_int((H, W), pts, (720, 1280))
    assert got.dtype == np.int32
    assert got.tolist() == [[0, 0], [0, 0], [0, 0], [0, 2], [1278, 718], [1278, 720], [1278, 720], [1280, 720]]
    # fractional results truncate toward zero (after the clip at 0 nothing is negative): 333x517, gain 1.2379, pady 1.89
    H, W = _letterboxed(333, 517)
    pts = np.array([[1, 1], [1, 2], [2, 3], [100, 200], [639, 414]], np.int32)
    got = hostops.scale_coords_int((H, W), pts, (333, 517))
    want = np.array(hostops.scale_coords((H, W), pts, (333, 517)), dtype=np.int32)
    assert np.array_equal(got, want)
    f = hostops.scale_coords((H, W), pts, (333, 517))
    assert np.all(got == np.floor(f)) and np.any(f != np.floor(f))


def test_finish_contour_keeps_a_rectangle_in_original_pixels():
    poly = np.array([[10, 20], [10, 40], [50, 40], [50, 20]], np.int32)
    rect = np.array([80.0, 40.0])
    host_mask = lambda: pytest.fail("the host trace must not run when the device has a polygon")   # noqa: E731
    want_poly = hostops.scale_coords((384, 640), poly, (720, 1280)).astype(np.float32)
    # existing callers: a rectangle measured in mask pixels is dropped when the mask is not at the original size
    p, r = _finish_contour(poly, rect, None, "all", host_mask, (384, 640), (720, 1280))
    assert np.array_equal(p, want_poly) and r is None
    # already in original pixels: kept, and the polygon is scaled all the same
    p, r = _finish_contour(poly, rect, None, "all", host_mask, (384, 640), (720, 1280), rect_in_orig=True)
    assert np.array_equal(p, want_poly) and r == (80.0, 40.0)
    # declined by the device ((-1, -1)): the host measures it
    p, r = _finish_contour(poly, np.array([-1.0, -1.0]), None, "all", host_mask, (384, 640), (720, 1280), rect_in_orig=True)
    assert r is None
    # no device polygon: the host traces the mask, and no device rectangle survives
    m = np.zeros((384, 640), bool)
    m[20:41, 10:51] = True
    p, r = _finish_contour(None, rect, None, "all", lambda: m, (384, 640), (720, 1280), rect_in_orig=True)
    assert r is None and np.array_equal(p, want_poly)
    # "all_merged": the bridge keeps the point set, so the rectangle stays valid
    two = np.concatenate([poly, poly + 100]).astype(np.int32)
    p, r = _finish_contour(two, rect, [4, 4], "all_merged", host_mask, (384, 640), (720, 1280), rect_in_orig=True)
    assert r == (80.0, 40.0)
    assert set(map(tuple, p.tolist())) == set(map(tuple, hostops.scale_coords((384, 640), two, (720, 1280)).tolist()))


@pytest.fixture
def seg_model(monkeypatch):
    m = YOLO("synthetic:v8n-seg", dtype="fp32")

    def no_engine(*a, **k):
        raise AssertionError("an engine was built before the arguments were checked")

    monkeypatch.setattr(m, "_engine", no_engine)
    return m


def test_predict_clip_input_argument_errors(seg_model):
    f = np.zeros((72, 128, 3), np.uint8)
    r = seg_model.predict_clip([], retina_masks=False)
    assert isinstance(r, ClipResults) and tuple(r) == ([], [], [])
    with pytest.raises(ValueError, match="batch_size"):
        seg_model.predict_clip([f], batch_size=0, retina_masks=False)
    with pytest.raises(ValueError, match="differ in shape"):
        seg_model.predict_clip([f, np.zeros((72, 130, 3), np.uint8)], retina_masks=False)
    with pytest.raises(TypeError):
        seg_model.predict_clip([f.astype(np.float32)], retina_masks=False)
