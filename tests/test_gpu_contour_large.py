"""yp_mask_contours_large (csrc/contour_large.hip: bit image, border starts and segment records in a device workspace, RETR_EXTERNAL by a
walk from the nearest pixel to the west) - the device path for the masks yp_mask_contours declines: 4K frames, bounding boxes beyond its
LDS image, more than 64 outer borders. Same checkers as tests/test_gpu_contour.py, imported from it: tests/suzuki_abe.py point for point,
the brute-force rectangle, hostops.mask_polygon as the second statement. No mask of any list here may be declined by the large path."""
import ctypes as C

import numpy as np
import pytest
import torch

from suzuki_abe import find_contours_external_simple
from test_gpu_contour import ALL, _assert_rect, _blobs, _oracle_polygon, _rot_rect
from test_gpu_yolo_clip_input import _scaled_masks, assert_rect
from yolo_puncture_amd import hostops
from yolo_puncture_amd.engine import (CONTOUR_STRATEGIES, YP_CONTOURS_ONLY_DECLINED, YolopError, load_library, mask_contours_device,
                                      mask_contours_large_device)

pytestmark = pytest.mark.gpu


def _check_rect(rect_row, want, where):
    if want.shape[0] >= 3:
        _assert_rect(rect_row, want, where)
    elif want.shape[0] == 2:
        assert rect_row[0] == pytest.approx(float(np.hypot(*(want[1] - want[0]).astype(np.float64))), abs=1e-12) and rect_row[1] == pytest.approx(0.0, abs=1e-12)
    else:
        assert rect_row[0] == 0.0 and rect_row[1] == 0.0


def _random_masks():
    """the 320 masks of test_gpu_contour.test_random_masks_against_suzuki_abe"""
    rng = np.random.default_rng(11)
    H, W, N = 24, 40, 320
    ms = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        h, w = int(rng.integers(3, H + 1)), int(rng.integers(3, W + 1))
        m = rng.random((h, w)) < rng.choice([0.15, 0.35, 0.5, 0.65, 0.8])
        if i % 5 == 0 and h >= 9 and w >= 9:
            m[:] = False
            m[1:h - 1, 1:w - 1] = True
            m[2 + i % 2:h - 2, 2:w - 2 - i % 3] = rng.random((h - 4 - i % 2, w - 4 - i % 3)) < 0.3
        ms[i, :h, :w] = m
    return ms


# ---- 1. same answers where both paths work ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["all", "largest"])
@pytest.mark.parametrize("name,mask", ALL, ids=[n for n, _ in ALL])
def test_large_matches_lds_path(name, mask, strategy):
    d = torch.from_numpy(mask)[None].cuda()
    polys, rect, parts = mask_contours_large_device(d, max_pts=8192, strategy=strategy, want_parts=True)
    lp, lrect, lparts = mask_contours_device(d, max_pts=8192, strategy=strategy, want_parts=True)
    want, want_parts = _oracle_polygon(mask, strategy)
    assert polys[0] is not None, "the large path must not decline this mask"
    assert polys[0].dtype == np.int32 and polys[0].shape == want.shape and np.array_equal(polys[0], want)
    assert parts[0] == want_parts
    if lp[0] is not None:
        assert np.array_equal(polys[0], lp[0]) and parts[0] == lparts[0]
        assert rect[0, 0] == pytest.approx(lrect[0, 0], rel=1e-12, abs=1e-12) and rect[0, 1] == pytest.approx(lrect[0, 1], rel=1e-12, abs=1e-9)
    else:
        assert name in ("dots", "many_dots_nested") and strategy == "all"
    _check_rect(rect[0], want, name)
    assert np.array_equal(polys[0], hostops.mask_polygon(mask.astype(bool), strategy))


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_large_random_masks_batched_and_alone(strategy):
    ms = _random_masks()
    d = torch.from_numpy(ms).cuda()
    polys, rect, parts = mask_contours_large_device(d, strategy=strategy, want_parts=True)
    lp, lrect, lparts = mask_contours_device(d, strategy=strategy, want_parts=True)
    for i in range(len(ms)):
        want, want_parts = _oracle_polygon(ms[i], strategy)
        assert polys[i] is not None, i
        assert np.array_equal(polys[i], want) and parts[i] == want_parts, (i, strategy)
        if lp[i] is not None:
            assert np.array_equal(polys[i], lp[i]) and parts[i] == lparts[i], i
            assert rect[i, 0] == pytest.approx(lrect[i, 0], rel=1e-12, abs=1e-12) and rect[i, 1] == pytest.approx(lrect[i, 1], rel=1e-12, abs=1e-9), i
        _check_rect(rect[i], want, (i, strategy))
    # one batched call = per-mask calls, byte for byte
    for i in list(range(0, len(ms), 7)) + [len(ms) - 1]:
        p1, r1, q1 = mask_contours_large_device(d[i:i + 1], max_pts=16384, strategy=strategy, want_parts=True)
        assert p1[0].tobytes() == polys[i].tobytes() and r1[0].tobytes() == rect[i].tobytes() and q1[0] == parts[i], i


def test_large_random_masks_with_many_borders():
    """Sparse noise, 48x80: most of these have more than 64 outer borders, some of them nested in the rings drawn over the noise - "all"
    declines them on the LDS path, the large path lists every contour."""
    rng = np.random.default_rng(23)
    N, H, W = 48, 48, 80
    ms = (rng.random((N, H, W)) < rng.choice([0.08, 0.15, 0.25], size=(N, 1, 1))).astype(np.uint8)
    for i in range(0, N, 3):
        ms[i, 8:40, 10:70] = 1
        ms[i, 10:38, 12:68] = rng.random((28, 56)) < 0.12
    d = torch.from_numpy(ms).cuda()
    polys, rect, parts = mask_contours_large_device(d, strategy="all", want_parts=True)
    lp, _ = mask_contours_device(d, strategy="all")
    many = 0
    for i in range(N):
        want, want_parts = _oracle_polygon(ms[i], "all")
        assert polys[i] is not None and np.array_equal(polys[i], want) and parts[i] == want_parts, i
        _check_rect(rect[i], want, i)
        if lp[i] is None:
            many += 1
            assert len(want_parts) > 64
        else:
            assert np.array_equal(polys[i], lp[i])
    assert many >= N // 4


# ---- 2. masks the LDS kernel cannot take --------------------------------------------------------------------------------------------------
def _mask_d():
    D = np.zeros((2160, 3840), np.uint8)
    D[100:2060, 100:3740] = 1; D[300:1860, 300:3540] = 0; D[700:1500, 900:2900] = 1; D[900:1300, 1200:2600] = 0; D[1000:1200, 1500:2300] = 1
    D[700, 910:2890:7] = 0
    return D


def _mask_e():
    E = np.zeros((2160, 3840), np.uint8)
    E[::40, ::40] = 1; E[500:1700, 800:3000] = 0; E[520:1680, 820:2980] = 1; E[600:1600, 900:2900] = 0; E[800:1400:40, 1200:2600:40] = 1
    return E


def _needle_4k():
    return _rot_rect(2160, 3840, 1900, 1100, 900, 25, 0.45)


def _needle_4k_cut():
    m = _needle_4k()
    m[:, 1500:1506] = 0; m[:, 2100:2103] = 0; m[:, 2600:2602] = 0
    return m


def _big():
    big = np.zeros((900, 2200), np.uint8)
    big[10:890, 5:2195] = 1
    return big


LARGE = [("needle_4k", _needle_4k), ("needle_4k_cut", _needle_4k_cut), ("blobs_4k_0", lambda: _blobs(2160, 3840, 0)),
         ("blobs_4k_1", lambda: _blobs(2160, 3840, 1)), ("blobs_4k_2", lambda: _blobs(2160, 3840, 2)), ("rings_4k_D", _mask_d),
         ("dots_ring_4k_E", _mask_e), ("big", _big), ("blobs_1080p_4", lambda: _blobs(1080, 1920, 4))]


@pytest.mark.parametrize("name,make", LARGE, ids=[n for n, _ in LARGE])
def test_masks_the_lds_kernel_declines(name, make):
    mask = make()
    d = torch.from_numpy(mask)[None].cuda()
    cs = find_contours_external_simple(mask.astype(bool))              # (about a second per 4K mask: once for both strategies)
    for strategy in ("all", "largest"):
        assert mask_contours_device(d, strategy=strategy)[0][0] is None, "the premise: the LDS kernel declines this mask"
        if strategy == "all":
            want, want_parts = np.concatenate(cs).astype(np.int32), [len(c) for c in cs]
        else:
            best = max(range(len(cs)), key=lambda i: (len(cs[i]), -i))
            want, want_parts = cs[best].astype(np.int32), [len(cs[best])]
        polys, rect, parts = mask_contours_large_device(d, strategy=strategy, want_parts=True)
        assert polys[0] is not None, (name, strategy)
        assert polys[0].shape == want.shape and np.array_equal(polys[0], want), (name, strategy)
        assert parts[0] == want_parts, (name, strategy)
        _check_rect(rect[0], want, (name, strategy))
    assert np.array_equal(polys[0], hostops.mask_polygon(mask.astype(bool), "largest"))


# ---- 3. YP_CONTOURS_ONLY_DECLINED ------------------------------------------------------------------------------------------------------------
def test_only_declined_fills_in_shared_buffers():
    H, W = 900, 2200
    ms = np.zeros((4, H, W), np.uint8)
    ms[0, :120, :160] = _blobs(120, 160, 0)
    ms[1] = _big()
    ms[2, 300:420, 1000:1160] = _blobs(120, 160, 3)
    d = torch.from_numpy(ms).cuda()                                     # mask 3 is empty
    n, max_pts, parts_cap = 4, 4096, 65
    lib = load_library()
    count = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    parts = torch.full((n, parts_cap), 77, dtype=torch.int32, device="cuda")
    rect = torch.full((n, 2), 77.0, dtype=torch.float64, device="cuda")
    pts = torch.zeros((n, max_pts, 2), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.yp_mask_contours(vp(d), n, H, W, CONTOUR_STRATEGIES["all"], max_pts, vp(pts), vp(count), vp(parts), parts_cap, vp(rect), st) == 0
    torch.cuda.synchronize()
    c1, p1, r1, x1 = count.cpu().numpy().copy(), parts.cpu().numpy().copy(), rect.cpu().numpy().copy(), pts.cpu().numpy().copy()
    assert c1[0] > 0 and c1[1] == -1 and c1[2] > 0 and c1[3] == 0
    nbytes = int(lib.yp_mask_contours_large_workspace(n, H, W))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    assert lib.yp_mask_contours_large(vp(d), n, H, W, CONTOUR_STRATEGIES["all"], max_pts, vp(pts), vp(count), vp(parts), parts_cap, vp(rect), 0, 0,
                                      YP_CONTOURS_ONLY_DECLINED, vp(ws), nbytes, st) == 0, lib.yp_last_error()
    torch.cuda.synchronize()
    c2, p2, r2, x2 = count.cpu().numpy(), parts.cpu().numpy(), rect.cpu().numpy(), pts.cpu().numpy()
    for i in (0, 2, 3):                                                  # untouched: every byte of every row
        assert c2[i] == c1[i] and p2[i].tobytes() == p1[i].tobytes() and r2[i].tobytes() == r1[i].tobytes() and x2[i].tobytes() == x1[i].tobytes(), i
    assert c2[1] == 4 and x2[1, :4].tolist() == [[5, 10], [5, 889], [2194, 889], [2194, 10]]
    assert p2[1, 0] == 1 and p2[1, 1] == 4
    assert r2[1].tolist() == pytest.approx([2189.0, 879.0], rel=1e-12)


# ---- 4. scaled rectangle on wide frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h0,w0", [(1152, 2048), (2160, 3840)])
def test_scaled_rectangle_on_wide_frames(h0, w0):
    m, H, W = _scaled_masks(h0, w0)
    polys, _ = mask_contours_device(m, max_pts=16384, strategy="all")
    spolys, srect = mask_contours_large_device(m, max_pts=16384, strategy="all", orig_hw=(h0, w0))
    for i in range(m.shape[0]):
        assert spolys[i] is not None and np.array_equal(spolys[i], polys[i]), i
        assert srect[i].tolist() != [-1.0, -1.0] and srect[i, 0] >= 0, i
        pts = np.array(hostops.scale_coords((H, W), polys[i], (h0, w0)), dtype=np.int32)
        if len(pts) >= 3:
            assert_rect(float(srect[i, 0]), float(srect[i, 1]), pts, (i, h0, w0))
    want = hostops.scale_coords_int((H, W), np.array([[0, 0], [W - 1, H - 1]]), (h0, w0))
    assert srect[4].tolist() == pytest.approx(sorted([float(want[1, 0] - want[0, 0]), float(want[1, 1] - want[0, 1])], reverse=True), rel=1e-12)
    # narrower frames: the same rectangles as the LDS kernel's scaled form
    m, H, W = _scaled_masks(720, 1280)
    _, lrect = mask_contours_device(m, max_pts=16384, strategy="all", orig_hw=(720, 1280))
    _, srect = mask_contours_large_device(m, max_pts=16384, strategy="all", orig_hw=(720, 1280))
    assert srect == pytest.approx(lrect, rel=1e-12)


# ---- 5. limits decline, they do not lie ----------------------------------------------------------------------------------------------------------
def test_limits_decline():
    checker = torch.from_numpy((np.indices((64, 80)).sum(0) % 2).astype(np.uint8))[None].cuda()
    polys, _ = mask_contours_large_device(checker, max_pts=16)
    assert polys[0] is None
    polys, _ = mask_contours_large_device(checker, max_pts=8192)
    assert polys[0] is not None
    # include/yolop.h: H or W above YP_CONTOURS_LARGE_MAX_DIM is an argument error, nothing is launched
    for shape in ((1, 4097, 8), (1, 8, 4097)):
        with pytest.raises(YolopError, match="4096"):
            mask_contours_large_device(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    edge = torch.zeros((1, 4096, 4096), dtype=torch.uint8, device="cuda")
    edge[0, 4000:4096, 4000:4096] = 1
    polys, rect = mask_contours_large_device(edge)
    assert polys[0].tolist() == [[4000, 4000], [4000, 4095], [4095, 4095], [4095, 4000]] and rect[0].tolist() == pytest.approx([95.0, 95.0])
