"""YOLO.predict_clip without a GPU: the carry-forward of the app's first video loop (hostops.clip_track) against a literal restatement of
yolo_seg/app.py:93-113, the chunk / pad plan (hostops.clip_plan), and argument errors raised before any engine is built."""
import types

import numpy as np
import pytest
import torch

from yolo_puncture_amd import hostops
from yolo_puncture_amd.classify import predict_and_find_start_inserted
from yolo_puncture_amd.predictor import YOLO, ClipResults


def app_loop(per_frame, width, height):
    """yolo_seg/app.py:93-113 as written, over per-frame (conf array, xyxy array, polygon list) of one `predict` result each."""
    yolo_pred_xyxy, coord_xys, lens = [], [], []
    last_box, last_rect_len = None, 0
    for confs, xyxys, segs in per_frame:
        if len(confs) > 0:
            best_conf_idx = np.argmax(confs)
            xyxy_box = xyxys[best_conf_idx].squeeze()
            xyxy_box = list(map(int, xyxy_box))
            last_box = xyxy_box
            seg_mask = segs[best_conf_idx]
            coord_xys.append(seg_mask)
            rect_len, _ = hostops.get_coord_min_rect_len(seg_mask)
            last_rect_len = rect_len
            lens.append(rect_len)
        else:
            if last_box is None:
                xyxy_box = 0, 0, width, height
            else:
                xyxy_box = last_box
            coord_xys.append(None)
            lens.append(last_rect_len)
        yolo_pred_xyxy.append(xyxy_box)
    return yolo_pred_xyxy, coord_xys, lens


def _square(x, y, s):
    return np.array([[x, y], [x, y + s], [x + s, y + s], [x + s, y]], dtype=np.float32)


def _track(per_frame, width, height):
    det, xyxy, polys, rl = [], [], [], []
    for confs, xyxys, segs in per_frame:
        if len(confs):
            b = int(np.argmax(confs))
            det.append(True)
            xyxy.append(xyxys[b])
            polys.append(segs[b])
            rl.append(hostops.get_coord_min_rect_len(segs[b])[0])
        else:
            det.append(False)
            xyxy.append(None)
            polys.append(None)
            rl.append(0)
    return hostops.clip_track(det, xyxy, polys, rl, width, height)


def _same(a, b):
    assert [list(x) for x in a[0]] == [list(x) for x in b[0]]
    assert [type(x) for x in a[0]] == [type(x) for x in b[0]]
    assert len(a[1]) == len(b[1])
    for p, q in zip(a[1], b[1]):
        assert (p is None and q is None) or np.array_equal(p, q)
    assert a[2] == b[2]


NONE = (np.zeros(0, np.float32), np.zeros((0, 4), np.float32), [])


def _det(boxes, confs, polys):
    return np.array(confs, np.float32), np.array(boxes, np.float32).reshape(-1, 4), polys


def test_clip_track_matches_app_loop():
    seqs = [
        # no detection in frame 0 (and 1), then detections with float boxes that truncate
        [NONE, NONE, _det([[10.9, 20.2, 300.7, 400.99]], [0.8], [_square(10, 20, 50)]), NONE,
         _det([[1.5, 2.5, 3.5, 4.5], [0.1, 0.2, 1279.9, 719.9]], [0.3, 0.9], [_square(1, 2, 3), _square(0, 0, 100)])],
        # detection first, gaps in the middle, a polygon with fewer than 3 points (length 0 is carried forward as well)
        [_det([[5, 5, 50, 50]], [0.5], [_square(5, 5, 40)]), NONE, NONE,
         _det([[7.99, 8.01, 9.5, 10.5]], [0.6], [np.array([[7, 8], [9, 10]], np.float32)]), NONE,
         _det([[0, 0, 1, 1]], [0.7], [np.zeros((0, 2), np.float32)]), NONE, _det([[100.2, 0.0, 200.8, 99.9]], [0.95], [_square(100, 0, 99)])],
        # nothing detected at all
        [NONE, NONE, NONE],
        # ties: np.argmax takes the first
        [_det([[1, 1, 2, 2], [3, 3, 4, 4]], [0.5, 0.5], [_square(1, 1, 1), _square(3, 3, 1)])],
    ]
    for seq in seqs:
        _same(_track(seq, 1280, 720), app_loop(seq, 1280, 720))
    assert hostops.clip_track([], [], [], [], 1280, 720) == ([], [], [])
    boxes, coords, lens = hostops.clip_track([False, True, False], [None, np.array([1.7, 2.2, 3.9, 4.1], np.float32), None],
                                             [None, _square(0, 0, 2), None], [0, 2.0, 0], 640, 360)
    assert boxes == [(0, 0, 640, 360), [1, 2, 3, 4], [1, 2, 3, 4]] and coords[0] is None and coords[2] is None and lens == [0, 2.0, 2.0]


@pytest.mark.parametrize("n,bs,expect", [
    (1, 32, (1, [(0, 1)])),
    (5, 32, (5, [(0, 5)])),
    (5, 2, (2, [(0, 2), (2, 2), (4, 1)])),
    (32, 32, (32, [(0, 32)])),
    (33, 32, (32, [(0, 32), (32, 1)])),
    (64, 32, (32, [(0, 32), (32, 32)])),
    (64, 5, (5, [(s, min(5, 64 - s)) for s in range(0, 64, 5)])),
    (0, 8, (0, [])),
])
def test_clip_plan(n, bs, expect):
    B, chunks = hostops.clip_plan(n, bs)
    assert (B, chunks) == expect
    assert sum(c for _, c in chunks) == n and all(c <= B for _, c in chunks)
    assert all(chunks[i][0] + chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))


def test_clip_plan_rejects_batch_size():
    with pytest.raises(ValueError):
        hostops.clip_plan(5, 0)


@pytest.fixture
def seg_model(monkeypatch):
    m = YOLO("synthetic:n-seg", dtype="fp32")

    def no_engine(*a, **k):
        raise AssertionError("an engine was built before the arguments were checked")

    monkeypatch.setattr(m, "_engine", no_engine)
    return m


def test_predict_clip_argument_errors(seg_model, monkeypatch):
    f = np.zeros((72, 128, 3), np.uint8)
    with pytest.raises(ValueError, match="batch_size"):
        seg_model.predict_clip([f], batch_size=0)
    with pytest.raises(ValueError, match="differ in shape"):
        seg_model.predict_clip([f, np.zeros((72, 130, 3), np.uint8)])
    with pytest.raises(TypeError):
        seg_model.predict_clip([f.astype(np.float32)])
    with pytest.raises(TypeError):
        seg_model.predict_clip([np.zeros((72, 128), np.uint8)])
    with pytest.raises(TypeError):
        seg_model.predict_clip([np.zeros((72, 128, 4), np.uint8)])
    with pytest.raises(TypeError):
        seg_model.predict_clip(torch.zeros((2, 72, 128, 3), dtype=torch.uint8))           # a tensor on the host, not the engine's device
    from yolo_puncture_amd import predictor
    monkeypatch.setattr(predictor, "MASK_POLYGON_STRATEGY", "biggest")
    with pytest.raises(ValueError, match="MASK_POLYGON_STRATEGY"):
        seg_model.predict_clip([f])
    monkeypatch.setattr(predictor, "MASK_POLYGON_STRATEGY", "all")
    r = seg_model.predict_clip([])
    assert isinstance(r, ClipResults) and tuple(r) == ([], [], []) and r.detected == [] and r.conf == [] and r.xyxy == []
    boxes, coords, lens = r
    assert boxes == coords == lens == []


def test_predict_clip_needs_seg(monkeypatch):
    m = YOLO("synthetic:n", dtype="fp32")
    monkeypatch.setattr(m, "_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("engine built")))
    with pytest.raises(ValueError, match="-seg"):
        m.predict_clip([np.zeros((72, 128, 3), np.uint8)])


def test_classifier_rejects_host_tensor():
    model = types.SimpleNamespace(device_index=0)
    with pytest.raises(TypeError):
        predict_and_find_start_inserted(model, torch.zeros((2, 72, 128, 3), dtype=torch.uint8), [(0, 0, 10, 10)] * 2)
