"""`imgsz=1280` through the drop-in surface: a 1080p frame letterboxes to 736x1280 (19320 anchors, 920 attention tokens), which the
engine refused before the heads' large forms. predict() returns boxes in frame pixels, retina masks at the frame size and masks.xy;
predict_clip(imgsz=1280) equals per-frame predict() on the same frames, as test_gpu_yolo_clip.py asserts it at 640; a same-shape group
larger than the engine's largest batch is split and gives the same rows."""
import numpy as np
import pytest
import torch

from helpers import rand_image
from test_gpu_yolo_clip import assert_same, oracle_clip, v10_seg_state
from yolo_puncture_amd import hostops
from yolo_puncture_amd.engine import Engine
from yolo_puncture_amd.predictor import YOLO
from yolo_puncture_amd.weights import save_as_ultralytics_pt

pytestmark = pytest.mark.gpu
N = 3


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """-> (YOLO on a v10-N-seg checkpoint calibrated on the letterboxed frames, N 1080p frames, conf)"""
    frames = [f.numpy() for f in rand_image((N, 1080, 1920, 3), seed=9)]
    boxed = [hostops.letterbox(f, 1280)[0] for f in frames]
    assert boxed[0].shape == (736, 1280, 3)
    path = str(tmp_path_factory.mktemp("large") / "v10n-seg.pt")
    save_as_ultralytics_pt(v10_seg_state(boxed), path)
    model = YOLO(path)
    model._engine().set_autotune(False)
    best = [float(r.boxes.cpu().numpy().conf.max()) for r in model.predict(frames, conf=0.01, imgsz=1280)]
    return model, frames, min(0.25, 0.5 * min(best))


def test_predict_1080p_at_imgsz_1280(case):
    model, frames, conf = case
    eng = model._engine()
    r = model.predict(frames[0], conf=conf, imgsz=1280, retina_masks=True)[0]
    ops = eng.plan(1, 736, 1280)                               # (the plan predict() made: same shape, kept as it is)
    assert "head_select_large_kernel" in ops[-1]["kernel"]
    b = r.boxes.cpu().numpy()
    n = len(b.cls)
    assert n >= 1 and b.xyxy.shape == (n, 4)
    assert float(b.xyxy.min()) >= 0.0 and float(b.xyxy[:, [0, 2]].max()) <= 1920.0 and float(b.xyxy[:, [1, 3]].max()) <= 1080.0
    assert tuple(r.masks.data.shape) == (n, 1080, 1920)
    assert len(r.masks.xy) == n
    big = int(np.argmax([int(m.sum()) for m in r.masks.data.cpu()]))
    poly = r.masks.xy[big]
    assert poly.ndim == 2 and poly.shape[1] == 2 and len(poly) >= 3
    assert float(poly[:, 0].max()) <= 1920.0 and float(poly[:, 1].max()) <= 1080.0
    # the same rows as the engine gives on the letterboxed frame, scaled back
    boxed = torch.from_numpy(hostops.letterbox(frames[0], 1280)[0][None]).cuda()
    det = eng.forward(boxed)["det"][0].cpu()
    det = det[det[:, 4] > conf]
    assert det.shape[0] == n
    want = hostops.scale_boxes_t((736, 1280), det[:, :4].clone(), (1080, 1920))
    assert np.array_equal(b.xyxy, want.numpy()) and np.array_equal(b.conf, det[:, 4].numpy())


def test_predict_clip_at_imgsz_1280_matches_predict(case, monkeypatch):
    model, frames, conf = case
    predict = model.predict
    monkeypatch.setattr(model, "predict", lambda *a, **k: predict(*a, imgsz=1280, **k))      # oracle_clip calls predict(chunk, conf=, retina_masks=)
    for bs in (1, 2, 32):
        ref = oracle_clip(model, frames, conf, bs)
        assert any(c is not None for c in ref[1])
        got = model.predict_clip(frames, conf=conf, batch_size=bs, imgsz=1280)
        assert_same(got, ref)


def test_group_larger_than_max_batch_is_split(case, monkeypatch):
    """With the engine's largest batch forced down to 2, predict() runs the three same-shape frames as 2 + 1 and predict_clip in chunks
    of 2: the same rows as those very runs made by hand."""
    model, frames, conf = case
    by_hand = model.predict(frames[:2], conf=conf, imgsz=1280) + model.predict(frames[2:], conf=conf, imgsz=1280)
    clip_by_hand = model.predict_clip(frames, conf=conf, batch_size=2, imgsz=1280)
    planned = []
    forward = Engine.forward
    monkeypatch.setattr(Engine, "max_batch", lambda self, H, W: 2)
    monkeypatch.setattr(Engine, "forward", lambda self, im, out=None: (planned.append(int(im.shape[0])), forward(self, im, out))[1])
    split = model.predict(frames, conf=conf, imgsz=1280)
    assert planned == [2, 1]
    for a, b in zip(split, by_hand):
        pa, pb = a.boxes.cpu().numpy(), b.boxes.cpu().numpy()
        assert np.array_equal(pa.xyxy, pb.xyxy) and np.array_equal(pa.conf, pb.conf) and np.array_equal(pa.cls, pb.cls)
    del planned[:]
    got = model.predict_clip(frames, conf=conf, batch_size=32, imgsz=1280)
    assert planned == [2, 2]
    assert_same(got, clip_by_hand)
