"""A 3840x2160 clip end to end: the masks the LDS contour kernel declines (csrc/contour.hip: bounding box beyond its bit image, W0 >= 2048 for
the scaled rectangle) are traced and measured on the device by the large path (csrc/contour_large.hip) - hostops.mask_polygon is never
reached. The oracle side runs with the large path switched off, i.e. as the host fallback computes the same clip."""
import numpy as np
import pytest
import torch

from suzuki_abe import find_contours_external_simple
from test_gpu_contour import _assert_rect, _rot_rect
from test_gpu_yolo_clip import clip_case, oracle_clip
from test_gpu_yolo_clip_input import assert_same_input, oracle_clip_input
from yolo_puncture_amd import hostops, predictor
from yolo_puncture_amd.engine import Engine
from yolo_puncture_amd.predictor import Masks

pytestmark = pytest.mark.gpu


def _needle_4k():
    """the first mask of test_gpu_contour_large.LARGE: a shaft 1800 px long and 50 px wide in a 4K frame, bounding box 1643x827"""
    return _rot_rect(2160, 3840, 1900, 1100, 900, 25, 0.45)


def test_masks_xy_of_a_4k_mask_stays_on_the_device(monkeypatch):
    mask = _needle_4k()
    want = np.concatenate(find_contours_external_simple(mask.astype(bool))).astype(np.int32)

    def no_host(*a, **k):
        pytest.fail("hostops.mask_polygon was called: the 4K mask fell back to the host trace")

    monkeypatch.setattr(hostops, "mask_polygon", no_host)
    u8 = torch.from_numpy(mask)[None].cuda()
    masks = Masks(None, (2160, 3840), u8=u8)
    poly = masks.xy[0]
    assert poly.dtype == np.float32 and np.array_equal(poly, want.astype(np.float32))
    length, ratio = masks.min_rect_len(0)
    _assert_rect((length, length / ratio), want, "needle_4k")
    assert 1790 < length < 1810 and 48 < length / ratio < 53


def upsample_4k(frames_720p):
    """720x1280 frames -> 3x nearest -> 2160x3840"""
    return [np.ascontiguousarray(np.repeat(np.repeat(f, 3, 0), 3, 1)) for f in frames_720p]


def _needle_in_best_masks(monkeypatch):
    """The needle above is OR-ed into the best detection's 4K retina mask of every frame, on both sides alike: Engine.masks (predict(), the
    oracle: row 0 is the best row) and Engine.masks_frames (predict_clip: one mask per detected frame). Each such mask keeps its own
    blobs and has a bounding box of at least 1643x827, which the LDS kernel declines."""
    real_masks, real_frames = Engine.masks, Engine.masks_frames
    needle = torch.from_numpy(_needle_4k()).cuda()

    def masks(self, b, coeff, boxes, out_hw, retina=True, **k):
        m, ids, kept = real_masks(self, b, coeff, boxes, out_hw, retina=retina, **k)
        if retina and tuple(out_hw) == (2160, 3840) and m is not None and m.shape[0]:
            torch.maximum(m[0], needle, out=m[0])
        return m, ids, kept

    def masks_frames(self, frame_idx, coeff, boxes, out_hw, out=None, retina=True):
        m = real_frames(self, frame_idx, coeff, boxes, out_hw, out=out, retina=retina)
        if retina and tuple(out_hw) == (2160, 3840) and m.shape[0]:
            torch.maximum(m, needle[None], out=m)
        return m

    monkeypatch.setattr(Engine, "masks", masks)
    monkeypatch.setattr(Engine, "masks_frames", masks_frames)


def _decline_everything(masks, max_pts=None, want_rect=True, strategy="all", want_parts=False, orig_hw=None):
    n = int(masks.shape[0])
    out = ([None] * n, np.zeros((n, 2)))
    return out + ([None] * n,) if want_parts else out


@pytest.mark.parametrize("retina", [True, False], ids=["retina", "input"])
def test_predict_clip_4k(retina, tmp_path_factory, monkeypatch):
    """The clip of test_gpu_yolo_clip.clip_case("11") (its first seed, its conf), first 7 frames, upsampled to 3840x2160, batch_size=4.
    retina_masks=True: whether the synthetic model's own masks outgrow the LDS image was not relied upon - the 4K needle of the first test
    is OR-ed into every detected frame's mask on both sides (see _needle_in_best_masks), so the LDS pass declines each of them;
    retina_masks=False: the masks are 384x640 and every frame's scaled rectangle is declined by the LDS pass (W0 = 3840). Either way the
    host trace and the host rectangle are never reached on the side under test, while the oracle side ends on them."""
    model, frames, conf = clip_case("11", tmp_path_factory)
    frames = upsample_4k(frames[:7])
    if retina:
        _needle_in_best_masks(monkeypatch)
    with monkeypatch.context() as mp:                                   # the oracle: as the parent commit computes it, on the host
        mp.setattr(predictor, "mask_contours_large_device", _decline_everything)
        ref = oracle_clip(model, frames, conf, 4) if retina else oracle_clip_input(model, frames, conf, 4)
    assert any(c is not None for c in ref[1]), "no frame of the 4K clip detects anything"

    real = predictor.mask_contours_device
    declined, host_calls, host_rects = [], [], []

    def recording(masks, *a, **k):
        out = real(masks, *a, **k)
        declined.extend(p is None or (k.get("orig_hw") is not None and out[1][t][0] < 0) for t, p in enumerate(out[0]))
        return out

    real_polygon, real_rect_len = hostops.mask_polygon, hostops.get_coord_min_rect_len
    monkeypatch.setattr(predictor, "mask_contours_device", recording)
    monkeypatch.setattr(hostops, "mask_polygon", lambda *a, **k: (host_calls.append(1), real_polygon(*a, **k))[1])
    monkeypatch.setattr(hostops, "get_coord_min_rect_len", lambda c: (host_rects.append(len(c)), real_rect_len(c))[1])
    got = model.predict_clip(frames, conf=conf, batch_size=4, retina_masks=retina)
    assert any(got.detected)
    assert any(declined), "the premise: the LDS pass declines at least one mask (or rectangle) of this clip"
    assert not host_calls, "hostops.mask_polygon was reached"
    if not retina:
        assert all(n < 3 for n in host_rects), "hostops.get_coord_min_rect_len was reached with a polygon"
    # boxes and polygons exactly; lengths in the tolerance form: the oracle measured the declined masks on the host
    assert_same_input(got, ref)
