"""The clip form of `auto_segment` without a GPU: the workspace grouping (hostops.group_frames_by_workspace), yp_id_masks_frames_workspace,
every argument check of yp_id_masks_frames (all of them run before the device is touched), and the clip arguments of
YOLO.predict_id_mask_clip / auto_segment_clip, refused before any engine is built."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from yolo_puncture_amd import hostops
from yolo_puncture_amd.engine import ID_MASKS_FRAMES_BUDGET, MAX_MASKS, Engine
from yolo_puncture_amd.predictor import YOLO

YP_ERR_ARG, YP_ERR_STATE = -1, -2
AA_KMAX = 36


# ---- grouping ------------------------------------------------------------------------------------------------------------------------------
def _linear(per_frame, per_row):
    return lambda n, k: 256 + per_frame * k + per_row * n


def _check_cover(groups, n_frames):
    flat = [j for _, js in groups for j in js]
    assert flat == list(range(n_frames)), "every frame once, in order"
    assert all(js for _, js in groups) and all(len(js) == 1 for b, js in groups if not b)


def test_grouping_keeps_order_and_budget():
    counts = [3, 0, 7, 7, 0, 0, 12, 1, 5]
    ws = _linear(100, 1000)
    for budget in (10 ** 9, 20000, 13000, 8000, 1400):
        groups = hostops.group_frames_by_workspace(counts, ws, budget)
        _check_cover(groups, len(counts))
        for batched, js in groups:
            need = ws(sum(counts[j] for j in js), len(js))
            assert (need <= budget) == batched
        # greedy: a batched group could not have taken the next frame as well
        for (b0, js0), (b1, js1) in zip(groups, groups[1:]):
            if b0 and b1:
                assert ws(sum(counts[j] for j in js0) + counts[js1[0]], len(js0) + 1) > budget
    assert hostops.group_frames_by_workspace(counts, ws, 10 ** 9) == [(True, list(range(len(counts))))]
    assert hostops.group_frames_by_workspace([], ws, 10 ** 9) == []


def test_grouping_hands_a_frame_that_does_not_fit_to_the_one_frame_path():
    ws = _linear(0, 1000)
    groups = hostops.group_frames_by_workspace([2, 50, 3, 0, 4], ws, 10000)
    assert groups == [(True, [0]), (False, [1]), (True, [2, 3, 4])]
    # sizes the query declines (0) cannot be batched either; neither can more rows than one call takes
    assert hostops.group_frames_by_workspace([1, 1], lambda n, k: 0, 10 ** 9) == [(False, [0]), (False, [1])]
    assert hostops.group_frames_by_workspace([3, 3, 3], ws, 10 ** 9, max_rows=6) == [(True, [0, 1]), (True, [2])]
    with pytest.raises(ValueError):
        hostops.group_frames_by_workspace([1, -1], ws, 10 ** 9)


def test_grouping_of_frames_without_masks():
    ws = _linear(100, 1000)
    assert hostops.group_frames_by_workspace([0, 0, 0], ws, 10 ** 6) == [(True, [0, 1, 2])]
    assert hostops.group_frames_by_workspace([0, 0, 0], ws, 256 + 200) == [(True, [0, 1]), (True, [2])]
    assert hostops.group_frames_by_workspace([0, 9, 0], ws, 5000) == [(True, [0]), (False, [1]), (True, [2])]


# ---- workspace query -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    e = Engine("n", 80, True, "fp32", 0)
    assert e.id_masks_frames_workspace(5, 2, (96, 160)) == 0, "no plan yet"
    e.plan(4, 96, 160)                                      # prototypes 24 x 40; a (96,160) output takes the whole map
    yield e
    e.close()


def _payload(n, k, hw, out_hw):
    """the bytes the kernels use, block by block (csrc/mask.hip): the one-frame tail's blocks with n = n_total, and frame_idx | row_off"""
    (oh, ow), (rh, rw) = hw, out_hw
    ch, cw = 24, 40
    blocks = [(2 * k + 1) * 4, n * 4, n * 4, n * ch * cw * 4, n * oh * ow]
    if out_hw != hw:
        blocks += [n * 8, 2 * (rw + rh) * 4, (rw + rh) * AA_KMAX * 4, n * oh * rw * 4, n * rh * rw]
    return blocks


def test_workspace_query(planned):
    e = planned
    for out_hw in ((96, 160), (144, 240), (6, 10)):
        prev = 0
        for n in (0, 1, 2, 17, 480, 481, 5000):
            for k in (1, 2, 33):
                got = e.id_masks_frames_workspace(n, k, (96, 160), out_hw)
                blocks = _payload(n, k, (96, 160), out_hw)
                # the relation: every block of the layout rounded up to 256 bytes, nothing else - for k = 1 that is the one-frame tail's
                # buffers (masks_workspace_bytes, which keeps 768 bytes of slack instead) plus the 12 bytes of frame_idx | row_off
                assert got == sum((b + 255) // 256 * 256 for b in blocks), (n, k, out_hw)
                assert sum(blocks) <= got < sum(blocks) + 256 * len(blocks)
            a, b = (e.id_masks_frames_workspace(n, k, (96, 160), out_hw) for k in (1, 64))
            assert prev < a <= b, "monotone in n_total and in k"
            prev = a
    assert e.id_masks_frames_workspace(5, 70, (96, 160)) > e.id_masks_frames_workspace(5, 2, (96, 160)), "strictly, once the index block grows"
    assert e.id_masks_frames_workspace(5, 2, (96, 160), (96, 160)) == e.id_masks_frames_workspace(5, 2, (96, 160))
    # sizes the call refuses
    for bad in ((5, 0, (96, 160), None), (5, 2, (0, 160), None), (5, 2, (96, 160), (5, 10)), (70000, 2, (96, 160), None), (5, 70000, (96, 160), None),
                (5, 2, (46341, 46341), None), (-1, 2, (96, 160), None), (65535, 2, (720, 1280), None)):
        assert e.id_masks_frames_workspace(*bad) == 0, bad
    assert ID_MASKS_FRAMES_BUDGET == 1 << 30 and MAX_MASKS == 480
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yolop.h")).read()
    assert "#define YP_ID_MASKS_FRAMES_BUDGET (1ull << 30)" in hdr and "#define YP_MAX_MASKS 480" in hdr
    d = Engine("n", 80, False, "fp32", 0)
    d.plan(4, 96, 160)
    assert d.id_masks_frames_workspace(5, 2, (96, 160)) == 0, "a detect engine has no prototypes"
    d.close()


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------
def _call(e, fidx, row_off, k, hw=(96, 160), out_hw=(96, 160), coeff=True, boxes=True, ids=True, kept=True, handle=True):
    stub = (C.c_float * 64)()                                # never read or written: every call here is refused first
    fi = None if fidx is None else np.asarray(fidx, dtype=np.int32)
    ro = None if row_off is None else np.asarray(row_off, dtype=np.int32)
    p = lambda on: C.cast(stub, C.c_void_p) if on else None
    rc = e.lib.yp_id_masks_frames(e._h if handle else None, None if fi is None else fi.ctypes.data_as(C.c_void_p),
                                  None if ro is None else ro.ctypes.data_as(C.c_void_p), k, p(coeff), p(boxes), hw[0], hw[1], out_hw[0], out_hw[1],
                                  p(ids), p(kept), 1, 100, None)
    return rc, e.lib.yp_last_error().decode()


def test_every_refusal_names_the_call(planned):
    e = planned
    ok = dict(fidx=[0, 3, 3], row_off=[0, 2, 2, 5], k=3)
    big = 46341
    refusals = {
        "null engine": dict(handle=False),
        "k = 0": dict(k=0),
        "k < 0": dict(k=-1),
        "null frame_idx": dict(fidx=None),
        "null row_off": dict(row_off=None),
        "null ids_out": dict(ids=False),
        "null coeff": dict(coeff=False),
        "null boxes": dict(boxes=False),
        "null kept_out": dict(kept=False),
        "row_off[0] != 0": dict(row_off=[1, 2, 2, 5]),
        "row_off decreases": dict(row_off=[0, 2, 1, 5]),
        "481 masks in a frame": dict(row_off=[0, 2, 2 + MAX_MASKS + 1, 2 + MAX_MASKS + 1]),
        "frame index == B": dict(fidx=[0, 4, 3]),
        "frame index < 0": dict(fidx=[0, -1, 3]),
        "oh = 0": dict(hw=(0, 160)),
        "ow < 0": dict(hw=(96, -160)),
        "rh = 0": dict(out_hw=(0, 240)),
        "rw = 0": dict(out_hw=(144, 0)),
        "16x": dict(out_hw=(5, 160)),
        "16x in x": dict(out_hw=(96, 9)),
        "a plane of 2^31 pixels": dict(hw=(big, big), out_hw=(big, big)),
        "oh * rw >= 2^31": dict(hw=(65536, 4096), out_hw=(4096, 32768)),
        "n_total * plane >= 2^32": dict(hw=(2048, 2048), out_hw=(2048, 2048), fidx=[0] * 4, k=4, row_off=[0, 300, 600, 900, 1200]),
    }
    for what, kw in refusals.items():
        rc, msg = _call(e, **{**ok, **kw})
        assert rc == YP_ERR_ARG and "yp_id_masks_frames" in msg, (what, rc, msg)
    # more than 65535 masks in all / frames: row_off itself says so
    k = 140
    rc, msg = _call(e, [0] * k, [MAX_MASKS * j for j in range(k + 1)], k)
    assert rc == YP_ERR_ARG and "65535 masks" in msg
    rc, msg = _call(e, [0] * 65536, [0] * 65537, 65536)
    assert rc == YP_ERR_ARG and "65535 frames" in msg
    # valid arguments (480 masks in a frame, n_j = 0 frames, the 16x limit itself): a plan, but no forward - no device here
    for kw in ({}, dict(row_off=[0, MAX_MASKS, MAX_MASKS, MAX_MASKS + 3]), dict(out_hw=(6, 10)), dict(out_hw=(144, 240)),
               dict(row_off=[0, 0, 0, 0], coeff=False, boxes=False, kept=False)):
        rc, msg = _call(e, **{**ok, **kw})
        assert rc == YP_ERR_STATE and "yp_id_masks_frames" in msg and "no forward" in msg, (kw, rc, msg)


def test_state_errors():
    e = Engine("n", 80, True, "fp32", 0)                    # never planned
    rc, msg = _call(e, [0, 3, 3], [0, 2, 2, 5], 3)
    assert rc == YP_ERR_STATE and "yp_id_masks_frames" in msg and "no forward" in msg
    e.close()
    d = Engine("n", 80, False, "fp32", 0)
    d.plan(4, 96, 160)
    rc, msg = _call(d, [0, 3, 3], [0, 2, 2, 5], 3)
    assert rc == YP_ERR_STATE and "yp_id_masks_frames" in msg and "YP_TASK_SEGMENT" in msg
    d.close()


def test_engine_wrapper_checks_before_the_call(planned):
    host = torch.zeros((5, 32))
    with pytest.raises(ValueError, match="counts"):
        planned.id_masks_frames([0, 1], [5], host, torch.zeros((5, 4)), (96, 160))
    with pytest.raises(ValueError, match="negative"):
        planned.id_masks_frames([0, 1], [6, -1], host, torch.zeros((5, 4)), (96, 160))
    with pytest.raises(ValueError, match="coeff"):
        planned.id_masks_frames([0, 1], [2, 3], host, torch.zeros((5, 4)), (96, 160))      # not on the device


# ---- the facade's arguments ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def seg_model(monkeypatch):
    m = YOLO("synthetic:n-seg", dtype="fp32")

    def no_engine(*a, **k):
        raise AssertionError("an engine was built before the arguments were checked")

    monkeypatch.setattr(m, "_engine", no_engine)
    return m


def _both(model):
    from yolo_puncture_amd import auto_segment_clip
    return (lambda images, **kw: model.predict_id_mask_clip(images, **kw),
            lambda images, **kw: auto_segment_clip({}, images, model, 36, True, **kw))


def test_clip_arguments_are_refused_in_predict_clips_words(seg_model):
    f = np.zeros((72, 128, 3), np.uint8)
    for call in _both(seg_model):
        with pytest.raises(ValueError, match="batch_size must be >= 1"):
            call([f], batch_size=0)
        with pytest.raises(ValueError, match="frames differ in shape"):
            call([f, np.zeros((72, 130, 3), np.uint8)])
        for bad in ([f.astype(np.float32)], [np.zeros((72, 128), np.uint8)], [np.zeros((72, 128, 4), np.uint8)], [f, "frame.png"],
                    torch.zeros((2, 72, 128, 3), dtype=torch.uint8),             # a tensor on the host, not the engine's device
                    torch.zeros((2, 72, 128, 3))):
            with pytest.raises(TypeError, match="expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor"):
                call(bad)
        assert call([]) == []
    with pytest.raises(TypeError, match="predict_clip expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor"):
        seg_model.predict_clip([f.astype(np.float32)])       # predict_clip's own words, as before


def test_clip_needs_a_segmentation_model(monkeypatch):
    m = YOLO("synthetic:n", dtype="fp32")
    monkeypatch.setattr(m, "_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("engine built")))
    with pytest.raises(ValueError, match="segmentation"):
        m.predict_id_mask_clip([np.zeros((72, 128, 3), np.uint8)])


def test_auto_segment_clip_is_exported():
    import yolo_puncture_amd
    from yolo_puncture_amd import deva_adapter
    assert yolo_puncture_amd.auto_segment_clip is deva_adapter.auto_segment_clip and yolo_puncture_amd.auto_segment is deva_adapter.auto_segment
