"""EfficientNet-B3 needle classifier, host side (no GPU): weight table of libyolop.so against the folded state dict, the state-dict key
list and parameter count of efficientnet_pytorch, the static padding table, checkpoint formats, crop geometry, insertion search and
repair against the test-side restatement (tests/effnet_ref.py)."""
import random

import numpy as np
import pytest
import torch

import effnet_ref as R
from yolo_puncture_amd import classify as C
from yolo_puncture_amd.engine import YolopError


def test_weight_table_matches_folded_state():
    e = C.ClassifierEngine("fp32", 0)
    exp = e.expected_weights()
    got = []
    for k, (w, b) in C.fold_state(C.synthetic_state(0)).items():
        got += [(k + ".weight", tuple(w.shape)), (k + ".bias", tuple(b.shape))]
    assert exp == got
    e.close()


def test_other_variants_are_refused():
    with pytest.raises(ValueError):
        C.ClassifierEngine("fp32", 0, name="efficientnet-b4")
    lib = C.load_library()
    C._declare(lib)
    h = C.C.c_void_p()
    for v in (0, 4, 5, 7):
        assert lib.yp_cls_create(v, 1, 0, C.C.byref(h)) < 0
        assert b"efficientnet-b3" in lib.yp_last_error()
    with pytest.raises(NotImplementedError):
        C._load_net("van_b0", checkpoint="x.pth")


def test_state_keys_and_parameter_count():
    st = C.synthetic_state(0)
    assert list(st) == R.keys()
    assert C.param_count() == 10_699_306
    assert sum(v.numel() for k, v in st.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) == 10_699_306
    assert len(C.block_specs()) == 26


def test_static_padding_table():
    t = C.padding_table()
    assert t == R.pads()
    assert t["_conv_stem"] == (0, 1)
    firsts = {2: (0, 1), 5: (2, 2), 8: (0, 1), 18: (2, 2)}            # stride-2 depthwise convs: stages 2, 3, 4, 6
    for i, b in enumerate(C.block_specs()):
        p = t[f"_blocks.{i}._depthwise_conv"]
        if b["s"] == 2:
            assert p == firsts[i]
        else:
            assert p == ((1, 1) if b["k"] == 3 else (2, 2))
    # computed from the real 380 input, stage 6's first depthwise conv would get (1, 2): the padding is for image size 300
    assert C.same_padding(24, 5, 2) == (1, 2) and t["_blocks.18._depthwise_conv"] == (2, 2)


def _roundtrip(tmp_path, obj, fname):
    p = tmp_path / fname
    torch.save(obj, p)
    return C.read_checkpoint(str(p))


def test_checkpoint_formats(tmp_path):
    st = C.synthetic_state(1)
    for obj, fn in ((st, "raw.pth"), ({"state_dict": {"module." + k: v for k, v in st.items()}, "epoch": 3}, "wrapped.pth"),
                    ({"state_dict": st, "state_dict_ema": st, "arch": "efficientnet_b3"}, "model_best.pth.tar")):
        got = _roundtrip(tmp_path, obj, fn)
        assert list(got) == list(st) and all(torch.equal(got[k], st[k]) for k in st)
    bad = dict(st)
    del bad["_blocks.3._se_reduce.bias"]
    with pytest.raises(KeyError, match="_blocks.3._se_reduce.bias"):
        _roundtrip(tmp_path, bad, "missing.pth")
    bad = dict(st, extra_head=torch.zeros(2))
    with pytest.raises(KeyError, match="extra_head"):
        _roundtrip(tmp_path, bad, "extra.pth")
    bad = dict(st)
    bad["_fc.weight"] = torch.zeros(3, 1536)
    with pytest.raises(ValueError, match="_fc.weight"):
        _roundtrip(tmp_path, bad, "shape.pth")
    with pytest.raises(FileNotFoundError):
        C.load_classify_net(name="nope.pth", weights_dir=str(tmp_path))


BOXES = [(100, 100, 200, 201), (101, 100, 200, 200), (0, 0, 10, 10), (1270, 710, 1280, 720), (0, 300, 20, 400), (600, 0, 700, 5),
         (1200, 300, 1279, 400), (0, 0, 1280, 720), (500, 200, 503, 207), (0, 0, 1920, 1080), (1000, 900, 1100, 1080)]


@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920), (300, 500), (500, 300), (200, 250), (380, 380)])
def test_crop_geometry(hw):
    h, w = hw
    rng = np.random.RandomState(h + w)
    frame = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    boxes = list(BOXES) + [(0, 0, w, h)]
    for _ in range(40):
        x1, y1 = rng.randint(0, w), rng.randint(0, h)
        boxes.append((x1, y1, rng.randint(x1, w + 1), rng.randint(y1, h + 1)))
    for bx in boxes:
        bx = tuple(min(v, lim) for v, lim in zip(bx, (w, h, w, h)))
        x0, y0, cw, ch = C.crop_geometry(bx, h, w)
        x1, y1, x2, y2 = R.crop_box(frame.shape, bx)
        assert (x0, y0, cw, ch) == (x1, y1, max(0, x2 - x1), max(0, y2 - y1)), bx
        np.testing.assert_array_equal(C.crop_roi(frame, bx), R.crop(frame, bx))


def _hand_cases():
    ones = [1] * 30
    return [
        ([0] * 30, [0.9] * 30, 20),                                   # no qualifying window
        ([1] * 10, [0.99] * 10, 20),                                  # shorter than judge_wnd
        (ones, [0.9] * 30, 20),                                       # exactly at 0.9: strict >, falls to 0.8
        (ones, [0.6] * 30, 20),                                       # exactly at the lowest threshold: no hit
        (ones, [0.95] * 30, 20),                                      # insertion at frame 0
        ([0] * 10 + [1] * 20, [0.8] * 10 + [0.95] * 20, 20),           # already correct around the cut
        ([0, 1, 0, 0, 1] + [1] * 25, [0.7, 0.65, 0.8, 0.9, 0.7] + [0.85] * 25, 20),
        ([0] * 5 + [1] * 18 + [0, 1] + [1] * 5, [0.7] * 5 + [0.85] * 25, 20),
        ([1, 1, 0, 1] + [1] * 26, [0.61, 0.7, 0.9, 0.95] + [0.75] * 26, 10),
    ]


def test_search_and_repair_hand_cases():
    for cls, prb, wnd in _hand_cases():
        idx = C.find_insert_index(cls, prb, wnd)
        assert idx == R.find_start(cls, prb, wnd), (cls, prb)
        a = C.fix_class_prob(list(cls), list(prb), idx)
        b = R.repair(list(cls), list(prb), idx)
        assert a == b
    assert C.find_insert_index(*_hand_cases()[0]) == 0
    assert C.find_insert_index(*_hand_cases()[1]) == 0
    assert C.find_insert_index(*_hand_cases()[4]) == 0
    assert C.fix_class_prob([1, 0, 1], [0.7, 0.8, 0.9], 1) == ([0, 0, 1], [0.6, 0.8, 0.9])


def test_search_and_repair_random():
    rng = random.Random(7)
    for _ in range(1000):
        n = rng.randint(0, 80)
        wnd = rng.choice([5, 10, 20])
        cut = rng.randint(0, n)
        flip = rng.random() * 0.3
        cls = [int((i >= cut) != (rng.random() < flip)) for i in range(n)]
        prb = [np.float32(rng.choice([0.6, 0.7, 0.8, 0.9, rng.uniform(0.5, 1.0)])) for _ in range(n)]
        idx = C.find_insert_index(cls, prb, wnd)
        assert idx == R.find_start(cls, prb, wnd)
        assert C.fix_class_prob(list(cls), list(prb), idx) == R.repair(list(cls), list(prb), idx)


def test_forward_needs_a_device():
    e = C.ClassifierEngine("fp32", 0)
    e.load_state(C.synthetic_state(0))
    if not torch.cuda.is_available():
        with pytest.raises(YolopError):
            e.finalize()
    e.close()
