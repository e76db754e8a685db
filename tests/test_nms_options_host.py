"""tests/nms_option_cases.py on the CPU: the reference with default options is the oracle's nms_postprocess, every case does what its name
says, every deliberate mistake (nms_option_cases.VARIANTS) changes the rows of the case aimed at it, and yp_set_nms_options refuses bad
arguments on an engine that never touches the GPU."""
import ctypes as C

import pytest
import torch

import head_cases as H
import nms_option_cases as N

BY_ID = {c.id: c for c in N.CASES}


def _case(cid):
    return N.resolve(BY_ID[cid])


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b))


def _counts(rows):
    return [r[0].shape[0] for r in rows]


@pytest.mark.parametrize("c", H.NMS_CASES, ids=H.nms_id)
def test_default_options_are_the_oracle(c):
    rows, boxes, scores = H.nms_reference(c)
    t = H.nms_inputs(c)
    got = [N.nms_postprocess_opts(boxes[b], scores[b], t["cf"][b], c.conf, c.iou, c.max_det, **N.DEFAULTS) for b in range(H.B)]
    assert _same(got, rows)


def test_case_ids_are_unique_and_cover_both_paths():
    assert len(BY_ID) == len(N.CASES)
    assert any(N.n_anchors(c) > H.CAP for c in N.CASES) and any(N.n_anchors(c) <= H.CAP for c in N.CASES)
    assert N.n_anchors(BY_ID["past_cap-default"]) == 16800 and N.is_default(BY_ID["past_cap-default"])


def test_past_the_cap():
    full, dflt, cut = _case("past_cap-max_nms30000"), _case("past_cap-default"), _case("past_cap-cut_in_round2")
    assert N.inputs(full)["info"]["nblk"] == 280
    rf, rd, rc = N.reference(full), N.reference(dflt), N.reference(cut)
    for b in range(N.B):
        assert N.sorted_candidates(full, b).numel() == 16800
        ranks = N.late_survivor_ranks(full, b)
        assert ranks[0] >= N.NCAP, "the four late survivors lie behind the default cut"
        assert torch.equal(rf[b][1][:276], rd[b][1]), "the default rows are a prefix of the whole list's"
    assert _counts(rf) == [280, 280] and _counts(rd) == [276, 276]
    # the cut of the third case falls between two of image 0's late survivors: a partial second round, some of the four rows
    ranks = N.late_survivor_ranks(full, 0)
    assert ranks[0] < cut.max_nms <= ranks[3] and N.NCAP < cut.max_nms < 2 * N.NCAP
    assert 276 < _counts(rc)[0] < 280 and torch.equal(rc[0][1], rf[0][1][:_counts(rc)[0]])


def test_second_round_holds_a_victim_of_the_first():
    c = _case("past_cap_tail-max_nms30000")
    rows = N.reference(c)
    assert _counts(rows) == [280, 280]
    for b, a in enumerate(N.inputs(c)["info"]["moved"]):
        order = N.sorted_candidates(c, b)
        assert int(order[-1]) == a, "the re-scored anchor is the last of the list: in the second round"
        blk = N.inputs(c)["info"]["block_of"]
        first = next(int(x) for x in order if blk[x] == blk[a])
        assert int(torch.nonzero(order == first)[0]) < N.NCAP and first in rows[b][1].tolist() and a not in rows[b][1].tolist()


@pytest.mark.parametrize("cid,total", [("blocks-M-max_nms2000", 106), ("blocks-L-max_nms5000", 134)])
def test_cut_below_the_count(cid, total):
    c = _case(cid)
    rows, whole = N.reference(c), N.reference(c, max_nms=N.NCAP)
    for b in range(N.B):
        assert N.sorted_candidates(c, b).numel() > c.max_nms
        n = rows[b][0].shape[0]
        assert n < whole[b][0].shape[0] == total and torch.equal(rows[b][1], whole[b][1][:n])
        pos = {int(a): i for i, a in enumerate(N.sorted_candidates(c, b))}
        assert all(pos[int(a)] < c.max_nms for a in rows[b][1]) and pos[int(whole[b][1][n])] >= c.max_nms


def test_agnostic_cases():
    c = _case("same_box-agnostic")
    a0, a1 = N.inputs(c)["info"]["pair"]
    rows, dflt = N.reference(c), N.reference(c, agnostic=False)
    assert a0 in dflt[0][1].tolist() and a1 in dflt[0][1].tolist(), "one box in two classes: both stay by default"
    assert a0 in rows[0][1].tolist() and a1 not in rows[0][1].tolist(), "the second goes under agnostic"
    assert _counts(rows)[0] == _counts(dflt)[0] - 1 and _counts(rows)[1] == _counts(dflt)[1]
    for cid in ("argmax-agnostic", "equal_scores-agnostic"):
        c = _case(cid)
        rows, dflt = N.reference(c), N.reference(c, agnostic=False)
        assert all(set(r[1].tolist()) <= set(d[1].tolist()) for r, d in zip(rows, dflt)), "agnostic only ever drops more"
    assert not _same(N.reference(_case("argmax-agnostic")), N.reference(_case("argmax-agnostic"), agnostic=False))
    # blocks: the boxes of two different blocks meet with IoU <= 0.25 < iou, so agnostic changes nothing
    c = _case("blocks-M-agnostic")
    boxes = torch.unique(N.decoded(c)[0][0], dim=0)
    assert boxes.shape[0] == 106
    lt, rb = torch.maximum(boxes[:, None, :2], boxes[None, :, :2]), torch.minimum(boxes[:, None, 2:], boxes[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(-1)
    area = (boxes[:, 2:] - boxes[:, :2]).prod(-1)
    iou = inter / (area[:, None] + area[None] - inter)
    iou.fill_diagonal_(0)
    assert float(iou.max()) <= 0.25 < c.iou
    assert _same(N.reference(c), N.reference(c, agnostic=False))


def test_class_cases():
    for cid in ("random_boxes-classes1", "random_boxes-classes0_2"):
        c = _case(cid)
        rows, dflt = N.reference(c), N.reference(c, classes=None)
        for b in range(N.B):
            keep = torch.isin(dflt[b][0][:, 5].long(), torch.tensor(c.classes))
            assert 0 < rows[b][0].shape[0] < dflt[b][0].shape[0]
            assert set(rows[b][0][:, 5].long().tolist()) == set(c.classes)
            # (classes never interact in class-offset NMS: the set's rows are the default's rows of those classes, none cut by max_det here)
            assert torch.equal(rows[b][1], dflt[b][1][keep])
    c = _case("none_and_many-empties_image1")
    assert _counts(N.reference(c)) == [0, 0] and _counts(N.reference(c, classes=None)) == [0, 300]
    c = _case("random_boxes-class_without_candidate")
    assert _counts(N.reference(c)) == [0, 0] and min(_counts(N.reference(c, classes=None))) > 0
    c = _case("random_boxes-all_classes")
    assert len(c.classes) == N.NC and _same(N.reference(c), N.reference(c, classes=None))


def test_filter_comes_before_the_cut():
    """the class set acts on the candidates, the cut on what the set leaves. With max_nms = 2000 every block of the scene except the late
    ones has met its survivor under either order (the rows agree); with max_nms = 200 the order of the two steps decides the rows"""
    c = _case("blocks-M-even-max_nms2000")
    assert all(N.sorted_candidates(c, b).numel() > c.max_nms for b in range(N.B)), "the filtered list is still longer than the cut"
    assert all(set(r[0][:, 5].long().tolist()) <= set(N.EVEN) for r in N.reference(c))
    assert _counts(N.reference(c)) < _counts(N.reference(c, max_nms=N.NCAP))
    c = _case("blocks-M-even-max_nms200")
    right, wrong = N.reference(c), N.reference(c, "cut_before_filter")
    assert all(w[0].shape[0] < r[0].shape[0] for r, w in zip(right, wrong)), "cut first: about half of the 200 are of the set"


VARIANT_TARGETS = {
    "cut_before_filter": "blocks-M-even-max_nms200",
    "offset_under_agnostic": "same_box-agnostic",
    "class_shortcut_under_agnostic": "same_box-agnostic",
    "rounds_not_presuppressed": "past_cap_tail-max_nms30000",
    "cut_by_score_only": "past_cap-cut_in_round2",
}


@pytest.mark.parametrize("variant", N.VARIANTS)
def test_each_mistake_changes_the_case_aimed_at_it(variant):
    c = _case(VARIANT_TARGETS[variant])
    right, wrong = N.reference(c), N.reference(c, variant)
    assert not _same(right, wrong), (variant, c.id)
    if variant == "rounds_not_presuppressed":
        assert all(n > 280 for n in _counts(wrong)), "victims of first-round boxes come back"
    if variant == "cut_before_filter":
        assert all(N.sorted_candidates(c, b).numel() > c.max_nms for b in range(N.B)), "the filtered list is still longer than the cut"
    # and a variant leaves the default options alone where its step does not act
    d = _case("random_boxes-classes1")
    if variant != "cut_by_score_only":
        assert _same(N.reference(d), N.reference(d, variant))


def test_default_plan_keeps_its_kernels():
    """The plan names the default kernels unless an option differs from its default; the option forms are kernels of their own, on both
    paths, and setting the defaults again names the default kernels again. Host only."""
    from yolo_puncture_amd.engine import Engine
    e = Engine("n", 80, True, "bf16", 0, family="11")
    names = {640: ("head_nms_kernel", "head_nms_opt_kernel"),
             1280: ("head_nms_gather_kernel + head_nms_large_kernel", "head_nms_gather_opt_kernel + head_nms_large_opt_kernel")}
    head = lambda s: e.plan(1, s, s)[-1]["kernel"]
    for s, (dflt, opt) in names.items():
        assert head(s) == dflt
        for o in (dict(max_nms=30000), dict(classes=[0]), dict(agnostic=True), dict(max_nms=16383)):
            e.set_nms_options(**o)
            assert head(s) == opt, (s, o)
            e.set_nms_options()
            assert head(s) == dflt
        e.set_nms_options(classes=list(range(80)))               # (a set is a set, even one that covers every class)
        assert head(s) == opt
        e.set_nms_options(classes=[], agnostic=False, max_nms=16384)
        assert head(s) == dflt
    e.close()


def test_set_nms_options_argument_errors():
    """yp_set_nms_options through ctypes: validation happens before anything touches a device (the engines are never finalized)."""
    from yolo_puncture_amd.engine import Engine, YolopError, load_library
    lib = load_library()
    e = Engine("n", 80, True, "bf16", 0, family="11")
    ids = lambda *v: (C.c_int32 * len(v))(*v)
    assert lib.yp_set_nms_options(e._h, ids(0, 79), 2, 1, 30000) == 0
    assert lib.yp_set_nms_options(e._h, None, 0, 0, 16384) == 0
    assert lib.yp_set_nms_options(e._h, ids(3), 0, 0, 16384) == 0            # n_classes == 0: all classes
    for bad in (80, -1, 1 << 20):
        assert lib.yp_set_nms_options(e._h, ids(1, bad), 2, 0, 16384) < 0
        assert b"class id" in lib.yp_last_error() and str(bad).encode() in lib.yp_last_error()
    for bad in (0, -5, 294912 + 1):
        assert lib.yp_set_nms_options(e._h, None, 0, 0, bad) < 0 and b"max_nms" in lib.yp_last_error()
    assert lib.yp_set_nms_options(e._h, None, 0, 0, 294912) == 0
    assert lib.yp_set_nms_options(e._h, ids(1), -1, 0, 16384) < 0
    assert lib.yp_set_nms_options(None, None, 0, 0, 16384) < 0
    e.set_nms_options(classes=7, agnostic=True, max_nms=30000)                 # the Python form: an int, a sequence, None
    e.set_nms_options(classes=[1, 2, 3])
    e.set_nms_options()
    with pytest.raises(YolopError, match="class id"):
        e.set_nms_options(classes=[80])
    e.close()
    v10 = Engine("n", 80, True, "bf16", 0)
    assert lib.yp_set_nms_options(v10._h, None, 0, 0, 16384) < 0 and b"v10" in lib.yp_last_error() and b"host" in lib.yp_last_error()
    with pytest.raises(YolopError, match="no NMS"):
        v10.set_nms_options(classes=[1])
    v10.close()
