"""CPU checks of tests/head_cases.py, for every case id tests/test_gpu_head_crafted.py uses: each case does what its name says (no case is
vacuous), its inputs keep the rules that make the comparison exact, and the fp32 and fp64 references agree wherever nothing saturates -
so a failure on the GPU is the kernel's."""
import pytest
import torch

import head_cases as H


def _assert_logit_rules(cls):
    """two logits are equal or their float32 sigmoids are >= 1e-5 apart; saturated ones are >= 20; nothing in (15, 17.5) or below -80"""
    u = torch.unique(cls)
    assert float(u.min()) >= -80.0 and not bool(((u > 15.0) & (u < 17.5)).any())
    sat = u >= 20.0
    assert bool((u[sat].sigmoid() == 1.0).all()) and bool((u[~sat] <= 15.0).all())
    s = u[~sat].sigmoid()
    real = s[u[~sat] > -80.0]                       # (the floor logit is one value: equal to itself)
    if real.numel() > 1:
        assert float((real[1:] - real[:-1]).min()) >= 1e-5, float((real[1:] - real[:-1]).min())
    if real.numel() and bool((u == -80.0).any()):
        assert float(real.min()) - float(torch.tensor(-80.0).sigmoid()) >= 1e-5


def _assert_onehot_exact(shape, dist, boxes32, boxes64, xywh):
    """oracle decode == (anchor -+ q) * stride bit for bit, in both precisions"""
    pts, strd = H.Oracle.make_anchors(H.levels(shape), dt=torch.float64)
    d = dist.double()
    want = torch.stack((pts[:, 0] - d[..., 0], pts[:, 1] - d[..., 1], pts[:, 0] + d[..., 2], pts[:, 1] + d[..., 3]), -1) * strd[None, :, None]
    assert torch.equal(boxes32.double(), want) and torch.equal(boxes64.double(), want)


@pytest.mark.parametrize("c", H.V10_CASES, ids=H.v10_id)
def test_v10_case(c):
    t = H.v10_inputs(c)
    A = H.n_anchors(c.shape)
    k = min(c.max_det, A)
    _assert_logit_rules(t["cls"])
    det, idx, boxes = H.v10_reference(c, "fp32")
    det64, idx64, boxes64 = H.v10_reference(c, "fp64")
    assert det.shape == (H.B, k, 6) and idx.shape == (H.B, k)
    _assert_onehot_exact(c.shape, t["dist"], boxes, boxes64, False)
    exp = H.V10_EXPECT[c.pattern]
    stats = [H.v10_stage_stats(c, b) for b in range(H.B)]
    print(H.v10_id(c), stats)
    if not exp.get("sat"):
        assert torch.equal(idx, idx64) and torch.equal(det[..., 5], det64[..., 5]) and torch.equal(det[..., :4], det64[..., :4])
    else:
        assert not torch.equal(idx, idx64), "1.0f ties are what the case is about: in fp64 they are no ties"
        assert float(det[..., 4].min()) == 1.0
    images = (0,) if c.pattern == "equal_vs_random" else range(H.B)
    for b in images:
        s = stats[b]
        assert s["filter"] == exp["filter"], s
        for key in ("tie1", "tie2"):
            if exp.get(key) and (key == "tie1" or c.nc > 1):
                assert s[key], (key, s)
        if exp.get("multi"):
            assert s["multi"] >= 3, "one anchor contributes several classes"
    ncand = max(s["ncand"] for s in stats)
    assert c.rounds in (1, 2)
    if c.rounds == 2:
        assert ncand >= H.CAP + 1, "a second stage-2 round needs more candidates than a round holds"
    else:
        assert ncand <= H.CAP
    if c.pattern == "all_equal" and c.shape == "S":
        rows = torch.arange(k) // c.nc                          # stage-1 ranks are the anchors themselves: rows are ranks 0..3 (nc 80)
        assert torch.equal(idx, rows.expand(H.B, k)) and torch.equal(det[..., 5], (torch.arange(k) % c.nc).float().expand(H.B, k))
        assert c.nc != 80 or int(idx.max()) == 3
    if c.pattern == "thr_zero":
        assert stats[0]["thr"] == float(torch.tensor(-80.0).sigmoid()) > 1e-37, "the smallest normal score the rules allow"
    if c.pattern == "equal_vs_random":
        assert stats[1]["ncand"] <= H.CAP < stats[0]["ncand"]


def _kept(c, b, **kw):
    return H.nms_reference(c, **kw)[0][b][1].tolist()


def _iou32(box_a, box_b, cls):
    """the reference's float32 IoU of two class-offset boxes"""
    a, b = box_a + cls * 7680.0, box_b + cls * 7680.0
    iw = (torch.minimum(a[2], b[2]) - torch.maximum(a[0], b[0])).clamp(min=0)
    ih = (torch.minimum(a[3], b[3]) - torch.maximum(a[1], b[1])).clamp(min=0)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


@pytest.mark.parametrize("c", H.NMS_CASES, ids=H.nms_id)
def test_nms_case(c):
    t = H.nms_inputs(c)
    info = t["info"]
    A = H.n_anchors(c.shape)
    _assert_logit_rules(t["cls"])
    rows, boxes, scores = H.nms_reference(c, "fp32")
    rows64, boxes64, _ = H.nms_reference(c, "fp64")
    m, cls = scores.max(2)
    ncand = [int((m[b] > c.conf).sum()) for b in range(H.B)]
    nkept = [r[0].shape[0] for r in rows]
    print(H.nms_id(c), "candidates", ncand, "kept", nkept)
    saturated = bool((t["cls"] >= 20).any())
    if c.name != "random_boxes":
        _assert_onehot_exact(c.shape, t["dist"], boxes, boxes64, True)
        if not saturated:
            for b in range(H.B):
                assert torch.equal(rows[b][1], rows64[b][1]) and torch.equal(rows[b][0][:, 5], rows64[b][0][:, 5])
                assert torch.equal(rows[b][0][:, :4], rows64[b][0][:, :4])
    for b in range(H.B):
        assert torch.equal(rows[b][2], t["cf"][b][rows[b][1]])
    unlimited = [len(_kept(c._replace(max_det=10 ** 6), b)) for b in range(H.B)]
    n = c.name
    if n == "none_and_many":
        assert ncand == [0, 350] and nkept == [0, 300] and 301 <= unlimited[1] <= 400
    elif n == "many_k480":
        assert nkept[0] == 480 < unlimited[0] and 0 < nkept[1] < 300
    elif n == "n1_n32":
        assert ncand == [1, 32] and nkept == [1, 32]
    elif n == "n33_conf_edge":
        assert ncand[0] == 33 and nkept[0] == 33
        assert int((m[1] == c.conf).sum()) == 10 == len(info["edge"]) and not set(info["edge"]) & set(_kept(c, 1))
        assert ncand[1] == 15 == nkept[1]
    elif n == "conf_zero":
        assert ncand == [A, A] and nkept == [300, 300] and all(300 < u <= A - 20 for u in unlimited)
    elif n == "same_box":
        p, q = info["pair"]
        for b in range(H.B):
            assert torch.equal(boxes[b, p], boxes[b, q])
        assert {p, q} <= set(_kept(c, 0)) and cls[0, p] != cls[0, q]
        assert p in _kept(c, 1) and q not in _kept(c, 1) and cls[1, p] == cls[1, q]
    elif n == "iou_exact":
        thr32 = torch.tensor(c.iou, dtype=torch.float32)
        below = float(torch.nextafter(thr32, torch.tensor(0.0)))        # ovr > below  <=>  ovr >= iou in float32
        for b in range(H.B):
            p, q, r, s = info["pairs"][b]
            assert _iou32(boxes[b, p], boxes[b, q], cls[b, p].float()) == thr32, "ovr == iou exactly in the reference's arithmetic"
            assert _iou32(boxes[b, r], boxes[b, s], cls[b, r].float()) > thr32
            kept = set(_kept(c, b))
            assert {p, q, r} <= kept and s not in kept
            flipped = set(_kept(c, b, iou=below))
            assert flipped == kept - {q}, "`>=` instead of `>` drops exactly the box at the threshold"
    elif n == "chain":
        for b in range(H.B):
            pa, pb, pc = info["trip"][b]
            f = lambda i, j: float(_iou32(boxes[b, i], boxes[b, j], torch.tensor(17.0)))
            assert f(pa, pb) > c.iou and f(pb, pc) > c.iou and f(pa, pc) <= c.iou
            kept = set(_kept(c, b))
            assert pa in kept and pb not in kept and pc in kept, "B is dead when it is visited: C stays"
    elif n == "equal_scores":
        kept = set(_kept(c, 0))
        for lo, hi in info["pairs0"]:
            assert m[0, lo] == m[0, hi] and lo < hi and lo in kept and hi not in kept
        (lo0, hi1), (lo0b, hi1b) = info["cross"]
        kept = set(_kept(c, 1))
        assert lo0 < H.levels(c.shape)[0][0] * H.levels(c.shape)[0][1] <= hi1, "the pair crosses levels"
        assert m[1, lo0] == m[1, hi1] and lo0 in kept and hi1 not in kept
        assert m[1, hi1b] > m[1, lo0b] and hi1b in kept and lo0b not in kept
    elif n == "argmax":
        want = [5, 5, 5, 9, 5] * H.B
        for i, (b, a0) in enumerate(info["anchors"]):
            assert int(cls[b, a0]) == want[i], (i, int(cls[b, a0]))
            kept = set(_kept(c, b))
            assert a0 in kept and ((a0 + 1) in kept) == (want[i] != 5)
        b, a0 = info["anchors"][1]
        assert t["cls"][b, a0, 5] == 20.0 and t["cls"][b, a0, 9] == 30.0 and scores[b, a0, 5] == scores[b, a0, 9] == 1.0
    elif n == "blocks":
        np2, ncache = H.ncache_of(A)
        assert (np2, ncache) == {"M": (8192, 3276), "L": (H.NCAP, 0)}[c.shape]
        for b in range(H.B):
            order = info["order"][b]
            assert torch.equal(H.sorted_candidates(c, b), order) and ncand[b] == A
            pos = torch.empty(A, dtype=torch.long)
            pos[order] = torch.arange(A)
            kept = torch.tensor(_kept(c, b))
            kpos = pos[kept]
            assert bool((kpos == 31).any()) and bool((kpos == 32).any()), "survivors at bit 31 of a word and bit 0 of the next"
            assert torch.equal(torch.sort(info["block_of"][kept]).values, torch.arange(int(info["block_of"].max()) + 1)), "one per block"
            assert int((kpos >= max(ncache, A - 4 * 64 - 16)).sum()) == 4, "the late blocks' survivors"
            # victims of a survivor: the rest of its block. Pairs with both boxes in the cache, one on each side, both beyond:
            first = torch.full((int(info["block_of"].max()) + 1,), A, dtype=torch.long).scatter_reduce(0, info["block_of"], pos, "amin")
            kp = first[info["block_of"]]                        # sorted position of each anchor's suppressor
            victim = pos > kp
            if ncache:
                assert bool((victim & (kp < ncache) & (pos < ncache)).any()) and bool((victim & (kp < ncache) & (pos >= ncache)).any())
            assert bool((victim & (kp >= ncache) & (pos >= ncache)).any())
    elif n == "random_boxes":
        for b in range(H.B):
            (d32, i32, _), (d64, i64, _) = rows[b], rows64[b]
            assert 5 <= nkept[b] < ncand[b], "the case must make NMS work"
            same = (i64 == i32) & (d64[:, 5] == d32[:, 5]) if d64.shape[0] == d32.shape[0] else torch.zeros(nkept[b], dtype=torch.bool)
            assert float(same.float().mean()) > 0.5
    elif n == "large_gather":
        assert A > 12288
        for b in range(H.B):
            kept = set(_kept(c, b))
            assert int((m[b] == c.conf).sum()) == 40 and not set(info[f"edge{b}"]) & kept
            p, q = info[f"pair{b}"]
            assert p in kept and q not in kept
            assert any(a > 12288 for a in kept), "rows from beyond the first 12288 anchors"
    else:
        raise KeyError(n)
    assert nkept[0] != nkept[1] or not torch.equal(rows[0][1], rows[1][1]), "the two images differ"


def test_case_ids_are_unique():
    assert len({H.v10_id(c) for c in H.V10_CASES}) == len(H.V10_CASES) and len({H.nms_id(c) for c in H.NMS_CASES}) == len(H.NMS_CASES)
