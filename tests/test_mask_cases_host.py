"""CPU proofs about tests/mask_cases.py, for every case tests/test_gpu_mask_crafted.py runs: the exact cases are exact (float32 and float64 give
the same logits, bit for bit), every size has the crop rectangle it claims, the cases named after a property have it (no case is vacuous), the
area cases keep their distance from the threshold, and the random cases' inputs keep the exemption cap - so a failure on the GPU is the kernel's."""
import math

import pytest
import torch

import mask_cases as K
from oracle import postprocess_oracle as po


def _maps(proto_hwc, coeff, boxes, hw, retina):
    chw = proto_hwc.permute(2, 0, 1).contiguous()
    m32 = K.logit_map(chw, coeff, boxes, hw, retina)
    m64 = K.logit_map(chw.double(), coeff.double(), boxes.double(), hw, retina)
    return m32, m64


def test_crafted_prototypes():
    for rig in K.RIGS:
        p = K.int_protos(rig)
        assert tuple(p.shape) == K.proto_shape(rig) + (32,)
        assert torch.equal(p, p.round()) and float(p.abs().max()) <= 4 and float(p[..., 31].min()) >= 1
        assert torch.equal(K.to_storage(p, "bf16"), p), "integers up to 4 are bf16 numbers"
        for b in range(1, p.shape[0]):
            assert float((p[b] != p[0]).float().mean()) > 0.5, "images differ: a wrong image stride shows"
        assert torch.equal(K.to_storage(K.rect_protos(rig), "bf16"), K.rect_protos(rig))


@pytest.mark.parametrize("hw", list(K.RETINA_SIZES), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_retina_size_has_the_crop_it_claims(hw):
    (t, b, l, r), (num, den), rem = K.RETINA_SIZES[hw]
    assert po.scale_masks_region(24, 40, hw[0], hw[1]) == (t, b, l, r)
    assert ((b - t) * (r - l)) % 16 == rem
    # the map from output to crop pixels is the dyadic scale named, on both axes: every interpolation weight is a multiple of 1/16
    assert (b - t) * num == hw[0] * den and (r - l) * num == hw[1] * den
    assert num in (1, 2, 4, 8) and den in (1, 2)
    sizes = K.RETINA_SIZES
    assert {sizes[s][2] for s in K.COUNT_SIZES} == {0, 8} and any(sizes[s][1] == (1, 1) for s in K.COUNT_SIZES)
    if hw in ((23, 40), (24, 39)):
        assert (hw[0] * hw[1]) % 16 != 0, "a 16-byte line of the clip writers straddles two masks"


def test_exact_case_list_is_complete():
    cs = K.EXACT_CASES
    assert len(set(cs)) == len(cs)
    assert {c.hw for c in cs if c.retina} == set(K.RETINA_SIZES)
    for hw in K.COUNT_SIZES:
        assert {c.n for c in cs if c.retina and c.hw == hw} == set(K.COUNTS)
    assert {c.n for c in cs if not c.retina and c.hw == (96, 160)} == set(K.COUNTS)
    assert any(not c.retina and c.hw == (64, 96) for c in cs)
    assert {c.b for c in cs if c.rig == "A"} == {0, 1}
    for c in cs:
        assert c.hw == K.RIGS[c.rig][1:] or c.retina
    assert K.BIG_CASE.n == K.YP_MAX_MASKS and (K.YP_MAX_MASKS + 15) // 16 * 16 * 32 * 4 == 60 * 1024      # launch_masks' LDS bound, met exactly


@pytest.mark.parametrize("c", K.EXACT_CASES + [K.BIG_CASE], ids=K.exact_id)
def test_exact_case(c):
    coeff, boxes = K.exact_inputs(c)
    ref = K.exact_reference(c)
    assert ref.dtype == torch.uint8 and tuple(ref.shape) == (c.n,) + c.hw
    if c.n == 0:
        return
    assert torch.equal(coeff, coeff.round()) and float(coeff.abs().max()) <= 3 and bool(torch.isfinite(boxes).all())
    m32, m64 = _maps(K.int_protos(c.rig)[c.b], coeff, boxes, c.hw, c.retina)
    assert torch.equal(m32.double(), m64), "float32 and float64 disagree: the case is not exact"
    assert torch.equal((m64 > 0).to(torch.uint8), ref), "logit_map is not the oracle function"
    assert torch.equal(m64 * 256, (m64 * 256).round()), "every logit is a multiple of 1/256 or coarser"
    plan = K.row_plan(c)
    inbox = K.inside_box(boxes, c.hw)
    zeros = 0
    for i, (ck, bk) in enumerate(plan):
        if bk in ("empty", "inverted"):
            assert int(ref[i].sum()) == 0 and (not c.retina or int(inbox[i].sum()) == 0)
        if ck == "minus":
            assert int(ref[i].sum()) == 0 and float(m64[i].max()) < 0
        if ck == "plus" and c.retina:
            assert torch.equal(ref[i].bool(), inbox[i]), "an all-positive row's mask is its box"
        if ck == "plus" and c.retina and bk == "half":
            x1, y1, x2, y2 = boxes[i].tolist()
            cols, rows = torch.nonzero(ref[i].any(0)).flatten(), torch.nonzero(ref[i].any(1)).flatten()
            assert (int(cols[0]), int(cols[-1]), int(rows[0]), int(rows[-1])) == (math.ceil(x1), math.ceil(x2) - 1, math.ceil(y1), math.ceil(y2) - 1)
            assert x1 != int(x1) and int(cols[0]) == int(x1) + 1
        if bk == "one_pixel" and ck == "plus" and c.retina:
            assert int(ref[i].sum()) == 1
        if ck == "sparse" and bk == "whole":
            zeros += int(((m64[i] == 0) & inbox[i]).sum())
        if ck == "neg":
            a, b = ref[i - 1].bool(), ref[i].bool()
            assert torch.equal(boxes[i], boxes[i - 1]) and not bool((a & b).any())
            z = (m64[i] == 0) & inbox[i]
            assert bool(z.any()) and not bool(((a | b) & z).any()), "at an exact zero both rows are 0"
            assert torch.equal(a | b, inbox[i] & (m64[i] != 0)), "where one has +v the other has -v"
        if not c.retina and ck == "plus" and bk in K.box_kinds_input(*c.hw):
            outside = ref[i].bool() & ~inbox[i]
            assert bool(outside.any()), f"{bk}: a pixel outside the box takes an inside tap and is set"
    print(f"{K.exact_id(c)}: {zeros} exact-zero logits inside the whole-image boxes of the sparse rows")
    assert zeros > 0, "the strict > 0 must be met on values that are 0"
    if c.n >= 15:
        kinds = {bk for _, bk in plan}
        assert set(K.box_kinds(*c.hw)) <= kinds and {ck for ck, _ in plan} == {"dense", "sparse", "neg", "minus", "plus"}
        if not c.retina and c.n >= 17:
            assert set(K.box_kinds_input(*c.hw)) <= kinds
            assert any(ck == "plus" and bk in ("between_q", "between_h") for ck, bk in plan) or c.n < 33
        assert len({tuple(r) for r in torch.cat([coeff, boxes], 1).tolist()}) >= min(c.n, 17) - 1, "rows differ"


def test_exact_input_boxes_scale_exactly():
    """retina=0: box coordinates x 1/4 are exact in float32, and the proto_exact kind lands on prototype pixels"""
    for hw in ((96, 160), (64, 96)):
        for name, box in {**K.box_kinds(*hw), **K.box_kinds_input(*hw)}.items():
            b = torch.tensor(box, dtype=torch.float32)
            assert torch.equal((b * 0.25).double(), b.double() / 4), name
        b = torch.tensor(K.box_kinds_input(*hw)["proto_exact"])
        assert torch.equal(b / 4, (b / 4).round())
        for name in ("between_q", "between_h"):
            b = torch.tensor(K.box_kinds_input(*hw)[name]) / 4
            assert not bool((b == b.round()).any()), name


@pytest.mark.parametrize("k", list(K.CLIP_FRAMES))
@pytest.mark.parametrize("hw,retina", K.CLIP_SIZES)
def test_clip_case(hw, retina, k):
    fidx, coeff, boxes = K.clip_inputs(hw, retina, k)
    B = K.RIGS[K.CLIP_RIG][0]
    assert len(fidx) == k and max(fidx) < B
    if k > 1:
        assert len(set(fidx)) < k, "a repeat"
        assert set(range(min(fidx), max(fidx) + 1)) - set(fidx), "a gap"
    ref = K.clip_reference(hw, retina, k)
    assert tuple(ref.shape) == (k,) + hw
    assert len({tuple(b) for b in boxes.tolist()}) == k, "neighbouring masks have different boxes"
    for j, f in enumerate(fidx):
        m32, m64 = _maps(K.int_protos(K.CLIP_RIG)[f], coeff[f, :1], boxes[j:j + 1], hw, retina)
        assert torch.equal(m32.double(), m64) and torch.equal((m64 > 0).to(torch.uint8)[0], ref[j])
        assert 0 < int(ref[j].sum()) < hw[0] * hw[1]
    if k > 1:      # the repeated frame gives different masks under different boxes
        assert not torch.equal(ref[0], ref[1]) or fidx[0] != fidx[1]
        rep = [j for j in range(1, k) if fidx[j] == fidx[j - 1]]
        assert rep and not torch.equal(ref[rep[0]], ref[rep[0] - 1])


@pytest.mark.parametrize("c", K.PAINT_CASES, ids=lambda c: c.name)
def test_paint_case(c):
    coeff, boxes = K.rect_inputs(c.rows)
    want = K.rect_masks(c.rows, K.PAINT_HW)
    for rig in ("A",):
        assert torch.equal(K.oracle_masks(K.rect_protos(rig)[0], coeff, boxes, K.PAINT_HW, True), want), "rect masks are their boxes"
    areas = [int(m.sum()) for m in want]
    for (sign, (x1, y1, x2, y2)), a in zip(c.rows, areas):
        assert a == ((x2 - x1) * (y2 - y1) if sign > 0 else 0)
    ids, kept = K.paint_reference(want, K.PAINT_HW, c.suppress, c.min_area)
    assert kept.tolist() == c.kept
    if c.name == "area_on_and_below_threshold":
        assert areas == [c.min_area, c.min_area - 1]
    if c.name == "overlap_later_wins_suppressed_between":
        assert int((ids == 1).sum()) > 0 and int((ids == 2).sum()) == areas[2] and int((ids == 1).sum()) < areas[0]
        assert bool((want[0].bool() & want[1].bool() & want[2].bool()).any()), "the suppressed row lies on the overlap of the two kept rows"
        assert set(ids.unique().tolist()) == {0, 1, 2}
    if c.name == "empty_mask_takes_an_id":
        assert set(ids.unique().tolist()) == {0, 1, 3}
    if c.name in ("all_suppressed", "none"):
        assert int(ids.abs().sum()) == 0


@pytest.mark.parametrize("c", K.RESIZE_CASES, ids=lambda c: c.name)
def test_resize_case(c):
    coeff, boxes = K.rect_inputs(c.rows)
    want = K.rect_masks(c.rows, c.mask_hw)
    assert torch.equal(K.oracle_masks(K.rect_protos("A")[0], coeff, boxes, c.mask_hw, True), want)
    areas = K.resized_areas(want, c.out_hw)
    print(c.name, areas, c.min_area)
    assert all(abs(a - c.min_area) >= 1.0 for a in areas), (areas, "min_area must keep 1.0 from every row's float area (the device sums in double)")
    assert any(a < c.min_area for a in areas) and any(a > c.min_area for a in areas)
    ids, kept = K.paint_reference(want, c.out_hw, 1, c.min_area)
    assert int((kept > 0).sum()) >= 2 and set(ids.unique().tolist()) == {0} | set(kept[kept > 0].tolist())
    ratio = max(c.mask_hw[0] / c.out_hw[0], c.mask_hw[1] / c.out_hw[1])
    assert ratio <= 16 and math.ceil(max(ratio, 1.0)) * 2 + 1 <= K.AA_KMAX
    if c.name == "down_16_1":
        assert c.mask_hw[0] / c.out_hw[0] == 16 and c.mask_hw[1] / c.out_hw[1] == 16 and math.ceil(ratio) * 2 + 1 == 33
    if c.name == "up_2_3":
        f = torch.nn.functional.interpolate(want[:1, None].float(), size=c.out_hw, mode="bilinear", align_corners=False, antialias=True)
        assert int((f == 0.5).sum()) > 50, "exact 0.5 ties on the edges: `> 0.5` leaves them out"


def test_axis_restates_torch():
    """the float32 source coordinates of mask_cases._axis against torch's bilinear interpolate itself: a ramp resized by torch equals the ramp
    blended with our indices and weights (float64 blend of float32 weights, rounded once)"""
    for n_src, n_dst in ((23, 90), (40, 160), (24, 200), (40, 333), (40, 161), (24, 96), (16, 64)):
        i0, i1, l0, l1 = K._axis(n_dst, n_src)
        ramp = torch.arange(n_src, dtype=torch.float32) ** 2
        got = torch.nn.functional.interpolate(ramp[None, None, None], size=(1, n_dst), mode="bilinear", align_corners=False)[0, 0, 0]
        want = torch.from_numpy(l0 * ramp.double().numpy()[i0] + l1 * ramp.double().numpy()[i1])
        assert float((got.double() - want).abs().max()) <= 2 * 2.0 ** -24 * float(ramp.max()), (n_src, n_dst)


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("c", K.RANDOM_CASES, ids=K.random_id)
def test_random_case_keeps_the_cap(c, dtype):
    ref, A, inbox = K.random_case_reference(c, dtype)
    assert tuple(ref.shape) == (c.n,) + c.hw
    exempt = K.rule_stats(ref, A)
    npix = int(inbox.sum())
    print(f"{K.random_id(c)} {dtype}: {int(exempt.sum())} exempt of {npix} in-box pixels; median allowance {float((K.GAMMA * K.U32 * A[inbox]).median()):.3e}")
    assert npix >= c.hw[0] * c.hw[1] // 8
    assert int(exempt.sum()) <= K.EXEMPT_CAP * npix, (int(exempt.sum()), npix)
    # the reference is the oracle function up to pixels near zero (it restates it; the oracle function is float32 throughout)
    coeff, boxes = K.random_inputs(c)
    orc = K.oracle_masks(K.to_storage(K.rand_protos(c.rig, c.seed), dtype)[c.b], coeff, boxes, c.hw, c.retina)
    K.check_rule(f"oracle function vs float64 reference, {K.random_id(c)} {dtype}", orc, ref, A)
    assert 0.2 < float((ref > 0)[inbox].float().mean()) < 0.8


def test_rule_refuses_a_one_column_shift():
    """what the share allowance of 2e-4 let through: one mask's box one column wider. Under the rule it fails."""
    c = [c for c in K.RANDOM_CASES if c.hw == (200, 333) and c.n == 7][0]
    ref, A, _ = K.random_case_reference(c, "fp32")
    coeff, boxes = K.random_inputs(c)
    wider = boxes.clone()
    wider[3, 2] += 1.0
    got = K.oracle_masks(K.rand_protos(c.rig, c.seed)[c.b], coeff, wider, c.hw, True)
    assert float((got != (ref > 0)).float().mean()) < 2e-4
    with pytest.raises(AssertionError, match="outside the allowance"):
        K.check_rule("shifted", got, ref, A)


def test_valu_subset():
    assert {(c.retina, c.n) for c in K.VALU_EXACT} == {(True, 1), (True, 17), (False, 1), (False, 17)}
    assert {K.RETINA_SIZES[c.hw][2] for c in K.VALU_EXACT if c.retina} == {0, 8}
