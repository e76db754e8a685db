"""Inputs beyond 12288 anchors, host side (no GPU): the plan takes the heads' large forms from 12289 anchors on and the LDS forms up to
12288, reports kernel symbols libyolop.so contains, and refuses - in yp_plan, naming the quantity and the largest value that fits - what
no kernel holds: more than YP_MAX_ANCHORS anchors, more attention tokens than the generic attention kernel keeps in LDS, an activation
of 2^31 bytes."""
import pytest

from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import MAX_ANCHORS, Engine, YolopError, load_library


def _anchors(H, W):
    return sum((H // s) * (W // s) for s in (8, 16, 32))


def _head(e, B, H, W):
    ops = e.plan(B, H, W)
    assert ops[-1]["kind"] == "head"
    return ops[-1]["kernel"]


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
@pytest.mark.parametrize("family,seg", [("v10", False), ("v8", True), ("11", True)])
def test_large_form_from_12289_anchors(family, seg):
    assert _anchors(800, 768) == 12600 and _anchors(768, 768) == 12096
    syms = _kernel_symbols(load_library()._name)
    e = Engine("n", 80, seg, "bf16", 0, family=family)
    large = _head(e, 1, 800, 768)
    small = _head(e, 1, 768, 768)
    e.close()
    parts = [k.strip().replace(" ", "") for k in large.split("+")]
    mine = [k for k in parts if "large" in k or "chunk" in k or "gather" in k]      # (the branch kernels behind them are template families)
    assert len(mine) == 2
    for k in mine:
        assert k in syms, (large, k)
    if family == "v10":
        assert "head_chunk_topk_kernel" in parts and "head_select_large_kernel<1>" in parts and "head_select_kernel<1>" not in parts
        assert small.startswith("head_select_kernel") and "large" not in small and "chunk" not in small
    else:
        assert parts == ["head_nms_gather_kernel", "head_nms_large_kernel"]
        assert small == "head_nms_kernel"


def test_dense_v10_head_large_form(monkeypatch):
    monkeypatch.setenv("YOLOP_DENSE_HEAD", "1")
    e = Engine("n", 80, False, "bf16", 0)
    assert _head(e, 1, 800, 768) == "head_chunk_topk_kernel + head_select_large_kernel<0>"
    assert _head(e, 1, 768, 768) == "head_select_kernel"
    e.close()


def test_attention_tokens_are_refused_at_plan_time():
    # 2560 x 1472: 80 x 46 = 3680 tokens; the generic attention kernel keeps 16 x N scores + 16 x 32 keys in 150 KiB of LDS: N <= 2368
    for family, seg in (("v10", False), ("11", True)):
        e = Engine("n", 80, seg, "bf16", 0, family=family)
        with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368"):
            e.plan(1, 2560, 1472)
        assert len(e.plan(1, 1088, 1920)) > 0            # 2040 tokens
        e.close()
    e = Engine("n", 80, True, "bf16", 0, family="v8")      # no attention in v8
    assert _head(e, 1, 2560, 1472) == "head_nms_gather_kernel + head_nms_large_kernel"
    e.close()


def test_max_batch_is_the_analytic_bound_and_one_more_is_refused():
    e = Engine("n", 80, True, "bf16", 0, family="v8")
    e.plan(1, 640, 640)
    shapes = [(320, 320), (384, 640), (640, 640), (736, 1280), (1280, 1280), (2176, 3840)]
    got = []
    for H, W in shapes:
        # bytes of the largest tensor of one image, from the engine's own tensor list (planned at B = 1)
        e.plan(1, H, W)
        per = max(t["shape"][1] * t["shape"][2] * t["shape"][3] * (4 if t["f32"] else 2) for t in e.tensors())
        mb = e.max_batch(H, W)
        assert mb == min((2 ** 31 - 1) // per, 1 << 20), (H, W, per, mb)
        assert mb * per < 2 ** 31 <= (mb + 1) * per or mb == 1 << 20
        got.append(mb)
    assert all(a >= b for a, b in zip(got, got[1:])), got     # monotone in H * W
    H, W = 1280, 1280
    mb = e.max_batch(H, W)
    assert len(e.plan(mb, H, W)) > 0
    with pytest.raises(YolopError, match=rf"2\^31 bytes.*largest batch that fits is {mb}\b"):
        e.plan(mb + 1, H, W)
    # a refused plan leaves the previous one in place
    assert e.lib.yp_debug_host_selftest(e._h) > 0
    with pytest.raises(YolopError):
        e.max_batch(100, 640)
    e.close()


def test_one_past_max_anchors_is_refused():
    # a 4K frame letterboxed to 2176 x 3840 has 171360 anchors; the bound also covers the 214200 the selection test drives
    assert MAX_ANCHORS == 12288 * (12288 // 512) and _anchors(2176, 3840) == 171360 and 214200 <= MAX_ANCHORS
    e = Engine("n", 80, True, "bf16", 0, family="v8")
    # 3744 x 3840 (294840 anchors) is the last shape of that width below the bound; one more row of 32 pixels passes it
    assert len(e.plan(1, 2176, 3840)) > 0
    assert _anchors(3744, 3840) <= MAX_ANCHORS < _anchors(3776, 3840)
    assert len(e.plan(1, 3744, 3840)) > 0
    with pytest.raises(YolopError, match=rf"{_anchors(3776, 3840)} anchors.*at most {MAX_ANCHORS}"):
        e.plan(1, 3776, 3840)
    e.close()
