"""EfficientNet-B3 needle classifier on the MI355X (yp_cls_*): fp32 parity with the fp64 / fp32 restatement (tests/effnet_ref.py) on
logits and taps, bf16 per-op parity (teacher-forced), ROI equivalence, batch / graph invariance and the reference's entry points."""
import numpy as np
import pytest
import torch

import effnet_ref as R
from helpers import assert_within_noise_floor
from yolo_puncture_amd import classify as C

pytestmark = pytest.mark.gpu

ST = C.synthetic_state(0)


def _frames(B, seed, h=720, w=1280):
    rng = np.random.RandomState(seed)
    fr = rng.randint(0, 256, (B, h, w, 3), dtype=np.uint8)
    # smooth structure on top of the noise so that the crops differ in more than noise
    yy, xx = np.mgrid[0:h, 0:w]
    for b in range(B):
        blob = (np.sin(xx / (37 + 11 * b)) * np.cos(yy / (23 + 5 * b)) * 100).astype(np.int16)
        fr[b] = np.clip(fr[b].astype(np.int16) // 2 + 64 + blob[..., None], 0, 255).astype(np.uint8)
    boxes = [(600, 300, 700, 420), (0, 0, 40, 30), (1240, 690, 1280, 720), (0, 0, w, h), (101, 250, 330, 611), (1100, 10, 1279, 200),
             (300, 700, 500, 720)]
    return fr, [boxes[(b + seed) % len(boxes)] for b in range(B)]


def _ref_input(frames_bgr, boxes):
    crops = np.stack([R.crop(f[..., ::-1], bx) for f, bx in zip(frames_bgr, boxes)])
    return R.normalise(crops)


def _run(eng, frames, boxes, bgr=True):
    logits, prob, cls = eng.forward(torch.from_numpy(frames).cuda(), torch.tensor(boxes, dtype=torch.int32).cuda(), bgr=bgr)
    torch.cuda.synchronize()
    return logits.cpu(), prob.cpu(), cls.cpu()


@pytest.fixture(scope="module")
def eng32():
    e = C.ClassifierEngine("fp32", 0, state=ST)
    yield e
    e.close()


@pytest.mark.parametrize("B", [1, 4, 7])
def test_fp32_logits_and_taps(eng32, B):
    frames, boxes = _frames(B, B)
    logits, prob, cls = _run(eng32, frames, boxes)
    x = _ref_input(frames, boxes)
    t32, t64 = {}, {}
    o32 = R.forward(ST, x, "fp32", tap=lambda n, t: t32.__setitem__(n, t))
    o64 = R.forward(ST, x, "fp64", tap=lambda n, t: t64.__setitem__(n, t))
    assert_within_noise_floor(f"classifier logits B={B}", logits, o32, o64, 1e-3)
    p64 = torch.softmax(o64, 1)
    margin = (o64[:, 1] - o64[:, 0]).abs()
    sure = margin > 1e-4
    assert sure.any()
    assert torch.equal(cls.long()[sure], p64.argmax(1)[sure])
    torch.testing.assert_close(prob.double(), p64.max(1).values, rtol=0, atol=1e-5)
    last = {}
    for i, b in enumerate(C.block_specs()):
        last[b["stage"]] = i
    for name in ["stem", "_blocks.18"] + [f"_blocks.{i}" for i in sorted(last.values())] + ["head.pool"]:
        got = eng32.read_tensor(name)
        # a tap after n blocks carries n blocks of the engine's own fp32 rounding against n of the oracle's: two independent noise
        # samples that compound, so the taps get factor 4 (the logits above keep the default 2)
        assert_within_noise_floor(f"tap {name} B={B}", got, t32[name].permute(0, 2, 3, 1), t64[name].permute(0, 2, 3, 1), 1e-3, factor=4.0)


def test_roi_equivalence_and_input(monkeypatch):
    monkeypatch.setenv("YOLOP_CLS_TAP_INPUT", "1")
    e = C.ClassifierEngine("fp32", 0, state=ST)
    frames, boxes = _frames(3, 11)
    _run(e, frames, boxes)
    x = _ref_input(frames, boxes)
    assert torch.equal(e.read_tensor("input"), x.permute(0, 2, 3, 1))             # crop + pad + /255 + normalise, bit-exact
    l_full, _, _ = _run(e, frames, boxes)
    crops = np.ascontiguousarray(np.stack([R.crop(f, bx) for f, bx in zip(frames, boxes)]))
    l_crop, _, _ = _run(e, crops, [(0, 0, 380, 380)] * 3)
    assert torch.equal(l_full, l_crop)
    e.close()


def test_batch_and_graph_invariance(eng32):
    frames, boxes = _frames(8, 3)
    l8, p8, c8 = _run(eng32, frames, boxes)
    for b in range(8):
        l1, _, _ = _run(eng32, frames[b:b + 1], boxes[b:b + 1])
        assert torch.equal(l1[0], l8[b])
    e = C.ClassifierEngine("bf16", 0, state=ST)
    for eng in (eng32, e):
        fr, bx = torch.from_numpy(frames).cuda(), torch.tensor(boxes, dtype=torch.int32).cuda()
        eager = [t.clone() for t in eng.forward(fr, bx)]
        eng.set_graph(True)
        for _ in range(3):                   # capture, then replays
            got = eng.forward(fr, bx)
            torch.cuda.synchronize()
            for a, g in zip(eager, got):
                assert torch.equal(a, g)
        eng.set_graph(False)
    e.close()


def _ulp_ok(got, ref):
    """|got - ref| <= 1 bf16 ulp of ref, on >= 98 % of the elements."""
    ulp = torch.where(ref == 0, torch.full_like(ref, 2.0 ** -133), 2.0 ** (torch.floor(torch.log2(ref.abs())) - 7))
    return ((got - ref).abs() <= ulp + 1e-30).float().mean().item()


def test_bf16_ops_teacher_forced():
    e = C.ClassifierEngine("bf16", 0, state=ST)
    frames, boxes = _frames(2, 5)
    _run(e, frames, boxes)
    nchw = lambda n: e.read_tensor(n).permute(0, 3, 1, 2)
    pads = R.pads()
    fold = lambda c, b: R.fold(ST, c, b)
    worst = 1.0
    cur = nchw("stem")
    x = _ref_input(frames, boxes)
    frac = _ulp_ok(nchw("stem"), R.bf_conv(x, *fold("_conv_stem", "_bn0"), 2, pads["_conv_stem"]))
    worst = min(worst, frac)
    for i, b in enumerate(C.block_specs()):
        p = f"_blocks.{i}"
        h = cur
        if b["expand"]:
            got = nchw(f"{p}.expand")
            worst = min(worst, _ulp_ok(got, R.bf_conv(h, *fold(f"{p}._expand_conv", f"{p}._bn0"))))
            h = got
        dw = nchw(f"{p}.dw")
        worst = min(worst, _ulp_ok(dw, R.bf_conv(h, *fold(f"{p}._depthwise_conv", f"{p}._bn1"), b["s"], pads[f"{p}._depthwise_conv"], groups=h.shape[1])))
        g = R.se_gate(ST, p, dw)
        torch.testing.assert_close(nchw(f"{p}.gate"), g, rtol=1e-5, atol=1e-6)
        out = nchw(p)
        ref = R.bf_conv(R.bfr(dw * g), *fold(f"{p}._project_conv", f"{p}._bn2"), act=False, res=cur if b["residual"] else None)
        frac = _ulp_ok(out, ref)
        print(f"{p}: {frac:.4f} within 1 bf16 ulp")
        worst = min(worst, frac)
        cur = out
    assert worst >= 0.98, worst
    pooled = R.bf_conv(cur, *fold("_conv_head", "_bn1"), rnd=False).mean((2, 3))
    torch.testing.assert_close(e.read_tensor("head.pool")[:, 0, 0], pooled, rtol=1e-4, atol=1e-5)
    e.close()


def test_video_entry_points(eng32):
    frames, boxes = _frames(60, 9, 360, 640)
    boxes = [tuple(min(v, lim) for v, lim in zip(bx, (640, 360, 640, 360))) for bx in boxes]
    res = [C.predict_and_find_start_inserted(eng32, list(frames), boxes, judge_wnd=20, batch_size=bs) for bs in (1, 4, 8, 32)]
    for r in res[1:]:
        assert r[2] == res[0][2] and [int(c) for c in r[0]] == [int(c) for c in res[0][0]] and np.array_equal(r[1], res[0][1])
    _, prob, cls = _run(eng32, frames, boxes)
    cl, pl = [int(c) for c in cls], list(prob.numpy())
    idx = R.find_start(cl, pl, 20)
    cl, pl = R.repair(cl, pl, idx)
    assert res[0][2] == idx and [int(c) for c in res[0][0]] == cl and np.array_equal(np.array(res[0][1]), np.array(pl))
    # predict_images: RGB, 380^2 passes through, other sizes go through the same PIL bilinear resize as torchvision's Resize
    from PIL import Image
    rng = np.random.RandomState(2)
    ims = [rng.randint(0, 256, (380, 380, 3), dtype=np.uint8), rng.randint(0, 256, (240, 320, 3), dtype=np.uint8)]
    idxs, probs = C.predict_images(eng32, ims)
    ref_in = np.stack([ims[0], np.asarray(Image.fromarray(ims[1]).resize((380, 380), Image.BILINEAR))])
    o64 = R.forward(ST, R.normalise(ref_in), "fp64")
    p64 = torch.softmax(o64, 1)
    assert [int(i) for i in idxs] == p64.argmax(1).tolist()
    np.testing.assert_allclose(np.array(probs, dtype=np.float64), p64.max(1).values.numpy(), atol=1e-5)
