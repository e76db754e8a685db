"""YOLOv8-seg / YOLO11-seg engines on inputs beyond 12288 anchors: the candidates above conf are gathered over the whole chip into a
per-image key list (head_nms_gather_kernel); head_nms_large_kernel sorts and sweeps them as head_nms_kernel does, after cutting the list to
its 16384 largest keys when it is longer (an exact threshold select). The reference is oracle/yolo_seg_oracle.py's post-process applied to
the ENGINE's own head tensors, so the comparison is of the post-process alone and holds for a bf16 engine.

ultralytics cuts at max_nms = 30000 candidates by score, this engine at 16384. The two can differ only when fewer than max_det boxes survive
among the first 16384, i.e. when NMS would have reached candidate 16385: no case here (nor any real frame at conf >= 0.001) gets there, and
a test cannot tell the caps apart otherwise - the conf = 0 case therefore truncates the host list the same way and checks that the cut is
exact (the 16384 largest keys, ties by anchor index)."""
import pytest
import torch

from helpers import assert_within_noise_floor, make_case_family
from oracle.yolo_seg_oracle import SegOracle, nms_postprocess

pytestmark = pytest.mark.gpu
NCAP = 16384


def _host_rows(st, family, mode, eng, shape, conf, b):
    """the oracle's decode + NMS on the engine's head tensors of image b -> det [n, 6], anchor idx [n], coeff [n, 32], candidates"""
    hi = 22 if family == "v8" else 23
    B = shape[0]
    dt = torch.float64 if mode == "fp64" else torch.float32
    cat = lambda pre, C: torch.cat([eng.read_tensor(eng.find_tensor(f"model.{hi}.{pre}.{l}.2")).reshape(B, -1, C) for l in range(3)], 1).permute(0, 2, 1)
    bl, cl, cf = cat("cv2", 64), cat("cv3", 80), cat("cv4", 32)
    o = SegOracle(st, family, "n", 80, mode)
    shapes = [(shape[1] // s, shape[2] // s) for s in (8, 16, 32)]
    boxes, scores = o.decode(bl.to(dt).contiguous(), cl.to(dt).contiguous(), shapes)
    cxy, wh = (boxes[..., :2] + boxes[..., 2:]) / 2, boxes[..., 2:] - boxes[..., :2]
    boxes = torch.cat((cxy - wh / 2, cxy + wh / 2), -1)
    sc = scores[b].float().clone()
    m = sc.max(1).values
    ncand = int((m > conf).sum())
    if ncand > NCAP:      # the engine's cut: the NCAP largest keys score_bits << 32 | (0xFFFFFFFF - anchor) take part
        A = m.shape[0]
        keys = (m.view(torch.int32).long() << 32) | (0xFFFFFFFF - torch.arange(A, dtype=torch.int64))
        keys[~(m > conf)] = -1
        out = torch.sort(keys, descending=True).indices[NCAP:]
        sc[out] = 0.0
    det, idx, c = nms_postprocess(boxes[b].float(), sc, cf[b].permute(1, 0).float(), conf, 0.7)
    return det, idx, c, ncand


@pytest.mark.parametrize("family", ["v8", "11"])
@pytest.mark.parametrize("shape,confs", [((1, 800, 768), (0.25, 0.001)), ((1, 1024, 800), (0.0,))])
def test_large_nms_rows_match_host_postprocess(family, shape, confs):
    from yolo_puncture_amd.engine import Engine
    st, im = make_case_family(family, "n", 80, 0, shape)
    eng = Engine("n", 80, True, "bf16", 0, state=st, family=family)
    eng.set_autotune(False)
    assert eng.plan(*shape)[-1]["kernel"] == "head_nms_gather_kernel + head_nms_large_kernel"
    A = sum((shape[1] // s) * (shape[2] // s) for s in (8, 16, 32))
    imc = im.cuda()
    for conf in confs:
        eng.set_nms(conf, 0.7)
        out = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
        torch.cuda.synchronize()
        det, idx, cf = out["det"].cpu()[0], out["idx"].cpu()[0].long(), out["coeff"].cpu()[0]
        want, widx, wcf, ncand = _host_rows(st, family, "fp32", eng, shape, conf, 0)
        w64, i64, _, _ = _host_rows(st, family, "fp64", eng, shape, conf, 0)
        n = want.shape[0]
        print(f"{family} {shape} conf {conf}: {ncand} candidates of {A} anchors, {n} rows kept")
        if conf == 0.0:
            assert ncand == A > NCAP, "every anchor must be a candidate: the case is about the cut to NCAP"
        if conf <= 0.001:
            assert ncand > 12288, "more candidates than the LDS gather of head_nms_kernel could hold"
        assert n >= 5 and n < ncand, "the case must make NMS work"
        got_n = int((idx >= 0).sum())
        assert got_n == n, (got_n, n)
        assert bool((idx[n:] == -1).all()) and (n == det.shape[0] or float(det[n:].abs().max()) == 0.0)
        assert torch.equal(idx[:n], widx) and torch.equal(det[:n, 5], want[:, 5])
        assert torch.equal(cf[:n], wcf)                       # (rows of the engine's own coefficient maps)
        same = (i64 == widx) & (w64[:, 5].float() == want[:, 5]) if w64.shape[0] == n else torch.zeros(n, dtype=torch.bool)
        assert same.float().mean() > 0.5
        assert_within_noise_floor(f"{family} conf {conf} NMS rows: boxes [px]", det[:n, :4][same], want[:, :4][same], w64[:, :4][same], 1e-3)
        assert_within_noise_floor(f"{family} conf {conf} NMS rows: scores", det[:n, 4][same], want[:, 4][same], w64[:, 4][same], 1e-3, ceiling=1e-4)
        # graph replay == eager
        eng.set_graph(True)
        rep = eng.forward(imc)
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(rep[k], out[k]), k
        eng.set_graph(False)
    eng.close()


def test_large_nms_fp32_against_oracle_forward():
    """fp32 engine vs the oracle's own forward at 800x768, under the contract of test_nms_rows_match_oracle."""
    from yolo_puncture_amd.engine import Engine
    family, shape, conf = "11", (1, 800, 768), 0.25
    st, im = make_case_family(family, "n", 80, 0, shape)
    ref = SegOracle(st, family, "n", 80, "fp32").forward(im, conf=conf)
    ref64 = SegOracle(st, family, "n", 80, "fp64").forward(im, conf=conf)
    eng = Engine("n", 80, True, "fp32", 0, state=st, family=family)
    eng.set_nms(conf, 0.7)
    out = eng.forward(im.cuda())
    torch.cuda.synchronize()
    det, idx, cf = out["det"].cpu()[0], out["idx"].cpu()[0].long(), out["coeff"].cpu()[0]
    eng.close()
    want, widx, wcf = ref["det"][0], ref["idx"][0], ref["coeff"][0]
    n = want.shape[0]
    ncand = int((ref["scores"][0].max(1).values > conf).sum())
    assert n >= 5 and n < ncand, "the case must make NMS work"
    assert int((idx >= 0).sum()) == n
    s = want[:, 4]
    gap = (s[:-1] - s[1:]).abs()
    clear = torch.ones(n, dtype=torch.bool)
    clear[1:] &= gap > 1e-5
    clear[:-1] &= gap > 1e-5
    assert clear.float().mean() > 0.5
    assert torch.equal(idx[:n][clear], widx[clear]) and torch.equal(det[:n, 5][clear], want[:, 5][clear])
    w64, i64, c64 = ref64["det"][0], ref64["idx"][0], ref64["coeff"][0]
    assert w64.shape[0] == n, "fp32 and fp64 oracle keep different row counts: pick another seed / conf for this case"
    same = clear & (i64 == widx) & (w64[:, 5].float() == want[:, 5]) & (idx[:n] == widx)
    assert same.float().mean() > 0.5
    assert_within_noise_floor("NMS rows: boxes [px]", det[:n, :4][same], want[:, :4][same], w64[:, :4][same], 1e-3)
    assert_within_noise_floor("NMS rows: scores", det[:n, 4][same], want[:, 4][same], w64[:, 4][same], 1e-3, ceiling=1e-4)
    assert_within_noise_floor("NMS rows: mask coefficients", cf[:n][same], wcf[same], c64[same], 1e-3)
