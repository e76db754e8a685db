"""The two post-process heads on crafted inputs (tests/head_cases.py): ties, saturation, thresholds met exactly, more survivors than rows,
boxes on both sides of the NMS kernel's LDS cache - what the scores of a seeded random network never produce.

A real engine is built from plain synthetic weights and run once (that allocates its plan); the crafted class logits, box logits and mask
coefficients are written over the head's input tensors (fp32 in both numeric modes), then the three class-max ops and the head op are
launched on them, as an engine's forward would launch them. References and tolerances: head_cases.py; tests/test_head_cases_host.py
proves on the CPU that every case reaches the branch it is named after."""
import pytest
import torch

import head_cases as H
from helpers import assert_within_noise_floor

pytestmark = pytest.mark.gpu

_RIGS = {}
_STATES = {}


class _Rig:
    """an engine whose head can be launched on tensors of our making"""

    def __init__(self, family, dtype, dense, nc, max_det, shape, seg, monkeypatch):
        from yolo_puncture_amd.engine import Engine
        from yolo_puncture_amd.weights import synthetic_state, synthetic_state_family
        key = (family, nc, seg)
        if key not in _STATES:
            _STATES[key] = synthetic_state("n", nc, seg, seed=0) if family == "v10" else synthetic_state_family(family, "n", nc, seed=0)
        if dense:
            monkeypatch.setenv("YOLOP_DENSE_HEAD", "1")          # read by yp_create
        else:
            monkeypatch.delenv("YOLOP_DENSE_HEAD", raising=False)
        self.eng = eng = Engine("n", nc, seg, dtype, 0, max_det=max_det, state=_STATES[key], family=family)
        eng.set_autotune(False)
        Hh, Ww = H.SHAPES[shape]
        self.im = torch.zeros((H.B, Hh, Ww, 3), dtype=torch.uint8, device="cuda")
        self.out = eng.forward(self.im)                          # allocates the plan
        torch.cuda.synchronize()
        ops = eng.plan(H.B, Hh, Ww)
        self.head = [i for i, o in enumerate(ops) if o["kind"] == "head"]
        assert len(self.head) == 1
        self.head = self.head[0]
        self.kernel = ops[self.head]["kernel"]
        am = sorted((o["name"], i, o["out"][0]) for i, o in enumerate(ops) if o["kind"] == "amax")
        assert [n.rsplit(".", 1)[1] for n, _, _ in am] == ["0", "1", "2"], am
        self.amax = [(i, t) for _, i, t in am]
        hi = am[0][0].split(".")[1]
        pre = "one2one_" if family == "v10" else ""
        names = {t["name"]: t for t in eng.tensors()}

        def find(n):
            t = names.get(n)
            assert t is None or t["f32"], n
            return None if t is None else t["index"]
        self.cls = [find(f"model.{hi}.{pre}cv3.{l}.2") for l in range(3)]
        self.box = [find(f"model.{hi}.{pre}cv2.{l}.2") for l in range(3)]
        self.cf = [find(f"model.{hi}.cv4.{l}.2") for l in range(3)] if seg else [None] * 3
        assert None not in self.cls
        self.sparse = family == "v10" and bool(eng.head_winners(H.B)[0] & 1)
        self.seg, self.max_det = seg, max_det

    def launch(self, cls, box, cf, write=True):
        """-> det [B,max_det,6], idx [B,max_det], coeff [B,max_det,32] | None, class-max keys [B,A] (host tensors)"""
        eng = self.eng
        if write:
            for l in range(3):
                eng.write_tensor(self.cls[l], 0, cls[l])
                if self.box[l] is not None and not self.sparse:
                    eng.write_tensor(self.box[l], 0, box[l])
                if self.cf[l] is not None and not self.sparse:
                    eng.write_tensor(self.cf[l], 0, cf[l])
        self.out["det"].fill_(7.0)                               # rows past the count must be WRITTEN as zero / -1
        self.out["idx"].fill_(12345)
        if self.out.get("coeff") is not None:
            self.out["coeff"].fill_(7.0)
        for i, _ in self.amax:
            eng.run_op(i, self.im, self.out)
        eng.run_op(self.head, self.im, self.out)
        torch.cuda.synchronize()
        keys = torch.cat([eng.read_tensor(t).reshape(H.B, -1) for _, t in self.amax], 1)
        cfo = self.out["coeff"].cpu().clone() if self.out.get("coeff") is not None else None
        return self.out["det"].cpu().clone(), self.out["idx"].cpu().long(), cfo, keys


def _rig(monkeypatch, family, dtype, dense, nc, max_det, shape, seg):
    """Engines stay open until the module ends (about 37 of variant n, a few hundred MB in all): a dense and a winners-only engine of one
    configuration are needed side by side, and every case of a configuration reuses them."""
    key = (family, dtype, dense, nc, max_det, shape, seg)
    if key not in _RIGS:
        _RIGS[key] = _Rig(family, dtype, dense, nc, max_det, shape, seg, monkeypatch)
    return _RIGS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RIGS.values():
        r.eng.close()
    _RIGS.clear()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_scores(what, got, want):
    """values within 2e-7 of torch's sigmoid; descending; rows the reference ties carry bit-equal scores"""
    if got.numel() == 0:
        return
    err = float((got - want).abs().max())
    print(f"[head scores] {what}: max |engine - torch sigmoid| {err:.3e} (bound {H.SCORE_TOL:g}), {got.numel()} rows")
    assert err <= H.SCORE_TOL, (what, err)
    assert bool((got[1:] <= got[:-1]).all()), what
    tie = want[1:] == want[:-1]
    assert torch.equal(_bits(got[1:])[tie], _bits(got[:-1])[tie]), f"{what}: tied rows differ in their score bits"


def _assert_amax(what, keys, cls_flat, idx, det, n_rows):
    """class-max keys: within 2e-7 of sigmoid(max_c logit) everywhere; bit-equal to the score column of the head's own rows wherever a row
    is its anchor's best class"""
    mx = cls_flat.max(2).values
    assert float((keys - mx.sigmoid()).abs().max()) <= H.SCORE_TOL, what
    nrow = 0
    for b in range(H.B):
        n = n_rows[b]
        a, c = idx[b, :n], det[b, :n, 5].long()
        top = cls_flat[b, a, c] == mx[b, a]
        assert torch.equal(_bits(keys[b, a[top]]), _bits(det[b, :n, 4][top])), f"{what}: class-max key != score of the same logit"
        nrow += int(top.sum())
    assert nrow > 0 or sum(n_rows) == 0


V10_KINDS = {"fp32": ("fp32", True), "bf16_dense": ("bf16", True), "bf16_winners": ("bf16", False)}


def _v10_run(monkeypatch, kind, c, swap=False):
    dtype, dense = V10_KINDS[kind]
    rig = _rig(monkeypatch, "v10", dtype, dense, c.nc, c.max_det, c.shape, c.seg)
    t = H.v10_inputs(c)
    order = [1, 0] if swap else [0, 1]
    cls, box, cf = H.tensors({k: t[k][order] for k in ("cls", "box", "cf")}, c.shape)
    return rig, rig.launch(cls, box, cf)


@pytest.mark.parametrize("c", H.V10_CASES, ids=H.v10_id)
@pytest.mark.parametrize("kind", list(V10_KINDS))
def test_v10_head_on_crafted_logits(kind, c, monkeypatch):
    rig, (det, idx, cf, keys) = _v10_run(monkeypatch, kind, c)
    t = H.v10_inputs(c)
    A = H.n_anchors(c.shape)
    k = min(c.max_det, A)
    want, widx, _ = H.v10_reference(c, "fp32")
    if kind == "bf16_winners" and c.nc == 80:
        assert rig.sparse and "head_select" in rig.kernel, rig.kernel
    if kind != "bf16_winners":
        assert not rig.sparse
    if c.shape == "XL":
        assert "large" in rig.kernel, rig.kernel
    assert torch.equal(idx[:, :k], widx), (int((idx[:, :k] != widx).sum()), "rows differ in their anchor")
    assert torch.equal(det[:, :k, 5], want[..., 5])
    for b in range(H.B):
        _assert_scores(f"{H.v10_id(c)} {kind} image {b}", det[b, :k, 4], want[b, :, 4])
    assert bool((idx[:, k:] == -1).all()) and (k == c.max_det or float(det[:, k:].abs().max()) == 0.0)
    _assert_amax(f"{H.v10_id(c)} {kind}", keys, t["cls"], idx, det, [k] * H.B)
    if not rig.sparse:
        assert torch.equal(det[:, :k, :4], want[..., :4]), "one-hot boxes decode exactly"
        if c.seg:
            bi = torch.arange(H.B)[:, None].expand(H.B, k)
            assert torch.equal(cf[:, :k], t["cf"][bi, widx]) and (k == c.max_det or float(cf[:, k:].abs().max()) == 0.0)
    else:
        # only the class logits of this engine can be crafted (its boxes are recomputed at the winners): everything the select decides
        # must equal the dense engine's
        _, (ddet, didx, _, _) = _v10_run(monkeypatch, "bf16_dense", c)
        assert torch.equal(idx, didx) and torch.equal(_bits(det[..., 4:]), _bits(ddet[..., 4:]))
    # the same launch again: identical bytes; images swapped: rows swapped
    det2, idx2, cf2, keys2 = rig.launch(None, None, None, write=False)
    assert torch.equal(_bits(det2), _bits(det)) and torch.equal(idx2, idx) and torch.equal(_bits(keys2), _bits(keys))
    assert cf is None or torch.equal(_bits(cf2), _bits(cf))
    _, (sdet, sidx, scf, skeys) = _v10_run(monkeypatch, kind, c, swap=True)
    assert torch.equal(sidx, idx.flip(0)) and torch.equal(_bits(skeys), _bits(keys.flip(0)))
    cols = slice(4, 6) if rig.sparse else slice(0, 6)           # (the winners-only engine's boxes come from its own frames: both are zeros)
    assert torch.equal(_bits(sdet[..., cols]), _bits(det.flip(0)[..., cols]))
    if cf is not None and not rig.sparse:
        assert torch.equal(_bits(scf), _bits(cf.flip(0)))


def _nms_run(monkeypatch, family, c, swap=False):
    rig = _rig(monkeypatch, family, "bf16", False, H.NC, c.max_det, c.shape, True)
    rig.eng.set_nms(c.conf, c.iou)
    t = H.nms_inputs(c)
    order = [1, 0] if swap else [0, 1]
    cls, box, cf = H.tensors({k: t[k][order] for k in ("cls", "box", "cf")}, c.shape)
    return rig, rig.launch(cls, box, cf)


@pytest.mark.parametrize("c", H.NMS_CASES, ids=H.nms_id)
@pytest.mark.parametrize("family", ["v8", "11"])
def test_nms_head_on_crafted_logits(family, c, monkeypatch):
    rig, (det, idx, cf, keys) = _nms_run(monkeypatch, family, c)
    t = H.nms_inputs(c)
    rows, _, _ = H.nms_reference(c, "fp32")
    rows64, _, _ = H.nms_reference(c, "fp64")
    large = H.n_anchors(c.shape) > 12288
    assert ("gather" in rig.kernel) == large, rig.kernel
    for b in range(H.B):
        want, widx, wcf = rows[b]
        n = want.shape[0]
        got_n = int((idx[b] >= 0).sum())
        assert got_n == n, (b, got_n, n)
        assert bool((idx[b, n:] == -1).all()) and (n == c.max_det or (float(det[b, n:].abs().max()) == 0.0 and float(cf[b, n:].abs().max()) == 0.0))
        assert torch.equal(idx[b, :n], widx), (b, int((idx[b, :n] != widx).sum()))
        assert torch.equal(det[b, :n, 5], want[:, 5])
        assert torch.equal(cf[b, :n], wcf), "coefficients of kept rows are the rows that were written"
        _assert_scores(f"{H.nms_id(c)} {family} image {b}", det[b, :n, 4], want[:, 4])
        if c.name != "random_boxes":
            assert torch.equal(det[b, :n, :4], want[:, :4]), "one-hot boxes decode exactly"
        else:
            w64, i64, _ = rows64[b]
            same = (i64 == widx) & (w64[:, 5] == want[:, 5]) if w64.shape[0] == n else torch.zeros(n, dtype=torch.bool)
            assert float(same.float().mean()) > 0.5
            assert_within_noise_floor(f"{H.nms_id(c)} {family} image {b}: boxes [px]", det[b, :n, :4][same], want[:, :4][same], w64[:, :4][same], 1e-3)
    _assert_amax(f"{H.nms_id(c)} {family}", keys, t["cls"], idx, det, [r[0].shape[0] for r in rows])
    det2, idx2, cf2, _ = rig.launch(None, None, None, write=False)
    assert torch.equal(_bits(det2), _bits(det)) and torch.equal(idx2, idx) and torch.equal(_bits(cf2), _bits(cf))
    _, (sdet, sidx, scf, _) = _nms_run(monkeypatch, family, c, swap=True)
    assert torch.equal(sidx, idx.flip(0)) and torch.equal(_bits(sdet), _bits(det.flip(0))) and torch.equal(_bits(scf), _bits(cf.flip(0)))


def test_max_det_beyond_the_head_kernels_is_refused_at_create():
    """include/yolop.h, yp_create and the kernels name one bound: 512 rows for detect engines (MAXK / NMAXK), 480 for segment engines
    (YP_MAX_MASKS). Nothing is launched: yp_create validates before it touches the device."""
    from yolo_puncture_amd.engine import Engine, YolopError
    for max_det in (513, 600, 1024):
        with pytest.raises(YolopError, match="512"):
            Engine("n", 80, False, "bf16", 0, max_det=max_det)
    for family in ("v10", "v8", "11"):
        with pytest.raises(YolopError, match="480"):
            Engine("n", 80, True, "bf16", 0, max_det=481, family=family)
    Engine("n", 80, False, "bf16", 0, max_det=512).close()
    Engine("n", 80, True, "bf16", 0, max_det=480, family="v8").close()
