"""predict(classes=, agnostic_nms=, max_nms=) on the GPU: the NMS head's option kernels against the reference of tests/nms_option_cases.py.

As tests/test_gpu_head_crafted.py: a real 11n-seg engine, the crafted class logits, box logits and mask coefficients written over its head
tensors, the class-max ops and the head op launched on them - on both paths (up to 12288 anchors: head_nms_opt_kernel; beyond:
head_nms_gather_opt_kernel + head_nms_large_opt_kernel, two rounds at 16800 candidates). Then the engine as a whole: graph replay under
changing options, options set and reset, the facade for a v8-seg checkpoint, and v10 (host filter; the C entry refuses)."""
import numpy as np
import pytest
import torch

import head_cases as H
import nms_option_cases as N
from helpers import assert_within_noise_floor, make_case, make_case_family
from oracle.yolo_seg_oracle import SegOracle

pytestmark = pytest.mark.gpu

_RIGS = {}


class _Rig:
    """an 11n-seg engine at one input size whose head can be launched on tensors of our making"""

    def __init__(self, hw):
        from yolo_puncture_amd.engine import Engine
        from yolo_puncture_amd.weights import synthetic_state_family
        if "state" not in _RIGS:
            _RIGS["state"] = synthetic_state_family("11", "n", N.NC, seed=0)
        self.eng = eng = Engine("n", N.NC, True, "bf16", 0, max_det=300, state=_RIGS["state"], family="11")
        eng.set_autotune(False)
        self.hw = hw
        self.im = torch.zeros((N.B, hw[0], hw[1], 3), dtype=torch.uint8, device="cuda")
        self.out = eng.forward(self.im)                          # allocates the plan
        torch.cuda.synchronize()
        ops = eng.plan(N.B, *hw)
        (self.head,) = [i for i, o in enumerate(ops) if o["kind"] == "head"]
        am = sorted((o["name"], i) for i, o in enumerate(ops) if o["kind"] == "amax")
        self.amax = [i for _, i in am]
        hi = am[0][0].split(".")[1]
        self.cls = [eng.find_tensor(f"model.{hi}.cv3.{l}.2") for l in range(3)]
        self.box = [eng.find_tensor(f"model.{hi}.cv2.{l}.2") for l in range(3)]
        self.cf = [eng.find_tensor(f"model.{hi}.cv4.{l}.2") for l in range(3)]
        self.written = None

    def kernel(self):
        return self.eng.plan(N.B, *self.hw)[self.head]["kernel"]

    def launch(self, c, scene_key):
        eng = self.eng
        if self.written != scene_key:
            t = N.inputs(c)
            for l in range(3):
                eng.write_tensor(self.cls[l], 0, N.split_levels(c, t["cls"])[l])
                eng.write_tensor(self.box[l], 0, N.split_levels(c, t["box"])[l])
                eng.write_tensor(self.cf[l], 0, N.split_levels(c, t["cf"])[l])
            self.written = scene_key
        self.out["det"].fill_(7.0)                               # rows past the count must be WRITTEN as zero / -1
        self.out["idx"].fill_(12345)
        self.out["coeff"].fill_(7.0)
        for i in self.amax:
            eng.run_op(i, self.im, self.out)
        eng.run_op(self.head, self.im, self.out)
        torch.cuda.synchronize()
        return self.out["det"].cpu().clone(), self.out["idx"].cpu().long(), self.out["coeff"].cpu().clone()


def _rig(hw):
    if hw not in _RIGS:
        _RIGS[hw] = _Rig(hw)
    return _RIGS[hw]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, r in _RIGS.items():
        if k != "state":
            r.eng.close()
    _RIGS.clear()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_rows(what, c, det, idx, cf, rows, exact_boxes=True):
    for b in range(N.B):
        want, widx, wcf = rows[b]
        n = want.shape[0]
        got_n = int((idx[b] >= 0).sum())
        print(f"[nms options] {what} image {b}: {got_n} rows (reference {n})")
        assert got_n == n, (what, b, got_n, n)
        assert bool((idx[b, n:] == -1).all())
        assert n == c.max_det or (float(det[b, n:].abs().max()) == 0.0 and float(cf[b, n:].abs().max()) == 0.0)
        assert torch.equal(idx[b, :n], widx), (what, b, int((idx[b, :n] != widx).sum()))
        assert torch.equal(det[b, :n, 5], want[:, 5])
        assert torch.equal(cf[b, :n], wcf), "coefficients of kept rows are the rows that were written"
        if n:
            err = float((det[b, :n, 4] - want[:, 4]).abs().max())
            print(f"[nms options] {what} image {b}: max |score - torch sigmoid| {err:.3e} (bound {N.SCORE_TOL:g})")
            assert err <= N.SCORE_TOL
            assert bool((det[b, 1:n, 4] <= det[b, :n - 1, 4]).all())
        if exact_boxes:
            assert torch.equal(det[b, :n, :4], want[:, :4]), "one-hot boxes decode exactly"


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_option_kernels_on_crafted_logits(c):
    c = N.resolve(c)
    rig = _rig(N.case_hw(c))
    rig.eng.set_nms(c.conf, c.iou)
    rig.eng.set_nms_options(c.classes, c.agnostic, c.max_nms)
    large = N.n_anchors(c) > H.CAP
    want_kernel = {(False, False): "head_nms_kernel", (False, True): "head_nms_opt_kernel",
                   (True, False): "head_nms_gather_kernel + head_nms_large_kernel",
                   (True, True): "head_nms_gather_opt_kernel + head_nms_large_opt_kernel"}[(large, not N.is_default(c))]
    assert rig.kernel() == want_kernel
    det, idx, cf = rig.launch(c, (c.scene, c.shape))
    exact = c.scene != "random_boxes"                           # (real-valued boxes: compared with the default kernel's below)
    _assert_rows(c.id, c, det, idx, cf, N.reference(c), exact_boxes=exact)
    # the same launch again: identical bytes
    det2, idx2, cf2 = rig.launch(c, (c.scene, c.shape))
    assert torch.equal(_bits(det2), _bits(det)) and torch.equal(idx2, idx) and torch.equal(_bits(cf2), _bits(cf))
    # back to the default options on the same tensors: the default kernel, the oracle's rows
    rig.eng.set_nms_options()
    assert "opt" not in rig.kernel()
    ddet, didx, dcf = rig.launch(c, (c.scene, c.shape))
    _assert_rows(c.id + " (defaults again)", c, ddet, didx, dcf, N.reference(c, **N.DEFAULTS), exact_boxes=exact)
    # an anchor that is a row under both settings carries the same bytes in both (one decode kernel serves both forms)
    for b in range(N.B):
        at = {int(a): r for r, a in enumerate(didx[b]) if a >= 0}
        both = [(r, at[int(a)]) for r, a in enumerate(idx[b]) if int(a) in at]
        if both:
            ro, rd = (torch.tensor(v) for v in zip(*both))
            assert torch.equal(_bits(det[b, ro]), _bits(ddet[b, rd]))


@pytest.fixture(scope="module")
def real_case():
    """a calibrated 11n-seg network and the frames it was calibrated on: rows of several classes, overlapping boxes"""
    return make_case_family("11", "n", 80, 0, (2, 96, 128))


def _engine(st, graph):
    from yolo_puncture_amd.engine import Engine
    eng = Engine("n", 80, True, "bf16", 0, state=st, family="11")
    eng.set_autotune(False)
    eng.set_graph(1 if graph else 0)
    return eng


def _forward(eng, im):
    out = eng.forward(im)
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in out.items() if v is not None}


def _same_out(a, b):
    return torch.equal(_bits(a["det"]), _bits(b["det"])) and torch.equal(a["idx"], b["idx"]) and torch.equal(_bits(a["coeff"]), _bits(b["coeff"]))


def test_graph_replay_follows_the_options(real_case):
    """Options changed between two replays of one captured graph: the replay equals an eager engine with the same options (the values
    live in device memory), and a change among non-default options captures nothing anew."""
    st, im = real_case
    im = im.cuda()
    g, e = _engine(st, True), _engine(st, False)
    for eng in (g, e):
        eng.set_nms(0.05, 0.7)
    base = _forward(e, im)
    assert _same_out(_forward(g, im), base)
    cls0 = base["det"][0, :, 5][base["idx"][0] >= 0]
    k = int(torch.mode(cls0).values)
    assert len(set(cls0.tolist())) > 1, "the frame has rows of more than one class"
    settings = [dict(classes=[k]), dict(classes=[k], agnostic=True, max_nms=40), dict(agnostic=True), dict(max_nms=7)]
    captures, outs = [], []
    for s in settings:
        for eng in (g, e):
            eng.set_nms_options(**s)
        _forward(g, im)                                              # (the first replay after a change ...)
        got, want = _forward(g, im), _forward(e, im)                 # (... and the one after it)
        assert _same_out(got, want), s
        captures.append(g.graph_info()["captures"])
        outs.append(got)
        assert g.graph_info()["live"]
    assert captures[0] == captures[-1], "option values change under a captured graph without a new capture"
    n0 = int((outs[0]["idx"][0] >= 0).sum())
    assert 0 < n0 < int((base["idx"][0] >= 0).sum()) and bool((outs[0]["det"][0, :n0, 5] == k).all())
    assert int((outs[3]["idx"][0] >= 0).sum()) <= 7
    assert torch.equal(outs[3]["idx"][0, :1], base["idx"][0, :1]), "the best candidate always stays"
    for eng in (g, e):
        eng.set_nms_options()
    assert _same_out(_forward(g, im), base) and _same_out(_forward(e, im), base)
    g.close(); e.close()


def test_options_set_and_reset_equal_never_set(real_case):
    st, im = real_case
    im = im.cuda()
    for graph in (False, True):
        a, b = _engine(st, graph), _engine(st, graph)
        for eng in (a, b):
            eng.set_nms(0.05, 0.7)
        a.set_nms_options(classes=[0, 3], agnostic=True, max_nms=30000)  # before the first forward
        changed = _forward(a, im)
        head = a.plan(2, 96, 128)[-1]["kernel"]
        assert head == "head_nms_opt_kernel", head
        a.set_nms_options()
        assert a.plan(2, 96, 128)[-1]["kernel"] == "head_nms_kernel" == b.plan(2, 96, 128)[-1]["kernel"]
        never = _forward(b, im)
        assert _same_out(_forward(a, im), never) and not _same_out(changed, never)
        a.close(); b.close()


def _head_rows(eng, st, family, hw, conf, iou, **opts):
    """the reference on the ENGINE's own head tensors of image 0 (as tests/test_gpu_large_nms.py _host_rows) -> fp32 rows, fp64 rows"""
    hi = 22 if family == "v8" else 23
    cat = lambda pre, C: torch.cat([eng.read_tensor(eng.find_tensor(f"model.{hi}.{pre}.{l}.2")).reshape(1, -1, C) for l in range(3)], 1).permute(0, 2, 1)
    bl, cl, cf = cat("cv2", 64), cat("cv3", 80), cat("cv4", 32)
    out = []
    for mode, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
        o = SegOracle(st, family, "n", 80, mode)
        boxes, scores = o.decode(bl.to(dt).contiguous(), cl.to(dt).contiguous(), [(hw[0] // s, hw[1] // s) for s in (8, 16, 32)])
        cxy, wh = (boxes[..., :2] + boxes[..., 2:]) / 2, boxes[..., 2:] - boxes[..., :2]
        boxes = torch.cat((cxy - wh / 2, cxy + wh / 2), -1)
        out.append(N.nms_postprocess_opts(boxes[0].float(), scores[0].float(), cf[0].permute(1, 0).float(), conf, iou, 300, **opts))
    return out


def test_facade_predict_with_classes_and_agnostic_nms(tmp_path):
    from yolo_puncture_amd import YOLO
    from yolo_puncture_amd.weights import read_ultralytics_pt, save_as_ultralytics_pt
    family, hw = "v8", (384, 640)
    st, ims = make_case_family(family, "n", 80, 0, (1,) + hw)          # 384x640 letterboxes to itself
    frame = ims[0].numpy()
    path = str(tmp_path / "v8n-seg.pt")
    save_as_ultralytics_pt(st, path)
    st_rt, _ = read_ultralytics_pt(path)
    model = YOLO(path, dtype="fp32")
    eng = model._engine()
    eng.set_autotune(False)
    conf = 0.3
    r0 = model.predict(frame, conf=conf, device="cuda")[0]
    cls0 = r0.boxes.cpu().numpy().cls.astype(int)
    assert len(set(cls0.tolist())) >= 3
    classes = sorted(set(cls0.tolist()))[:-1]                           # every class of the default rows but one
    r = model.predict(frame, conf=conf, classes=classes, agnostic_nms=True)[0]
    assert "opt" in eng.plan(1, *hw)[-1]["kernel"]
    (want, widx, wcf), (w64, i64, _) = _head_rows(eng, st_rt, family, hw, conf, 0.7, classes=classes, agnostic=True)
    dflt = _head_rows(eng, st_rt, family, hw, conf, 0.7)[0]
    b = r.boxes.cpu().numpy()
    n = want.shape[0]
    dropped = sorted(set(cls0.tolist()))[-1]
    assert bool((dflt[0][:, 5] == dropped).any()) and not torch.equal(dflt[1][:n], widx), "the options change this frame's rows"
    assert n > 0 and len(b.cls) == n and set(b.cls.astype(int).tolist()) <= set(classes)
    out = model._out_cache[(model._dev_index, 1)]
    assert torch.equal(out["idx"][0, :n].cpu().long(), widx) and bool((out["idx"][0, n:] == -1).all())
    assert torch.equal(torch.from_numpy(b.cls), want[:, 5])
    assert float((torch.from_numpy(b.conf) - want[:, 4]).abs().max()) <= N.SCORE_TOL
    same = (i64 == widx) & (w64[:, 5] == want[:, 5]) if w64.shape[0] == n else torch.zeros(n, dtype=torch.bool)
    assert float(same.float().mean()) > 0.5
    clip = lambda d: torch.stack((d[:, 0].clamp(0, hw[1]), d[:, 1].clamp(0, hw[0]), d[:, 2].clamp(0, hw[1]), d[:, 3].clamp(0, hw[0])), 1)
    assert_within_noise_floor("facade boxes under options [px]", torch.from_numpy(b.xyxy)[same], clip(want[:, :4])[same], clip(w64[:, :4])[same], 1e-3)
    # the masks belong to the kept rows: the engine's coefficient rows are those anchors' (exact), and the masks are the mask tail's on them
    assert torch.equal(out["coeff"][0, :n].cpu(), wcf)
    m, _, _ = eng.masks(0, wcf.cuda(), out["det"][0, :n, :4].clone(), hw, retina=False)
    assert r.masks is not None and tuple(r.masks.data.shape) == (n,) + hw and torch.equal(r.masks.data.cpu(), m.float().cpu())
    # arguments are checked against the model
    with pytest.raises(ValueError, match="not a class"):
        model.predict(frame, classes=[80])
    with pytest.raises(ValueError, match="max_nms"):
        model.predict(frame, max_nms=0)
    # and a later call with fixed arguments finds the defaults again
    assert len(model.predict(frame, conf=conf)[0].boxes.cls) == len(cls0)
    assert "opt" not in eng.plan(1, *hw)[-1]["kernel"]


def test_v10_filters_rows_on_the_host(tmp_path):
    from yolo_puncture_amd import YOLO
    from yolo_puncture_amd.engine import YolopError
    from yolo_puncture_amd.weights import save_as_ultralytics_pt
    st, ims = make_case("n", 80, True, 0, (1, 384, 640))
    frame = ims[0].numpy()
    path = str(tmp_path / "v10n-seg.pt")
    save_as_ultralytics_pt(st, path)
    model = YOLO(path, dtype="fp32")
    model._engine().set_autotune(False)
    conf = 0.05
    r0 = model.predict(frame, conf=conf, device="cuda")[0]
    b0 = r0.boxes.cpu().numpy()
    k = int(np.bincount(b0.cls.astype(int)).argmax())
    keep = b0.cls.astype(int) == k
    assert 0 < keep.sum() < len(keep)
    r = model.predict(frame, conf=conf, classes=[k], agnostic_nms=True, max_nms=30000)[0]     # (the last two: accepted, no effect)
    b = r.boxes.cpu().numpy()
    assert np.array_equal(b.cls, b0.cls[keep]) and np.array_equal(b.conf, b0.conf[keep]) and np.array_equal(b.xyxy, b0.xyxy[keep])
    assert torch.equal(r.masks.data.cpu(), r0.masks.data.cpu()[torch.from_numpy(keep)])
    assert len(model.predict(frame, conf=conf, classes=k)[0].boxes.cls) == int(keep.sum())
    with pytest.raises(YolopError, match="no NMS"):
        model._engine().set_nms_options(classes=[k])
    with pytest.raises(ValueError, match="v8 / 11"):
        model.predict_clip([frame], conf=conf, classes=[k])
