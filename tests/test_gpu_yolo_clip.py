"""YOLO.predict_clip on the GPU: yp_letterbox_batch and yp_masks_frames byte-equal to their per-frame forms, and the clip's (boxes, coords,
lens) equal to predict() on each padded chunk of the same YOLO instance followed by the app's per-frame extraction (yolo_seg/app.py:91-113),
for the v8, 11 and v10 seg layouts, host and device frames, every polygon strategy; the classifier's clip call on device frames."""
import numpy as np
import pytest
import torch

from helpers import _CalibOracle, make_case_family, rand_image
from yolo_puncture_amd import hostops, predictor
from yolo_puncture_amd import classify as C
from yolo_puncture_amd.engine import Engine, letterbox_batch_device, letterbox_device
from yolo_puncture_amd.predictor import YOLO
from yolo_puncture_amd.weights import save_as_ultralytics_pt, synthetic_state

pytestmark = pytest.mark.gpu
N = 12


def upsample_720p(ims):
    """384x640 frames -> 2x nearest -> 720x1280 (as tools/seg_frame_trace.py)."""
    return [np.ascontiguousarray(np.repeat(np.repeat(im, 2, 0), 2, 1)[:720, :1280]) for im in ims]


def v10_seg_state(ims, seed=3):
    """A calibrated v10-N-seg state dict (the ckpt fixture of the facade tests, restated): synthetic weights rescaled on these frames."""
    st0 = synthetic_state("n", 80, True, seed=seed, cls_bias=-1.0)
    co = _CalibOracle(st0, "n", 80, True, "fp32")
    co.forward(torch.from_numpy(np.stack(ims)))
    st = {}
    for name, (w, b) in co.w.items():
        if f"{name}.conv.weight" in st0:
            c2 = w.shape[0]
            st.update({f"{name}.conv.weight": w, f"{name}.bn.weight": torch.ones(c2), f"{name}.bn.bias": b,
                       f"{name}.bn.running_mean": torch.zeros(c2), f"{name}.bn.running_var": torch.full((c2,), 1 - 1e-3)})
        else:
            st.update({f"{name}.weight": w, f"{name}.bias": b})
    return st


_CASES = {}


def clip_case(fam, tmp_path_factory, n=N):
    """-> (YOLO, 720p frames, conf): frame order and conf chosen so that about a third of the frames, frame 0 among them, detect nothing."""
    key = (fam, n)
    if key in _CASES:
        return _CASES[key]
    if fam == "v10":
        ims = [im.numpy() for im in rand_image((n, 384, 640, 3), seed=5)]
        st = v10_seg_state(ims)
    else:
        st, t = make_case_family(fam, "n", 80, 0, (n, 384, 640))
        ims = [im.numpy() for im in t]
    path = str(tmp_path_factory.mktemp("clip") / f"{fam}n-seg.pt")
    save_as_ultralytics_pt(st, path)
    model = YOLO(path)
    frames = upsample_720p(ims)
    best = []
    for r in model.predict(frames, conf=0.01, retina_masks=True):
        c = r.boxes.cpu().numpy().conf
        best.append(float(c.max()) if len(c) else 0.0)
    order = np.argsort(best, kind="stable")
    order = [int(order[0])] + [int(i) for i in np.random.RandomState(1).permutation(order[1:])]
    frames = [frames[i] for i in order]
    s = np.sort(best)
    cut = max(1, n // 3)
    conf = float((s[cut - 1] + s[cut]) / 2) if s[cut] > s[cut - 1] else float(s[cut - 1])
    assert s[-1] > conf, "no frame of the clip detects anything"
    _CASES[key] = (model, frames, conf)
    return _CASES[key]


def oracle_clip(model, frames, conf, bs):
    """predict() on each padded chunk (same instance), then the app's per-frame extraction and carry-forward (yolo_seg/app.py:91-113)."""
    B, chunks = hostops.clip_plan(len(frames), bs)
    H, W = frames[0].shape[:2]
    boxes, coords, lens = [], [], []
    last_box, last_rect_len = None, 0
    for s0, c in chunks:
        chunk = frames[s0:s0 + c] + [frames[s0 + c - 1]] * (B - c)
        res = model.predict(chunk, conf=conf, retina_masks=True)
        for r in res[:c]:
            pb = r.boxes.cpu().numpy()
            if len(pb.cls) > 0:
                best = np.argmax(pb.conf)
                box = list(map(int, pb.xyxy[best].squeeze()))
                last_box = box
                seg = r.masks.xy[best]
                coords.append(seg)
                rect_len, _ = r.masks.min_rect_len(int(best))
                last_rect_len = rect_len
                lens.append(rect_len)
            else:
                box = (0, 0, W, H) if last_box is None else last_box
                coords.append(None)
                lens.append(last_rect_len)
            boxes.append(box)
    return boxes, coords, lens


def assert_same(got, ref):
    gb, gc, gl = got
    rb, rc, rl = ref
    assert [list(b) for b in gb] == [list(b) for b in rb]
    assert len(gc) == len(rc)
    for i, (p, q) in enumerate(zip(gc, rc)):
        assert (p is None) == (q is None), i
        if p is not None:
            assert p.dtype == np.float32 and np.array_equal(p, q), i
    assert gl == rl


# ---- kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h0,w0", [(720, 1280), (1080, 1920), (333, 517)])
def test_letterbox_batch_parity(h0, w0):
    rng = np.random.RandomState(h0)
    fr = torch.from_numpy(rng.randint(0, 256, (3, h0, w0, 3), dtype=np.uint8)).cuda()
    geo = hostops.letterbox_geometry(h0, w0, 640)
    out = torch.full((3, geo["out_h"], geo["out_w"], 3), 7, dtype=torch.uint8, device="cuda")
    letterbox_batch_device(fr, geo, out)
    ref = torch.stack([letterbox_device(fr[i].contiguous(), geo) for i in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    # oracle of the per-frame kernel: the host restatement
    assert np.array_equal(out[1].cpu().numpy(), hostops.letterbox(fr[1].cpu().numpy())[0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masks_frames_parity(dtype):
    ims = [im.numpy() for im in rand_image((4, 384, 640, 3), seed=11)]
    eng = Engine("n", 80, True, dtype, 0, state=v10_seg_state(ims, seed=4))
    out = eng.forward(torch.from_numpy(np.stack(ims)).cuda())
    oh, ow = 720, 1280
    boxes = torch.tensor([[0.0, 100.5, 300.2, 500.7],          # touches the left edge
                          [200.3, 0.0, 900.9, 300.1],          # the top edge
                          [700.4, 200.6, 1280.0, 600.2],       # the right edge
                          [100.0, 400.2, 1100.8, 720.0],       # the bottom edge
                          [640.2, 360.3, 640.9, 360.8],        # under one pixel
                          [0.0, 0.0, 1280.0, 720.0],           # the whole frame
                          [50.5, 60.5, 1200.5, 700.5]], dtype=torch.float32, device="cuda")
    fidx = [3, 0, 0, 2, 3, 0, 2]                                # frame 1 never, frames 0 / 2 / 3 repeated
    got = eng.masks_frames(fidx, out["coeff"], boxes, (oh, ow))
    # an output buffer that does not start on a 16-byte line: the partial lines at both ends take byte stores
    raw = torch.full((len(fidx) * oh * ow + 17,), 9, dtype=torch.uint8, device="cuda")
    got2 = eng.masks_frames(fidx, out["coeff"], boxes, (oh, ow), out=raw[3:3 + len(fidx) * oh * ow].view(len(fidx), oh, ow))
    refs = []
    for j, f in enumerate(fidx):
        m, _, _ = eng.masks(f, out["coeff"][f, :1], boxes[j:j + 1], (oh, ow), retina=True)
        refs.append(m[0].clone())
    torch.cuda.synchronize()
    ref = torch.stack(refs)
    assert torch.equal(got, ref) and torch.equal(got2, ref)
    assert int(raw[:3].ne(9).sum()) == 0 and int(raw[3 + len(fidx) * oh * ow:].ne(9).sum()) == 0
    assert int(ref.sum()) > 1000, "the masks are (nearly) empty: the test would not see the interpolation"
    for j in range(len(fidx)):                                  # nothing outside the box
        x1, y1, x2, y2 = boxes[j].tolist()
        ys, xs = torch.nonzero(got[j], as_tuple=True)
        if len(ys):
            assert xs.min() >= x1 - 1 and xs.max() < x2 + 1 and ys.min() >= y1 - 1 and ys.max() < y2 + 1
    with pytest.raises(ValueError):
        eng.masks_frames([4], out["coeff"], boxes[:1], (oh, ow))
    eng.close()


# ---- predict_clip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["v8", "11", "v10"])
def test_predict_clip_matches_predict(fam, tmp_path_factory):
    model, frames, conf = clip_case(fam, tmp_path_factory)
    dev_frames = torch.from_numpy(np.stack(frames)).cuda()
    seen_gap = False
    for bs in (1, 5, 32):
        ref = oracle_clip(model, frames, conf, bs)
        assert ref[1][0] is None, "frame 0 must detect nothing"
        seen_gap |= any(c is None for c in ref[1][1:]) and any(c is not None for c in ref[1])
        got = model.predict_clip(frames, conf=conf, batch_size=bs)
        assert_same(got, ref)
        assert got.detected == [c is not None for c in ref[1]]
        for i, d in enumerate(got.detected):
            assert (got.xyxy[i] is not None) == d and (got.conf[i] is not None) == d
            if d:
                assert got.conf[i] > conf and [int(v) for v in got.xyxy[i]] == list(ref[0][i])
        got_dev = model.predict_clip(dev_frames, conf=conf, batch_size=bs)
        assert_same(got_dev, ref)
    assert seen_gap


@pytest.mark.parametrize("fam", ["v8", "11"])
@pytest.mark.parametrize("strategy", ["largest", "all", "all_merged"])
def test_predict_clip_strategies(fam, strategy, tmp_path_factory, monkeypatch):
    model, frames, conf = clip_case(fam, tmp_path_factory)
    frames = frames[:6]
    monkeypatch.setattr(predictor, "MASK_POLYGON_STRATEGY", strategy)
    ref = oracle_clip(model, frames, conf, 4)
    got = model.predict_clip(frames, conf=conf, batch_size=4)
    assert_same(got, ref)


def test_predict_clip_host_fallback(tmp_path_factory, monkeypatch):
    """A mask the device declines is traced on the host for that frame only, as Masks.xy does: forced here by a contour list too short
    for any mask of the clip."""
    model, frames, conf = clip_case("11", tmp_path_factory)
    frames = frames[:6]
    real = predictor.mask_contours_device
    calls = []

    def short(masks, max_pts=None, **kw):
        calls.append(int(masks.shape[0]))
        return real(masks, max_pts=2, **kw)

    monkeypatch.setattr(predictor, "mask_contours_device", short)
    ref = oracle_clip(model, frames, conf, 4)                  # (Masks.xy declines and falls back too)
    n_ref = len(calls)
    got = model.predict_clip(frames, conf=conf, batch_size=4)
    assert len(calls) > n_ref and any(got.detected)
    assert_same(got, ref)


# ---- classifier on device frames ---------------------------------------------------------------------------------------------------
def test_classifier_device_frames():
    eng = C.ClassifierEngine("fp32", 0, state=C.synthetic_state(0))
    rng = np.random.RandomState(4)
    frames = rng.randint(0, 256, (11, 360, 640, 3), dtype=np.uint8)
    boxes = [(600, 300, 640, 360), (0, 0, 40, 30), (100, 50, 300, 260), (0, 0, 640, 360)] * 3
    boxes = boxes[:11]
    ref = C.predict_and_find_start_inserted(eng, list(frames), boxes, judge_wnd=4, batch_size=4)
    got = C.predict_and_find_start_inserted(eng, torch.from_numpy(frames).cuda(), boxes, judge_wnd=4, batch_size=4)
    assert got[2] == ref[2] and [int(c) for c in got[0]] == [int(c) for c in ref[0]] and np.array_equal(np.array(got[1]), np.array(ref[1]))
    eng.close()
