"""U^2-Net-P over a whole clip (yp_u2net_forward_crops / unet_predict_clip) on the GPU: device crop, per-frame normPRED, the paste into
full-frame masks, chunking and the per-shape tuning memo. Bounds are those of test_gpu_u2net.py: prob within 1e-3 of the oracle, the
uint8 mask exact wherever the normalised value is not within 1e-4 of 0.5 (fewer than 5e-3 of the pixels are)."""
import numpy as np
import pytest
import torch

from helpers import rand_image
from oracle.u2net_oracle import U2NetOracle, numpy2tensor_oracle, unet_predict_oracle
from test_u2net_clip_host import crop_frame_np
from yolo_puncture_amd.u2net import U2NetEngine, clip_chunks, crop_window, synthetic_state, unet_predict, unet_predict_clip

pytestmark = pytest.mark.gpu
H, W = 720, 1280
# (centre x, centre y) of a 60 x 60 box: interior, left / right edge (narrow: padded to 380 x 380), top / bottom edge (short: unpadded
# h x 380), the four corners (padded); several heights so that the clip has more than one crop shape
CENTRES = [(640, 360), (100, 360), (1200, 400), (640, 100), (700, 650), (50, 60), (1230, 40), (80, 690), (1250, 700),
           (400, 150), (900, 600), (640, 120)]


def clip_boxes(n):
    out = []
    for i in range(n):
        cx, cy = CENTRES[i % len(CENTRES)]
        cx, cy = cx + (i // len(CENTRES)) * 7, cy + (i // len(CENTRES)) * 3
        out.append((cx - 30, cy - 30, cx + 30, cy + 30))
    return out


@pytest.fixture(scope="module")
def clip():
    st = synthetic_state("p", 0)
    frames = rand_image((24, H, W, 3), seed=31).numpy()
    boxes = clip_boxes(24)
    oracle = []
    for f, b in zip(frames, boxes):
        crop, _ = crop_frame_np(f, b)
        norm, mask = unet_predict_oracle(st, crop)
        with torch.no_grad():
            prob = U2NetOracle(st, "p").forward(numpy2tensor_oracle(crop)[None])[0][0, 0].numpy()
        oracle.append((crop, prob, norm, mask))
    eng = U2NetEngine("p", "fp32", 0, state=st)
    res = unet_predict_clip(eng, list(frames), boxes)                 # host frames, one chunk at a time
    torch.cuda.synchronize()
    yield dict(st=st, frames=frames, boxes=boxes, oracle=oracle, eng=eng, res=res)
    eng.close()


def test_clip_against_oracle(clip):
    shapes = set()
    near_total, n_total = 0, 0
    for i, ((mask, win), (crop, _, norm, want)) in enumerate(zip(clip["res"], clip["oracle"])):
        assert win == crop_frame_np(clip["frames"][i], clip["boxes"][i])[1]
        assert mask.dtype == np.uint8 and mask.shape == crop.shape[:2] and set(np.unique(mask)) <= {0, 255}
        near = np.abs(norm - 0.5) < 1e-4
        assert np.array_equal(mask[~near], want[~near]), f"frame {i}"
        near_total += near.sum()
        n_total += near.size
        shapes.add(mask.shape)
    assert near_total / n_total < 5e-3
    assert (380, 380) in shapes and len(shapes) >= 3                  # padded crops and short unpadded ones both ran
    # prob from the device crops (frames already on the device), per crop shape
    dev = torch.from_numpy(clip["frames"]).cuda()
    geo = [crop_window(b, H, W) for b in clip["boxes"]]
    for shape, idx in clip_chunks([g[1] for g in geo], 16):
        prob, cmask, _ = clip["eng"].forward_crops(dev, [geo[i][0] for i in idx], idx, shape)
        for j, i in enumerate(idx):
            err = float(np.abs(prob[j].cpu().numpy() - clip["oracle"][i][1]).max())
            assert err < 1e-3, (i, err)
            assert np.array_equal(cmask[j].cpu().numpy(), clip["res"][i][0])


def test_clip_against_unet_predict(clip):
    for i, ((mask, _), (crop, _, norm, _)) in enumerate(zip(clip["res"], clip["oracle"])):
        got = unet_predict(clip["eng"], crop)
        near = np.abs(norm - 0.5) < 1e-4
        assert np.array_equal(mask[~near], got[~near]), f"frame {i}"


def test_normalisation_is_per_frame():
    """Two crops with different prob ranges (the second mostly zero pad): the clip path equals the two B = 1 calls; forward() over the
    stack, which normalises over the whole call, differs in at least one pixel well away from the threshold."""
    a = rand_image((1, 160, 160, 3), seed=21)[0]
    b = torch.zeros_like(a)
    b[:60, :60] = a[:60, :60]
    stack = torch.stack([a, b]).cuda()
    eng = U2NetEngine("p", "fp32", 0, state=synthetic_state("p", 0))
    try:
        _, cmask, _ = eng.forward_crops(stack, [(0, 0, 160, 160), (0, 0, 160, 160)], [0, 1], (160, 160))
        clip_masks = cmask.cpu()
        singles = [[t.cpu() for t in eng.forward(stack[i:i + 1])] for i in range(2)]
        for i, (_, norm, mask) in enumerate(singles):
            near = (norm[0] - 0.5).abs() < 1e-4
            assert torch.equal(clip_masks[i][~near], mask[0][~near])
        _, wnorm, wmask = (t.cpu() for t in eng.forward(stack))
        torch.cuda.synchronize()
        differs = []
        for i in range(2):
            far = ((singles[i][1][0] - 0.5).abs() > 1e-4) & ((wnorm[i] - 0.5).abs() > 1e-4)
            differs.append(int((wmask[i] != clip_masks[i])[far].sum()))
        print("pixels where whole-call normalisation differs from per-frame:", differs)
        assert max(differs) > 0
    finally:
        eng.close()


def test_chunking_is_bit_identical(clip, monkeypatch):
    """YOLOP_U2_SMALL_MAX=0 puts conv_igemm on every layer. Its per-element K order does not depend on M: every workgroup walks the
    whole padded K in 32-deep tiles in the same order, and the tile choice (conv_tile_choice) only sets the Cout width of a tile. The
    input, pool, up-sample and tail kernels are per element, and the per-image min / max is an exact atomic reduction. So batch 1, 5
    and 16 give the same bits."""
    monkeypatch.setenv("YOLOP_U2_SMALL_MAX", "0")
    eng = U2NetEngine("p", "fp32", 0, state=clip["st"])
    try:
        frames = torch.from_numpy(clip["frames"][:12]).cuda()
        boxes = clip["boxes"][:12]
        geo = [crop_window(b, H, W) for b in boxes]
        runs = []
        for bs in (1, 5, 16):
            probs = [None] * 12
            for shape, idx in clip_chunks([g[1] for g in geo], bs):
                prob, _, _ = eng.forward_crops(frames, [geo[i][0] for i in idx], idx, shape, want_crop_mask=False)
                for j, i in enumerate(idx):
                    probs[i] = prob[j].cpu()
            masks = unet_predict_clip(eng, frames, boxes, batch_size=bs)
            full = unet_predict_clip(eng, frames, boxes, batch_size=bs, full_frame=True).cpu()
            runs.append((probs, masks, full))
        for probs, masks, full in runs[1:]:
            for i in range(12):
                assert torch.equal(probs[i], runs[0][0][i]), i
                assert np.array_equal(masks[i][0], runs[0][1][i][0]) and masks[i][1] == runs[0][1][i][1], i
            assert torch.equal(full, runs[0][2])
    finally:
        eng.close()


def test_full_frame_paste(clip):
    full = unet_predict_clip(clip["eng"], torch.from_numpy(clip["frames"]).cuda(), clip["boxes"], full_frame=True)
    assert full.dtype == torch.uint8 and tuple(full.shape) == (24, H, W) and full.is_cuda
    full = full.cpu().numpy()
    for i, (mask, (x1, y1, x2, y2)) in enumerate(clip["res"]):
        inside = np.zeros((H, W), bool)
        inside[y1:y2, x1:x2] = True
        assert not full[i][~inside].any(), f"frame {i}: nonzero outside the window"
        assert np.array_equal(full[i][y1:y2, x1:x2], mask[:y2 - y1, :x2 - x1]), f"frame {i}"
        host = np.zeros((H, W), np.uint8)                               # the app's paste, restricted to the window
        host[y1:y2, x1:x2] = mask[:y2 - y1, :x2 - x1]
        assert np.array_equal(full[i], host)
    # host frames take the same path through a staging chunk; another batch size may time other conv kernels, so the bits may differ
    # where the normalised value is within 1e-4 of the threshold
    again = unet_predict_clip(clip["eng"], list(clip["frames"][:5]), clip["boxes"][:5], batch_size=4, full_frame=True).cpu().numpy()
    for i in range(5):
        x1, y1, x2, y2 = clip["res"][i][1]
        near = np.zeros((H, W), bool)
        near[y1:y2, x1:x2] = np.abs(clip["oracle"][i][2][:y2 - y1, :x2 - x1] - 0.5) < 1e-4
        assert np.array_equal(again[i][~near], full[i][~near]), f"frame {i}"


def test_tuning_memo(monkeypatch, capfd):
    """Shape A, shape B, shape A again: the third call restores A's timed choices and times nothing."""
    monkeypatch.delenv("YOLOP_U2_SMALL_MAX", raising=False)
    monkeypatch.setenv("YOLOP_U2_TUNE_LOG", "1")
    frames = rand_image((2, 200, 240, 3), seed=5).cuda()
    eng = U2NetEngine("p", "fp32", 0, state=synthetic_state("p", 0))
    try:
        logs, results = [], []
        for win, shape in (((0, 0, 96, 96), (96, 96)), ((0, 0, 128, 64), (64, 128)), ((0, 0, 96, 96), (96, 96))):
            capfd.readouterr()
            prob, _, _ = eng.forward_crops(frames, [win, win], [0, 1], shape)
            torch.cuda.synchronize()
            results.append(prob.cpu())
            logs.append(capfd.readouterr().err)
        assert "[u2 tune]" in logs[0] and "[u2 tune]" in logs[1]
        assert "[u2 tune]" not in logs[2]
        assert torch.equal(results[0], results[2])                     # same choices, same bits
    finally:
        eng.close()


def test_bf16_clip_is_close(clip):
    st = clip["st"]
    eng = U2NetEngine("p", "bf16", 0, state=st)
    try:
        frames = torch.from_numpy(clip["frames"][:8]).cuda()
        geo = [crop_window(b, H, W) for b in clip["boxes"][:8]]
        errs = []
        for shape, idx in clip_chunks([g[1] for g in geo], 16):
            prob, _, _ = eng.forward_crops(frames, [geo[i][0] for i in idx], idx, shape)
            for j, i in enumerate(idx):
                errs.append(float(np.abs(prob[j].cpu().numpy() - clip["oracle"][i][1]).mean()))
        print("bf16 mean |prob - oracle| per crop:", errs)
        assert max(errs) < 3e-2
        res = unet_predict_clip(eng, frames, clip["boxes"][:8])
        assert all(m.shape == clip["res"][i][0].shape for i, (m, _) in enumerate(res))
    finally:
        eng.close()


def test_engine_refuses_bad_windows(clip):
    eng = clip["eng"]
    frames = torch.from_numpy(clip["frames"][:2]).cuda()
    from yolo_puncture_amd.engine import YolopError
    for win, idx, shape in (([(0, 0, 400, 380)], [0], (380, 380)),         # wider than the crop
                            ([(1000, 0, 1281, 380)], [0], (380, 380)),     # leaves the frame
                            ([(0, 0, 380, 380)], [2], (380, 380)),         # no such frame
                            ([(0, 0, 380, 380)] * 30, [0] * 30, (380, 380))):   # above the 32-bit offset guard
        with pytest.raises(YolopError):
            eng.forward_crops(frames, win, idx, shape)
    with pytest.raises(YolopError):
        eng.forward_crops(frames, [(0, 0, 380, 380)] * 2, [1, 1], (380, 380), frame_mask=True)
