"""yp_overlay_frames / overlay_clip / render_clip on the GPU, byte-exact against hostops.overlay_frame (integer data: no tolerance). The
shapes are the smallest at which the vector path can go wrong (overlay_cases.SHAPES); each runs the copy form and the in-place form."""
import numpy as np
import pytest
import torch

from overlay_cases import SHAPES, VARIANTS, make_case, reference, region_mask
from yolo_puncture_amd import hostops
from yolo_puncture_amd.overlay import overlay_clip, render_clip, render_labels
from yolo_puncture_amd.u2net import U2NetEngine, synthetic_state, unet_predict_clip

pytestmark = pytest.mark.gpu


def on_device(case, offset=0):
    """the case's tensors on the GPU; offset > 0 puts the frames' first byte that many bytes past an aligned address"""
    frames = torch.from_numpy(case["frames"])
    if offset:
        buf = torch.empty(frames.numel() + offset, dtype=torch.uint8, device="cuda")
        dev = buf[offset:].view(frames.shape)
        dev.copy_(frames)
    else:
        dev = frames.cuda()
    return dev, torch.from_numpy(case["masks"]).cuda(), torch.from_numpy(case["labels"]).cuda()


def run_both(case, frames, masks, labels, out=None):
    kw = dict(crop_index=case["crop_index"], color=case["col"])
    before = frames.clone()
    copied = overlay_clip(frames, masks, case["windows"], case["rois"], labels, case["label_xy"], out=out, **kw)
    assert torch.equal(frames, before)                          # the copy form leaves its source alone
    offset = frames.data_ptr() % 16                             # the in-place run gets the alignment of the frames
    work = torch.empty(frames.numel() + offset, dtype=torch.uint8, device="cuda")[offset:].view(frames.shape)
    work.copy_(frames)
    same = overlay_clip(work, masks, case["windows"], case["rois"], labels, case["label_xy"], inplace=True, **kw)
    assert same.data_ptr() == work.data_ptr()
    torch.cuda.synchronize()
    return copied.cpu().numpy(), work.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", range(VARIANTS))
def test_both_forms_equal_overlay_frame(shape, variant):
    case = make_case(*shape, variant)
    want = reference(case, hostops.overlay_frame)
    copied, inplace = run_both(case, *on_device(case))
    assert np.array_equal(copied, want)
    assert np.array_equal(inplace, want)
    assert np.array_equal(copied, inplace)
    outside = ~region_mask(case)
    assert np.array_equal(inplace[outside], case["frames"][outside])       # nothing outside the regions changed
    assert (want != case["frames"]).any()


@pytest.mark.parametrize("offset,out_offset", [(1, 1), (7, 7), (0, 5)])
def test_misaligned_base(offset, out_offset):
    """frames whose first byte is not 16-byte aligned; with another alignment for out, the copy form has no aligned pair and goes bytewise"""
    case = make_case(*SHAPES[0], 1)
    want = reference(case, hostops.overlay_frame)
    frames, masks, labels = on_device(case, offset)
    assert frames.data_ptr() % 16 == offset
    buf = torch.zeros(frames.numel() + 32, dtype=torch.uint8, device="cuda")
    out = buf[out_offset:out_offset + frames.numel()].view(frames.shape)
    copied, inplace = run_both(case, frames, masks, labels, out=out)
    assert np.array_equal(copied, want) and np.array_equal(inplace, want)
    rest = buf.cpu().numpy()
    assert not rest[:out_offset].any() and not rest[out_offset + frames.numel():].any()     # not a byte around out was written


def test_full_frame_mask_and_no_mask():
    case = make_case(*SHAPES[0], 2)
    N, H, W = SHAPES[0]
    full = np.random.default_rng(3).integers(0, 256, (N, H, W), dtype=np.uint8)
    frames, _, labels = on_device(case)
    got = overlay_clip(frames, torch.from_numpy(full).cuda(), None, case["rois"], labels, case["label_xy"]).cpu().numpy()
    bare = overlay_clip(frames, None, None, case["rois"]).cpu().numpy()
    for n in range(N):
        lx, ly, lw, lh = (int(v) for v in case["label_xy"][n])
        label = case["labels"][n][:lh, :lw] if lw and lh else None
        assert np.array_equal(got[n], hostops.overlay_frame(case["frames"][n], full[n], (0, 0, W, H), case["rois"][n], label, (lx, ly)))
        assert np.array_equal(bare[n], hostops.overlay_frame(case["frames"][n], None, (0, 0, 0, 0), case["rois"][n]))


def test_frame_offsets_past_2_31():
    """360 frames of 1080 x 1920: the last frame starts 2.2 GB into the tensor. In place, so only the regions are touched."""
    N, H, W = 360, 1080, 1920
    frames = torch.full((N, H, W, 3), 100, dtype=torch.uint8, device="cuda")
    crop = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1, 380, 380), dtype=np.uint8)).cuda()
    windows = np.tile(np.array([[700, 300, 1080, 680]], np.int32), (N, 1))
    rois = np.tile(np.array([[650, 250, 1130, 730]], np.int32), (N, 1))
    overlay_clip(frames, crop, windows, rois, crop_index=np.zeros(N, np.int32), inplace=True)
    want = hostops.overlay_frame(np.full((H, W, 3), 100, np.uint8), crop[0].cpu().numpy(), windows[0], rois[0])
    for n in (0, N - 1):
        assert np.array_equal(frames[n].cpu().numpy(), want), n
    assert int(frames[N // 2].to(torch.int64).sum()) == int(want.astype(np.int64).sum())


def test_engine_refuses_what_the_abi_refuses():
    from yolo_puncture_amd.engine import YolopError
    case = make_case(*SHAPES[1], 0)
    frames, masks, labels = on_device(case)
    bad = case["windows"].copy()
    bad[0] = (0, 0, 17, 4)
    with pytest.raises(YolopError):
        overlay_clip(frames, masks, bad, case["rois"])
    with pytest.raises(YolopError):
        overlay_clip(frames, masks, case["windows"], case["rois"], crop_index=[0, 3])
    with pytest.raises(ValueError):
        overlay_clip(frames, masks, case["windows"], case["rois"], out=frames)


# ---- render_clip: 1080 x 1920 frames through the network and the overlay --------------------------------------------------------------
H, W = 1080, 1920
BOXES = [(900, 500, 960, 560), (40, 500, 100, 560), (1850, 1000, 1910, 1060), (1000, 300, 1080, 380), (700, 700, 760, 760)]
ROIS = [(840, 440, 1020, 620), (0, 440, 160, 620), (1790, 940, 1920, 1080), (0, 0, 1920, 1080), (640, 0, 820, 820)]
TEXTS = ["0 0 0.98 30.00 17.50", "1 1 0.75 28.40 -", "", "3 0 0.60 30.00 12.00", "4 1 0.99 2.50mm/s"]


@pytest.fixture(scope="module")
def rendered():
    import os
    old = os.environ.get("YOLOP_U2_SMALL_MAX")
    os.environ["YOLOP_U2_SMALL_MAX"] = "0"          # one conv kernel for every layer: the masks do not depend on the chunk size
    try:
        eng = U2NetEngine("p", "fp32", 0, state=synthetic_state("p", 0))
    finally:
        if old is None:
            del os.environ["YOLOP_U2_SMALL_MAX"]
        else:
            os.environ["YOLOP_U2_SMALL_MAX"] = old
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (len(BOXES), H, W, 3), dtype=np.uint8)
    bitmaps, xy = render_labels(TEXTS, ROIS)
    want = []
    for i, (mask, window) in enumerate(unet_predict_clip(eng, list(frames), BOXES, batch_size=4)):
        lx, ly, lw, lh = (int(v) for v in xy[i])
        want.append(hostops.overlay_frame(frames[i], mask, window, ROIS[i], bitmaps[i][:lh, :lw] if lw else None, (lx, ly)))
    yield dict(eng=eng, frames=frames, want=want)
    eng.close()


@pytest.mark.parametrize("batch_size", [2, 4])
@pytest.mark.parametrize("source", ["host", "device"])
def test_render_clip(rendered, batch_size, source):
    frames = list(rendered["frames"]) if source == "host" else torch.from_numpy(rendered["frames"]).cuda()
    order = []
    for i, image in render_clip(rendered["eng"], frames, BOXES, ROIS, TEXTS, batch_size=batch_size, to_host=True):
        assert isinstance(image, np.ndarray) and image.shape == (H, W, 3)
        assert np.array_equal(image, rendered["want"][i]), f"frame {i}"
        order.append(i)
    assert order == list(range(len(BOXES)))
    out = render_clip(rendered["eng"], frames, BOXES, ROIS, TEXTS, batch_size=batch_size, to_host=False)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (len(BOXES), H, W, 3)
    out = out.cpu().numpy()
    for i in range(len(BOXES)):
        assert np.array_equal(out[i], rendered["want"][i]), f"frame {i}"
    if source == "device":
        assert np.array_equal(frames.cpu().numpy(), rendered["frames"])      # the caller's frames are left as they are
