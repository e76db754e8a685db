"""Host side of the U^2-Net-P clip path (no GPU): crop_window against a restatement of the reference's crop_frame, the chunk planner of
unet_predict_clip, and its argument checks, which must all fire before the engine is touched."""
import numpy as np
import pytest
import torch

from yolo_puncture_amd.u2net import clip_chunks, crop_window, max_crops_per_call, unet_predict_clip


def crop_frame_np(frame, xyxy, crop_size=380, need_padding=False):
    """yolo_seg/utils/transform.py:22-50, line for line (the padding test keeps its `A and B or C` grouping)."""
    height, width, _ = frame.shape
    x1, y1, x2, y2 = xyxy
    x_center, y_center = int((x1 + x2) / 2), int((y1 + y2) / 2)
    half_size = crop_size // 2
    x1, y1 = x_center - half_size, y_center - half_size
    x2, y2 = x_center + half_size, y_center + half_size
    x1, y1 = max(0, x1), max(0, y1)
    x2, y2 = min(width, x2), min(height, y2)
    cropped_image = frame[y1:y2, x1:x2]
    if need_padding and cropped_image.shape[0] < crop_size or cropped_image.shape[1] < crop_size:
        padded_image = np.zeros((crop_size, crop_size, 3), dtype=np.uint8)
        padded_image[:cropped_image.shape[0], :cropped_image.shape[1]] = cropped_image
        cropped_image = padded_image
    return cropped_image, (x1, y1, x2, y2)


def apply_window(frame, window, shape):
    """What the device crop kernel reads: the window at the top-left of a zero image of the crop shape."""
    x1, y1, x2, y2 = window
    out = np.zeros(shape + (3,), dtype=np.uint8)
    out[:y2 - y1, :x2 - x1] = frame[y1:y2, x1:x2]
    return out


H, W = 720, 1280
CASES = {
    "interior": (600, 300, 700, 420),
    "left": (10, 300, 90, 400),
    "right": (1200, 300, 1279, 400),
    "top": (600, 0, 700, 60),
    "bottom": (600, 680, 700, 719),
    "top_left": (0, 0, 40, 40),
    "top_right": (1250, 5, 1280, 50),
    "bottom_left": (3, 700, 50, 720),
    "bottom_right": (1200, 650, 1280, 720),
    "fallback": (0, 0, W, H),
    "odd_centre": (601, 301, 702, 418),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_crop_window_matches_crop_frame(name):
    rng = np.random.RandomState(len(name))
    frame = rng.randint(0, 256, (H, W, 3), dtype=np.uint8)
    box = CASES[name]
    want, want_coords = crop_frame_np(frame, box)
    window, shape = crop_window(box, H, W)
    assert window == want_coords
    assert shape == want.shape[:2]
    assert np.array_equal(apply_window(frame, window, shape), want)


def test_crop_window_short_and_narrow_frames():
    rng = np.random.RandomState(1)
    narrow = rng.randint(0, 256, (500, 300, 3), dtype=np.uint8)        # narrower than 380: always padded to 380 x 380
    short = rng.randint(0, 256, (250, 640, 3), dtype=np.uint8)         # shorter than 380, wide: an unpadded 250 x 380 crop
    for frame, box, shape in ((narrow, (100, 200, 180, 260), (380, 380)), (short, (300, 50, 360, 200), (250, 380)),
                              (short, (0, 0, 640, 250), (250, 380)), (short, (600, 100, 640, 150), (380, 380))):
        want, coords = crop_frame_np(frame, box)
        window, got_shape = crop_window(box, frame.shape[0], frame.shape[1])
        assert window == coords and got_shape == shape == want.shape[:2]
        assert np.array_equal(apply_window(frame, window, got_shape), want)


def test_crop_window_other_crop_size_and_numpy_ints():
    frame = np.random.RandomState(2).randint(0, 256, (400, 500, 3), dtype=np.uint8)
    box = tuple(np.int64(v) for v in (10, 10, 200, 90))
    for cs in (160, 161, 380):
        want, coords = crop_frame_np(frame, box, crop_size=cs)
        window, shape = crop_window(box, 400, 500, crop_size=cs)
        assert window == coords and shape == want.shape[:2]
        assert np.array_equal(apply_window(frame, window, shape), want)


@pytest.mark.parametrize("batch_size", [1, 3, 5, 16, 64])
def test_chunks_restore_order_and_respect_the_guard(batch_size):
    rng = np.random.RandomState(batch_size)
    pool = [(380, 380), (250, 380), (380, 380), (190, 380), (32, 4000)]
    shapes = [pool[i] for i in rng.randint(0, len(pool), 57)]
    chunks = clip_chunks(shapes, batch_size)
    seen = []
    sizes = {}
    for shape, idx in chunks:
        assert all(shapes[i] == shape for i in idx)
        n = len(idx)
        assert n & (n - 1) == 0 and 1 <= n <= batch_size                 # powers of two up to batch_size
        assert n <= max_crops_per_call(*shape)
        assert n * shape[0] * shape[1] * 128 * 4 < 2 ** 31               # the engine's 32-bit offset guard
        assert idx == sorted(idx)
        sizes.setdefault(shape, set()).add(n)
        seen += idx
    assert sorted(seen) == list(range(len(shapes)))
    for shape, s in sizes.items():
        assert len(s) <= int(np.log2(batch_size)) + 1
    # what unet_predict_clip does with the chunks: results land back at their input positions
    out = [None] * len(shapes)
    for shape, idx in chunks:
        for i in idx:
            out[i] = (i, shape)
    assert out == [(i, s) for i, s in enumerate(shapes)]


def test_chunk_cap_of_a_full_crop():
    assert max_crops_per_call(380, 380) == 29
    chunks = clip_chunks([(380, 380)] * 45, 32)
    assert [len(i) for _, i in chunks] == [16, 16, 8, 4, 1]
    with pytest.raises(ValueError):
        clip_chunks([(380, 380)], 0)


class _NoEngine:
    """Any use of the model fails the test: argument errors must be raised first."""
    def __getattr__(self, name):
        raise AssertionError(f"engine touched ({name}) before the arguments were checked")


def test_argument_errors_raise_without_a_gpu():
    m = _NoEngine()
    frames = [np.zeros((720, 1280, 3), np.uint8) for _ in range(3)]
    boxes = [(600, 300, 700, 400)] * 3
    assert unet_predict_clip(m, [], []) == []
    with pytest.raises(ValueError):
        unet_predict_clip(m, frames, boxes[:2])                         # lengths differ
    with pytest.raises(TypeError):
        unet_predict_clip(m, [f.astype(np.float32) for f in frames], boxes)
    with pytest.raises(TypeError):
        unet_predict_clip(m, [f[..., :1] for f in frames], boxes)       # one channel
    with pytest.raises(TypeError):
        unet_predict_clip(m, [f[..., 0] for f in frames], boxes)        # HW only
    with pytest.raises(ValueError):
        unet_predict_clip(m, frames[:2] + [np.zeros((480, 640, 3), np.uint8)], boxes)
    with pytest.raises(TypeError):
        unet_predict_clip(m, torch.zeros((3, 720, 1280, 3), dtype=torch.uint8), boxes)   # a host tensor, not a CUDA one
    with pytest.raises(ValueError):
        unet_predict_clip(m, frames, boxes, batch_size=0)
    with pytest.raises(ValueError):
        unet_predict_clip(m, frames, [(3000, 300, 3100, 400)] * 3)       # centre outside the frame: crop_frame's slice is empty
