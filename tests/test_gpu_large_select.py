"""Stage 1 of the top-k head alone (yp_debug_topk_anchors), on crafted class-max keys at anchor counts no input shape has (stage 2 and the
NMS heads on crafted logits of a real engine: tests/test_gpu_head_crafted.py).
The entry runs the kernels an engine takes for the anchor count: head_select_kernel<1> up to 12288 anchors (the control case here),
head_chunk_topk_kernel + head_select_large_kernel<1> beyond. Reference: torch.sort of the same unique 64-bit keys
score_bits << 32 | (0xFFFFFFFF - anchor) on the host; winners (in rank order) and the stage-1 threshold must match bit for bit, for score
patterns that defeat anything relying on how scores are distributed: mass ties, one value everywhere, winners all in the last chunk, all in
the first, spread one per 1024 anchors, packed into the last 100 anchors, fewer non-zero scores than k."""
import pytest
import torch

from yolo_puncture_amd.engine import topk_anchors

pytestmark = pytest.mark.gpu

# anchors -> the three levels. 12600 = 800x768, 25200 = 1280x960, 42840 = 1088x1920, 214200 = 3200x3264 (real level splits); 12288 (the last
# count of the LDS form) and 12289 are no multiple of 21, so no input shape has them: 96x96 + 48x48 + the rest on the third level
LEVELS = {12288: ((96, 96), (48, 48), (24, 32)), 12289: ((96, 96), (48, 48), (769, 1)), 12600: ((100, 96), (50, 48), (25, 24)),
          25200: ((160, 120), (80, 60), (40, 30)), 42840: ((136, 240), (68, 120), (34, 60)), 214200: ((400, 408), (200, 204), (100, 102))}
PATTERNS = ("uniform", "eight", "equal", "ascending", "descending", "mod1024", "last100", "sparse")


def _scores(pattern, A, k, b, g):
    """float32 scores in [0, 1] of image b"""
    a = torch.arange(A, dtype=torch.float64)
    if pattern == "uniform":
        return torch.rand(A, generator=g)
    if pattern == "eight":
        return torch.randint(0, 8, (A,), generator=g).float() / 8.0 + 0.0625
    if pattern == "equal":
        return torch.full((A,), 0.25 + 0.5 * b)
    if pattern in ("ascending", "descending"):
        up = ((a + 1.0) / (A + 1.0)).float()
        assert bool((up[1:] > up[:-1]).all())
        return up if (pattern == "ascending") == (b == 0) else up.flip(0)      # (the second image runs the other way)
    s = torch.rand(A, generator=g) * 0.5
    if pattern == "mod1024":      # every anchor = b mod 1024 above everything else (as many as A has; the rest of the k come from below)
        at = torch.arange(b, A, 1024)
        s[at] = 0.75 + 0.25 * torch.rand(at.numel(), generator=g)
    elif pattern == "last100":
        s[A - 100:] = 0.75 + 0.25 * torch.rand(100, generator=g)
    elif pattern == "sparse":     # fewer than k non-zero scores: the zero ties behind them are ordered by anchor index
        nz = torch.randperm(A, generator=g)[:k // 2]
        v = s[nz] + 0.01
        s = torch.zeros(A)
        s[nz] = v
    return s


def _reference(bits, k):
    """bits int64 [B, A] -> (anchors [B, k] by rank, threshold bits [B])"""
    A = bits.shape[1]
    keys = (bits << 32) | (0xFFFFFFFF - torch.arange(A, dtype=torch.int64))[None]      # scores are non-negative floats: keys fit int64
    top = torch.sort(keys, dim=1, descending=True).values[:, :k]
    return 0xFFFFFFFF - (top & 0xFFFFFFFF), top[:, -1] >> 32


@pytest.mark.parametrize("A", sorted(LEVELS))
def test_topk_anchors_matches_host_sort(A):
    hw = LEVELS[A]
    sizes = [h * w for h, w in hw]
    assert sum(sizes) == A
    B = 2
    g = torch.Generator().manual_seed(A)
    for pattern in PATTERNS:
        for k in (1, 300, 512):
            s = torch.stack([_scores(pattern, A, k, b, g) for b in range(B)])
            assert s.dtype == torch.float32 and float(s.min()) >= 0.0 and float(s.max()) <= 1.0
            bits32 = s.view(torch.int32)
            mk = [t.contiguous().cuda() for t in bits32.split(sizes, dim=1)]
            sel, thr = topk_anchors(mk, hw, k)
            want_sel, want_thr = _reference(bits32.long(), k)
            got_sel, got_thr = sel.cpu()[:, :k].long(), thr.cpu().long()
            assert torch.equal(got_sel, want_sel), (A, pattern, k, int((got_sel != want_sel).sum()))
            assert torch.equal(got_thr, want_thr), (A, pattern, k)


def test_topk_anchors_validates_its_arguments():
    from yolo_puncture_amd.engine import MAX_ANCHORS, YolopError
    hw = LEVELS[12600]
    mk = [torch.zeros((1, h * w), dtype=torch.int32, device="cuda") for h, w in hw]
    for k in (0, 513):
        with pytest.raises(YolopError):
            topk_anchors(mk, hw, k)
    big = ((512, 512), (128, 256), (1, 1))      # one past the bound
    assert sum(h * w for h, w in big) == MAX_ANCHORS + 1
    with pytest.raises(YolopError, match=str(MAX_ANCHORS)):
        topk_anchors([torch.zeros((1, h * w), dtype=torch.int32, device="cuda") for h, w in big], big, 300)
