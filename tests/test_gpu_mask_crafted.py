"""The segmentation tail (csrc/mask.hip) on crafted inputs (tests/mask_cases.py): byte equality with the oracle where the reference is exact,
a derived per-pixel allowance on random data, the area / suppression / paint decisions on their thresholds, the clip writers at odd byte
offsets, and the scalar GEMM against the matrix-core one.

A real engine per numeric mode is built from plain synthetic weights and run once at the rig's shape (that allocates its plan and its
prototype tensor); the crafted prototypes are written over `.proto.cv3` (Engine.write_tensor - bf16 in the bf16 engine), read back and
compared with what was meant, and the mask entry points are called on them as `predict` calls them. tests/test_mask_cases_host.py proves on
the CPU that every case does what its name says and that every exact case is exact."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":                                 # (the child of test_scalar_gemm_gives_the_same_bytes)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_cases as K

pytestmark = pytest.mark.gpu

_RIGS = {}
SENTINEL = 0xA5


class _Rig:
    """one engine whose prototypes are ours"""

    def __init__(self, dtype):
        from yolo_puncture_amd.engine import Engine
        from yolo_puncture_amd.weights import synthetic_state
        self.dtype = dtype
        self.eng = Engine("n", 80, True, dtype, 0, max_det=K.CLIP_MAX_DET, state=synthetic_state("n", 80, True, seed=0))
        self.eng.set_autotune(False)
        self.rig = self.tag = self.protos = None

    def use(self, rig, tag, protos):
        """forward at the rig's shape if the engine is at another; write `protos` [B,Hp,Wp,32] if the tensor holds something else.
        -> what the kernel sees (the read-back values)"""
        eng = self.eng
        if self.rig != rig:
            B, H, W = K.RIGS[rig]
            eng.forward(torch.zeros((B, H, W, 3), dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            self.rig, self.tag = rig, None
        if self.tag != tag:
            ti = [t for t in eng.tensors() if t["name"].endswith(".proto.cv3")]
            assert len(ti) == 1 and tuple(ti[0]["shape"]) == tuple(protos.shape), (ti, protos.shape)
            assert ti[0]["f32"] == (self.dtype == "fp32")
            eng.write_tensor(ti[0]["index"], 0, protos)
            back = eng.read_tensor(ti[0]["index"])
            assert torch.equal(back, K.to_storage(protos, self.dtype)), "the prototypes did not arrive as written"
            self.tag, self.protos = tag, back
        return self.protos


def _rig(dtype):
    if dtype not in _RIGS:
        _RIGS[dtype] = _Rig(dtype)
    return _RIGS[dtype]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RIGS.values():
        r.eng.close()
    _RIGS.clear()


def _masks(rig, b, coeff, boxes, hw, retina, **kw):
    m, ids, kept = rig.eng.masks(b, coeff.cuda(), boxes.cuda(), hw, retina=retina, **kw)
    torch.cuda.synchronize()
    return m.cpu(), (None if ids is None else ids.cpu()), (None if kept is None else kept.cpu())


def _where(got, want):
    d = torch.nonzero(got != want)
    return f"{d.shape[0]} bytes differ, first at (mask, y, x) = {d[0].tolist() if d.shape[0] else None}"


# ---- 1. exact cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.EXACT_CASES, ids=K.exact_id)
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_exact_case(dtype, c):
    rig = _rig(dtype)
    seen = rig.use(c.rig, "int", K.int_protos(c.rig))
    assert torch.equal(seen, K.int_protos(c.rig))          # bf16 storage keeps these integers: one reference serves both engines
    coeff, boxes = K.exact_inputs(c)
    m, _, _ = _masks(rig, c.b, coeff, boxes, c.hw, c.retina)
    want = K.exact_reference(c)
    assert m.dtype == torch.uint8 and m.shape == want.shape
    assert torch.equal(m, want), _where(m, want)


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_exact_case_at_the_mask_limit(dtype):
    """n = YP_MAX_MASKS = 480: exactly the 60 KiB of coefficients launch_masks admits, 30 accumulator blocks, with the id paint"""
    c = K.BIG_CASE
    rig = _rig(dtype)
    rig.use(c.rig, "int", K.int_protos(c.rig))
    coeff, boxes = K.exact_inputs(c)
    m, ids, kept = _masks(rig, c.b, coeff, boxes, c.hw, c.retina, want_ids=True, suppress_small=True, min_area=100)
    want = K.exact_reference(c)
    assert torch.equal(m, want), _where(m, want)
    wids, wkept = K.paint_reference(want, c.hw, 1, 100)
    assert 0 < int((wkept == 0).sum()) < c.n
    assert torch.equal(ids, wids) and torch.equal(kept, wkept)


def _raw_call(rig, fn, n, hw, out_hw=None):
    """yp_masks / yp_id_mask_resized on sentinel-filled outputs -> (return code, the three buffers)"""
    eng = rig.eng
    oh, ow = hw
    coeff = torch.ones((max(n, 1), 32), device="cuda")
    boxes = torch.tensor([[0.0, 0.0, ow, oh]], device="cuda").repeat(max(n, 1), 1)
    masks = torch.full((max(n, 1) * oh * ow,), SENTINEL, dtype=torch.uint8, device="cuda")
    rh, rw = out_hw or hw
    ids = torch.full((rh, rw), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    if fn == "yp_masks":
        rc = eng.lib.yp_masks(eng._h, 0, p(coeff), p(boxes), n, oh, ow, 1, p(masks), p(ids), p(kept), 0, 100, st)
    else:
        rc = eng.lib.yp_id_mask_resized(eng._h, 0, p(coeff), p(boxes), n, oh, ow, rh, rw, p(ids), p(kept), 0, 100, st)
    torch.cuda.synchronize()
    return rc, masks.cpu(), ids.cpu(), kept.cpu()


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_more_masks_than_the_limit_are_refused(dtype):
    rig = _rig(dtype)
    rig.use("A", "int", K.int_protos("A"))
    for fn, out_hw in (("yp_masks", None), ("yp_id_mask_resized", (144, 240))):
        rc, masks, ids, kept = _raw_call(rig, fn, K.YP_MAX_MASKS + 1, (96, 160), out_hw)
        assert rc < 0 and b"480" in rig.eng.lib.yp_last_error(), (fn, rc)
        assert bool((masks == SENTINEL).all()) and bool((ids == -7).all()) and bool((kept == -7).all()), f"{fn} wrote something"


# ---- 2. area, suppression, paint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.PAINT_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_paint_case(dtype, c):
    rig = _rig(dtype)
    rig.use("A", "rect", K.rect_protos("A"))
    coeff, boxes = K.rect_inputs(c.rows)
    want = K.rect_masks(c.rows, K.PAINT_HW)
    wids, wkept = K.paint_reference(want, K.PAINT_HW, c.suppress, c.min_area)
    assert wkept.tolist() == c.kept
    for b in (0, 1):
        m, ids, kept = _masks(rig, b, coeff, boxes, K.PAINT_HW, True, want_ids=True, suppress_small=bool(c.suppress), min_area=c.min_area)
        assert torch.equal(m, want), _where(m, want)
        assert torch.equal(ids, wids) and torch.equal(kept, wkept), (kept.tolist(), c.kept)


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_no_masks_still_writes_the_id_image(dtype):
    rig = _rig(dtype)
    rig.use("A", "rect", K.rect_protos("A"))
    rc, masks, ids, kept = _raw_call(rig, "yp_masks", 0, (96, 160))
    assert rc == 0 and int(ids.abs().sum()) == 0, "n = 0: ids must be WRITTEN as zeros"
    assert bool((masks == SENTINEL).all()) and bool((kept == -7).all())
    rc, _, ids, _ = _raw_call(rig, "yp_id_mask_resized", 0, (96, 160), (144, 240))
    assert rc == 0 and int(ids.abs().sum()) == 0


@pytest.mark.parametrize("c", K.RESIZE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_resize_case(dtype, c):
    rig = _rig(dtype)
    rig.use("A", "rect", K.rect_protos("A"))
    coeff, boxes = K.rect_inputs(c.rows)
    want = K.rect_masks(c.rows, c.mask_hw)
    m, _, _ = _masks(rig, 1, coeff, boxes, c.mask_hw, True)
    assert torch.equal(m, want), _where(m, want)
    for suppress in (1, 0):
        wids, wkept = K.paint_reference(want, c.out_hw, suppress, c.min_area)
        ids, kept = rig.eng.id_mask_resized(1, coeff.cuda(), boxes.cuda(), c.mask_hw, c.out_hw, suppress_small=bool(suppress), min_area=c.min_area)
        assert torch.equal(ids.cpu(), wids), int((ids.cpu() != wids).sum())
        assert torch.equal(kept.cpu(), wkept)


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_resize_edges(dtype):
    """(rh, rw) == (oh, ow) is yp_masks with ids; a ratio beyond 16 is refused with nothing written"""
    from yolo_puncture_amd.engine import YolopError
    rig = _rig(dtype)
    rig.use("A", "rect", K.rect_protos("A"))
    c = K.RESIZE_CASES[0]
    coeff, boxes = K.rect_inputs(c.rows)
    _, ids0, kept0 = _masks(rig, 0, coeff, boxes, c.mask_hw, True, want_ids=True, suppress_small=True, min_area=500)
    ids, kept = rig.eng.id_mask_resized(0, coeff.cuda(), boxes.cuda(), c.mask_hw, c.mask_hw, suppress_small=True, min_area=500)
    assert torch.equal(ids.cpu(), ids0) and torch.equal(kept.cpu(), kept0) and 0 < int((kept0 > 0).sum()) < len(c.rows)
    rc, _, ids, kept = _raw_call(rig, "yp_id_mask_resized", 3, (96, 160), (5, 10))
    assert rc < 0 and bool((ids == -7).all()) and bool((kept == -7).all())
    with pytest.raises(YolopError, match="16x"):
        rig.eng.id_mask_resized(0, coeff.cuda(), boxes.cuda(), (96, 160), (5, 10))


# ---- 3. clip forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", list(K.CLIP_FRAMES))
@pytest.mark.parametrize("hw,retina", K.CLIP_SIZES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else ("retina" if v else "input"))
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_clip_case(dtype, hw, retina, k):
    rig = _rig(dtype)
    rig.use(K.CLIP_RIG, "int", K.int_protos(K.CLIP_RIG))
    fidx, coeff, boxes = K.clip_inputs(hw, retina, k)
    want = K.clip_reference(hw, retina, k)
    coeff_d, boxes_d = coeff.cuda(), boxes.cuda()
    nbytes = k * hw[0] * hw[1]
    for off in K.CLIP_OFFSETS:
        buf = torch.full((nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + nbytes].view(k, hw[0], hw[1])
        assert view.data_ptr() % 16 == off
        rig.eng.masks_frames(fidx, coeff_d, boxes_d, hw, out=view, retina=retina)
        torch.cuda.synchronize()
        host = buf.cpu()
        got = host[off:off + nbytes].view(k, hw[0], hw[1])
        assert torch.equal(got, want), (off, _where(got, want))
        assert bool((host[:off] == SENTINEL).all()) and bool((host[off + nbytes:] == SENTINEL).all()), f"offset {off}: bytes beside the view were written"


# ---- 5. random data ----------------------------------------------------------------------------------------------------------------------
def _random_run(rig, c):
    seen = rig.use(c.rig, f"rand{c.seed}", K.rand_protos(c.rig, c.seed))
    coeff, boxes = K.random_inputs(c)
    m, _, _ = _masks(rig, c.b, coeff, boxes, c.hw, c.retina)
    return m, seen


@pytest.mark.parametrize("c", K.RANDOM_CASES, ids=K.random_id)
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_random_case(dtype, c):
    rig = _rig(dtype)
    m, seen = _random_run(rig, c)
    ref, A, inbox = K.random_case_reference(c, dtype)       # (on the values rig.use has just compared with the tensor's)
    exempt, _ = K.check_rule(f"{K.random_id(c)} {dtype}", m, ref, A)
    assert exempt <= K.EXEMPT_CAP * int(inbox.sum())


# ---- 4. scalar GEMM ------------------------------------------------------------------------------------------------------------------------
def _digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def _valu_digests():
    """{case id: sha256 of the mask bytes} over the subset both processes run (the GEMM's float result stays in the engine's workspace: no
    entry point returns it, so the masks are what is hashed)"""
    out = {}
    for dtype in K.DTYPES:
        rig = _rig(dtype)
        for c in K.VALU_EXACT:
            rig.use(c.rig, "int", K.int_protos(c.rig))
            coeff, boxes = K.exact_inputs(c)
            m, _, _ = _masks(rig, c.b, coeff, boxes, c.hw, c.retina)
            out[f"exact {K.exact_id(c)} {dtype}"] = _digest(m)
        m, _ = _random_run(rig, K.VALU_RANDOM)
        K.check_rule(f"{K.random_id(K.VALU_RANDOM)} {dtype}", m, *K.random_case_reference(K.VALU_RANDOM, dtype)[:2])
        out[f"random {K.random_id(K.VALU_RANDOM)} {dtype}"] = _digest(m)
    return out


def test_scalar_gemm_gives_the_same_bytes():
    """YOLOP_MASK_VALU=1 (read once per process, hence the child): mask_gemm_kernel instead of mask_gemm_mfma_kernel. Its masks equal the
    reference on the exact cases and the matrix-core GEMM's on all of them, the random case included."""
    assert os.environ.get("YOLOP_MASK_VALU", "0")[:1] != "1", "the parent must run the matrix-core GEMM"
    env = dict(os.environ, YOLOP_MASK_VALU="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "valu"], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-3000:])
    assert r.returncode == 0 and "valu ok" in r.stdout
    child = dict(line[len("DIGEST "):].rsplit(" ", 1) for line in r.stdout.splitlines() if line.startswith("DIGEST "))
    mine = _valu_digests()
    assert set(child) == set(mine) and len(mine) == 2 * (len(K.VALU_EXACT) + 1)
    for name, d in mine.items():
        assert child[name] == d, f"{name}: the scalar and the matrix-core GEMM give different masks"
    for dtype in K.DTYPES:
        for c in K.VALU_EXACT:
            assert child[f"exact {K.exact_id(c)} {dtype}"] == _digest(K.exact_reference(c)), (K.exact_id(c), dtype)


if __name__ == "__main__" and sys.argv[1:] == ["valu"]:
    assert os.environ.get("YOLOP_MASK_VALU") == "1"
    for name_, d_ in _valu_digests().items():
        print(f"DIGEST {name_} {d_}")
    for r_ in _RIGS.values():
        r_.eng.close()
    print("valu ok")
