"""The fp32 streaming attention kernel for 36/72 heads (csrc/attention_stream_wide_f32.hip): alone through yp_debug_attention_f32 under
switch value 3 on the cases of attention_f32_wide_cases.py - inside the fp32 contract of attention_ref.py (at most twice the error of
torch's own float32 expression against the fp64 reference; no figure of it comes from a kernel) -, independent of the workgroup split, the
batch and the slices it reads and writes, fed zeros (not what lies behind the tensor or the row) for the keys past N and the dead output
columns; and inside a graph, past the generic kernel's 2364 tokens in a whole fp32 YOLOv10-M engine and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as A
import attention_f32_wide_cases as W
from helpers import assert_within_noise_floor, make_case, rand_image

pytestmark = pytest.mark.gpu

I32 = torch.int32
KD, HD = W.KD, W.HD
SENTINEL = 0x5A5B5C5D


def _launch(qkv, nh=2, kd=KD, hd=HD, f32="stream_wide", **kw):
    from yolo_puncture_amd.engine import attention_f32
    out, kernel = attention_f32(qkv if qkv.is_cuda else qkv.cuda(), nh, kd, hd, f32=f32, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kernel


@pytest.mark.parametrize("case", W.CASES, ids=A.case_id)
def test_wide_stream_contract(case):
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd)
    assert kernel == W.STREAM_WIDE_F32, f"kernel {kernel}"
    assert bool(torch.isfinite(got).all())
    assert_within_noise_floor(f"fp32 wide stream {A.case_id(case)}", got, o32, o64, A.F32_TARGET)


def test_kernel_selection_at_the_switch_over():
    qkv = A.f32_case(2, 400, 2, KD, HD, "peaked")[0]
    on, k_on = _launch(qkv)
    off, k_off = _launch(qkv, f32="generic")
    assert k_on == W.GENERIC and k_off == W.GENERIC, "up to 400 tokens the generic kernel keeps the call, switch or not"
    assert torch.equal(on.view(I32), off.view(I32))
    qkv = A.f32_case(2, 401, 2, KD, HD, "peaked")[0]
    assert _launch(qkv)[1] == W.STREAM_WIDE_F32 and _launch(qkv, f32="generic")[1] == W.GENERIC
    assert _launch(qkv, f32="stream")[1] == W.GENERIC, "value 1 is the 32/64 kernel's alone"


def test_32_64_heads_under_3_are_what_they_are_under_1():
    qkv = A.f32_case(2, 513, 2, 32, 64, "peaked")[0]
    wide, k_wide = _launch(qkv, 2, 32, 64, f32="stream_wide")
    one, k_one = _launch(qkv, 2, 32, 64, f32="stream")
    assert k_wide == W.STREAM_F32 and k_one == W.STREAM_F32
    assert torch.equal(wide.view(I32), one.view(I32))


def test_split_batch_and_repeat_do_not_change_the_bits():
    B, N, nh = 3, 1025, 2
    qkv = A.make_qkv("peaked", B, N, nh, KD, HD, torch.float32)[0]
    base, kernel = _launch(qkv)                                      # one query group per workgroup
    assert kernel == W.STREAM_WIDE_F32 and W.groups_per_workgroup(B, N, nh) == (17, 1)
    again, _ = _launch(qkv)
    assert torch.equal(base.view(I32), again.view(I32)), "two launches are bit-equal"
    for wgs in (1, 8, 256):                                          # runs of 17, 9 and 1 groups
        got, kernel = _launch(qkv, wgs=wgs)
        assert kernel == W.STREAM_WIDE_F32 and torch.equal(got.view(I32), base.view(I32)), wgs
    assert [W.groups_per_workgroup(B, N, nh, w)[1] for w in (1, 8, 256)] == [17, 9, 1]
    for b in range(B):
        one, kernel = _launch(qkv[b:b + 1].contiguous())
        assert kernel == W.STREAM_WIDE_F32 and torch.equal(one.view(I32), base[b:b + 1].view(I32)), f"image {b} alone differs from image {b} of the batch"


def test_slices_leave_their_surroundings_alone():
    B, N, nh, kd, hd, dist = case = (2, 513, 2, KD, HD, "peaked")
    qkv, o32, o64 = A.f32_case(*case)
    q_stride, q_coff, o_stride, o_coff = nh * 144 + 24, 8, nh * 72 + 16, 12
    wide = A.embed(qkv, q_stride, q_coff, float("nan"))
    out = torch.full((B, N, o_stride), SENTINEL, dtype=I32).view(torch.float32).cuda()
    got_wide, kernel = _launch(wide, q_coff=q_coff, out=out, o_coff=o_coff)
    assert kernel == W.STREAM_WIDE_F32
    got = got_wide[..., o_coff:o_coff + nh * hd]
    outside = torch.ones(o_stride, dtype=torch.bool)
    outside[o_coff:o_coff + nh * hd] = False
    assert bool((got_wide.view(I32)[..., outside] == SENTINEL).all()), "a store left the output slice"
    assert bool(torch.isfinite(got).all()), "a NaN outside the qkv slice was read into the result"
    assert_within_noise_floor(f"fp32 wide stream slice {A.case_id(case)}", got, o32, o64, A.F32_TARGET)
    compact, _ = _launch(qkv)
    assert torch.equal(compact.view(I32), got.contiguous().view(I32)), "the slice changes addresses only"


def test_ragged_key_block_is_fed_zeros():
    """N = 513 leaves 63 absent keys in the last block of either image; behind the tensor the allocation holds NaN (0 x NaN = NaN)"""
    B, N, nh, kd, hd, dist = case = (2, 513, 2, KD, HD, "peaked")
    qkv, o32, o64 = A.f32_case(*case)
    n = qkv.numel()
    buf = torch.full((n + 256 * 256,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:n] = qkv.cuda().reshape(-1)
    got, kernel = _launch(buf[:n].view(B, N, -1))
    assert kernel == W.STREAM_WIDE_F32 and bool(torch.isfinite(got).all())
    assert_within_noise_floor(f"fp32 wide stream ragged {A.case_id(case)}", got, o32, o64, A.F32_TARGET)


def test_refusals_happen_on_the_host():
    from yolo_puncture_amd.engine import load_library
    lib = load_library()
    nh = 2
    qkv = torch.zeros((1, 2365, nh * 144 + 8), dtype=torch.float32, device="cuda")
    out = torch.full((1, 2365, nh * 72 + 8), SENTINEL, dtype=torch.int32, device="cuda")
    ok = dict(B=1, N=2365, kd=36, hd=72, on=3, q_stride=nh * 144 + 8)
    cases = [("switch 2", dict(on=2, N=401), "f32_stream"),
             ("36/72 past the LDS under the 32/64 kernel's value", dict(on=1), "2364"),
             ("36/56 past the LDS under 3", dict(hd=56), "2364"),
             ("q_stride % 4 under 3", dict(q_stride=nh * 144 + 6), "multiples of 4"),
             ("qkv of 2^31 bytes under 3", dict(B=1 + (1 << 31) // (2365 * (nh * 144 + 8) * 4)), "2^31 bytes")]
    for what, change, msg in cases:
        a = dict(ok)
        a.update(change)
        k = C.c_int(-7)
        rc = lib.yp_debug_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), a["B"], a["N"], nh, a["kd"], a["hd"], a["q_stride"], 0,
                                        nh * 72 + 8, 0, 0, a["on"], C.byref(k), None)
        err = lib.yp_last_error().decode()
        assert rc < 0 and msg in err, (what, rc, err)
        assert k.value == -7, (what, "kernel_out was written")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"


# ---- inside a graph -------------------------------------------------------------------------------------------------------------------
def test_m_engine_past_the_generic_limit():
    """1760 x 1408 (2420 tokens) is refused without the switch; with it the engine's own attention output against attention_ref.reference of
    its own qkv holds the fp32 contract and hipGraph replay equals eager, bit for bit, on every output"""
    from yolo_puncture_amd.engine import Engine, YolopError
    shape = (1, 1408, 1760)
    N = (shape[1] // 32) * (shape[2] // 32)
    st, im = make_case("m", 80, False, 0, shape)
    imc = im.cuda()
    eng = Engine("m", 80, False, "fp32", 0, state=st)
    try:
        eng.set_autotune(False)
        with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364 \(a streaming form is not built\)"):
            eng.plan(*shape)
        eng.set_attention_f32("stream_wide")
        ref = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
        torch.cuda.synchronize()
        op = [o for o in eng.plan(*shape) if o["name"].endswith(".attn.o")][0]
        assert op["kernel"] == "attention_stream_wide_f32_kernel"
        qkv = eng.read_tensor(eng.find_tensor(op["name"][:-2] + ".qkv")).reshape(1, N, -1).float()
        o = eng.read_tensor(op["out"][0]).reshape(1, N, -1)[..., op["out"][1]:op["out"][1] + op["out"][2]].float()
        nh = op["out"][2] // HD
        assert nh == 4 and qkv.shape[2] == nh * (2 * KD + HD)
        o64 = A.reference(qkv, nh, KD, HD, 0, "fp32")[0]
        o32 = A.oracle_expression(qkv, nh, KD, HD, torch.float32)
        assert_within_noise_floor(f"v10-m fp32 .attn.o at {shape}", o, o32, o64, A.F32_TARGET)
        eng.set_graph(True)
        for _ in range(2):
            out = eng.forward(imc)
            torch.cuda.synchronize()
            for k in ref:
                assert torch.equal(out[k], ref[k]), k
    finally:
        eng.close()


def test_facade_predicts_at_imgsz_1760():
    from yolo_puncture_amd import hostops
    from yolo_puncture_amd.engine import YolopError
    from yolo_puncture_amd.predictor import YOLO
    from yolo_puncture_amd import predictor
    frame = rand_image((1, 1408, 1760, 3), seed=11)[0].numpy()
    boxed = hostops.letterbox(frame, 1760)[0]
    assert boxed.shape == (1408, 1760, 3)
    cached = set(predictor._ENGINE_CACHE)
    try:
        default = YOLO("synthetic:m", dtype="fp32")
        with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364 \(a streaming form is not built\)"):
            default.predict(frame, imgsz=1760)
        model = YOLO("synthetic:m", dtype="fp32", attention_f32="stream_wide")
        eng = model._engine()
        assert eng is not default._engine(), "the switch is part of the engine-cache key"
        eng.set_autotune(False)
        conf = 0.25
        r = model.predict(frame, conf=conf, imgsz=1760)[0]
        b = r.boxes.cpu().numpy()
        assert [o["kernel"] for o in eng.plan(1, 1408, 1760) if o["name"].endswith(".attn.o")] == ["attention_stream_wide_f32_kernel"]
        det = eng.forward(torch.from_numpy(boxed[None]).cuda())["det"][0].cpu()
        det = det[det[:, 4] > conf]
        assert det.shape[0] == len(b.cls)
        want = hostops.scale_boxes_t((1408, 1760), det[:, :4].clone(), (1408, 1760))
        assert np.array_equal(b.xyxy, want.numpy()) and np.array_equal(b.conf, det[:, 4].numpy())
    finally:                                 # the two v10-M engines (arenas, a captured graph) do not stay behind in the process
        torch.cuda.synchronize()
        for key in set(predictor._ENGINE_CACHE) - cached:
            predictor._ENGINE_CACHE.pop(key).close()
