"""The fp32 streaming attention kernel (csrc/attention_stream_f32.hip): alone through yp_debug_attention_f32 on the cases of
attention_f32_stream_cases.py - inside the fp32 contract of attention_ref.py (at most twice the error of torch's own float32 expression
against the fp64 reference; no figure of it comes from a kernel) -, independent of the workgroup split, the batch and the slices it reads
and writes, fed zeros (not what lies behind the tensor) for the keys past N; and inside a graph, past the generic kernel's 2368 tokens in
whole fp32 engines and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as A
import attention_f32_stream_cases as S
from helpers import assert_within_noise_floor, make_case, make_case_family, rand_image

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _launch(qkv, nh=2, kd=32, hd=64, f32="stream", **kw):
    from yolo_puncture_amd.engine import attention_f32
    out, kernel = attention_f32(qkv if qkv.is_cuda else qkv.cuda(), nh, kd, hd, f32=f32, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kernel


@pytest.mark.parametrize("case", S.CASES, ids=A.case_id)
def test_stream_contract(case):
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd)
    assert kernel == S.STREAM_F32, f"kernel {kernel}"
    assert bool(torch.isfinite(got).all())
    assert_within_noise_floor(f"fp32 stream {A.case_id(case)}", got, o32, o64, A.F32_TARGET)


def test_kernel_selection_at_the_switch_over():
    qkv = A.f32_case(2, 400, 2, 32, 64, "peaked")[0]
    on, k_on = _launch(qkv)
    off, k_off = _launch(qkv, f32="generic")
    assert k_on == S.GENERIC and k_off == S.GENERIC, "up to 400 tokens the generic kernel keeps the call, switch or not"
    assert torch.equal(on.view(I32), off.view(I32))
    qkv = A.f32_case(2, 401, 2, 32, 64, "peaked")[0]
    assert _launch(qkv)[1] == S.STREAM_F32 and _launch(qkv, f32="generic")[1] == S.GENERIC


def test_split_batch_and_repeat_do_not_change_the_bits():
    B, N, nh = 3, 1025, 2
    qkv = A.make_qkv("peaked", B, N, nh, 32, 64, torch.float32)[0]
    base, kernel = _launch(qkv)                                      # one query group per workgroup
    assert kernel == S.STREAM_F32 and S.groups_per_workgroup(B, N, nh) == (17, 1)
    again, _ = _launch(qkv)
    assert torch.equal(base.view(I32), again.view(I32)), "two launches are bit-equal"
    for wgs in (1, 8, 256):                                          # runs of 17, 9 and 1 groups
        got, kernel = _launch(qkv, wgs=wgs)
        assert kernel == S.STREAM_F32 and torch.equal(got.view(I32), base.view(I32)), wgs
    assert [S.groups_per_workgroup(B, N, nh, w)[1] for w in (1, 8, 256)] == [17, 9, 1]
    for b in range(B):
        one, kernel = _launch(qkv[b:b + 1].contiguous())
        assert kernel == S.STREAM_F32 and torch.equal(one.view(I32), base[b:b + 1].view(I32)), f"image {b} alone differs from image {b} of the batch"


def test_slices_leave_their_surroundings_alone():
    B, N, nh, kd, hd, dist = case = (2, 513, 2, 32, 64, "peaked")
    qkv, o32, o64 = A.f32_case(*case)
    sentinel = 0x5A5B5C5D
    q_stride, q_coff, o_stride, o_coff = nh * 128 + 24, 8, nh * 64 + 16, 12
    wide = A.embed(qkv, q_stride, q_coff, float("nan"))
    out = torch.full((B, N, o_stride), sentinel, dtype=I32).view(torch.float32).cuda()
    got_wide, kernel = _launch(wide, q_coff=q_coff, out=out, o_coff=o_coff)
    assert kernel == S.STREAM_F32
    got = got_wide[..., o_coff:o_coff + nh * hd]
    outside = torch.ones(o_stride, dtype=torch.bool)
    outside[o_coff:o_coff + nh * hd] = False
    assert bool((got_wide.view(I32)[..., outside] == sentinel).all()), "a store left the output slice"
    assert bool(torch.isfinite(got).all()), "a NaN outside the qkv slice was read into the result"
    assert_within_noise_floor(f"fp32 stream slice {A.case_id(case)}", got, o32, o64, A.F32_TARGET)
    compact, _ = _launch(qkv)
    assert torch.equal(compact.view(I32), got.contiguous().view(I32)), "the slice changes addresses only"


def test_ragged_key_block_is_fed_zeros():
    """N = 513 leaves 63 absent keys in the last block of either image; behind the tensor the allocation holds NaN (0 x NaN = NaN)"""
    B, N, nh, kd, hd, dist = case = (2, 513, 2, 32, 64, "peaked")
    qkv, o32, o64 = A.f32_case(*case)
    n = qkv.numel()
    buf = torch.full((n + 256 * 256,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:n] = qkv.cuda().reshape(-1)
    got, kernel = _launch(buf[:n].view(B, N, -1))
    assert kernel == S.STREAM_F32 and bool(torch.isfinite(got).all())
    assert_within_noise_floor(f"fp32 stream ragged {A.case_id(case)}", got, o32, o64, A.F32_TARGET)


def test_refusals_happen_on_the_host():
    from yolo_puncture_amd.engine import load_library
    lib = load_library()
    nh = 2
    qkv = torch.zeros((1, 2369, nh * 136 + 8), dtype=torch.float32, device="cuda")
    out = torch.full((1, 2369, nh * 64 + 8), 0x5A5B5C5D, dtype=torch.int32, device="cuda")
    ok = dict(B=1, N=2369, kd=32, hd=64, on=1, q_stride=nh * 136 + 8)
    cases = [("past the LDS with the switch off", dict(on=0), "2368"), ("kd 36 past the LDS with the switch on", dict(N=2365, kd=36, hd=56), "2364"),
             ("switch 2", dict(on=2, N=401), "f32_stream"), ("switch -1", dict(on=-1, N=401), "f32_stream"),
             ("q_stride % 4 with the switch on", dict(q_stride=nh * 128 + 6), "multiples of 4"),
             ("qkv of 2^31 bytes with the switch on", dict(B=1 + (1 << 31) // (2369 * (nh * 136 + 8) * 4)), "2^31 bytes")]
    for what, change, msg in cases:
        a = dict(ok)
        a.update(change)
        k = C.c_int(-7)
        rc = lib.yp_debug_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), a["B"], a["N"], nh, a["kd"], a["hd"], a["q_stride"], 0,
                                        nh * 64 + 8, 0, 0, a["on"], C.byref(k), None)
        err = lib.yp_last_error().decode()
        assert rc < 0 and msg in err, (what, rc, err)
        assert k.value == -7, (what, "kernel_out was written")
    torch.cuda.synchronize()
    assert bool((out == 0x5A5B5C5D).all()), "a refused call wrote to the output"


# ---- inside a graph -------------------------------------------------------------------------------------------------------------------
def _own_attention_in_contract(eng, shape, what):
    """the engine's own .attn.o against attention_ref.reference of its own .attn.qkv"""
    op = [o for o in eng.plan(*shape) if o["name"].endswith(".attn.o")][0]
    N = (shape[1] // 32) * (shape[2] // 32)
    qkv = eng.read_tensor(eng.find_tensor(op["name"][:-2] + ".qkv")).reshape(1, N, -1).float()
    o = eng.read_tensor(op["out"][0]).reshape(1, N, -1)[..., op["out"][1]:op["out"][1] + op["out"][2]].float()
    nh = op["out"][2] // 64
    assert qkv.shape[2] == nh * 128
    o64 = A.reference(qkv, nh, 32, 64, 0, "fp32")[0]
    o32 = A.oracle_expression(qkv, nh, 32, 64, torch.float32)
    assert_within_noise_floor(what, o, o32, o64, A.F32_TARGET)
    return op


@pytest.mark.parametrize("family,seg", [("11", True), ("v10", False)])
def test_engine_past_the_generic_limit(family, seg):
    """2560 x 1472 (3680 tokens) is refused without the switch; with it the engine's own attention output holds the fp32 contract and
    hipGraph replay equals eager, bit for bit, on every output"""
    from yolo_puncture_amd.engine import Engine, YolopError
    shape = (1, 1472, 2560)
    st, im = make_case("n", 80, seg, 0, shape) if family == "v10" else make_case_family(family, "n", 80, 0, shape)
    imc = im.cuda()
    eng = Engine("n", 80, seg, "fp32", 0, state=st, family=family)
    eng.set_autotune(False)
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)"):
        eng.plan(*shape)
    eng.set_attention_f32("stream")
    ref = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    op = _own_attention_in_contract(eng, shape, f"{family}-n fp32 .attn.o at {shape}")
    assert op["kernel"] == "attention_stream_f32_kernel"
    eng.set_graph(True)
    for _ in range(2):
        out = eng.forward(imc)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    eng.close()


def test_engine_between_the_limits_with_the_switch_on_and_off():
    """1088 x 1920 (2040 tokens): either kernel holds the shape, and the engine's own attention output holds the contract under both"""
    from yolo_puncture_amd.engine import Engine
    shape = (1, 1088, 1920)
    st, im = make_case("n", 80, False, 0, shape)
    imc = im.cuda()
    eng = Engine("n", 80, False, "fp32", 0, state=st)
    eng.set_autotune(False)
    for value, kernel in (("stream", "attention_stream_f32_kernel"), ("generic", "attention_kernel")):
        eng.set_attention_f32(value)
        eng.forward(imc)
        torch.cuda.synchronize()
        op = _own_attention_in_contract(eng, shape, f"v10-n fp32 .attn.o at {shape}, attention_f32={value}")
        assert op["kernel"] == kernel
        prof = [o for o in eng.profile(imc, iters=1) if o["name"] == op["name"]]
        assert [o["kernel"] for o in prof] == [kernel], (value, "profile", prof)
    eng.close()


def test_facade_predicts_at_imgsz_2560():
    from yolo_puncture_amd import hostops
    from yolo_puncture_amd.engine import YolopError
    from yolo_puncture_amd.predictor import YOLO
    frame = rand_image((1, 1472, 2560, 3), seed=11)[0].numpy()
    boxed = hostops.letterbox(frame, 2560)[0]
    assert boxed.shape == (1472, 2560, 3)
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)"):
        YOLO("synthetic:n", dtype="fp32").predict(frame, imgsz=2560)
    model = YOLO("synthetic:n", dtype="fp32", attention_f32="stream")
    eng = model._engine()
    eng.set_autotune(False)
    conf = 0.25
    r = model.predict(frame, conf=conf, imgsz=2560)[0]
    b = r.boxes.cpu().numpy()
    det = eng.forward(torch.from_numpy(boxed[None]).cuda())["det"][0].cpu()
    det = det[det[:, 4] > conf]
    assert det.shape[0] == len(b.cls)
    want = hostops.scale_boxes_t((1472, 2560), det[:, :4].clone(), (1472, 2560))
    assert np.array_equal(b.xyxy, want.numpy()) and np.array_equal(b.conf, det[:, 4].numpy())
