"""The streaming attention kernel (csrc/attention_stream.hip): alone through yp_debug_attention_form on the cases of
attention_stream_cases.py - in contract with the fp64 reference of attention_ref.py, whose bounds come from no kernel -, independent of
the workgroup split, the batch and the slices it reads and writes, fed zeros (not what lies behind the tensor) for the keys past N; and
inside a graph, at 441 tokens under the per-op harness and past the generic kernel's 2368 tokens in whole engines and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as A
import attention_stream_cases as S
import perop_bf16
from helpers import make_case, make_case_family, rand_image

pytestmark = pytest.mark.gpu

I16 = torch.int16


def _launch(qkv, nh=2, kd=32, hd=64, **kw):
    from yolo_puncture_amd.engine import attention
    out, kernel = attention(qkv if qkv.is_cuda else qkv.cuda(), nh, kd, hd, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kernel


@pytest.mark.parametrize("case", S.CASES, ids=A.case_id)
def test_stream_contract(case):
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd, form="stream")
    assert kernel == S.STREAM, f"kernel {kernel}"
    A.assert_bf16_contract(f"stream {A.case_id(case)}", got, want, P, v, dist)
    if dist == "lookup":
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        sel = want == exp
        assert float(sel.double().mean()) > 0.999 and bool((got.double()[sel] == exp[sel]).all()), "a query selects exactly its key's value row"


def test_kernel_selection_at_the_switch_over():
    qkv = A.bf16_case(2, 400, 2, 32, 64, "peaked")[0]
    auto, k_auto = _launch(qkv, form="auto")
    stream, k_stream = _launch(qkv, form="stream")
    assert k_auto == S.MFMA and k_stream == S.MFMA, "up to 400 tokens the resident kernel keeps the call under either form"
    assert torch.equal(auto.view(I16), stream.view(I16))
    qkv = A.bf16_case(2, 401, 2, 32, 64, "peaked")[0]
    assert _launch(qkv, form="auto")[1] == S.GENERIC and _launch(qkv)[1] == S.GENERIC and _launch(qkv, form="stream")[1] == S.STREAM


def test_split_batch_and_repeat_do_not_change_the_bits():
    B, N, nh = 2, 1025, 2
    qkv = A.bf16_case(B, N, nh, 32, 64, "peaked")[0]
    base, kernel = _launch(qkv, form="stream")                       # one query group per workgroup
    assert kernel == S.STREAM and S.groups_per_workgroup(B, N, nh) == (9, 1)
    again, _ = _launch(qkv, form="stream")
    assert torch.equal(base.view(I16), again.view(I16)), "two launches are bit-equal"
    for wgs in (4, 8, 12, 20):                                       # runs of 9, 5, 3 and 2 groups
        assert S.groups_per_workgroup(B, N, nh, wgs)[1] > 1
        got, kernel = _launch(qkv, form="stream", wgs=wgs)
        assert kernel == S.STREAM and torch.equal(got.view(I16), base.view(I16)), wgs
    for b in range(B):
        one, kernel = _launch(qkv[b:b + 1].contiguous(), form="stream")
        assert kernel == S.STREAM and torch.equal(one.view(I16), base[b:b + 1].view(I16)), f"image {b} alone differs from image {b} of the batch"


def test_slices_leave_their_surroundings_alone():
    B, N, nh, kd, hd, dist = case = (2, 513, 2, 32, 64, "peaked")
    qkv, _, want, P, v = A.bf16_case(*case)
    sentinel = 0x5A5B
    q_stride, q_coff, o_stride, o_coff = nh * 128 + 24, 8, nh * 64 + 16, 8
    wide = A.embed(qkv, q_stride, q_coff, float("nan"))
    out = torch.full((B, N, o_stride), sentinel, dtype=I16).view(torch.bfloat16).cuda()
    got_wide, kernel = _launch(wide, q_coff=q_coff, out=out, o_coff=o_coff, form="stream")
    assert kernel == S.STREAM
    got = got_wide[..., o_coff:o_coff + nh * hd]
    outside = torch.ones(o_stride, dtype=torch.bool)
    outside[o_coff:o_coff + nh * hd] = False
    assert bool((got_wide.view(I16)[..., outside] == sentinel).all()), "a store left the output slice"
    A.assert_bf16_contract(f"stream slice {A.case_id(case)}", got, want, P, v, dist)
    compact, _ = _launch(qkv, form="stream")
    assert torch.equal(compact.view(I16), got.contiguous().view(I16)), "the slice changes addresses only"


def test_ragged_key_block_is_fed_zeros():
    """N = 513 leaves 127 absent keys in the last block of either image; behind the tensor the allocation holds NaN (0 x NaN = NaN)"""
    B, N, nh, kd, hd, dist = case = (2, 513, 2, 32, 64, "peaked")
    qkv, _, want, P, v = A.bf16_case(*case)
    n = qkv.numel()
    buf = torch.full((n + 256 * 256,), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[:n] = qkv.cuda().reshape(-1)
    got, kernel = _launch(buf[:n].view(B, N, -1), form="stream")
    assert kernel == S.STREAM and bool(torch.isfinite(got).all())
    A.assert_bf16_contract(f"stream ragged {A.case_id(case)}", got, want, P, v, dist)


def test_refusals_happen_on_the_host():
    from yolo_puncture_amd.engine import load_library, YP_BF16, YP_F32
    lib = load_library()
    nh = 2
    qkv = torch.zeros((1, 2369, nh * 136 + 8), dtype=torch.float32, device="cuda")
    out = torch.full((1, 2369, nh * 64 + 8), 0x5A5B5C5D, dtype=torch.int32, device="cuda")
    ok = dict(dtype=YP_BF16, N=2369, kd=32, hd=64, form=1)
    cases = [("fp32 past the LDS under the form", dict(dtype=YP_F32), "2368"), ("kd 36 past the LDS under the form", dict(N=2365, kd=36, hd=56), "2364"),
             ("form 2", dict(form=2), "form"), ("form -1", dict(form=-1, N=401), "form"), ("q_stride % 4 under the form", dict(q_stride=nh * 128 + 6), "multiples of 4")]
    for what, change, msg in cases:
        a = dict(ok, q_stride=nh * 136 + 8)
        a.update(change)
        k = C.c_int(-7)
        rc = lib.yp_debug_attention_form(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), a["dtype"], 1, a["N"], nh, a["kd"], a["hd"], a["q_stride"], 0,
                                         nh * 64 + 8, 0, 0, a["form"], C.byref(k), None)
        err = lib.yp_last_error().decode()
        assert rc < 0 and msg in err, (what, rc, err)
        assert k.value == -7, (what, "kernel_out was written")
    torch.cuda.synchronize()
    assert bool((out == 0x5A5B5C5D).all()), "a refused call wrote to the output"


# ---- inside a graph -------------------------------------------------------------------------------------------------------------------
def test_per_op_contract_at_441_tokens(monkeypatch):
    """672 x 672: the project's per-op harness (every op fed the oracle's tensors, <= 1 bf16 ulp on < 2 % of the elements) with the PSA block
    on the streaming kernel. (On the CPU the oracle's own tap of that op is within 1 ulp of the fp64 statement with 0.01 % of the elements
    differing: the bound is attainable.)"""
    from yolo_puncture_amd.engine import Engine
    monkeypatch.setenv("YOLOP_ATTN_FORM", "stream")
    e = Engine("n", 80, False, "bf16", 0)
    assert [o["kernel"] for o in e.plan(1, 672, 672) if o["name"] == "model.10.attn.o"] == ["attention_stream_kernel"]
    e.close()
    r = perop_bf16.per_op_bf16("n", False, (1, 672, 672), -1, True, monkeypatch, 80, autotune=False)
    assert "model.10.attn.o" in [n for n, _, _ in r["rows"]]


def test_form_change_on_a_warmed_engine():
    """one engine, one shape, forwarded under auto, stream and auto again: the plan names the kernel that runs at each step (the per-shape
    tuning memo survives the change and must not bring the other form's name back), the outputs of the two auto steps are bit-equal"""
    from yolo_puncture_amd.engine import Engine
    shape = (1, 672, 672)                                        # 441 tokens
    st, im = make_case("n", 80, False, 0, shape)
    imc = im.cuda()
    eng = Engine("n", 80, False, "bf16", 0, state=st)
    eng.set_autotune(False)
    outs = []
    for form, kernel in (("auto", "attention_kernel"), ("stream", "attention_stream_kernel"), ("auto", "attention_kernel"), ("stream", "attention_stream_kernel")):
        eng.set_attention_form(form)
        out = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
        torch.cuda.synchronize()
        names = [o["kernel"] for o in eng.plan(*shape) if o["name"] == "model.10.attn.o"]
        assert names == [kernel], (form, names)
        prof = [o for o in eng.profile(imc, iters=1) if o["name"] == "model.10.attn.o"]
        assert [o["kernel"] for o in prof] == [kernel], (form, "profile", prof)
        outs.append(out)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[2][k]) and torch.equal(outs[1][k], outs[3][k]), k
    eng.close()


@pytest.mark.parametrize("family,seg", [("11", True), ("v10", False)])
def test_engine_past_the_generic_limit(family, seg):
    """2560 x 1472 (3680 tokens) was refused: the engine's own .attn.o holds attention_ref.reference of its own .attn.qkv under the widened
    contract, and hipGraph replay equals eager, bit for bit, on every output"""
    from yolo_puncture_amd.engine import Engine
    shape = (1, 1472, 2560)
    st, im = make_case("n", 80, seg, 0, shape) if family == "v10" else make_case_family(family, "n", 80, 0, shape)
    imc = im.cuda()
    eng = Engine("n", 80, seg, "bf16", 0, state=st, family=family, attention="stream")
    eng.set_autotune(False)
    op = [o for o in eng.plan(*shape) if o["name"].endswith(".attn.o")][0]
    assert op["kernel"] == "attention_stream_kernel"
    ref = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    N = (shape[1] // 32) * (shape[2] // 32)
    qkv = eng.read_tensor(eng.find_tensor(op["name"][:-2] + ".qkv")).reshape(1, N, -1).bfloat16()
    o = eng.read_tensor(op["out"][0]).reshape(1, N, -1)[..., op["out"][1]:op["out"][1] + op["out"][2]]
    nh = op["out"][2] // 64
    assert qkv.shape[2] == nh * 128 and N == 3680
    want, P, v = A.reference(qkv, nh, 32, 64, 0, "bf16")
    A.assert_bf16_contract(f"{family}-n .attn.o at {shape}", o, want, P, v, "peaked")
    eng.set_graph(True)
    for _ in range(2):
        out = eng.forward(imc)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    eng.close()


def test_facade_predicts_at_imgsz_2560():
    from yolo_puncture_amd import hostops
    from yolo_puncture_amd.engine import YolopError
    from yolo_puncture_amd.predictor import YOLO
    frame = rand_image((1, 1472, 2560, 3), seed=11)[0].numpy()
    boxed = hostops.letterbox(frame, 2560)[0]
    assert boxed.shape == (1472, 2560, 3)
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368"):
        YOLO("synthetic:11n-seg").predict(frame, imgsz=2560)
    model = YOLO("synthetic:11n-seg", attention="stream")
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
