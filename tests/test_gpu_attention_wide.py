"""The wide-head streaming attention kernel (csrc/attention_stream_wide.hip: bf16, key_dim 36, head_dim 72): alone through
yp_debug_attention_form under the form "stream_wide" on the cases of attention_wide_cases.py - in contract with the fp64 reference of
attention_ref.py, whose bounds come from no kernel -, taken exactly where its scope holds, independent of the workgroup split, the batch
and the slices it reads and writes, fed zeros (not what lies behind the tensor) for the keys past N; and inside a graph: YOLOv10-M at 156
tokens under the per-op harness, and past the generic kernel's 2364 tokens in a whole engine and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as A
import attention_wide_cases as W
import perop_bf16
from helpers import make_case, rand_image

pytestmark = pytest.mark.gpu

I16 = torch.int16
WIDE_KERNEL = "attention_stream_wide_kernel"


def _launch(qkv, nh=2, kd=W.KD, hd=W.HD, **kw):
    from yolo_puncture_amd.engine import attention
    out, kernel = attention(qkv if qkv.is_cuda else qkv.cuda(), nh, kd, hd, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kernel


@pytest.mark.parametrize("case", W.CASES, ids=A.case_id)
def test_wide_contract(case):
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd, form="stream_wide")
    assert kernel == W.WIDE, f"kernel {kernel}"
    A.assert_bf16_contract(f"stream_wide {A.case_id(case)}", got, want, P, v, dist)
    if dist == "lookup":
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        sel = want == exp
        assert float(sel.double().mean()) > 0.999 and bool((got.double()[sel] == exp[sel]).all()), "a query selects exactly its key's value row"


def test_kernel_selection():
    for N in (20, 401):                                              # no resident sibling: the wide kernel takes either side of 400
        qkv = A.bf16_case(2, N, 2, 36, 72, "peaked")[0]
        assert _launch(qkv)[1] == W.GENERIC and _launch(qkv, form="auto")[1] == W.GENERIC and _launch(qkv, form="stream")[1] == W.GENERIC
        assert _launch(qkv, form="stream_wide")[1] == W.WIDE
    qkv = A.make_qkv("peaked", 2, 129, 2, 36, 56)[0]                 # another head size: the generic kernel, under every form
    assert _launch(qkv, 2, 36, 56, form="stream_wide")[1] == W.GENERIC
    # 32/64 heads behave under the form exactly as under "stream"
    qkv = A.bf16_case(2, 400, 2, 32, 64, "peaked")[0]
    auto, k_auto = _launch(qkv, 2, 32, 64, form="auto")
    wide, k_wide = _launch(qkv, 2, 32, 64, form="stream_wide")
    assert k_auto == W.MFMA and k_wide == W.MFMA and torch.equal(auto.view(I16), wide.view(I16))
    qkv = A.bf16_case(2, 401, 2, 32, 64, "peaked")[0]
    stream, k_stream = _launch(qkv, 2, 32, 64, form="stream")
    wide, k_wide = _launch(qkv, 2, 32, 64, form="stream_wide")
    assert k_stream == W.STREAM and k_wide == W.STREAM and torch.equal(stream.view(I16), wide.view(I16))


def test_split_batch_and_repeat_do_not_change_the_bits():
    B, N, nh = 2, 1025, 2
    qkv = A.bf16_case(B, N, nh, 36, 72, "peaked")[0]
    base, kernel = _launch(qkv, form="stream_wide")                  # one query group per workgroup
    assert kernel == W.WIDE and W.groups_per_workgroup(B, N, nh) == (9, 1)
    again, _ = _launch(qkv, form="stream_wide")
    assert torch.equal(base.view(I16), again.view(I16)), "two launches are bit-equal"
    for wgs in (4, 8, 12, 20):                                       # runs of 9, 5, 3 and 2 groups
        assert W.groups_per_workgroup(B, N, nh, wgs)[1] > 1
        got, kernel = _launch(qkv, form="stream_wide", wgs=wgs)
        assert kernel == W.WIDE and torch.equal(got.view(I16), base.view(I16)), wgs
    for b in range(B):
        one, kernel = _launch(qkv[b:b + 1].contiguous(), form="stream_wide")
        assert kernel == W.WIDE and torch.equal(one.view(I16), base[b:b + 1].view(I16)), f"image {b} alone differs from image {b} of the batch"


@pytest.mark.parametrize("o_pad,o_coff", [(16, 8), (12, 4)], ids=["o16-aligned", "o8-aligned"])
def test_slices_leave_their_surroundings_alone(o_pad, o_coff):
    """qkv embedded in NaN (what follows a head's V is the next head or foreign data), the output in a sentinel; with o_stride = nh * 72 + 12
    and o_coff = 4 the output rows are only 8-byte aligned"""
    B, N, nh, kd, hd, dist = case = (2, 513, 2, 36, 72, "peaked")
    qkv, _, want, P, v = A.bf16_case(*case)
    sentinel = 0x5A5B
    q_stride, q_coff, o_stride = nh * 144 + 24, 8, nh * 72 + o_pad
    wide = A.embed(qkv, q_stride, q_coff, float("nan"))
    out = torch.full((B, N, o_stride), sentinel, dtype=I16).view(torch.bfloat16).cuda()
    got_wide, kernel = _launch(wide, q_coff=q_coff, out=out, o_coff=o_coff, form="stream_wide")
    assert kernel == W.WIDE
    got = got_wide[..., o_coff:o_coff + nh * hd]
    outside = torch.ones(o_stride, dtype=torch.bool)
    outside[o_coff:o_coff + nh * hd] = False
    assert bool((got_wide.view(I16)[..., outside] == sentinel).all()), "a store left the output slice"
    A.assert_bf16_contract(f"stream_wide slice {A.case_id(case)}", got, want, P, v, dist)
    compact, _ = _launch(qkv, form="stream_wide")
    assert torch.equal(compact.view(I16), got.contiguous().view(I16)), "the slice changes addresses only"


@pytest.mark.parametrize("N", [513, 129])
def test_ragged_key_block_is_fed_zeros(N):
    """N = 513 / 129 leave 127 absent keys in the last block of either image; behind the tensor the allocation holds NaN (0 x NaN = NaN)"""
    B, _, nh, kd, hd, dist = case = (2, N, 2, 36, 72, "peaked")
    qkv, _, want, P, v = A.bf16_case(*case)
    n = qkv.numel()
    buf = torch.full((n + 256 * 288,), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[:n] = qkv.cuda().reshape(-1)
    got, kernel = _launch(buf[:n].view(B, N, -1), form="stream_wide")
    assert kernel == W.WIDE and bool(torch.isfinite(got).all())
    A.assert_bf16_contract(f"stream_wide ragged {A.case_id(case)}", got, want, P, v, dist)


def test_refusals_happen_on_the_host():
    from yolo_puncture_amd.engine import load_library, YP_BF16, YP_F32
    lib = load_library()
    nh, N = 2, W.GENERIC_TOKENS + 1
    qkv = torch.zeros((1, N, nh * 144 + 8), dtype=torch.float32, device="cuda")
    out = torch.full((1, N, nh * 72 + 8), 0x5A5B5C5D, dtype=torch.int32, device="cuda")
    ok = dict(dtype=YP_BF16, N=N, form=3, q_stride=nh * 144 + 8)
    cases = [("form 2", dict(form=2), "0 auto | 1 stream | 3 stream_wide"), ("form -1", dict(form=-1, N=401), "0 auto | 1 stream | 3 stream_wide"),
             ("fp32 past the LDS under the form", dict(dtype=YP_F32), "2364"), ("q_stride % 4 under the form", dict(q_stride=nh * 144 + 6), "multiples of 4")]
    for what, change, msg in cases:
        a = dict(ok)
        a.update(change)
        k = C.c_int(-7)
        rc = lib.yp_debug_attention_form(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), a["dtype"], 1, a["N"], nh, 36, 72, a["q_stride"], 0,
                                         nh * 72 + 8, 0, 0, a["form"], C.byref(k), None)
        err = lib.yp_last_error().decode()
        assert rc < 0 and msg in err, (what, rc, err)
        assert k.value == -7, (what, "kernel_out was written")
    torch.cuda.synchronize()
    assert bool((out == 0x5A5B5C5D).all()), "a refused call wrote to the output"


# ---- inside a graph -------------------------------------------------------------------------------------------------------------------
def test_per_op_contract_at_156_tokens(monkeypatch):
    """384 x 416 (12 x 13 = 156 tokens: two key blocks, the second ragged): the project's per-op harness (every op fed the oracle's
    tensors, <= 1 bf16 ulp on < 2 % of the elements) on YOLOv10-M with the PSA block on the wide kernel. (On the CPU the oracle's own tap
    of that op against the fp64 statement of its own .attn.qkv tap: worst 1.0 ulp, 0.002 % of the elements differing, none above 1 ulp -
    the harness bound is attainable, so it applies as it is.)"""
    from yolo_puncture_amd.engine import Engine
    monkeypatch.setenv("YOLOP_ATTN_FORM", "stream_wide")
    e = Engine("m", 80, False, "bf16", 0)
    assert [o["kernel"] for o in e.plan(1, 384, 416) if o["name"] == "model.10.attn.o"] == [WIDE_KERNEL]
    e.close()
    r = perop_bf16.per_op_bf16("m", False, (1, 384, 416), -1, True, monkeypatch, 80, autotune=False)
    assert "model.10.attn.o" in [n for n, _, _ in r["rows"]]


def test_form_change_on_a_warmed_engine():
    """one M engine, one shape, forwarded under auto, stream, stream_wide and auto again: the plan and the profile name the kernel that runs
    at each step, the outputs of the two auto steps are bit-equal"""
    from yolo_puncture_amd.engine import Engine
    shape = (1, 384, 416)
    st, im = make_case("m", 80, False, 0, shape)
    imc = im.cuda()
    eng = Engine("m", 80, False, "bf16", 0, state=st)
    eng.set_autotune(False)
    outs = []
    for form, kernel in (("auto", "attention_kernel"), ("stream", "attention_kernel"), ("stream_wide", WIDE_KERNEL), ("auto", "attention_kernel")):
        eng.set_attention_form(form)
        out = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
        torch.cuda.synchronize()
        names = [o["kernel"] for o in eng.plan(*shape) if o["name"] == "model.10.attn.o"]
        assert names == [kernel], (form, names)
        prof = [o for o in eng.profile(imc, iters=1) if o["name"] == "model.10.attn.o"]
        assert [o["kernel"] for o in prof] == [kernel], (form, "profile", prof)
        outs.append(out)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[3][k]) and torch.equal(outs[0][k], outs[1][k]), k
    eng.close()


def test_engine_past_the_generic_limit():
    """1408 x 1760 (2420 tokens) is refused without the form: the engine's own .attn.o holds attention_ref.reference of its own .attn.qkv
    under the widened contract, and hipGraph replay equals eager, bit for bit, on every output"""
    from yolo_puncture_amd.engine import Engine
    shape = (1, 1408, 1760)
    st, im = make_case("m", 80, False, 0, shape)
    imc = im.cuda()
    eng = Engine("m", 80, False, "bf16", 0, state=st, attention="stream_wide")
    eng.set_autotune(False)
    op = [o for o in eng.plan(*shape) if o["name"].endswith(".attn.o")][0]
    assert op["kernel"] == WIDE_KERNEL
    ref = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    N = (shape[1] // 32) * (shape[2] // 32)
    qkv = eng.read_tensor(eng.find_tensor(op["name"][:-2] + ".qkv")).reshape(1, N, -1).bfloat16()
    o = eng.read_tensor(op["out"][0]).reshape(1, N, -1)[..., op["out"][1]:op["out"][1] + op["out"][2]]
    assert qkv.shape[2] == 4 * 144 and op["out"][2] == 4 * 72 and N == 2420
    want, P, v = A.reference(qkv, 4, 36, 72, 0, "bf16")
    A.assert_bf16_contract(f"v10-m .attn.o at {shape}", o, want, P, v, "peaked")
    eng.set_graph(True)
    for _ in range(2):
        out = eng.forward(imc)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
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
        default = YOLO("synthetic:m")
        with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364"):
            default.predict(frame, imgsz=1760)
        model = YOLO("synthetic:m", attention="stream_wide")
        eng = model._engine()
        assert eng is not default._engine(), "the form is part of the engine-cache key"
        eng.set_autotune(False)
        conf = 0.25
        r = model.predict(frame, conf=conf, imgsz=1760)[0]
        b = r.boxes.cpu().numpy()
        det = eng.forward(torch.from_numpy(boxed[None]).cuda())["det"][0].cpu()
        det = det[det[:, 4] > conf]
        assert det.shape[0] == len(b.cls)
        want = hostops.scale_boxes_t((1408, 1760), det[:, :4].clone(), (1408, 1760))
        assert np.array_equal(b.xyxy, want.numpy()) and np.array_equal(b.conf, det[:, 4].numpy())
    finally:                                 # the two v10-M engines (arenas, a captured graph) do not stay behind in the process
        torch.cuda.synchronize()
        for key in set(predictor._ENGINE_CACHE) - cached:
            predictor._ENGINE_CACHE.pop(key).close()
