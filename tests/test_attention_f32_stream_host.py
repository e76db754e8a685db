"""The fp32 streaming attention kernel, host side (no GPU): the CPU restatement of the kernel's block and summation order
(attention_f32_stream_cases.emulate) stays inside the fp32 contract - so the order was chosen before the kernel ran, and a failure of
test_gpu_attention_f32_stream.py is the kernel's -, and the planner takes the kernel only where an engine's switch is on and the kernel's
scope holds: everything else plans, names, counts and refuses as before."""
import pytest
import torch

import attention_ref as A
import attention_f32_stream_cases as S
from helpers import assert_within_noise_floor
from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import ATTENTION_F32, EXPORTS, Engine, YolopError, load_library

KERNEL = "attention_stream_f32_kernel"
SHAPES_PAST_THE_GENERIC_LIMIT = ((1, 2560, 1472), (1, 2176, 3840))      # 3680 and 8160 tokens


@pytest.mark.parametrize("case", S.EMULATION_CASES, ids=A.case_id)
def test_emulated_order_stays_in_contract(case):
    """engine error / oracle error, measured over the list: 0.72 0.69 0.75 (401 flat, peaked, shifted), 0.63 0.66 0.49 (513),
    0.45 0.60 0.95 (2369), 0.77 0.52 0.63 (3680); the bound is 2"""
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    got = S.emulate(qkv, nh, kd, hd)
    assert bool(torch.isfinite(got).all())
    e = assert_within_noise_floor(f"emulated fp32 stream {A.case_id(case)}", got, o32, o64, A.F32_TARGET)
    f = float((o32.double() - o64).abs().max())
    print(f"[attention f32 stream] {A.case_id(case)}: emulation / oracle = {e / f:.2f}")


def test_split_formula():
    assert S.groups_per_workgroup(1, 3680, 2) == (58, 1) and S.groups_per_workgroup(8, 1600, 4) == (25, 1) and S.groups_per_workgroup(32, 1600, 4) == (7, 4)
    assert [S.groups_per_workgroup(1, 1025, 2, w) for w in (1, 8, 256)] == [(1, 17), (4, 5), (17, 1)]


def _attn(ops):
    got = [o for o in ops if o["name"].endswith(".attn.o")]
    assert len(got) == 1
    return got[0]


def _rows(ops, with_attn=True):
    return [(o["name"], o["kernel"], o["flops"]) for o in ops if with_attn or not o["name"].endswith(".attn.o")]


def _engines(dtype="fp32", **kw):
    return (("v10-n detect", lambda: Engine("n", 80, False, dtype, 0, **kw)), ("11-n seg", lambda: Engine("n", 80, True, dtype, 0, family="11", **kw)))


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_the_planned_name_is_a_kernel_symbol():
    assert KERNEL in _kernel_symbols(load_library()._name)


def test_exports_name_the_new_calls():
    assert {"yp_set_attention_f32_stream", "yp_debug_attention_f32"} <= set(EXPORTS)
    assert ATTENTION_F32 == {"generic": 0, "stream": 1}


def test_switched_engines_plan_past_the_generic_limit():
    for what, make in _engines(attention_f32="stream"):
        e, d = make(), make()
        d.set_attention_f32("generic")
        for B, H, W in SHAPES_PAST_THE_GENERIC_LIMIT:
            op = _attn(e.plan(B, H, W))
            assert op["kernel"] == KERNEL, (what, H, W, op["kernel"])
            N = (H // 32) * (W // 32)
            nh = op["out"][2] // 64
            assert op["flops"] == 2.0 * B * nh * N * N * (32 + 32 + 64), "Q.K^T counts twice: the kernel computes it in both passes"
            assert e.lib.yp_debug_host_selftest(e._h) > 0, (what, e.lib.yp_last_error())
            with pytest.raises(YolopError, match=rf"{N} attention tokens.*at most 2368 \(a streaming form is not built\)"):
                d.plan(B, H, W)
        # 400 tokens: nothing at all changes
        assert _rows(e.plan(1, 640, 640)) == _rows(d.plan(1, 640, 640))
        # between the two limits the switch changes the attention op and nothing else of the plan
        pe, pd = e.plan(1, 1088, 1920), d.plan(1, 1088, 1920)
        assert _attn(pe)["kernel"] == KERNEL and _attn(pd)["kernel"] == "attention_kernel"
        assert _attn(pe)["flops"] == _attn(pd)["flops"] + 2.0 * (_attn(pe)["out"][2] // 64) * 2040 * 2040 * 32
        assert _rows(pe, False) == _rows(pd, False)
        e.close()
        d.close()


def test_default_engines_refuse_as_before():
    for what, make in _engines():
        e = make()
        with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)") as err:
            e.plan(1, 2560, 1472)
        assert 'attention_f32="stream"' in str(err.value), "the refusal names the switch that would hold the shape"
        assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
        e.close()


def test_bf16_engines_ignore_the_switch():
    for form in ("auto", "stream"):
        for what, make in _engines("bf16", attention=form):
            e, d = make(), make()
            e.set_attention_f32("stream")
            for B, H, W in ((1, 640, 640), (1, 1088, 1920)):
                assert _rows(e.plan(B, H, W)) == _rows(d.plan(B, H, W)), (what, form, H, W)
            if form == "stream":
                assert _rows(e.plan(1, 2560, 1472)) == _rows(d.plan(1, 2560, 1472))
                continue
            texts = []
            for eng in (e, d):
                with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)") as err:
                    eng.plan(1, 2560, 1472)
                texts.append(str(err.value))
            assert texts[0] == texts[1] and "attention_f32" not in texts[0]
            e.close()
            d.close()


def test_fp32_m_keeps_the_generic_kernel_and_its_bound():
    e, d = Engine("m", 80, False, "fp32", 0, attention_f32="stream"), Engine("m", 80, False, "fp32", 0)
    texts = []
    for eng in (e, d):
        with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364 \(a streaming form is not built\)") as err:
            eng.plan(1, 1408, 1760)
        texts.append(str(err.value))
    assert texts[0] == texts[1] and "attention_f32" not in texts[0] and "stream_wide" not in texts[0]
    for B, H, W in ((1, 640, 640), (1, 1088, 1920)):
        assert _rows(e.plan(B, H, W)) == _rows(d.plan(B, H, W))
        assert _attn(e.plan(B, H, W))["kernel"] == "attention_kernel"
    e.close()
    d.close()


def test_a_batch_past_the_byte_bound_is_refused_as_such_under_the_switch():
    """qkv of 2^31 bytes leaves the kernel's scope; the caller is told the byte bound (and the batch that fits), not the generic kernel's
    token bound behind it"""
    for what, make in _engines(attention_f32="stream"):
        e = make()
        mb = e.max_batch(2560, 1472)
        assert len(e.plan(mb, 2560, 1472)) > 0
        with pytest.raises(YolopError, match=rf"2\^31 bytes.*largest batch that fits is {mb}"):
            e.plan(mb + 1, 2560, 1472)
        e.close()


def test_switch_values_and_a_change_drops_the_plan():
    e = Engine("n", 80, False, "fp32", 0)
    for bad in (2, -1, 7):
        assert e.lib.yp_set_attention_f32_stream(e._h, bad) < 0 and b"yp_set_attention_f32_stream" in e.lib.yp_last_error()
    assert e.lib.yp_set_attention_f32_stream(None, 1) < 0
    with pytest.raises(ValueError):
        e.set_attention_f32("flash")
    with pytest.raises(ValueError):
        Engine("n", 80, False, "fp32", 0, attention_f32="flash")
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.set_attention_f32("stream")                                              # the same shape plans again, under the switch
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == KERNEL
    assert len(e.plan(1, 2560, 1472)) > 0
    for form in ("stream", "stream_wide", "auto"):                             # the form is another matter: an fp32 engine plans the same
        e.set_attention_form(form)
        assert _attn(e.plan(1, 2560, 1472))["kernel"] == KERNEL
    e.set_attention_f32("generic")
    with pytest.raises(YolopError, match="3680 attention tokens"):
        e.plan(1, 2560, 1472)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.close()


def test_environment_sets_the_switch_at_create(monkeypatch):
    monkeypatch.setenv("YOLOP_ATTN_F32", "stream")
    e = Engine("n", 80, False, "fp32", 0)
    monkeypatch.delenv("YOLOP_ATTN_F32")
    d = Engine("n", 80, False, "fp32", 0)
    assert _attn(e.plan(1, 2560, 1472))["kernel"] == KERNEL                    # read at yp_create, per engine
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368"):
        d.plan(1, 2560, 1472)
    e.set_attention_f32("generic")                                             # an explicit call overrides what the variable said
    with pytest.raises(YolopError, match="3680 attention tokens"):
        e.plan(1, 2560, 1472)
    e.close()
    d.close()
    for bad in ("flash", "1", "generic"):
        monkeypatch.setenv("YOLOP_ATTN_F32", bad)
        with pytest.raises(YolopError, match="YOLOP_ATTN_F32"):
            Engine("n", 80, False, "fp32", 0)
    monkeypatch.setenv("YOLOP_ATTN_F32", "")
    Engine("n", 80, False, "fp32", 0).close()


def test_facade_keys_its_engines_by_the_switch(monkeypatch):
    from yolo_puncture_amd import YOLO, predictor
    with pytest.raises(ValueError):
        YOLO("synthetic:n", dtype="fp32", attention_f32="flash")
    plain, switched = YOLO("synthetic:n", dtype="fp32"), YOLO("synthetic:n", dtype="fp32", attention_f32="stream")
    assert plain.attention_f32 is None and switched.attention_f32 == "stream"
    made = []

    def fake_engine(*a, **kw):                                   # (a real one would upload weights: no GPU here)
        made.append(kw)
        return object()
    monkeypatch.setattr(predictor, "Engine", fake_engine)
    monkeypatch.setattr(predictor, "_ENGINE_CACHE", {})
    a, b = plain._engine(), switched._engine()
    assert a is not b and a is plain._engine() and b is switched._engine(), "one cached engine per value of the switch"
    assert [kw["attention_f32"] for kw in made] == [None, "stream"]
