"""The fp32 streaming attention kernel for 36/72 heads, host side (no GPU): the CPU restatement of the kernel's block and summation order
(attention_f32_wide_cases.emulate) stays inside the fp32 contract - so the order was chosen before the kernel ran, and a failure of
test_gpu_attention_f32_wide.py is the kernel's -, and the planner takes the kernel only where an engine's switch has the wide bit
(value 3, "stream_wide") and the kernel's scope holds: everything else plans, names, counts and refuses as before."""
import pytest
import torch

import attention_ref as A
import attention_f32_wide_cases as W
from helpers import assert_within_noise_floor
from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import ATTENTION_F32, ATTENTION_F32_WIDE, Engine, YolopError, load_library

KERNEL = "attention_stream_wide_f32_kernel"
KERNEL_32_64 = "attention_stream_f32_kernel"
SHAPES_PAST_THE_GENERIC_LIMIT = ((1, 1408, 1760), (1, 2560, 1472), (1, 2176, 3840))      # 2420, 3680 and 8160 tokens


@pytest.mark.parametrize("case", W.EMULATION_CASES, ids=A.case_id)
def test_emulated_order_stays_in_contract(case):
    """engine error / oracle error, measured over the list: 0.48 0.62 0.88 (401 flat, peaked, shifted), 0.57 0.52 0.38 (513),
    0.40 0.49 0.63 (2365), 0.58 0.54 0.43 (3680); the bound is 2"""
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    got = W.emulate(qkv, nh, kd, hd)
    assert bool(torch.isfinite(got).all())
    e = assert_within_noise_floor(f"emulated fp32 wide stream {A.case_id(case)}", got, o32, o64, A.F32_TARGET)
    f = float((o32.double() - o64).abs().max())
    assert f > 0, "the float32 oracle's own error on the case is the bound's unit"
    print(f"[attention f32 wide stream] {A.case_id(case)}: emulation / oracle = {e / f:.2f}")


def test_score_chains_cover_every_key_dimension_once():
    for order in W.ORDERS:
        assert sorted(d for c in W.score_chains(order) for d in c) == list(range(36)), order
    assert [len(c) for c in W.score_chains()] == [8, 8, 8, 8, 4]
    assert W.score_chains()[0] == [0, 8, 16, 24, 1, 9, 17, 25] and W.score_chains()[4] == [32, 33, 34, 35]


def test_split_formula():
    assert W.groups_per_workgroup(1, 3680, 4) == (58, 1) and W.groups_per_workgroup(8, 1600, 4) == (25, 1) and W.groups_per_workgroup(32, 1600, 4) == (7, 4)
    assert [W.groups_per_workgroup(3, 1025, 2, w) for w in (1, 8, 256)] == [(1, 17), (2, 9), (17, 1)]


def _attn(ops):
    got = [o for o in ops if o["name"].endswith(".attn.o")]
    assert len(got) == 1
    return got[0]


def _rows(ops, with_attn=True):
    return [(o["name"], o["kernel"], o["flops"]) for o in ops if with_attn or not o["name"].endswith(".attn.o")]


def _m(dtype="fp32", **kw):
    return Engine("m", 80, False, dtype, 0, **kw)


def _n_engines(**kw):
    return (("v10-n detect", lambda: Engine("n", 80, False, "fp32", 0, **kw)), ("11-n seg", lambda: Engine("n", 80, True, "fp32", 0, family="11", **kw)))


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_the_planned_name_is_a_kernel_symbol():
    assert KERNEL in _kernel_symbols(load_library()._name)


def test_the_name_has_a_table_of_its_own():
    assert ATTENTION_F32 == {"generic": 0, "stream": 1} and ATTENTION_F32_WIDE == {"stream_wide": 3}


def test_m_under_the_switch_plans_past_the_generic_limit():
    e, d = _m(attention_f32="stream_wide"), _m()
    for B, H, W_ in SHAPES_PAST_THE_GENERIC_LIMIT:
        op = _attn(e.plan(B, H, W_))
        assert op["kernel"] == KERNEL, (H, W_, op["kernel"])
        N = (H // 32) * (W_ // 32)
        nh = op["out"][2] // 72
        assert nh == 4
        assert op["flops"] == 2.0 * B * nh * N * N * (36 + 36 + 72), "Q.K^T counts twice: the kernel computes it in both passes"
        assert e.lib.yp_debug_host_selftest(e._h) > 0, (H, W_, e.lib.yp_last_error())
        with pytest.raises(YolopError, match=rf"{N} attention tokens.*at most 2364 \(a streaming form is not built\)"):
            d.plan(B, H, W_)
    # 400 tokens: nothing at all changes
    assert _rows(e.plan(1, 640, 640)) == _rows(d.plan(1, 640, 640))
    # between the two limits the switch changes the attention op and nothing else of the plan
    pe, pd = e.plan(1, 1088, 1920), d.plan(1, 1088, 1920)
    assert _attn(pe)["kernel"] == KERNEL and _attn(pd)["kernel"] == "attention_kernel"
    assert _attn(pe)["flops"] == _attn(pd)["flops"] + 2.0 * 4 * 2040 * 2040 * 36
    assert _rows(pe, False) == _rows(pd, False)
    e.close()
    d.close()


def test_32_64_engines_plan_under_3_as_under_1():
    for what, make in _n_engines():
        e, d = make(), make()
        e.set_attention_f32("stream_wide")
        d.set_attention_f32("stream")
        for B, H, W_ in ((1, 640, 640), (1, 1088, 1920), (1, 2560, 1472), (1, 2176, 3840)):
            assert _rows(e.plan(B, H, W_)) == _rows(d.plan(B, H, W_)), (what, H, W_)
        assert _attn(e.plan(1, 2560, 1472))["kernel"] == KERNEL_32_64
        e.close()
        d.close()


def test_a_bf16_m_engine_ignores_the_switch():
    for form in ("auto", "stream_wide"):
        e, d = _m("bf16", attention=form), _m("bf16", attention=form)
        e.set_attention_f32("stream_wide")
        for B, H, W_ in ((1, 640, 640), (1, 1088, 1920)):
            assert _rows(e.plan(B, H, W_)) == _rows(d.plan(B, H, W_)), (form, H, W_)
        if form == "stream_wide":
            assert _rows(e.plan(1, 1408, 1760)) == _rows(d.plan(1, 1408, 1760))
        else:
            texts = []
            for eng in (e, d):
                with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364 \(a streaming form is not built\)") as err:
                    eng.plan(1, 1408, 1760)
                texts.append(str(err.value))
            assert texts[0] == texts[1] and "attention_f32" not in texts[0]
        e.close()
        d.close()


def test_switch_values_and_a_change_drops_the_plan():
    e = _m()
    for bad in (2, -1, 7, 4):
        assert e.lib.yp_set_attention_f32_stream(e._h, bad) < 0 and b"yp_set_attention_f32_stream" in e.lib.yp_last_error()
    assert e.lib.yp_set_attention_f32_stream(e._h, 3) == 0
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == KERNEL
    assert e.lib.yp_set_attention_f32_stream(e._h, 1) == 0                    # the same shape plans again, under the narrower value
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364"):
        e.plan(1, 1408, 1760)
    e.set_attention_f32("stream_wide")
    assert len(e.plan(1, 1408, 1760)) > 0
    for form in ("stream", "stream_wide", "auto"):                             # the form is another matter: an fp32 engine plans the same
        e.set_attention_form(form)
        assert _attn(e.plan(1, 1408, 1760))["kernel"] == KERNEL
    e.set_attention_f32("generic")
    with pytest.raises(YolopError, match="2420 attention tokens"):
        e.plan(1, 1408, 1760)
    with pytest.raises(ValueError):
        e.set_attention_f32("wide")
    e.close()
    e = Engine("m", 80, False, "fp32", 0, attention_f32="stream_wide")         # the constructor's argument
    assert _attn(e.plan(1, 1408, 1760))["kernel"] == KERNEL
    e.close()


def test_environment_sets_the_switch_at_create(monkeypatch):
    monkeypatch.setenv("YOLOP_ATTN_F32", "stream_wide")
    e, n = _m(), Engine("n", 80, False, "fp32", 0)
    monkeypatch.delenv("YOLOP_ATTN_F32")
    d = _m()
    assert _attn(e.plan(1, 1408, 1760))["kernel"] == KERNEL                    # read at yp_create, per engine
    assert _attn(n.plan(1, 2560, 1472))["kernel"] == KERNEL_32_64              # value 3 has bit 0 too
    with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364"):
        d.plan(1, 1408, 1760)
    e.set_attention_f32("generic")                                             # an explicit call overrides what the variable said
    with pytest.raises(YolopError, match="2420 attention tokens"):
        e.plan(1, 1408, 1760)
    for eng in (e, n, d):
        eng.close()
    monkeypatch.setenv("YOLOP_ATTN_F32", "wide")
    with pytest.raises(YolopError, match="YOLOP_ATTN_F32"):
        _m()


def test_facade_keys_its_engines_by_the_switch(monkeypatch):
    from yolo_puncture_amd import YOLO, predictor
    models = [YOLO("synthetic:m", dtype="fp32", attention_f32=v) for v in (None, "stream", "stream_wide")]
    assert [m.attention_f32 for m in models] == [None, "stream", "stream_wide"]
    made = []

    def fake_engine(*a, **kw):                                   # (a real one would upload weights: no GPU here)
        made.append(kw)
        return object()
    monkeypatch.setattr(predictor, "Engine", fake_engine)
    monkeypatch.setattr(predictor, "_ENGINE_CACHE", {})
    engines = [m._engine() for m in models]
    assert len({id(x) for x in engines}) == 3 and all(m._engine() is x for m, x in zip(models, engines)), "one cached engine per value of the switch"
    assert [kw["attention_f32"] for kw in made] == [None, "stream", "stream_wide"]


def test_a_batch_past_the_byte_bound_is_refused_as_such_under_the_switch():
    """qkv of 2^31 bytes leaves the kernel's scope; the caller is told the byte bound (and the batch that fits), not the generic kernel's
    token bound behind it"""
    e = _m(attention_f32="stream_wide")
    mb = e.max_batch(1408, 1760)
    assert len(e.plan(mb, 1408, 1760)) > 0
    with pytest.raises(YolopError, match=rf"2\^31 bytes.*largest batch that fits is {mb}") as err:
        e.plan(mb + 1, 1408, 1760)
    assert "attention tokens" not in str(err.value)
    e.close()
