"""The wide-head streaming attention form ("stream_wide", value 3), host side (no GPU): the reference pair alone stays inside the contract
on every stand-alone case of attention_wide_cases.py (so a failure of test_gpu_attention_wide.py is the kernel's), a YOLOv10-M engine
under the form plans past the generic kernel's 2364 tokens on attention_stream_wide_kernel, engines with 32/64 heads plan under it as they
do under "stream", and everything outside the kernel's scope plans, names and refuses as before."""
import pytest
import torch

import attention_ref as A
import attention_wide_cases as W
from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import ATTENTION_FORMS, Engine, YolopError, load_library

WIDE_KERNEL = "attention_stream_wide_kernel"
M_SHAPES = ((1, 1408, 1760), (1, 2560, 1472), (1, 2176, 3840))      # 2420, 3680 and 8160 tokens


@pytest.mark.parametrize("case", W.CASES, ids=A.case_id)
def test_reference_pair_stays_in_contract(case):
    """the oracle's float32 restatement against the fp64 reference; measured over the list: worst / allowed <= 0.88, <= 0.21 % of the
    elements differing, <= 0.027 % above 1 ulp - the caps of attention_ref.py (2 %, 0.5 %) are reachable and leave a broken kernel no room"""
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    assert qkv.dtype == torch.bfloat16 and bool(torch.isfinite(want).all())
    o32 = A.oracle_expression(qkv, nh, kd, hd, torch.float32, "bf16")
    A.assert_bf16_contract(f"float32 restatement {A.case_id(case)}", o32, want, P, v, dist)
    if dist == "lookup":
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        assert float((want == exp).double().mean()) > 0.999
        assert bool((o32.double()[want == exp] == exp[want == exp]).all())


def _attn(ops):
    got = [o for o in ops if o["name"].endswith(".attn.o")]
    assert len(got) == 1
    return got[0]


def _m(form=None, dtype="bf16"):
    return Engine("m", 80, False, dtype, 0, attention=form)


def test_m_engine_plans_past_the_generic_limit():
    assert (1408 // 32) * (1760 // 32) == 2420 > W.GENERIC_TOKENS
    e = _m("stream_wide")
    for B, H, Wd in M_SHAPES + ((1, 640, 640), (16, 640, 640)):        # (the wide kernel has no resident sibling: 400 tokens too)
        op = _attn(e.plan(B, H, Wd))
        assert op["kernel"] == WIDE_KERNEL, (H, Wd, op["kernel"])
        N = (H // 32) * (Wd // 32)
        assert op["out"][2] == 4 * W.HD
        assert op["flops"] == 2.0 * B * 4 * N * N * (36 + 36 + 72), "Q.K^T counts twice: the kernel computes it in both passes"
        assert e.lib.yp_debug_host_selftest(e._h) > 0, (H, Wd, e.lib.yp_last_error())
    e.close()


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_the_planned_name_is_a_kernel_symbol():
    syms = _kernel_symbols(load_library()._name)
    assert WIDE_KERNEL in syms and "attention_stream_kernel" in syms


def test_the_form_changes_the_attention_op_and_nothing_else_of_the_plan():
    e, d = _m("stream_wide"), _m("auto")
    pe, pd = e.plan(1, 1088, 1920), d.plan(1, 1088, 1920)
    assert _attn(pe)["kernel"] == WIDE_KERNEL and _attn(pd)["kernel"] == "attention_kernel"
    assert [(o["name"], o["kernel"], o["flops"]) for o in pe if not o["name"].endswith(".attn.o")] == \
           [(o["name"], o["kernel"], o["flops"]) for o in pd if not o["name"].endswith(".attn.o")]
    e.close()
    d.close()


def test_m_engines_outside_the_form_or_the_scope_refuse_as_before():
    for form, dtype in (("auto", "bf16"), ("stream", "bf16"), ("stream_wide", "fp32")):
        e = _m(form, dtype)
        with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364 \(a streaming form is not built\)"):
            e.plan(1, 1408, 1760)
        assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel", (form, dtype)
        assert _attn(e.plan(1, 640, 640))["kernel"] == "attention_kernel", (form, dtype)
        e.close()


def test_narrow_head_engines_plan_as_under_stream():
    for what, make in (("v10-n detect", lambda f: Engine("n", 80, False, "bf16", 0, attention=f)),
                       ("11-n seg", lambda f: Engine("n", 80, True, "bf16", 0, family="11", attention=f))):
        w, s = make("stream_wide"), make("stream")
        for B, H, Wd in ((1, 640, 640), (1, 1088, 1920), (1, 2560, 1472)):
            rows_w = [(o["name"], o["kernel"], o["flops"]) for o in w.plan(B, H, Wd)]
            rows_s = [(o["name"], o["kernel"], o["flops"]) for o in s.plan(B, H, Wd)]
            assert rows_w == rows_s, (what, H, Wd)
            assert WIDE_KERNEL not in [k for _, k, _ in rows_w]
        assert _attn(w.plan(1, 2560, 1472))["kernel"] == "attention_stream_kernel"
        w.close()
        s.close()


def test_form_values_and_a_change_drops_the_plan():
    assert ATTENTION_FORMS == {"auto": 0, "stream": 1, "stream_wide": 3}
    e = _m()
    for bad in (2, -1, 7):
        assert e.lib.yp_set_attention_form(e._h, bad) < 0
        assert b"0 auto | 1 stream | 3 stream_wide" in e.lib.yp_last_error()
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    assert e.lib.yp_set_attention_form(e._h, 3) == 0                           # the same shape plans again, under the new form
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == WIDE_KERNEL
    assert len(e.plan(1, 1408, 1760)) > 0
    e.set_attention_form("stream")
    with pytest.raises(YolopError, match="2420 attention tokens"):
        e.plan(1, 1408, 1760)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.set_attention_form("stream_wide")
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == WIDE_KERNEL
    e.set_attention_form("auto")
    with pytest.raises(YolopError, match="2420 attention tokens"):
        e.plan(1, 1408, 1760)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.close()


def test_environment_sets_the_form_at_create(monkeypatch):
    monkeypatch.setenv("YOLOP_ATTN_FORM", "stream_wide")
    e = _m()
    monkeypatch.delenv("YOLOP_ATTN_FORM")
    d = _m()
    assert _attn(e.plan(1, 1408, 1760))["kernel"] == WIDE_KERNEL               # read at yp_create, per engine
    with pytest.raises(YolopError, match=r"2420 attention tokens.*at most 2364"):
        d.plan(1, 1408, 1760)
    e.set_attention_form("auto")                                               # an explicit call overrides what the variable said
    with pytest.raises(YolopError, match="2420 attention tokens"):
        e.plan(1, 1408, 1760)
    e.close()
    d.close()
    monkeypatch.setenv("YOLOP_ATTN_FORM", "wide")
    with pytest.raises(YolopError, match="YOLOP_ATTN_FORM"):
        _m()


def test_facade_keys_its_engines_by_the_form():
    from yolo_puncture_amd import YOLO
    assert YOLO("synthetic:m", attention="stream_wide").attention == "stream_wide" and YOLO("synthetic:m").attention == "auto"
    with pytest.raises(ValueError):
        YOLO("synthetic:m", attention="wide")


def test_a_batch_past_the_byte_bound_is_refused_as_such_under_the_form():
    """qkv of 2^31 bytes leaves the wide kernel's scope; the caller is told the byte bound (and the batch that fits), not the generic
    kernel's token bound behind it"""
    e = _m("stream_wide")
    mb = e.max_batch(2560, 1472)
    assert len(e.plan(mb, 2560, 1472)) > 0
    with pytest.raises(YolopError, match=rf"2\^31 bytes.*largest batch that fits is {mb}"):
        e.plan(mb + 1, 2560, 1472)
    e.close()


def test_a_refusal_names_the_form_that_would_hold_the_shape():
    e = _m("auto")
    with pytest.raises(YolopError, match=r"at most 2364 \(a streaming form is not built\).*stream_wide"):
        e.plan(1, 1408, 1760)
    e.close()
    e = _m("stream_wide", "fp32")
    with pytest.raises(YolopError) as err:
        e.plan(1, 1408, 1760)
    assert "stream_wide" not in str(err.value)
    e.close()
