"""The streaming attention form, host side (no GPU): the reference pair alone stays inside the contract on every stand-alone case of
attention_stream_cases.py (so a failure of test_gpu_attention_stream.py is the kernel's), and the planner takes the form only where an
engine asked for it and the kernel's scope holds - everything else plans, names and refuses as a default engine does."""
import pytest
import torch

import attention_ref as A
import attention_stream_cases as S
from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import EXPORTS, Engine, YolopError, load_library

SHAPES_PAST_THE_GENERIC_LIMIT = ((1, 2560, 1472), (1, 2176, 3840))      # 3680 and 8160 tokens


@pytest.mark.parametrize("case", S.CASES, ids=A.case_id)
def test_reference_pair_stays_in_contract(case):
    """the oracle's float32 restatement against the fp64 reference; measured over the list: worst / allowed <= 0.90, <= 0.19 % of the
    elements differing, <= 0.02 % above 1 ulp - the caps (2 %, 0.5 %) are reachable and leave a broken kernel no room"""
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    assert qkv.dtype == torch.bfloat16 and bool(torch.isfinite(want).all())
    o32 = A.oracle_expression(qkv, nh, kd, hd, torch.float32, "bf16")
    A.assert_bf16_contract(f"float32 restatement {A.case_id(case)}", o32, want, P, v, dist)
    if dist == "lookup":
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        assert float((want == exp).double().mean()) > 0.999
        assert bool((o32.double()[want == exp] == exp[want == exp]).all())


def test_split_formula():
    assert S.groups_per_workgroup(2, 1025, 2) == (9, 1)
    assert [S.groups_per_workgroup(2, 1025, 2, w) for w in (4, 8, 12, 20)] == [(1, 9), (2, 5), (3, 3), (5, 2)]
    assert S.groups_per_workgroup(1, 3680, 2) == (29, 1) and S.groups_per_workgroup(32, 1600, 4) == (2, 7)


def _attn(ops):
    got = [o for o in ops if o["name"].endswith(".attn.o")]
    assert len(got) == 1
    return got[0]


def _engines(**kw):
    return (("v10-n detect", lambda: Engine("n", 80, False, "bf16", 0, **kw)), ("11-n seg", lambda: Engine("n", 80, True, "bf16", 0, family="11", **kw)))


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_the_planned_name_is_a_kernel_symbol():
    assert "attention_stream_kernel" in _kernel_symbols(load_library()._name)


def test_stream_engines_plan_past_the_generic_limit():
    for what, make in _engines(attention="stream"):
        e, d = make(), make()
        d.set_attention_form("auto")
        for B, H, W in SHAPES_PAST_THE_GENERIC_LIMIT:
            op = _attn(e.plan(B, H, W))
            assert op["kernel"] == "attention_stream_kernel", (what, H, W, op["kernel"])
            N = (H // 32) * (W // 32)
            nh = op["out"][2] // 64
            assert op["flops"] == 2.0 * B * nh * N * N * (32 + 32 + 64), "Q.K^T counts twice: the kernel computes it in both passes"
            assert e.lib.yp_debug_host_selftest(e._h) > 0, (what, e.lib.yp_last_error())
        # 400 tokens: the resident kernel's, under either form
        assert _attn(e.plan(1, 640, 640))["kernel"] == _attn(d.plan(1, 640, 640))["kernel"]
        assert _attn(e.plan(1, 640, 640))["flops"] == _attn(d.plan(1, 640, 640))["flops"]
        # between the two limits the form changes the kernel and nothing else of the plan
        pe, pd = e.plan(1, 1088, 1920), d.plan(1, 1088, 1920)
        assert _attn(pe)["kernel"] == "attention_stream_kernel" and _attn(pd)["kernel"] == "attention_kernel"
        assert [(o["name"], o["kernel"]) for o in pe if not o["name"].endswith(".attn.o")] == \
               [(o["name"], o["kernel"]) for o in pd if not o["name"].endswith(".attn.o")]
        e.close()
        d.close()


def test_default_engines_refuse_as_before():
    for what, make in _engines():
        e = make()
        with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)"):
            e.plan(1, 2560, 1472)
        assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
        e.close()


def test_out_of_scope_engines_keep_the_generic_limit_under_the_form():
    e = Engine("n", 80, False, "fp32", 0, attention="stream")
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368 \(a streaming form is not built\)"):
        e.plan(1, 2560, 1472)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.close()
    e = Engine("m", 80, False, "bf16", 0, attention="stream")                  # key_dim 36
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2364 \(a streaming form is not built\)"):
        e.plan(1, 2560, 1472)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.close()


def test_a_batch_past_the_byte_bound_is_refused_as_such_under_the_form():
    """qkv of 2^31 bytes leaves the streaming kernel's scope; the caller is told the byte bound (and the batch that fits), not the generic
    kernel's token bound behind it"""
    for what, make in _engines(attention="stream"):
        e = make()
        mb = e.max_batch(2560, 1472)
        assert len(e.plan(mb, 2560, 1472)) > 0
        with pytest.raises(YolopError, match=rf"2\^31 bytes.*largest batch that fits is {mb}"):
            e.plan(mb + 1, 2560, 1472)
        e.close()


def test_form_values_and_a_change_drops_the_plan():
    e = Engine("n", 80, False, "bf16", 0)
    for bad in (2, -1, 7):
        assert e.lib.yp_set_attention_form(e._h, bad) < 0 and b"yp_set_attention_form" in e.lib.yp_last_error()
    assert e.lib.yp_set_attention_form(None, 1) < 0
    with pytest.raises(ValueError):
        e.set_attention_form("flash")
    with pytest.raises(ValueError):
        Engine("n", 80, False, "bf16", 0, attention="flash")
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.set_attention_form("stream")                                             # the same shape plans again, under the new form
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_stream_kernel"
    assert len(e.plan(1, 2560, 1472)) > 0
    e.set_attention_form("auto")
    with pytest.raises(YolopError, match="3680 attention tokens"):
        e.plan(1, 2560, 1472)
    assert _attn(e.plan(1, 1088, 1920))["kernel"] == "attention_kernel"
    e.close()


def test_environment_sets_the_form_at_create(monkeypatch):
    monkeypatch.setenv("YOLOP_ATTN_FORM", "stream")
    e = Engine("n", 80, False, "bf16", 0)
    monkeypatch.delenv("YOLOP_ATTN_FORM")
    d = Engine("n", 80, False, "bf16", 0)
    assert _attn(e.plan(1, 2560, 1472))["kernel"] == "attention_stream_kernel"        # read at yp_create, per engine
    with pytest.raises(YolopError, match=r"3680 attention tokens.*at most 2368"):
        d.plan(1, 2560, 1472)
    e.set_attention_form("auto")                                                       # an explicit call overrides what the variable said
    with pytest.raises(YolopError, match="3680 attention tokens"):
        e.plan(1, 2560, 1472)
    e.close()
    d.close()
    monkeypatch.setenv("YOLOP_ATTN_FORM", "flash")
    with pytest.raises(YolopError, match="YOLOP_ATTN_FORM"):
        Engine("n", 80, False, "bf16", 0)


def test_facade_keys_its_engines_by_the_form():
    from yolo_puncture_amd import YOLO
    with pytest.raises(ValueError):
        YOLO("synthetic:n", attention="flash")
    assert YOLO("synthetic:n").attention == "auto" and YOLO("synthetic:n", attention="stream").attention == "stream"


def test_exports_name_the_new_calls():
    assert {"yp_set_attention_form", "yp_debug_attention_form"} <= set(EXPORTS)
