"""The fused launch forms of a plan, as yp_debug_op_form reports them from the form table (csrc/engine.hip kForms): every op that launches
nothing is accounted for by exactly one launching op, the work it reported moved to that op, and the depthwise / stem kernel names a plan
reports are kernels libyolop.so contains. Plans are host-side: no GPU needed."""
import json
import os
import subprocess
import sys

import pytest

from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import Engine, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("v10", "n", False), ("v10", "n", True), ("v10", "s", False), ("v10", "s", True), ("11", "n", True), ("11", "s", True)]   # (family, variant, seg)
# (1, 64, 128) besides the two small frames: conv_dwpw works in 8 x 16-pixel tiles and refuses a map it would pad by more than half, so the
# dw -> pw form first occurs where the P3 map (1/8 of the frame) is a whole tile; at 8 x 8 and 12 x 20 those pairs run as pwsp or apart
SHAPES = [(1, 64, 64), (2, 96, 160), (1, 64, 128)]
KEYS = [(c, s) for c in CASES for s in SHAPES]
# What each form takes over, written down here and not read from the table: the kinds of the absorbed ops, in the order the kernel runs them
# (the TAIL form with or without the class-max keys). A record that lists an op too few or too many fails this.
ABSORBS = {"dwpw": [("dwconv",)], "dwpw_tail": [("dwconv", "conv"), ("dwconv", "conv", "amax")], "s2pw": [("conv",)], "frontend": [("stem", "conv")],
           "c2f": [("conv", "conv")], "scdown": [("conv",)], "pwsp": [("conv",)], "cls_out": [("amax",)]}


def _plans():
    out = {}
    for fam, v, seg in CASES:
        e = Engine(v, 80, seg, "bf16", 0, family=fam)
        for s in SHAPES:
            out[((fam, v, seg), s)] = e.plan(*s)
        e.close()
    return out


@pytest.fixture(scope="module")
def fused():
    assert os.environ.get("YOLOP_NO_FUSE") != "1"
    return _plans()


@pytest.fixture(scope="module")
def unfused():
    """The same plans with every form off. YOLOP_NO_FUSE is read at yp_create and the per-form switches once per process: a child process."""
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_plan_forms_host as t; "
            "print(json.dumps([[o['flops'] for o in p] for p in t._plans().values()]))" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, YOLOP_NO_FUSE="1"), capture_output=True, text=True, check=True)
    return dict(zip(KEYS, json.loads(r.stdout.splitlines()[-1])))


def _dense_head_branch(o):
    """A box / mask-coefficient conv of the v10 head: dense in the op list, evaluated at the winners only inside the head op."""
    return o["kind"] == "conv" and o["name"].startswith(("model.23.one2one_cv2.", "model.23.cv4."))


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "%s-%s-%s-%dx%dx%d" % (k[0][0], k[0][1], "seg" if k[0][2] else "det", *k[1]))
def test_absorbed_ops_are_accounted_for(key, fused, unfused):
    ops, plain = fused[key], unfused[key]
    assert len(plain) == len(ops)
    owner = {}
    for i, o in enumerate(ops):
        assert (o["form"] == "plain") == (not o["absorbed"]), (o["name"], o["form"], o["absorbed"])
        if o["kernel"] == "-":
            assert o["form"] == "plain" and o["flops"] == 0 and o["bytes"] == 0, o          # launches nothing, reports nothing
            continue
        if o["absorbed"]:
            assert tuple(ops[a]["kind"] for a in o["absorbed"]) in ABSORBS[o["form"]], (o["name"], o["form"], o["absorbed"])
        for a in o["absorbed"]:
            assert a not in owner, (ops[a]["name"], "absorbed by", ops[owner[a]]["name"], "and", o["name"])
            owner[a] = i
            assert ops[a]["kernel"] == "-", (ops[a]["name"], "is absorbed by", o["name"], "and launches", ops[a]["kernel"])
        # the work moved: at least what the op and its absorbed ops report as plain launches
        assert o["flops"] >= plain[i] + sum(plain[a] for a in o["absorbed"]), (o["name"], o["form"])
    # the only ops that launch nothing without a form taking them over: a folded upsample, the dense convs of a winners-only head branch
    for i, o in enumerate(ops):
        if o["kernel"] == "-" and i not in owner:
            assert o["kind"] == "upsample" or _dense_head_branch(o), (o["name"], o["kind"])
    for i in owner:
        assert ops[i]["kind"] != "upsample" and not _dense_head_branch(ops[i]), ops[i]["name"]


def test_every_form_occurs(fused):
    seen = {o["form"] for ops in fused.values() for o in ops}
    assert {"dwpw", "s2pw", "c2f", "scdown", "pwsp", "cls_out"} <= seen, seen


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_depthwise_and_stem_names_are_kernel_symbols(fused):
    syms = _kernel_symbols(load_library()._name)
    names = {o["kernel"] for ops in fused.values() for o in ops if o["kernel"].startswith(("dwconv_", "stem_"))}
    assert any(n.startswith("dwconv_") for n in names) and any(n.startswith("stem_") for n in names), names
    for n in sorted(names):
        assert n.replace(" ", "") in syms, n
