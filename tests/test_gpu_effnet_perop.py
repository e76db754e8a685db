"""Every kernel of csrc/effnet.hip held to the per-op contract of tests/perop_effnet.py on the MI355X, fp32 and bf16: one B = 2 forward
per dtype (an interior window and one clipped on two sides, perop_effnet.make_case), then stem, each of the 7 stages and head + tail
against references of each op alone built from the engine's own stored tensors. The network's fixed shapes already hold the edges:
HW % 64 in {4, 1, 0, 16}, K % 32 in {8, 24, 16, 0}, N % 32 != 0 (40, 24, 48, 136, 232), k3 / k5, s1 / s2 with asymmetric static pads.
The FC / softmax / argmax tail, which synthetic_state(0) only ever drives to class 0 with a 0.015 margin, gets crafted `_fc` states:
the tie, class 1, both saturations, and a direction that separates the two images, which also feeds the insertion search a class list
that is not all zeros."""
import os

import numpy as np
import pytest
import torch

import effnet_ref as R
import perop_effnet as pe
from yolo_puncture_amd import classify as C

pytestmark = pytest.mark.gpu

ST = C.synthetic_state(0)
FRAMES, BOXES = pe.make_case()
PARTS = {"stem": ["stem"], **{f"stage{s}": pe.stage_ops(s) for s in range(1, 8)}, "head+tail": ["head.pool", "tail"]}


def _forward(eng, frames, boxes):
    out = eng.forward(torch.from_numpy(frames).cuda(), torch.tensor(boxes, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def _engine_run(dtype):
    old = os.environ.get("YOLOP_CLS_TAP_INPUT")
    os.environ["YOLOP_CLS_TAP_INPUT"] = "1"              # read by yp_cls_create: keeps the 'input' tap for (g)
    try:
        eng = C.ClassifierEngine(dtype, 0, state=ST)
    finally:
        if old is None:
            del os.environ["YOLOP_CLS_TAP_INPUT"]
        else:
            os.environ["YOLOP_CLS_TAP_INPUT"] = old
    return eng, _forward(eng, FRAMES, BOXES)


@pytest.fixture(scope="module")
def run_fp32():
    eng, out = _engine_run("fp32")
    yield eng, out
    eng.close()


@pytest.fixture(scope="module")
def run_bf16():
    eng, out = _engine_run("bf16")
    yield eng, out
    eng.close()


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_per_op_contract(request, dtype, part):
    eng, out = request.getfixturevalue(f"run_{dtype}")
    label = f"[{dtype} {part}]"
    stats, failures = pe.check_forward(eng, ST, FRAMES, BOXES, dtype, out=out, ops=PARTS[part], label=label)
    print("\n".join(stats["rows"]))
    print("\n".join(pe.summarise(stats, label + " SUMMARY")))
    assert not failures, f"{len(failures)} violations:\n" + "\n".join(failures)
    assert set(stats["ops"]) == set(PARTS[part])


# ---- crafted tails ----------------------------------------------------------------------------------------------------------------------
def _fc_state(w, b):
    return dict(ST, **{"_fc.weight": w.float().contiguous(), "_fc.bias": torch.as_tensor(b, dtype=torch.float32)})


def _separating(P, centred):
    """row 1 = -row 0 = d / |d|^2 with d = P[0] - P[1]: the two images' margins l1 - l0 = 2 d.P_b / |d|^2 differ by exactly 2. With zero
    bias they straddle 0 only if | |P0|^2 - |P1|^2 | < |d|^2, which two pooled vectors of a common large mean do not satisfy (here
    |P|^2 ~ 83, |d|^2 ~ 0.04: both margins ~ +30); `centred` adds the bias -/+ (m0 + m1) / 4 that puts them at +1 and -1."""
    P = P.double()
    d = P[0] - P[1]
    w1 = d / d.dot(d)
    m = 2 * (P @ w1)
    b1 = -float(m.sum()) / 4 if centred else 0.0
    w = torch.stack((-w1, w1))
    b = torch.tensor([-b1, b1], dtype=torch.float64)
    margin = (P @ w.float().double().T + b.float().double()) @ torch.tensor([-1.0, 1.0], dtype=torch.float64)     # of the fp32 parameters, in fp64
    return _fc_state(w, b), margin


ZERO_W = torch.zeros(2, 1536)
TAILS = ["tie", "class1", "sat0", "sat1", "direction", "direction_centred"]


def _tail_state(kind, P):
    if kind == "tie":
        return _fc_state(ZERO_W, [0.0, 0.0]), None
    if kind == "class1":
        return _fc_state(ZERO_W, [-1.0, 1.0]), None
    if kind == "sat0":
        return _fc_state(ZERO_W, [50.0, -50.0]), None
    if kind == "sat1":
        return _fc_state(ZERO_W, [-50.0, 50.0]), None
    return _separating(P, kind == "direction_centred")


@pytest.mark.parametrize("kind", TAILS)
def test_crafted_tail(run_fp32, kind):
    """engines that differ only in _fc.*; all held to (f), plus what each state makes exact"""
    P = run_fp32[0].read_tensor("head.pool")[:, 0, 0, :]
    state, margin = _tail_state(kind, P)
    eng = C.ClassifierEngine("fp32", 0, state=state)
    try:
        out = _forward(eng, FRAMES, BOXES)
        logits, prob, cls = out
        assert torch.equal(eng.read_tensor("head.pool")[:, 0, 0, :], P)            # the rest of the state is shared: the same pool, bit for bit
        stats, failures = pe.check_forward(eng, state, FRAMES, BOXES, "fp32", out=out, ops=["tail"], label=f"[tail {kind}]")
        print("\n".join(stats["rows"]), cls.tolist(), prob.tolist(), None if margin is None else margin.tolist())
        assert not failures, "\n".join(failures)
        if kind == "tie":
            assert torch.equal(logits, torch.zeros(2, 2)) and cls.tolist() == [0, 0] and prob.tolist() == [0.5, 0.5]
        elif kind == "class1":
            assert torch.equal(logits, torch.tensor([[-1.0, 1.0]] * 2)) and cls.tolist() == [1, 1]
            assert float((prob.double() - torch.sigmoid(torch.tensor(2.0, dtype=torch.float64))).abs().max()) <= pe.PROB_TOL
        elif kind in ("sat0", "sat1"):
            assert bool(torch.isfinite(logits).all()) and prob.tolist() == [1.0, 1.0] and cls.tolist() == [int(kind == "sat1")] * 2
        else:
            assert float(margin.abs().min()) > 1e-3, margin                         # the fp64 margin decides before the class is trusted
            assert cls.tolist() == (margin > 0).long().tolist()
            assert abs(float(margin[0] - margin[1]) - 2.0) < 1e-4
            if kind == "direction_centred":
                assert cls.tolist() == [1, 0] and float((margin.abs() - 1.0).abs().max()) < 1e-3
                want = torch.sigmoid(margin.abs())
                assert float((prob.double() - want).abs().max()) < 1e-4           # |l1 - l0| = 1: prob = sigmoid(1) = 0.731, between the 0.7 and 0.8 thresholds
    finally:
        eng.close()


# hand-chosen: the first window with >= 18 class-1 frames starts at 2 (frames 3 and 8 are class 0), and its first run of five class-1
# frames starts at 9; sigmoid(1) = 0.731 passes the 0.7 threshold only. The repair then rewrites frames 2, 4..7 to 0 and 22 to 1.
PATTERN = [0, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]


def test_insertion_search_on_a_mixed_class_list(run_fp32):
    P = run_fp32[0].read_tensor("head.pool")[:, 0, 0, :]
    state, margin = _separating(P, True)
    assert margin[0] > 0.9 and margin[1] < -0.9
    which = [0 if c == 1 else 1 for c in PATTERN]                                  # image 0 lands on class 1, image 1 on class 0
    frames, boxes = FRAMES[which], [BOXES[i] for i in which]
    eng = C.ClassifierEngine("fp32", 0, state=state)
    try:
        _, prob, cls = _forward(eng, frames, boxes)
        cl, pl = [int(c) for c in cls], list(prob.numpy())
        assert cl == PATTERN
        res = [C.predict_and_find_start_inserted(eng, list(frames), boxes, judge_wnd=20, batch_size=bs) for bs in (8, 5)]
    finally:
        eng.close()
    idx = R.find_start(cl, pl, 20)
    assert idx == 9
    cl, pl = R.repair(cl, pl, idx)
    assert cl == [0] * 9 + [1] * 15
    for r in res:
        assert r[2] == idx and [int(c) for c in r[0]] == cl and np.array_equal(np.array(r[1]), np.array(pl))
