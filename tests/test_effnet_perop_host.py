"""The per-op walk of tests/perop_effnet.py, exercised without a GPU. EmuClassifier serves tensors() / read_tensor() from the taps of
effnet_ref.forward (fp32: the unfolded conv + BatchNorm in torch's fp32 order, another correct ordering than the engine's; bf16: the
engine's storage format), which is what a correct engine looks like to the walk: it must pass every bound with room. Then one stored
tensor at a time is replaced by what a subtly wrong kernel would have written from the same inputs - the mistakes cls_pw / cls_dw /
cls_se / cls_fc can make at their tails and borders - and the walk must name that op."""
import pytest
import torch
import torch.nn.functional as F

import effnet_ref as R
import perop_effnet as pe
from yolo_puncture_amd import classify as C

ST = C.synthetic_state(0)
FRAMES, BOXES = pe.make_case()


class EmuClassifier:
    """tensors() / read_tensor() / out of a ClassifierEngine after one forward, computed on the CPU from effnet_ref.forward's taps"""

    def __init__(self, state, dtype, frames, boxes):
        self.dtype, self.state = dtype, state
        x = pe.ref_input(frames, boxes)
        self.t = {"input": x.permute(0, 2, 3, 1).contiguous()}
        logits = R.forward(state, x, dtype, tap=lambda n, t: self.t.__setitem__(n, t.float().permute(0, 2, 3, 1).contiguous())).float()
        self.out = self.tail(logits)

    @staticmethod
    def tail(logits, ge=False):
        cls = (logits[:, 1] >= logits[:, 0]) if ge else (logits[:, 1] > logits[:, 0])
        return logits, torch.softmax(logits, 1).max(1).values, cls.to(torch.int32)

    def tensors(self):
        return [dict(index=i, name=n, shape=tuple(t.shape)) for i, (n, t) in enumerate(self.t.items())]

    def read_tensor(self, name):
        return self.t[name].clone()

    def nchw(self, name):
        return self.t[name].permute(0, 3, 1, 2)

    def put(self, name, y):
        """replace one stored tensor (y NCHW), in the engine's storage format"""
        self.t[name] = (pe.bf16_round(y) if self.dtype == "bf16" and not name.endswith((".gate", "head.pool")) else y).permute(0, 2, 3, 1).contiguous()


def test_case_windows():
    """the case is what its docstring says: image 0's window is whole, image 1's is clipped on two sides, and its crop holds frame
    pixels, the short frame's zero padding and the crop's own zero padding"""
    H, W = FRAMES.shape[1:3]
    assert C.crop_geometry(BOXES[0], H, W)[2:] == (380, 380)
    x0, y0, cw, ch = C.crop_geometry(BOXES[1], H, W)
    assert (cw, ch) == (260, 260) and x0 + cw == W and y0 + ch == H
    crop = R.crop(FRAMES[1], BOXES[1])
    assert crop[:300 - y0, :360 - x0].any() and not crop[300 - y0:].any() and not crop[:, 360 - x0:].any() and 300 - y0 < ch


@pytest.fixture(scope="module")
def emus():
    return {dt: EmuClassifier(ST, dt, FRAMES, BOXES) for dt in ("fp32", "bf16")}


def _fresh(emus, dtype):
    e = object.__new__(EmuClassifier)
    e.dtype, e.state, e.t, e.out = dtype, emus[dtype].state, dict(emus[dtype].t), emus[dtype].out
    return e


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_correct_emulation_passes_with_room(emus, dtype):
    e = emus[dtype]
    stats, failures = pe.check_forward(e, ST, FRAMES, BOXES, dtype, out=e.out, label=f"emu {dtype}")
    print("\n".join(stats["rows"]))
    print("\n".join(pe.summarise(stats, f"emu {dtype}")))
    print(f"emu {dtype} worst: " + ", ".join(f"{k} {stats[k]:.3g}" for k in ("a", "b", "ulp", "frac", "d", "e", "f", "prob")))
    assert not failures, "\n".join(failures)
    assert len(stats["ops"]) == 1 + 4 * 26 - 2 + 2                                  # stem, 26 blocks (stage 1's two have no expand), pool, tail
    # another correct ordering sits well inside every bound
    assert stats["d"] < 0.5 and stats["e"] < 0.5 and stats["f"] < 0.5 and stats["prob"] <= pe.PROB_TOL / 2
    if dtype == "fp32":
        assert stats["a"] < 0.5 and stats["b"] < pe.RMS_FACTOR / 2
    else:
        assert stats["ulp"] <= 1.0 and stats["frac"] < pe.FRAC_CAP / 5


def test_se_gate_restatement_passes_its_bound(emus):
    """effnet_ref.se_gate in torch fp32 (the restatement test_gpu_classify.py compares gates with) is itself inside (d), on all 26
    blocks, from fp32 and from bf16-rounded depthwise maps"""
    worst = 0.0
    for dtype in ("fp32", "bf16"):
        for i in range(len(pe.BLOCKS)):
            p = f"_blocks.{i}"
            dw = emus[dtype].t[f"{p}.dw"]
            g64, dg = pe.gate_bounds(dw, *(ST[f"{p}.{k}"] for k in ("_se_reduce.weight", "_se_reduce.bias", "_se_expand.weight", "_se_expand.bias")))
            err = (R.se_gate(ST, p, dw.permute(0, 3, 1, 2))[:, :, 0, 0].double() - g64).abs()
            assert bool((err <= dg).all()), (dtype, p, float((err / dg).max()))
            worst = max(worst, float((err / dg).max()))
    print(f"effnet_ref.se_gate (torch fp32) against (d): worst |err| / bound {worst:.3f}")
    assert worst < 0.5


# ---- mutations: each rewrites one stored tensor of a copy of the emulation and returns the op that must be named --------------------------
def _ops(e, i):
    """the emulation's own per-op functions of block i, from its own stored tensors (teacher-forced, like the walk)"""
    p, bl, bf = f"_blocks.{i}", pe.BLOCKS[i], e.dtype == "bf16"
    q = pe.bf16_round if bf else (lambda w: w)
    inp = e.nchw("stem" if i == 0 else f"_blocks.{i - 1}")
    res = inp if (bl["s"] == 1 and bl["cin"] == bl["cout"]) else None

    def expand(x=inp):
        w, b = R.fold(ST, f"{p}._expand_conv", f"{p}._bn0")
        return R.swish(F.conv2d(x, q(w), b))

    def dw_pre(pp=R.pads()[f"{p}._depthwise_conv"]):
        w, b = R.fold(ST, f"{p}._depthwise_conv", f"{p}._bn1")
        x = e.nchw(f"{p}.expand") if bl["e"] != 1 else inp
        return F.conv2d(R._pad(x, pp), q(w), b, stride=bl["s"], groups=x.shape[1]), x, q(w)

    def project(xg=None, r=res):
        w, b = R.fold(ST, f"{p}._project_conv", f"{p}._bn2")
        xg = q(e.nchw(f"{p}.dw") * e.nchw(f"{p}.gate")) if xg is None else xg
        y = F.conv2d(xg, q(w), b)
        return (y if r is None else y + r), xg, q(w)

    def gate(mean):
        s = R.swish(F.conv2d(mean, ST[f"{p}._se_reduce.weight"], ST[f"{p}._se_reduce.bias"]))
        return torch.sigmoid(F.conv2d(s, ST[f"{p}._se_expand.weight"], ST[f"{p}._se_expand.bias"]))
    return dict(inp=inp, res=res, expand=expand, dw_pre=dw_pre, project=project, gate=gate, q=q)


def m_ktail(e):         # 1: the K % 32 = 8 tail. Stage 1 has no expand conv: the network's K = 40 1x1 conv is block 0's projection
    o = _ops(e, 0)
    xg = o["project"]()[1].clone()
    xg[:, 32:40] = 0.0
    e.put("_blocks.0", o["project"](xg)[0])
    return "_blocks.0"


def m_ktail_expand(e):  # 1': the same tail in an expand conv: K = 136 (stage 6's first block), the k-slice 128..135
    o = _ops(e, 18)
    x = o["inp"].clone()
    x[:, 128:136] = 0.0
    e.put("_blocks.18.expand", o["expand"](x))
    return "_blocks.18.expand"


def m_ntail(e):         # 2: N = 136: columns >= 128 take the neighbouring column
    y = _ops(e, 13)["project"]()[0].clone()
    y[:, 128:136] = y[:, 127:135].clone()
    e.put("_blocks.13", y)
    return "_blocks.13"


def m_stale_rows(e):    # 3: the last HW % 64 = 4 pixel rows of the 190^2 x 144 GEMM keep another forward's values
    y = e.nchw("_blocks.2.expand").clone().flatten(2)
    y[:, :, -(190 * 190 % 64):] = y.flip(0)[:, :, -(190 * 190 % 64):]
    e.put("_blocks.2.expand", y.view(2, 144, 190, 190))
    return "_blocks.2.expand"


def m_pad_380(e):       # 4: stage 6's first depthwise conv with the pad derived from the 380 input, (1, 2), not the configured 300's (2, 2)
    assert R.static_pad(24, 5, 2) == (1, 2) and R.pads()["_blocks.18._depthwise_conv"] == (2, 2)
    e.put("_blocks.18.dw", R.swish(_ops(e, 18)["dw_pre"]((1, 2))[0]))
    return "_blocks.18.dw"


def m_border_tap(e):    # 5: k5 s2 (block 5, 95 -> 48, pad 2): tap (2, 2) of the last output row dropped; it reads input row 94, the map's last
    z, x, w = _ops(e, 5)["dw_pre"]()
    one = torch.zeros_like(w)
    one[:, :, 2, 2] = w[:, :, 2, 2]
    z = z.clone()
    z[:, :, -1] -= F.conv2d(R._pad(x, (2, 2)), one, None, stride=2, groups=x.shape[1])[:, :, -1]
    e.put("_blocks.5.dw", R.swish(z))
    return "_blocks.5.dw"


def m_gate_skipped(e):  # 6: one 8-channel group of the K operand is not gated
    o = _ops(e, 13)
    xg = o["project"]()[1].clone()
    xg[:, 8:16] = e.nchw("_blocks.13.dw")[:, 8:16]
    e.put("_blocks.13", o["project"](xg)[0])
    return "_blocks.13"


def m_res_other_image(e):   # 7
    o = _ops(e, 25)
    e.put("_blocks.25", o["project"](r=o["res"].flip(0))[0])
    return "_blocks.25"


def m_se_mean_hin(e):   # 8: stride-2 block 5: the squeeze divides by Hin Win = 95^2, not Hout Wout = 48^2
    dw = e.nchw("_blocks.5.dw")
    e.put("_blocks.5.gate", _ops(e, 5)["gate"](dw.sum((2, 3), keepdim=True) / (95 * 95)))
    return "_blocks.5.gate"


def m_se_chunk_lost(e):  # 9: one row chunk (an output row) left out of the squeeze
    dw = e.nchw("_blocks.20.dw")
    e.put("_blocks.20.gate", _ops(e, 20)["gate"]((dw.sum((2, 3), keepdim=True) - dw[:, :, 7:8].sum((2, 3), keepdim=True)) / (dw.shape[2] * dw.shape[3])))
    return "_blocks.20.gate"


def m_pool_chunk_lost(e):   # 10: the pool's last, partial 32-row chunk (pixels 128..143 of 144) dropped
    w, b = R.fold(ST, "_conv_head", "_bn1")
    y = R.swish(F.conv2d(e.nchw("_blocks.25"), _ops(e, 25)["q"](w), b)).flatten(2)
    e.put("head.pool", (y[:, :, :128].sum(2) / 144)[:, :, None, None])
    return "head.pool"


def m_truncate(e):      # 11: bf16 stored by truncation, not round-to-nearest-even
    y = _ops(e, 8)["expand"]()
    e.t["_blocks.8.expand"] = (y.contiguous().view(torch.int32) & -65536).view(torch.float32).permute(0, 2, 3, 1).contiguous()
    return "_blocks.8.expand"


def m_bf16_product(e):  # 12: fp32 GEMM (K = 2304) with one product per output taken in bf16
    y, xg, w = _ops(e, 25)["project"]()
    p = xg[:, 5:6] * w[None, :, 5, :, :].view(1, -1, 1, 1)
    e.put("_blocks.25", y + (pe.bf16_round(p) - p))
    return "_blocks.25"


def m_cls_ge(e):        # 13: the tie: l1 >= l0 gives 1, the contract 0
    e.state = dict(e.state, **{"_fc.weight": torch.zeros(2, 1536), "_fc.bias": torch.zeros(2)})
    e.out = EmuClassifier.tail(torch.zeros(2, 2), ge=True)
    return "tail"


MUTATIONS = [(m_ktail, ("fp32", "bf16"), None), (m_ktail_expand, ("fp32", "bf16"), None), (m_ntail, ("fp32", "bf16"), None),
             (m_stale_rows, ("fp32", "bf16"), None), (m_pad_380, ("fp32", "bf16"), None), (m_border_tap, ("fp32", "bf16"), None),
             (m_gate_skipped, ("fp32", "bf16"), None), (m_res_other_image, ("fp32", "bf16"), None), (m_se_mean_hin, ("fp32", "bf16"), "(d)"),
             (m_se_chunk_lost, ("fp32", "bf16"), "(d)"), (m_pool_chunk_lost, ("fp32", "bf16"), "(e)"), (m_truncate, ("bf16",), "(c)"),
             (m_bf16_product, ("fp32",), "(b)"), (m_cls_ge, ("fp32", "bf16"), "(f)")]


@pytest.mark.parametrize("mutation,dtype,bound", [pytest.param(m, dt, bd, id=f"{m.__name__[2:]}-{dt}") for m, dts, bd in MUTATIONS for dt in dts])
def test_wrong_emulation_is_named(emus, mutation, dtype, bound):
    clean, e = _fresh(emus, dtype), _fresh(emus, dtype)
    op = mutation(e)
    if op == "tail":                                                       # the tie state, with the contract's class
        clean.state, clean.out = e.state, EmuClassifier.tail(torch.zeros(2, 2))
    _, before = pe.check_forward(clean, clean.state, FRAMES, BOXES, dtype, out=clean.out, ops=[op])
    assert not before, before                                              # the op passes before the mutation ...
    _, failures = pe.check_forward(e, e.state, FRAMES, BOXES, dtype, out=e.out, ops=[op], label="emu")
    print("\n".join(failures))
    assert failures and all(f"op '{op}'" in f for f in failures), failures      # ... and is the one named after it
    if bound is not None:
        assert all(f"{bound} violated" in f or (bound == "(f)" and "(f)" in f) for f in failures), failures


def test_tail_bounds_catch_wrong_logits_and_prob(emus):
    e = emus["fp32"]
    pool = e.t["head.pool"][:, 0, 0, :]
    logits, prob, cls = e.out
    assert not pe.tail_failures(ST, pool, e.out)[2]
    assert pe.tail_failures(ST, pool, (logits + 1e-3, prob, cls))[2]              # 32 u (sum |w p| + |b|) is ~1e-4 with the synthetic FC's gain
    assert pe.tail_failures(ST, pool, (logits, prob + 4e-7, cls))[2]
    assert pe.tail_failures(ST, pool, (logits, prob, 1 - cls))[2]
    sat = torch.tensor([[50.0, -50.0], [-50.0, 50.0]])
    st = dict(ST, **{"_fc.weight": torch.zeros(2, 1536), "_fc.bias": torch.tensor([50.0, -50.0])})
    assert not pe.tail_failures(st, pool, EmuClassifier.tail(sat[:1].expand(2, 2)))[2]
    assert EmuClassifier.tail(sat)[1].tolist() == [1.0, 1.0] and EmuClassifier.tail(sat)[2].tolist() == [0, 1]
