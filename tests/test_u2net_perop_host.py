"""The per-op walk of tests/perop_u2net.py, exercised without a GPU: the plan comes from the library's own graph builder
(yp_u2net_op_info needs no device), the tensors from a plain torch emulation of every op in the engine's storage format. A correct
emulation - another fp32 summation order than the fp64 reference, so what a correct kernel looks like to the walk - must pass every bound
with room to spare; a tensor the engine would not have written is poisoned with NaN, so a walk that read it fails; and subtly wrong
emulations (one weight tap dropped, the half-pixel offset of the up-sample dropped, the residual added before the ReLU) must be named."""
import pytest
import torch
import torch.nn.functional as F

import perop_u2net as pu
from helpers import rand_image
from yolo_puncture_amd.u2net import U2NetEngine

SHAPE = (1, 33, 47)


class EmuEngine:
    """ops() / tensors() / read_tensor() of a U2NetEngine after one forward, computed on the CPU. fused: every conv that can take its pool
    / up-sample while loading does (impl 2) and that pool / up-sample does not run; otherwise impl 0 everywhere."""

    def __init__(self, variant, dtype, folded, im, fused, mutate=None):
        real = U2NetEngine(variant, dtype, 0)                 # graph only: no weights, no device
        self._ops, names = real.ops(), [(t["name"], t["shape"][3]) for t in real.tensors()]
        real.close()
        self.bf = dtype == "bf16"
        mutate = mutate or {}
        store = (lambda x, name: x if not self.bf or name in pu.SIDES else pu.bf16_round(x))
        buf = {}
        B = im.shape[0]

        def out(v, y):                                         # y NCHW
            t, c0, c = v
            if t not in buf:
                buf[t] = torch.full((B, y.shape[2], y.shape[3], names[t][1]), float("nan"))
            buf[t][..., c0:c0 + c] = store(y, names[t][0]).permute(0, 2, 3, 1)

        def view(v):
            t, c0, c = v
            return pu.nchw(buf[t][..., c0:c0 + c])

        for o in self._ops:
            if o["kind"] == "conv":
                o["impl"] = 2 if fused and (o["pool_op"] >= 0 or o["up_op"] >= 0) else (1 if fused else 0)
        for o in self._ops:
            if o["kind"] == "input":
                x = im.flip(-1).permute(0, 3, 1, 2).float() / 255.0
                out(o["out"], torch.cat((x, torch.zeros(B, 5, *x.shape[2:])), 1))
            elif o["kind"] == "pool":
                if not (o["consumer"] >= 0 and self._ops[o["consumer"]]["impl"] == 2):
                    out(o["out"], F.max_pool2d(view(o["in"]), 2, 2, ceil_mode=True))
            elif o["kind"] == "up":
                if not (o["consumer"] >= 0 and self._ops[o["consumer"]]["impl"] == 2):
                    out(o["out"], self._up(view(o["in"]), buf[o["out"][0]].shape[1:3], mutate))
            else:
                if o["impl"] == 2 and o["pool_op"] >= 0:
                    x = F.max_pool2d(view(self._ops[o["pool_op"]]["in"]), 2, 2, ceil_mode=True)
                elif o["impl"] == 2:
                    u = self._ops[o["up_op"]]
                    t, _, c = o["in"]
                    hi = store(self._up(view(u["in"]), buf[t].shape[1:3], mutate), "")
                    x = torch.cat((hi, view((t, u["out"][2], c - u["out"][2]))), 1)
                else:
                    x = view(o["in"])
                w, b = folded[o["name"]]
                w = pu.bf16_round(w) if self.bf else w
                if mutate.get("drop_tap", ("",))[0] == o["name"]:          # one (input channel, tap) pair of the weights
                    w = w.clone()
                    w[:, int(x[:, :o["cin"]].abs().mean((0, 2, 3)).argmax()), mutate["drop_tap"][1], mutate["drop_tap"][2]] = 0.0   # (of a live channel)
                y = F.conv2d(x[:, :o["cin"]], w, b, padding=o["dil"], dilation=o["dil"])
                if o["res"][0] >= 0 and mutate.get("res_before_act") == o["name"]:
                    y = (y + view(o["res"])).relu()
                else:
                    y = y.relu() if o["act"] == 2 else y
                    y = y + view(o["res"]) if o["res"][0] >= 0 else y
                out(o["out"], y)
        self._buf = buf
        self._names = names

    @staticmethod
    def _up(x, size, mutate):
        if mutate.get("up_no_half"):                          # another sampling grid than align_corners=False, as with its half-pixel offset lost
            return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)
        return pu.bilinear_f32(x.contiguous(), *size)         # the engine's operation order (kernel_util.h: bilinear_tap, bilinear_blend)

    def ops(self):
        return self._ops

    def tensors(self):
        return [dict(index=i, name=n, shape=tuple(self._buf[i].shape) if i in self._buf else (0, 0, 0, c)) for i, (n, c) in enumerate(self._names)]

    def read_tensor(self, name):
        i = [n for n, _ in self._names].index(name)
        return self._buf[i].clone()

    def tail(self, folded):
        wf, b = folded["outconv"]
        H, W = self._buf[0].shape[1:3]
        maps = [F.interpolate(pu.nchw(self.read_tensor(n)), size=(H, W), mode="bilinear", align_corners=False) for n in pu.SIDES]
        prob = torch.sigmoid(F.conv2d(torch.cat(maps, 1), wf, b))[:, 0]
        norm = (prob - prob.min()) / (prob.max() - prob.min())
        return prob, norm, (norm > 0.5).to(torch.uint8) * 255


@pytest.fixture(scope="module")
def case():
    _, folded = pu.case_state("p")
    return folded, rand_image(SHAPE + (3,), seed=5)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fused", [False, True])
def test_correct_emulation_passes_with_room(case, dtype, fused):
    folded, im = case
    e = EmuEngine("p", dtype, folded, im, fused)
    stats, failures = pu.check_forward(e, "p", dtype, folded, "emu")
    failures += pu.check_tail(e, folded, *e.tail(folded), "emu")
    assert not failures, "\n".join(failures)
    assert stats["impls"] == ([1, 2] if fused else [0])
    assert (stats["fused_pool"] > 0 and stats["fused_up"] > 0) if fused else (stats["fused_pool"] == stats["fused_up"] == 0)
    # another correct fp32 ordering (the emulation convolves channels-last views, the walk's fp32 reference contiguous tensors) sits far
    # inside (a), and inside (b) or the walk had reported it
    assert stats["a"] < 0.25 and stats["b"] < pu.RMS_FACTOR and stats["frac"] < 0.005
    print(dtype, fused, {k: stats[k] for k in ("a", "b", "ulp", "frac")})


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mutate,op", [({"drop_tap": ("stage5.rebnconv4", 1, 1)}, "stage5.rebnconv4"),     # dilation 8 on the 3x3 map: only the centre tap is inside
                                       ({"drop_tap": ("stage1d.rebnconv2d", 0, 2)}, "stage1d.rebnconv2d"),  # a conv that fuses its up-sample
                                       ({"res_before_act": "stage2.rebnconv1d"}, "stage2.rebnconv1d"),
                                       ({"up_no_half": True}, None)])
def test_wrong_emulation_is_named(case, dtype, mutate, op):
    folded, im = case
    for fused in (False, True):
        e = EmuEngine("p", dtype, folded, im, fused, mutate)
        _, failures = pu.check_forward(e, "p", dtype, folded, "emu")
        assert failures, (mutate, fused)
        if op is not None:
            assert all(f"'{op}'" in f for f in failures), failures           # that op, and no other: every op is judged on its own inputs
        else:
            assert all((" up " in f) or (" impl 2" in f) for f in failures), failures


def test_tail_checks_catch_a_wrong_range_and_threshold(case):
    folded, im = case
    e = EmuEngine("p", "fp32", folded, im, False)
    prob, norm, mask = e.tail(folded)
    assert not pu.check_norm(prob, norm, mask)
    wide = (prob - prob.min() * 0.999) / (prob.max() - prob.min() * 0.999)
    assert pu.check_norm(prob, wide, (wide > 0.5).to(torch.uint8) * 255)
    flipped = mask.clone()
    flipped.view(-1)[int((norm - 0.5).abs().argmin())] ^= 255
    assert pu.check_norm(prob, norm, flipped)
    assert pu.check_tail(e, folded, prob + 3e-6, norm, mask)
