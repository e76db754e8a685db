"""Every U^2-Net kernel held to the per-op contract of tests/perop_u2net.py, fp32 and bf16, under each forced conv
policy and under the tuner's own choice, at the smallest shapes that reach the edges:
  (1, 33, 47): every level odd or clipped (33x47, 17x24, 9x12, 5x6, 3x3, 2x2): partial conv_halo_f32 tiles in both directions, conv_small
               with M = 4, dilations 4 and 8 larger than the map;
  (3, 35, 33): batch > 1: conv_small workgroups span images (12 pixels at level 5), the fused up-sample's per-lane image index.
Variant 'p' runs both, variant 'f' the first (FN = 2 of conv_small / conv_halo_f32, the 128 .. 1024-channel conv_igemm layers).
The coverage assertions keep a case from passing by checking nothing: all 118 convs are walked, and each policy must show the impls it
is there for (U2NetEngine.ops())."""
import pytest
import torch

import perop_u2net as pu
from helpers import rand_image

pytestmark = pytest.mark.gpu

GRAPHS = [("p", (1, 33, 47)), ("p", (3, 35, 33)), ("f", (1, 33, 47))]
MODES = [("igemm", "fp32"), ("igemm", "bf16"), ("small_fused", "fp32"), ("small_fused", "bf16"), ("small_unfused", "fp32"),
         ("small_unfused", "bf16"), ("halo", "fp32"), ("tuned", "fp32"), ("tuned", "bf16")]


@pytest.mark.parametrize("variant,shape", GRAPHS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
@pytest.mark.parametrize("policy,dtype", MODES)
def test_per_op_contract(policy, dtype, variant, shape, monkeypatch):
    s = pu.run_case(variant, dtype, shape, policy, monkeypatch)
    impls, by_cout = set(s["impls"]), s["impl_by_cout"]
    if policy == "igemm":
        assert impls == {0}, impls
    elif policy == "small_fused":
        assert {1, 2} <= impls and s["fused_pool"] > 0 and s["fused_up"] > 0, (impls, s["fused_pool"], s["fused_up"])
        if variant == "f":
            assert (32, 1) in by_cout or (32, 2) in by_cout, "no 32-output-channel layer ran conv_small (FN = 2)"
    elif policy == "small_unfused":
        assert impls == {0, 1} and s["fused_pool"] == s["fused_up"] == 0, (impls, s["fused_pool"], s["fused_up"])
    elif policy == "halo":
        assert 3 in impls, impls
        if variant == "f":
            assert (32, 3) in by_cout, "no 32-output-channel layer ran conv_halo_f32 (FN = 2)"
    else:
        assert impls <= {0, 1, 2, 3}


def test_crop_normalisation_is_per_crop_and_exact(monkeypatch):
    """forward_crops with two crops of one shape: each crop's mask is 255 (normPRED > 0.5) over THAT crop's min / max of the engine's own
    prob (integer atomics on the bits: exact). The kernel evaluates (p - mi) / (ma - mi) > 0.5 in fp32 like the line below; a pixel may
    differ only where that value is within one fp32 ulp of 0.5 (the bound the whole-call norm is held to)."""
    from yolo_puncture_amd.u2net import U2NetEngine
    pu.set_policy(monkeypatch, "tuned")
    st, _ = pu.case_state("p")
    frames = rand_image((2, 64, 80, 3), seed=7)
    frames[1] //= 8                         # a dark frame: its crop's range is narrower (the CPU oracle has 29 pixels flip under a shared range)
    wins, ch, cw = [(3, 5, 43, 41), (30, 20, 70, 56)], 36, 40
    eng = U2NetEngine("p", "fp32", 0, state=st)
    try:
        prob, cmask, _ = eng.forward_crops(frames.cuda(), wins, [0, 1], (ch, cw))
        torch.cuda.synchronize()
    finally:
        eng.close()
    prob, cmask = prob.cpu(), cmask.cpu()
    ranges = [(float(prob[b].min()), float(prob[b].max())) for b in range(2)]
    assert ranges[0][0] != ranges[1][0] and ranges[0][1] != ranges[1][1], ranges      # else per-crop and whole-call could not be told apart
    whole = ((prob - prob.min()) / (prob.max() - prob.min()) > 0.5).to(torch.uint8) * 255
    told_apart = 0
    for b in range(2):
        norm = (prob[b] - prob[b].min()) / (prob[b].max() - prob[b].min())
        want = (norm > 0.5).to(torch.uint8) * 255
        edge = (norm - 0.5).abs() <= 2.0 ** -24
        assert torch.equal(cmask[b][~edge], want[~edge]), (b, int((cmask[b] != want).sum()))
        told_apart += int((whole[b] != want)[~edge].sum())
    print("crop ranges", ranges, "pixels a whole-call range would flip:", told_apart)
    assert told_apart > 0
