"""Register-weights instances of the stride-2 halo conv (conv_halo_s2.hip) against its LDS-weights kernels.

A launch of id 500 (<2,2,4,2>) or 501 (<1,2,4,2>) with Cin = 32 / 64 takes a register-weights instance: the same tile, or under 501 on a
layer of more than 96 channels <2,2,2,4> (both 64-channel blocks in one workgroup). The conv runs alone (engine.conv_s2 ->
yp_debug_conv_s2) on seeded tensors, once as the launcher picks and once with the weights kept in LDS (lds_weights). A register-weights
instance accumulates every output element in the order of the LDS kernels (chunk, kx, ky), so its output must be EQUAL, bit for bit, to the
LDS launch of the same id - and to 501's where 500 has none (Cin = 64: the 8-row tile needs 182 KB with its weights in LDS).
So that a mistake both share does not pass, every output is also held to the per-op bf16 contract (perop_bf16.py) against a float64
convolution of the same bf16 inputs: at most 1 bf16 ulp on fewer than 2 % of the elements; fp32 outputs as the fp32 ops there (2e-5).

Shapes (input B, H, W), the smallest that reach each way the kernel can go wrong:
  (2, 40, 56)    Ho = 20: a multiple of 4, not of 8; Wo = 28: not a multiple of 16 - partial tile rows and columns, halo rows and columns
                 outside the image on every side. All channel cases run here: Cin 32 / 64 (one / two chunks), Cout 64 / 128 (one / two
                 channel blocks; 128: the one-block instance under 501), Cout 96 (last block partly masked), 160 (the second 128-channel
                 block partly masked), residual, fp32 output.
  (3, 128, 128)  64 -> 128: 192 tiles of 4 rows; the LDS launch has 128 workgroups per channel block - some walk two tiles, some one: the
                 ring across a tile boundary and the wait selection behind an epilogue (epmask). The register instances (192 / 96 tiles
                 on up to 256 workgroups) walk one tile each here; several per workgroup: (6, 128, 128).
  (6, 128, 128)  64 -> 128: 384 tiles of 4 rows on 256 workgroups (one or two each), 192 of 8 rows on 128 per channel block.
  (1, 16, 32)    one 8-row tile (two of 4 rows): most workgroups of a full launch would have none; the grid shrinks to the tiles."""
import pytest
import torch

from helpers import rel_err
from perop_bf16 import ulps_bf16

pytestmark = pytest.mark.gpu

#        (B, H, W), Cin, Cout, residual, fp32 out
CASES = [((2, 40, 56), 32, 64, False, False),
         ((2, 40, 56), 64, 64, False, False),
         ((2, 40, 56), 32, 128, False, False),
         ((2, 40, 56), 64, 128, False, False),
         ((2, 40, 56), 64, 96, False, False),
         ((2, 40, 56), 32, 96, False, False),
         ((2, 40, 56), 64, 160, False, False),
         ((2, 40, 56), 64, 128, True, False),
         ((2, 40, 56), 64, 128, False, True),
         ((2, 40, 56), 32, 64, True, False),
         ((2, 40, 56), 32, 64, False, True),
         ((3, 128, 128), 64, 128, False, False),
         ((6, 128, 128), 64, 128, False, False),
         ((1, 16, 32), 64, 128, False, False),
         ((1, 16, 32), 32, 64, False, False)]


def _inputs(shape, cin, cout, has_res):
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * cin + cout + H)
    x = torch.randn((B, H, W, cin), generator=g).to(torch.bfloat16)
    w = (torch.randn((cout, 3, 3, cin), generator=g) / (9 * cin) ** 0.5).to(torch.bfloat16)
    bias = 0.1 * torch.randn((cout,), generator=g)
    res = torch.randn((B, H // 2, W // 2, cout), generator=g).to(torch.bfloat16) if has_res else None
    return x, w, bias, res


def _reference(x, w, bias, res):
    """float64 on the CPU, from the bf16 values: SiLU(conv + bias) [+ res], NHWC"""
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), bias.double(), stride=2, padding=1)
    y = y * torch.sigmoid(y)
    y = y.permute(0, 2, 3, 1)
    return y + res.double() if res is not None else y


@pytest.mark.parametrize("shape,cin,cout,has_res,f32", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{ci}to{co}{'-res' if r else ''}{'-f32' if f else ''}"
                                                                   for s, ci, co, r, f in CASES])
def test_register_weights_equal_lds_weights(shape, cin, cout, has_res, f32):
    from yolo_puncture_amd.engine import conv_s2, conv_s2_admits
    B, H, W = shape
    x, w, bias, res = _inputs(shape, cin, cout, has_res)
    want = _reference(x, w, bias, res)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    rd = res.cuda() if has_res else None
    # (id, weights in LDS) -> (admitted, LDS bytes, kernel); the predicate itself is pinned by test_halo_s2_wreg_host.py
    launches = {(c, l): conv_s2_admits(c, B, H, W, cin, cout, has_res, f32, lds_weights=l) for c in (500, 501) for l in (False, True)}
    nch = cin // 32
    assert launches[(501, False)][0] and launches[(501, True)][0] and launches[(500, False)][0], launches
    assert launches[(500, True)][0] == (cin == 32), launches                 # (the 8-row LDS kernel holds one chunk of weights only)
    assert launches[(500, False)][2].startswith("conv_halo_s2_kernel<2,2,4,2,3,") and launches[(500, False)][2].endswith(f",false,{nch}>")
    assert launches[(501, False)][2].startswith("conv_halo_s2_kernel<2,2,2,4,3," if cout > 96 else "conv_halo_s2_kernel<1,2,4,2,3,")
    assert launches[(501, False)][2].endswith(f",false,{nch}>") and launches[(501, True)][2].endswith(",false>")
    got = {}
    for key, (ok, _, kernel) in launches.items():
        if not ok:
            continue
        runs = [conv_s2(xd, wd, bd, key[0], res=rd, out_f32=f32, lds_weights=key[1]).cpu() for _ in range(2)]
        assert torch.equal(runs[0], runs[1]), (key, "two runs of one launch differ")
        got[key] = runs[0]
        # the per-op contract against the float64 convolution
        if f32:
            err = rel_err(got[key].double(), want)
            print(f"  {key} {kernel}: fp32 output, relative error {err:.3e}")
            assert err < 2e-5, (key, err)
        else:
            u = ulps_bf16(got[key].double(), want.to(torch.bfloat16).double())
            frac = float((u > 0).double().mean())
            print(f"  {key} {kernel}: max ulp {float(u.max()):.3f}, differing fraction {frac:.5f}")
            assert float(u.max()) <= 1.0 + 1e-6, (key, float(u.max()))
            assert frac < 0.02, (key, frac)
    for c in (500, 501):
        ref = (c, True) if (c, True) in got else (501, True)
        n = int((got[(c, False)] != got[ref]).sum())
        print(f"  id {c} with register weights against {ref}: {n} differing elements of {got[ref].numel()}")
        assert torch.equal(got[(c, False)], got[ref]), (c, ref, n)


def test_tiles_per_workgroup_of_the_multi_tile_cases():
    """restated from the launcher: workgroups per channel block = 256 / channel blocks, one workgroup per CU"""
    Ho, Wo = 64, 64
    t4, t8 = (Ho // 4) * (Wo // 16), (Ho // 8) * (Wo // 16)
    assert 3 * t4 == 192 and 128 < 3 * t4 < 2 * 128            # 501 with LDS weights, two channel blocks: one or two tiles
    assert 256 < 6 * t4 < 2 * 256                               # <2,2,2,4>, one channel block
    assert 128 < 6 * t8 < 2 * 128                               # <2,2,4,2> with register weights, two channel blocks


def test_refused_shape_launches_nothing():
    from yolo_puncture_amd.engine import YolopError, conv_s2
    x = torch.zeros((1, 16, 32, 128), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((128, 3, 3, 128), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros((128,), device="cuda")
    for c in (500, 501, 504, 505, 499):
        with pytest.raises(YolopError):
            conv_s2(x, w, b, c)
