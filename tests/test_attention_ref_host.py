"""CPU checks of tests/attention_ref.py, for every case id tests/test_gpu_attention.py uses: the fp64 reference restates the oracle's
expression, the input makers give the score distributions they promise, and the reference pair alone (the oracle's float32 restatement
against the fp64 reference) stays inside the bounds the kernels are held to - so a failure on the GPU is the kernel's."""
import pytest
import torch

import attention_ref as A

_BF16 = sorted(set(A.BF16_CASES), key=A.BF16_CASES.index)


@pytest.mark.parametrize("mode,dt", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
@pytest.mark.parametrize("shape", [(2, 37, 2, 32, 64), (1, 50, 4, 36, 72)], ids=A.case_id)
def test_reference_equals_oracle_expression(shape, mode, dt):
    B, N, nh, kd, hd = shape
    qkv = torch.randn(B, N, nh * (2 * kd + hd), generator=torch.Generator().manual_seed(N), dtype=torch.float64).to(dt)
    want = A.oracle_expression(qkv, nh, kd, hd, torch.float64, mode)
    # through a strided, offset slice as well: the channels outside it are NaN and must not be read
    for q_coff, stride in ((0, qkv.shape[2]), (8, qkv.shape[2] + 24)):
        got, _, _ = A.reference(A.embed(qkv, stride, q_coff, float("nan")), nh, kd, hd, q_coff, mode)
        if mode == "fp32":
            assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
        else:       # two fp64 programs can round a probability on a tie differently: identical but for (at most) isolated elements
            assert float((got != want).double().mean()) < 1e-3 and float(A.ulps_bf16(got, want).max()) <= 1.0


@pytest.mark.parametrize("case", _BF16, ids=A.case_id)
def test_bf16_case_inputs_and_reference_pair(case):
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    assert qkv.dtype == torch.bfloat16 and bool(torch.isfinite(want).all())
    x = qkv.double().reshape(B, N, nh, -1)
    heads = x.permute(0, 2, 1, 3).reshape(B * nh, -1)
    assert B * nh == 1 or torch.unique(heads, dim=0).shape[0] == B * nh, "every image and head has its own data"
    s = torch.einsum("bnhc,bmhc->bhnm", x[..., :kd], x[..., kd:2 * kd]) * kd ** -0.5
    neff = 1.0 / (P ** 2).sum(-1)
    print(f"[attention inputs] {A.case_id(case)}: score mean {float(s.mean()):.2f} std {float(s.std()) if N > 1 else 0.0:.2f}, "
          f"effective keys max {float(neff.max()):.1f} of {N}")
    if dist == "flat" and N >= 64:
        assert 0.8 < float(s.std()) < 1.25
    if dist in ("peaked", "shifted") and N >= 64:
        assert 0.75 * A.PEAK_STD < float(s.std(-1).mean()) < 1.25 * A.PEAK_STD
        assert float(neff.max()) < N / 8
    if dist == "shifted" and N >= 2:
        assert float(s.min()) > 0 and abs(float(s.mean()) - A.SHIFT) < 3.0
        if N >= 255:      # 60 + 8 sigma passes log(FLT_MAX) = 88.7 once a head has tens of thousands of scores
            assert not bool(torch.isfinite(torch.exp(s.float())).all()), "without the max subtraction exp overflows in float32"
    if dist == "lookup":
        hit = torch.gather(torch.softmax(s, -1), 3, pi[..., None])
        assert float(hit.min()) >= 1.0 - 2.0 ** -9
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        assert float((want == exp).double().mean()) > 0.999, "the reference's output is v[pi(n)] (almost) everywhere"
    # the reference pair alone inside the bound of the GPU test
    o32 = A.oracle_expression(qkv, nh, kd, hd, torch.float32, "bf16")
    A.assert_bf16_contract(f"float32 restatement {A.case_id(case)}", o32, want, P, v, dist)
    if dist == "lookup":
        assert bool((o32.double()[want == exp] == exp[want == exp]).all())


_FLOORS = {}


@pytest.mark.parametrize("case", A.F32_ALL_CASES, ids=A.case_id)
def test_fp32_case_noise_floor(case):
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    assert qkv.dtype == torch.float32 and o32.dtype == torch.float32 and bool(torch.isfinite(o64).all())
    f = float((o32.double() - o64).abs().max())
    _FLOORS[case] = f
    print(f"[attention fp32 floor] {A.case_id(case)}: |o32 - o64| max {f:.3e}")
    # (the float32 expression's summation order, and with it f, moves by tens of percent with the host's BLAS blocking and thread count)
    assert f <= 2.0 * A.F32_MEASURED_FLOOR, "the recorded floor (attention_ref.F32_MEASURED_FLOOR) is the largest over the fp32 cases"
    if dist in ("peaked", "shifted") and N >= 64:
        _, P, _ = A.reference(qkv, nh, kd, hd)
        assert float((1.0 / (P ** 2).sum(-1)).max()) < N / 8
    if case == A.F32_ALL_CASES[-1]:
        assert max(_FLOORS.values()) >= 0.5 * A.F32_MEASURED_FLOOR, "the recorded floor is stale: measure again"


def test_split_formula_gives_the_runs_the_cases_name():
    assert [A.tiles_per_workgroup(2, n, 2, w) for n, w in ((400, 4), (400, 8), (400, 12), (285, 8), (129, 4))] == [(1, 25), (2, 13), (3, 9), (2, 9), (1, 9)]
    assert A.tiles_per_workgroup(*A.BENCH_SPLIT_CASE[:3]) == (2, 13)
    assert all(A.tiles_per_workgroup(3, n, 2)[1] == 1 for n in A.MFMA_N)         # B * nh = 6: one tile per workgroup, the case the graphs give
