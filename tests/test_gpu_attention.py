"""The PSA attention kernels of csrc/attention.hip alone (yp_debug_attention), against the fp64 reference of tests/attention_ref.py, at the
edges no graph puts them: token counts beside every boundary of the two kernels, workgroups that walk runs of query tiles (the launcher's
`wgs` target is set per call), peaked / shifted / one-hot score rows on which a wrong mask, a lost max subtraction or a permuted key is an
O(1) error, strided and offset slices, and the host check's refusals. Bounds: attention_ref.py (none comes from a kernel's output)."""
import ctypes as C

import pytest
import torch

import attention_ref as A
from helpers import assert_within_noise_floor

pytestmark = pytest.mark.gpu

MFMA, GENERIC = 1, 0


def _launch(qkv, nh, kd, hd, **kw):
    from yolo_puncture_amd.engine import attention
    out, kernel = attention(qkv.cuda(), nh, kd, hd, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kernel


def _check_bf16(case, kernel_want, wgs=0):
    B, N, nh, kd, hd, dist = case
    qkv, pi, want, P, v = A.bf16_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd, wgs=wgs)
    assert kernel == kernel_want, f"kernel {kernel}"
    A.assert_bf16_contract(f"{A.case_id(case)} wgs {wgs}", got, want, P, v, dist)
    if dist == "lookup":
        exp = A.lookup_expected(qkv, pi, nh, kd, hd)
        sel = want == exp
        assert float(sel.double().mean()) > 0.999 and bool((got.double()[sel] == exp[sel]).all()), "a query selects exactly its key's value row"
    return got


@pytest.mark.parametrize("case", A.MFMA_CASES, ids=A.case_id)
def test_mfma_bf16_token_counts(case):
    assert A.tiles_per_workgroup(case[0], case[1], case[2])[1] == 1
    _check_bf16(case, MFMA)


@pytest.mark.parametrize("case", A.RUN_CASES, ids=A.case_id)
def test_mfma_bf16_runs_of_tiles(case):
    B, N, nh, wgs = case[0], case[1], case[2], case[6]
    nsplit, tpw = A.tiles_per_workgroup(B, N, nh, wgs)
    assert tpw >= 9, "a wave of the workgroup gets a second tile"
    _check_bf16(case[:6], MFMA, wgs=wgs)


def test_mfma_bf16_bench_split():
    """B = 32 of v10-S at 640x640: the launcher's own split, 2 workgroups of 13 and 12 tiles per head"""
    B, N, nh = A.BENCH_SPLIT_CASE[:3]
    assert A.tiles_per_workgroup(B, N, nh) == (2, 13)
    _check_bf16(A.BENCH_SPLIT_CASE, MFMA)


@pytest.mark.parametrize("case", A.GENERIC_BF16_CASES, ids=A.case_id)
def test_generic_bf16(case):
    _check_bf16(case, GENERIC)


@pytest.mark.parametrize("case", A.F32_CASES, ids=A.case_id)
def test_generic_fp32(case):
    B, N, nh, kd, hd, dist = case
    qkv, o32, o64 = A.f32_case(*case)
    got, kernel = _launch(qkv, nh, kd, hd)
    assert kernel == GENERIC and bool(torch.isfinite(got).all())
    assert_within_noise_floor(f"attention fp32 {A.case_id(case)}", got, o32, o64, A.F32_TARGET)


@pytest.mark.parametrize("case", A.SLICE_CASES, ids=A.case_id)
def test_slices_leave_their_surroundings_alone(case):
    """qkv is a slice at channel 8 of a wider tensor whose other channels are NaN; the output is a slice at channel 8 of a wider tensor
    pre-filled with a sentinel bit pattern: the result is in contract and no bit outside the slice changes."""
    name, B, N, nh, kd, hd, dist, kernel_want = case
    dt, bits, sentinel = (torch.bfloat16, torch.int16, 0x5A5B) if name == "bf16" else (torch.float32, torch.int32, 0x5A5B5C5D)
    blk = 2 * kd + hd
    q_stride, q_coff, o_stride, o_coff = nh * blk + 24, 8, nh * hd + 16, 8
    if name == "bf16":
        qkv, _, want, P, v = A.bf16_case(B, N, nh, kd, hd, dist)
    else:
        qkv, o32, o64 = A.f32_case(B, N, nh, kd, hd, dist)
    wide = A.embed(qkv, q_stride, q_coff, float("nan"))
    out = torch.full((B, N, o_stride), sentinel, dtype=bits).view(dt).cuda()
    got_wide, kernel = _launch(wide, nh, kd, hd, q_coff=q_coff, out=out, o_coff=o_coff)
    assert kernel == kernel_want
    got = got_wide[..., o_coff:o_coff + nh * hd]
    assert bool(torch.isfinite(got).all())
    outside = torch.ones(o_stride, dtype=torch.bool)
    outside[o_coff:o_coff + nh * hd] = False
    assert bool((got_wide.view(bits)[..., outside] == sentinel).all()), "a store left the output slice"
    if name == "bf16":
        A.assert_bf16_contract(f"slice {A.case_id(case)}", got, want, P, v, dist)
    else:
        assert_within_noise_floor(f"attention fp32 slice {A.case_id(case)}", got, o32, o64, A.F32_TARGET)
    # the slice changes addresses only: the compact launch gives the same bits
    compact, _ = _launch(qkv, nh, kd, hd)
    assert torch.equal(compact.view(bits), got.contiguous().view(bits))


@pytest.mark.parametrize("case", A.SLICE_CASES, ids=A.case_id)
def test_images_are_independent_and_launches_repeat(case):
    name, B, N, nh, kd, hd, dist, kernel_want = case
    bits = torch.int16 if name == "bf16" else torch.int32
    qkv = A.bf16_case(B, N, nh, kd, hd, dist)[0] if name == "bf16" else A.f32_case(B, N, nh, kd, hd, dist)[0]
    whole, kernel = _launch(qkv, nh, kd, hd)
    again, _ = _launch(qkv, nh, kd, hd)
    assert kernel == kernel_want and torch.equal(whole.view(bits), again.view(bits)), "two launches are bit-equal"
    for b in range(B):
        one, k1 = _launch(qkv[b:b + 1].contiguous(), nh, kd, hd)
        assert k1 == kernel_want and torch.equal(one.view(bits), whole[b:b + 1].view(bits)), f"image {b} alone differs from image {b} of the batch"


def test_mfma_bf16_split_does_not_change_the_bits():
    """the run a tile belongs to decides which wave computes it and how its query fragment is fetched, never its value"""
    B, N, nh, kd, hd, dist = 2, 400, 2, 32, 64, "peaked"
    qkv = A.bf16_case(B, N, nh, kd, hd, dist)[0]
    base, _ = _launch(qkv, nh, kd, hd)                       # one tile per workgroup
    for wgs in (4, 8, 12):
        got, kernel = _launch(qkv, nh, kd, hd, wgs=wgs)
        assert kernel == MFMA and torch.equal(got.view(torch.int16), base.view(torch.int16)), wgs


# ---- refusals: only arguments the host check rejects; nothing here may launch -------------------------------------------------------------
def _raw(lib, qkv, out, dtype, B, N, nh, kd, hd, q_stride, q_coff, o_stride, o_coff, wgs=0, kernel=True):
    k = C.c_int(-7)
    rc = lib.yp_debug_attention(C.c_void_p(qkv), C.c_void_p(out), dtype, B, N, nh, kd, hd, q_stride, q_coff, o_stride, o_coff, wgs,
                                C.byref(k) if kernel else None, None)
    return rc, lib.yp_last_error().decode(), k.value


def test_refusals_happen_on_the_host():
    from yolo_puncture_amd.engine import load_library, YP_BF16, YP_F32
    lib = load_library()
    B, N, nh, kd, hd = 1, 2369, 2, 32, 64
    qkv = torch.zeros((B, N, nh * 128 + 8), dtype=torch.bfloat16, device="cuda")
    out = torch.full((B, N, nh * 64 + 8), 0x5A5B, dtype=torch.int16, device="cuda")
    q, o = qkv.data_ptr(), out.data_ptr()
    ok = dict(dtype=YP_BF16, B=1, N=400, nh=nh, kd=kd, hd=hd, q_stride=nh * 128 + 8, q_coff=0, o_stride=nh * 64 + 8, o_coff=0)
    cases = [
        ("null", dict(qkv=0), "null"), ("null", dict(out=0), "null"), ("null", dict(kernel=False), "null"),
        ("dtype", dict(dtype=2), "dtype"),
        ("B = 0", dict(B=0), "non-positive"), ("N = 0", dict(N=0), "non-positive"), ("nh = -1", dict(nh=-1), "non-positive"),
        ("kd = 0", dict(kd=0), "non-positive"), ("hd = 0", dict(hd=0), "non-positive"), ("q_stride = 0", dict(q_stride=0), "non-positive"),
        ("o_coff < 0", dict(o_coff=-4), "non-positive"), ("wgs < 0", dict(wgs=-1), "non-positive"),
        ("qkv slice past its stride", dict(q_coff=12), "does not fit q_stride"),
        ("output slice past its stride", dict(o_coff=12), "does not fit o_stride"),
        ("q_stride % 4", dict(q_stride=nh * 128 + 6), "multiples of 4"), ("q_coff % 4", dict(q_coff=2), "multiples of 4"),
        ("o_stride % 4", dict(o_stride=nh * 64 + 6), "multiples of 4"), ("o_coff % 4", dict(o_coff=2), "multiples of 4"),
        ("kd % 4", dict(kd=30, hd=60), "multiples of 4"),
        ("N past the LDS", dict(N=2369), "2368"), ("N past the LDS, fp32", dict(N=2369, dtype=YP_F32), "2368"),
        ("N past the LDS, kd 36", dict(N=2365, kd=36, hd=56), "2364"),
    ]
    for what, change, msg in cases:
        a = dict(ok, qkv=q, out=o, kernel=True, wgs=0)
        a.update(change)
        rc, err, k = _raw(lib, **a)
        assert rc < 0 and msg in err, (what, rc, err)
        assert k == -7, (what, "kernel_out was written")
    torch.cuda.synchronize()
    assert bool((out == 0x5A5B).all()), "a refused call wrote to the output"
