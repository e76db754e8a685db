"""Stand-alone reference, inputs and bounds for the PSA attention core (csrc/attention.hip), shared by test_attention_ref_host.py (CPU) and
test_gpu_attention.py (the kernels, through yp_debug_attention).

The op, per image and head, on the NHWC qkv tensor [B, N, q_stride] whose head h holds q(kd) | k(kd) | v(hd) at channels
q_coff + h * (2 kd + hd):      P = softmax_m(q_n . k_m * kd^-0.5),      o[n] = sum_m P[n, m] v[m].
`reference` states it in fp64. Its bf16 mode follows oracle/yolov10_oracle.py::attention: the inputs are bf16 values, P is rounded to bf16
and so is the output. `oracle_expression` is the oracle's own torch expression in a chosen dtype: in fp64 it must equal `reference`, in
float32 it is the noise-floor sample (what the reference program's arithmetic gives on the same input).

Bounds, none of them taken from a kernel:
  bf16  every element within 1 bf16 ulp of the reference (perop_bf16.ulps_bf16) and fewer than 2 % of the elements differing at all. For the
        distributions in WIDENED the float32 restatement of the oracle itself exceeds 1 ulp (measured below): a flip of one bf16 probability
        moves o[n, d] by ulp(P[n, m]) |v[m, d]|, many ulps of an output that cancels to ~0. There the per-element bound is
        1 output ulp + 2 max_m ulp_bf16(P[n, m]) |v[m, d]| (two simultaneous flips at the row's largest contributor), and fewer than 0.5 %
        of the elements may lie above 1 ulp (the fused-op cap of perop_bf16.py).
  fp32  helpers.assert_within_noise_floor(got, o32, o64, F32_TARGET): at most twice the float32 restatement's own error on the same case.
"""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from perop_bf16 import ulps_bf16  # noqa: E402

DISTS = ("flat", "peaked", "shifted", "lookup")
PEAK_STD = 8.0          # standard deviation of the scaled scores of `peaked` and `shifted`
SHIFT = 60.0            # common lift of every scaled score of `shifted`
LOOKUP_MISS = 2.0 ** -16    # `lookup`: c is the smallest power of two with 1 - P[n, pi(n)] <= this in the reference (the contract asks 2^-9)

# Measured by test_attention_ref_host.py over every bf16 case id of the GPU file: the worst ulps_bf16 of the oracle's float32 restatement
# against the fp64 reference is 48 for flat (N = 48), 76 for peaked (N = 2368), 164 for shifted (N = 255) and 0 for lookup. None of the
# three random distributions stays inside the plain contract on the reference alone: the float32 and the fp64 softmax round a few
# probabilities per ten thousand to different bf16 values, and on an output that cancels to ~0 one such flip is many output ulps (flat rows
# as well: P ~ 1/N is flipped by 2^-8 / N, an output near the 2^-10 max floor of ulps_bf16 has an ulp of 2^-18). So all three take the
# widened per-element bound; the restatement then reaches at most 0.87 of what is allowed. lookup keeps the plain contract.
WIDENED = ("flat", "peaked", "shifted")
MAX_DIFFER = 0.02       # share of elements that may differ at all
MAX_ABOVE_1ULP = 0.005  # share of elements above 1 ulp where the widened bound applies

# fp32: 16 x the largest |o32 - o64| that test_attention_ref_host.py measures over the fp32 cases (measured 3.19e-05, `shifted` at N = 2368;
# flat stays below 7e-07, peaked below 1.3e-05).
F32_MEASURED_FLOOR = 3.2e-05
F32_TARGET = 16 * F32_MEASURED_FLOOR


def _rng(dist, B, N, nh, kd, hd, seed):
    key = 0
    for x in (DISTS.index(dist), B, N, nh, kd, hd, seed):
        key = (key * 1000003 + x) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(key)


@functools.lru_cache(maxsize=4)
def make_qkv(dist, B, N, nh, kd, hd, dtype=torch.bfloat16, seed=0):
    """-> (qkv [B, N, nh * (2 kd + hd)] of `dtype`, pi): seeded, different per image and head. pi: int64 [B, nh, N], the key each query of
    `lookup` selects (None otherwise). The values are exact in `dtype`: the reference and the kernels read the same numbers."""
    assert dist in DISTS
    g = _rng(dist, B, N, nh, kd, hd, seed)
    q = torch.randn(B, N, nh, kd, generator=g, dtype=torch.float64)
    k = torch.randn(B, N, nh, kd, generator=g, dtype=torch.float64)
    v = torch.randn(B, N, nh, hd, generator=g, dtype=torch.float64)
    pi = None
    if dist in ("peaked", "shifted"):
        # q . k / sqrt(kd) of two N(0, s^2) vectors has standard deviation s^2
        q, k = q * PEAK_STD ** 0.5, k * PEAK_STD ** 0.5
    if dist == "shifted":
        # a common component c u on both sides (u a unit vector, q and k made orthogonal to it first) lifts every score by c^2 / sqrt(kd)
        u = torch.full((kd,), kd ** -0.5, dtype=torch.float64)
        c = (SHIFT * kd ** 0.5) ** 0.5
        q = q - (q @ u)[..., None] * u + c * u
        k = k - (k @ u)[..., None] * u + c * u
    if dist == "lookup":
        for _ in range(64):          # distinct sign vectors per (image, head): redraw in the (unlikely) case of a repeated row
            k = torch.where(torch.rand(B, N, nh, kd, generator=g) < 0.5, -1.0, 1.0).double()
            if all(torch.unique(k[b, :, h], dim=0).shape[0] == N for b in range(B) for h in range(nh)):
                break
        else:
            raise AssertionError("no set of distinct sign vectors")
        pi = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(nh)]) for _ in range(B)])     # [B, nh, N]
        ksel = torch.gather(k.permute(0, 2, 1, 3), 2, pi[..., None].expand(B, nh, N, kd)).permute(0, 2, 1, 3)      # k[b, pi[b, h, n], h]
        c = 1.0
        while True:                  # powers of two: c k is exact in bf16
            s = torch.einsum("bnhc,bmhc->bhnm", c * ksel, k) * kd ** -0.5
            hit = torch.gather(s.softmax(-1), 3, pi[..., None])
            if float((1.0 - hit).max()) <= LOOKUP_MISS:
                break
            c *= 2.0
            assert c <= 2.0 ** 12
        q = c * ksel
    qkv = torch.cat([q, k, v], dim=3).reshape(B, N, nh * (2 * kd + hd)).to(dtype)
    return qkv, pi


def embed(x, stride, coff, fill):
    """x [B, N, C] placed at channels [coff, coff + C) of a new [B, N, stride]; every other channel holds `fill`."""
    B, N, C = x.shape
    out = torch.full((B, N, stride), fill, dtype=x.dtype)
    out[..., coff:coff + C] = x
    return out


def _round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def reference(qkv, nh, kd, hd, q_coff=0, mode="fp32"):
    """fp64 statement of the op on qkv [B, N, q_stride] (any float dtype; channels outside the slice are never read).
    -> (o [B, N, nh * hd] float64, P [B, nh, N, N] float64, v [B, N, nh, hd] float64). mode "bf16": P and o rounded to bf16 values."""
    assert mode in ("fp32", "bf16")
    B, N, _ = qkv.shape
    blk = 2 * kd + hd
    x = qkv[..., q_coff:q_coff + nh * blk].double().reshape(B, N, nh, blk)
    q, k, v = x[..., :kd], x[..., kd:2 * kd], x[..., 2 * kd:]
    s = torch.einsum("bnhc,bmhc->bhnm", q, k) * kd ** -0.5
    P = torch.softmax(s, dim=-1)
    if mode == "bf16":
        P = _round_bf16(P)
    o = torch.einsum("bhnm,bmhd->bnhd", P, v).reshape(B, N, nh * hd)
    if mode == "bf16":
        o = _round_bf16(o)
    return o, P, v


def oracle_expression(qkv, nh, kd, hd, dt, mode="fp32"):
    """The lines of oracle/yolov10_oracle.py::attention between the qkv conv and the `.o` tap, on a compact NHWC qkv [B, N, nh * (2 kd + hd)],
    computed in dtype `dt` (mode "bf16": the oracle's bf16emu roundings of P and o). -> o [B, N, nh * hd] of dtype dt."""
    B, N, _ = qkv.shape
    rq = _round_bf16 if mode == "bf16" else (lambda t: t)
    x = qkv.to(dt).permute(0, 2, 1).contiguous()                           # the oracle's NCHW map, H * W = N
    q, k, v = x.view(B, nh, 2 * kd + hd, N).split([kd, kd, hd], dim=2)
    attn = (q.transpose(-2, -1) @ k) * (kd ** -0.5)
    attn = rq(attn.softmax(dim=-1))
    o = rq((v @ attn.transpose(-2, -1)).reshape(B, nh * hd, N))
    return o.permute(0, 2, 1).contiguous()


def bf16_ulp(x):
    """the bf16 spacing at |x| (0 at 0)"""
    a = x.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -1000))) - 7), torch.zeros_like(a))


def flip_term(P, v):
    """max_m ulp_bf16(P[n, m]) |v[m, d]| per output element -> [B, N, nh * hd]: what one flipped bf16 probability can move o[n, d] by."""
    B, nh, N, _ = P.shape
    hd = v.shape[3]
    out = torch.empty(B, N, nh, hd, dtype=torch.float64)
    for b in range(B):
        for h in range(nh):
            up, av = bf16_ulp(P[b, h]).float(), v[b, :, h].abs().float()      # [N, N], [N, hd]
            for d0 in range(0, hd, 16):
                out[b, :, h, d0:d0 + 16] = (up[:, :, None] * av[None, :, d0:d0 + 16]).amax(1).double()
    return out.reshape(B, N, nh * hd)


def bf16_report(got, want, P, v, dist):
    """-> dict(worst ulp, share differing, share above 1 ulp, worst ulp / allowed ulp) of `got` against the bf16 reference `want`."""
    got, want = got.double(), want.double()
    u = ulps_bf16(got, want)
    allowed = torch.ones_like(u)
    if dist in WIDENED:
        mag = want.abs().clamp_min(float(want.abs().max()) * 2.0 ** -10 + 2.0 ** -126)       # the magnitude floor of ulps_bf16
        allowed = 1.0 + 2.0 * flip_term(P, v) / torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return {"worst": float(u.max()), "differ": float((u > 0).double().mean()), "above1": float((u > 1.0 + 1e-6).double().mean()),
            "ratio": float((u / allowed).max()), "finite": bool(torch.isfinite(got).all())}


def assert_bf16_contract(what, got, want, P, v, dist):
    r = bf16_report(got, want, P, v, dist)
    print(f"[attention bf16] {what}: worst {r['worst']:.2f} ulp, {100 * r['differ']:.3f} % differ, {100 * r['above1']:.3f} % above 1 ulp, "
          f"worst / allowed {r['ratio']:.3f}")
    assert r["finite"], what
    assert r["ratio"] <= 1.0 + 1e-6, (what, r)
    assert r["differ"] < MAX_DIFFER, (what, r)
    if dist in WIDENED:
        assert r["above1"] < MAX_ABOVE_1ULP, (what, r)
    else:
        assert r["worst"] <= 1.0 + 1e-6, (what, r)
    return r


# ---- the cases of tests/test_gpu_attention.py (test_attention_ref_host.py walks the same lists) ----------------------------------------
# (B, N, nh, kd, hd, dist[, wgs])
MFMA_N = (1, 15, 16, 17, 31, 33, 48, 255, 384, 385, 399, 400)
MFMA_ALL_DISTS_N = (17, 255, 399, 400)
MFMA_CASES = [(3, n, 2, 32, 64, d) for n in MFMA_N for d in (DISTS if n in MFMA_ALL_DISTS_N else ("flat", "peaked"))]
RUN_CASES = [(2, n, 2, 32, 64, d, wgs) for n, wgs in ((400, 4), (400, 8), (400, 12), (285, 8), (129, 4)) for d in DISTS]
BENCH_SPLIT_CASE = (32, 400, 4, 32, 64, "peaked")
GENERIC_BF16_CASES = ([(2, n, 2, 32, 64, d) for n in (401, 512, 513) for d in ("flat", "peaked")] +
                      [(1, 2368, 2, 32, 64, d) for d in ("flat", "peaked")] +
                      [(2, n, 4, 36, 72, d) for n in (15, 20, 257, 400, 401) for d in ("flat", "peaked")])
F32_CASES = [(2, n, 2, 32, 64, d) for n in (1, 15, 16, 17, 255, 256, 257, 400, 2368) for d in ("flat", "peaked", "shifted")]
# slices: (dtype name, B, N, nh, kd, hd, dist, expected kernel)
SLICE_CASES = [("bf16", 3, 399, 2, 32, 64, "peaked", 1), ("bf16", 3, 401, 2, 32, 64, "peaked", 0), ("fp32", 3, 257, 2, 32, 64, "peaked", 0)]
F32_ALL_CASES = F32_CASES + [c[1:7] for c in SLICE_CASES if c[0] == "fp32"]
BF16_CASES = MFMA_CASES + [c[:6] for c in RUN_CASES] + [BENCH_SPLIT_CASE] + GENERIC_BF16_CASES + [c[1:7] for c in SLICE_CASES if c[0] == "bf16"]


def case_id(c):
    return "-".join(str(x) for x in c)


def tiles_per_workgroup(B, N, nh, wgs=0):
    """the launcher's split of the matrix-core form (launch_attention): (workgroups per head, query tiles each walks)"""
    target = wgs if wgs > 0 else 256
    ntiles, BH = (N + 15) // 16, B * nh
    nsplit = min(ntiles, max(1, (target + BH - 1) // BH))
    tpw = (ntiles + nsplit - 1) // nsplit
    return (ntiles + tpw - 1) // tpw, tpw


@functools.lru_cache(maxsize=2)
def bf16_case(B, N, nh, kd, hd, dist):
    """-> (qkv bf16, pi, want o, P, v): computed once, shared by the tests of a case; callers leave them unchanged"""
    qkv, pi = make_qkv(dist, B, N, nh, kd, hd, torch.bfloat16)
    o, P, v = reference(qkv, nh, kd, hd, 0, "bf16")
    return qkv, pi, o, P, v


@functools.lru_cache(maxsize=2)
def f32_case(B, N, nh, kd, hd, dist):
    """-> (qkv float32, o32 the oracle's float32 restatement, o64 the fp64 reference)"""
    qkv, _ = make_qkv(dist, B, N, nh, kd, hd, torch.float32)
    o64, _, _ = reference(qkv, nh, kd, hd, 0, "fp32")
    return qkv, oracle_expression(qkv, nh, kd, hd, torch.float32), o64


def lookup_expected(qkv, pi, nh, kd, hd):
    """v[pi(n)] per query -> [B, N, nh * hd] float64"""
    B, N, _ = qkv.shape
    v = qkv.double().reshape(B, N, nh, 2 * kd + hd)[..., 2 * kd:]                                                  # [B, N, nh, hd]
    return torch.gather(v.permute(0, 2, 1, 3), 2, pi[..., None].expand(B, nh, N, hd)).permute(0, 2, 1, 3).reshape(B, N, nh * hd)
