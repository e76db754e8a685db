"""Per-op contract of the U^2-Net engine (u2net.hip over conv_igemm / conv_small / conv_halo_f32), fp32 and bf16: DESIGN.md section 2.

One forward runs, then every op of the plan (U2NetEngine.ops()) is held to a reference of THAT OP ALONE, built from the tensors the engine
itself stored (read_tensor): every tensor has its own arena slot and is written once per forward, so afterwards each still holds what its
readers read. The one exception is the output of a pool / up-sample whose consumer took it while loading (impl 2): nothing wrote it, and
the consumer's operand is rebuilt from the pool's / up-sample's own input instead. Weights and bias are u2net.fold_state's.

Bounds (none comes from the kernels):
 (a) fp32, per element: any-order fp32 summation of K = 9 Cin products + bias + residual obeys
         |got - y64| <= (K + 4) 2^-24 (|w| (*) |x| + |b| + |res|)                  (y64, and the right side, in fp64)
 (b) fp32, per op with >= 1024 outputs: rms(got - y64) <= 4 rms(torch_fp32 - y64)  (the project's factor between two fp32 orderings)
 (c) bf16: reference = bf16 rounding of y64 from bf16-rounded weights (fp32 bias, the engine's bf16-exact inputs);
         perop_bf16.ulps_bf16 <= 1 everywhere, differing elements <= max(1, 2 %). The fp32 side maps are held to (a).
 pools: bit-equal. up-samples: fp32 within 8 2^-24 max|x| of F.interpolate; bf16 within 1 ulp of its bf16 rounding, same 2 % cap; and
         bit-equal to bilinear_f32 below, the engine's own operation order, which is the operand of a conv that took its up-sample
         while loading (the strict contract (c) needs that operand exact: see check_forward).
 tail: prob within 1e-6 of fp64 sigmoid(sum fuse_k up(side_k) + bias) on the engine's own side maps; normPRED range = min / max of the
         engine's own prob exactly; norm within 1 fp32 ulp; mask == 255 (norm > 0.5) on the engine's own norm.
`check_forward` takes anything with ops() / tensors() / read_tensor(name) (tests/test_u2net_perop_host.py feeds it a CPU emulation)."""
import functools
import math

import torch
import torch.nn.functional as F

from perop_bf16 import ulps_bf16

EPS32 = 2.0 ** -24
RMS_FACTOR = 4.0           # (b)
RMS_MIN_ELEMS = 1024       # (b) is asserted on tensors at least this large
PROB_TOL = 1e-6
SIDES = tuple(f"side{k}" for k in range(1, 7))

# forced policy -> environment read by yp_u2net_create ("tuned": nothing set, the per-layer timing decides)
POLICIES = {
    "igemm": {"YOLOP_U2_SMALL_MAX": "0"},
    "small_fused": {"YOLOP_U2_SMALL_MAX": "1000000000"},
    "small_unfused": {"YOLOP_U2_SMALL_MAX": "1000000000", "YOLOP_U2_FUSE_POOL": "0"},
    "halo": {"YOLOP_U2_SMALL_MAX": "1"},
    "tuned": {},
}


def set_policy(monkeypatch, policy):
    for k in ("YOLOP_U2_SMALL_MAX", "YOLOP_U2_FUSE_POOL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in POLICIES[policy].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def case_state(variant):
    from yolo_puncture_amd.u2net import fold_state, synthetic_state
    st = synthetic_state(variant, 0)
    return st, fold_state(st, variant)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def ulp32(x):
    """spacing of fp32 at x (x fp32)"""
    return (torch.nextafter(x.abs(), torch.full_like(x, math.inf)) - x.abs())


def _pattern(bad):
    """where the failing elements of an NHWC map sit: the evidence a kernel fix starts from"""
    idx = bad.nonzero()
    B, H, W, C = bad.shape

    def axis(k, n):
        v = sorted(set(idx[:, k].tolist()))
        return f"{v[0]}..{v[-1]} ({len(v)} of {n})" if len(v) > 6 else f"{v} of {n}"
    return (f"{idx.shape[0]} of {bad.numel()} elements; images {axis(0, B)}, rows {axis(1, H)}, cols {axis(2, W)}, channels {axis(3, C)}; "
            f"first {idx[:4].tolist()}")


# ---- the engine's bilinear resize, restated: one IEEE fp32 rounding per operation, in the order of csrc/kernel_util.h ------------------
# (bilinear_tap / bilinear_blend are compiled without FMA contraction, so u2_up_kernel, conv_small's fused load and the tail all evaluate
# exactly this; F.interpolate evaluates the same formula with other roundings and agrees within the stand-alone up-sample's bound.)
def _taps_f32(n_in, n_out):
    d = torch.arange(n_out, dtype=torch.float32)
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    f = (scale * (d + 0.5) - 0.5).clamp_min(0.0)         # area_pixel_compute_source_index, align_corners=False
    i0 = f.floor().long()
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    l1 = f - i0.float()
    return i0, i1, 1.0 - l1, l1


def _blend(x, H, W, dt):
    y0, y1, ly0, ly1 = _taps_f32(x.shape[2], H)
    x0, x1, lx0, lx1 = _taps_f32(x.shape[3], W)
    ly0, ly1, lx0, lx1 = ly0.to(dt)[:, None], ly1.to(dt)[:, None], lx0.to(dt), lx1.to(dt)
    top, bot = x[:, :, y0], x[:, :, y1]
    return ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])


def bilinear_f32(x, H, W):
    """x fp32 [B,C,h,w] -> [B,C,H,W], the bits the engine's kernels produce (same size: the values unchanged, as in u2_up_kernel)"""
    return x.clone() if tuple(x.shape[2:]) == (H, W) else _blend(x, H, W, torch.float32)


def up64(x, H, W):
    """x fp64 [B,C,h,w] -> [B,C,H,W]: the fp32 tap weights, blended in fp64 (the tail's reference)"""
    return x if tuple(x.shape[2:]) == (H, W) else _blend(x, H, W, torch.float64)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def check_forward(eng, variant, dtype, folded, label=""):
    """Walk eng.ops() after one forward. Returns (stats, failures): every violated bound is one line of `failures` naming the op, its impl,
    shape and where the bad elements sit; the caller asserts the list is empty."""
    ops, tinfo = eng.ops(), eng.tensors()
    cache = {}

    def rd(v):
        t, c0, c = v
        if t not in cache:
            cache[t] = eng.read_tensor(tinfo[t]["name"])
        return cache[t][..., c0:c0 + c]

    bf = dtype == "bf16"
    failures, rows = [], []
    nconv = 0
    standalone, through = set(), set()
    worst = dict(a=0.0, b=0.0, frac=0.0, ulp=0.0)
    for o in ops:
        who = f"{label} op {o['index']} '{o['name']}' {o['kind']} impl {o['impl']}"
        if o["kind"] == "conv":
            assert o["impl"] in (0, 1, 2, 3), f"{who}: no kernel chosen after a forward"
            # ---- the operand as the kernel saw it
            if o["impl"] == 2:
                assert (o["pool_op"] >= 0) != (o["up_op"] >= 0), f"{who}: impl 2 needs exactly one of pool_op / up_op"
            if o["impl"] == 2 and o["pool_op"] >= 0:
                x = F.max_pool2d(nchw(rd(ops[o["pool_op"]]["in"])), 2, 2, ceil_mode=True)
                through.add(o["pool_op"])
            elif o["impl"] == 2:
                u = ops[o["up_op"]]
                t, c0, c = o["in"]
                cu = u["out"][2]
                assert c0 == 0 and u["out"][0] == t and u["out"][1] == 0, f"{who}: the fused up-sample must fill the first channels of the conv's input"
                # the bilinear resize as the engine evaluates it, bit for bit (bilinear_f32): F.interpolate's other fp32 roundings flip the bf16
                # rounding of ~3e-4 of the operand's elements, and one such flip moves a near-zero output by tens of its floored ulps
                hi = bilinear_f32(nchw(rd(u["in"])).contiguous(), *tinfo[t]["shape"][1:3])
                if bf:
                    hi = bf16_round(hi)                                # rounded as the stand-alone kernel stores it (CsT<__bf16>::lerp2)
                x = torch.cat((hi, nchw(rd((t, cu, c - cu)))), 1)
                through.add(o["up_op"])
            else:
                x = nchw(rd(o["in"]))
            x = x[:, :o["cin"]].contiguous()
            w, b = folded[o["name"]]
            if bf:
                w = bf16_round(w)
            got = rd(o["out"])
            res = rd(o["res"]) if o["res"][0] >= 0 else None
            assert tuple(w.shape) == (o["out"][2], o["cin"], 3, 3), (who, tuple(w.shape))
            d = o["dil"]
            y64 = F.conv2d(x.double(), w.double(), None, padding=d, dilation=d) + b.double()[None, :, None, None]
            mag = F.conv2d(x.double().abs(), w.double().abs(), None, padding=d, dilation=d) + b.double().abs()[None, :, None, None]
            if o["act"] == 2:
                y64 = y64.relu()
            else:
                assert o["act"] == 0, (who, o["act"])
            if res is not None:                                       # activation first, then the block residual
                y64 = y64 + nchw(res).double()
                mag = mag + nchw(res).double().abs()
            y64, mag = y64.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
            assert got.shape == y64.shape, (who, got.shape, y64.shape)
            if not bool(torch.isfinite(got).all()):
                failures.append(f"{who} {tuple(got.shape)}: non-finite output: {_pattern(~torch.isfinite(got))}")
                continue
            f32_out = not bf or tinfo[o["out"][0]]["name"] in SIDES
            K = 9 * o["cin"]
            err = (got.double() - y64).abs()
            line = f"{who} Cin {o['cin']} dil {d} out {tuple(got.shape)}"
            if f32_out:
                bound = (K + 4) * EPS32 * mag
                use = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
                bad = err > bound
                worst["a"] = max(worst["a"], use)
                line += f": (a) worst |err| / bound {use:.3f}"
                if bool(bad.any()):
                    failures.append(f"{line}: {_pattern(bad)}")
                if not bf:
                    y32 = F.conv2d(x, w, b, padding=d, dilation=d)
                    if o["act"] == 2:
                        y32 = y32.relu()
                    if res is not None:
                        y32 = y32 + nchw(res)
                    floor = float((y32.permute(0, 2, 3, 1).double() - y64).pow(2).mean().sqrt())
                    rms = float(err.pow(2).mean().sqrt())
                    ratio = rms / floor if floor > 0 else (0.0 if rms == 0 else math.inf)
                    line += f", (b) rms {rms:.3e} / torch fp32 {floor:.3e} = {ratio:.2f}"
                    if got.numel() >= RMS_MIN_ELEMS:
                        worst["b"] = max(worst["b"], ratio)
                        if ratio > RMS_FACTOR:
                            k = min(8, err.numel())
                            top = torch.topk((err / bound.clamp_min(1e-300)).flatten(), k).values.tolist()
                            failures.append(f"{line} > {RMS_FACTOR}: largest |err| / bound(a) {[round(v, 3) for v in top]}")
                    else:
                        line += " (not asserted: < 1024 elements)"
            else:
                u = ulps_bf16(got, bf16_round(y64.float()))
                ndiff = int((u > 0).sum())
                frac = ndiff / u.numel()
                worst["frac"], worst["ulp"] = max(worst["frac"], frac), max(worst["ulp"], float(u.max()))
                line += f": (c) max ulp {float(u.max()):.2f}, differing {ndiff} of {u.numel()}"
                if float(u.max()) > 1.0:
                    failures.append(f"{line}: {_pattern(u > 1.0)}")
                elif ndiff > max(1, int(0.02 * u.numel())):
                    failures.append(f"{line} > max(1, 2 %): {_pattern(u > 0)}")
            rows.append(line)
            nconv += 1
        elif o["kind"] in ("pool", "up"):
            c = o["consumer"]
            if c >= 0 and ops[c]["impl"] == 2:
                continue                                              # did not launch: checked through its consumer (asserted below)
            x, got = nchw(rd(o["in"])), rd(o["out"])
            H, W = tinfo[o["out"][0]]["shape"][1:3]
            if o["kind"] == "pool":
                want = F.max_pool2d(x, 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
                assert tuple(want.shape[1:3]) == (H, W), (who, want.shape)
                if not torch.equal(got, want):
                    failures.append(f"{who} {tuple(got.shape)}: not bit-equal to max_pool2d: {_pattern(got != want)}")
            else:
                want = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
                own = bilinear_f32(x.contiguous(), H, W).permute(0, 2, 3, 1)       # ... and the fused consumers' reference operand: the same bits
                if not torch.equal(got, bf16_round(own) if bf else own):
                    failures.append(f"{who} {tuple(got.shape)}: not the bits of bilinear_f32: {_pattern(got != (bf16_round(own) if bf else own))}")
                if bf:
                    u = ulps_bf16(got, bf16_round(want))
                    ndiff = int((u > 0).sum())
                    worst["frac"] = max(worst["frac"], ndiff / u.numel())
                    if float(u.max()) > 1.0 or not bool(torch.isfinite(got).all()):
                        failures.append(f"{who} {tuple(got.shape)}: max ulp {float(u.max()):.2f}: {_pattern(~(u <= 1.0))}")
                    elif ndiff > max(1, int(0.02 * u.numel())):
                        failures.append(f"{who} {tuple(got.shape)}: {ndiff} of {u.numel()} elements differ > max(1, 2 %): {_pattern(u > 0)}")
                else:
                    tol = 8 * EPS32 * float(x.abs().max())
                    bad = ~((got - want).abs() <= tol)
                    if bool(bad.any()):
                        failures.append(f"{who} {tuple(got.shape)}: |got - interpolate| up to {float((got - want).abs().max()):.3e} > {tol:.3e}: {_pattern(bad)}")
            standalone.add(o["index"])
    # ---- coverage: the walk must not pass by checking nothing
    assert nconv == 118, f"{label}: {nconv} conv ops checked, the plan of either variant has 112 REBNCONVs + 6 side convs"
    pre = {o["index"] for o in ops if o["kind"] in ("pool", "up")}
    assert pre and pre == standalone | through and not (standalone & through), (sorted(pre - standalone - through), sorted(standalone & through))
    stats = dict(worst, rows=rows, impls=sorted({o["impl"] for o in ops if o["kind"] == "conv"}),
                 fused_pool=sum(1 for o in ops if o["kind"] == "conv" and o["impl"] == 2 and o["pool_op"] >= 0),
                 fused_up=sum(1 for o in ops if o["kind"] == "conv" and o["impl"] == 2 and o["up_op"] >= 0),
                 impl_by_cout={(o["out"][2], o["impl"]) for o in ops if o["kind"] == "conv"})
    return stats, failures


def check_tail(eng, folded, prob, norm, mask, label=""):
    """side maps -> fusion -> sigmoid -> normPRED -> mask of a whole-call forward, on the engine's own side maps / prob / norm"""
    failures = []
    prob, norm, mask = prob.cpu(), norm.cpu(), mask.cpu()
    B, H, W = prob.shape
    wf, bfuse = folded["outconv"]
    logit = torch.zeros(B, 1, H, W, dtype=torch.float64)
    for k, name in enumerate(SIDES):
        logit = logit + float(wf[0, k, 0, 0]) * up64(nchw(eng.read_tensor(name)).double(), H, W)
    want = torch.sigmoid(logit + float(bfuse[0]))[:, 0]
    err = (prob.double() - want).abs()
    print(f"{label} tail: max |prob - fp64| {float(err.max()):.3e}")
    if not bool((err <= PROB_TOL).all()):
        failures.append(f"{label} tail: |prob - fp64 fusion| up to {float(err.max()):.3e} > {PROB_TOL}: {_pattern((~(err <= PROB_TOL))[..., None])}")
    failures += check_norm(prob, norm, mask, label)
    return failures


def check_norm(prob, norm, mask, label=""):
    """normPRED over `prob` as one range (the whole call, or one crop): the range is exactly prob's min and max (norm reaches 0 and 1 there),
    norm within 1 fp32 ulp of the fp32 expression, mask from the engine's own norm bit for bit"""
    failures = []
    mi, ma = prob.min(), prob.max()
    assert float(ma) > float(mi), f"{label}: flat prob map, the case tests nothing"
    want = (prob - mi) / (ma - mi)
    if not (float(norm.min()) == 0.0 and float(norm.max()) == 1.0 and float(norm.flatten()[prob.argmin()]) == 0.0 and float(norm.flatten()[prob.argmax()]) == 1.0):
        failures.append(f"{label} normPRED: range is not [min, max] of the engine's prob: norm spans [{float(norm.min())!r}, {float(norm.max())!r}]")
    bad = ~((norm - want).abs() <= ulp32(want))
    if bool(bad.any()):
        failures.append(f"{label} normPRED: norm off by up to {float((norm - want).abs().max()):.3e} (> 1 fp32 ulp): {_pattern(bad[..., None])}")
    if not torch.equal(mask, (norm > 0.5).to(torch.uint8) * 255):
        failures.append(f"{label} mask != 255 (norm > 0.5): {_pattern((mask != (norm > 0.5).to(torch.uint8) * 255)[..., None])}")
    return failures


# ---- a GPU case -------------------------------------------------------------------------------------------------------------------------
def run_case(variant, dtype, shape, policy, monkeypatch):
    """fresh engine under `policy`, one forward of rand_image(shape), the walk and the tail. Returns the walk's stats; fails with every
    violated bound listed."""
    import time
    from helpers import rand_image
    from yolo_puncture_amd.u2net import U2NetEngine
    t0 = time.time()
    st, folded = case_state(variant)
    set_policy(monkeypatch, policy)
    label = f"[{variant} {dtype} {tuple(shape)} {policy}]"
    eng = U2NetEngine(variant, dtype, 0, state=st)
    try:
        prob, norm, mask = eng.forward(rand_image(tuple(shape) + (3,), seed=5).cuda())
        torch.cuda.synchronize()
        stats, failures = check_forward(eng, variant, dtype, folded, label)
        failures += check_tail(eng, folded, prob, norm, mask, label)
    finally:
        eng.close()
    stats["seconds"] = time.time() - t0
    print("\n".join(stats["rows"]))
    print(f"{label} SUMMARY impls {stats['impls']} fused pool / up {stats['fused_pool']} / {stats['fused_up']}: worst (a) {stats['a']:.3f}, worst (b) {stats['b']:.2f}, "
          f"worst bf16 ulp {stats['ulp']:.2f}, worst bf16 differing fraction {stats['frac']:.2e}, {stats['seconds']:.1f} s")
    assert not failures, f"{len(failures)} violations:\n" + "\n".join(failures)
    return stats
