"""Per-op contract of the EfficientNet-B3 classifier engine (csrc/effnet.hip: cls_stem / cls_pw / cls_dw / cls_se / cls_fc / cls_crop
kernels), fp32 and bf16: DESIGN.md sections 2 and 9.

One forward runs, then every op is held to a reference of THAT OP ALONE, built from the tensors the engine itself stored (read_tensor):
'stem', every '_blocks.{i}.expand' / '.dw' / '.gate' / '_blocks.{i}' (the projection's output) and 'head.pool' has its own arena slot and
is written once per forward. Weights are effnet_ref.fold's. The head conv's 12x12x1536 map is never stored, so it is checked through its
pool. With u = 2^-24, y64 the op in fp64 and S = |w| (*) |x| + |b| in fp64, the bounds (none comes from the kernels) are

 (a) fp32 convs, per element: before the activation |z - z64| <= (K + 4) u S with K = Cin k^2; after swish 1.1 x that + 4 u |y64|
     (|swish'| <= 1.1, plus the roundings of expf, the division and the product); with a residual + 2 u (|res| + |y64|). The projection's
     operand is the fp32 product dw * gate, one IEEE multiply of the engine's own dw and the engine's own gate, as the kernel forms it.
 (b) fp32 convs with >= 1024 outputs, per op: rms(got - y64) <= 4 rms(torch_fp32 - y64) (perop_u2net.RMS_FACTOR): what (a), 100-400 x
     loose at large K, cannot see.
 (c) bf16 convs: reference = bf16 rounding of y64 from bf16-rounded weights, the fp32 bias and the engine's own bf16-exact input (the
     projection's operand: bf16(fp32(dw * gate)) with the engine's own gate, so the operand is exact); perop_bf16.ulps_bf16 <= 1
     everywhere and at most 0.5 % of an op's elements differ. The head conv is not rounded (its output goes into the pool): (a) with
     bf16 weights, through (e).
 (d) SE gate, both dtypes: fp64 mean -> reduce -> swish -> expand -> sigmoid of the engine's own stored dw (bf16 mode: the rounded values,
     which are what the kernel sums), within a forward error bound propagated in fp64:
         dmean_c = (D + 1) u mean|v|_c, D = ceil(Wo / 8) + 7 + Ho (the longest addition chain through cls_dw_kernel and sum_chunks,
                   one more for the division)
         ds_j    = 1.1 (sum_c |wr_jc| dmean_c + (ceil(C / 64) + 8) u (sum |wr mean| + |br|)) + 4 u |s_j|
         dz_c    = sum_j |we_cj| ds_j + (sq + 2) u (sum |we s| + |be|)
         dgate   = dz / 4 + 4 u
 (e) head.pool: mean of the fp64 head conv + swish over the engine's own last block, within the mean of (a)'s per-element bounds
     + (ceil(HW / 32) + 8 + 2 + 1) u mean|v|.
 (f) tail, on the engine's own tensors: logits against the fp64 FC of the engine's own head.pool within (ceil(C / 64) + 8) u (sum |w p|
     + |b|); prob within 4 u of the fp64 max softmax of the engine's OWN logits; cls == int(l1 > l0) on the engine's own fp32 logits,
     exactly (a tie gives 0).
 (g) stem input: the 'input' tap, where the engine keeps it, is bit-equal to effnet_ref.normalise(effnet_ref.crop(...)), and that is
     the stem conv's operand.
`check_forward` takes anything with tensors() / read_tensor(name) (tests/test_effnet_perop_host.py feeds it a CPU emulation)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import effnet_ref as R
from perop_bf16 import ulps_bf16
from perop_u2net import RMS_FACTOR, RMS_MIN_ELEMS, _pattern

U = 2.0 ** -24
FRAC_CAP = 0.005           # (c)
PROB_TOL = 4 * U           # (f)
BLOCKS = R.blocks()
PADS = R.pads()


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def swish64(z):
    return z * torch.sigmoid(z)


def block_ops(i):
    p = f"_blocks.{i}"
    return ([f"{p}.expand"] if BLOCKS[i]["e"] != 1 else []) + [f"{p}.dw", f"{p}.gate", p]


def stage_ops(stage):
    return [n for i, b in enumerate(BLOCKS) if b["stage"] == stage for n in block_ops(i)]


def all_ops():
    return ["stem"] + [n for i in range(len(BLOCKS)) for n in block_ops(i)] + ["head.pool", "tail"]


def stage_of(name):
    return f"stage {BLOCKS[int(name.split('.')[1])]['stage']}" if name.startswith("_blocks.") else name


def make_case(seed=5):
    """The B = 2 case of the GPU and the host test: BGR uint8 frames [2,400,520,3] and xyxy boxes. Image 0 is a 400x520 frame with an
    interior box (the whole 380^2 window inside). Image 1 is a 300x360 frame padded with zeros into the same tensor; its box sits at
    the tensor's bottom-right corner, so the window is clipped on two sides to 260x260 and lands at the top-left of the zero crop: the
    crop holds frame pixels, the frame's own zero padding and crop_frame's zero padding. After normalisation zero uint8 is -mean / std,
    not 0, and the convs' SAME padding is 0."""
    rng = np.random.RandomState(seed)
    H, W = 400, 520
    fr = np.zeros((2, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b, (h, w) in enumerate(((H, W), (300, 360))):
        noise = rng.randint(0, 256, (h, w, 3)).astype(np.int16)
        blob = (np.sin(xx[:h, :w] / (37 + 11 * b)) * np.cos(yy[:h, :w] / (23 + 5 * b)) * 100).astype(np.int16)
        fr[b, :h, :w] = np.clip(noise // 2 + 64 + blob[..., None], 0, 255).astype(np.uint8)
    return fr, [(200, 150, 320, 260), (420, 300, 480, 360)]


def ref_input(frames_bgr, boxes):
    """(g): the normalised 380^2 crops [B,3,380,380] the stem reads"""
    return R.normalise(np.stack([R.crop(f[..., ::-1], bx) for f, bx in zip(frames_bgr, boxes)]))


def _conv_ref(x, w, b, stride, pp, groups, act, res, dt):
    """conv (static pad pp) + bias [+ swish] [+ res] in dt"""
    y = F.conv2d(R._pad(x.to(dt), pp), w.to(dt), b.to(dt), stride=stride, groups=groups)
    if act:
        y = swish64(y)
    return y if res is None else y + res.to(dt)


def conv_bounds(x, w, b, stride, pp, groups, act, res, K):
    """(y64, per-element bound (a)) of one conv op, NCHW fp64"""
    z = F.conv2d(R._pad(x.double(), pp), w.double(), b.double(), stride=stride, groups=groups)
    S = F.conv2d(R._pad(x.double().abs(), pp), w.double().abs(), b.double().abs(), stride=stride, groups=groups)
    bound = (K + 4) * U * S
    y = z
    if act:
        y = swish64(z)
        bound = 1.1 * bound + 4 * U * y.abs()
    if res is not None:
        y = y + res.double()
        bound = bound + 2 * U * (res.double().abs() + y.abs())
    return y, bound


def gate_bounds(v, wr, br, we, be):
    """(d): v = the stored depthwise output NHWC; returns (gate64 [B,C], dgate [B,C])"""
    B, Ho, Wo, C = v.shape
    sq = wr.shape[0]
    v = v.double()
    wr, br, we, be = wr.double().view(sq, C), br.double(), we.double().view(C, sq), be.double()
    mean, mabs = v.mean((1, 2)), v.abs().mean((1, 2))
    D = math.ceil(Wo / 8) + 7 + Ho
    dmean = (D + 1) * U * mabs
    s = swish64(mean @ wr.T + br)
    ds = 1.1 * (dmean @ wr.abs().T + (math.ceil(C / 64) + 8) * U * (mean.abs() @ wr.abs().T + br.abs())) + 4 * U * s.abs()
    z = s @ we.T + be
    dz = ds @ we.abs().T + (sq + 2) * U * (s.abs() @ we.abs().T + be.abs())
    return torch.sigmoid(z), dz / 4 + 4 * U


def tail_failures(state, pool, out, label=""):
    """(f) on the engine's own head.pool [B,C] and its returned (logits, prob, cls)"""
    logits, prob, cls = (t.detach().cpu() for t in out)
    fails = []
    w, b = state["_fc.weight"].double(), state["_fc.bias"].double()
    P = pool.double()
    C = P.shape[1]
    want = P @ w.T + b
    bound = (math.ceil(C / 64) + 8) * U * (P.abs() @ w.abs().T + b.abs())
    err = (logits.double() - want).abs()
    use = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    line = f"{label} op 'tail' fc: (f) logits {logits.tolist()} worst |err| / bound {use:.3f}"
    if not bool((err <= bound).all()) or not bool(torch.isfinite(logits).all()):
        fails.append(f"{line}: images {(~(err <= bound)).any(1).nonzero().flatten().tolist()}, fp64 FC of the engine's pool {want.tolist()}")
    p64 = torch.softmax(logits.double(), 1).max(1).values
    perr = (prob.double() - p64).abs()
    line += f", max |prob - fp64| {float(perr.max()):.3e}"
    if not bool((perr <= PROB_TOL).all()):
        fails.append(f"{label} op 'tail' softmax: (f) |prob - fp64 max softmax of the engine's logits| up to {float(perr.max()):.3e} > {PROB_TOL:.3e}: "
                     f"images {(~(perr <= PROB_TOL)).nonzero().flatten().tolist()}, prob {prob.tolist()}")
    wc = (logits[:, 1] > logits[:, 0]).long()
    if not torch.equal(cls.long(), wc):
        fails.append(f"{label} op 'tail' argmax: (f) cls {cls.tolist()} != int(l1 > l0) {wc.tolist()} on the engine's own logits {logits.tolist()}")
    return line, dict(f=use, prob=float(perr.max())), fails


def check_forward(eng, state, frames, boxes, dtype, out=None, ops=None, label=""):
    """Walk stem -> 26 blocks -> head -> tail after one forward of (frames BGR uint8 [B,H,W,3], boxes) and hold every op (or those named
    in `ops`: 'stem', '_blocks.{i}.expand' / '.dw' / '.gate', '_blocks.{i}', 'head.pool', 'tail') to its bound. `out` is the forward's
    (logits, prob, cls), needed by 'tail'. Returns (stats, failures): every violated bound is one line naming the op and where the bad
    elements sit; stats['ops'][name] holds the op's figures, stats['rows'] one printable line per op."""
    assert dtype in ("fp32", "bf16"), dtype
    bf = dtype == "bf16"
    names = all_ops()
    want = set(names if ops is None else ops)
    assert want <= set(names), sorted(want - set(names))
    have = {t["name"]: tuple(t["shape"]) for t in eng.tensors()}
    cache = {}

    def rd(name):                                   # NCHW view of the engine's NHWC tensor
        if name not in cache:
            cache[name] = eng.read_tensor(name)
        return cache[name].permute(0, 3, 1, 2)

    failures, rows, per = [], [], {}
    wq = (lambda w: bf16_round(w)) if bf else (lambda w: w)

    def conv_op(name, kind, x, w, b, stride=1, pp=(0, 0), groups=1, act=True, res=None):
        who = f"{label} op '{name}' {kind}"
        K = w.shape[1] * w.shape[2] * w.shape[3]
        w = wq(w)
        got = rd(name)
        y64, bound = conv_bounds(x, w, b, stride, pp, groups, act, res, K)
        assert got.shape == y64.shape, (who, tuple(got.shape), tuple(y64.shape))
        line = f"{who} K {K} out {tuple(got.shape)}"
        st = dict(kind=kind)
        nhwc = lambda t: t.permute(0, 2, 3, 1)
        if not bool(torch.isfinite(got).all()):
            failures.append(f"{line}: non-finite output: {_pattern(nhwc(~torch.isfinite(got)))}")
            rows.append(line)
            per[name] = st
            return
        err = (got.double() - y64).abs()
        if not bf:
            use = float((err / bound.clamp_min(1e-300)).max())
            floor = float((_conv_ref(x, w, b, stride, pp, groups, act, res, torch.float32).double() - y64).pow(2).mean().sqrt())
            rms = float(err.pow(2).mean().sqrt())
            ratio = rms / floor if floor > 0 else (0.0 if rms == 0 else math.inf)
            st.update(a=use, b=ratio)
            line += f": (a) worst |err| / bound {use:.3f}, (b) rms {rms:.3e} / torch fp32 {floor:.3e} = {ratio:.2f}"
            if bool((err > bound).any()):
                failures.append(f"{line}: (a) violated: {_pattern(nhwc(err > bound))}")
            if got.numel() >= RMS_MIN_ELEMS and ratio > RMS_FACTOR:
                top = torch.topk((err / bound.clamp_min(1e-300)).flatten(), min(8, err.numel())).values.tolist()
                failures.append(f"{line}: (b) violated, > {RMS_FACTOR}: largest |err| / bound(a) {[round(v, 3) for v in top]}")
        else:
            u = ulps_bf16(got, y64.to(torch.bfloat16).float())
            ndiff = int((u > 0).sum())
            frac = ndiff / u.numel()
            st.update(ulp=float(u.max()), frac=frac)
            line += f": (c) max ulp {float(u.max()):.2f}, differing {ndiff} of {u.numel()} ({100 * frac:.4f} %)"
            if float(u.max()) > 1.0:
                failures.append(f"{line}: (c) violated, > 1 ulp: {_pattern(nhwc(u > 1.0))}")
            elif frac > FRAC_CAP:
                failures.append(f"{line}: (c) violated, > {100 * FRAC_CAP} % differ: {_pattern(nhwc(u > 0))}")
        rows.append(line)
        per[name] = st

    if "stem" in want:
        x = ref_input(frames, boxes)
        if "input" in have and have["input"][0] > 0:                                         # (g)
            try:
                tap = eng.read_tensor("input")
            except Exception:
                tap = None                                                                  # not kept by this engine
            if tap is not None and not torch.equal(tap, x.permute(0, 2, 3, 1)):
                failures.append(f"{label} op 'stem' crop: (g) input tap is not bit-equal to normalise(crop): {_pattern(tap != x.permute(0, 2, 3, 1))}")
        conv_op("stem", "stem conv", x, *R.fold(state, "_conv_stem", "_bn0"), stride=2, pp=PADS["_conv_stem"])
    for i, bl in enumerate(BLOCKS):
        p = f"_blocks.{i}"
        if not (set(block_ops(i)) & want):
            continue
        inp = rd("stem" if i == 0 else f"_blocks.{i - 1}")
        if f"{p}.expand" in want:
            conv_op(f"{p}.expand", "expand 1x1", inp, *R.fold(state, f"{p}._expand_conv", f"{p}._bn0"))
        if f"{p}.dw" in want:
            xin = rd(f"{p}.expand") if bl["e"] != 1 else inp
            conv_op(f"{p}.dw", f"depthwise k{bl['k']} s{bl['s']}", xin, *R.fold(state, f"{p}._depthwise_conv", f"{p}._bn1"), stride=bl["s"],
                    pp=PADS[f"{p}._depthwise_conv"], groups=xin.shape[1])
        if f"{p}.gate" in want:
            got = rd(f"{p}.gate")[:, :, 0, 0]
            g64, dg = gate_bounds(rd(f"{p}.dw").permute(0, 2, 3, 1), state[f"{p}._se_reduce.weight"], state[f"{p}._se_reduce.bias"],
                                  state[f"{p}._se_expand.weight"], state[f"{p}._se_expand.bias"])
            err = (got.double() - g64).abs()
            use = float((err / dg).max())
            line = f"{label} op '{p}.gate' SE: (d) worst |err| / bound {use:.3f} (bound up to {float(dg.max()):.2e})"
            if not bool((err <= dg).all()):
                failures.append(f"{line}: (d) violated: {_pattern((~(err <= dg))[:, None, None, :])}")
            rows.append(line)
            per[f"{p}.gate"] = dict(kind="SE", d=use)
        if p in want:
            dw, g = rd(f"{p}.dw"), rd(f"{p}.gate")
            xg = dw * g                                   # one IEEE fp32 multiply, the engine's own dw and the engine's own gate
            xg = bf16_round(xg) if bf else xg
            res = inp if (bl["s"] == 1 and bl["cin"] == bl["cout"]) else None
            conv_op(p, "project 1x1" + (" + residual" if res is not None else ""), xg, *R.fold(state, f"{p}._project_conv", f"{p}._bn2"), act=False, res=res)
    pool = None
    if "head.pool" in want or "tail" in want:
        pool = rd("head.pool")[:, :, 0, 0]
    if "head.pool" in want:
        x = rd(f"_blocks.{len(BLOCKS) - 1}")
        w, b = R.fold(state, "_conv_head", "_bn1")
        y64, bound = conv_bounds(x, wq(w), b, 1, (0, 0), 1, True, None, w.shape[1])
        HW = y64.shape[2] * y64.shape[3]
        ref = y64.mean((2, 3))
        pb = bound.mean((2, 3)) + (math.ceil(HW / 32) + 8 + 2 + 1) * U * y64.abs().mean((2, 3))
        err = (pool.double() - ref).abs()
        use = float((err / pb).max())
        line = f"{label} op 'head.pool' head 1x1 + pool K {w.shape[1]} HW {HW}: (e) worst |err| / bound {use:.3f}"
        if not bool((err <= pb).all()):
            failures.append(f"{line}: (e) violated: {_pattern((~(err <= pb))[:, None, None, :])}")
        rows.append(line)
        per["head.pool"] = dict(kind="pool", e=use)
    if "tail" in want:
        assert out is not None, "the tail needs the forward's (logits, prob, cls)"
        line, st, fails = tail_failures(state, pool, out, label)
        rows.append(line)
        per["tail"] = dict(kind="tail", **st)
        failures += fails
    assert set(per) == want, sorted(want - set(per))                       # the walk must not pass by checking nothing
    worst = {k: max([s[k] for s in per.values() if k in s], default=0.0) for k in ("a", "b", "ulp", "frac", "d", "e", "f", "prob")}
    return dict(worst, ops=per, rows=rows), failures


def summarise(stats, label=""):
    """per-stage maxima of every figure, one line per stage: what DESIGN section 9 records"""
    by = {}
    for name, st in stats["ops"].items():
        d = by.setdefault(stage_of(name), {})
        for k, v in st.items():
            if k != "kind":
                d[k] = max(d.get(k, 0.0), v)
    return [f"{label} {s}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(d.items())) for s, d in by.items()]
