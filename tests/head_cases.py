"""Crafted inputs of the two post-process heads and their references (no GPU in here).

tests/test_gpu_head_crafted.py writes these tensors over a real engine's head inputs (Engine.write_tensor; they are fp32 in both numeric
modes) and launches the class-max ops and the head op on them (Engine.run_op); tests/test_head_cases_host.py checks on the CPU that every
case does what its name says. Both take their case ids from V10_CASES / NMS_CASES below.

A maker returns flat tensors over the image's anchors (level 0 first, row-major: the engine's anchor index): class logits [B, A, nc],
DFL bin indices [B, A, 4] (one-hot cases) or box logits [B, A, 64], mask coefficients [B, A, 32]. `tensors` splits them into the three
levels' [B, H, W, C] maps. The references are the project's own - Oracle.decode + v10_postprocess, and decode + the xywh round trip +
nms_postprocess - applied to those tensors in fp32 and in fp64.

What makes the comparison sharp:
  boxes   one-hot DFL logits (+30 at bin q, -30 elsewhere) decode to the integer distance q exactly (exp(-60) vanishes against 1.0 in
          fp32 and in fp64), so corners, areas and IoUs are exact small multiples of the stride and compare with torch.equal;
  scores  two logits of a case are either equal or so far apart that their float32 sigmoids differ by >= 1e-5: logits live on a 1/64
          grid in [-6, 6] (sigmoid' >= 2.4e-3 there), on a 1/8 grid in [7, 9], at -10 / -80 (floors) and at 20 / 25 / 30 (exactly 1.0f);
          none lies in (15, 17.5), where two sigmoid implementations may disagree about saturation, and none below -80 (denormals).
          The engine's 1/(1+expf(-x)) and torch's sigmoid are independent programs: score VALUES get 2e-7 absolute (the tolerance
          perop_bf16.py uses for the same pair), score ORDER and ties are exact."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import torch

from oracle.yolo_seg_oracle import nms_postprocess
from oracle.yolov10_oracle import Oracle, v10_postprocess

B = 2
CAP = 12288            # csrc/head_select.h: LDS key capacity of a stage-2 round
NCAP = 16384           # csrc/head_nms_common.h: sorted-key capacity of the NMS kernel
SCORE_TOL = 2e-7
SHAPES = {"S": (160, 192), "M": (512, 640), "L": (640, 640), "XL": (800, 768)}      # 630 / 6720 / 8400 / 12600 anchors


def levels(shape):
    H, W = SHAPES[shape]
    return [(H // s, W // s) for s in (8, 16, 32)]


def n_anchors(shape):
    return sum(h * w for h, w in levels(shape))


def grid(lo, hi):
    """the 1/64 logit grid on [lo, hi] (exact in float32)"""
    return torch.arange(round(lo * 64), round(hi * 64) + 1, dtype=torch.float32) / 64.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(key).encode()))


def _pick(values, n, g, replace=True):
    if replace:
        return values[torch.randint(0, values.numel(), (n,), generator=g)]
    assert n <= values.numel(), (n, values.numel())
    return values[torch.randperm(values.numel(), generator=g)[:n]]


def onehot_box_logits(dist):
    """DFL bin indices [..., 4] (0..15) -> box logits [..., 64]: +30 at the bin, -30 elsewhere"""
    out = torch.full(dist.shape[:-1] + (4, 16), -30.0)
    out.scatter_(-1, dist.long().unsqueeze(-1), 30.0)
    return out.reshape(dist.shape[:-1] + (64,))


def anchor(shape, l, y, x):
    hw = levels(shape)
    return sum(h * w for h, w in hw[:l]) + y * hw[l][1] + x


# ---------------------------------------------------------------------------------------------------------------------------------
# v10 (top-k head)
# ---------------------------------------------------------------------------------------------------------------------------------
V10Case = namedtuple("V10Case", "pattern nc max_det shape seg rounds")      # rounds: stage-2 rounds of the image with the most candidates (CAP per round)
# expectations the host test asserts, per pattern: filter ("on" / "off"), tie1 / tie2 (a tie
# group across anchor k of stage 1 / row k of stage 2), sat (saturated scores: the fp64 reference orders them differently)
V10_EXPECT = {
    "all_equal": dict(filter="on", tie1=True, tie2=True),
    "filter_off": dict(filter="off"),
    "tie_stage2": dict(filter="on", tie2=True, multi=True),
    "tie_stage1": dict(filter="on", tie1=True),
    "saturated": dict(filter="off", tie1=True, tie2=True, sat=True, multi=True),
    "thr_zero": dict(filter="on", tie1=True, tie2=True),
    "equal_vs_random": dict(filter="on"),
    "random": dict(filter="on"),
}
V10_CASES = [
    V10Case("all_equal", 80, 300, "S", False, 2),          # 24000 candidates reach the threshold: two rounds, rows are ranks 0..3
    V10Case("filter_off", 80, 300, "S", False, 2),         # every winner's maximum >= logit 7: thr >= 0.999, two rounds
    V10Case("tie_stage2", 80, 300, "S", False, 1),
    V10Case("tie_stage1", 80, 300, "S", False, 1),
    V10Case("saturated", 80, 300, "S", False, 2),
    V10Case("thr_zero", 80, 300, "S", False, 2),
    V10Case("equal_vs_random", 80, 300, "S", False, 2),    # (image 0 takes two rounds, image 1 one)
    V10Case("all_equal", 30, 512, "S", False, 2),          # scalar scan, 15360 candidates: two rounds
    V10Case("random", 1, 300, "S", False, 1),
    V10Case("random", 3, 300, "S", False, 1),
    V10Case("random", 80, 1, "S", False, 1),
    V10Case("random", 80, 7, "S", False, 1),
    V10Case("tie_stage2", 80, 512, "S", False, 1),
    V10Case("tie_stage2", 80, 480, "S", True, 1),          # segment engines: up to 480 rows, coefficients of the kept rows
    V10Case("all_equal", 80, 300, "XL", False, 2),         # head_select_large_kernel
    V10Case("saturated", 80, 300, "XL", False, 2),
]


def v10_id(c):
    return f"{c.pattern}-nc{c.nc}-k{c.max_det}-{c.shape}" + ("-seg" if c.seg else "")


def _v10_cls(c):
    A, nc, k = n_anchors(c.shape), c.nc, min(c.max_det, n_anchors(c.shape))
    g = _gen("v10", v10_id(c))
    rnd = lambda lo, hi: _pick(grid(lo, hi), B * A * nc, g).reshape(B, A, nc)
    p = c.pattern
    if p == "all_equal":
        return torch.stack([torch.full((A, nc), -3.0), torch.full((A, nc), -1.5)])
    if p == "equal_vs_random":
        cls = rnd(-6, 6)
        cls[0] = -3.0
        return cls
    if p == "random":
        return rnd(-6, 6)
    if p == "filter_off":        # 1..3 classes per anchor in [7, 9] (1/8 apart: sigmoids >= 1.4e-5 apart), the rest anywhere below
        cls = rnd(-6, 6)
        hi = 7.0 + torch.arange(17, dtype=torch.float32) / 8.0
        for b in range(B):
            for a in range(A):
                n = int(torch.randint(1, 4, (1,), generator=g))
                cls[b, a, torch.randperm(nc, generator=g)[:n]] = _pick(hi, n, g)
        return cls
    if p == "saturated":         # 1.5 k anchors with 1..3 classes at 20 / 25 / 30, all 1.0f
        cls = rnd(-6, 6)
        sat = torch.tensor([20.0, 25.0, 30.0])
        for b in range(B):
            for a in torch.randperm(A, generator=g)[:k + k // 2].tolist():
                n = int(torch.randint(1, 4, (1,), generator=g))
                cls[b, a, torch.randperm(nc, generator=g)[:n]] = _pick(sat, n, g)
        return cls
    if p == "thr_zero":          # k / 2 anchors with a real score; everything else at the floor the rules allow
        cls = torch.full((B, A, nc), -80.0)
        for b in range(B):
            at = torch.randperm(A, generator=g)[:k // 2]
            cls[b, at, torch.randint(0, nc, (k // 2,), generator=g)] = _pick(grid(-6, 6), k // 2, g, replace=False)
        return cls
    if p in ("tie_stage2", "tie_stage1"):
        v = 0.0                  # the tied logit; singles above it are distinct, everything else lies a logit or more below
        cls = rnd(-6, v - 1.0)
        for b in range(B):
            perm = torch.randperm(A, generator=g)
            if p == "tie_stage2":    # 2k/3 single winners + k/5 anchors with 4 tied classes each: 0.8 k tied candidates for k/3 rows
                nhi, nt, per = 2 * k // 3, k // 5, 4
            else:                    # 5k/6 single winners + k/3 anchors tied on their maximum for k/6 places
                nhi, nt, per = 5 * k // 6, k // 3, 1
            hi_at, tie_at = perm[:nhi], perm[nhi:nhi + nt]
            cls[b, hi_at, torch.randint(0, nc, (nhi,), generator=g)] = _pick(grid(v + 0.5, 6), nhi, g, replace=False)
            for a in tie_at.tolist():
                cls[b, a, torch.randperm(nc, generator=g)[:per]] = v
            if p == "tie_stage2":    # and some single winners carry a second, lower class that makes the rows too
                two = hi_at[:nhi // 8]
                cls[b, two, (cls[b, two].argmax(1) + 1) % nc] = v + 0.25
        return cls
    raise KeyError(p)


@functools.lru_cache(maxsize=None)
def v10_inputs(c):
    """-> dict(cls [B,A,nc], dist [B,A,4] int64, box [B,A,64], cf [B,A,32])"""
    A = n_anchors(c.shape)
    g = _gen("v10box", v10_id(c))
    cls = _v10_cls(c)
    assert cls.shape == (B, A, c.nc) and cls.dtype == torch.float32 and not torch.equal(cls[0], cls[1])
    dist = torch.randint(0, 16, (B, A, 4), generator=g)
    return dict(cls=cls, dist=dist, box=onehot_box_logits(dist), cf=torch.randn(B, A, 32, generator=g))


def _decode(shape, box, cls, dt):
    o = Oracle.__new__(Oracle)          # decode reads nothing but the working dtype: no weights needed
    o.dt = dt
    return o.decode(box.to(dt).permute(0, 2, 1).contiguous(), cls.to(dt).permute(0, 2, 1).contiguous(), levels(shape))


@functools.lru_cache(maxsize=None)
def v10_reference(c, mode="fp32"):
    """-> det [B,k,6] (float32), anchor idx [B,k], boxes of all anchors [B,A,4] (in the mode's dtype)"""
    t = v10_inputs(c)
    boxes, scores = _decode(c.shape, t["box"], t["cls"], torch.float64 if mode == "fp64" else torch.float32)
    det, idx = v10_postprocess(boxes, scores, max_det=c.max_det)
    return det.float(), idx, boxes


def v10_stage_stats(c, b):
    """What the select kernel meets on image b, from the float32 reference: stage-1 threshold, whether the logit filter is on, the
    (rank, class) candidates that reach its logit, and the tie groups at the two cuts."""
    cls = v10_inputs(c)["cls"][b]
    A, nc = cls.shape
    k = min(c.max_det, A)
    s = cls.sigmoid()
    m = s.amax(1)
    order = torch.sort(m, descending=True, stable=True).indices
    thr = float(m[order[k - 1]])
    on = 0.0 < thr < 0.999
    rows = cls[order[:k]]
    if on:
        t32 = torch.tensor(thr, dtype=torch.float32)
        lthr = float(torch.log(t32 / (1.0 - t32))) - 1e-3
        # (every logit of a case is equal to the threshold's or >= 1/64 away from it: the count does not hang on the filter's rounding)
        assert not bool(((rows - lthr).abs() < 5e-4).any())
        ncand = int((rows >= lthr).sum())
    else:
        ncand = k * nc
    s2 = torch.sort(s[order[:k]].flatten(), descending=True, stable=True).values
    per_anchor = torch.bincount(v10_reference(c)[1][b], minlength=A)
    return dict(thr=thr, filter="on" if on else "off", ncand=ncand, tie1=k < A and bool(m[order[k - 1]] == m[order[k]]),
                tie2=k < k * nc and bool(s2[k - 1] == s2[k]), multi=int(per_anchor.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# v8 / 11 (NMS head)
# ---------------------------------------------------------------------------------------------------------------------------------
NmsCase = namedtuple("NmsCase", "name shape conf iou max_det")
NMS_CASES = [
    NmsCase("none_and_many", "S", 0.25, 0.7, 300),      # no candidate in image 0; 350 disjoint survivors in image 1: the first 300
    NmsCase("n1_n32", "S", 0.25, 0.7, 300),
    NmsCase("n33_conf_edge", "S", 0.5, 0.7, 300),       # 33 candidates; scores exactly at conf stay out
    NmsCase("conf_zero", "S", 0.0, 0.5, 300),           # every anchor a candidate, more than 300 survive
    NmsCase("same_box", "S", 0.25, 0.5, 300),           # one box in two classes (both kept) / in one class (second dropped)
    NmsCase("iou_exact", "S", 0.25, 0.5, 300),          # IoU == iou stays, the next larger IoU goes
    NmsCase("iou_exact", "S", 0.25, 0.7, 300),
    NmsCase("chain", "S", 0.25, 0.5, 300),              # A > B, B > C, A does not reach C: C stays
    NmsCase("equal_scores", "S", 0.25, 0.5, 300),       # overlapping pairs with one score, on a level and across levels: lower anchor stays
    NmsCase("argmax", "S", 0.25, 0.5, 300),             # first maximum of the sigmoid scores: equal logits, logits 20 and 30
    NmsCase("many_k480", "S", 0.25, 0.7, 480),
    NmsCase("blocks", "M", 0.0, 0.5, 300),              # np2 = 8192, ncache = 3276: pairs on both sides of the LDS box cache
    NmsCase("blocks", "L", 0.0, 0.5, 300),              # np2 = NCAP, ncache = 0
    NmsCase("random_boxes", "S", 0.25, 0.7, 300),       # not one-hot: floats against the references' noise floor
    NmsCase("large_gather", "XL", 0.5, 0.5, 300),       # head_nms_gather_kernel + head_nms_large_kernel
]
NC = 80
BG = -6.0


def nms_id(c):
    return f"{c.name}-{c.shape}-conf{c.conf:g}-iou{c.iou:g}-k{c.max_det}"


def ncache_of(n):
    """(np2, ncache) of nms_sort_sweep_rows for n candidates"""
    np2 = 2
    while np2 < n:
        np2 <<= 1
    return np2, min(n, ((NCAP - np2) * 8) // 20)


class _Scene:
    """class logits at the background value, every box the anchor's own cell (l, t, r, b) = (0, 0, 1, 1): boxes of one level are disjoint,
    boxes of two levels overlap with IoU <= 0.25"""

    def __init__(self, shape, bg=BG):
        self.shape, self.A = shape, n_anchors(shape)
        self.cls = torch.full((B, self.A, NC), bg)
        self.dist = torch.tensor([0, 0, 1, 1]).repeat(B, self.A, 1)
        self.info = {}

    def put(self, b, a, c, logit, ltrb=None):
        self.cls[b, a, c] = logit
        if ltrb is not None:
            self.dist[b, a] = torch.tensor(ltrb)

    def scatter(self, b, n, g, values, exclude=()):
        """n anchors outside `exclude`, one random class each, logits drawn from `values` without replacement"""
        free = torch.ones(self.A, dtype=torch.bool)
        free[list(exclude)] = False
        at = torch.nonzero(free).squeeze(1)
        at = at[torch.randperm(at.numel(), generator=g)[:n]]
        self.cls[b, at, torch.randint(0, NC, (n,), generator=g)] = _pick(values, n, g, replace=False)
        return at


def _blocks(c, g, sc):
    """Every anchor a candidate (conf = 0). The anchors of an 8x8 block of a level all decode to ONE box (l = x % 8, r = 7 - x % 8, ...)
    and carry the block's class: the first of a block in the sorted list survives and suppresses the other 63 wherever they sit.
    Sorted position -> anchor is known by construction (info["order"]): positions 31 and 32 open two reserved blocks, and the anchors of
    four `late` blocks fill the end of the list, so their survivors and victims both lie beyond any box cache."""
    A, hw = sc.A, levels(c.shape)
    block_of, nblk = torch.empty(A, dtype=torch.long), 0
    for l, (h, w) in enumerate(hw):
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        a0 = anchor(c.shape, l, 0, 0)
        block_of[a0:a0 + h * w] = (nblk + (y // 8) * ((w + 7) // 8) + x // 8).flatten()
        d = torch.stack((x % 8, y % 8, 7 - x % 8, 7 - y % 8), -1).reshape(-1, 4)
        sc.dist[:, a0:a0 + h * w] = d
        nblk += ((h + 7) // 8) * ((w + 7) // 8)
    orders = []
    for b in range(B):
        bperm = torch.randperm(nblk, generator=g)
        late, reserved = bperm[:4], bperm[4:6]
        is_late, is_res = torch.isin(block_of, late), torch.isin(block_of, reserved)
        early = torch.nonzero(~is_late & ~is_res).squeeze(1)
        early = early[torch.randperm(early.numel(), generator=g)]
        res = [torch.nonzero(block_of == r).squeeze(1) for r in reserved]
        rest = torch.cat((early[31:], res[0][1:], res[1][1:]))
        rest = rest[torch.randperm(rest.numel(), generator=g)]
        tail = torch.nonzero(is_late).squeeze(1)
        tail = tail[torch.randperm(tail.numel(), generator=g)]
        order = torch.cat((early[:31], res[0][:1], res[1][:1], rest, tail))
        assert order.numel() == A and torch.unique(order).numel() == A
        # logits by sorted position: the first 64 distinct, then groups of G on one grid value (ordered by anchor inside a group)
        G = -(-(A - 64) // 700)
        pos = torch.arange(A)
        lvl = torch.where(pos < 64, pos, 64 + (pos - 64) // G)
        for s in range(64, A, G):
            order[s:s + G] = torch.sort(order[s:s + G]).values
        logit = 6.0 - lvl.float() / 64.0
        assert float(logit.min()) >= -6.0
        sc.cls[b, order, block_of[order] % NC] = logit
        orders.append(order)
        sc.info[f"late{b}"], sc.info[f"reserved{b}"] = late, reserved
    sc.info["order"], sc.info["block_of"] = orders, block_of


def _nms_scene(c):
    g = _gen("nms", nms_id(c._replace(max_det=0)))      # (the scene does not depend on max_det)
    S = c.shape
    sc = _Scene(S, bg=-10.0 if c.name in ("conf_zero", "blocks") else BG)
    above = grid(-1.0, 6.0)               # sigmoid(-1) = 0.269 > 0.25
    n = c.name
    if n == "none_and_many":
        sc.scatter(1, 350, g, above)
    elif n == "many_k480":
        sc.scatter(0, 520, g, torch.cat((above, above)))
        sc.scatter(1, 30, g, above)
    elif n == "n1_n32":
        sc.scatter(0, 1, g, above)
        sc.scatter(1, 32, g, above)
    elif n == "n33_conf_edge":            # conf = 0.5 = sigmoid(0) in any implementation
        sc.scatter(0, 33, g, grid(0.25, 6))
        at = sc.scatter(1, 15, g, grid(0.25, 6))
        used = set(at.tolist())
        free = [a for a in torch.randperm(sc.A, generator=g).tolist() if a not in used][:10]
        for a in free:
            sc.put(1, a, int(torch.randint(0, NC, (1,), generator=g)), 0.0)
        sc.info["edge"] = free
    elif n == "conf_zero":
        # one class per anchor on the grid; 20 pairs of neighbours on level 0 with 3/5 IoU in one class: the lower-scoring one goes
        for b in range(B):
            sc.cls[b, torch.arange(sc.A), torch.randint(0, NC, (sc.A,), generator=g)] = _pick(grid(-5, 6), sc.A, g)
            rows = torch.randperm(20, generator=g)
            for i in range(20):
                y, x = int(rows[i]), int(torch.randint(0, 19, (1,), generator=g))
                a0 = anchor(S, 0, y, x)
                for a, lg in ((a0, 5.0 - i / 8.0), (a0 + 1, 4.9375 - i / 8.0)):
                    sc.cls[b, a] = -10.0
                    sc.put(b, a, 11, lg, (0, 0, 4, 1))
    elif n == "same_box":
        for b, classes in ((0, (3, 7)), (1, (7, 7))):
            sc.put(b, anchor(S, 0, 5, 5), classes[0], 3.0, (0, 0, 3, 2))
            sc.put(b, anchor(S, 0, 5, 6), classes[1], 2.0, (1, 0, 2, 2))
            sc.scatter(b, 20 + b, g, grid(-1, 1.5), exclude=[anchor(S, 0, 5, 5), anchor(S, 0, 5, 6)])
        sc.info["pair"] = (anchor(S, 0, 5, 5), anchor(S, 0, 5, 6))
    elif n == "iou_exact":
        # iou 0.5: boxes 3 wide, 1 apart (2 / 4), control 4 wide, 1 apart (3 / 5); iou 0.7: boxes 17 wide, 3 apart (14 / 20), control 2 apart (15 / 19)
        (ltrb, step), (ltrb_c, step_c) = (((0, 0, 3, 1), 1), ((0, 0, 4, 1), 1)) if c.iou == 0.5 else (((2, 0, 15, 1), 3), ((2, 0, 15, 1), 2))
        x0 = 3
        pairs = []
        for b, (l, cl) in enumerate(((0, 0), (1, 79))):          # level 0 / class 0; level 1 / class 79 (the largest class offset)
            assert x0 + step < levels(S)[l][1]
            at, closer = anchor(S, l, 2, x0), anchor(S, l, 6, x0)
            sc.put(b, at, cl, 3.0, ltrb); sc.put(b, at + step, cl, 2.0, ltrb)                 # exactly at iou: both stay
            sc.put(b, closer, cl, 3.5, ltrb_c); sc.put(b, closer + step_c, cl, 2.5, ltrb_c)   # above: the second goes
            pairs.append((at, at + step, closer, closer + step_c))
            sc.scatter(b, 12 + b, g, grid(-1, 1.5), exclude=list(pairs[-1]))
        sc.info["pairs"] = pairs
    elif n == "chain":
        # 1-D: A = [0, 10], B = [3, 13], C = [6, 16] units: IoU(A,B) = IoU(B,C) = 7/13, IoU(A,C) = 4/16
        trip = []
        for b, l in enumerate((0, 1)):
            a0 = anchor(S, l, 3, 0)
            for i, lg in enumerate((4.0, 3.0, 2.0)):
                sc.put(b, a0 + 3 * i, 17, lg, (0, 0, 10, 1))
            trip.append((a0, a0 + 3, a0 + 6))
            sc.scatter(b, 10 + b, g, grid(-1, 1.5), exclude=list(trip[-1]))
        sc.info["trip"] = trip
    elif n == "equal_scores":
        # image 0: three pairs of level-0 neighbours (3/5 IoU) with one logit each
        pairs = []
        for i, y in enumerate((1, 8, 15)):
            a0 = anchor(S, 0, y, 4 + i)
            sc.put(0, a0, 40 + i, 1.0 + i, (0, 0, 4, 1)); sc.put(0, a0 + 1, 40 + i, 1.0 + i, (0, 0, 4, 1))
            pairs.append((a0, a0 + 1))
        sc.scatter(0, 9, g, grid(-1, 0.5), exclude=[a for p in pairs for a in p])
        # image 1: across levels - level 1 (2, 2) with (1, 1, 1, 1) is [24, 56]^2 px, level 0 (4, 4) with (2, 2, 2, 2) is [20, 52]^2 px: IoU 784 / 1264.
        # Equal logits: the level-0 anchor (lower index) stays. A second pair, where the level-1 box scores higher: it stays.
        lo0, hi1 = anchor(S, 0, 4, 4), anchor(S, 1, 2, 2)
        sc.put(1, lo0, 5, 2.0, (2, 2, 2, 2)); sc.put(1, hi1, 5, 2.0, (1, 1, 1, 1))
        lo0b, hi1b = anchor(S, 0, 12, 12), anchor(S, 1, 6, 6)
        sc.put(1, lo0b, 5, 1.0, (2, 2, 2, 2)); sc.put(1, hi1b, 5, 1.5, (1, 1, 1, 1))
        sc.scatter(1, 10, g, grid(-1, 0.5), exclude=[lo0, hi1, lo0b, hi1b])
        sc.info["pairs0"], sc.info["cross"] = pairs, ((lo0, hi1), (lo0b, hi1b))
    elif n == "argmax":
        # the anchor's class decides whether its neighbour (class 5, 3/5 IoU, lower score) goes
        cases = []
        for b in range(B):
            subs = [(((5, 2.0), (9, 2.0)), 1), (((5, 20.0), (9, 30.0)), 5), (((5, 30.0), (9, 20.0)), 9),
                    (((9, 2.0), (5, 2.0 - 1.0 / 64)), 13), (((5, 25.0), (60, 25.0)), 17)]
            for i, (two, y) in enumerate(subs):
                a0 = anchor(S, 0, y, 2 + 3 * b)
                for cl, lg in two:
                    sc.put(b, a0, cl, lg, (0, 0, 4, 1))
                sc.put(b, a0 + 1, 5, 1.0 - i / 8.0, (0, 0, 4, 1))
                cases.append((b, a0))
            sc.scatter(b, 8 + b, g, grid(-1, 0.5), exclude=[a for bb, a0 in cases if bb == b for a in (a0, a0 + 1)])
        sc.info["anchors"] = cases
    elif n == "blocks":
        _blocks(c, g, sc)
    elif n == "large_gather":
        for b in range(B):
            a0 = anchor(S, 1, 30, 10 + b)
            at = sc.scatter(b, 60 + 5 * b, g, grid(0.25, 6), exclude=[a0, a0 + 1])
            last = torch.arange(sc.A - 40, sc.A - 40 + 12)              # candidates among the last anchors too (index > 12288)
            sc.cls[b, last, torch.randint(0, NC, (12,), generator=g)] = _pick(grid(0.25, 3), 12, g, replace=False)
            used = set(at.tolist()) | set(last.tolist()) | {a0, a0 + 1}
            edge = [a for a in torch.randperm(sc.A, generator=g).tolist() if a not in used][:40]
            for a in edge:
                sc.put(b, a, int(torch.randint(0, NC, (1,), generator=g)), 0.0)
            sc.put(b, a0, 33, 5.5, (0, 0, 4, 1)); sc.put(b, a0 + 1, 33, 5.25, (0, 0, 4, 1))
            sc.info[f"edge{b}"], sc.info[f"pair{b}"] = edge, (a0, a0 + 1)
    elif n == "random_boxes":
        # classes 0..2 only and wide random boxes: neighbours overlap in one class, NMS has work
        for b in range(B):
            at = torch.randperm(sc.A, generator=g)[:200]
            sc.cls[b, at, torch.randint(0, 3, (200,), generator=g)] = _pick(above, 200, g, replace=False)
    else:
        raise KeyError(n)
    return sc


@functools.lru_cache(maxsize=None)
def nms_inputs(c):
    sc = _nms_scene(c)
    g = _gen("nmsbox", nms_id(c._replace(max_det=0)))
    box = torch.randn(B, sc.A, 64, generator=g) * 2.0 if c.name == "random_boxes" else onehot_box_logits(sc.dist)
    assert not torch.equal(sc.cls[0], sc.cls[1])
    return dict(cls=sc.cls, dist=sc.dist, box=box, cf=torch.randn(B, sc.A, 32, generator=g), info=sc.info)


@functools.lru_cache(maxsize=None)
def nms_reference(c, mode="fp32", iou=None):
    """-> per image (det [n,6] float32, anchor idx [n], coeff [n,32]); and the decoded boxes [B,A,4] and scores [B,A,nc] (float32).
    `iou`: another threshold than the case's (the host test moves it by one ulp)."""
    t = nms_inputs(c)
    boxes, scores = _decode(c.shape, t["box"], t["cls"], torch.float64 if mode == "fp64" else torch.float32)
    cxy, wh = (boxes[..., :2] + boxes[..., 2:]) / 2, boxes[..., 2:] - boxes[..., :2]        # dist2bbox(xywh=True), then xywh2xyxy
    boxes = torch.cat((cxy - wh / 2, cxy + wh / 2), -1).float()
    scores = scores.float()
    rows = [nms_postprocess(boxes[b], scores[b], t["cf"][b], c.conf, c.iou if iou is None else iou, max_det=c.max_det) for b in range(B)]
    return rows, boxes, scores


def sorted_candidates(c, b):
    """anchors of image b's candidates in the kernel's order (score descending, anchor ascending), from the float32 reference"""
    m = nms_reference(c)[2][b].max(1).values
    cand = torch.nonzero(m > c.conf).squeeze(1)
    return cand[torch.sort(m[cand], descending=True, stable=True).indices]


def split_levels(shape, flat):
    """[B, A, C] -> the three levels' [B, H, W, C]"""
    out, a0 = [], 0
    for h, w in levels(shape):
        out.append(flat[:, a0:a0 + h * w].reshape(flat.shape[0], h, w, flat.shape[-1]).contiguous())
        a0 += h * w
    return out


def tensors(inputs, shape):
    """a maker's flat tensors -> (class logits, box logits, coefficients), each a list of the three levels' [B, H, W, C] maps"""
    return split_levels(shape, inputs["cls"]), split_levels(shape, inputs["box"]), split_levels(shape, inputs["cf"])
