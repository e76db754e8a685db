"""Crafted inputs of the segmentation tail (csrc/mask.hip) and their references (no GPU in here).

tests/test_gpu_mask_crafted.py writes these prototypes over a real engine's `.proto.cv3` tensor (Engine.write_tensor; bf16 in a bf16 engine)
and calls yp_masks / yp_masks_frames / yp_masks_frames_input / yp_id_mask_resized on them; tests/test_mask_cases_host.py proves on the CPU
that every case does what its name says. Three families of inputs:

EXACT (sections "exact", "clip", "scalar GEMM").  Integer prototypes in [-4, 4] and integer coefficients in [-3, 3]: every 32-term dot product
  is an integer of magnitude <= 384, exact in float32 in any summation order, and in bf16 storage too (integers up to 4 are bf16 numbers).
  Output sizes whose prototype crop maps at a scale of 1/8, 1/4, 1/2, 1 or 2: every interpolation weight is a multiple of 1/16, every blend of
  integers with such weights is a multiple of 1/256 below 2^9 and exact. So the float32 and the float64 evaluation of the reference produce the SAME logits
  (`logit_map`, asserted bit for bit by the host test), the reference masks are `oracle.postprocess_oracle.process_mask_native` /
  `process_mask`, and the GPU assertion is torch.equal - no allowance. (The oracle functions cast the prototypes to float32 themselves, so the
  float64 evaluation is `logit_map`, which restates their three steps - product, torch's bilinear interpolate, crop_mask - in the dtype it is
  given; the host test ties it to the oracle functions.) Such maps hold exact zeros, so the strict `> 0` is met on values that really are 0.

RECT (section "paint").  Prototype channel 0 is +1 everywhere, every other channel 0: the coefficient row [+1, 0, ...] makes a mask equal to its
  box, [-1, 0, ...] an empty one, and with integer box edges the area is w*h exactly. References: `auto_segment_oracle` (ids, kept rows), with
  torch's own antialiased interpolate for the second resize.

RANDOM (section "random").  torch.randn prototypes and coefficients prove what integers cannot: that GEMM and blend are accurate on real values.
  The reference (`random_reference`) computes the product and the blend in float64 and the source coordinates and the four weights in float32,
  operation by operation as PyTorch's upsample_bilinear2d (align_corners=False) states them: scale = (float)ch / (float)oh,
  src = max(scale * (dst + 0.5) - 0.5, 0), l1 = src - floor(src), l0 = 1 - l1. Beside the logit it carries A = sum_k |c_k| |p_k| through the same
  blend: the magnitude every rounding error of the float32 evaluation scales with.

  Rule: a pixel may differ from `reference > 0` only if |reference| <= GAMMA * 2^-24 * A_blend(pixel); every other pixel must be equal.

  GAMMA, from the operation count (u = 2^-24, the unit roundoff of float32; nothing here is fitted to the kernel):
    * the dot product is a chain of 32 fused multiply-adds, one rounding each: |fl(sum) - sum| <= ((1+u)^32 - 1) * sum_k |c_k p_k| = 32 u A_tap
      to first order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), in any order of the chain;
    * the blend l_y0 * (l_x0 v00 + l_x1 v01) + l_y1 * (l_x0 v10 + l_x1 v11) is 4 + 2 products and 2 + 1 sums. Counted without
      following paths - the four products with a tap or a row in them and the three sums, each weighing at most u * (blend of the |taps|) -
      that is 7 u A_blend. (Followed tap by tap, a
      value passes only product, sum, product, sum = 4 roundings; a compiler that contracts products into fused multiply-adds removes
      some. 7 is the looser count and is kept: a bound derived twice takes the larger.)
    * the complementary weights l_x0 = 1 - l_x1, l_y0 = 1 - l_y1 are one rounding each: 2 u A_blend. (The reference forms them in float32 as
      well, so this term is slack, not need.)
    GAMMA = 32 + 7 + 2 = 41. Second-order terms ((1+u)^41 - 1 - 41u ~ 5e-14) and the float64 reference's own error (2^-53 * 41 * A) are
    eleven and nine orders below it.

  Cap: the rule may exempt at most 1e-4 of a case's in-box pixels. That is a condition on the INPUTS (how many reference logits lie that
  close to zero), checked from the reference alone by the host test; a seed that missed it would be changed, never the cap."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import postprocess_oracle as po

YP_MAX_MASKS = 480                                         # include/yolop.h: 480 rows of 32 floats = the 60 KiB LDS bound of launch_masks
AA_KMAX = 36                                               # csrc/mask.hip: taps of the antialiased second resize
RIGS = {"A": (2, 96, 160), "B": (1, 64, 96), "C": (4, 96, 160)}      # forward shapes; prototypes are a quarter of them: 24x40, 16x24, 24x40
DTYPES = ("fp32", "bf16")


def proto_shape(rig):
    B, H, W = RIGS[rig]
    return B, H // 4, W // 4


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def to_storage(x, dtype):
    """what a tensor of the engine holds after Engine.write_tensor: bf16 engines keep the prototypes as bf16 (round to nearest even)"""
    return x.bfloat16().float() if dtype == "bf16" else x.float().clone()


# ---------------------------------------------------------------------------------------------------------------------------------
# prototypes
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_protos(rig):
    """[B,Hp,Wp,32] integers in [-4, 4], every image different; channel 31 in [1, 4] (a coefficient row with that channel alone has one sign)"""
    B, Hp, Wp = proto_shape(rig)
    g = _gen("int_protos", rig)
    p = torch.randint(-4, 5, (B, Hp, Wp, 32), generator=g).float()
    p[..., 31] = torch.randint(1, 5, (B, Hp, Wp), generator=g).float()
    return p


@functools.lru_cache(maxsize=None)
def rect_protos(rig):
    B, Hp, Wp = proto_shape(rig)
    p = torch.zeros(B, Hp, Wp, 32)
    p[..., 0] = 1.0
    return p


@functools.lru_cache(maxsize=None)
def rand_protos(rig, seed=0):
    B, Hp, Wp = proto_shape(rig)
    return torch.randn(B, Hp, Wp, 32, generator=_gen("rand_protos", rig, seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------------------------------------------
def box_kinds(oh, ow):
    """name -> box (x1, y1, x2, y2) at an (oh, ow) output; the first ten are used in both retina modes"""
    qx, qy, hx, hy = max(ow // 4, 1), max(oh // 4, 1), ow // 2, oh // 2
    return {
        "whole": (0.0, 0.0, float(ow), float(oh)),
        "integer": (float(qx), float(qy), float(ow - qx), float(oh - qy)),
        "half": (qx + 0.5, qy + 0.5, ow - qx - 0.5, oh - qy - 0.5),       # x1 = q + 0.5: the first pixel set is q + 1; x2 = r - 0.5: the last is r - 1
        "to_edge": (float(hx), 0.0, float(ow), float(oh)),                  # x2 == ow, y2 == oh
        "beyond": (float(hx), float(hy), ow + 7.0, oh + 3.5),
        "negative": (-5.0, -2.5, float(hx), float(hy)),
        "empty": (float(qx), 0.0, float(qx), float(oh)),                    # x2 == x1: all zero
        "inverted": (float(hx), 1.0, float(hx - 3), float(oh - 1)),         # x2 < x1: all zero
        "one_pixel": (3.0, 2.0, 4.0, 3.0),
        "one_row": (0.0, float(hy), float(ow), float(hy + 1)),
    }


def box_kinds_input(ih, iw):
    """retina=0 only (boxes are scaled by 1/4 to prototype pixels and the TAPS are cropped): edges that fall between prototype pixels, and edges
    that are prototype pixels exactly (the `>=` / `<` pair at prototype resolution: pixel a is inside [a, b), pixel b is not)"""
    a, b, c, d = iw // 16, 3 * (iw // 16), ih // 16, 3 * (ih // 16)          # prototype pixels at a quarter and three quarters of the map
    return {
        "between_q": (4 * a - 1.0, 4 * c + 1.0, 4 * b + 1.0, 4 * d - 1.0),   # scaled: a - 0.25, c + 0.25, b + 0.25, d - 0.25
        "between_h": (4 * a + 2.0, 4 * c + 2.0, 4 * b + 2.0, 4 * d + 2.0),   # scaled: a + 0.5 ...
        "proto_exact": (4.0 * a, 4.0 * c, 4.0 * b, 4.0 * d),                 # scaled: a, c, b, d exactly
        "proto_one": (4.0 * a, 4.0 * c, 4.0 * a + 4.0, 4.0 * c + 4.0),       # one prototype pixel
    }


# ---------------------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------------------
# retina output sizes at 24x40 prototypes: (oh, ow) -> (crop top, bottom, left, right), 1/scale as (num, den) of out/crop, crop pixels % 16
RETINA_SIZES = {
    (96, 160): ((0, 24, 0, 40), (4, 1), 0),
    (92, 160): ((0, 23, 0, 40), (4, 1), 8),               # padding lanes of the matrix-core GEMM
    (96, 156): ((0, 24, 0, 39), (4, 1), 8),
    (88, 160): ((1, 23, 0, 40), (4, 1), 0),               # p.t != 0
    (96, 152): ((0, 24, 1, 39), (4, 1), 0),               # p.l != 0
    (46, 80): ((0, 23, 0, 40), (2, 1), 8),
    (192, 320): ((0, 24, 0, 40), (8, 1), 0),
    (184, 320): ((0, 23, 0, 40), (8, 1), 8),
    (12, 20): ((0, 24, 0, 40), (1, 2), 0),                # down-scaling
    (23, 40): ((0, 23, 0, 40), (1, 1), 8),                # plane of 920 bytes: no multiple of 16
    (24, 39): ((0, 24, 0, 39), (1, 1), 8),                # plane of 936 bytes
}
COUNT_SIZES = [(96, 160), (92, 160), (23, 40)]            # every mask count runs at these three
COUNTS = (0, 1, 15, 16, 17, 33)

ExactCase = namedtuple("ExactCase", "rig b hw retina n")


def _exact_cases():
    out = []
    for i, hw in enumerate(RETINA_SIZES):
        out.append(ExactCase("A", i % 2, hw, True, 17))
    for i, hw in enumerate(COUNT_SIZES):
        out += [ExactCase("A", (i + j) % 2, hw, True, n) for j, n in enumerate(COUNTS) if n != 17]
    out += [ExactCase("A", j % 2, (96, 160), False, n) for j, n in enumerate(COUNTS)]
    out += [ExactCase("B", 0, (64, 96), False, n) for n in (1, 17, 33)]
    return out


EXACT_CASES = _exact_cases()
BIG_CASE = ExactCase("A", 1, (96, 160), True, YP_MAX_MASKS)


def exact_id(c):
    return f"{c.rig}{c.b}-{c.hw[0]}x{c.hw[1]}-{'retina' if c.retina else 'input'}-n{c.n}"


def row_plan(c):
    """[(coefficient kind, box kind)] for the n rows of an exact case. Kinds: "dense" 32 random integers; "sparse" three non-zero entries (small
    logits: many exact zeros); "neg" the negation of the row before it, same box; "minus" -3 on channel 31 alone (every logit negative);
    "plus" +3 on channel 31 alone (every logit positive: the mask is the cropped region itself, so its edges are the box's)."""
    names = list(box_kinds(*c.hw))
    extra = [] if c.retina else list(box_kinds_input(*c.hw))
    if c.n == 0:
        return []
    if c.n == 1:
        return [("sparse", "whole")]
    plan = []
    for i in range(c.n):
        r = i % 17
        if r < 10:
            plan.append(("dense" if (i // 17 + r) % 2 == 0 else "plus", names[r]))
        elif r == 10:
            plan.append(("minus", "whole"))
        elif r == 11:
            plan.append(("sparse", "whole"))
        elif r == 12:
            plan.append(("neg", "whole"))
        elif not c.retina:
            plan.append(("plus" if i % 2 else "dense", extra[r - 13]))
        else:
            plan.append(("sparse" if r % 2 else "dense", names[(r + i // 17) % 6]))
    return plan


@functools.lru_cache(maxsize=None)
def exact_inputs(c):
    """-> coeff [n,32] float32 integers in [-3,3], boxes [n,4] float32"""
    g = _gen("exact", exact_id(c))
    kinds = dict(box_kinds(*c.hw))
    if not c.retina:
        kinds.update(box_kinds_input(*c.hw))
    coeff, boxes = torch.zeros(c.n, 32), torch.zeros(c.n, 4)
    for i, (ck, bk) in enumerate(row_plan(c)):
        if ck == "dense":
            coeff[i] = torch.randint(-3, 4, (32,), generator=g).float()
        elif ck == "sparse":
            ch = torch.randperm(31, generator=g)[:3]
            coeff[i, ch] = torch.tensor([1.0, -1.0, 2.0])[torch.randperm(3, generator=g)]
        elif ck == "neg":
            coeff[i] = -coeff[i - 1]
        elif ck == "minus":
            coeff[i, 31] = -3.0
        elif ck == "plus":
            coeff[i, 31] = 3.0
        boxes[i] = torch.tensor(kinds[bk])
    return coeff, boxes


def logit_map(proto_chw, coeff, boxes, hw, retina):
    """the float logits behind process_mask_native (retina) / process_mask: product, torch's bilinear interpolate, crop_mask - in the dtype of
    its arguments (all float32 or all float64); the masks are `logit_map(...) > 0`. Pixels outside the crop are 0."""
    c, mh, mw = proto_chw.shape
    m = (coeff @ proto_chw.reshape(c, -1)).view(-1, mh, mw)
    if retina:
        t, b, l, r = po.scale_masks_region(mh, mw, hw[0], hw[1])
        m = F.interpolate(m[None, :, t:b, l:r], size=tuple(hw), mode="bilinear", align_corners=False)[0]
        return po.crop_mask(m, boxes)
    ds = boxes.clone()
    ds[:, 0] *= mw / hw[1]
    ds[:, 2] *= mw / hw[1]
    ds[:, 1] *= mh / hw[0]
    ds[:, 3] *= mh / hw[0]
    m = po.crop_mask(m, ds)
    return F.interpolate(m[None], size=tuple(hw), mode="bilinear", align_corners=False)[0]


def oracle_masks(proto_hwc, coeff, boxes, hw, retina):
    """the reference of every exact case: the oracle's own function on float32 tensors -> uint8 [n,oh,ow]"""
    if coeff.shape[0] == 0:
        return torch.zeros((0,) + tuple(hw), dtype=torch.uint8)
    fn = po.process_mask_native if retina else po.process_mask
    return fn(proto_hwc.permute(2, 0, 1).contiguous(), coeff, boxes, tuple(hw)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def exact_reference(c):
    coeff, boxes = exact_inputs(c)
    return oracle_masks(int_protos(c.rig)[c.b], coeff, boxes, c.hw, c.retina)


def inside_box(boxes, hw):
    """[n,oh,ow] bool: (x >= x1) & (x < x2) & (y >= y1) & (y < y2) at output pixels"""
    x = torch.arange(hw[1], dtype=boxes.dtype)[None, None, :]
    y = torch.arange(hw[0], dtype=boxes.dtype)[None, :, None]
    b = boxes[:, :, None, None]
    return (x >= b[:, 0]) & (x < b[:, 2]) & (y >= b[:, 1]) & (y < b[:, 3])


# ---------------------------------------------------------------------------------------------------------------------------------
# clip forms: one mask per selected frame, row 0 of each frame's coefficient block
# ---------------------------------------------------------------------------------------------------------------------------------
CLIP_RIG = "C"
CLIP_MAX_DET = 300
CLIP_FRAMES = {1: [2], 3: [0, 0, 3], 5: [3, 0, 0, 2, 3]}            # repeats; frame 1 is never taken (a gap)
CLIP_OFFSETS = (1, 7, 15)                                          # byte offsets of the output view in a sentinel-filled buffer
CLIP_SIZES = [((96, 160), True), ((92, 160), True), ((23, 40), True), ((24, 39), True), ((96, 160), False)]
CLIP_BOXES = ("half", "whole", "integer", "negative", "to_edge")   # mask j takes kind j: neighbours in the byte stream have different boxes


@functools.lru_cache(maxsize=None)
def clip_inputs(hw, retina, k):
    """-> frame_idx list, coeff [B,max_det,32] (row 0 crafted, the rest a sentinel no mask may depend on), boxes [k,4]"""
    B = RIGS[CLIP_RIG][0]
    g = _gen("clip", hw, retina, k)
    coeff = torch.full((B, CLIP_MAX_DET, 32), 3.0)
    coeff[:, 0] = torch.randint(-3, 4, (B, 32), generator=g).float()
    kinds = box_kinds(*hw)
    boxes = torch.tensor([kinds[CLIP_BOXES[j]] for j in range(k)], dtype=torch.float32)
    return list(CLIP_FRAMES[k]), coeff, boxes


@functools.lru_cache(maxsize=None)
def clip_reference(hw, retina, k):
    fidx, coeff, boxes = clip_inputs(hw, retina, k)
    P = int_protos(CLIP_RIG)
    return torch.cat([oracle_masks(P[f], coeff[f, :1], boxes[j:j + 1], hw, retina) for j, f in enumerate(fidx)])


# ---------------------------------------------------------------------------------------------------------------------------------
# area, suppression and paint on rectangular masks
# ---------------------------------------------------------------------------------------------------------------------------------
PaintCase = namedtuple("PaintCase", "name rows suppress min_area kept")       # rows: (sign, (x1,y1,x2,y2)); kept: the expected `kept` vector
PAINT_HW = (96, 160)
_A100, _A99 = (10, 10, 20, 20), (30, 10, 41, 19)                               # 10 x 10 = 100 and 11 x 9 = 99 pixels
PAINT_CASES = [
    PaintCase("area_on_and_below_threshold", [(1, _A100), (1, _A99)], 1, 100, [1, 0]),          # `<`: area == min_area is kept
    PaintCase("same_rows_unsuppressed", [(1, _A100), (1, _A99)], 0, 100, [1, 2]),
    PaintCase("overlap_later_wins_suppressed_between", [(1, (10, 10, 60, 50)), (1, (35, 25, 46, 34)), (1, (40, 30, 90, 70))], 1, 100, [1, 0, 2]),
    PaintCase("empty_mask_takes_an_id", [(1, _A100), (-1, (0, 0, 160, 96)), (1, (15, 15, 40, 30))], 0, 100, [1, 2, 3]),
    PaintCase("all_suppressed", [(1, _A99), (1, (50, 50, 59, 61)), (-1, (0, 0, 160, 96))], 1, 100, [0, 0, 0]),
    PaintCase("none", [], 1, 100, []),
]

ResizeCase = namedtuple("ResizeCase", "name mask_hw out_hw rows min_area")
RESIZE_CASES = [
    # 2:3 up: boxes with odd edges put hundreds of pixels at exactly 0.5 along them; areas 2.25 x (1200, 400, 900)
    ResizeCase("up_2_3", (96, 160), (144, 240), [(1, (21, 21, 61, 51)), (1, (70, 10, 90, 30)), (-1, (0, 0, 160, 96)), (1, (41, 41, 71, 71))], 1500),
    # 3:2 down: areas (1200, 400, 900) / 2.25
    ResizeCase("down_3_2", (96, 162), (64, 108), [(1, (21, 21, 61, 51)), (1, (72, 9, 92, 29)), (1, (42, 42, 72, 72))], 300),
    # 16:1 down, the widest filter the kernel admits: 33 of AA_KMAX = 36 taps; areas (3072, 256, 4096) / 256
    ResizeCase("down_16_1", (96, 160), (6, 10), [(1, (16, 16, 80, 64)), (1, (96, 32, 112, 48)), (1, (64, 32, 128, 96))], 5),
]


def rect_inputs(rows):
    n = len(rows)
    coeff, boxes = torch.zeros(n, 32), torch.zeros(n, 4)
    for i, (sign, box) in enumerate(rows):
        coeff[i, 0] = float(sign)
        boxes[i] = torch.tensor(box, dtype=torch.float32)
    return coeff, boxes


def rect_masks(rows, hw):
    """what the rows must give, from their definition alone: the box for sign +1 (integer edges, clipped to the image), nothing for -1"""
    m = torch.zeros((len(rows),) + tuple(hw), dtype=torch.uint8)
    for i, (sign, (x1, y1, x2, y2)) in enumerate(rows):
        if sign > 0:
            m[i, max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = 1
    return m


def paint_reference(masks, out_hw, suppress, min_area):
    """auto_segment_oracle -> (ids int64 [out_hw], kept int32 [n]: the id of a kept row, 0 for a suppressed one)"""
    n = masks.shape[0]
    ids, info = po.auto_segment_oracle(masks.float() if n else None, torch.arange(n, dtype=torch.float32), torch.zeros(n), tuple(out_hw), bool(suppress), min_area)
    kept = torch.zeros(n, dtype=torch.int32)
    for cur, row, _ in info:
        kept[int(row)] = cur
    return ids, kept


def resized_areas(masks, out_hw):
    """the float areas the oracle tests against min_area: sum of torch's antialiased resize of each {0,1} mask"""
    return [float(F.interpolate(m[None, None].float(), size=tuple(out_hw), mode="bilinear", align_corners=False, antialias=True).sum()) for m in masks]


# ---------------------------------------------------------------------------------------------------------------------------------
# random data, per-pixel rule
# ---------------------------------------------------------------------------------------------------------------------------------
GAMMA = 32 + 7 + 2                                         # module docstring
U32 = 2.0 ** -24
EXEMPT_CAP = 1e-4

RandomCase = namedtuple("RandomCase", "rig b hw retina n seed")
RANDOM_CASES = [RandomCase("A", (i + j) % 2, hw, True, n, 0) for i, hw in enumerate([(90, 160), (200, 333), (90, 161)]) for j, n in enumerate((1, 7, 40))] + \
               [RandomCase("A", j % 2, (96, 160), False, n, 0) for j, n in enumerate((1, 7, 40))]


def random_id(c):
    return f"{c.rig}{c.b}-{c.hw[0]}x{c.hw[1]}-{'retina' if c.retina else 'input'}-n{c.n}"


def random_boxes(n, hw, g):
    """tests/test_gpu_facade.py's recipe: x1, y1 in the first half, x2, y2 in the second; row 0 the whole image"""
    oh, ow = hw
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([ow / 2, oh / 2, ow / 2, oh / 2]) + torch.tensor([0, 0, ow / 2, oh / 2])
    if n:
        boxes[0] = torch.tensor([0., 0., float(ow), float(oh)])
    return boxes


@functools.lru_cache(maxsize=None)
def random_inputs(c):
    g = _gen("random", random_id(c), c.seed)
    return torch.randn(c.n, 32, generator=g), random_boxes(c.n, c.hw, g)


def _axis(n_dst, n_src):
    """upsample_bilinear2d, align_corners=False, one axis, in float32: -> i0, i1 (int64), l0, l1 (float32 values as float64)"""
    f32 = np.float32
    scale = f32(n_src) / f32(n_dst)
    src = scale * (np.arange(n_dst, dtype=np.float32) + f32(0.5)) - f32(0.5)
    src = np.maximum(src, f32(0.0))
    assert src.dtype == np.float32
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_src - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f32(1.0) - l1
    assert l0.dtype == np.float32
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def random_reference(proto_hwc, coeff, boxes, hw, retina):
    """-> ref float64 [n,oh,ow] (the logit; -1 where the output-space crop excludes the pixel), A float64 [n,oh,ow] (blend of sum |c||p|; 0 where no
    tap contributes: such a pixel has no allowance), inbox bool [n,oh,ow] (pixels that count for the cap)"""
    P = proto_hwc.double().numpy()
    C = coeff.double().numpy()
    bx = boxes.float().numpy()
    mh, mw = P.shape[:2]
    oh, ow = hw
    n = C.shape[0]
    if retina:
        t, b, l, r = po.scale_masks_region(mh, mw, oh, ow)
    else:
        t, b, l, r = 0, mh, 0, mw
    P = P[t:b, l:r]
    M = np.einsum("nk,yxk->nyx", C, P)
    A = np.einsum("nk,yxk->nyx", np.abs(C), np.abs(P))
    ch, cw = P.shape[:2]
    if not retina:                                          # taps outside the box scaled to prototype pixels are zeroed before the blend
        f32 = np.float32
        bsx, bsy = f32(mw) / f32(ow), f32(mh) / f32(oh)
        xs, ys = np.arange(cw, dtype=np.float32)[None, None, :], np.arange(ch, dtype=np.float32)[None, :, None]
        x1, y1, x2, y2 = [(bx[:, i] * (bsx if i % 2 == 0 else bsy))[:, None, None] for i in range(4)]
        assert x1.dtype == np.float32
        tap_in = (xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)
        M = M * tap_in
        A = A * tap_in
    y0, y1i, ly0, ly1 = _axis(oh, ch)
    x0, x1i, lx0, lx1 = _axis(ow, cw)

    def blend(V):
        r0 = lx0 * V[:, y0][:, :, x0] + lx1 * V[:, y0][:, :, x1i]
        r1 = lx0 * V[:, y1i][:, :, x0] + lx1 * V[:, y1i][:, :, x1i]
        return ly0[None, :, None] * r0 + ly1[None, :, None] * r1
    ref, Ab = blend(M), blend(A)
    if retina:
        inbox = inside_box(boxes.float(), hw).numpy() if n else np.zeros((0, oh, ow), dtype=bool)
        ref = np.where(inbox, ref, -1.0)
        Ab = np.where(inbox, Ab, 0.0)
    else:
        inbox = Ab > 0
    return torch.from_numpy(ref), torch.from_numpy(Ab), torch.from_numpy(inbox)


def rule_stats(ref, A):
    """-> (exempt bool map, in-box pixel count is the caller's)"""
    return (ref.abs() <= GAMMA * U32 * A) & (A > 0)


def check_rule(what, got, ref, A):
    """the per-pixel rule on masks `got` (uint8 / bool [n,oh,ow]); prints the number of exempt pixels and the largest |reference| among the
    pixels that differ; -> (exempt pixels, differing pixels)"""
    want = ref > 0
    differ = got.bool() != want
    exempt = rule_stats(ref, A)
    bad = differ & ~exempt
    worst = float(ref[differ].abs().max()) if bool(differ.any()) else 0.0
    print(f"[mask rule] {what}: {int(exempt.sum())} exempt pixels of {int((A > 0).sum())}, {int(differ.sum())} differ, largest |reference| among them {worst:.3e}")
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ outside the allowance, first at {i}: reference {float(ref[tuple(i)]):.6e}, "
                             f"allowance {GAMMA * U32 * float(A[tuple(i)]):.3e}")
    return int(exempt.sum()), int(differ.sum())


@functools.lru_cache(maxsize=None)
def random_case_reference(c, dtype):
    coeff, boxes = random_inputs(c)
    return random_reference(to_storage(rand_protos(c.rig, c.seed), dtype)[c.b], coeff, boxes, c.hw, c.retina)


# ---------------------------------------------------------------------------------------------------------------------------------
# scalar GEMM (YOLOP_MASK_VALU=1, a child process): a subset of the exact cases and one random case
# ---------------------------------------------------------------------------------------------------------------------------------
VALU_EXACT = [c for c in EXACT_CASES if c.n in (1, 17) and ((c.retina and c.hw in ((96, 160), (92, 160))) or (not c.retina and c.rig == "A"))]
VALU_RANDOM = RandomCase("A", 0, (200, 333), True, 7, 0)
assert VALU_RANDOM in RANDOM_CASES and len(VALU_EXACT) == 6
