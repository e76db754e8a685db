"""Crafted inputs and the reference for the NMS head's options: predict(classes=, agnostic_nms=, max_nms=) (no GPU in here).

The contract is ultralytics' `non_max_suppression` with multi_label=False, per image:
  1. candidates: anchors whose best sigmoid score is > conf; the class is the first arg-max
  2. `classes` given: keep the candidates whose class is in the set
  3. more than max_nms left: keep the max_nms best - score descending, lower anchor first among equal scores (the project's tie rule)
  4. greedy NMS on box + cls * 7680, or on the boxes themselves when agnostic; `> iou` drops
  5. the first max_det survivors
`nms_postprocess_opts` follows these steps on the oracle's `nms_greedy`. The scenes are head_cases' (one-hot box logits, logits on the
1/64 grid): corners, areas and IoUs are exact, so anchors, classes and boxes compare with torch.equal and scores get SCORE_TOL.

`past_cap` is the `blocks` scene of head_cases at 1024x800: 16 800 anchors, all of them candidates at conf = 0, 280 blocks - one survivor
each. The anchors of the four `late` blocks fill the end of the sorted list, behind rank 16 384: the default max_nms gives 276 rows, the
whole list 280, and the 276 are a prefix of the 280.

tests/test_nms_options_host.py proves on the CPU that every case does what its name says and that each `variant` below (a deliberate
mistake in one step) changes the result of the case aimed at it; tests/test_gpu_nms_options.py holds the kernels to the reference."""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

import head_cases as H
from oracle.yolo_seg_oracle import MAX_WH, nms_greedy
from oracle.yolov10_oracle import Oracle

B, NC, NCAP, SCORE_TOL = H.B, H.NC, H.NCAP, H.SCORE_TOL
PAST_CAP_HW = (1024, 800)

# scene: a head_cases NmsCase name + shape, "none_and_many_gap", or "past_cap" / "past_cap_tail" (1024x800). classes: None or a tuple;
# max_nms: an int, or a callable(case) -> int for a cut taken from the scene's sorted order (resolve)
OptCase = namedtuple("OptCase", "id scene shape conf iou max_det classes agnostic max_nms")
DEFAULTS = dict(classes=None, agnostic=False, max_nms=NCAP)


def _levels_hw(hw):
    return [(hw[0] // s, hw[1] // s) for s in (8, 16, 32)]


def case_hw(c):
    return PAST_CAP_HW if c.shape == "P" else H.SHAPES[c.shape]


def case_levels(c):
    return _levels_hw(case_hw(c))


def n_anchors(c):
    return sum(h * w for h, w in case_levels(c))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _greedy_same_class_only(boxes, scores, cls, iou):
    """nms_greedy with the `other class: skip` shortcut of the kernel's sweep (used by a variant only)"""
    order = torch.sort(scores, descending=True, stable=True).indices
    b, k = boxes[order], cls[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = torch.zeros(b.shape[0], dtype=torch.bool)
    keep = []
    for i in range(b.shape[0]):
        if dead[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        inter = (torch.minimum(b[i, 2], r[:, 2]) - torch.maximum(b[i, 0], r[:, 0])).clamp(min=0) * \
                (torch.minimum(b[i, 3], r[:, 3]) - torch.maximum(b[i, 1], r[:, 1])).clamp(min=0)
        dead[i + 1:] |= (inter / (area[i] + area[i + 1:] - inter) > iou) & (k[i + 1:] == k[i])
    return order[torch.tensor(keep, dtype=torch.long)]


VARIANTS = ("cut_before_filter", "offset_under_agnostic", "class_shortcut_under_agnostic", "rounds_not_presuppressed", "cut_by_score_only")


def nms_postprocess_opts(boxes, scores, coeff, conf, iou, max_det, classes=None, agnostic=False, max_nms=NCAP, variant=None):
    """One image: boxes [A,4] xyxy px, scores [A,nc], coeff [A,32] -> det [n,6], anchor idx [n], coeff [n,32] (steps 1-5 above).
    `variant`: one of VARIANTS - the same with one step done wrong (the host test shows that a case notices)."""
    assert variant is None or variant in VARIANTS
    s, j = scores.max(1)                                                       # 1 (first maximum)
    cand = torch.nonzero(s > conf).squeeze(1)

    def by_class(cand):                                                        # 2
        if classes is None:
            return cand
        return cand[torch.isin(j[cand], torch.as_tensor(list(classes), dtype=j.dtype))]

    def best(cand):                                                            # 3 (cand ascends by anchor: the stable sort keeps the tie rule)
        src = cand.flip(0) if variant == "cut_by_score_only" else cand
        return src[torch.sort(s[src], descending=True, stable=True).indices][:max_nms]

    cand = by_class(best(cand)) if variant == "cut_before_filter" else best(by_class(cand))
    cand = cand[torch.sort(cand, stable=True).indices]                         # back to anchor order: nms_greedy's stable sort orders ties
    cand = cand[torch.sort(s[cand], descending=True, stable=True).indices]
    sc, cl, bx = s[cand], j[cand], boxes[cand]
    off = cl.to(bx.dtype) * MAX_WH if (not agnostic or variant == "offset_under_agnostic") else torch.zeros_like(sc)   # 4
    if variant == "class_shortcut_under_agnostic":
        keep = _greedy_same_class_only(bx, sc, cl, iou)
    elif variant == "rounds_not_presuppressed":
        keep = torch.cat([r0 + nms_greedy((bx + off[:, None])[r0:r0 + NCAP], sc[r0:r0 + NCAP], iou) for r0 in range(0, max(len(cand), 1), NCAP)])
    else:
        keep = nms_greedy(bx + off[:, None], sc, iou)
    keep = keep[:max_det]                                                      # 5
    det = torch.cat((bx[keep], sc[keep, None], cl[keep, None].to(bx.dtype)), 1)
    return det, cand[keep], (coeff[cand[keep]] if coeff is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _blocks_hw(hw, g, bg=-10.0):
    """head_cases._blocks for an input size that is not one of head_cases.SHAPES: every anchor a candidate, the anchors of an 8x8 block
    of a level decode to one box and carry the block's class, four `late` blocks fill the end of the sorted list."""
    lv = _levels_hw(hw)
    A = sum(h * w for h, w in lv)
    cls = torch.full((B, A, NC), bg)
    dist = torch.empty((B, A, 4), dtype=torch.long)
    block_of, nblk, a0 = torch.empty(A, dtype=torch.long), 0, 0
    for h, w in lv:
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        block_of[a0:a0 + h * w] = (nblk + (y // 8) * ((w + 7) // 8) + x // 8).flatten()
        dist[:, a0:a0 + h * w] = torch.stack((x % 8, y % 8, 7 - x % 8, 7 - y % 8), -1).reshape(-1, 4)
        nblk += ((h + 7) // 8) * ((w + 7) // 8)
        a0 += h * w
    info = {"block_of": block_of, "nblk": nblk, "order": []}
    G = -(-(A - 64) // 700)
    pos = torch.arange(A)
    lvl = torch.where(pos < 64, pos, 64 + (pos - 64) // G)
    logit = 6.0 - lvl.float() / 64.0
    assert float(logit.min()) > -6.0
    for b in range(B):
        bperm = torch.randperm(nblk, generator=g)
        is_late = torch.isin(block_of, bperm[:4])
        early = torch.nonzero(~is_late).squeeze(1)
        early = early[torch.randperm(early.numel(), generator=g)]
        tail = torch.nonzero(is_late).squeeze(1)
        tail = tail[torch.randperm(tail.numel(), generator=g)]
        order = torch.cat((early, tail))
        for s in range(64, A, G):                    # groups of G on one grid value: ordered by anchor inside a group
            order[s:s + G] = torch.sort(order[s:s + G]).values
        cls[b, order, block_of[order] % NC] = logit
        info["order"].append(order)
        info[f"late{b}"] = bperm[:4]
    return dict(cls=cls, dist=dist, info=info)


@functools.lru_cache(maxsize=None)
def _past_cap_scene(tail):
    g = H._gen("nms_options", "past_cap")
    sc = _blocks_hw(PAST_CAP_HW, g)
    info = sc["info"]
    if tail:
        # an anchor of an EARLY block, not the block's survivor, re-scored to the very end of the list (logit -6, below every other): its
        # block's survivor is kept in the first round of NCAP keys and must still suppress it in the second
        sc = dict(cls=sc["cls"].clone(), dist=sc["dist"], info=dict(info))
        moved = []
        for b in range(B):
            order, block_of = info["order"][b], info["block_of"]
            blk = block_of[order[100]]                                      # position 100's block: its survivor sits at or before 100
            later = [int(a) for a in order[200:NCAP] if block_of[a] == blk]
            a = later[0]
            sc["cls"][b, a, int(blk) % NC] = -6.0
            moved.append(a)
        sc["info"]["moved"] = moved
    A = sc["cls"].shape[1]
    sc["box"] = H.onehot_box_logits(sc["dist"])
    sc["cf"] = torch.randn(B, A, 32, generator=H._gen("nms_options", "past_cap", "cf"))
    return sc


GAP = (78, 79)


@functools.lru_cache(maxsize=None)
def _none_and_many_gap():
    """head_cases' none_and_many (no candidate in image 0, 350 in image 1, which carry every class) with the candidates of classes 78 / 79
    moved to classes 76 / 77: the set {78, 79} then empties image 1 while the default keeps 300 rows"""
    t = dict(H.nms_inputs(next(n for n in H.NMS_CASES if n.name == "none_and_many")))
    cls = t["cls"].clone()
    at = torch.nonzero(torch.isin(cls[1].argmax(1), torch.tensor(GAP)) & (cls[1].amax(1) > H.BG)).squeeze(1)
    assert at.numel() > 0
    cls[1, at] = torch.roll(cls[1, at], -2, 1)
    t["cls"] = cls
    return t


def _base_case(c):
    return next(n for n in H.NMS_CASES if n.name == c.scene and n.shape == c.shape)


def inputs(c):
    """-> dict(cls [B,A,nc], box [B,A,64], cf [B,A,32], info)"""
    if c.scene in ("past_cap", "past_cap_tail"):
        return _past_cap_scene(c.scene == "past_cap_tail")
    if c.scene == "none_and_many_gap":
        return _none_and_many_gap()
    return H.nms_inputs(_base_case(c))


@functools.lru_cache(maxsize=None)
def _decoded(scene, shape):
    c = OptCase("", scene, shape, 0, 0, 0, None, False, 0)
    t = inputs(c)
    o = Oracle.__new__(Oracle)
    o.dt = torch.float32
    boxes, scores = o.decode(t["box"].permute(0, 2, 1).contiguous(), t["cls"].permute(0, 2, 1).contiguous(), case_levels(c))
    cxy, wh = (boxes[..., :2] + boxes[..., 2:]) / 2, boxes[..., 2:] - boxes[..., :2]        # dist2bbox(xywh=True), then xywh2xyxy
    return torch.cat((cxy - wh / 2, cxy + wh / 2), -1).float(), scores.float()


def decoded(c):
    """boxes [B,A,4], scores [B,A,nc] (float32), as head_cases.nms_reference decodes them"""
    return _decoded(c.scene, c.shape)


def sorted_candidates(c, b, classes="case"):
    """anchors of image b's candidates after the class filter, in the kernel's order (score descending, anchor ascending)"""
    s, j = decoded(c)[1][b].max(1)
    cand = torch.nonzero(s > c.conf).squeeze(1)
    cl = c.classes if classes == "case" else classes
    if cl is not None:
        cand = cand[torch.isin(j[cand], torch.tensor(list(cl)))]
    return cand[torch.sort(s[cand], descending=True, stable=True).indices]


def max_nms_of(c):
    return c.max_nms(c) if callable(c.max_nms) else c.max_nms


@functools.lru_cache(maxsize=None)
def reference(c, variant=None, **over):
    """-> per image (det [n,6], anchor idx [n], coeff [n,32]). `over`: options other than the case's (the host test's controls)."""
    boxes, scores = decoded(c)
    t = inputs(c)
    o = dict(classes=c.classes, agnostic=c.agnostic, max_nms=max_nms_of(c))
    o.update(over)
    return [nms_postprocess_opts(boxes[b], scores[b], t["cf"][b], c.conf, c.iou, c.max_det, variant=variant, **o) for b in range(B)]


def late_survivor_ranks(c, b):
    """ranks (positions in the sorted list) of the four late blocks' survivors of image b: the first anchor of each block in that order"""
    info = inputs(c)["info"]
    order = sorted_candidates(c, b, classes=None)
    blk = info["block_of"][order]
    return sorted(int(torch.nonzero(blk == l)[0]) for l in info[f"late{b}"])


def _between_late_survivors(c):
    """a max_nms whose cut falls between two of image 0's late survivors AND inside a group of equal scores whose members the anchor
    rule decides: the first such cut for which choosing the group's HIGHER anchors instead would change the rows"""
    ranks = late_survivor_ranks(c, 0)
    for m in [r + 1 for r in ranks[:3]] + [r for r in ranks[1:]]:
        if not ranks[0] < m <= ranks[3]:
            continue
        probe = c._replace(max_nms=m)
        if not torch.equal(reference(probe)[0][1], reference(probe, "cut_by_score_only")[0][1]):
            return m
    raise AssertionError("no cut between the late survivors meets a tie group that matters")


EVEN = tuple(range(0, NC, 2))
_P = ("past_cap", "P", 0.0, 0.5, 300)
CASES = [
    # past the cap (head_nms_gather_opt_kernel + head_nms_large_opt_kernel: two rounds)
    OptCase("past_cap-max_nms30000", *_P, None, False, 30000),                 # 280 rows
    OptCase("past_cap-default", *_P, None, False, NCAP),                       # 276 rows (default options: the default kernels)
    OptCase("past_cap-cut_in_round2", *_P, None, False, _between_late_survivors),   # a partial second round, an exact cut inside it
    OptCase("past_cap_tail-max_nms30000", "past_cap_tail", "P", 0.0, 0.5, 300, None, False, 30000),   # round 2 holds a victim of round 1
    OptCase("past_cap-agnostic-even-30000", *_P, EVEN, True, 30000),           # all three options on the large path (one round: 8 4xx keys)
    # a cut below the candidate count
    OptCase("blocks-M-max_nms2000", "blocks", "M", 0.0, 0.5, 300, None, False, 2000),
    OptCase("blocks-L-max_nms5000", "blocks", "L", 0.0, 0.5, 300, None, False, 5000),
    # agnostic
    OptCase("same_box-agnostic", "same_box", "S", 0.25, 0.5, 300, None, True, NCAP),
    OptCase("argmax-agnostic", "argmax", "S", 0.25, 0.5, 300, None, True, NCAP),
    OptCase("equal_scores-agnostic", "equal_scores", "S", 0.25, 0.5, 300, None, True, NCAP),
    OptCase("blocks-M-agnostic", "blocks", "M", 0.0, 0.5, 300, None, True, NCAP),   # condition: boxes of two blocks meet with IoU <= 0.25
    # classes
    OptCase("random_boxes-classes1", "random_boxes", "S", 0.25, 0.7, 300, (1,), False, NCAP),
    OptCase("random_boxes-classes0_2", "random_boxes", "S", 0.25, 0.7, 300, (0, 2), False, NCAP),
    OptCase("none_and_many-empties_image1", "none_and_many_gap", "S", 0.25, 0.7, 300, GAP, False, NCAP),
    OptCase("random_boxes-class_without_candidate", "random_boxes", "S", 0.25, 0.7, 300, (5,), False, NCAP),
    OptCase("random_boxes-all_classes", "random_boxes", "S", 0.25, 0.7, 300, tuple(range(NC)), False, NCAP),
    # filter before cut
    OptCase("blocks-M-even-max_nms2000", "blocks", "M", 0.0, 0.5, 300, EVEN, False, 2000),
    # (at 2000 every block but the late ones has had its survivor whichever step comes first; at 200 the order of the two steps shows)
    OptCase("blocks-M-even-max_nms200", "blocks", "M", 0.0, 0.5, 300, EVEN, False, 200),
    # beyond 12288 anchors with a class set (head_cases' large_gather scene)
    OptCase("large_gather-XL-class33-agnostic", "large_gather", "XL", 0.5, 0.5, 300, (33,), True, NCAP),
]


def resolve(c):
    """the case with a max_nms that is taken from the scene's order worked out"""
    return c._replace(max_nms=max_nms_of(c))


def case_id(c):
    return c.id


def is_default(c):
    return c.classes is None and not c.agnostic and c.max_nms == NCAP


def split_levels(c, flat):
    """[B, A, C] -> the three levels' [B, H, W, C]"""
    out, a0 = [], 0
    for h, w in case_levels(c):
        out.append(flat[:, a0:a0 + h * w].reshape(flat.shape[0], h, w, flat.shape[-1]).contiguous())
        a0 += h * w
    return out
