"""Crafted contour lists for the "all_merged" bridge (yp_mask_contours_merge, csrc/contour_merge.hip), fed as point buffers - no mask
needed. A case is a list of masks, a mask a list of contours (int32 [m,2], coordinates below 4096). tests/test_merge_host.py holds the
numpy emulation (tests/merge_ref.py) to them on the CPU, tests/test_gpu_contour_merge.py the kernels; the reference of both is
hostops.merge_contours."""
import numpy as np


def _c(*pts):
    return np.asarray(pts, np.int32).reshape(-1, 2)


def ring(cx, cy, r, m):
    """m points on a circle, rounded to pixels (duplicates and equal distances are welcome)"""
    t = 2 * np.pi * np.arange(m) / m
    return np.stack([np.rint(cx + r * np.cos(t)), np.rint(cy + r * np.sin(t))], 1).astype(np.int32)


def blobs(k, per_row=50, pitch=6):
    """k four-point contours (filled rectangles as the trace lists them: top-left, bottom-left, bottom-right, top-right), bottom-up"""
    out = []
    for i in reversed(range(k)):
        x, y = pitch * (i % per_row), pitch * (i // per_row)
        out.append(_c((x, y), (x, y + 3), (x + 2 + i % 2, y + 3), (x + 2 + i % 2, y)))
    return out


def pairs(k, per_row=64):
    """k two-point contours"""
    return [_c((4 * (i % per_row), 3 * (i // per_row)), (4 * (i % per_row) + 1 + i % 2, 3 * (i // per_row))) for i in range(k)]


def tie_pair(la, lb, ties, far_a=False):
    """two contours of la and lb points whose squared-distance table has its minimum, 9, exactly at the (ia, ib) of `ties`: a on the line
    y = 1000, the b of a tie 3 pixels below its a, every other b (and, with far_a, every a without a tie) far away"""
    a = np.stack([2 * np.arange(la), np.full(la, 1000)], 1).astype(np.int32)
    if far_a:
        keep = {ia for ia, _ in ties}
        for i in range(la):
            if i not in keep:
                a[i, 1] = 10 + i % 7
    b = np.stack([np.arange(lb) % 4000, np.full(lb, 3000)], 1).astype(np.int32)
    xs = {}
    for ia, ib in ties:
        assert xs.setdefault(ib, a[ia, 0]) == a[ia, 0], "one b point per tie column"
        b[ib] = (a[ia, 0], 1003)
    return [a, b]


def flipped_middle():
    """three contours, the middle one entered at index 4 and left at index 0: reversed, indices swapped"""
    return [_c((0, 0), (0, 5)), _c((20, 0), (15, 2), (12, 7), (8, 0), (5, 3)), _c((30, 0), (30, 4))]


def same_entry_exit():
    """three contours, the middle one entered and left at its point 0"""
    return [_c((8, 0), (0, 0)), _c((10, 2), (10, 50), (60, 50)), _c((12, 0), (20, 0))]


def four_contours():
    """two middle contours: their way-back pieces come in reverse contour order"""
    return [ring(20, 20, 8, 11), ring(45, 22, 9, 13), ring(70, 18, 7, 9), ring(95, 25, 10, 12)]


def cases(T, S):
    """name -> list of masks. T: tile size, S: scan block size, as the library exports them (engine.merge_sizes())."""
    out = {
        "two": [[ring(30, 30, 12, 17), ring(70, 34, 15, 23)]],
        "flipped_middle": [flipped_middle()],
        "same_entry_exit": [same_entry_exit()],
        "four_contours": [four_contours()],
        "one_point_contours": [[_c((5, 5)), _c((9, 9)), _c((1, 1))], [_c((3, 3)), ring(40, 40, 10, 9), _c((41, 41)), _c((0, 0))],
                               [_c((7, 7)), _c((7, 7))]],
        "n0": [[]],
        "n1": [[ring(50, 50, 20, 31)]],
        "n1_one_point": [[_c((3, 4))]],
        # equal minima in different a-tiles and b-tiles; the first in row-major order must win whichever tile is looked at first
        "ties_first_row_last_btile": [tie_pair(T + 1, 2 * T + 3, [(7, 2 * T + 1), (9, 2), (T, 0)])],
        "ties_same_row_two_btiles": [tie_pair(T + 1, 2 * T + 3, [(5, T + 7), (5, 3), (T, 1)])],
        "ties_second_atile": [tie_pair(T + 1, 2 * T + 3, [(T, 2 * T + 2), (T, 5)], far_a=True)],
        "ties_swapped_lengths": [tie_pair(2 * T + 3, T + 1, [(2 * T + 2, 0), (T + 1, T), (T + 1, 4)])],
        "ties_b_groups": [tie_pair(T + 1, 4 * T + 5, [(T, 3), (3, 4 * T + 4), (3, 4 * T + 2)])],
        "ties_middle": [[ring(500, 2500, 30, 40)] + tie_pair(T + 1, 2 * T + 3, [(T - 1, 2 * T + 2), (T, 0)]) + [ring(100, 3500, 30, 21)]],
        "corners": [[_c((0, 0), (0, 4095)), _c((4095, 4095), (4095, 0))], [_c((0, 0)), _c((4095, 4095))],
                    [_c((4095, 0), (4000, 0)), _c((0, 4095)), _c((4095, 4095), (0, 0))]],
        "blobs_700": [blobs(700)],
        "scan_block_minus": [pairs(S - 1)],
        "scan_block": [pairs(S)],
        "scan_block_plus": [pairs(S + 1)],
        "batch": [four_contours(), [], [ring(9, 9, 5, 8)], flipped_middle(), blobs(70), [], same_entry_exit(),
                  tie_pair(T + 1, 2 * T + 3, [(7, 2 * T + 1), (9, 2), (T, 0)])],
    }
    return out


def merged_len(mask):
    m = sum(len(c) for c in mask)
    return m if len(mask) <= 1 else m + 2 * len(mask) - 2


def pack(masks, max_pts=None, parts_cap=None):
    """the buffers a contour call with YP_CONTOURS_ALL would have filled: pts int32 [n,max_pts,2], count int32 [n], parts int32 [n,parts_cap];
    rows past a mask's data hold a pattern that is no valid data"""
    n = len(masks)
    if max_pts is None:
        max_pts = max([2] + [sum(len(c) for c in m) for m in masks])
    if parts_cap is None:
        parts_cap = 1 + max([1] + [len(m) for m in masks])
    pts = np.full((n, max_pts, 2), -77, np.int32)
    count = np.zeros(n, np.int32)
    parts = np.full((n, parts_cap), -5, np.int32)
    for i, m in enumerate(masks):
        parts[i, 0] = len(m)
        if m:
            allp = np.concatenate(m)
            count[i] = len(allp)
            pts[i, :len(allp)] = allp
            k = min(len(m), parts_cap - 1)                   # (as many lengths as fit, as the contour calls do)
            parts[i, 1:1 + k] = [len(c) for c in m[:k]]
    return pts, count, parts
