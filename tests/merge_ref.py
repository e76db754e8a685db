"""numpy restatement of csrc/contour_merge.hip, step by step as the kernels work - not as hostops.merge_contours is written:

  closest pair   the |a| x |b| table cut into tiles of T x T points; inside a tile every a-row keeps its FIRST minimum while ib ascends;
                 rows and tiles are combined by the minimum of the packed key (d2 << 38 | ia << 19 | ib), in any order
  plan           per contour: start index, distance entry -> exit, flip, length of the way-out piece and of the way-back piece, the
                 exclusive scan of the first and the inclusive scan of the second
  emission       one slot per point of sum(n_i + 2): slot -> contour -> index in the rolled, closed, possibly reversed contour -> place

`mistake` plants one deliberate error (tests/test_merge_host.py shows that each breaks the case aimed at it):
  "last_min"           ties go to the last (ia, ib) instead of the first
  "no_flip"            a middle contour with entry > exit is not reversed
  "back_not_reversed"  the way-back pieces are laid in contour order
  "no_close"           the closing point of every contour is dropped
"""
import numpy as np

IDX_BITS = 19
MISTAKES = ("last_min", "no_flip", "back_not_reversed", "no_close")


def tiled_closest(a, b, T, mistake=None, order=None):
    """(ia, ib) of the closest pair as the tiles find it. `order`: a permutation seed for the order in which the tiles are combined."""
    a, b = np.asarray(a, np.int64).reshape(-1, 2), np.asarray(b, np.int64).reshape(-1, 2)
    tiles = [(a0, b0) for a0 in range(0, len(a), T) for b0 in range(0, len(b), T)]
    if order is not None:
        tiles = [tiles[i] for i in np.random.default_rng(order).permutation(len(tiles))]
    best = None
    for a0, b0 in tiles:
        ta, tb = a[a0:a0 + T], b[b0:b0 + T]
        d = (ta[:, None, 0] - tb[None, :, 0]) ** 2 + (ta[:, None, 1] - tb[None, :, 1]) ** 2
        assert d.max() < 1 << 26
        rows = np.arange(len(ta))
        if mistake == "last_min":                             # smallest distance, then the LARGEST indices
            ib = d.shape[1] - 1 - d[:, ::-1].argmin(1)
            dr = d[rows, ib]
            r = int(np.flatnonzero(dr == dr.min()).max())
            cand = (int(dr[r]), -(r + a0), -(int(ib[r]) + b0))
            if best is None or cand < best:
                best = cand
            continue
        ib = d.argmin(1)                                      # first minimum of each row
        k = int(((d[rows, ib] << (2 * IDX_BITS)) | ((rows + a0) << IDX_BITS) | (ib + b0)).min())
        best = k if best is None else min(best, k)
    if mistake == "last_min":
        return -best[1], -best[2]
    mask = (1 << IDX_BITS) - 1
    return (best >> IDX_BITS) & mask, best & mask


def merge_emulated(contours, T=256, mistake=None, order=None):
    """hostops.merge_contours(contours) the way the device computes it -> int32 [m,2]."""
    segs = [np.asarray(c, np.int32).reshape(-1, 2) for c in contours]
    n = len(segs)
    if n == 0:
        return np.zeros((0, 2), np.int32)
    if n == 1:
        return segs[0]
    lens = np.array([len(s) for s in segs], np.int64)
    assert lens.min() >= 1
    off = np.concatenate([[0], np.cumsum(lens)])
    pts = np.concatenate(segs)
    pair = [tiled_closest(segs[j], segs[j + 1], T, mistake, None if order is None else order + j) for j in range(n - 1)]
    # plan
    start, dist, flip, fwd, back = (np.zeros(n, np.int64) for _ in range(5))
    for i in range(n):
        e = pair[i - 1][1] if i > 0 else -1
        x = pair[i][0] if i < n - 1 else -1
        if i == 0 or i == n - 1:
            start[i], fwd[i] = (x if i == 0 else e), lens[i] + 1
        else:
            flip[i] = int(e > x) if mistake != "no_flip" else 0
            start[i], dist[i] = min(e, x), abs(e - x)
            fwd[i], back[i] = dist[i] + 1, lens[i] + 1 - dist[i]
    fwd_off = np.cumsum(fwd) - fwd
    back_inc = np.cumsum(back)
    total = int(fwd.sum() + back.sum())
    assert total == int(lens.sum()) + 2 * n - 2
    # emission: one slot per point of sum(L + 2)
    out = np.full((total, 2), -1, np.int32)
    written = np.zeros(total, bool)
    slot_off = off[:-1] + 2 * np.arange(n)
    for s in range(int(off[-1]) + 2 * n):
        i = int(np.searchsorted(slot_off, s, side="right")) - 1
        r, L = s - int(slot_off[i]), int(lens[i])
        if i == 0 or i == n - 1:
            if r > L:
                continue
            k, dst = r, fwd_off[i] + r
        elif r <= dist[i]:
            k, dst = r, fwd_off[i] + r
        else:
            k = r - 1
            if mistake == "back_not_reversed":
                dst = int(fwd.sum()) + (back_inc[i] - back[i]) + (k - dist[i])
            else:
                dst = total - back_inc[i] + (k - dist[i])
        if mistake == "no_close" and k == L:
            continue
        j = (int(start[i]) + k) % L
        src = L - 1 - j if flip[i] else j
        assert not written[dst]
        out[dst] = pts[off[i] + src]
        written[dst] = True
    if mistake == "no_close":
        return out[written]
    assert written.all()
    return out
