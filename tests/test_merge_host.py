"""The "all_merged" bridge without a GPU: the numpy emulation of the device algorithm (tests/merge_ref.py: tiled argmin with a packed key,
emission plan, one slot per point) against hostops.merge_contours on the crafted lists of tests/merge_cases.py and on 1000 seeded random
lists; four deliberate mistakes that each break the case aimed at them; the row-blocked distance table of hostops.merge_contours against
the one-piece table it replaced; the host arithmetic of the C entry points (tile-list size, workspace, refusals)."""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
from merge_ref import MISTAKES, merge_emulated, tiled_closest
from yolo_puncture_amd import hostops
from yolo_puncture_amd.engine import MERGE_MAX_PTS, load_library, merge_sizes, merge_tiles

T, S = merge_sizes()
CASES = mc.cases(T, S)


def merge_unblocked(contours):
    """hostops.merge_contours as it was before the distance table was cut into row blocks: one |a| x |b| x 2 int64 array per pair"""
    segs = [np.asarray(c).reshape(-1, 2) for c in contours]
    n = len(segs)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if n == 1:
        return segs[0]
    near = [[] for _ in range(n)]
    for i in range(1, n):
        a, b = segs[i - 1].astype(np.int64), segs[i].astype(np.int64)
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        j = int(d.argmin())
        near[i - 1].append(j // d.shape[1])
        near[i].append(j % d.shape[1])
    out, back = [], []
    for i in range(n):
        idx = near[i]
        seg = segs[i]
        if len(idx) == 2 and idx[0] > idx[1]:
            idx, seg = idx[::-1], seg[::-1]
        seg = np.roll(seg, -idx[0], axis=0)
        seg = np.concatenate([seg, seg[:1]])
        if i == 0 or i == n - 1:
            out.append(seg)
        else:
            out.append(seg[:idx[1] - idx[0] + 1])
            back.append(seg[abs(near[i][1] - near[i][0]):])
    return np.concatenate(out + back[::-1], axis=0)


def random_lists(count=1000, seed=5):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(rng.integers(0, 7))
        span = int(rng.choice([4, 12, 60, 4096]))           # small spans: many equal distances
        yield [rng.integers(0, span, size=(int(rng.integers(1, 41)), 2)).astype(np.int32) for _ in range(n)]


def test_exported_sizes():
    assert T >= 64 and T & (T - 1) == 0 and S >= 64
    assert MERGE_MAX_PTS == 1 << 19


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_equals_merge_contours_on_the_cases(name):
    for k, mask in enumerate(CASES[name]):
        want = hostops.merge_contours(mask)
        got = merge_emulated(mask, T)
        assert got.shape == want.shape and np.array_equal(got, want), (name, k)
        assert len(want) == mc.merged_len(mask)
        if name.startswith("ties"):                          # ... and in whatever order the tiles are combined
            assert np.array_equal(merge_emulated(mask, T, order=3), want)


def test_the_cases_are_what_they_claim():
    fl = mc.flipped_middle()
    assert hostops._closest_pair(fl[0], fl[1])[1] > hostops._closest_pair(fl[1], fl[2])[0]
    eq = mc.same_entry_exit()
    assert hostops._closest_pair(eq[0], eq[1])[1] == hostops._closest_pair(eq[1], eq[2])[0]
    a, b = CASES["ties_first_row_last_btile"][0]
    assert (len(a), len(b)) == (T + 1, 2 * T + 3)
    d = ((a[:, None, :].astype(np.int64) - b[None, :, :]) ** 2).sum(-1)
    at = np.argwhere(d == d.min())
    assert [tuple(r) for r in at] == [(7, 2 * T + 1), (9, 2), (T, 0)]          # three equal minima: a-tiles 0, 0, 1; b-tiles 2, 0, 0
    assert hostops._closest_pair(a, b) == (7, 2 * T + 1) == tiled_closest(a, b, T) == tiled_closest(a, b, T, order=1)
    a, b = CASES["ties_second_atile"][0]
    assert hostops._closest_pair(a, b) == (T, 5)
    a, b = CASES["ties_b_groups"][0]
    assert hostops._closest_pair(a, b) == (3, 4 * T + 2)
    assert len(CASES["blobs_700"][0]) == 700 and all(len(c) == 4 for c in CASES["blobs_700"][0])
    assert [len(CASES[k][0]) for k in ("scan_block_minus", "scan_block", "scan_block_plus")] == [S - 1, S, S + 1]
    assert max(int(np.concatenate(m).max()) for m in CASES["corners"]) == 4095 and min(int(np.concatenate(m).min()) for m in CASES["corners"]) == 0
    assert {0, 1} < {len(m) for m in CASES["batch"]} and len({len(m) for m in CASES["batch"]}) >= 4


def test_emulation_equals_merge_contours_on_random_lists():
    multi = 0
    for k, mask in enumerate(random_lists()):
        want = hostops.merge_contours(mask)
        got = merge_emulated(mask, 8, order=k)               # 8-point tiles: up to 5 x 5 tiles per pair
        assert got.shape == want.shape and np.array_equal(got, want), k
        multi += len(mask) > 2
    assert multi > 400


@pytest.mark.parametrize("mistake,name", [("last_min", "ties_first_row_last_btile"), ("no_flip", "flipped_middle"),
                                          ("back_not_reversed", "four_contours"), ("no_close", "two")])
def test_each_mistake_breaks_its_case(mistake, name):
    assert mistake in MISTAKES
    mask = CASES[name][0]
    want = hostops.merge_contours(mask)
    assert np.array_equal(merge_emulated(mask, T), want)
    bad = merge_emulated(mask, T, mistake=mistake)
    assert bad.shape != want.shape or not np.array_equal(bad, want), f"{mistake} goes unnoticed on {name}"


def test_blocked_table_equals_unblocked(monkeypatch):
    lists = [m for name in sorted(CASES) for m in CASES[name]] + list(random_lists(200, seed=9))
    for cells in (hostops._MERGE_BLOCK_CELLS, 64, 1):       # the shipped block, blocks of a few rows, one row per block
        monkeypatch.setattr(hostops, "_MERGE_BLOCK_CELLS", cells)
        for k, mask in enumerate(lists):
            if cells == 1 and sum(len(c) for c in mask) > 600:
                continue
            got, want = hostops.merge_contours(mask), merge_unblocked(mask)
            assert got.shape == want.shape and np.array_equal(got, want), (cells, k)


def test_blocked_table_keeps_the_first_minimum_across_blocks(monkeypatch):
    a, b = CASES["ties_first_row_last_btile"][0]
    monkeypatch.setattr(hostops, "_MERGE_BLOCK_CELLS", 8 * len(b))         # 8 rows a block: the ties sit in blocks 0, 1 and T // 8
    assert hostops._closest_pair(a, b) == (7, 2 * T + 1)
    a, b = CASES["ties_swapped_lengths"][0]
    assert hostops._closest_pair(a, b) == (T + 1, 4)


# ---- host arithmetic of the C entry points (nothing is launched) ------------------------------------------------------------------------
def test_tile_list_sizes():
    G = 4 * T                                                # b-points of a work tile: four LDS tiles
    assert merge_tiles([]) == 0 and merge_tiles([5]) == 0
    assert merge_tiles([1, 1]) == 1
    assert merge_tiles([T, G]) == 1 and merge_tiles([T + 1, G]) == 2 and merge_tiles([T, G + 1]) == 2 and merge_tiles([T + 1, G + 1]) == 4
    assert merge_tiles([6000, 6000, 3000]) == -(-6000 // T) * -(-6000 // G) + -(-6000 // T) * -(-3000 // G)
    assert merge_tiles([4] * 3000) == 2999
    assert merge_tiles([MERGE_MAX_PTS, MERGE_MAX_PTS]) == (MERGE_MAX_PTS // T) * (MERGE_MAX_PTS // G)
    assert merge_tiles([3, 0, 3]) == 0 and merge_tiles([3, -1]) == 0 and merge_tiles([MERGE_MAX_PTS + 1, 2]) == 0


def test_workspace_query():
    q = load_library().yp_mask_contours_merge_workspace
    assert q(0, 65) == 0
    per = q(1, 65) - 16                                      # one mask's slice; in front of the slices: n + 1 64-bit tile offsets, padded to 16 bytes
    assert per > 0 and per % 16 == 0
    for n in (1, 2, 7, 480):
        assert q(n, 65) == (2 * (n + 1) + 3) // 4 * 16 + n * per
    caps = [q(3, c) for c in (2, 3, 65, 66, 1025, 65537)]
    assert caps == sorted(caps) and caps[-1] > caps[0]
    assert q(1, 65537) >= 65536 * 8 * 4 and q(1, 65537) < 4 << 20          # offsets, tile offsets, a 64-bit key and a 4-word plan per contour
    for bad in ((-1, 65), (65536, 65), (1, 1), (1, 0), (1, 65538)):
        assert q(*bad) == 0, bad


def test_refusals_come_before_any_launch():
    lib = load_library()
    f = lib.yp_mask_contours_merge
    n, max_pts, parts_cap, out_cap = 2, 256, 9, 300
    need = lib.yp_mask_contours_merge_workspace(n, parts_cap)
    one = C.c_void_p(0x1000)                                 # never dereferenced: every call below fails its checks
    ok = dict(pts=one, count=one, parts=one, n=n, max_pts=max_pts, parts_cap=parts_cap, out=one, out_count=one, out_cap=out_cap, ws=one,
              ws_bytes=need, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = f(a["pts"], a["count"], a["parts"], a["n"], a["max_pts"], a["parts_cap"], a["out"], a["out_count"], a["out_cap"], a["ws"],
               a["ws_bytes"], a["stream"])
        return rc, lib.yp_last_error().decode()

    for kw, word in ((dict(n=-1), "bad sizes"), (dict(n=65536), "bad sizes"), (dict(max_pts=1), "bad sizes"),
                     (dict(max_pts=MERGE_MAX_PTS + 1), "bad sizes"), (dict(out_cap=0), "bad sizes"), (dict(parts_cap=1), "parts_cap"),
                     (dict(parts_cap=65538), "parts_cap"), (dict(pts=None), "null"), (dict(count=None), "null"), (dict(parts=None), "null"),
                     (dict(out=None), "null"), (dict(out_count=None), "null"), (dict(pts=C.c_void_p(0x1004)), "aligned"),
                     (dict(out=C.c_void_p(0x1004)), "aligned"), (dict(ws=None), "workspace"), (dict(ws=C.c_void_p(0x1008)), "workspace"),
                     (dict(ws_bytes=need - 1), "needed")):
        rc, msg = call(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)
    assert call(n=0, pts=None, count=None, parts=None, out=None, out_count=None, ws=None, ws_bytes=0)[0] == 0      # nothing to do
