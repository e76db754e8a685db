"""Host side of yp_mask_contours_large: the workspace query and the argument checks, which return before anything is launched (no GPU)."""
import ctypes as C

import pytest

from yolo_puncture_amd.engine import YP_CONTOURS_ONLY_DECLINED, load_library


def test_workspace_query_is_monotone_and_zero_on_bad_sizes():
    lib = load_library()
    q = lib.yp_mask_contours_large_workspace
    base = q(1, 720, 1280)
    assert base > 0 and base % 16 == 0
    assert q(0, 720, 1280) == 0
    for n in (1, 2, 5, 33):
        assert q(n, 720, 1280) == n * base
    hs = [q(1, h, 1280) for h in (1, 2, 24, 384, 720, 1080, 2160, 4096)]
    assert all(a > 0 for a in hs) and hs == sorted(hs) and hs[-1] > hs[0]
    ws = [q(1, 720, w) for w in (1, 2, 31, 32, 33, 40, 640, 1280, 1920, 3840, 4096)]        # (columns come in words of 32)
    assert all(a > 0 for a in ws) and ws == sorted(ws) and ws[-1] > ws[0]
    # the bit image of a 3840x2160 frame with its zero border: (2160 + 2) rows of (120 + 3) words, three tables of that size among the rest
    assert q(1, 2160, 3840) >= 3 * 2162 * 123 * 4
    assert q(1, 2160, 3840) < 16 << 20
    for bad in ((-1, 720, 1280), (1, 0, 1280), (1, 720, 0), (1, -3, 5), (1, 4097, 1280), (1, 720, 4097)):
        assert q(*bad) == 0, bad


def test_argument_checks_come_before_any_launch():
    lib = load_library()
    f = lib.yp_mask_contours_large
    H, W, n, max_pts = 64, 80, 2, 256
    need = lib.yp_mask_contours_large_workspace(n, H, W)
    one = C.c_void_p(0x1000)                    # never dereferenced: every call below fails its checks (16-byte aligned, not null)
    ok = dict(masks=one, n=n, H=H, W=W, strategy=1, max_pts=max_pts, pts=one, count=one, parts=None, parts_cap=0, rect=None, H0=0, W0=0, flags=0,
              ws=one, ws_bytes=need, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = f(a["masks"], a["n"], a["H"], a["W"], a["strategy"], a["max_pts"], a["pts"], a["count"], a["parts"], a["parts_cap"], a["rect"],
               a["H0"], a["W0"], a["flags"], a["ws"], a["ws_bytes"], a["stream"])
        return rc, lib.yp_last_error().decode()

    for kw, word in ((dict(masks=None), "null buffer"), (dict(pts=None), "null buffer"), (dict(count=None), "null buffer"),
                     (dict(ws=None), "workspace"), (dict(ws=C.c_void_p(0x1004)), "aligned"),
                     (dict(ws_bytes=need - 1), "needed"), (dict(ws_bytes=0), "needed"),
                     (dict(strategy=2), "strategy"), (dict(strategy=-1), "strategy"),
                     (dict(H0=720, W0=0), "original size"), (dict(H0=0, W0=1280), "original size"), (dict(H0=-720, W0=1280), "original size"),
                     (dict(H0=720, W0=-1280), "original size"), (dict(H0=-1, W0=-1), "original size"),
                     (dict(H=4097), "4096"), (dict(W=5000), "4096"), (dict(n=-1), "bad sizes"), (dict(max_pts=1), "bad sizes"), (dict(H=0), "bad sizes"),
                     (dict(flags=2), "flags"), (dict(flags=YP_CONTOURS_ONLY_DECLINED | 4), "flags"),
                     (dict(parts=one, parts_cap=1), "parts_cap")):
        rc, msg = call(**kw)
        assert rc < 0, kw
        assert "yp_mask_contours_large" in msg and word in msg, (kw, msg)
    # nothing to do is not an error
    assert call(n=0, masks=None, pts=None, count=None, ws=None, ws_bytes=0)[0] == 0
