#!/usr/bin/env python3
"""Latency of the large contour path (yp_mask_contours_large, csrc/contour_large.hip) against what it replaces. One process, masks and
frames resident in HBM, every leg warmed, then timed repeats with a device synchronisation each (best and median in ms):
  per mask, for four masks the LDS kernel declines (4K needle, 4K blobs, 1080p blobs, 4K dots around a ring - the lists of
  tests/test_gpu_contour_large.py):
    (a) the host fallback: mask_contours_device -> None -> device-to-host copy + hostops.mask_polygon + get_coord_min_rect_len
    (b) mask_contours_large_device
  predict_clip per frame on an 8-frame 3840x2160 clip (the 720p frames of the clip tools, 3x nearest), both mask modes, with the large
  path (this tree) and with it switched off (every decline ends on the host, as before it existed);
  `--regress`: predict_clip on a 64-frame 720p clip of the same layout, both modes, the large path on and off interleaved over several
  rounds. With the 11n-seg synthetic (the default) the masks are noise with more than 64 outer borders, which the LDS pass declines in
  strategy "all": this is the many-border case at 720p. Where nothing is declined the large path is not launched at all; that case is
  measured with tools/yolo_clip_latency.py / tools/yolo_clip_input_latency.py (v8n-seg layout) on the parent's tree and this one in turn,
  and those figures are added to the JSON by hand (`clip_720p_v8_parent_vs_change_ms_per_frame_bs32_dev`).
Writes profiles/contour_large_latency.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_puncture_amd import hostops, predictor  # noqa: E402
from yolo_puncture_amd.engine import mask_contours_device, mask_contours_large_device  # noqa: E402
from yolo_puncture_amd.predictor import YOLO  # noqa: E402
from yolo_puncture_amd.weights import save_as_ultralytics_pt  # noqa: E402


def _blobs(h, w, seed, thr=0.55, cells=9):
    g = torch.Generator().manual_seed(seed)
    f = torch.rand(1, 1, cells, cells, generator=g)
    m = torch.nn.functional.interpolate(f, size=(h, w), mode="bicubic", align_corners=False)[0, 0]
    return (m > thr).numpy().astype(np.uint8)


def _rot_rect(h, w, cx, cy, a, b, ang):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    u = (xx - cx) * c + (yy - cy) * s
    v = -(xx - cx) * s + (yy - cy) * c
    return ((np.abs(u) <= a) & (np.abs(v) <= b)).astype(np.uint8)


def _dots_ring():
    E = np.zeros((2160, 3840), np.uint8)
    E[::40, ::40] = 1; E[500:1700, 800:3000] = 0; E[520:1680, 820:2980] = 1; E[600:1600, 900:2900] = 0; E[800:1400:40, 1200:2600:40] = 1
    return E


MASKS = {"needle_4k": lambda: _rot_rect(2160, 3840, 1900, 1100, 900, 25, 0.45), "blobs_4k_0": lambda: _blobs(2160, 3840, 0),
         "blobs_1080p_4": lambda: _blobs(1080, 1920, 4), "dots_ring_4k_E": _dots_ring}


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"best_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "reps": reps}


def host_fallback(d, strategy="all"):
    polys, _ = mask_contours_device(d, strategy=strategy)
    assert polys[0] is None, "the LDS kernel took this mask"
    poly = hostops.mask_polygon(d[0].cpu().numpy() > 0, strategy)
    return poly, hostops.get_coord_min_rect_len(poly.astype(np.float32))


def _decline_everything(masks, max_pts=None, want_rect=True, strategy="all", want_parts=False, orig_hw=None):
    n = int(masks.shape[0])
    out = ([None] * n, np.zeros((n, 2)))
    return out + ([None] * n,) if want_parts else out


class large_path_off:
    def __enter__(self):
        self.real = predictor.mask_contours_large_device
        predictor.mask_contours_large_device = _decline_everything

    def __exit__(self, *a):
        predictor.mask_contours_large_device = self.real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_large_latency.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--family", default="11")
    ap.add_argument("--regress", action="store_true", help="also the 720p clips, large path on / off interleaved")
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    res = {"gpu": torch.cuda.get_device_name(0), "per_mask": {}, "clip_4k_ms_per_frame": {}}
    for name, make in MASKS.items():
        m = make()
        d = torch.from_numpy(m)[None].cuda()
        row = {"shape": list(m.shape)}
        for strategy in ("all", "largest"):
            big = timed(lambda: mask_contours_large_device(d, strategy=strategy), a.reps)
            host = timed(lambda: host_fallback(d, strategy), max(2, a.reps // 2), warm=1)
            p, r = mask_contours_large_device(d, strategy=strategy)
            hp, hl = host_fallback(d, strategy)
            row[strategy] = {"a_host_fallback": host, "b_large_device": big, "points": int(len(p[0])), "same_polygon": bool(np.array_equal(p[0], hp)),
                             "host_over_device_best": round(host["best_ms"] / big["best_ms"], 1)}
        res["per_mask"][name] = row
        print(name, json.dumps(row), flush=True)

    from helpers import make_case_family
    st, ims = make_case_family(a.family, "n", 80, 0, (8, 384, 640))
    base = [np.ascontiguousarray(np.repeat(np.repeat(im.numpy(), 2, 0), 2, 1)[:720, :1280]) for im in ims]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"{a.family}n-seg.pt")
        save_as_ultralytics_pt(st, path)
        model = YOLO(path)
        scores = [float(r.boxes.cpu().numpy().conf.max()) if len(r.boxes) else 0.0 for r in model.predict(base, conf=0.01)]
        conf = float(np.sort(scores)[len(scores) // 3]) - 1e-6
        clip4k = torch.from_numpy(np.stack([np.repeat(np.repeat(f, 3, 0), 3, 1) for f in base])).cuda()
        n4 = int(clip4k.shape[0])
        for retina in (True, False):
            key = "retina" if retina else "input"
            run = lambda: model.predict_clip(clip4k, conf=conf, batch_size=8, retina_masks=retina)
            on = timed(run, a.reps)
            with large_path_off():
                off = timed(run, max(2, a.reps // 2), warm=1)
            got = run()
            res["clip_4k_ms_per_frame"][key] = {"large_path": round(on["best_ms"] / n4, 4), "host_fallback": round(off["best_ms"] / n4, 4),
                                                "detected_frames": int(sum(got.detected)), "frames": n4}
            print("clip_4k", key, json.dumps(res["clip_4k_ms_per_frame"][key]), flush=True)
        if a.regress:
            frames = [base[i % len(base)] for i in range(64)]
            clip = torch.from_numpy(np.stack(frames)).cuda()
            reg = {}
            for retina in (True, False):
                run = lambda: model.predict_clip(clip, conf=conf, batch_size=32, retina_masks=retina)
                on, off = [], []
                for _ in range(a.rounds):
                    on.append(round(timed(run, 3)["best_ms"] / 64, 4))
                    with large_path_off():
                        off.append(round(timed(run, 3)["best_ms"] / 64, 4))
                reg["retina" if retina else "input"] = {"large_path_on": on, "large_path_off": off}
                print("clip_720p", retina, on, off, flush=True)
            res["clip_720p_ms_per_frame_bs32_dev"] = reg
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
