#!/usr/bin/env python3
"""Latency of the YOLO segmentation pass of the app's video loop over a clip: ms per frame (device synchronised) for
  (a) the app's per-frame loop: predict(frame, conf, retina_masks=True) -> best row -> masks.xy[best] -> min_rect_len(best)
      (yolo_seg/app.py:91-103, what profiles/r04_latency_b1.json measures as v8n-seg_predict+xy+rect_720p);
  (b) YOLO.predict_clip at batch_size 1, 8, 16, 32, with the frames on the host (uploaded a chunk at a time) and already on the device;
on a 64-frame 1280x720 clip of a calibrated v8n-seg layout (frames upsampled 2x from the 384x640 frames it was calibrated on, as
tools/seg_frame_trace.py). Every chunk size is warmed (planned and tuned) first. Writes one JSON (default profiles/yolo_clip_latency.json).
`--only 32:host` runs one leg (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_puncture_amd.predictor import YOLO  # noqa: E402
from yolo_puncture_amd.weights import save_as_ultralytics_pt  # noqa: E402

N = 64


def app_loop(model, frames, conf):
    """yolo_seg/app.py:91-113, one frame per call."""
    boxes, coords, lens = [], [], []
    last_box, last_len = None, 0
    for f in frames:
        r = model.predict(f, conf=conf, retina_masks=True)[0]
        b = r.boxes.cpu().numpy()
        if len(b.cls) > 0:
            best = int(np.argmax(b.conf))
            last_box = list(map(int, b.xyxy[best].squeeze()))
            coords.append(r.masks.xy[best])
            last_len = r.masks.min_rect_len(best)[0]
            lens.append(last_len)
            boxes.append(last_box)
        else:
            boxes.append((0, 0, f.shape[1], f.shape[0]) if last_box is None else last_box)
            coords.append(None)
            lens.append(last_len)
    return boxes, coords, lens


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3 / N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_clip_latency.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--family", default="v8")
    ap.add_argument("--only", default=None, help="batch_size:host|dev - run that leg only, for a kernel trace")
    a = ap.parse_args()
    from helpers import make_case_family
    st, ims = make_case_family(a.family, "n", 80, 0, (8, 384, 640))
    base = [np.ascontiguousarray(np.repeat(np.repeat(im.numpy(), 2, 0), 2, 1)[:720, :1280]) for im in ims]
    frames = [base[i % len(base)] for i in range(N)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{a.family}n-seg.pt")
        save_as_ultralytics_pt(st, path)
        model = YOLO(path)
        scores = [float(r.boxes.cpu().numpy().conf.max()) if len(r.boxes) else 0.0 for r in model.predict(base, conf=0.01)]
        conf = float(np.sort(scores)[len(scores) // 3]) - 1e-6          # about a third of the frames detect nothing
        dev_frames = torch.from_numpy(np.stack(frames)).cuda()
        if a.only:
            bs, where = a.only.split(":")
            src = dev_frames if where == "dev" else frames
            ms = timed(lambda: model.predict_clip(src, conf=conf, batch_size=int(bs)), a.reps)
            print(json.dumps({"leg": a.only, "ms_per_frame": round(ms, 4)}))
            return
        legs = {"a_app_loop": lambda: app_loop(model, frames, conf)}
        for bs in (1, 8, 16, 32):
            legs[f"b_clip_bs{bs}_host"] = (lambda bs=bs: model.predict_clip(frames, conf=conf, batch_size=bs))
            legs[f"b_clip_bs{bs}_dev"] = (lambda bs=bs: model.predict_clip(dev_frames, conf=conf, batch_size=bs))
        out = {}
        for name, fn in legs.items():
            out[name] = round(timed(fn, a.reps), 4)
            print(name, f"{out[name]:.3f} ms/frame", flush=True)
        ref = app_loop(model, frames, conf)
        got = model.predict_clip(frames, conf=conf, batch_size=32)
        same = ref[0] == list(got[0]) and ref[2] == got[2]
        res = {"gpu": torch.cuda.get_device_name(0), "layout": f"{a.family}n-seg", "dtype": model.dtype, "frames": N, "frame": [720, 1280],
               "detected_frames": int(sum(got.detected)), "conf": conf, "clip_equals_app_loop_bs32": bool(same), "ms_per_frame": out,
               "speedup_vs_app_loop": {k: round(out["a_app_loop"] / v, 3) for k, v in out.items()}}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["speedup_vs_app_loop"]))


if __name__ == "__main__":
    main()
