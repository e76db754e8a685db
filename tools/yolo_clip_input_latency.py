#!/usr/bin/env python3
"""Latency of the YOLO segmentation pass of the speed-evaluation script's video loop (dev_tools/auto_speed_calc.py:56-84: predict without
retina masks) over a clip: ms per frame (device synchronised) for
  (a) the script's per-frame loop: predict(frame, conf) -> best row -> masks.xy[best] -> hostops.get_coord_min_rect_len;
  (b) YOLO.predict_clip(retina_masks=False) at batch_size 1, 8, 16, 32, with the frames on the host and already on the device;
on the clip of tools/yolo_clip_latency.py (64 frames of 1280x720, calibrated v8n-seg layout). Every chunk size is warmed first. Writes one
JSON (default profiles/yolo_clip_input_latency.json). `--only 32:host` runs one leg (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yolo_clip_latency import N, timed  # noqa: E402
from yolo_puncture_amd import hostops  # noqa: E402
from yolo_puncture_amd.predictor import YOLO  # noqa: E402
from yolo_puncture_amd.weights import save_as_ultralytics_pt  # noqa: E402


def script_loop(model, frames, conf):
    """dev_tools/auto_speed_calc.py:56-84 (its first loop), one frame per call."""
    boxes, coords, lens = [], [], []
    last_box, last_len = None, 0
    for f in frames:
        r = model.predict(source=f, conf=conf)[0]
        b = r.boxes.cpu().numpy()
        if len(b.cls) > 0:
            best = int(np.argmax(b.conf))
            last_box = list(map(int, b.xyxy[best].squeeze()))
            seg = r.masks.xy[best]
            coords.append(seg)
            last_len = hostops.get_coord_min_rect_len(seg)[0]
            lens.append(last_len)
            boxes.append(last_box)
        else:
            boxes.append((0, 0, f.shape[1], f.shape[0]) if last_box is None else last_box)
            coords.append(None)
            lens.append(last_len)
    return boxes, coords, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_clip_input_latency.json"))
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
            ms = timed(lambda: model.predict_clip(src, conf=conf, batch_size=int(bs), retina_masks=False), a.reps)
            print(json.dumps({"leg": a.only, "ms_per_frame": round(ms, 4)}))
            return
        legs = {"a_script_loop": lambda: script_loop(model, frames, conf)}
        for bs in (1, 8, 16, 32):
            legs[f"b_clip_bs{bs}_host"] = (lambda bs=bs: model.predict_clip(frames, conf=conf, batch_size=bs, retina_masks=False))
            legs[f"b_clip_bs{bs}_dev"] = (lambda bs=bs: model.predict_clip(dev_frames, conf=conf, batch_size=bs, retina_masks=False))
        out = {}
        for name, fn in legs.items():
            out[name] = round(timed(fn, a.reps), 4)
            print(name, f"{out[name]:.3f} ms/frame", flush=True)
        ref = script_loop(model, frames, conf)
        got = model.predict_clip(frames, conf=conf, batch_size=32, retina_masks=False)
        same_boxes = ref[0] == list(got[0])
        rel = max((abs(x - y) / max(abs(y), 1e-300) for x, y in zip(got[2], ref[2]) if x != y), default=0.0)
        res = {"gpu": torch.cuda.get_device_name(0), "layout": f"{a.family}n-seg", "dtype": model.dtype, "frames": N, "frame": [720, 1280],
               "masks": "process_mask at the letterboxed input (retina_masks=False)", "detected_frames": int(sum(got.detected)), "conf": conf,
               "clip_boxes_equal_script_loop_bs32": bool(same_boxes), "clip_lens_max_rel_diff_bs32": rel, "ms_per_frame": out,
               "speedup_vs_script_loop": {k: round(out["a_script_loop"] / v, 3) for k, v in out.items()}}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["speedup_vs_script_loop"]))


if __name__ == "__main__":
    main()
