#!/usr/bin/env python3
"""Latency of `auto_segment`'s YOLO pass over the detection frames of a DEVA run: ms per frame (device synchronised) on 64 1280x720 frames
resident on the device, yolo11n-seg layout, bf16, for
  (a) a loop of YOLO.predict_id_mask, one frame per call (the per-frame path, untouched by the clip form);
  (b) YOLO.predict_id_mask_clip at batch_size 1, 4, 8 and 32;
once as is and once with `pre_resize` for min_side = 480 (the antialiased second resize back to 720p), and for
  (c) the tail alone on one forward of 32 frames: Engine.id_masks_frames of the chunk against 32 one-frame calls.
The legs alternate in one process, five passes each, best pass reported; (a)'s five passes give its spread. `conf` is taken from the model's own
scores so that the mean number of masks per frame lies between 1 and 8 (a run without masks measures nothing). The gate: (b) at batch 32
is faster per frame than (a) by more than (a)'s spread. Writes one JSON (default profiles/auto_segment_clip_latency.json).
`--only clip32` / `--only loop` runs one leg (for a rocprofv3 kernel trace)."""
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
from yolo_puncture_amd import hostops  # noqa: E402
from yolo_puncture_amd.predictor import YOLO  # noqa: E402
from yolo_puncture_amd.weights import save_as_ultralytics_pt  # noqa: E402

N, PASSES, HW, MIN_SIDE = 64, 5, (720, 1280), 480
BATCHES = (1, 4, 8, 32)


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(legs, per):
    """every leg once per pass, PASSES passes after one warm pass -> {name: [ms per `per` items of each pass]}"""
    for fn in legs.values():
        fn()
    out = {name: [] for name in legs}
    for _ in range(PASSES):
        for name, fn in legs.items():
            out[name].append(once(fn) / per)
    return out


def pick_conf(model, base):
    """a threshold with about four masks per frame, from the model's own scores (the NMS of the 11 family runs at the threshold, so the
    mean is measured again by the caller)"""
    rows = model.predict_id_mask_clip(base, conf=1e-4, batch_size=len(base))
    scores = np.sort(np.concatenate([r[2].numpy() for r in rows]))[::-1]
    want = 4 * len(base)
    assert len(scores) > want, "the model gives too few rows to choose a threshold from"
    return float((scores[want - 1] + scores[want]) / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_segment_clip_latency.json"))
    ap.add_argument("--only", default=None, help="loop | clip32 (optionally :pre) - run that leg alone, for a kernel trace")
    a = ap.parse_args()
    from helpers import make_case_family
    st, ims = make_case_family("11", "n", 80, 0, (8, 384, 640))
    base = [np.ascontiguousarray(np.repeat(np.repeat(im.numpy(), 2, 0), 2, 1)[:HW[0], :HW[1]]) for im in ims]
    frames = [base[i % len(base)] for i in range(N)]
    scale = MIN_SIDE / min(HW)
    pre = (int(HW[1] * scale), int(HW[0] * scale))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "11n-seg.pt")
        save_as_ultralytics_pt(st, path)
        model = YOLO(path, dtype="bf16")
        conf = pick_conf(model, base)
        dev_frames = torch.from_numpy(np.stack(frames)).cuda()
        res = {"gpu": torch.cuda.get_device_name(0), "layout": "11n-seg", "dtype": model.dtype, "frames": N, "frame": list(HW), "conf": conf,
               "passes": PASSES, "min_side": MIN_SIDE}
        for tag, pr in (("as_is", None), ("pre_resize", pre)):
            kw = dict(conf=conf, out_hw=HW, suppress_small=True, min_area=100, pre_resize=pr)
            loop = lambda kw=kw: [model.predict_id_mask(f, **kw) for f in frames]
            legs = {"a_loop": loop}
            for bs in BATCHES:
                legs[f"b_clip_bs{bs}"] = (lambda bs=bs, kw=kw: model.predict_id_mask_clip(dev_frames, batch_size=bs, **kw))
            if a.only:
                leg, _, which = a.only.partition(":")
                if (which == "pre") != (pr is not None):
                    continue
                fn = legs["a_loop" if leg == "loop" else "b_clip_bs32"]
                fn()
                print(json.dumps({"leg": a.only, "ms_per_frame": round(once(fn) / N, 4)}))
                return
            # the same pictures: the loop against the clip at batch 1 (a bf16 forward at another batch runs other tile configurations, so
            # batch 32 is compared with the one-frame tail on its own forward by tests/test_gpu_id_masks_frames.py, not here)
            ref, one, got = loop(), legs["b_clip_bs1"](), legs["b_clip_bs32"]()
            same = all(torch.equal(r[0], g[0]) and torch.equal(r[1], g[1]) for r, g in zip(ref, one))
            masks = [int(g[1].shape[0]) for g in got]
            t = alternate(legs, N)
            best = {k: round(min(v), 4) for k, v in t.items()}
            spread = round(max(t["a_loop"]) - min(t["a_loop"]), 4)
            res[tag] = {"mean_masks_per_frame": round(float(np.mean(masks)), 3), "max_masks_per_frame": max(masks),
                        "clip_bs1_equals_loop": bool(same), "ms_per_frame": best, "a_loop_passes": [round(v, 4) for v in t["a_loop"]],
                        "a_loop_spread": spread, "speedup_vs_loop": {k: round(best["a_loop"] / v, 3) for k, v in best.items()},
                        "gate_bs32_faster_than_loop_by_more_than_its_spread": bool(best["a_loop"] - best["b_clip_bs32"] > spread)}
            print(tag, json.dumps(res[tag]), flush=True)
            assert 1 <= res[tag]["mean_masks_per_frame"] <= 8, "conf must leave between 1 and 8 masks per frame"
        # (c) the tail alone, on the forward the last 32-frame chunk left in the engine (as-is sizes: masks and ids at 720p)
        model.predict_id_mask_clip(dev_frames, conf=conf, out_hw=HW, suppress_small=True, min_area=100, batch_size=32)
        eng = model._engine()
        geo = hostops.letterbox_geometry(HW[0], HW[1], 640)
        out = model.__dict__["_out_cache"][(model._dev_index, 32)]
        det = out["det"].cpu()
        keeps = [torch.nonzero(det[j, :, 4] > conf).flatten() for j in range(32)]
        counts = [int(k.shape[0]) for k in keeps]
        boxes = [hostops.scale_boxes_t((geo["out_h"], geo["out_w"]), det[j][keeps[j], :4], HW).cuda() for j in range(32)]
        coeff = [out["coeff"][j][keeps[j].cuda()] for j in range(32)]
        call = dict(suppress_small=True, min_area=100)
        for tag, out_hw, mask_hw in (("tail_as_is", HW, HW), ("tail_resized", HW, (pre[1], pre[0]))):
            # (the resized leg reuses the 720p boxes on 480-line masks: the work is that of the pre_resize path, the pictures are not)
            sc = torch.tensor([mask_hw[1] / HW[1], mask_hw[0] / HW[0]] * 2, device="cuda")
            bx = [b * sc for b in boxes]
            all_c, all_b = torch.cat(coeff), torch.cat(bx)
            if mask_hw == out_hw:
                one = lambda: [eng.masks(j, coeff[j], bx[j], mask_hw, retina=True, want_masks=False, want_ids=True, **call) for j in range(32)]
            else:
                one = lambda: [eng.id_mask_resized(j, coeff[j], bx[j], mask_hw, out_hw, **call) for j in range(32)]
            many = lambda: eng.id_masks_frames(list(range(32)), counts, all_c, all_b, mask_hw, out_hw, **call)
            t = alternate({"one_frame_calls": one, "id_masks_frames": many}, 32)
            res[tag] = {"masks": int(sum(counts)), "workspace_bytes": eng.id_masks_frames_workspace(sum(counts), 32, mask_hw, out_hw),
                        "ms_per_frame": {k: round(min(v), 4) for k, v in t.items()}}
            print(tag, json.dumps(res[tag]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k]["gate_bs32_faster_than_loop_by_more_than_its_spread"] for k in ("as_is", "pre_resize")}))


if __name__ == "__main__":
    main()
