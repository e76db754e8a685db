#!/usr/bin/env python3
"""Step time of inputs beyond 12288 anchors (the heads' large forms, csrc/head_large.hip, and the generic attention kernel above 400
tokens) beside the 640x640 step of the same pixel count. Engines: YOLOv10-S detect and YOLO11-N seg, bf16, synthetic weights, tile
configurations tuned on first use (no packaged table covers the large shapes). Shapes:
    32x640x640   the flagship batch (8400 anchors, 400 tokens: LDS heads, matrix-core attention)
    8x1280x1280  the same pixel count, so the same convolution work (33600 anchors, 1600 tokens)
    4x1088x1920  a 1080p frame at imgsz=1920 (42840 anchors, 2040 tokens)
    1x736x1280   a 1080p frame at imgsz=1280 (19320 anchors, 920 tokens)
Per engine and shape: the forward eager and as hipGraph replay (frames resident in HBM, warmed, a device synchronisation per timed call;
best and median in ms), and the per-op event timings (Engine.profile, eager, one event pair per launch) of the class-max pass, the head op
(select or NMS kernels) and the attention op. `ratio_8x1280_vs_32x640` is the replay step of 8x1280x1280 over that of 32x640x640; the
per-op lines say how much of the excess is the head's and how much the attention's.
Writes profiles/large_input_latency.json.

--attention stream: the same engines with the PSA block's streaming kernel (Engine.set_attention_form) beside the default form, per shape
one after the other in one process (the form is switched on one engine: same weights, same tile configurations), over the shapes above
400 tokens plus two the default form refuses: 1x1472x2560 (3680 tokens) and 1x2176x3840, a 4K frame at its own size (8160 tokens). Each
shape holds one record per form ("auto": the timings, or the planner's refusal). Writes profiles/large_input_latency_stream.json.

--attention stream_wide: the same comparison for a YOLOv10-M detect engine (key_dim 36, head_dim 72: attention_stream_wide_kernel at every
token count) at 16x640x640 (its packaged workload, 400 tokens), 8x1280x1280, 1x1472x2560 and 1x2176x3840; the default form refuses the
last two (above 2364 tokens). Writes profiles/large_input_latency_stream_wide.json."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_puncture_amd.engine import Engine, YolopError  # noqa: E402
from yolo_puncture_amd.weights import synthetic_state, synthetic_state_family  # noqa: E402

SHAPES = [(32, 640, 640), (8, 1280, 1280), (4, 1088, 1920), (1, 736, 1280)]
STREAM_SHAPES = [(8, 1280, 1280), (4, 1088, 1920), (1, 736, 1280), (1, 1472, 2560), (1, 2176, 3840)]
WIDE_SHAPES = [(16, 640, 640), (8, 1280, 1280), (1, 1472, 2560), (1, 2176, 3840)]
ENGINES = [("v10", "s", False), ("11", "n", True)]
WIDE_ENGINES = [("v10", "m", False)]


def timed(fn, reps, warm=3):
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


def op_lines(ops):
    """the ops the large forms change: class-max pass (its own launch or fused into the logits conv), head, attention"""
    out = {"class_max_ms": 0.0, "head_ms": 0.0, "attention_ms": 0.0, "total_ms": round(sum(o["ms"] for o in ops), 4), "kernels": {}}
    for o in ops:
        if o["kernel"] == "-":
            continue
        key = None
        if o["kind"] == "head":
            key = "head_ms"
        elif o["kind"] == "attn":
            key = "attention_ms"
        elif o["kind"] == "amax" or o["form"] == "cls_out":
            key = "class_max_ms"
        if key:
            out[key] = round(out[key] + o["ms"], 4)
            out["kernels"][o["name"]] = {"kernel": o["kernel"], "ms": round(o["ms"], 4)}
    return out


def measure(eng, im, reps):
    B, H, W = im.shape[:3]
    rec = {"anchors": sum((H // s) * (W // s) for s in (8, 16, 32)), "tokens": (H // 32) * (W // 32), "max_batch": eng.max_batch(H, W)}
    eng.set_graph(False)
    eng.forward(im)                                    # plans, tunes
    torch.cuda.synchronize()
    rec["eager"] = timed(lambda: eng.forward(im), reps)
    eng.set_graph(True)
    rec["replay"] = timed(lambda: eng.forward(im), reps)
    eng.set_graph(False)
    rec["ops"] = op_lines(eng.profile(im, iters=5))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--attention", choices=("auto", "stream", "stream_wide"), default="auto",
                    help="stream / stream_wide: both forms per shape, into large_input_latency_stream.json / large_input_latency_stream_wide.json")
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="", help="comma-separated indices into the shape list (default: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("large_input_latency.py measures on the GPU; none is visible")
    stream = a.attention != "auto"
    all_shapes = {"auto": SHAPES, "stream": STREAM_SHAPES, "stream_wide": WIDE_SHAPES}[a.attention]
    shapes = [all_shapes[int(i)] for i in a.shapes.split(",")] if a.shapes else all_shapes
    a.out = a.out or os.path.join(ROOT, "profiles", {"auto": "large_input_latency.json", "stream": "large_input_latency_stream.json",
                                                     "stream_wide": "large_input_latency_stream_wide.json"}[a.attention])
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "reps": a.reps, "engines": {}}
    for family, variant, seg in (WIDE_ENGINES if a.attention == "stream_wide" else ENGINES):
        st = synthetic_state(variant, 80, seg, seed=0, cls_bias=-3.0) if family == "v10" else synthetic_state_family(family, variant, 80, seed=0, cls_bias=-3.0)
        eng = Engine(variant, 80, seg, "bf16", 0, state=st, family=family)
        rows = {}
        for B, H, W in shapes:
            g = torch.Generator().manual_seed(B * H + W)
            im = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
            if stream:
                rec = {}
                for form in ("auto", a.attention):
                    eng.set_attention_form(form)
                    try:
                        rec[form] = measure(eng, im, a.reps)
                    except YolopError as e:                    # the default form above 2368 tokens
                        rec[form] = {"refused": str(e)}
                    print(family + variant, f"{B}x{H}x{W}", form, json.dumps(rec[form].get("replay", rec[form])),
                          json.dumps({k: v for k, v in rec[form].get("ops", {}).items() if k != "kernels"}), flush=True)
                if "replay" in rec["auto"]:
                    rec["replay_best_auto_over_stream"] = round(rec["auto"]["replay"]["best_ms"] / rec[a.attention]["replay"]["best_ms"], 4)
                    rec["attention_ms_auto_over_stream"] = round(rec["auto"]["ops"]["attention_ms"] / rec[a.attention]["ops"]["attention_ms"], 2)
                rows[f"{B}x{H}x{W}"] = rec
                continue
            rec = measure(eng, im, a.reps)
            rows[f"{B}x{H}x{W}"] = rec
            print(family + variant, f"{B}x{H}x{W}", json.dumps(rec["replay"]), json.dumps({k: v for k, v in rec["ops"].items() if k != "kernels"}), flush=True)
        if "32x640x640" in rows and "8x1280x1280" in rows:
            s, l = rows["32x640x640"], rows["8x1280x1280"]
            rows["ratio_8x1280_vs_32x640"] = {
                "replay_best": round(l["replay"]["best_ms"] / s["replay"]["best_ms"], 4),
                "eager_best": round(l["eager"]["best_ms"] / s["eager"]["best_ms"], 4),
                "per_op_excess_ms": {k: round(l["ops"][k] - s["ops"][k], 4) for k in ("class_max_ms", "head_ms", "attention_ms", "total_ms")}}
        res["engines"][f"{family}{variant}-{'seg' if seg else 'det'}"] = rows
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
