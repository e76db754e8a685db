#!/usr/bin/env python3
"""Head-op time of the NMS families under yp_set_nms_options, and of the default path against another build of the project.

  --part default   the head op of a synthetic 11n-seg engine at 32x640x640 and 8x1280x1280 under DEFAULT options (per-op HIP events,
                   Engine.profile), one record appended to --records. `--tree DIR` imports the package from another checkout that has
                   been built (the parent commit): run the two trees alternately, at least three rounds each, in ONE session on one
                   machine - the spread of a tree's own repeated records is what a difference has to be read against.
  --part options   the option kernels, one record appended to --records:
                   * the 1024x800 `blocks` scene of tests/nms_option_cases.py (16 800 candidates per image, B = 2, written over the
                     engine's head tensors) at max_nms 16384 (the default kernels) against 30000 (two rounds);
                   * 32x640x640 on the network's own scores at conf 0.25: default, a class set of 40 classes, agnostic, both.
  --part report    --records -> profiles/nms_options_latency.json: per tree and shape the records' median, min and max; the new tree's
                   default path passes when its median lies inside [min, max] of the parent's own records or below.
Nothing here runs without a GPU; a figure that is missing from the JSON was not measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SHAPES = [(32, 640, 640), (8, 1280, 1280)]


def _engine(shape, cache=None, calibrated=True):
    """-> (11n-seg bf16 engine, uint8 frames [B,H,W,3] on the device). calibrated: the weights are calibrated on the frame (tests/helpers.py
    make_case_family: scores of a plausible spread), which is repeated B times; `cache`: a directory that keeps the calibrated state"""
    import torch
    from yolo_puncture_amd.engine import Engine
    from yolo_puncture_amd.weights import synthetic_state_family
    B, H, W = shape
    if calibrated:
        path = os.path.join(cache, f"11n_seg_{H}x{W}.pt") if cache else None
        if path and os.path.isfile(path):
            st, im = torch.load(path)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from helpers import make_case_family
            st, im = make_case_family("11", "n", 80, 0, (1, H, W))
            if path:
                os.makedirs(cache, exist_ok=True)
                torch.save((st, im), path)
        im = im.expand(B, H, W, 3).contiguous()
    else:
        st = synthetic_state_family("11", "n", 80, seed=0)
        im = torch.zeros((B, H, W, 3), dtype=torch.uint8)
    eng = Engine("n", 80, True, "bf16", 0, state=st, family="11")
    eng.set_autotune(False)
    return eng, im.cuda()


def _head_ms(eng, im, iters):
    import torch
    out = eng.forward(im)                                 # (pushes the options, warms every kernel of the plan)
    torch.cuda.synchronize()
    rows = int((out["idx"] >= 0).sum())
    ops = eng.profile(im, iters)
    (h,) = [o for o in ops if o["kind"] == "head"]
    return h["ms"], h["kernel"], rows


def part_default(a):
    rec = {"part": "default", "label": a.label, "iters": a.iters, "shapes": {}}
    for shape in DEFAULT_SHAPES:
        eng, im = _engine(shape, a.cache)
        eng.set_nms(0.25, 0.7)
        _head_ms(eng, im, 3)
        ms, kernel, rows = _head_ms(eng, im, a.iters)
        rec["shapes"]["x".join(map(str, shape))] = {"head_ms": ms, "kernel": kernel, "rows": rows}
        eng.close()
    return rec


def part_options(a):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nms_option_cases as N
    rec = {"part": "options", "label": a.label, "iters": a.iters, "past_cap_1024x800": {}, "32x640x640": {}}
    # the crafted scene: head op alone, an event pair around `iters` launches
    c = N.resolve(next(c for c in N.CASES if c.id == "past_cap-max_nms30000"))
    t = N.inputs(c)
    eng, im = _engine((N.B,) + N.PAST_CAP_HW, calibrated=False)
    out = eng.forward(im)
    ops = eng.plan(N.B, *N.PAST_CAP_HW)
    (head,) = [i for i, o in enumerate(ops) if o["kind"] == "head"]
    amax = [i for i, o in enumerate(ops) if o["kind"] == "amax"]
    hi = ops[amax[0]]["name"].split(".")[1]
    for pre, key in (("cv3", "cls"), ("cv2", "box"), ("cv4", "cf")):
        for l in range(3):
            eng.write_tensor(eng.find_tensor(f"model.{hi}.{pre}.{l}.2"), 0, N.split_levels(c, t[key])[l])
    eng.set_nms(c.conf, c.iou)
    for max_nms in (16384, 30000):
        eng.set_nms_options(max_nms=max_nms)
        for i in amax:
            eng.run_op(i, im, out)
        for _ in range(3):
            eng.run_op(head, im, out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            eng.run_op(head, im, out)
        e1.record()
        torch.cuda.synchronize()
        rec["past_cap_1024x800"][f"max_nms{max_nms}"] = {"head_ms": e0.elapsed_time(e1) / a.iters, "kernel": eng.plan(N.B, *N.PAST_CAP_HW)[head]["kernel"],
                                                         "rows": [int(v) for v in (out["idx"] >= 0).sum(1)]}
    eng.close()
    eng, im = _engine((32, 640, 640), a.cache)
    eng.set_nms(0.25, 0.7)
    for name, o in (("default", {}), ("classes40", dict(classes=range(40))), ("agnostic", dict(agnostic=True)),
                    ("classes40_agnostic", dict(classes=range(40), agnostic=True))):
        eng.set_nms_options(**o)
        _head_ms(eng, im, 3)
        ms, kernel, rows = _head_ms(eng, im, a.iters)
        rec["32x640x640"][name] = {"head_ms": ms, "kernel": kernel, "rows": rows}
    eng.close()
    return rec


def part_report(a):
    recs = [json.loads(line) for line in open(a.records) if line.strip()]
    out = {"default_path": {}, "option_paths": None, "note": "head op time in ms; per-op HIP events (Engine.profile) unless stated"}
    trees = sorted({r["label"] for r in recs if r["part"] == "default"})
    for shape in ["x".join(map(str, s)) for s in DEFAULT_SHAPES]:
        per = {}
        for tr in trees:
            v = [r["shapes"][shape]["head_ms"] for r in recs if r["part"] == "default" and r["label"] == tr and shape in r["shapes"]]
            if v:
                per[tr] = {"records": v, "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v),
                           "kernel": next(r["shapes"][shape]["kernel"] for r in recs if r["part"] == "default" and r["label"] == tr)}
        if "parent" in per and "new" in per:
            per["new_within_parent_spread"] = per["new"]["median"] <= per["parent"]["max"]
        out["default_path"][shape] = per or "not measured"
    opts = [r for r in recs if r["part"] == "options"]
    out["option_paths"] = opts[-1] if opts else "not measured"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["default_path"]))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("default", "options", "report"), required=True)
    ap.add_argument("--tree", default=ROOT, help="checkout to import yolo_puncture_amd from (built); default: this one")
    ap.add_argument("--label", default="new", help="name of the tree in the records (the report compares `parent` and `new`)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cache", default=None, help="directory that keeps the calibrated weights between runs (they take a CPU forward to make)")
    ap.add_argument("--records", default=os.path.join(ROOT, "profiles", "nms_options_latency.jsonl"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_options_latency.json"))
    a = ap.parse_args()
    if a.part == "report":
        return part_report(a)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        sys.exit("nms_options_latency.py measures on the GPU; none is visible")
    rec = part_default(a) if a.part == "default" else part_options(a)
    rec["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.records)), exist_ok=True)
    with open(a.records, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
