#!/usr/bin/env python3
"""Latency of the "all_merged" bridge on the device (yp_mask_contours_merge, csrc/contour_merge.hip) against the host bridge it replaces.
One process, every buffer resident in HBM, every leg warmed, then timed repeats with a device synchronisation each (best, median and the
spread min .. max in ms):
  per contour list, fed as point buffers (three rings of 6000 / 6000 / 3000 points; 3000 four-point blobs):
    (a) host_parent   what ran before the device bridge: device-to-host copy of counts, lengths and points + the bridge with one
                      |a| x |b| x 2 int64 table per pair (restated here as `parent_merge_contours`)
    (b) host_blocked  the same copy + hostops.merge_contours as it is now (the table in row blocks)
    (c) device        contours_merge_device + the copy of the bridged list to the host
  a single-contour 1280x720 mask (the app's case) through mask_contours_device: strategy "all" against "all_merged", interleaved over
  several rounds; the difference is what the bridge's five launches cost where there is nothing to bridge.
Writes profiles/contour_merge_latency.json. The default-strategy predict_clip (no new code runs) is timed with
tools/yolo_clip_latency.py --only 32:dev on the parent's tree and on this one in turn; those figures are added to the JSON by hand
(`clip_720p_v8_parent_vs_change_ms_per_frame_bs32_dev`), as are bench.py's on both trees and the launch cost quoted from
profiles/r01_micro_launch_bench.txt; a later run of this tool keeps those keys (HAND_KEYS) and replaces only its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_puncture_amd import hostops  # noqa: E402
from yolo_puncture_amd.engine import contours_merge_device, mask_contours_device  # noqa: E402


# keys of the JSON that this tool does not measure (see the docstring): a run keeps what the file holds under them
HAND_KEYS = ("clip_720p_v8_parent_vs_change_ms_per_frame_bs32_dev", "bench_py_parent_vs_change_ms_per_step", "launch_cost_us_per_kernel")


def parent_merge_contours(contours):
    """hostops.merge_contours before its distance table was cut into row blocks"""
    segs = [np.asarray(c).reshape(-1, 2) for c in contours]
    n = len(segs)
    if n < 2:
        return segs[0] if n else np.zeros((0, 2), dtype=np.int32)
    near = [[] for _ in range(n)]
    for i in range(1, n):
        a, b = segs[i - 1].astype(np.int64), segs[i].astype(np.int64)
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        j = int(d.argmin())
        near[i - 1].append(j // d.shape[1])
        near[i].append(j % d.shape[1])
    out, back = [], []
    for i in range(n):
        idx, seg = near[i], segs[i]
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
    return {"best_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "max_ms": round(max(ts), 4), "reps": reps}


def main():
    from merge_cases import blobs, pack, ring
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_merge_latency.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {"gpu": torch.cuda.get_device_name(0), "lists": {}}
    lists = {"rings_6000_6000_3000": [ring(1000, 1000, 900, 6000), ring(3000, 1000, 900, 6000), ring(2000, 3000, 450, 3000)],
             "blobs_3000_x4": blobs(3000, per_row=60)}
    for name, mask in lists.items():
        pts, count, parts = (torch.from_numpy(x).cuda() for x in pack([mask]))
        lens = [len(c) for c in mask]

        def host(merge):
            c = int(count.cpu()[0])
            ln = parts[0, 1:1 + int(parts[0, 0].cpu())].cpu().numpy()
            return merge(np.split(pts[0, :c].cpu().numpy(), np.cumsum(ln)[:-1]))

        def device():
            out, oc = contours_merge_device(pts, count, parts)
            return out[0, :int(oc.cpu()[0])].cpu().numpy()

        want = host(hostops.merge_contours)
        row = {"contours": len(lens), "points": int(sum(lens)), "merged_points": int(len(want)),
               "same_as_host": bool(np.array_equal(device(), want) and np.array_equal(host(parent_merge_contours), want)),
               "a_host_parent": timed(lambda: host(parent_merge_contours), a.host_reps, warm=1),
               "b_host_blocked": timed(lambda: host(hostops.merge_contours), a.host_reps, warm=1),
               "c_device": timed(device, a.reps)}
        row["host_parent_over_device_median"] = round(row["a_host_parent"]["median_ms"] / row["c_device"]["median_ms"], 1)
        res["lists"][name] = row
        print(name, json.dumps(row), flush=True)

    m = np.zeros((1, 720, 1280), np.uint8)
    yy, xx = np.mgrid[0:720, 0:1280]
    m[0] = (np.abs((xx - 640) * 0.9 + (yy - 360) * 0.43) <= 420) & (np.abs(-(xx - 640) * 0.43 + (yy - 360) * 0.9) <= 14)      # a slanted needle
    d = torch.from_numpy(m).cuda()
    p_all, _ = mask_contours_device(d, strategy="all")
    p_mrg, _ = mask_contours_device(d, strategy="all_merged")
    one = {"shape": [720, 1280], "points": int(len(p_all[0])), "same_polygon": bool(np.array_equal(p_all[0], p_mrg[0])), "all": [], "all_merged": []}
    for _ in range(a.rounds):
        one["all"].append(timed(lambda: mask_contours_device(d, strategy="all"), a.reps)["median_ms"])
        one["all_merged"].append(timed(lambda: mask_contours_device(d, strategy="all_merged"), a.reps)["median_ms"])
    one["all_median_of_rounds_ms"] = round(statistics.median(one["all"]), 4)
    one["all_merged_median_of_rounds_ms"] = round(statistics.median(one["all_merged"]), 4)
    one["extra_ms"] = round(one["all_merged_median_of_rounds_ms"] - one["all_median_of_rounds_ms"], 4)
    res["single_contour_720p"] = one
    print("single_contour_720p", json.dumps(one), flush=True)
    if os.path.isfile(a.out):                                # figures recorded by hand beside the tool's own keys stay in the file
        with open(a.out) as f:
            res = {**{k: v for k, v in json.load(f).items() if k in HAND_KEYS}, **res}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
