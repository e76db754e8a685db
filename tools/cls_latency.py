"""Latency of the EfficientNet-B3 needle classifier (yp_cls_forward): ms per forward for fp32 and bf16 at B = 1, 4 (the app's batch) and
32, eager launches and hipGraph replay, from 1280x720 BGR frames already on the device; plus the CPU restatement (tests/effnet_ref.py,
fp32, 16 threads) at B = 1 and 4 for scale. Writes one JSON (default profiles/cls_latency.json) with the algorithmic MACs and bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_puncture_amd import classify as C  # noqa: E402


def algorithmic():
    """MACs and minimal activation bytes (each tensor written once and read once; weights once) per 380^2 image."""
    macs, acts = 3 * 9 * 40 * 190 * 190, 190 * 190 * 40
    for b in C.block_specs():
        hi, ho = b["hin"] ** 2, b["hout"] ** 2
        if b["expand"]:
            macs += hi * b["cin"] * b["cexp"]
            acts += hi * b["cexp"]
        macs += ho * b["cexp"] * b["k"] ** 2 + 2 * b["cexp"] * b["sq"] + ho * b["cexp"] * b["cout"]
        acts += ho * b["cexp"] + ho * b["cout"]
    macs += 144 * 384 * 1536 + 1536 * 2
    return macs, acts


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_latency.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    st = C.synthetic_state(0)
    rng = np.random.RandomState(0)
    res = {"gpu": torch.cuda.get_device_name(0), "frame": [720, 1280], "ms_per_forward": {}}
    for dtype in ("fp32", "bf16"):
        e = C.ClassifierEngine(dtype, 0, state=st)
        for B in (1, 4, 32):
            fr = torch.from_numpy(rng.randint(0, 256, (B, 720, 1280, 3), dtype=np.uint8)).cuda()
            bx = torch.tensor([[500 + 7 * b, 200, 700, 400] for b in range(B)], dtype=torch.int32).cuda()
            for mode in ("eager", "graph"):
                e.set_graph(mode == "graph")
                ms = timeit(lambda: e.forward(fr, bx), a.iters)
                res["ms_per_forward"][f"{dtype}_B{B}_{mode}"] = round(ms, 4)
                print(f"{dtype} B={B} {mode}: {ms:.3f} ms/forward, {ms / B:.3f} ms/image", flush=True)
            e.set_graph(False)
        e.close()
    if not a.no_cpu:
        import effnet_ref as R
        torch.set_num_threads(16)
        for B in (1, 4):
            x = torch.randn(B, 3, 380, 380)
            with torch.no_grad():
                R.forward(st, x, "fp32")
                t = time.perf_counter()
                for _ in range(3):
                    R.forward(st, x, "fp32")
            ms = (time.perf_counter() - t) * 1e3 / 3
            res["ms_per_forward"][f"cpu_restatement_fp32_B{B}_16threads"] = round(ms, 2)
            print(f"CPU restatement fp32 B={B}: {ms:.1f} ms", flush=True)
    macs, acts = algorithmic()
    res["per_image"] = {"GMAC": round(macs / 1e9, 3), "activation_MB_bf16": round(2 * 2 * acts / 1e6, 1),
                        "activation_MB_fp32": round(2 * 4 * acts / 1e6, 1), "weights_MB_fp32": round(4 * C.param_count() / 1e6, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
