#!/usr/bin/env python3
"""The generic fp32 attention kernel and the fp32 streaming kernel alone, side by side (yp_debug_attention_f32, key_dim 32, head_dim 64):
one process, the two kernels alternating on the same qkv tensor after a warm-up, an event pair around each batch of `--launches` calls
(>= 20), best of `--rounds`. The hook drains the stream before it returns, so a figure is launch + kernel + drain per call, the same
overhead on both sides: the ratio understates the kernels' own.
Cases (B, N, nh): (8, 1600, 4) v10-S at 8x1280x1280, (4, 2040, 4) v10-S at 4x1088x1920, (1, 920, 4) v10-S at 1x736x1280, (1, 3680, 2) 11n
at 2560x1472 and (1, 8160, 2) 11n on a 4K frame at its own size. The generic kernel is timed where it runs (N <= 2368). TFLOP/s count the
algorithm (2 B nh N^2 (kd + hd)), not the streaming kernel's second Q.K^T.
Writes profiles/attention_stream_f32_latency.json and exits non-zero when the streaming kernel is not faster than the generic one at
(8, 1600, 4).
--heads wide: the same for YOLOv10-M's heads (key_dim 36, head_dim 72) and attention_stream_wide_f32_kernel (switch value "stream_wide"):
(8, 1600, 4), (4, 2040, 4), (1, 920, 4), (1, 3680, 4), (1, 8160, 4), the generic kernel where it runs (N <= 2364), the same gate; writes
profiles/attention_stream_wide_f32_latency.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_puncture_amd.engine import attention_f32  # noqa: E402

GATE = (8, 1600, 4)
# per --heads: cases (B, N, nh), key_dim, head_dim, the generic kernel's last N, the switch value, the kernel number it must report, output
HEADS = {"narrow": ([(8, 1600, 4), (4, 2040, 4), (1, 920, 4), (1, 3680, 2), (1, 8160, 2)], 32, 64, 2368, "stream", 4, "attention_stream_f32_latency.json"),
         "wide": ([(8, 1600, 4), (4, 2040, 4), (1, 920, 4), (1, 3680, 4), (1, 8160, 4)], 36, 72, 2364, "stream_wide", 5, "attention_stream_wide_f32_latency.json")}


def batch_ms(qkv, out, nh, kd, hd, f32, launches, wgs=0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        attention_f32(qkv, nh, kd, hd, out=out, f32=f32, wgs=wgs)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wgs", type=int, default=0, help="the streaming kernel's workgroup target for the run (0: the launcher's own)")
    ap.add_argument("--heads", choices=sorted(HEADS), default="narrow", help="narrow: 32/64 heads; wide: YOLOv10-M's 36/72")
    ap.add_argument("--out", default=None, help="default: profiles/attention_stream_f32_latency.json, attention_stream_wide_f32_latency.json for --heads wide")
    a = ap.parse_args()
    CASES, KD, HD, GENERIC_MAX_TOKENS, value, number, name = HEADS[a.heads]
    WANT = {"generic": 0, "stream": number}
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", name)
    if not torch.cuda.is_available():
        sys.exit("attention_f32_latency.py measures on the GPU; none is visible")
    if a.launches < 20:
        sys.exit("--launches: at least 20")
    res = {"device": torch.cuda.get_device_name(0), "dtype": "fp32", "kd": KD, "hd": HD, "launches_per_batch": a.launches, "rounds": a.rounds, "wgs": a.wgs,
           "cases": {}}
    for B, N, nh in CASES:
        g = torch.Generator().manual_seed(B * 100003 + N * 7 + nh)
        qkv = torch.randn((B, N, nh * (2 * KD + HD)), generator=g).cuda()
        out = torch.empty((B, N, nh * HD), dtype=torch.float32, device="cuda")
        kinds = (["generic"] if N <= GENERIC_MAX_TOKENS else []) + ["stream"]
        for f in kinds:                                            # warm-up (and: each side takes the kernel this file is about)
            for _ in range(3):
                assert attention_f32(qkv, nh, KD, HD, out=out, f32=value if f == "stream" else f)[1] == WANT[f]
        ts = {f: [] for f in kinds}
        for _ in range(a.rounds):                                  # alternating
            for f in kinds:
                ts[f].append(batch_ms(qkv, out, nh, KD, HD, value if f == "stream" else f, a.launches, a.wgs if f == "stream" else 0))
        flop = 2.0 * B * nh * N * N * (KD + HD)
        rec = {}
        for f in kinds:
            best = min(ts[f])
            rec[f] = {"best_ms": round(best, 4), "median_ms": round(statistics.median(ts[f]), 4), "tflops_at_best": round(flop / best * 1e-9, 2)}
        if "generic" in rec:
            rec["generic_over_stream"] = round(rec["generic"]["best_ms"] / rec["stream"]["best_ms"], 2)
        res["cases"][f"{B}x{N}x{nh}"] = rec
        print(f"{B}x{N}x{nh}", json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    gate = res["cases"]["%dx%dx%d" % GATE]
    if not gate["stream"]["best_ms"] < gate["generic"]["best_ms"]:
        sys.exit("the streaming kernel is not faster than the generic one at (8, 1600, 4)")


if __name__ == "__main__":
    main()
