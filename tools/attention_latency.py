#!/usr/bin/env python3
"""The generic and the streaming attention kernel alone, side by side (yp_debug_attention_form, bf16, key_dim 32, head_dim 64): one
process, the two kernels alternating on the same qkv tensor after a warm-up, an event pair around each batch of `--launches` calls (>= 20).
The hook drains the stream before it returns, so a figure is launch + kernel + drain per call, the same overhead on both sides: the ratio
understates the kernels' own (per-op event timings inside an engine: tools/large_input_latency.py --attention stream).
Cases (B, N, nh): (8, 1600, 4) v10-S at 8x1280x1280, (4, 2040, 4) v10-S at 4x1088x1920, (1, 920, 4) v10-S at 1x736x1280, (8, 1600, 2)
11n at 8x1280x1280, (1, 3680, 2) 11n at 2560x1472 and (1, 8160, 2) 11n on a 4K frame at its own size. The generic kernel is timed where it
runs (N <= 2368). TFLOP/s count the algorithm (2 B nh N^2 (kd + hd)), not the streaming kernel's second Q.K^T.
Writes profiles/attention_stream_latency.json and exits non-zero when the streaming kernel is not faster than the generic one at
(8, 1600, 4).

--heads wide: the same for key_dim 36, head_dim 72 (YOLOv10-M, four heads), the generic kernel against attention_stream_wide_kernel (form
"stream_wide"), which takes every token count. Cases: (16, 400, 4) M's packaged 16x640x640 workload, (1, 400, 4) one such image (16
workgroups), (8, 1600, 4), (4, 2040, 4), and (1, 3680, 4), (1, 8160, 4), which the generic kernel refuses (N > 2364). Same gate, at
(8, 1600, 4). Writes profiles/attention_stream_wide_latency.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_puncture_amd.engine import attention  # noqa: E402

GATE = (8, 1600, 4)
# --heads: (cases, kd, hd, the generic kernel's last N, the streaming form, its kernel_out, the output file)
HEADS = {"narrow": ([(8, 1600, 4), (4, 2040, 4), (1, 920, 4), (8, 1600, 2), (1, 3680, 2), (1, 8160, 2)], 32, 64, 2368, "stream", 2,
                    "attention_stream_latency.json"),
         "wide": ([(16, 400, 4), (1, 400, 4), (8, 1600, 4), (4, 2040, 4), (1, 3680, 4), (1, 8160, 4)], 36, 72, 2364, "stream_wide", 3,
                  "attention_stream_wide_latency.json")}
KD, HD = 32, 64


def batch_ms(qkv, out, nh, form, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        attention(qkv, nh, KD, HD, out=out, form=form)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--heads", choices=sorted(HEADS), default="narrow", help="wide: key_dim 36, head_dim 72 under the form stream_wide")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    global KD, HD
    CASES, KD, HD, GENERIC_MAX_TOKENS, stream_form, stream_kernel, out_name = HEADS[a.heads]
    a.out = a.out or os.path.join(ROOT, "profiles", out_name)
    if not torch.cuda.is_available():
        sys.exit("attention_latency.py measures on the GPU; none is visible")
    if a.launches < 20:
        sys.exit("--launches: at least 20")
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "kd": KD, "hd": HD, "launches_per_batch": a.launches, "rounds": a.rounds, "cases": {}}
    for B, N, nh in CASES:
        g = torch.Generator().manual_seed(B * 100003 + N * 7 + nh)
        qkv = torch.randn((B, N, nh * (2 * KD + HD)), generator=g).to(torch.bfloat16).cuda()
        out = torch.empty((B, N, nh * HD), dtype=torch.bfloat16, device="cuda")
        forms = (["auto"] if N <= GENERIC_MAX_TOKENS else []) + [stream_form]
        want = {"auto": 0, stream_form: stream_kernel}
        for f in forms:                                            # warm-up (and: each form takes the kernel this file is about)
            for _ in range(3):
                assert attention(qkv, nh, KD, HD, out=out, form=f)[1] == want[f]
        ts = {f: [] for f in forms}
        for _ in range(a.rounds):                                  # alternating
            for f in forms:
                ts[f].append(batch_ms(qkv, out, nh, f, a.launches))
        flop = 2.0 * B * nh * N * N * (KD + HD)
        rec = {}
        for f, name in (("auto", "generic"), (stream_form, "stream")):
            if f in ts:
                best = min(ts[f])
                rec[name] = {"best_ms": round(best, 4), "median_ms": round(statistics.median(ts[f]), 4), "tflops_at_best": round(flop / best * 1e-9, 2)}
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
