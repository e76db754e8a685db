"""Latency of U^2-Net-P over a clip: ms per frame (device synchronised) for
  (a) the reference-shaped loop: host crop_frame, unet_predict (B = 1, H2D + forward + D2H), host paste into a full-frame mask;
  (b) unet_predict_clip at batch_size 1, 4, 8, 16, with the frames on the host (uploaded a chunk at a time) and already on the device;
on a 64-frame 1280x720 synthetic clip whose boxes hit every crop case (interior, narrow edge -> padded, short edge -> unpadded h x 380,
corners), fp32 and bf16. Every crop shape and chunk size is warmed first. Writes one JSON (default profiles/u2net_clip_latency.json)
with the conv MACs per 380^2 crop and the achieved rate. `--only fp32:16:dev` runs one leg (for a rocprofv3 kernel trace)."""
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
from yolo_puncture_amd import u2net as U  # noqa: E402

H, W, N = 720, 1280, 64
CENTRES = [(640, 360), (100, 360), (1200, 400), (640, 100), (700, 650), (50, 60), (1230, 40), (80, 690), (1250, 700),
           (400, 150), (900, 600), (640, 120), (300, 300), (1000, 450), (500, 500), (800, 250)]


def boxes():
    out = []
    for i in range(N):
        cx, cy = CENTRES[i % len(CENTRES)]
        out.append((cx - 30, cy - 30, cx + 30, cy + 30))
    return out


def conv_macs(h, w, variant="p"):
    """Multiply-accumulates of every convolution (conv_specs) for one h x w crop: 3x3 convs at their pyramid level (ceil-mode halving),
    side convs at their level, the 1x1 fusion at full size."""
    lh, lw = [h], [w]
    for _ in range(5):
        lh.append((lh[-1] + 1) // 2)
        lw.append((lw[-1] + 1) // 2)
    cfg = U._CFG[variant]
    kinds = {f"stage{i + 1}": k for i, (k, *_r) in enumerate(cfg["enc"])}
    kinds.update({f"stage{5 - j}d": k for j, (k, *_r) in enumerate(cfg["dec"])})
    total = 0
    for name, cin, cout, _ in U.conv_specs(variant):
        if name == "outconv":
            total += h * w * cin * cout
            continue
        if name.startswith("side"):
            lvl = int(name[4:]) - 1
        else:
            stage, conv = name.split(".")
            base = int(stage[5]) - 1
            kind = kinds[stage]
            n = 4 if kind == "RSU4F" else int(kind[3:])
            k = conv[len("rebnconv"):]
            if kind == "RSU4F" or k in ("in", "1", "1d"):
                lvl = base
            elif k.endswith("d"):
                lvl = base + int(k[:-1]) - 1
            elif int(k) == n:
                lvl = base + n - 2
            else:
                lvl = base + int(k) - 1
        total += lh[lvl] * lw[lvl] * cin * cout * 9
    return total


def reference_loop(eng, frames, bxs):
    out = []
    for f, b in zip(frames, bxs):
        (x1, y1, x2, y2), shape = U.crop_window(b, H, W)
        crop = np.zeros(shape + (3,), np.uint8)
        crop[:y2 - y1, :x2 - x1] = f[y1:y2, x1:x2]
        m = U.unet_predict(eng, crop)
        full = np.zeros((H, W), np.uint8)
        full[y1:y2, x1:x2] = m[:y2 - y1, :x2 - x1]
        out.append(full)
    return out


def timed(fn, reps):
    fn()                                   # warm: every shape and chunk size planned and tuned
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u2net_clip_latency.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="dtype:batch_size:host|dev - run that leg only, for a kernel trace")
    a = ap.parse_args()
    from helpers import rand_image
    frames = rand_image((N, H, W, 3), seed=7).numpy()
    bxs = boxes()
    shapes = sorted({U.crop_window(b, H, W)[1] for b in bxs})
    st = U.synthetic_state("p", 0)
    dev_frames = torch.from_numpy(frames).cuda()
    host_frames = list(frames)
    if a.only:
        dtype, bs, where = a.only.split(":")
        eng = U.U2NetEngine("p", dtype, 0, state=st)
        src = dev_frames if where == "dev" else host_frames
        ms = timed(lambda: U.unet_predict_clip(eng, src, bxs, batch_size=int(bs)), a.reps)
        print(json.dumps({"leg": a.only, "ms_per_frame": round(ms, 4)}))
        eng.close()
        return
    macs380 = conv_macs(380, 380)
    res = {"gpu": torch.cuda.get_device_name(0), "frames": N, "frame": [H, W], "crop_shapes": [list(s) for s in shapes],
           "conv_macs_per_380x380_crop": macs380, "ms_per_frame": {}, "conv_tmacs_per_s": {}, "speedup_vs_reference_loop": {}}
    for dtype in ("fp32", "bf16"):
        eng = U.U2NetEngine("p", dtype, 0, state=st)
        legs = {"a_reference_loop": lambda: reference_loop(eng, host_frames, bxs)}
        for bs in (1, 4, 8, 16):
            legs[f"b_clip_bs{bs}_host"] = (lambda bs=bs: U.unet_predict_clip(eng, host_frames, bxs, batch_size=bs))
            legs[f"b_clip_bs{bs}_dev"] = (lambda bs=bs: U.unet_predict_clip(eng, dev_frames, bxs, batch_size=bs))
        legs["b_clip_bs16_dev_full_frame"] = lambda: U.unet_predict_clip(eng, dev_frames, bxs, batch_size=16, full_frame=True)
        out, rate, sp = {}, {}, {}
        for name, fn in legs.items():
            ms = timed(fn, a.reps)
            out[name] = round(ms, 4)
            rate[name] = round(macs380 / (ms * 1e-3) / 1e12, 3)          # as if every crop were 380 x 380 (most are)
            print(dtype, name, f"{ms:.3f} ms/frame", flush=True)
        for name in out:
            sp[name] = round(out["a_reference_loop"] / out[name], 3)
        res["ms_per_frame"][dtype], res["conv_tmacs_per_s"][dtype], res["speedup_vs_reference_loop"][dtype] = out, rate, sp
        eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["speedup_vs_reference_loop"]))


if __name__ == "__main__":
    main()
