"""Latency of the app's output frames over a 32-frame clip at 1280x720 and 1920x1080, ms per frame:
  copy_form / inplace_form   yp_overlay_frames alone (overlay_clip), device events around 8 launches over the 32 frames each, enqueued
                             while the GPU is still busy with earlier copies (so the events time kernels, not the Python call);
  dst_copy                   `dst.copy_(src)` of the same [32,H,W,3] tensor, alternated with the two forms round by round: the copy form
                             moves those bytes plus the mask reads, so copy_form / dst_copy is its distance from a plain copy;
  render_clip_*              render_clip end to end (U^2-Net-P chunks of 16 + overlay), frames on the device, without and with the
                             download through the pinned buffers (host clock around a run that ends synchronised);
  host_overlay_frame*        hostops.overlay_frame, the numpy loop body this replaces: one thread, and 16 threads over the frames.
Every leg is warmed first. Writes one JSON (default profiles/render_clip_latency.json)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_puncture_amd import hostops, u2net as U  # noqa: E402
from yolo_puncture_amd.overlay import overlay_clip, render_clip, render_labels  # noqa: E402

N = 32


def clip(H, W, seed=3):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    boxes, rois, texts = [], [], []
    for i in range(N):
        cx, cy = int(W * (0.3 + 0.4 * (i % 8) / 7)), int(H * (0.35 + 0.3 * (i // 8) / 3))
        boxes.append((cx - 30, cy - 30, cx + 30, cy + 30))
        rois.append((max(0, cx - 90), max(0, cy - 90), min(W, cx + 90), min(H, cy + 90)))
        texts.append(f"{i} {i % 2} 0.{90 + i % 10} {30 - i * 0.5:.2f} {17 + i * 0.25:.2f}")
    return frames, boxes, rois, texts


def device_ms(fn, plug, calls):
    """device time of `calls` back-to-back fn(): the plug keeps the GPU busy while the host enqueues them, so that the events bracket
    kernels and not the host's time per call (a single overlay_clip launch is shorter than the Python call that makes it)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plug()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(samples):
    return {"median": round(statistics.median(samples) / N, 5), "min": round(min(samples) / N, 5)}


def host_clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return summary(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_clip_latency.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8, help="launches per timed window")
    ap.add_argument("--plug", type=int, default=256, help="tensor copies enqueued in front of a timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_clip_latency needs the GPU: nothing is measured without one")
    eng = U.U2NetEngine("p", "fp32", 0, state=U.synthetic_state("p", 0))
    res = {"gpu": torch.cuda.get_device_name(0), "frames": N, "unit": "ms per frame", "calls_per_window": a.calls, "sizes": {}}
    for H, W in ((720, 1280), (1080, 1920)):
        frames, boxes, rois, texts = clip(H, W)
        bitmaps, xy = render_labels(texts, rois)
        geo = [U.crop_window(b, H, W) for b in boxes]
        windows = np.array([g[0] for g in geo], np.int32)
        src = torch.from_numpy(frames).cuda()
        dst = torch.empty_like(src)
        work = src.clone()
        masks = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (N, 380, 380), dtype=np.uint8)).cuda()
        labels = torch.from_numpy(bitmaps).cuda()
        legs = {"dst_copy": lambda: dst.copy_(src),
                "copy_form": lambda: overlay_clip(src, masks, windows, rois, labels, xy, out=dst),
                "inplace_form": lambda: overlay_clip(work, masks, windows, rois, labels, xy, inplace=True)}
        spare = torch.empty_like(src)

        def plug():
            for _ in range(a.plug):
                spare.copy_(src)
        samples = {k: [] for k in legs}
        for r in range(a.rounds + 2):                       # two warm rounds, then the legs alternate
            for k, fn in legs.items():
                ms = device_ms(fn, plug, a.calls)
                if r >= 2:
                    samples[k].append(ms)
        out = {k: summary(v) for k, v in samples.items()}
        out["copy_form_over_dst_copy"] = round(out["copy_form"]["median"] / out["dst_copy"]["median"], 3)
        out["frame_bytes"] = H * W * 3
        out["copy_form_gbytes_per_s"] = round(2 * H * W * 3 / (out["copy_form"]["median"] * 1e-3) / 1e9, 1)      # read + write
        out["render_clip_device_out"] = host_clock(lambda: render_clip(eng, src, boxes, rois, (labels, xy), to_host=False), a.reps)
        out["render_clip_to_host"] = host_clock(lambda: sum(1 for _ in render_clip(eng, src, boxes, rois, (labels, xy), to_host=True)), a.reps)
        crops = [m.cpu().numpy() for m in masks]

        def one(i):
            lx, ly, lw, lh = (int(v) for v in xy[i])
            return hostops.overlay_frame(frames[i], crops[i], windows[i], rois[i], bitmaps[i][:lh, :lw], (lx, ly))
        out["host_overlay_frame_1_thread"] = host_clock(lambda: [one(i) for i in range(N)], a.reps)
        with ThreadPoolExecutor(16) as pool:
            out["host_overlay_frame_16_threads"] = host_clock(lambda: list(pool.map(one, range(N))), a.reps)
        res["sizes"][f"{W}x{H}"] = out
        print(f"{W}x{H}", json.dumps(out), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
