#!/usr/bin/env python3
"""tools/yuv_bench.py -- the fused average-and-convert kernel (ptl_average_to_yuv420p10, portal_amd/csrc/kernels/yuv10.hip) beside
the averaging kernel it grew from (ptl_average_images), on the same inputs, through the C ABI.

Algorithmic bytes per launch: (4 N + 3) W H for the fused kernel (N RGBA8 sub-frames read once, 3 bytes of planar 4:2:0 10 bit written
per pixel), (4 N + 4) W H for averaging (one RGBA8 frame written).  N = 1 has no averaging counterpart worth timing (callers skip it).
Each cell: warm-up launches, then `--launches` launches back to back between ONE pair of events, `--repeats` times, the two kernels
alternating; the median is reported, the spread beside it.  One JSON line per cell and kernel.
--deep adds the deep-colour kernel (ptl_average_f32_to_yuv420p10, yuv10_f32.hip) to the alternation, on float sub-frames of its own:
(16 N + 3) W H bytes per launch, and its bandwidth over the averaging kernel's as a third line.
--chroma 422,444 adds the other samplings (ptl_average_to_yuv10, yuv10.hip; with --deep ptl_average_f32_to_yuv10, yuv10_f32.hip) to
the same alternation: they write 4 and 6 bytes per pixel instead of 3, and each gets a line with its bandwidth over the 4:2:0 kernel's.

    python tools/yuv_bench.py [--launches 200] [--repeats 7] [--sizes 3840x2160,7680x4320] [--subframes 1,4,16] [--deep] [--chroma 422,444]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402


def time_launches(launch, stream, torch, launches, repeats_done):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        launch()
    e1.record(stream)
    e1.synchronize()
    repeats_done.append(e0.elapsed_time(e1) / launches)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="3840x2160,7680x4320")
    ap.add_argument("--subframes", default="1,4,16")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--chroma", default="", help="further samplings beside 4:2:0: 422, 444 or both, comma-separated")
    args = ap.parse_args()
    import torch

    if pa.device_count() < 1:
        sys.exit("yuv_bench: no HIP device visible (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    raw = stream.cuda_stream
    samplings = [int(v) for v in args.chroma.split(",") if v and int(v) != 420]
    out_bytes = {422: 4, 444: 6}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.subframes.split(",")):
            g = torch.Generator(device="cuda").manual_seed(n)
            frames = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(n)]
            ptrs = [f.data_ptr() for f in frames]
            rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
            yuv = torch.empty(pa.yuv10_frame_bytes(w, h, 444), dtype=torch.uint8, device=dev)  # (the largest of the three)
            kernels = {"ptl_average_to_yuv420p10": (lambda: pa.average_to_yuv420p10_device(ptrs, yuv.data_ptr(), w, h, stream=raw), (4 * n + 3) * w * h)}
            if n > 1:
                kernels["ptl_average_images"] = (lambda: pa.average_images_device(ptrs, rgba.data_ptr(), w, h, stream=raw), (4 * n + 4) * w * h)
            if args.deep:
                floats = [torch.rand((h, w, 4), dtype=torch.float32, device=dev, generator=g) for _ in range(n)]
                float_ptrs = [f.data_ptr() for f in floats]
                kernels["ptl_average_f32_to_yuv420p10"] = (lambda: pa.average_f32_to_yuv420p10_device(float_ptrs, yuv.data_ptr(), w, h, stream=raw), (16 * n + 3) * w * h)
            for c in samplings:
                kernels[f"ptl_average_to_yuv10:{c}"] = (lambda c=c: pa.average_to_yuv10_device(ptrs, yuv.data_ptr(), w, h, c, stream=raw), (4 * n + out_bytes[c]) * w * h)
                if args.deep:
                    kernels[f"ptl_average_f32_to_yuv10:{c}"] = (lambda c=c: pa.average_f32_to_yuv10_device(float_ptrs, yuv.data_ptr(), w, h, c, stream=raw), (16 * n + out_bytes[c]) * w * h)
            times = {name: [] for name in kernels}
            for name, (launch, _) in kernels.items():  # warm-up: code object loaded, clocks up, every buffer touched
                for _ in range(20):
                    launch()
            torch.cuda.synchronize()
            for _ in range(args.repeats):
                for name, (launch, _) in kernels.items():
                    time_launches(launch, stream, torch, args.launches, times[name])
            cell = {}
            for name, (_, nbytes) in kernels.items():
                ms = float(np.median(times[name]))
                cell[name] = nbytes / ms / 1e9
                print(json.dumps({"kernel": name, "frame": f"{w}x{h}", "subframes": n, "bytes": nbytes, "launches": args.launches, "repeats": args.repeats,
                                  "ms": round(ms, 5), "ms_min": round(min(times[name]), 5), "ms_max": round(max(times[name]), 5), "TB/s": round(nbytes / ms / 1e9, 3)}), flush=True)
            if "ptl_average_images" in cell:
                print(json.dumps({"frame": f"{w}x{h}", "subframes": n, "fused_over_averaging_bandwidth": round(cell["ptl_average_to_yuv420p10"] / cell["ptl_average_images"], 4)}), flush=True)
            for c in samplings:
                print(json.dumps({"frame": f"{w}x{h}", "subframes": n, f"yuv{c}_over_yuv420_bandwidth": round(cell[f"ptl_average_to_yuv10:{c}"] / cell["ptl_average_to_yuv420p10"], 4)}), flush=True)
                if args.deep:
                    print(json.dumps({"frame": f"{w}x{h}", "subframes": n, f"deep_yuv{c}_over_deep_yuv420_bandwidth":
                                      round(cell[f"ptl_average_f32_to_yuv10:{c}"] / cell["ptl_average_f32_to_yuv420p10"], 4)}), flush=True)
            if "ptl_average_images" in cell and "ptl_average_f32_to_yuv420p10" in cell:
                print(json.dumps({"frame": f"{w}x{h}", "subframes": n, "deep_over_averaging_bandwidth": round(cell["ptl_average_f32_to_yuv420p10"] / cell["ptl_average_images"], 4)}), flush=True)
