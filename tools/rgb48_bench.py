#!/usr/bin/env python3
"""tools/rgb48_bench.py -- the 16-bit RGB kernel (ptl_average_f32_to_rgb48, portal_amd/csrc/kernels/rgb48_f32.hip), both filters, beside the
kernel that moves the same bytes in both directions (ptl_average_f32_to_yuv10 at 4:4:4, yuv10_f32.hip), on the same float sub-frames,
through the C ABI.

Algorithmic bytes per launch: (16 N + 6) W H for all three (N RGBA32F sub-frames read once, 6 bytes written per pixel).  Each cell: warm-up
launches, then `--launches` launches back to back between ONE pair of events, `--repeats` times, the three kernels alternating; the median
is reported with the spread beside it, and each new kernel's bandwidth over the 4:4:4 kernel's.  One JSON line per cell and kernel.
Another build of the kernel (e.g. -DPTL_RGB48_UNROLL=1) is timed by building it in place of portal_amd/kernels/rgb48_f32.hsaco.

    python tools/rgb48_bench.py [--launches 200] [--repeats 7] [--sizes 3840x2160] [--subframes 1,4,16]
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
    ap.add_argument("--sizes", default="3840x2160")
    ap.add_argument("--subframes", default="1,4,16")
    args = ap.parse_args()
    import torch

    if pa.device_count() < 1:
        sys.exit("rgb48_bench: no HIP device visible (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    raw = stream.cuda_stream
    yardstick = "ptl_average_f32_to_yuv10:444"
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.subframes.split(",")):
            g = torch.Generator(device="cuda").manual_seed(n)
            floats = [torch.rand((h, w, 4), dtype=torch.float32, device=dev, generator=g) for _ in range(n)]
            ptrs = [f.data_ptr() for f in floats]
            assert pa.rgb48_frame_bytes(w, h) == pa.yuv10_frame_bytes(w, h, 444)
            out = torch.empty(pa.rgb48_frame_bytes(w, h), dtype=torch.uint8, device=dev)
            nbytes = (16 * n + 6) * w * h
            kernels = {yardstick: lambda: pa.average_f32_to_yuv10_device(ptrs, out.data_ptr(), w, h, 444, stream=raw),
                       "ptl_average_f32_to_rgb48:none": lambda: pa.average_f32_to_rgb48_device(ptrs, out.data_ptr(), w, h, pa.PNG_FILTER_NONE, stream=raw),
                       "ptl_average_f32_to_rgb48:sub": lambda: pa.average_f32_to_rgb48_device(ptrs, out.data_ptr(), w, h, pa.PNG_FILTER_SUB, stream=raw)}
            times = {name: [] for name in kernels}
            for launch in kernels.values():  # warm-up: code object loaded, clocks up, every buffer touched
                for _ in range(20):
                    launch()
            torch.cuda.synchronize()
            for _ in range(args.repeats):
                for name, launch in kernels.items():
                    time_launches(launch, stream, torch, args.launches, times[name])
            rate = {}
            for name in kernels:
                ms = float(np.median(times[name]))
                rate[name] = nbytes / ms / 1e9
                print(json.dumps({"kernel": name, "frame": f"{w}x{h}", "subframes": n, "bytes": nbytes, "launches": args.launches, "repeats": args.repeats, "ms": round(ms, 5),
                                  "ms_min": round(min(times[name]), 5), "ms_max": round(max(times[name]), 5), "spread_%": round(100.0 * (max(times[name]) - min(times[name])) / ms, 2),
                                  "TB/s": round(rate[name], 3)}), flush=True)
            for name in kernels:
                if name != yardstick:
                    print(json.dumps({"frame": f"{w}x{h}", "subframes": n, name.split(":")[1] + "_over_yuv444_bandwidth": round(rate[name] / rate[yardstick], 4)}), flush=True)
