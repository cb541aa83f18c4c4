#!/usr/bin/env python3
"""tools/pass_bench.py -- what the trace passes cost, through the Python mirror of the C ABI.

1. The headline frame (scenes/portal_in_portal.ron, 3840x2160, depth 40, one stream) drawn by the plain build and by the pass build of the
   same flags, alternating: plain with an RGBA8 target, plain with RGBA8 + RGBA32F (the same 16 bytes per pixel the record adds), the pass
   build with RGBA8 + records, and the pass build drawn plain (no records stored).  Per build: VGPRs, waves per SIMD and the sha256 of the
   code object.
2. ptl_pass_stats and both conversions of ptl_passes_to_gray16 on the records of that frame, beside ptl_average_images (N = 4) in the same
   run; TB/s over the bytes the algorithm needs (16, 18, 18 and 4 N + 4 per pixel).
Each cell: warm-up, then `--launches` calls back to back between ONE pair of events, `--repeats` times, the candidates alternating; median,
min and max.  One JSON line per cell.

    python tools/pass_bench.py [--launches 50] [--repeats 7] [--size 3840x2160]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402


def timed(launch, stream, torch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def measure(cells, stream, torch, launches, repeats):
    """cells: {name: launch} -> {name: [ms per launch, one per repeat]}, the cells alternating"""
    for launch in cells.values():
        for _ in range(10):
            launch()
    torch.cuda.synchronize()
    times = {name: [] for name in cells}
    for _ in range(repeats):
        for name, launch in cells.items():
            times[name].append(timed(launch, stream, torch, launches))
    return times


def report(kind, name, ms_list, extra):
    ms = float(np.median(ms_list))
    print(json.dumps(dict(kind=kind, cell=name, ms=round(ms, 5), ms_min=round(min(ms_list), 5), ms_max=round(max(ms_list), 5), **extra(ms))), flush=True)
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--depth", type=int, default=40)
    args = ap.parse_args()
    import torch

    if pa.device_count() < 1:
        sys.exit("pass_bench: no HIP device visible (nothing is measured without one)")
    w, h = (int(v) for v in args.size.split("x"))
    n_px = w * h
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    raw = stream.cuda_stream
    spec = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL
    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    builds = {"plain": pa.SceneRenderer(scene, device=0, flags=spec), "passes": pa.SceneRenderer(scene, device=0, flags=spec | pa.FLAG_PASSES)}
    for name, r in builds.items():
        r.set_option("render_depth", args.depth)
        vgprs = r.code_object_note(".vgpr_count")
        print(json.dumps(dict(kind="build", build=name, vgprs=vgprs, waves_per_simd=min(8, 512 // max(1, -(-vgprs // 8) * 8)), sgprs=r.code_object_note(".sgpr_count"),
                              scratch=r.code_object_note(".private_segment_fixed_size"), code_object_sha256=hashlib.sha256(r.code_object()).hexdigest())), flush=True)
    frame = pa.Frame(w, h, 0, 1, 0)
    out8 = torch.empty(n_px * 4, dtype=torch.uint8, device=dev)
    out32 = torch.empty(n_px * 4, dtype=torch.float32, device=dev)
    records = torch.empty(n_px * 16, dtype=torch.uint8, device=dev)
    draws = {"plain build, RGBA8": lambda: builds["plain"].draw_device(frame, out8.data_ptr(), stream=raw),
             "plain build, RGBA8 + RGBA32F": lambda: builds["plain"].draw_device(frame, out8.data_ptr(), out32.data_ptr(), stream=raw),
             "pass build, RGBA8 + records": lambda: builds["passes"].draw_passes_device(frame, records.data_ptr(), n_px * 16, out8.data_ptr(), stream=raw),
             "pass build, RGBA8, no records": lambda: builds["passes"].draw_device(frame, out8.data_ptr(), stream=raw)}
    base = None
    for name, ms_list in measure(draws, stream, torch, args.launches, args.repeats).items():
        ms = report("draw", name, ms_list, lambda ms: dict(frame=f"{w}x{h}", depth=args.depth, over_plain=round(ms / base, 4) if base else 1.0))
        base = base or ms

    # the post-process kernels on the records the last pass draw left
    block = torch.zeros(pa.PASS_STATS_BLOCK.itemsize, dtype=torch.uint8, device=dev)
    per_launch = torch.zeros(1, dtype=torch.int64, device=dev)
    grey = torch.empty(n_px * 2, dtype=torch.uint8, device=dev)
    subs = [torch.randint(0, 256, (n_px * 4,), dtype=torch.uint8, device=dev) for _ in range(4)]
    sub_ptrs = [s.data_ptr() for s in subs]
    kernels = {"ptl_average_images, N = 4": (lambda: pa.average_images_device(sub_ptrs, out8.data_ptr(), w, h, stream=raw), 20),
               "ptl_pass_stats": (lambda: pa.pass_stats_device(records.data_ptr(), n_px, block.data_ptr(), per_launch.data_ptr(), 0, stream=raw), 16),
               "ptl_passes_to_gray16, depth": (lambda: pa.passes_to_gray16_device(records.data_ptr(), n_px, grey.data_ptr(), pa.PASS_DEPTH, 1.0, 7.5, stream=raw), 18),
               "ptl_passes_to_gray16, trips": (lambda: pa.passes_to_gray16_device(records.data_ptr(), n_px, grey.data_ptr(), pa.PASS_TRIPS, stream=raw), 18)}
    for name, ms_list in measure({k: v[0] for k, v in kernels.items()}, stream, torch, args.launches * 4, args.repeats).items():
        nbytes = kernels[name][1] * n_px
        report("kernel", name, ms_list, lambda ms: {"frame": f"{w}x{h}", "bytes": nbytes, "TB/s": round(nbytes / ms / 1e9, 3)})
    torch.cuda.synchronize()
    stats = block.cpu().numpy().view(pa.PASS_STATS_BLOCK)[0]
    print(json.dumps(dict(kind="frame", pixels_per_sweep=n_px, exhausted=int(stats["exhausted"]), paths=int(stats["paths"]), max_trips=int(stats["max_trips"]),
                          trips_per_pixel=round(int(stats["trips"]) / max(1, int(stats["pixels"])), 3), depth_range=pa.pass_stats_depth_range(np.array([stats])))), flush=True)
