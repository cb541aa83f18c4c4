#!/usr/bin/env python3
"""tools/pass_slices_bench.py -- what ptl_pass_slices_to_gray16 reaches, through the Python mirror of the C ABI.

Random records of a 3840x2160 frame, N = 1, 4, 16 slices, one output (depth) and all three, alternating in one session with
ptl_passes_to_gray16 (both conversions) and ptl_average_images (N = 4): warm-up, then `--launches` calls back to back between ONE pair of events,
`--repeats` times; median, min and max, and TB/s over the bytes the algorithm needs (16 N + 2 k per pixel; 18; 4 N + 4).  The kernel's
registers come from the code object's metadata.  One JSON line per cell.

    python tools/pass_slices_bench.py [--launches 200] [--repeats 7] [--size 3840x2160]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402
from tools.pass_bench import measure, report  # noqa: E402


def code_object_notes(name):
    """vgpr / sgpr / scratch / LDS of a helper code object, from its metadata (llvm-readelf of the ROCm the kernels were built with)."""
    path = os.path.join(os.path.dirname(pa.__file__), "kernels", name)
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        return {}
    text = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
    return {key: int(value) for key, value in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s+(\d+)", text)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    args = ap.parse_args()
    import torch

    if pa.device_count() < 1:
        sys.exit("pass_slices_bench: no HIP device visible (nothing is measured without one)")
    w, h = (int(v) for v in args.size.split("x"))
    n_px = w * h
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    raw = stream.cuda_stream
    print(json.dumps(dict(kind="code object", file="pass_slices_gray16.hsaco", **code_object_notes("pass_slices_gray16.hsaco"))), flush=True)
    print(json.dumps(dict(kind="code object", file="pass_gray16.hsaco", **code_object_notes("pass_gray16.hsaco"))), flush=True)
    # records as a clip's sub-frames leave them: finite depths, a few trips, four paths per pixel of which some are cut
    rng = np.random.default_rng(1)
    one = np.zeros(n_px, pa.PASS_RECORD)
    one["depth_near"] = rng.uniform(1.0, 7.5, n_px).astype(np.float32)
    one["trips"] = rng.integers(1, 40, n_px)
    exhausted = rng.integers(0, 5, n_px) * (rng.random(n_px) < 0.3)
    one["final_escaped"] = (4 - exhausted).astype(np.uint32)
    one["exhausted_outside"] = exhausted.astype(np.uint32)
    host = torch.from_numpy(one.view(np.uint8).reshape(-1).copy())
    records = torch.empty(16 * n_px * 16, dtype=torch.uint8, device=dev)
    for z in range(16):
        records[z * n_px * 16:(z + 1) * n_px * 16] = host.to(dev).roll(16 * 4099 * z)  # (every slice its own pixels)
    grey = [torch.empty(n_px * 2, dtype=torch.uint8, device=dev) for _ in range(3)]
    out8 = torch.empty(n_px * 4, dtype=torch.uint8, device=dev)
    subs = [torch.randint(0, 256, (n_px * 4,), dtype=torch.uint8, device=dev) for _ in range(4)]
    sub_ptrs = [s.data_ptr() for s in subs]
    cells = {"ptl_average_images, N = 4": (lambda: pa.average_images_device(sub_ptrs, out8.data_ptr(), w, h, stream=raw), 20),
             "ptl_passes_to_gray16, depth": (lambda: pa.passes_to_gray16_device(records.data_ptr(), n_px, grey[0].data_ptr(), pa.PASS_DEPTH, 1.0, 7.5, stream=raw), 18),
             "ptl_passes_to_gray16, trips": (lambda: pa.passes_to_gray16_device(records.data_ptr(), n_px, grey[1].data_ptr(), pa.PASS_TRIPS, stream=raw), 18)}
    for n_slices in (1, 4, 16):
        for k, outs in ((1, (grey[0].data_ptr(), 0, 0)), (3, tuple(g.data_ptr() for g in grey))):
            cells[f"ptl_pass_slices_to_gray16, N = {n_slices}, {k} output{'s' if k > 1 else ''}"] = (
                lambda n_slices=n_slices, outs=outs: pa.pass_slices_to_gray16_device(records.data_ptr(), n_slices, n_px, n_px, *outs, lo=1.0, hi=7.5, stream=raw), 16 * n_slices + 2 * k)
    for name, ms_list in measure({k: v[0] for k, v in cells.items()}, stream, torch, args.launches, args.repeats).items():
        nbytes = cells[name][1] * n_px
        report("kernel", name, ms_list, lambda ms: {"frame": f"{w}x{h}", "bytes": nbytes, "TB/s": round(nbytes / ms / 1e9, 3)})
