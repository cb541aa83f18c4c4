#!/usr/bin/env python3
"""tools/png_deflate_bench.py -- the GPU deflate of an 8-bit PNG frame (ptl_png_deflate_rgba8: ptl_png_deflate_bands_kernel and
ptl_png_deflate_pack_kernel, portal_amd/csrc/kernels/png_deflate.hip) beside ptl_average_images on the same card, through the C ABI.

Frames: a rendered one (scenes/portal_in_portal.ron, render depth 40, drawn on the card at the size asked for) and uniform noise.  Each cell:
warm-up launches, then `--launches` calls back to back between ONE pair of events, `--repeats` times, the kernels alternating; the median is
reported with the spread beside it.  A call of ptl_png_deflate_rgba8 is both kernels; their split is read from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/png_deflate_bench.py --launches 20 --repeats 1).  The stream of every frame is inflated
with zlib and compared with the frame's raw scanlines, and its size is printed beside zlib's at levels 1 and 3.  One JSON line per cell.
`--codes dynamic` measures ptl_png_deflate_rgba8_codes with a Huffman code per band (ptl_png_huffman_bands_kernel,
portal_amd/csrc/kernels/png_huffman.hip, and the same pack kernel) instead; `--codes fixed,dynamic` both, alternating in the one session.

    python tools/png_deflate_bench.py [--launches 200] [--repeats 7] [--sizes 3840x2160] [--subframes 4] [--codes fixed|dynamic|fixed,dynamic]
"""
import argparse
import json
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402


def raw_scanlines(frame):
    h, w = frame.shape[:2]
    rows = frame.reshape(h, 4 * w)
    out = np.empty((h, 4 * w + 1), np.uint8)
    out[0, 0], out[1:, 0] = 0, 2
    out[0, 1:] = rows[0]
    out[1:, 1:] = rows[1:] - rows[:-1]
    return out.tobytes()


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
    ap.add_argument("--subframes", type=int, default=4)
    ap.add_argument("--codes", default="fixed", help="fixed, dynamic, or both separated by a comma")
    args = ap.parse_args()
    modes = args.codes.split(",")
    if not modes or any(m not in ("fixed", "dynamic") for m in modes) or len(set(modes)) != len(modes):
        sys.exit("png_deflate_bench: --codes fixed|dynamic|fixed,dynamic")
    CODES = {"fixed": pa.PNG_CODES_FIXED, "dynamic": pa.PNG_CODES_DYNAMIC}
    label = {"fixed": "ptl_png_deflate_rgba8:", "dynamic": "ptl_png_deflate_rgba8_codes[dynamic]:"}
    import torch

    if pa.device_count() < 1:
        sys.exit("png_deflate_bench: no HIP device visible (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    raw_stream = stream.cuda_stream
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
        r = pa.SceneRenderer(scene, device=0)
        r.set_option("render_depth", 40)
        rendered = np.array(r.draw(w, h, rgba8=True)["rgba8"])
        frames = {"portal_in_portal": rendered, "noise": np.random.default_rng(1).integers(0, 256, (h, w, 4), dtype=np.uint8)}
        n = args.subframes
        subs = [torch.from_numpy(np.roll(rendered, k, axis=1).copy()).to(dev) for k in range(n)]
        averaged = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        out = torch.empty(pa.png_stream_bytes(w, h), dtype=torch.uint8, device=dev)
        staged = {name: torch.from_numpy(f).to(dev) for name, f in frames.items()}
        kernels = {f"ptl_average_images:n={n}": lambda: pa.average_images_device([s.data_ptr() for s in subs], averaged.data_ptr(), w, h, stream=raw_stream)}
        for name, t in staged.items():
            for mode in modes:
                kernels[label[mode] + name] = lambda t=t, mode=mode: pa.png_deflate_rgba8_device(t.data_ptr(), out.data_ptr(), w, h, stream=raw_stream, codes=CODES[mode])
        sizes = {}
        for name, t, mode in [(name, t, mode) for name, t in staged.items() for mode in modes]:  # what the stream is, before anything is timed
            pa.png_deflate_rgba8_device(t.data_ptr(), out.data_ptr(), w, h, stream=raw_stream, codes=CODES[mode])
            torch.cuda.synchronize()
            host = out[:64].cpu().numpy().tobytes()
            count, adler = struct.unpack("<I", host[12:16])[0], struct.unpack("<I", host[16:20])[0]
            body = out[64: 64 + count].cpu().numpy().tobytes()
            raw = raw_scanlines(frames[name])
            assert zlib.decompress(b"\x78\x01" + body + b"\x03\x00" + struct.pack(">I", adler)) == raw, name
            sizes[label[mode] + name] = {"raw": len(raw), "stream": count, "zlib1": len(zlib.compress(raw, 1)), "zlib3": len(zlib.compress(raw, 3))}
        times = {name: [] for name in kernels}
        for launch in kernels.values():  # warm-up: code objects loaded, clocks up, every buffer touched
            for _ in range(20):
                launch()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, launch in kernels.items():
                time_launches(launch, stream, torch, args.launches, times[name])
        for name in kernels:
            ms = float(np.median(times[name]))
            line = {"kernel": name, "frame": f"{w}x{h}", "launches": args.launches, "repeats": args.repeats, "ms": round(ms, 5), "ms_min": round(min(times[name]), 5),
                    "ms_max": round(max(times[name]), 5), "spread_%": round(100.0 * (max(times[name]) - min(times[name])) / ms, 2)}
            if name.startswith("ptl_average_images"):
                line["TB/s"] = round((4 * n + 4) * w * h / ms / 1e9, 3)
            else:
                s = sizes[name]
                line.update(s)
                line["GB/s_of_raw"] = round(s["raw"] / ms / 1e6, 1)
                line["result_buffer_bytes"] = pa.png_stream_bytes(w, h)
            print(json.dumps(line), flush=True)
