#!/usr/bin/env python3
"""tools/png_deflate_bench.py -- the GPU deflate of an 8-bit PNG frame (ptl_png_deflate_rgba8: ptl_png_deflate_bands_kernel and
ptl_png_deflate_pack_kernel, portal_amd/csrc/kernels/png_deflate.hip) beside ptl_average_images on the same card, through the C ABI.

Frames: a rendered one (scenes/portal_in_portal.ron, render depth 40, drawn on the card at the size asked for) and uniform noise.  Each cell:
warm-up launches, then `--launches` calls back to back between ONE pair of events, `--repeats` times, the kernels alternating; the median is
reported with the spread beside it.  A call of ptl_png_deflate_rgba8 is both kernels; their split is read from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/png_deflate_bench.py --launches 20 --repeats 1).  The stream of every frame is inflated
with zlib and compared with the frame's raw scanlines, and its size is printed beside zlib's at levels 1 and 3, with the SHA-256 of its 64-byte
header and its bytes (`stream_sha256`: two builds that agree on it wrote the same stream).  One JSON line per cell.
`--codes dynamic` measures ptl_png_deflate_rgba8_codes with a Huffman code per band (ptl_png_huffman_bands_kernel,
portal_amd/csrc/kernels/png_huffman.hip, and the same pack kernel) instead; `--codes fixed,dynamic` both, alternating in the one session.
`--depth 16` measures ptl_png_deflate_rgb48 (ptl_png_deflate16_bands_kernel, portal_amd/csrc/kernels/png_huffman.hip: matches at pixel distance, a code per band) on the
unfiltered 16-bit rows of the same draw's float frame (ptl_average_f32_to_rgb48 with PTL_PNG_FILTER_NONE, made on the card) and on 16-bit
noise, alternating with the 8-bit dynamic call on the draw's RGBA8 frame; beside the stream's size: zlib at levels 1 and 3 of the same Up
scanlines, and level 3 of the Sub scanlines the host encoder of --png-depth 16 deflates.

    python tools/png_deflate_bench.py [--launches 200] [--repeats 7] [--sizes 3840x2160] [--subframes 4] [--codes fixed|dynamic|fixed,dynamic] [--depth 8|16 [--scene portal_in_portal] [--render-depth 40]]
"""
import argparse
import hashlib
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


def raw_scanlines16(rows):
    """(H, 6 W) unfiltered rows -> the Up scanlines ptl_png_deflate_rgb48 deflates, and the Sub scanlines ptl_png_write_rgb48 is given."""
    h, n = rows.shape
    up = np.empty((h, n + 1), np.uint8)
    up[0, 0], up[1:, 0] = 0, 2
    up[0, 1:] = rows[0]
    up[1:, 1:] = rows[1:] - rows[:-1]
    sub = np.empty((h, n + 1), np.uint8)
    sub[:, 0] = 1
    sub[:, 1:7] = rows[:, :6]
    sub[:, 7:] = rows[:, 6:] - rows[:, :-6]
    return up.tobytes(), sub.tobytes()


def bench16(args, torch, dev, stream):
    """--depth 16: one JSON line per cell, the 16-bit call on the rendered frame and on noise, the 8-bit dynamic call on the same draw between them."""
    raw_stream = stream.cuda_stream
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = pa.Scene.from_file(pa.scene_path(args.scene))
        r = pa.SceneRenderer(scene, device=0)
        r.set_option("render_depth", args.render_depth)
        drawn = r.draw(w, h, rgba8=True, rgba32f=True)
        eight = torch.from_numpy(np.array(drawn["rgba8"])).to(dev)
        floats = torch.from_numpy(np.ascontiguousarray(np.array(drawn["rgba32f"]), np.float32)).to(dev)
        rows = {args.scene: torch.empty(pa.rgb48_frame_bytes(w, h), dtype=torch.uint8, device=dev),
                "noise": torch.from_numpy(np.random.default_rng(1).integers(0, 256, 6 * w * h, dtype=np.uint8)).to(dev)}
        pa.average_f32_to_rgb48_device([floats.data_ptr()], rows[args.scene].data_ptr(), w, h, pa.PNG_FILTER_NONE, stream=raw_stream)
        torch.cuda.synchronize()
        out16 = torch.empty(pa.png_stream16_bytes(w, h), dtype=torch.uint8, device=dev)
        out8 = torch.empty(pa.png_stream_bytes(w, h), dtype=torch.uint8, device=dev)
        kernels = {"ptl_png_deflate_rgba8_codes[dynamic]:" + args.scene: lambda: pa.png_deflate_rgba8_device(eight.data_ptr(), out8.data_ptr(), w, h, stream=raw_stream, codes=pa.PNG_CODES_DYNAMIC)}
        for name, t in rows.items():
            kernels["ptl_png_deflate_rgb48:" + name] = lambda t=t: pa.png_deflate_rgb48_device(t.data_ptr(), out16.data_ptr(), w, h, stream=raw_stream)
        sizes = {"ptl_png_deflate_rgba8_codes[dynamic]:" + args.scene: {"raw": h * (4 * w + 1)}}
        for name, t in rows.items():  # what the stream is, before anything is timed
            pa.png_deflate_rgb48_device(t.data_ptr(), out16.data_ptr(), w, h, stream=raw_stream)
            torch.cuda.synchronize()
            host = out16[:64].cpu().numpy().tobytes()
            magic, count, adler = struct.unpack("<I", host[0:4])[0], struct.unpack("<I", host[12:16])[0], struct.unpack("<I", host[16:20])[0]
            body = out16[64: 64 + count].cpu().numpy().tobytes()
            up, sub = raw_scanlines16(t.cpu().numpy().reshape(h, 6 * w))
            assert magic == 0x364C5450 and zlib.decompress(b"\x78\x01" + body + b"\x03\x00" + struct.pack(">I", adler)) == up, name
            sizes["ptl_png_deflate_rgb48:" + name] = {"raw": len(up), "stream": count, "zlib1": len(zlib.compress(up, 1)), "zlib3": len(zlib.compress(up, 3)), "zlib3_sub": len(zlib.compress(sub, 3)),
                                                      "stream_sha256": hashlib.sha256(host + body).hexdigest()}
        times = {name: [] for name in kernels}
        for launch in kernels.values():  # warm-up: code objects loaded, clocks up, every buffer touched
            for _ in range(20):
                launch()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, launch in kernels.items():
                time_launches(launch, stream, torch, args.launches, times[name])
        per_byte = {}
        for name in kernels:
            ms = float(np.median(times[name]))
            per_byte[name] = ms / sizes[name]["raw"]
            line = {"kernel": name, "frame": f"{w}x{h}", "launches": args.launches, "repeats": args.repeats, "ms": round(ms, 5), "ms_min": round(min(times[name]), 5),
                    "ms_max": round(max(times[name]), 5), "spread_%": round(100.0 * (max(times[name]) - min(times[name])) / ms, 2)}
            line.update(sizes[name])
            line["GB/s_of_raw"] = round(sizes[name]["raw"] / ms / 1e6, 1)
            if name.startswith("ptl_png_deflate_rgb48"):
                line["per_byte_vs_8bit_dynamic"] = round(per_byte[name] / per_byte["ptl_png_deflate_rgba8_codes[dynamic]:" + args.scene], 3)
                line["result_buffer_bytes"] = pa.png_stream16_bytes(w, h)
            print(json.dumps(line), flush=True)


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
    ap.add_argument("--scene", default="portal_in_portal", help="with --depth 16: the scene that is drawn")
    ap.add_argument("--render-depth", type=int, default=40, help="with --depth 16: its render depth")
    ap.add_argument("--depth", type=int, default=8, choices=(8, 16), help="16: ptl_png_deflate_rgb48 on the 16-bit rows of the same draw")
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
    if args.depth == 16:
        bench16(args, torch, dev, stream)
        sys.exit(0)
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
            sizes[label[mode] + name] = {"raw": len(raw), "stream": count, "zlib1": len(zlib.compress(raw, 1)), "zlib3": len(zlib.compress(raw, 3)),
                                         "stream_sha256": hashlib.sha256(host + body).hexdigest()}
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
