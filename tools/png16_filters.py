#!/usr/bin/env python3
"""tools/png16_filters.py -- what PNG's row filters do to a rendered 16-bit frame: bytes and deflate seconds per filter and level.

Two frames at 1920x1080 (scenes/portal_in_portal.ron at render depth 40, scenes/monoportal.ron at depth 20) are drawn on the GPU with
their float output.  None and Sub are the shipped path: ptl_average_f32_to_rgb48 makes the rows on the card, ptl_png_write_rgb48 writes
them at deflate levels 3 and 6; the file's size and the writer's wall time are reported, and the file is read back (ptl_png_read).  Up and
Paeth are not in the kernel: their rows are made here in numpy from the unfiltered rows and deflated with Python's zlib (the same library
the writer links), so that the Sub-versus-Up trade is stated on the same frames.  The RGBA8 frame of the same draw is there for scale.
One JSON line per cell.

    python tools/png16_filters.py [--width 1920] [--height 1080] [--out-dir DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402

FRAMES = (("portal_in_portal", 40), ("monoportal", 20))


def up(raw):
    out = raw.copy()
    out[1:] = raw[1:] - raw[:-1]  # uint8: mod 256
    return out


def paeth(raw, bpp):
    a = np.zeros(raw.shape, np.int32)
    a[:, bpp:] = raw[:, :-bpp]
    b = np.zeros(raw.shape, np.int32)
    b[1:] = raw[:-1]
    c = np.zeros(raw.shape, np.int32)
    c[1:, bpp:] = raw[:-1, :-bpp]
    p = a + b - c
    pa_, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    predictor = np.where((pa_ <= pb) & (pa_ <= pc), a, np.where(pb <= pc, b, c))
    return ((raw.astype(np.int32) - predictor) % 256).astype(np.uint8)


def deflated(rows, filter_type, level):
    """(H, stride) uint8 -> (bytes of the zlib stream of the scanlines behind their filter-type byte, seconds)"""
    lines = np.concatenate([np.full((rows.shape[0], 1), filter_type, np.uint8), rows], axis=1).tobytes()
    t0 = time.perf_counter()
    size = len(zlib.compress(lines, level))
    return size, time.perf_counter() - t0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    import torch

    if pa.device_count() < 1:
        sys.exit("png16_filters: no HIP device visible (the frames are drawn and filtered on one)")
    w, h = args.width, args.height
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="png16_filters_")
    os.makedirs(out_dir, exist_ok=True)
    for scene_name, depth in FRAMES:
        r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene_name)), device=0)
        r.set_option("render_depth", depth)
        r.update(0.0)
        drawn = r.draw(w, h, rgba8=True, rgba32f=True)
        floats = torch.from_numpy(np.ascontiguousarray(drawn["rgba32f"])).cuda()
        rows = {}
        for name, filter in (("none", pa.PNG_FILTER_NONE), ("sub", pa.PNG_FILTER_SUB)):
            out = torch.empty(pa.rgb48_frame_bytes(w, h), dtype=torch.uint8, device="cuda")
            pa.average_f32_to_rgb48_device([floats.data_ptr()], out.data_ptr(), w, h, filter, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            rows[name] = out.cpu().numpy()
            for level in (3, 6):
                path = os.path.join(out_dir, f"{scene_name}_{name}_l{level}.png")
                pa.png_write_rgb48(path, rows[name], w, h, filter, level)  # (first call of the thread: its scratch is allocated here)
                t0 = time.perf_counter()
                pa.png_write_rgb48(path, rows[name], w, h, filter, level)
                seconds = time.perf_counter() - t0
                assert pa.png_read(path).shape == (h, w, 4)
                print(json.dumps({"frame": f"{scene_name} d{depth} {w}x{h}", "format": "RGB 16 bit", "filter": name, "by": "ptl_average_f32_to_rgb48 + ptl_png_write_rgb48", "level": level,
                                  "MB": round(os.path.getsize(path) / 1e6, 3), "seconds": round(seconds, 3)}), flush=True)
        raw = rows["none"].reshape(h, 6 * w)
        for name, filter_type, made in (("up", 2, up(raw)), ("paeth", 4, paeth(raw, 6))):
            for level in (3, 6):
                size, seconds = deflated(made, filter_type, level)
                print(json.dumps({"frame": f"{scene_name} d{depth} {w}x{h}", "format": "RGB 16 bit", "filter": name, "by": "numpy + zlib.compress", "level": level, "MB": round(size / 1e6, 3),
                                  "seconds": round(seconds, 3)}), flush=True)
        raw8 = np.ascontiguousarray(drawn["rgba8"]).reshape(h, 4 * w)
        for name, filter_type, made in (("none", 0, raw8), ("up", 2, up(raw8))):
            for level in (3, 6):
                size, seconds = deflated(made, filter_type, level)
                print(json.dumps({"frame": f"{scene_name} d{depth} {w}x{h}", "format": "RGBA 8 bit", "filter": name, "by": "numpy + zlib.compress", "level": level, "MB": round(size / 1e6, 3),
                                  "seconds": round(seconds, 3)}), flush=True)
