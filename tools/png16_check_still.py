#!/usr/bin/env python3
"""tools/png16_check_still.py -- is a still written by `portal-amd render-frame <scene> --png-depth 16` what the contract says?

The file is decoded with the tests' independent reader (tests/png16_reference.read_png16) and compared, pixel for pixel, with
yuv_deep_reference.encode16 of the float frame the Python mirror draws for the same state (the build render-frame uses: everything baked,
quick JIT; one sample per pixel unless --aa-count says otherwise); then ptl_png_read must open it and return the high bytes.

    portal_amd/portal-amd render-frame scenes/portal_in_portal.ron --width 3840 --height 2160 --render-depth 40 --png-depth 16 --output out.png
    python tools/png16_check_still.py out.png [--scene portal_in_portal] [--width 3840] [--height 2160] [--render-depth 40] [--aa-count 1]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402
from tests import png16_reference as pr  # noqa: E402
from tests import yuv_deep_reference as dr  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--scene", default="portal_in_portal")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--render-depth", type=int, default=40)
    ap.add_argument("--aa-count", type=int, default=1)
    args = ap.parse_args()
    if pa.device_count() < 1:
        sys.exit("png16_check_still: no HIP device visible (the frame to compare with is drawn on one)")
    w, h = args.width, args.height
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(args.scene)), device=0, flags=pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL | pa.FLAG_QUICK_JIT)
    r.set_option("aa_count", args.aa_count)
    r.set_option("render_depth", args.render_depth)
    r.set_option("view_angle", 90.0 / 180.0 * math.pi)
    r.update(0.0)
    want = dr.encode16([np.array(r.draw(w, h, rgba8=True, rgba32f=True)["rgba32f"])])
    image = pr.read_png16(args.path)
    print("still:", os.path.getsize(args.path), "bytes; pixels that differ from encode16:", int((image != want).any(axis=2).sum()), "of", w * h, "; distinct values:", len(np.unique(want)))
    opened = pa.png_read(args.path)
    print("ptl_png_read opens it:", opened.shape, "high bytes equal:", bool(np.array_equal(opened[..., :3], want >> 8)))
    sys.exit(0 if np.array_equal(image, want) and np.array_equal(opened[..., :3], want >> 8) else 1)
