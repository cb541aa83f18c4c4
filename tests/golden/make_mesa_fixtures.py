#!/usr/bin/env python3
"""tests/golden/make_mesa_fixtures.py -- OUTPUTS of the reference's shaders compiled and run by Mesa (llvmpipe).

Runs only where a Mesa software driver and the reference tree exist (`oracle.mesa.available()`); the tests need
neither, they read what this script stored under tests/golden/mesa/ (entries and checker: tests/mesa_pin.py):

  mesa/<case>.npz     the eleven frames of tests/reftext.py::FRAME_CASES; CPU reference: reference_text/<case>.npz
  mesa/corpus.npz     all corpus scenes, 32x18 at depth 12;                CPU reference: oracle.portal_oracle.Oracle
  mesa/random.npz     tests/test_scene_fuzz.py::random_scene, seeds 300..329, 40x24 at depth 10;  Oracle
  mesa/glsl.npz       tests/test_glsl_fuzz.py scenes, seeds 400..411, 192x12 at depth 2;           Oracle
  mesa/teleport.npz   the teleport query drawn into a real 2x3 RGBA8 target for the segments of
                      tests/reftext.py::teleport_segments, against reference_text/teleport.npz

Per frame entry: `mesa_bits` (Mesa's float frame), `listed` (flat indices of the pixels where the CPU reference is
beyond 1e-5 from Mesa on any channel; NaN on both sides is equal, on one side beyond) and `listed_bits` (the CPU
reference's bits there).  Every file carries GL_VERSION, GL_RENDERER and the digest of the reference's shader text.

  python tests/golden/make_mesa_fixtures.py            write the files
  python tests/golden/make_mesa_fixtures.py --check    regenerate into a temporary directory, compare bit for bit
"""
import os
import sys
import tempfile
import time
import warnings
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import mesa  # noqa: E402
from oracle import reference_shader as RS  # noqa: E402
from tests import mesa_pin as P  # noqa: E402
from tests import reftext as T  # noqa: E402

MAX_FILE_BYTES = 1_200_000
MAX_DIR_BYTES = 3_000_000


def frame_entry(job):
    family, name = job
    t0 = time.time()
    with tempfile.TemporaryDirectory() as scratch:
        shader, w, h = P.tracer(RS.ReferenceShader, family, name, scratch)
        try:
            frame = mesa.render(shader, w, h)
        except RuntimeError as e:  # Mesa refuses the text: reported at the end, the entry has to be excluded by name with that reason
            return family, name, None, str(e), time.time() - t0
        entry = P.make_entry(frame.view(np.uint32), P.cpu_reference_bits(family, name, scratch))
    return family, name, entry, mesa.gl_info(), time.time() - t0


def teleport_entry(scene):
    shader = RS.ReferenceShader(os.path.join(ROOT, "scenes", scene + ".ron"))
    raw = mesa.teleport_bytes(shader, T.teleport_segments(scene))
    decoded = np.array([[int(t), int(h), int(s), *pos] for t, h, s, pos in map(mesa.decode_teleport, raw)], np.uint32)
    flags, positions = P.unpack_reference_teleport(scene)
    flag_diff = np.flatnonzero((flags != decoded[:, :3].astype(bool)).any(axis=1)).astype(np.int32)
    same = np.setdiff1d(np.arange(len(raw)), flag_diff)
    distance = P.position_distance(positions[same], decoded[same, 3:6])
    return scene, {scene + ".bytes": raw, scene + ".decoded": decoded, scene + ".flag_diff": flag_diff, scene + ".distance": np.float64(distance)}, mesa.gl_info()


def generate(out_dir, workers):
    os.makedirs(out_dir, exist_ok=True)
    mesa.runner()  # built once, before the workers start
    jobs = [(family, name) for family in P.FAMILIES for name in P.names(family)]
    stores, info, refused = {}, None, []
    with ProcessPoolExecutor(max_workers=workers) as pool:
        teleports = [pool.submit(teleport_entry, scene) for scene in P.TELEPORT_SCENES]
        for family, name, entry, gl, seconds in pool.map(frame_entry, jobs, chunksize=1):
            if entry is None:
                refused.append(f"{family} {name}: {gl}")
                print(refused[-1], flush=True)
                continue
            info = gl
            store = stores.setdefault(P.family_file(family, name), {})
            for k, full in P.store_keys(family, name).items():
                store[full] = entry[k]
            h, w = entry["mesa_bits"].shape[:2]
            print(f"{family:7s} {name:44s} {w}x{h}  {seconds:6.1f} s  listed {len(entry['listed']):4d} of {w * h}", flush=True)
        tele = {}
        for f in teleports:
            scene, arrays, _ = f.result()
            tele.update(arrays)
            print(f"teleport {scene}: {len(arrays[scene + '.bytes'])} segments, flags differ on {list(arrays[scene + '.flag_diff'])}, "
                  f"position distance {float(arrays[scene + '.distance']):.3g}", flush=True)
        stores[os.path.join(P.MESA_DIR, "teleport.npz")] = tele
    stamp = dict(gl_version=np.array(info[0]), gl_renderer=np.array(info[1]), text_digest=np.array(RS.text_digest()))
    for path, store in stores.items():
        np.savez_compressed(os.path.join(out_dir, os.path.basename(path)), **store, **stamp)
    if refused:
        sys.exit("Mesa did not run these entries (find out why; only then exclude them in tests/mesa_pin.py):\n  " + "\n  ".join(refused))
    return info


def report(directory):
    total = 0
    for f in sorted(os.listdir(directory)):
        size = os.path.getsize(os.path.join(directory, f))
        total += size
        assert size <= MAX_FILE_BYTES, f"{f}: {size} bytes"
    assert total <= MAX_DIR_BYTES, f"{directory}: {total} bytes"
    print(f"{len(os.listdir(directory))} files, {total} bytes")
    for family in P.FAMILIES:
        listed = pixels = 0
        worst = (-1.0, "")
        for name in P.names(family):
            with np.load(os.path.join(directory, os.path.basename(P.family_file(family, name)))) as z:
                keys = P.store_keys(family, name)
                n, px = len(z[keys["listed"]]), z[keys["mesa_bits"]].shape[0] * z[keys["mesa_bits"]].shape[1]
            listed, pixels, worst = listed + n, pixels + px, max(worst, (n / px, name))
        print(f"{family}: {listed} of {pixels} pixels listed = {100 * listed / pixels:.3f} % (caps: entry {100 * P.CAPS[family][0]:g} %, family {100 * P.CAPS[family][1]:g} %); "
              f"largest entry {worst[1]} {100 * worst[0]:.2f} %; excluded: {', '.join(P.EXCLUDED[family]) or 'none'}")


def compare(fresh, committed):
    bad = []
    for f in sorted(set(os.listdir(fresh)) | set(os.listdir(committed))):
        if not (os.path.exists(os.path.join(fresh, f)) and os.path.exists(os.path.join(committed, f))):
            bad.append(f + ": only on one side")
            continue
        with np.load(os.path.join(fresh, f)) as a, np.load(os.path.join(committed, f)) as b:
            if set(a.files) != set(b.files):
                bad.append(f + ": other keys")
                continue
            for k in a.files:
                if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
                    bad.append(f"{f}: {k}")
    return bad


if __name__ == "__main__":
    if not mesa.available():
        sys.exit("no Mesa software driver (swrast_dri.so + libglapi.so.0) or no reference tree here")
    workers = max(1, min(8, (os.cpu_count() or 2) - 1))
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            info = generate(tmp, workers)
            report(tmp)
            bad = compare(tmp, P.MESA_DIR)
        print("GL:", *info)
        if bad:
            sys.exit("differs from the committed fixtures:\n  " + "\n  ".join(bad[:40]))
        print("check passed: every array equals the committed one bit for bit")
    else:
        info = generate(P.MESA_DIR, workers)
        report(P.MESA_DIR)
        print("GL:", *info)
