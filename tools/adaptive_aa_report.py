#!/usr/bin/env python3
"""tools/adaptive_aa_report.py -- what adaptive anti-aliasing buys and what it costs, on the five BASELINE configs at
their own sizes with aa 4, for T in {2, 4, 8, 16}.  One JSON line per (config, T):
    refined share; unrefined pixels whose RGB is beyond 2 / beyond 8 codes of the full aa-4 frame, and the largest such difference;
    GPU ms of the classification alone, of the adaptive draw and of the full aa-4 draw.
Times: the adaptive draw and the full draw alternate in the same run; each figure is `--draws` draws between one pair of events on one
stream, the median of `--repeats` such batches, after a warm-up of both.  The classification alone is timed the same way on the
one-sample frame.
    python tools/adaptive_aa_report.py > profiles/r08/adaptive_aa.jsonl        # GPU box
    python tools/adaptive_aa_report.py --configs C4,C5 --thresholds 4"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portal_amd as pa  # noqa: E402

CONFIGS = {  # BASELINE.json, every one with aa 4 (C5 has it anyway)
    "C1": ("basics", 256, 256, 4),
    "C2": ("monoportal", 1920, 1080, 20),
    "C3": ("triple_portal", 3840, 2160, 40),
    "C4": ("portal_in_portal", 3840, 2160, 40),
    "C5": ("mobius_monoportal", 7680, 4320, 64),
}


def timed_batches(fn, draws, repeats):
    import torch

    stream = torch.cuda.current_stream()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(draws):
            fn(stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / draws)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3,C4,C5")
    ap.add_argument("--thresholds", default="2,4,8,16")
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import torch

    flags = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL | pa.FLAG_REFINE
    for config in args.configs.split(","):
        name, w, h, depth = CONFIGS[config]
        r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(name)), device=0, flags=flags)
        r.set_option("render_depth", depth)
        r.set_option("aa_count", 4)
        frame = pa.Frame(w, h, 0, 1, 0)
        full_dev = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        adaptive_dev = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        sync = torch.cuda.synchronize
        full = lambda s: r.draw_device(frame, out_rgba8=full_dev.data_ptr(), stream=s)  # noqa: E731
        adaptive = lambda s: r.draw_adaptive_device(frame, adaptive_dev.data_ptr(), stream=s)  # noqa: E731
        full(0)
        sync()
        want = full_dev.cpu().numpy()[:, :, :3].astype(np.int16)
        regs = {k: r.code_object_note(".vgpr_count", k) for k in ("ptl_render_kernel", "ptl_render_refine_kernel")}
        for t in [int(x) for x in args.thresholds.split(",")]:
            r.set_option("adaptive_aa_threshold", t)
            adaptive(0)
            sync()
            lst, cnt = r.adaptive_result()
            count = int(pa.device_download(cnt, 4).view(np.uint32)[0])
            got = adaptive_dev.cpu().numpy()[:, :, :3].astype(np.int16)
            refined = np.zeros(w * h, bool)
            if count:
                refined[pa.device_download(lst, count * 4).view(np.uint32)] = True
            err = np.abs(got - want).max(axis=2).reshape(-1)
            assert not err[refined].any(), "a refined pixel differs from the full frame"
            unrefined_err = err[~refined]
            # the classification alone, on the one-sample frame the adaptive draw leaves wherever it did not refine (T = 255: everywhere)
            r.set_option("adaptive_aa_threshold", 255)
            adaptive(0)
            sync()
            r.set_option("adaptive_aa_threshold", t)
            classify = lambda s: pa.aa_edges_device(adaptive_dev.data_ptr(), w, h, t, lst, cnt, stream=s)  # noqa: E731
            for fn in (full, adaptive, classify):  # warm-up of all three
                for _ in range(3):
                    fn(torch.cuda.current_stream().cuda_stream)
            sync()
            ms_full, ms_adaptive = [], []
            for _ in range(args.repeats):  # alternating, in the same run
                ms_adaptive += timed_batches(adaptive, args.draws, 1)
                ms_full += timed_batches(full, args.draws, 1)
            ms_classify = timed_batches(classify, args.draws, args.repeats)
            row = {"config": config, "scene": name, "size": f"{w}x{h}", "depth": depth, "aa": 4, "threshold": t, "refined": count,
                   "refined_share": round(count / (w * h), 5), "unrefined_beyond_2": int((unrefined_err > 2).sum()), "unrefined_beyond_8": int((unrefined_err > 8).sum()),
                   "unrefined_max": int(unrefined_err.max()) if unrefined_err.size else 0, "ms_classify": round(statistics.median(ms_classify), 4),
                   "ms_adaptive": round(statistics.median(ms_adaptive), 4), "ms_full": round(statistics.median(ms_full), 4), "draws": args.draws, "repeats": args.repeats,
                   "vgprs": regs, "code_object_sha256": r.code_object_sha256()}
            row["speedup"] = round(row["ms_full"] / row["ms_adaptive"], 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
