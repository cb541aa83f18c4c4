#!/usr/bin/env python3
"""bench.py -- Mray/s and ms/frame of the portal trace kernel on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it is launched by
torch.distributed.run with one rank per GPU.  A "step" is one full frame of the headline
workload (BASELINE.json: scenes/portal_in_portal.ron, 3840x2160, aa 1, depth 40): every rank
renders its interleaved row blocks (no data-path collective while tracing) and the image is
assembled on rank 0 -- by ONE gather of the RGBA8 shards over RCCL plus a de-interleave copy, or
by the kernels storing straight into rank 0's frame over xGMI (whichever is faster here).  Inputs
(scene constants, portal matrices) are resident in device constant memory before the timed
region; the frame stays in HBM (no host copy inside the timed region).

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel (ptl_render_kernel).  The kernel is FP32-VALU-bound
(~10^3 flop per framebuffer byte), so `roofline.bound` is "valu".  Round 5: `frac` = min(count, hw_arith_frac).
  count          the oracle's ray-dependent binary32 operations per bounce-loop trip that the timed build still performs (tools/count_flops.py ->
                 profiles/r05/flops_per_segment.json: a >= 1 % pixel sample of THIS full-size frame; minus culled plane tests, zero / unit matrix
                 terms and, with affine rays, the terms that meet a ray's w) x the trips of this launch (counted on the GPU) / the kernel's mean
                 launch time (HIP events on the launch stream);
  hw_arith_frac  (2 x FMA + MUL + ADD + transcendental wave-instructions) x 64 x lane utilisation / time / peak from the committed rocprofv3 PMC
                 passes OF THE CODE OBJECT THAT WAS TIMED: the line carries the sha256 of that binary (`config.code_object_sha256`), every
                 profiles/r05/pmc_*.json the sha256 of the binary it counted, and a file of another binary is refused (`pmc_unavailable`).
`roofline.traffic` = HBM bytes per launch from the FETCH_SIZE / WRITE_SIZE passes of the same file.  `roofline_hbm` is the framebuffer store (4 B/pixel)
against HBM peak: tiny by construction.  `cpu_baseline` times the same generated source compiled for the host (oracle/host_build.py, "port") on a
bounded sample.  `workloads`: every other BASELINE.json config, the Panini variant and two deep views, each timed and checked the same way (N = 1).
`python bench.py --gpus N` without a launcher starts its own N ranks (torch.distributed.run, 127.0.0.1).

A plain run (no `--full`) does only what the headline needs: set-up (candidate builds, the fastest kept), warm-up, the K timed steps and the
line (`metric`, `value`, `unit`, `ms_per_step`, `higher_is_better`, `dtype`, ...).  `--full` adds everything else described above: the kernel's
own launch time and rooflines, the trip count, C5 and the other workloads, CPU baselines, the checker's verdicts, the other builds, the
peer transports at N > 1 and the detail record (`bench_detail.json`).  `--dump-outputs DIR` writes the frame of the last timed step as
float32 `.npy` files (the whole RGBA8 frame, or a fixed seeded sample of its pixels when the frame is larger than 64 MB as float32).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: peak FP32 vector



def scene_of(args, pa):
    """(path, SceneRenderer keyword arguments) of the workload's scene file"""
    if args.scene_file:
        path = os.path.join(HERE, args.scene_file)
        return path, {"asset_root": os.path.dirname(os.path.dirname(path))}
    return pa.scene_path(args.scene), {}


def workload_key(args):
    key = f"{args.scene}_{args.width}x{args.height}_d{args.depth}" + (f"_aa{args.aa}" if args.aa != 1 else "")
    if args.camera:
        key += "_cam" + args.camera.replace(",", "_")
    if args.panini >= 0.0:
        key += "_panini" if (args.panini == 1.0 and args.fov == 140.0) else f"_panini{args.panini}_fov{args.fov}"
    elif args.fov != 90.0:
        key += f"_fov{args.fov}"
    return key


PROFILE_ROUNDS = ("r06", "r05", "r04", "r03")  # newest first; a round's files are measurements of that round's kernels


def source_sha256(renderer):
    """sha256 of the generated kernel source the renderer's current build was compiled from: the candidate builds of one workload (w0 ... w5, minreg) share
    it -- they differ in the register budget / scheduler handed to the compiler, not in a single operation of the program."""
    import hashlib

    return hashlib.sha256(renderer.kernel_source().encode("utf-8")).hexdigest()


def stored_pmc(args, build, code_sha=None, source_sha=None):
    """The committed rocprofv3 PMC passes of exactly this workload (profiles/rNN/pmc_<workload>_<spec>_<build>.json, one counter group per
    pass, tools/collect_pmc.sh): HBM bytes per launch (FETCH_SIZE doubled per the gfx950 note in MI355X_MICROARCH.md, + WRITE_SIZE, KB units),
    SQ_INSTS_VALU and the instruction classes per launch.  Round 5: a PMC file names the sha256 of the code object whose launches it counted
    (`code_object_sha256`, written by tools/collect_pmc.sh from the bench line of the counted run); with `code_sha` given -- the timed build's
    -- only a file of the SAME binary is used.  Returns (counters or None, why not)."""
    import glob

    spec = {0: "dynamic", 1: "ints", 2: "spec"}[args.specialize]
    dirs = ([os.environ["PTL_PMC_DIR"]] if os.environ.get("PTL_PMC_DIR") else []) + [os.path.join(HERE, "profiles", rnd) for rnd in PROFILE_ROUNDS]
    refused = []
    for d in dirs:  # (PTL_PMC_DIR: passes collected a moment ago on this very box)
        base = os.path.join(d, f"pmc_{workload_key(args)}_{spec}_")
        paths = [base + build + ".json"] + sorted(p for p in glob.glob(base + "*.json") if p != base + build + ".json" and os.path.basename(p)[len(os.path.basename(base)):-5] in ("w0", "w3", "w4", "w5", "minreg"))
        for path in paths:
            try:
                doc = json.load(open(path))
                c = doc["counters"]
                match = "code object"
                if code_sha is not None and doc.get("code_object_sha256") != code_sha:
                    # round 6: ... or of another register budget of the SAME generated source (`kernel_source_sha256` in the file and in the line): the
                    # same program, the same arithmetic; the pick among candidates a per cent apart then no longer decides whether counters exist
                    if source_sha is not None and doc.get("kernel_source_sha256") == source_sha:
                        match = "same kernel source, another register budget"
                    else:
                        refused.append(f"{os.path.relpath(path, HERE)}: counted code object {str(doc.get('code_object_sha256'))[:16]}, timed {code_sha[:16]}")
                        continue
                out = {"traffic": int((2 * c["FETCH_SIZE"]["mean_per_launch"] + c["WRITE_SIZE"]["mean_per_launch"]) * 1024), "match": match,
                       "kernel_source_sha256": doc.get("kernel_source_sha256"),
                       "insts_valu": float(c["SQ_INSTS_VALU"]["mean_per_launch"]), "source": os.path.relpath(path, HERE), "code_object_sha256": doc.get("code_object_sha256")}
                classes = ("SQ_INSTS_VALU_FMA_F32", "SQ_INSTS_VALU_MUL_F32", "SQ_INSTS_VALU_ADD_F32", "SQ_INSTS_VALU_TRANS_F32", "SQ_INSTS_VALU_INT32", "GRBM_GUI_ACTIVE")
                if all(k in c for k in classes):
                    out["classes"] = {k: float(c[k]["mean_per_launch"]) for k in classes}
                if "SQ_THREAD_CYCLES_VALU" in c and "SQ_ACTIVE_INST_VALU" in c:  # lanes active per issued VALU instruction
                    out["lane_utilisation"] = float(c["SQ_THREAD_CYCLES_VALU"]["mean_per_launch"]) / (64.0 * float(c["SQ_ACTIVE_INST_VALU"]["mean_per_launch"]))
                return out, None
            except Exception:
                continue
    return None, ("; ".join(refused) if refused else "no stored PMC passes of this workload")


def flops_per_segment(args, affine=False):
    """Binary32 operations per bounce-loop trip (fma = 2) on a pixel sample of this full-size frame (tools/count_flops.py):
    (`flops_varying`, the ray-dependent ones, when the timed kernel has every scene uniform baked in and so folds the rest;
    `flops`, all of them, for a kernel that reads the uniforms at run time).  Data file only."""
    entry = source = None
    for rnd in PROFILE_ROUNDS:
        try:
            entry = json.load(open(os.path.join(HERE, "profiles", rnd, "flops_per_segment.json")))[workload_key(args)]
            source = f"profiles/{rnd}/flops_per_segment.json"
            break
        except Exception:
            continue
    if entry is None:
        return None
    # Ray-dependent operations only, for every build: a specialised build folds the uniform-only ones at JIT time; the others get most of
    # them from the prologue kernel (derived plane normals, glsl_hoist.h) -- what is left of them per ray is executed but NOT counted.
    which = "flops_varying"
    algorithmic = float(entry["per_segment"][which])
    # the translator defers loop-carried ray transforms nobody reads (glsl_translate.h): the kernel does not execute them, so they
    # are not counted as achieved work either (`..._executed`, tools/count_flops.py)
    executed = float(entry["per_segment"].get(which + "_executed", algorithmic))
    label = which + ("_executed" if executed != algorithmic else "")
    # ... and with the scene's matrices baked into the source (--specialize 2) a matrix product skips the terms whose matrix element is
    # zero (device/ptl_glsl.h `ptl_mterm`): counted by the oracle (`zero_term_flops_varying`) and taken off as well
    if args.specialize == 2 and not (args.extra_flags & 16384) and "flops_varying_executed_baked" in entry["per_segment"]:
        executed, label = float(entry["per_segment"]["flops_varying_executed_baked"]), "flops_varying_executed_baked"
        # round 5: neither the multiplications by +-1 matrix elements (one add each) nor -- in a kernel with affine rays -- the terms that
        # meet a ray's w (tools/count_flops.py: `unit_term`, `known_w_term`)
        want = "flops_varying_executed_baked_affine" if affine else "flops_varying_executed_baked_units"
        if want in entry["per_segment"]:
            executed, label = float(entry["per_segment"][want]), want
    # Comparisons are not claimed: the oracle tallies a compare as one operation, but a v_cmp is not a floating-point operation of the peak
    # this is priced against (round 3's count, with them, sat 2-3 % above the hardware's own instruction ceiling).
    compares = float(entry["per_segment"].get("cmp_varying", 0.0))
    return {"flops": max(0.0, executed - compares), "which": label + " - cmp_varying", "algorithmic": algorithmic, "with_compares": executed, "compares": compares,
            "sampled_pixels": entry["sampled_pixels"], "sampled_fraction_of_frame": entry["sampled_fraction_of_frame"],
            "all_flops": float(entry["per_segment"]["flops"]), "source": source}


WORKLOADS = {  # --workload NAME: BASELINE.json configs by name
    "c2": dict(scene="monoportal", width=1920, height=1080, depth=20, aa=1),
    "c3": dict(scene="triple_portal", width=3840, height=2160, depth=40, aa=1),
    "c4": dict(scene="portal_in_portal", width=3840, height=2160, depth=40, aa=1),
    "c5": dict(scene="mobius_monoportal", width=7680, height=4320, depth=64, aa=4),  # the divergent-ray stress config: ~13 ms per frame on one GPU
    # the deep-recursion regime the wave-level early-out exists for: the headline scene seen INTO the nested portals
    # (the views tests/test_gpu_oracle_fullsize.py checks at 320x180), and the corpus scene with four nested chains
    "c4-deep": dict(scene="portal_in_portal", width=3840, height=2160, depth=40, aa=1, camera="0,0,0,0.2,1.5,1.6"),
    "c4-deep2": dict(scene="portal_in_portal", width=3840, height=2160, depth=40, aa=1, camera="0.3,-0.1,0.2,2.8,1.0,2.4"),
    # the corpus scene whose default view takes 26 trips per primary ray at depth 40 (a room that contains itself): the one BASELINE-sized workload in
    # which "depth = 40" is what the frame costs (the five BASELINE views take 1.02-1.11 trips per ray)
    "recursive-room": dict(scene="recursive_room", scene_file="tests/corpus/scenes/recursive_room.ron", width=3840, height=2160, depth=40, aa=1),
    "plus-ultra": dict(scene="portal_in_portal_plus_ultra", scene_file="tests/corpus/scenes/portal_in_portal_plus_ultra.ron", width=3840, height=2160, depth=40, aa=1),
}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=400)   # 400 x 0.6 ms: a quarter of a second of timed region (20 steps = 13 ms were invisible
    p.add_argument("--warmup", type=int, default=20)   # to a once-per-second utilisation sampler)
    p.add_argument("--workload", default="", choices=[""] + sorted(WORKLOADS), help="a BASELINE.json config by name (c4 = the headline = the default; "
                   "c5 = mobius_monoportal 8K aa 4 depth 64, the second scaling workload: its per-rank trace stays far above collective latency at 8 GPUs)")
    p.add_argument("--scene", default="portal_in_portal")
    p.add_argument("--scene-file", default="", help="a .ron file outside scenes/ (repo-relative); its assets are looked up beside its `scenes` directory")
    p.add_argument("--camera", default="", help="look_at x,y,z,alpha,beta,r instead of the scene's `cam` block")
    p.add_argument("--width", type=int, default=3840)
    p.add_argument("--height", type=int, default=2160)
    p.add_argument("--depth", type=int, default=40)
    p.add_argument("--aa", type=int, default=1)
    p.add_argument("--panini", type=float, default=-1.0, help="Panini d parameter (enables the projection); fov via --fov")
    p.add_argument("--fov", type=float, default=90.0)
    p.add_argument("--specialize", type=int, default=2, help="JIT specialisation: 0 none, 1 bake Bool/Int scene uniforms, 2 bake all scene uniforms")
    p.add_argument("--waves", type=int, default=-1, help="occupancy hint (__launch_bounds__(256, n)); -1 = pick the fastest candidate build before timing")
    p.add_argument("--build", default="", help="pin one candidate build by name (w0, w3, w4, w5, minreg) instead of picking the fastest")
    p.add_argument("--extra-flags", type=int, default=0, help="extra SceneRenderer flag bits for A/B measurements (e.g. 16384 = FLAG_EXACT_CR, the round-2 numerics contract)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-second-workload", action="store_true", help="skip the C5 frames that follow the headline's timed region (`second_workload` in the JSON line)")
    p.add_argument("--no-segments", action="store_true", help="skip the trip-counting launch after the timed region (PMC passes: the last launches of "
                   "ptl_render_kernel are then exactly the timed ones)")
    p.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU time of the cpu_baseline sample")
    p.add_argument("--save-png", default="")
    p.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline (rooflines, other workloads and builds, "
                   "CPU baselines, oracle checks, peer transports) and write the detail record; a plain run times the headline only")
    p.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (float32)")
    p.add_argument("--lanes", type=int, default=2, help="frames in flight in the timed region at ONE GPU: consecutive frames go to alternating internal streams of the "
                   "renderer (options concurrent_draws K + lane_fence 0), a target per lane, joined at the end; 1 = one stream, one frame at a time (rounds 1-5)")
    args = p.parse_args()
    for k, v in WORKLOADS.get(args.workload, {}).items():
        setattr(args, k, v)
    return args


def cpu_baseline(args, pa):
    """The host build of the same generated kernel, timed on a bounded sample of the same frame:
    every `stride`-th 8-row block (so cheap and expensive image regions are both sampled)."""
    from oracle import host_build as hb

    scene_path, extra = scene_of(args, pa)
    scene = pa.Scene.from_file(scene_path)
    ref = pa.SceneRenderer(scene, device=-1, **extra)
    configure(ref, args)
    hk = hb.host_kernel_for(ref, scene, args.width, args.height, **extra)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    blocks = (args.height + 7) // 8

    def rows_of(block_ids):
        return np.concatenate([np.arange(8 * b, min(args.height, 8 * b + 8)) for b in block_ids]).astype(np.int32)

    # calibrate on 2*cores rows spread over the frame, then size the sample for ~cpu_seconds
    calib = rows_of(range(0, blocks, max(1, blocks // max(1, cores // 4))))
    t0 = time.perf_counter()
    hk.render(args.width, args.height, rows=calib, threads=cores, rgba32f=False)
    per_row = max(time.perf_counter() - t0, 1e-4) / len(calib)
    n_blocks = int(max(cores // 8 + 1, min(blocks, args.cpu_seconds / (per_row * 8))))
    stride = max(1, blocks // n_blocks)
    picked = list(range(0, blocks, stride))
    rows = rows_of(picked)
    reps = int(max(1, min(64, round(args.cpu_seconds / max(per_row * len(rows), 1e-3)))))  # fast hosts: repeat the sample
    t0 = time.perf_counter()
    for _ in range(reps):
        hk.render(args.width, args.height, rows=rows, threads=cores, rgba32f=False)
    dt = time.perf_counter() - t0
    rays = reps * len(rows) * args.width * args.aa
    return {
        "value": round(rays / dt / 1e6, 4),
        "unit": "Mray/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{reps} x {len(picked)} of {blocks} 8-row blocks (every {stride}th) of the {args.width}x{args.height} frame, "
                  f"{rays} primary rays in {dt:.2f} s, same generated source (dynamic uniforms) built with g++ -O2 -ffp-contract=off -mfma -fopenmp",
    }


def reference_text_baseline(args, pa, seconds=8.0, keep=None):
    """A second CPU figure that does not move when the product's translator improves: the reference's OWN shader text
    (oracle/reference_shader.py: library.glsl + frag.glsl with the generated slots, executed by the numpy GLSL interpreter, one core) on a
    seeded pixel sample of the same frame.  `kind: reference` -- the nearest thing to the reference's path that runs on a CPU at all."""
    import zlib

    from oracle import reference_shader as RS

    if not RS.available():
        return {"error": "reference shader text not present (oracle/_ref/reference_shader.bin: __graft_entry__.build() where /root/reference is mounted)"}
    scene_path, extra = scene_of(args, pa)
    o = RS.ReferenceShader(scene_path, **extra)
    o.options.update(render_depth=args.depth, aa_count=args.aa, view_angle=args.fov / 180.0 * np.pi)
    if args.panini >= 0.0:
        o.options.update(use_panini=True, panini_param=args.panini)
    if args.camera:
        c = [float(x) for x in args.camera.split(",")]
        o.camera = dict(look_at=tuple(c[:3]), alpha=c[3], beta=c[4], r=c[5])
    rng = np.random.default_rng(zlib.crc32(args.scene.encode()) + 7)
    n, done, t0 = 4096, 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        xs, ys = rng.integers(0, args.width, n), rng.integers(0, args.height, n)
        shaded = o.shade_pixels(args.width, args.height, xs, ys)
        if keep is not None:  # the colours are the reference text's answer for these pixels: reference_text_check compares them with the timed build's frame
            keep.append((xs, ys, shaded["rgba32f"], shaded["rgba8"]))
        done += n
    dt = time.perf_counter() - t0
    return {"value": round(done * args.aa / dt / 1e6, 5), "unit": "Mray/s", "cores": 1, "kind": "reference",
            "sample": f"{done} seeded pixels of the {args.width}x{args.height} frame in {dt:.1f} s: /root/reference/src/library.glsl + frag.glsl (text digest {RS.text_digest()}) "
                      "with the slots of scene.rs:693-1075, interpreted by oracle/glsl_interp.py on numpy lanes, single thread"}


def reference_text_check(args, pa, renderer, torch, dev, stream, kept):
    """The parity chain closed directly: the frame the TIMED renderer draws against the colours the reference's own shader text
    (/root/reference/src/frag.glsl:106-159,515-551 + library.glsl, executed by oracle/reference_shader.py) gave for the seeded pixels
    reference_text_baseline shaded -- float bits and RGBA8.  No hand oracle in between."""
    W, H = args.width, args.height
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    renderer.draw_device(pa.Frame(W, H, 0, 1), out_rgba8=u8.data_ptr(), out_rgba32f=f32.data_ptr(), stream=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    xs, ys = np.concatenate([k[0] for k in kept]), np.concatenate([k[1] for k in kept])
    want32, want8 = np.concatenate([k[2] for k in kept]), np.concatenate([k[3] for k in kept])
    sel = torch.as_tensor(ys * W + xs, device=dev)
    got32 = f32.view(-1, 4)[sel].cpu().numpy()
    got8 = u8.view(-1, 4)[sel].cpu().numpy()
    same = ((got32.view(np.uint32) == want32.view(np.uint32)) | (np.isnan(got32) & np.isnan(want32))).all(axis=1)
    ok8 = (got8 == want8).all(axis=1)
    err = np.abs(got32[:, :3].astype(np.float64) - want32[:, :3].astype(np.float64))
    return {"pixels": int(len(xs)), "float_bits_equal": int(same.sum()), "rgba8_equal": int(ok8.sum()), "bit_exact": bool(same.all() and ok8.all()),
            "max_abs_error": float(np.nanmax(err)) if len(err) else 0.0,
            "checker": "oracle/reference_shader.py: the reference's library.glsl + frag.glsl text, slots as scene.rs:693-1075 prints them, run by oracle/glsl_interp.py"}


def contract_distance(args, pa, torch, dev, stream, local_rank, spec_flags, workloads):
    """How far numerics contract 2 (the shipped default: 1/x and sqrt correctly rounded with the extremes flushed, a / b = a * (1/b)) sits
    from the IEEE evaluation (contract 1, FLAG_EXACT_CR: correctly rounded / and sqrt on every input) on whole BASELINE frames: the north
    star's bar is 1e-5 per channel against a CPU evaluation, so the cost of the contract is a number here, not an anecdote."""
    out = {}
    for key, w in workloads.items():
        scene = pa.Scene.from_file(pa.scene_path(w["scene"]))
        W, H = w["width"], w["height"]
        f32 = torch.empty((2, H, W, 4), dtype=torch.float32, device=dev)
        u8 = torch.empty((2, H, W, 4), dtype=torch.uint8, device=dev)
        ms = []
        for k, flags in enumerate((spec_flags, spec_flags | pa.FLAG_EXACT_CR)):
            r = pa.SceneRenderer(scene, device=local_rank, flags=flags)
            r.set_option("render_depth", w["depth"])
            r.set_option("aa_count", w["aa"])
            r.draw_device(pa.Frame(W, H, 0, 1), out_rgba8=u8[k].data_ptr(), out_rgba32f=f32[k].data_ptr(), stream=stream.cuda_stream)
            ms.append(float(np.median([r.draw_device(pa.Frame(W, H, 0, 1), out_rgba8=u8[k].data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(5)])))
            del r
        torch.cuda.synchronize(dev)
        err = (f32[0, :, :, :3] - f32[1, :, :, :3]).abs().amax(dim=2)
        err = torch.nan_to_num(err, nan=0.0)
        differ = (f32[0].view(torch.int32) != f32[1].view(torch.int32)).any(dim=2)
        out[key] = {"workload": f"scenes/{w['scene']}.ron {W}x{H} aa={w['aa']} depth={w['depth']}", "pixels": W * H,
                    "pixels_with_other_bits": int(differ.sum().item()), "pixels_beyond_1e-5": int((err > 1e-5).sum().item()),
                    "rgba8_pixels_differing": int((u8[0] != u8[1]).any(dim=2).sum().item()),
                    "max_abs_error": float(err.max().item()), "median_abs_error": float(err.median().item()),
                    "kernel_ms_contract2": round(ms[0], 4), "kernel_ms_contract1": round(ms[1], 4)}
        del f32, u8
    out["note"] = ("contract 2 (timed) against contract 1 = IEEE correctly rounded / and sqrt on every input (FLAG_EXACT_CR, `--exact-cr`), same scene, same build "
                   "otherwise; pixels beyond 1e-5 are pixels where a last-bit difference decides a path (object and portal edges)")
    return out


def oracle_check(args, pa, renderer, torch, dev, stream, n=2048):
    """The checker's verdict on the binary that was TIMED (cpu_baseline leg, outside the timed region): the frame this very
    renderer draws, at 2 x n seeded pixels of the full-size frame -- n uniform, n on colour discontinuities (portal rims, object
    edges: where one ulp flips a path) -- against the numpy oracle (oracle/portal_oracle.py), float bits and RGBA8."""
    import zlib

    from oracle.portal_oracle import Oracle

    W, H = args.width, args.height
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    renderer.draw_device(pa.Frame(W, H, 0, 1), out_rgba8=u8.data_ptr(), out_rgba32f=f32.data_ptr(), stream=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    img = u8.cpu().numpy()
    c = img[..., :3].astype(np.int16)
    e = np.zeros(c.shape[:2], bool)
    dx = np.abs(c[:, 1:] - c[:, :-1]).max(axis=2) > 24
    dy = np.abs(c[1:, :] - c[:-1, :]).max(axis=2) > 24
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:, :] |= dy
    e[:-1, :] |= dy
    edges = np.argwhere(e)
    rng = np.random.default_rng(zlib.crc32(args.scene.encode()) + 20260926)
    ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
    if len(edges):
        pick = edges[rng.choice(len(edges), size=n, replace=len(edges) < n)]
        ys, xs = np.concatenate([ys, pick[:, 0]]), np.concatenate([xs, pick[:, 1]])
    scene_path, extra = scene_of(args, pa)
    o = Oracle(scene_path, **extra)
    o.options.update(render_depth=args.depth, aa_count=args.aa, view_angle=args.fov / 180.0 * np.pi)
    if args.camera:
        c = [float(x) for x in args.camera.split(",")]
        o.camera = dict(look_at=tuple(c[:3]), alpha=c[3], beta=c[4], r=c[5])
    if args.panini >= 0.0:
        o.options.update(use_panini=True, panini_param=args.panini)
    t0 = time.perf_counter()
    want = o.shade_pixels(W, H, xs, ys)
    sel = torch.as_tensor(ys * W + xs, device=dev)
    got32 = f32.view(-1, 4)[sel].cpu().numpy()
    same = (got32.view(np.uint32) == want["rgba32f"].view(np.uint32)) | (np.isnan(got32) & np.isnan(want["rgba32f"]))
    ok8 = (img[ys, xs] == want["rgba8"]).all(axis=1)
    return {"pixels": int(len(ys)), "on_colour_edges": int(len(ys) - n), "float_bits_equal": int(same.all(axis=1).sum()), "rgba8_equal": int(ok8.sum()),
            "bit_exact": bool(same.all() and ok8.all()), "max_trips_in_sample": int(want["segments"].max()), "oracle_seconds": round(time.perf_counter() - t0, 1),
            "checker": "oracle/portal_oracle.py (numpy; pinned to the reference's shader text by tests/test_reference_text.py)"}


def valu_roofline(fl, pmc, segments, world, kernel_ms, traffic, specialize):
    """The binding roofline of a trace launch: binary32 arithmetic on the vector ALU (157.3 TFLOP/s; the f32 MFMA instructions run on the same
    FMA lanes and do not overlap with VALU work: tools/mfma_probe.hip, profiles/r02/mfma_probe.jsonl).  `fl`: flops_per_segment() of the
    workload, `pmc`: stored_pmc() of it or None, `segments`: bounce-loop trips of the frame (counted on the GPU), `kernel_ms`: this rank's
    launch.  With PMC counters stored, `frac` is capped at the hardware's own instruction ceiling -- for EVERY workload this is called for."""
    # the binding roofline: binary32 arithmetic on the vector ALU (157.3 TFLOP/s; the f32 MFMA instructions run on the same
    # FMA lanes and do not overlap with VALU work: tools/mfma_probe.hip, profiles/r02/mfma_probe.jsonl)
    tf = segments / world * fl["flops"] / (kernel_ms * 1e-3) / 1e12
    roof = {
        "bound": "valu", "achieved": round(tf, 3), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / FP32_PEAK_TFLOPS, 5),
        "traffic": traffic,
        # rounds 1-3 also claimed the oracle's comparisons as operations (a v_cmp is not a floating-point operation of this peak; with them the
        # count sat above the hardware's instruction ceiling): the same launch by that accounting, for comparison across rounds only
        "frac_with_comparisons_as_in_round_3": round(segments / world * fl.get("with_compares", fl["flops"]) / (kernel_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 5),
        "flops_per_segment": round(fl["flops"], 1), "flops_counted": fl["which"], "flops_sample_pixels": fl["sampled_pixels"],
        # the reference algorithm's arithmetic (as the oracle evaluates the GLSL) per second against the same peak: what the frame "is worth";
        # `frac` above counts only what this kernel still executes of it
        "reference_flops_per_segment": round(fl["algorithmic"], 1),
        "frac_of_reference_arithmetic": round(segments / world * fl["algorithmic"] / (kernel_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 5),
        "flops_source": fl["source"] + " (tools/count_flops.py: numpy oracle on a seeded pixel sample of this full-size frame; comparisons not claimed)",
        "note": "FP32-VALU-bound, no MFMA. achieved = binary32 operations per bounce-loop trip (fma = 2; / and sqrt = 1 each although they cost "
                "11 and 14 instructions) x trips of this launch (counted on the GPU) / kernel time."
                + (" Counted: operations with a ray-dependent operand -- the timed kernel has the scene uniforms baked in and folds the rest "
                   f"({fl['all_flops']:.0f} per trip with them)." if specialize == 2 else
                   " Counted: operations with a ray-dependent operand; most uniform-only ones come from the prologue kernel, the remainder is executed per ray "
                   f"but not counted ({fl['all_flops']:.0f} per trip with all of them).")
                + (f" Of the reference algorithm's {fl['algorithmic']:.0f} the kernel executes {fl['flops']:.0f}: loop-carried ray transforms of the scene "
                   "snippet that no statement reads are deferred away (counted on the host build), and while a ray still starts at the camera the origin "
                   "half of the snippet's ray chains comes from the prologue kernel (read off the generated source); generated plane tests the wave-level cull skips are subtracted too (tests and culls per trip counted on the host build), and so are the matrix-product terms with a baked zero matrix element, which this build never executes."
                   if fl["flops"] != fl["algorithmic"] else ""),
    }
    if pmc:
        # VALU issue: wave64 instructions x 2 cycles (the full-rate class) / (1024 SIMDs x kernel time x 2.4 GHz).  A floor: compares and
        # division helpers take 4 cycles, transcendentals 8 (profiles/r01/valu_rates.jsonl), and the sustained clock is below 2.4 GHz.
        roof["valu_issue_frac"] = round(pmc["insts_valu"] / world * 2.0 / 1024.0 / (kernel_ms * 1e-3 * 2.4e9), 4)
        roof["valu_insts_per_launch"] = pmc["insts_valu"]
        if "classes" in pmc:
            # What the pipes were busy with, from the instruction classes of the same PMC passes and the measured issue cost of each
            # (profiles/r01/valu_rates.jsonl: fma / mul / add / integer add 2 cycles per wave64 instruction, v_rcp / v_sqrt / v_rsq 8,
            # compares, selects, division helpers, floor ... 4).  The rest (moves, compares, selects, v_div_*) is not split further by
            # the counters: priced at 2 cycles it gives the lower bound, at 4 the upper one.  Denominator: GRBM_GUI_ACTIVE (busy
            # cycles per XCD, summed over the 8 XCDs by the collector) x 1024 SIMDs / 8.
            k = pmc["classes"]
            full = k["SQ_INSTS_VALU_FMA_F32"] + k["SQ_INSTS_VALU_MUL_F32"] + k["SQ_INSTS_VALU_ADD_F32"] + k["SQ_INSTS_VALU_INT32"]
            rest = max(0.0, pmc["insts_valu"] - full - k["SQ_INSTS_VALU_TRANS_F32"])
            simd_cycles = k["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0
            busy = [(2.0 * full + 8.0 * k["SQ_INSTS_VALU_TRANS_F32"] + price * rest) / simd_cycles for price in (2.0, 4.0)]
            roof["valu_busy_bounds"] = [round(busy[0], 3), round(busy[1], 3)]
            roof["valu_class_share"] = {"fma_mul_add_int": round(full / pmc["insts_valu"], 3), "transcendental": round(k["SQ_INSTS_VALU_TRANS_F32"] / pmc["insts_valu"], 3),
                                        "moves_compares_selects_division_helpers": round(rest / pmc["insts_valu"], 3)}
        roof["frac_ceiling_from_pmc"] = round(64 * 2 * pmc["insts_valu"] / (kernel_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4)  # every VALU instruction a full-width FMA
        if "classes" in pmc:
            k = pmc["classes"]
            t_s = kernel_ms * 1e-3
            # what the hardware COUNTED, against the same peak.  `frac_ceiling_valu_plus_fma`: every VALU instruction one operation,
            # FMAs two -- no count of executed arithmetic can exceed it, so `frac` must sit below.  `hw_flops_frac`: only the
            # floating-point arithmetic classes (2 x FMA + MUL + ADD) on the lanes that were active -- compares, selects, moves,
            # conversions, integer work and the division / square-root helper instructions count as nothing here, although the
            # oracle's operation count (`frac`) credits a compare, a min or a floor with 1 and `/`, sqrt with 1 each.
            util = pmc.get("lane_utilisation", 1.0)
            roof["frac_ceiling_valu_plus_fma"] = round((pmc["insts_valu"] + k["SQ_INSTS_VALU_FMA_F32"]) / world * 64 / t_s / 1e12 / FP32_PEAK_TFLOPS, 4)
            roof["hw_flops_frac"] = round((2 * k["SQ_INSTS_VALU_FMA_F32"] + k["SQ_INSTS_VALU_MUL_F32"] + k["SQ_INSTS_VALU_ADD_F32"]) / world * 64 * util / t_s / 1e12 / FP32_PEAK_TFLOPS, 4)
            roof["lane_utilisation"] = round(util, 4)
            # Round 5: what the hardware counted as ARITHMETIC -- 2 x FMA + MUL + ADD + the transcendental unit's instructions
            # (v_rcp / v_sqrt / v_rsq: one operation each) on the active lanes -- is what `frac` may claim at most.  The oracle's count is the
            # operations of the algorithm the kernel still has to perform; the compiler shares and folds more (common subexpressions across
            # the unrolled copies of a snippet, constants), so where the count is above the counters the counters are printed.
            hw = (2 * k["SQ_INSTS_VALU_FMA_F32"] + k["SQ_INSTS_VALU_MUL_F32"] + k["SQ_INSTS_VALU_ADD_F32"] + k["SQ_INSTS_VALU_TRANS_F32"]) / world * 64 * util / t_s / 1e12 / FP32_PEAK_TFLOPS
            roof["hw_arith_frac"] = round(hw, 4)
            roof["frac_counted_by_the_oracle"] = roof["frac"]
            roof["achieved_counted_by_the_oracle"] = roof["achieved"]
            roof["count_over_hardware"] = round(roof["frac"] / hw, 3) if hw > 0 else None
            if hw < roof["frac"]:
                roof["frac"] = round(hw, 5)
                roof["achieved"] = round(hw * FP32_PEAK_TFLOPS, 3)
            roof["frac_is"] = "min(the oracle's count of executed arithmetic, the hardware's FP32 arithmetic counters of the same code object)"
        roof["pmc_source"] = pmc["source"] + " (stored rocprofv3 PMC passes of the code object named in pmc_code_object_sha256 -- the one this run timed; not re-measured by this run)"
        roof["pmc_code_object_sha256"] = pmc.get("code_object_sha256")
        roof["pmc_kernel_source_sha256"] = pmc.get("kernel_source_sha256")
        roof["pmc_match"] = pmc.get("match")
    return roof


COMPACT_LINE_LIMIT = 4096  # bytes: the driver keeps ~8 KB of stdout; round 5's 32 KB line came back `parsed: null`


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(out, detail=True):
    """The ONE stdout line (<= 4 KB): the contract's keys, `roofline` + `cpu_baseline`, the checker's verdicts on the timed build and one short
    object per workload.  Everything else -- notes, tuning, contract distances, JIT detail, per-workload rooflines -- stays in the detail record
    (`bench_detail.json`, also one stderr line).  A test bounds the size (tests/test_host_logic.py, tests/test_gpu_parity.py)."""
    cfg = out.get("config", {})
    line = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype") if k in out}
    line["data"] = "synthetic: the reference's shipped scene file, scene camera, no stage"
    version = str(cfg.get("toolchain", ""))
    line["config"] = {**_pick(cfg, ("workload", "trips_per_primary_ray", "build", "code_object_sha256", "kernel_source_sha256", "affine_rays", "candidate_frames_identical", "transport", "frames_in_flight",
                                   "frames_identical_to_one_in_flight", "ms_per_step_one_frame_in_flight")),
                      "parallelism": str(cfg.get("parallelism", ""))[:60], "jit_specialisation": cfg.get("jit_specialisation"),
                      "hiprtc_version": version.split("hiprtc_version=")[-1] if "hiprtc_version=" in version else None}
    line.update(_pick(out, ("kernel_ms", "kernel_ms_per_rank", "transport_ms", "segments_per_frame", "segment_mray_s", "jit_seconds")))
    if "roofline" not in out:  # (a plain run measures no roofline)
        return _finish_line(line, detail)
    roof = out.get("roofline") or {}
    line["roofline"] = _pick(roof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "hw_arith_frac", "frac_counted_by_the_oracle", "lane_utilisation",
                                    "valu_insts_per_launch", "pmc_code_object_sha256", "pmc_kernel_source_sha256", "pmc_match"))
    if "traffic" not in line["roofline"]:
        line["roofline"]["traffic"] = None
    if roof.get("pmc_source"):
        line["roofline"]["pmc_source"] = roof["pmc_source"].split(" ")[0]
    if roof.get("pmc_unavailable"):
        line["roofline"]["pmc_unavailable"] = str(roof["pmc_unavailable"])[:120]
    if "roofline_hbm" in out:
        line["roofline_hbm"] = _pick(out["roofline_hbm"], ("bound", "achieved", "peak", "unit", "frac", "traffic"))
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        line["cpu_baseline"] = {**_pick(cb, ("value", "unit", "cores", "kind", "error")), **({"sample": str(cb["sample"]).split(", same generated")[0][:150]} if "sample" in cb else {})}
    if "cpu_baseline_reference_text" in out:
        line["cpu_baseline_reference_text"] = _pick(out["cpu_baseline_reference_text"], ("value", "unit", "cores", "kind"))
    parity = {}
    for key, short in (("reference_text_check_of_the_timed_build", "timed_build_vs_reference_text"), ("oracle_check_of_the_timed_build", "timed_build_vs_oracle")):
        if key in out:
            parity[short] = _pick(out[key], ("pixels", "bit_exact", "max_abs_error")) or {"error": str(out[key].get("error", ""))[:80]}
    if parity:
        line["parity"] = parity
    if "frame_check" in out:
        line["frame_check"] = out["frame_check"]
    other = {"unspecialised": out.get("kernel_ms_without_jit_specialisation"), "ints_baked": out.get("kernel_ms_with_only_int_uniforms_baked"),
             "patterns": out.get("kernel_ms_with_only_zero_patterns_and_mode_switches"), "tolerance_mode": (out.get("fast_math_mode") or {}).get("kernel_ms"),
             "several_frames_per_launch": (out.get("several_frames_per_launch") or {}).get("kernel_ms_per_frame")}
    other = {k: v for k, v in other.items() if v is not None}
    if other:
        line["other_builds_kernel_ms"] = other
    rows = []
    for w in out.get("workloads", []):
        if "error" in w:
            rows.append({"id": w.get("name"), "error": str(w["error"])[:60]})
            continue
        r = w.get("roofline") or {}
        row = {"id": w.get("name"), "ms_per_step": w.get("ms_per_step"), "kernel_ms": w.get("kernel_ms"), "mray_s": w.get("value"), "trips": w.get("trips_per_primary_ray"),
               "frac": r.get("frac"), "cpu_mray_s": (w.get("cpu_baseline") or {}).get("value"), "bit_exact": (w.get("oracle_check") or {}).get("bit_exact"),
               "in_flight": w.get("frames_in_flight")}
        if "kernel_ms_per_rank" in w:
            row["kernel_ms_per_rank"] = w["kernel_ms_per_rank"]
            if row["kernel_ms"] is None:
                row["kernel_ms"] = max(w["kernel_ms_per_rank"])
        if r.get("pmc_unavailable"):
            row["pmc"] = "unavailable"
        rows.append({k: v for k, v in row.items() if v is not None})
    if rows:
        line["workloads"] = rows
    return _finish_line(line, detail)


def _finish_line(line, detail):
    if detail:
        line["detail"] = "bench_detail.json (and one `[bench detail]` line on stderr): notes, tuning, every roofline in full"
    text = json.dumps(line, separators=(",", ":"))
    # belt: whatever a future field adds, the line that reaches the driver stays parseable
    for drop in ("other_builds_kernel_ms", "cpu_baseline_reference_text", "roofline_hbm", "workloads"):
        if len(text) <= COMPACT_LINE_LIMIT:
            break
        line.pop(drop, None)
        line["dropped_for_size"] = line.get("dropped_for_size", []) + [drop]
        text = json.dumps(line, separators=(",", ":"))
    return text


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: at most this much float32 data
DUMP_SAMPLE_PIXELS = 1 << 21  # pixels of the seeded sample of a frame above that (float32 RGBA + float64 index: 48 MiB)


def dump_outputs(directory, image):
    """--dump-outputs: the frame of the last timed step -- the (H, W, 4) RGBA8 array a caller of the timed path receives -- as float32 .npy in
    `directory`: `frame_rgba8.npy` whole when it fits in DUMP_LIMIT_BYTES, otherwise `frame_rgba8_sample.npy` (pixels x 4) at a fixed seeded sample of
    pixels whose flat indices (y * W + x) are `frame_rgba8_sample_pixels.npy`.  Same arguments, same files: two builds compare output for output."""
    os.makedirs(directory, exist_ok=True)
    h, w = image.shape[:2]
    if image.size * 4 <= DUMP_LIMIT_BYTES:
        np.save(os.path.join(directory, "frame_rgba8.npy"), image.astype(np.float32))
        return
    pixels = np.sort(np.random.default_rng(0).choice(h * w, size=DUMP_SAMPLE_PIXELS, replace=False))
    np.save(os.path.join(directory, "frame_rgba8_sample.npy"), image.reshape(-1, 4)[pixels].astype(np.float32))
    np.save(os.path.join(directory, "frame_rgba8_sample_pixels.npy"), pixels.astype(np.float64))


def emit(out, full=True):
    """detail record -> bench_detail.json (+ gpurun_out/ when that exists: it travels back from the GPU box) and stderr; compact line -> stdout (last)."""
    if not full:  # a plain run: the line alone
        print(compact_line(out, detail=False), flush=True)
        return
    detail = json.dumps(out)
    for d in (HERE, os.path.join(HERE, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.environ.get("PTL_BENCH_DETAIL") or os.path.join(d, "bench_detail.json"), "w") as f:
                    f.write(detail + "\n")
            except OSError:
                pass
            if os.environ.get("PTL_BENCH_DETAIL"):
                break
    print("[bench detail] " + detail, file=sys.stderr, flush=True)
    print(compact_line(out), flush=True)


def configure(renderer, args):
    renderer.set_option("render_depth", args.depth)
    renderer.set_option("aa_count", args.aa)
    if args.panini >= 0.0:
        renderer.set_option("use_panini_projection", 1)
        renderer.set_option("panini_param", args.panini)
    renderer.set_option("view_angle", args.fov / 180.0 * np.pi)
    if args.camera:
        c = [float(x) for x in args.camera.split(",")]
        renderer.set_camera(c[:3], c[3], c[4], c[5])


def main():
    args = parse_args()
    import torch
    import torch.distributed as dist

    import portal_amd as pa

    # PTL_BENCH_BACKEND=gloo is a rehearsal hook: the multi-rank control flow on a box with ONE GPU (all ranks share it, the
    # gather is staged through host memory).  The driver's runs use the default: one rank per GPU, RCCL.
    backend = os.environ.get("PTL_BENCH_BACKEND", "nccl")
    if args.gpus < 1:
        raise SystemExit(f"--gpus {args.gpus}: at least one GPU")
    launched = "RANK" in os.environ or "WORLD_SIZE" in os.environ
    if backend == "nccl" and not launched and args.gpus > (torch.cuda.device_count() if torch.cuda.is_available() else 0):
        # one rank per GPU over RCCL: never a line that says n_gpus: N for fewer devices, never a silent n_gpus: 1
        raise SystemExit(f"--gpus {args.gpus} but this node shows {torch.cuda.device_count() if torch.cuda.is_available() else 0} GPU(s) "
                         "(PTL_BENCH_BACKEND=gloo rehearses N ranks on fewer devices)")
    if args.gpus > 1 and not launched:
        # started as plain `python bench.py --gpus N`: launch the N ranks ourselves, exactly as the driver's torch.distributed.run line would
        import socket
        import subprocess

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print(f"[bench] --gpus {args.gpus} without a launcher: starting {args.gpus} ranks under torch.distributed.run (port {port})", file=sys.stderr, flush=True)
        raise SystemExit(subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))).returncode)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the render path has no CPU fallback)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the line would not describe the run")
    narrowed = any(os.environ.get(k) for k in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"))  # a launcher that shows each rank its own GPU
    if backend == "nccl" and world > torch.cuda.device_count() and not narrowed:
        raise SystemExit(f"--gpus {world} over RCCL needs one GPU per rank; this node shows {torch.cuda.device_count()}")
    # one rank per GPU: LOCAL_RANK is the device index when every rank sees the whole node (torchrun's default); when the launcher
    # narrows visibility to one GPU per process, or the gloo rehearsal shares one GPU, the modulo picks what is there
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        from datetime import timedelta

        # a collective that never completes (a rank died during start-up, a transport hung) fails loudly after 5 minutes instead of
        # sitting in the driver's window; `stage` lines on stderr say how far each rank got
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=timedelta(seconds=300))
        else:
            dist.init_process_group(backend, timeout=timedelta(seconds=300))

    t_start = time.perf_counter()

    def stage(what):
        if world > 1 or os.environ.get("PTL_BENCH_VERBOSE"):
            print(f"[bench r{rank}/{world} +{time.perf_counter() - t_start:6.1f}s] {what}", file=sys.stderr, flush=True)

    W, H = args.width, args.height
    scene_path, scene_kw = scene_of(args, pa)
    scene = pa.Scene.from_file(scene_path)
    from portal_amd import parallel

    frame = pa.Frame(W, H, rank, world)
    rows = pa.shard_rows(frame)
    shard = parallel.alloc_shard(H, W, world, dev)
    stream = torch.cuda.current_stream(dev)
    spec_flags = {0: 0, 1: pa.FLAG_SPECIALIZE_INTS, 2: pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL}[args.specialize] | args.extra_flags

    def make_renderer(waves, extra_flags=""):
        # PTL_HIPRTC_FLAGS is read when the kernel is compiled (and is part of the code-object cache key).  LLVM's -mllvm options are
        # process-wide and STICKY (a later compile that does not mention one keeps the earlier value), so a build with extra backend
        # options is compiled in a child process into the code-object cache first; this process then only loads it.
        if extra_flags:
            import subprocess

            child = ("import sys; sys.path.insert(0, sys.argv[1]); import portal_amd as pa; "
                     "pa.SceneRenderer(pa.Scene.from_file(sys.argv[2]), device=-1, flags=int(sys.argv[3]))")
            subprocess.run([sys.executable, "-c", child, HERE, scene_path, str(spec_flags | pa.flag_waves(waves))],
                           env=dict(os.environ, PTL_HIPRTC_FLAGS=((os.environ.get("PTL_HIPRTC_FLAGS", "") + " ") if os.environ.get("PTL_HIPRTC_FLAGS") else "") + extra_flags),
                           capture_output=True, timeout=600)
        saved = os.environ.get("PTL_HIPRTC_FLAGS")
        os.environ["PTL_HIPRTC_FLAGS"] = ((saved + " ") if saved else "") + extra_flags
        try:
            r = pa.SceneRenderer(scene, device=local_rank, flags=spec_flags | pa.flag_waves(waves), **scene_kw)
        finally:
            if saved is None:
                os.environ.pop("PTL_HIPRTC_FLAGS", None)
            else:
                os.environ["PTL_HIPRTC_FLAGS"] = saved
        configure(r, args)
        return r

    # untimed: JIT-compile the candidate builds (same arithmetic: different register budgets / instruction schedulers) and keep
    # the fastest on this rank's shard.  16 launches each after a short spin-up, so that differences of a few percent are real.
    candidates = {"w0": (0, ""), "w3": (3, ""), "w4": (4, ""), "w5": (5, ""), "minreg": (0, "-mllvm -amdgpu-sched-strategy=iterative-minreg")}
    if world > 1 and args.build != "minreg":
        candidates.pop("minreg")  # needs a child-process compile per rank (sticky -mllvm options): not worth a start-up hazard on 8 ranks
    if args.build:
        candidates = {args.build: candidates[args.build]}
    elif args.waves >= 0:
        candidates = {f"w{args.waves}": (args.waves, "")}
    # cold cache only: build the candidates side by side (hiprtc is thread-safe; a compile-only renderer needs no device) -- the loop
    # below then finds every code object in the cache.  Builds with extra backend options go through their own child process anyway.
    from concurrent.futures import ThreadPoolExecutor

    def prebuild(item):
        waves, extra = item
        if not extra:
            pa.SceneRenderer(pa.Scene.from_file(scene_path), device=-1, flags=spec_flags | pa.flag_waves(waves), **scene_kw)

    with ThreadPoolExecutor(max_workers=4) as pool:
        list(pool.map(prebuild, candidates.values()))
    tried = {}
    # Every candidate is the same source built with another register budget / scheduler, so every candidate must draw the same
    # bytes -- on a toolchain with a documented allocator miscompile that is checked, not assumed: the frame of each
    # build is compared with the first one's (`w0` unless a build is pinned) on the device, a build that differs is reported and
    # never timed for the value.  tests/test_reference_text.py checks the same builds against the oracle's frames.
    reference_frame, frames_differ = None, {}
    for name, (waves, extra) in candidates.items():
        stage(f"candidate build {name}")
        cand = make_renderer(waves, extra)
        for _ in range(8):
            cand.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream)
        ms = float(np.median([cand.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(16)]))
        torch.cuda.synchronize(dev)
        if reference_frame is None:
            reference_frame = shard.clone()
        same = torch.tensor([1 if torch.equal(shard, reference_frame) else 0], dtype=torch.int32, device=dev)
        if world > 1:
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
        if int(same.item()) == 0:
            frames_differ[name] = "frame differs from the first candidate's: excluded"
            continue
        tried[name] = (ms, cand, cand.resources(), waves)
    candidate_sha = None
    if rank == 0:
        import hashlib

        candidate_sha = hashlib.sha256(reference_frame[:rows].cpu().numpy().tobytes()).hexdigest()[:16]
    del reference_frame
    fastest = min(v[0] for v in tried.values())
    # a build that spills to scratch moves an order of magnitude more bytes than the framebuffer for a few
    # percent of time: take it only if it wins by more than 6 %, otherwise the fastest spill-free build
    clean = {k: v for k, v in tried.items() if v[2]["scratch_bytes"] == 0 and v[0] <= fastest * 1.06}
    pool = clean if clean else tried
    best = min(pool, key=lambda k: pool[k][0])
    # The candidates differ by a per cent or so and the pick would flip with the noise of 16 launches.  Among the builds within 1.5 % of the
    # fastest, one whose stored PMC passes counted THIS binary (same code-object sha256) is taken: the line's roofline then comes with the
    # hardware's own counters instead of without.
    if rank == 0 and not args.build and args.waves < 0:
        near = [k for k in pool if pool[k][0] <= pool[best][0] * 1.015]
        for k in sorted(near, key=lambda k: pool[k][0]):
            if stored_pmc(args, k, pool[k][1].code_object_sha256())[0] is not None:  # (an exact match first; below, the same source is accepted too)
                best = k
                break
    if world > 1:  # all ranks must run the same build: take rank 0's choice
        names = list(tried)
        choice = torch.tensor([names.index(best)], device=dev)
        dist.broadcast(choice, 0)
        best = names[int(choice.item())]
    renderer = tried[best][1]
    best_waves = tried[best][3]
    tuning = {k: {"ms": round(v[0], 4), **v[2]} for k, v in tried.items()}
    del tried
    # N > 1: how a frame reaches rank 0.  Two transports, same pixels:
    #   rccl-gather  packed shards, ONE dist.gather (RCCL send/recv group) + one strided de-interleave copy, double-buffered so
    #                that the gather of frame n overlaps the tracing of frame n+1;
    #   p2p-stores   rank 0's frame buffers are mapped into every rank (HIP IPC) and the kernel stores its row blocks straight
    #                into rank 0's HBM over xGMI; the collective shrinks to a one-element all-reduce used as a fence;
    #   p2p-copy     packed shard in the rank's own HBM + ONE strided hipMemcpy2DAsync into rank 0's mapped frame (SDMA over the rank's
    #                xGMI link, de-interleaving on the way) + the same fence.
    # PTL_BENCH_TRANSPORT=gather|p2p|copy|auto|fastest.  Default `auto`: the TIMED value goes through the single RCCL gather BASELINE.json's
    # north star names; the two peer transports are set up as well, must assemble the same bytes, and are timed (12 frames each, outside
    # the timed region) as extras in `config.transport_ms_per_frame`.  `fastest` times the value through whichever won; the other three pin one.
    staged = backend != "nccl"
    mode = os.environ.get("PTL_BENCH_TRANSPORT", "auto")
    keep_fastest = mode == "fastest"
    if keep_fastest:
        mode = "auto"
    transports = {}
    transport_notes = {}
    if world == 1 or mode in ("gather", "auto"):
        transports["rccl-gather"] = parallel.GatherTransport(H, W, rank, world, dev, depth=3, stage_through_host=staged)  # two gathers in flight behind the trace
    peer_kinds = {"p2p-stores": parallel.PeerTransport, "p2p-copy": parallel.CopyTransport}
    wanted = {"p2p": ["p2p-stores"], "copy": ["p2p-copy"], "auto": ["p2p-stores", "p2p-copy"]}.get(mode, [])
    if mode == "auto" and not (args.full or keep_fastest):
        wanted = []  # a plain run: the timed value goes through the gather, and the peer transports are --full's extras
    for kind in (wanted if world > 1 else []):
        stage(f"transport set-up {kind}")
        ok, peer = 1, None
        try:
            peer = peer_kinds[kind](H, W, rank, world, dev, host_fence=staged)
        except Exception as e:  # no IPC between these devices / processes: the gather remains
            ok = 0
            transport_notes[kind] = f"unavailable: {str(e)[:200]}"
        agreed = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(agreed, op=dist.ReduceOp.MIN)
        if int(agreed.item()) == 1:
            transports[kind] = peer
        else:
            transport_notes.setdefault(kind, "unavailable on another rank")
            if peer is not None:
                peer.abandon()  # not close(): that is collective, and the rank that failed is not taking part
    if not transports:
        raise SystemExit(f"PTL_BENCH_TRANSPORT={mode} but peer frame buffers are unavailable: {transport_notes}")

    def run_steps(tr, n, events=None, r=None):
        """n frames through transport `tr`; returns what tr.finish gave for the last one (the assembled frame on rank 0)."""
        r = r or renderer
        in_flight, last = [], None
        for k in range(n):
            slot = k % tr.depth
            while len(in_flight) >= tr.depth:  # a buffer is reused only after its frame has been assembled
                s0, work = in_flight.pop(0)
                last = tr.finish(work, s0)
            # `events`: a list of (start, end) pairs, one per step -- or a dict {first step of a group: (start, end, launches)}: ONE pair around a
            # group of consecutive launches (what the timed region of the headline uses: see there)
            if isinstance(events, dict):
                if k in events:
                    events[k][0].record(stream)
                r.draw_device(tr.frame, out_rgba8=tr.out_ptr(slot), stream=stream.cuda_stream)
                g0 = k - k % events["group"]
                if k == min(g0 + events["group"], n) - 1:
                    events[g0][1].record(stream)
            else:
                pair = events[k] if events is not None else None
                if pair is not None:
                    pair[0].record(stream)
                r.draw_device(tr.frame, out_rgba8=tr.out_ptr(slot), stream=stream.cuda_stream)
                if pair is not None:
                    pair[1].record(stream)
            in_flight.append((slot, tr.submit(slot)))
        for s0, work in in_flight:
            last = tr.finish(work, s0)
        return last

    def timed_steps(tr, n, events=None, r=None):
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        last = run_steps(tr, n, events, r)  # every frame of the timed region is fully assembled on rank 0
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), last

    def timed_in_flight(r, fr, targets, warm, n):
        """n frames of an unchanged state with len(targets) frames in flight: the renderer's lanes (concurrent_draws K, lane_fence 0: one packet per
        draw, no cross-stream wait), a target per lane, ONE join behind all of them; wall time between two synchronisations."""
        # Lanes that start together stay together: two launches queued at the same moment share the chip evenly, end at the same moment, and their
        # drains coincide -- one drain per PAIR is hidden instead of one per frame (half the gain), and a region of 20 frames ends before the phases
        # have drifted apart.  So the second lane's first launch of a region is issued half a launch later (the renderer's option `lane_stagger_us`: a
        # host-side wait while the GPU is busy with the first): the phases start apart and stay apart.  PTL_BENCH_STAGGER=<fraction of a launch> (0: off).
        launch_ms = float(np.median([r.draw_device(fr, out_rgba8=targets[0].data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(5)]))
        r.set_option("lane_stagger_us", float(os.environ.get("PTL_BENCH_STAGGER", "0.5")) * launch_ms * 1e3)

        def queue(m):
            for k in range(m):
                r.draw_device(fr, out_rgba8=targets[k % len(targets)].data_ptr(), stream=stream.cuda_stream)
            r.join(stream.cuda_stream)

        r.set_option("concurrent_draws", len(targets))
        r.set_option("lane_fence", 0)
        torch.cuda.synchronize(dev)  # (no fence: what the caller's stream holds -- the targets' initialisation -- has to be over before the first lane draws)
        queue(len(targets))          # the first draw on a lane creates its stream's queue and loads its kernel instance (milliseconds of host work, idle GPU)
        torch.cuda.synchronize(dev)
        spin_until = time.perf_counter() + 0.15  # ... so, like before the one-stream region: settled clocks first (untimed), then the W warm-up steps
        while time.perf_counter() < spin_until:
            queue(16)
            torch.cuda.synchronize(dev)
        queue(warm)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        queue(n)
        torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
        r.set_option("concurrent_draws", 1)  # (drops the lanes' kernel instances; what follows is one stream again)
        r.set_option("lane_fence", 1)
        r.set_option("lane_stagger_us", 0)
        return seconds

    # untimed: keep the GPU busy for ~0.25 s so that the W warm-up steps and the timed region run at settled clocks
    # (a 20-step timed region is ~15 ms of work; without this it rides the power-management ramp)
    spin_until = time.perf_counter() + 0.25
    while time.perf_counter() < spin_until:
        for _ in range(16):
            renderer.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)

    stage("transports ready: " + ", ".join(transports))
    if len(transports) > 1:
        # untimed: every transport must assemble the same frame on rank 0 (reference: the first one set up), then the fastest is kept
        images = {name: tr.download(run_steps(tr, 1)) for name, tr in transports.items()}
        names = list(transports)
        same = torch.ones(len(names), dtype=torch.int32, device=dev)
        if rank == 0:
            for k, name in enumerate(names[1:], start=1):
                if not np.array_equal(images[names[0]], images[name]):
                    same[k] = 0
        dist.broadcast(same, 0)
        # a transport whose transfer raised on ANY rank (it still took part in its fence, so nobody hangs) is dropped everywhere
        broke = torch.tensor([1 if getattr(transports[name], "failed", None) else 0 for name in names], dtype=torch.int32, device=dev)
        dist.all_reduce(broke, op=dist.ReduceOp.MAX)
        del images
        for k, name in enumerate(names):
            if int(broke[k].item()) == 1:
                transport_notes[name] = "dropped: " + (getattr(transports[name], "failed", None) or "its transfer failed on another rank")
                transports.pop(name).close()
            elif int(same[k].item()) == 0:
                transport_notes[name] = f"dropped: its frame differs from the one `{names[0]}` assembled"
                transports.pop(name).close()
    transport_ms = {}
    if len(transports) > 1:
        for name, tr in transports.items():
            run_steps(tr, 4)
            transport_ms[name] = round(timed_steps(tr, 12)[0] / 12 * 1e3, 4)
        # the times are maxima over ranks: every rank picks the same
        keep = min(transport_ms, key=transport_ms.get) if (keep_fastest or "rccl-gather" not in transports) else "rccl-gather"
        for name in [n for n in transports if n != keep]:
            transports.pop(name).close()
    transport = next(iter(transports.values()))

    stage(f"timed region through {transport.name}")
    run_steps(transport, args.warmup)
    # The kernel's launch duration is measured over GROUPS: one event pair around every eight consecutive launches of the timed region (around
    # every launch when the region is short), the elapsed time divided by the launches in the group.  An event record is a packet of its own in
    # the queue, and two of them around EVERY launch held consecutive frames 8 us apart -- 4 % of a headline step, 17 % of a 1080p step -- that a
    # renderer which just queues its frames does not pay (tools/small_frames.py: 0.1873 ms per frame back to back against 0.1957 per step
    # with the markers; profiles/r05/small_frames.jsonl); and a pair around ONE launch in eight measures that launch WITH its markers (0.1924
    # against 0.1884 ms per step).  Per group, the figure is what rocprofv3's per-dispatch duration + the dispatch gap add up to.
    # Round 6: a SHORT timed region (the driver's --steps 20) is ONE group -- one pair around all of it, nothing between its launches -- so that it
    # measures what the 400-step region measures (round 5 bracketed every launch of a short region and read 4.5 % slower there).
    every = 8 if args.steps >= 64 else max(1, args.steps)
    events = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), min(every, args.steps - k)) for k in range(0, args.steps, every)}
    events["group"] = every
    in_flight = None
    lanes_failed = None
    final_image = None  # the frame of the last timed step on rank 0 (numpy), for --save-png / --dump-outputs
    if world == 1 and args.lanes > 1:
        try:
            # Round 6: TWO FRAMES IN FLIGHT.  A launch of this kernel ramps up for ~10 us and drains for as long (the last workgroups of a
            # frame leave CUs idle that the next frame's first workgroups could use); a renderer that queues frames and looks at them later need not
            # pay that per frame.  The renderer's own option does it (include/portal_amd.h "lane_fence"): consecutive draws go round-robin to K
            # internal streams, each draw is ONE packet, each lane writes a target of its own, the caller's stream joins behind all of them at the
            # end.  Same kernel, same bytes (compared below); the timed region is K frames queued, one join, one synchronisation.
            lanes = args.lanes
            targets = [shard] + [torch.empty_like(shard) for _ in range(lanes - 1)]
            for t in targets:
                t.zero_()
            elapsed = timed_in_flight(renderer, frame, targets, max(args.warmup, lanes), args.steps)
            last = targets[(args.steps - 1) % lanes][:H]  # the frame of the last timed step
            in_flight = {"frames_in_flight": lanes}
            kernel_ms = kernel_ms_from = None
            if args.full:
                # ... and the SAME K steps one at a time on one stream, right behind it, between two synchronisations and between one pair of HIP events:
                # `kernel_ms` (the launch duration rocprofv3's per-dispatch average agrees with: what `roofline` divides by) and what a step costs with
                # one frame in flight (`ms_per_step_one_frame_in_flight`, rounds 1-5's figure)
                n_k = max(args.steps, 64)
                ev_k = {0: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), n_k), "group": n_k}
                one_elapsed, one_last = timed_steps(transport, n_k, ev_k)
                kernel_ms = float(ev_k[0][0].elapsed_time(ev_k[0][1]) / n_k)
                kernel_ms_from = (f"HIP events around ONE group of {n_k} consecutive launches on one stream, right behind the timed region (same kernel, same frame): elapsed / launches; "
                                  f"the timed region itself has {lanes} frames in flight on {lanes} streams, where a launch's own duration is not the time a frame costs")
                same_bytes = bool(all(torch.equal(t[: one_last.shape[0]], one_last) for t in targets))
                in_flight.update({"frames_identical_to_one_in_flight": same_bytes,
                                  "ms_per_step_one_frame_in_flight": round(one_elapsed / n_k * 1e3, 4), "steps_one_frame_in_flight": n_k})
                if not same_bytes:
                    raise SystemExit("bench: a frame drawn with two frames in flight differs from the frame drawn alone")
            del targets
        except Exception as e:  # (streams or kernel instances could not be had: the line must still come out -- one frame at a time, and it says so)
            lanes_failed = str(e)[:200]
            print(f"[bench] two frames in flight unavailable, timing one frame at a time: {lanes_failed}", file=sys.stderr)
            in_flight = None
            try:
                renderer.set_option("concurrent_draws", 1)
                renderer.set_option("lane_fence", 1)
            except Exception:
                pass
    if in_flight is not None:
        pass
    elif world == 1:
        elapsed, last = timed_steps(transport, args.steps, events)
        groups = [v for k, v in events.items() if k != "group"]
        kernel_ms = float(sum(a.elapsed_time(b) for a, b, _ in groups) / sum(c for _, _, c in groups))
        kernel_ms_from = f"HIP events around {len(groups)} group(s) of {every} consecutive launches of the {args.steps} timed ones: elapsed / launches"
    else:
        # N > 1: between two launches the launch stream also waits for the transport to hand a buffer back, so a pair around a GROUP would time
        # the transport too: the timed region runs without any event, and every rank's kernel time comes from a pass of its own right behind
        # it (same frames, same transport, one pair per launch)
        elapsed, last = timed_steps(transport, args.steps)
        kernel_ms = kernel_ms_from = None
        if args.full:
            n_k = max(16, min(args.steps, 64))
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_k)]
            # (the frame of the last timed step first: this pass reuses the transport's buffers)
            final_image = transport.download(last) if rank == 0 and (args.save_png or args.dump_outputs) else None
            run_steps(transport, n_k, pairs)
            torch.cuda.synchronize(dev)
            kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in pairs]))
            kernel_ms_from = f"HIP events around each of {n_k} launches of an untimed pass right behind the timed region (same frames, same transport)"
    if rank == 0 and (args.save_png or args.dump_outputs) and final_image is None:
        final_image = transport.download(last) if in_flight is None else last.cpu().numpy()
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, final_image)
    per_rank_ms = [kernel_ms]
    if world > 1 and kernel_ms is not None:  # every rank's own kernel time: load balance of the interleave, and the slowest sets the frame
        gathered = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(gathered, torch.tensor([kernel_ms], dtype=torch.float64, device=dev))
        per_rank_ms = [float(t.item()) for t in gathered]
    kernel_ms = max(per_rank_ms) if kernel_ms is not None else None

    # untimed, N > 1: the LAST frame of the timed region, as assembled on rank 0 by the kept transport, against the same frame
    # rendered by rank 0 alone (one launch, no sharding, no transport).  On one GPU the transports were rehearsed with every rank on
    # the same device; this is the check that a fence / visibility problem on real xGMI cannot get past.
    frame_check = None
    if world > 1 and args.full:
        assembled = transport.download(last) if rank == 0 else None
        ok = torch.tensor([1], dtype=torch.int32, device=dev)
        if rank == 0:
            whole = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
            renderer.draw_device(pa.Frame(W, H, 0, 1), out_rgba8=whole.data_ptr(), stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            same = bool(np.array_equal(assembled, whole.cpu().numpy()))
            ok[0] = 1 if same else 0
            del whole
        dist.broadcast(ok, 0)
        frame_check = {"last_timed_frame_equals_the_frame_rendered_by_rank0_alone": bool(int(ok.item()) == 1)}

    # After the headline's timed region: BASELINE.json's divergent-ray stress config (C5: mobius_monoportal 7680x4320, aa 4, depth 64)
    # for a few frames through the same gather, in the SAME JSON line.  The headline's per-rank trace at 8 GPUs (~55 us) is of the order of
    # one collective's latency, so its scaling curve is flat by construction; C5's 16 ms per frame is the workload whose curve says
    # something about the sharding.  Run at every N (the N = 1 line is the reference the driver computes efficiency against).
    second = None
    if args.full and not args.no_second_workload and workload_key(args) == "portal_in_portal_3840x2160_d40":
        try:
            stage("second workload: c5")
            w2 = WORKLOADS["c5"]
            scene2 = pa.Scene.from_file(pa.scene_path(w2["scene"]))
            r2 = pa.SceneRenderer(scene2, device=local_rank, flags=spec_flags)
            r2.set_option("render_depth", w2["depth"])
            r2.set_option("aa_count", w2["aa"])
            tr2 = parallel.GatherTransport(w2["height"], w2["width"], rank, world, dev, depth=3, stage_through_host=staged)
            run_steps(tr2, 2, r=r2)
            n2 = 6
            flight2 = None
            if world == 1:  # one pair around the region (nothing between its launches); N > 1: a pair per launch, so that a wait for the transport is not timed
                ev2 = {0: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), n2), "group": n2}
                el2, _last2 = timed_steps(tr2, n2, ev2, r=r2)
                k2 = [float(ev2[0][0].elapsed_time(ev2[0][1]) / n2)]
                # (one frame at a time: a 12.5 ms launch has nothing to gain from a second one in flight -- measured 12.64 against 12.58 ms, profiles/r06/README.md)
            else:
                ev2 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n2)]
                el2, _last2 = timed_steps(tr2, n2, ev2, r=r2)
                k2 = [float(np.mean([a.elapsed_time(b) for a, b in ev2]))]
            if world > 1:
                got2 = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
                dist.all_gather(got2, torch.tensor(k2, dtype=torch.float64, device=dev))
                k2 = [float(t.item()) for t in got2]
            ms2 = el2 / n2 * 1e3
            second = {"workload": f"scenes/{w2['scene']}.ron {w2['width']}x{w2['height']} aa={w2['aa']} depth={w2['depth']}", "steps": n2, "warmup": 2,
                      "ms_per_step": round(ms2, 4), "value": round(w2["width"] * w2["height"] * w2["aa"] / (ms2 * 1e-3) / 1e6, 3), "unit": "Mray/s",
                      "kernel_ms_per_rank": [round(x, 4) for x in k2], "transport_ms": round(max(0.0, ms2 - max(k2)), 4), "transport": tr2.name,
                      "jit_specialisation": ["none", "int/bool scene uniforms baked", "all scene uniforms baked (camera dynamic)"][args.specialize],
                      **(flight2 or {"frames_in_flight": 1})}
            # ... with its own roofline (same accounting as the headline's: trips counted on the GPU, the oracle's operations per trip, PMC cap)
            try:
                import argparse as _ap

                a2 = _ap.Namespace(**{**vars(args), **w2, "camera": "", "panini": -1.0, "fov": 90.0, "scene_file": ""})
                counting2 = pa.SceneRenderer(scene2, device=local_rank, flags=pa.FLAG_COUNT_SEGMENTS | spec_flags)
                counting2.set_option("render_depth", w2["depth"])
                counting2.set_option("aa_count", w2["aa"])
                seg2 = torch.zeros(1, dtype=torch.int64, device=dev)
                frame2 = pa.Frame(w2["width"], w2["height"], rank, world)
                buf2 = torch.empty((pa.shard_rows(frame2), w2["width"], 4), dtype=torch.uint8, device=dev)
                counting2.draw_device(frame2, out_rgba8=buf2.data_ptr(), segments=seg2.data_ptr(), stream=stream.cuda_stream)
                torch.cuda.synchronize(dev)
                if world > 1:
                    dist.all_reduce(seg2)
                sha2 = r2.code_object_sha256()
                fl2, (pmc2, why2) = flops_per_segment(a2, r2.affine_rays()), stored_pmc(a2, "w0", sha2, source_sha256(r2))
                second["segments_per_frame"] = int(seg2.item())
                second["trips_per_primary_ray"] = round(int(seg2.item()) / (w2["width"] * w2["height"] * w2["aa"]), 4)
                second["code_object_sha256"] = sha2
                if fl2:
                    second["roofline"] = valu_roofline(fl2, pmc2, int(seg2.item()), world, max(k2), pmc2["traffic"] if pmc2 else None, args.specialize)
                    if pmc2 is None:
                        second["roofline"]["pmc_unavailable"] = why2
                del counting2, buf2
                if world == 1 and not args.no_cpu_baseline:  # the checker's verdict and a bounded CPU baseline for this workload too
                    a2.cpu_seconds = min(args.cpu_seconds, 4.0)
                    second["cpu_baseline"] = cpu_baseline(a2, pa)
                    second["oracle_check"] = oracle_check(a2, pa, r2, torch, dev, stream, n=1024)
            except Exception as e:
                print(f"[bench] second workload roofline unavailable: {e}", file=sys.stderr)
                if world > 1:
                    raise
            tr2.close()
            del tr2, r2, _last2
        except Exception as e:  # the headline number does not depend on it
            print(f"[bench] second workload unavailable: {e}", file=sys.stderr)
            if world > 1:
                raise  # ... but at N > 1 a rank that skipped collectives would hang the others: fail loudly instead

    # After that, N = 1 only: the other BASELINE.json configs, SURVEY 8d's Panini variant and one DEEP view of the headline scene (into the nested
    # portals: several trips per primary ray, the regime "depth = 40" exists for), each timed like the headline -- K frames between two
    # synchronisations, the kernel's launches between HIP events -- with its trips per ray, its roofline, a bounded CPU baseline and the
    # checker's verdict on the frame of the build that was timed.  (one driver-run line for every workload.)
    others = []
    if args.full and world == 1 and not args.no_second_workload and not args.no_cpu_baseline and workload_key(args) == "portal_in_portal_3840x2160_d40":
        import argparse as _ap

        extra = [("c2", WORKLOADS["c2"]), ("c3", WORKLOADS["c3"]), ("c4-panini", dict(WORKLOADS["c4"], panini=1.0, fov=140.0)), ("c4-deep", WORKLOADS["c4-deep"]),
                 ("recursive-room", WORKLOADS["recursive-room"])]
        for wname, wl in extra:
            try:
                stage(f"workload {wname}")
                a = _ap.Namespace(**{**vars(args), "camera": "", "panini": -1.0, "fov": 90.0, "scene_file": "", **wl})
                a.cpu_seconds = min(args.cpu_seconds, 4.0)
                sc_path, sc_kw = scene_of(a, pa)
                sc = pa.Scene.from_file(sc_path)
                Wk, Hk = a.width, a.height
                fr = pa.Frame(Wk, Hk, 0, 1)
                buf = torch.empty((Hk, Wk, 4), dtype=torch.uint8, device=dev)
                waves = 0  # ONE build per workload (no occupancy hint): the binary whose PMC passes are stored under profiles/
                rr = pa.SceneRenderer(sc, device=local_rank, flags=spec_flags | pa.flag_waves(waves), **sc_kw)
                configure(rr, a)
                for _ in range(6):
                    rr.draw_device(fr, out_rgba8=buf.data_ptr(), stream=stream.cuda_stream)
                probe_ms = float(np.median([rr.draw_device(fr, out_rgba8=buf.data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(10)]))
                steps = int(max(10, min(200, 40.0 / max(probe_ms, 0.02))))  # ~40 ms of timed region
                ev_every = 8 if steps >= 64 else steps  # (like the headline's: one event pair around every eight consecutive launches; a short region is one group)
                ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), min(ev_every, steps - k)) for k in range(0, steps, ev_every)}
                flight_k = None
                if args.lanes > 1 and lanes_failed is None:  # like the headline: the timed frames with `lanes` in flight, then the same frames one at a time between one event pair
                    bufs = [buf] + [torch.empty_like(buf) for _ in range(args.lanes - 1)]
                    ms_flight = timed_in_flight(rr, fr, bufs, 6, steps) / steps * 1e3
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for k in range(steps):
                    if k in ev:
                        ev[k][0].record(stream)
                    rr.draw_device(fr, out_rgba8=buf.data_ptr(), stream=stream.cuda_stream)
                    g0 = k - k % ev_every
                    if k == min(g0 + ev_every, steps) - 1:
                        ev[g0][1].record(stream)
                torch.cuda.synchronize(dev)
                ms_step = (time.perf_counter() - t0) / steps * 1e3
                kms = float(sum(x.elapsed_time(y) for x, y, _ in ev.values()) / sum(c for _, _, c in ev.values()))
                if args.lanes > 1 and lanes_failed is None:
                    flight_k = {"frames_in_flight": args.lanes, "ms_per_step_one_frame_in_flight": round(ms_step, 4),
                                "frames_identical_to_one_in_flight": bool(all(torch.equal(b, buf) for b in bufs))}
                    ms_step = ms_flight
                    del bufs
                cnt = pa.SceneRenderer(sc, device=local_rank, flags=pa.FLAG_COUNT_SEGMENTS | spec_flags, **sc_kw)
                configure(cnt, a)
                seg = torch.zeros(1, dtype=torch.int64, device=dev)
                cnt.draw_device(fr, out_rgba8=buf.data_ptr(), segments=seg.data_ptr(), stream=stream.cuda_stream)
                torch.cuda.synchronize(dev)
                trips = int(seg.item())
                del cnt
                sha = rr.code_object_sha256()
                rec = {"name": wname, "workload": f"{a.scene_file or 'scenes/' + a.scene + '.ron'} {Wk}x{Hk} aa={a.aa} depth={a.depth}" + (f" panini d={a.panini} fov={a.fov}" if a.panini >= 0 else "")
                                                  + (f" camera look_at,alpha,beta,r={a.camera}" if a.camera else ""),
                       "steps": steps, "ms_per_step": round(ms_step, 4), "kernel_ms": round(kms, 4), "value": round(Wk * Hk * a.aa / (ms_step * 1e-3) / 1e6, 3), "unit": "Mray/s",
                       "build": f"w{waves}", "code_object_sha256": sha, "segments_per_frame": trips, "trips_per_primary_ray": round(trips / (Wk * Hk * a.aa), 4),
                       "segment_mray_s": round(trips / (ms_step * 1e-3) / 1e6, 3), **(flight_k or {"frames_in_flight": 1})}
                fl_k, (pmc_k, why_k) = flops_per_segment(a, rr.affine_rays()), stored_pmc(a, f"w{waves}", sha, source_sha256(rr))
                if fl_k:
                    rec["roofline"] = valu_roofline(fl_k, pmc_k, trips, 1, kms, pmc_k["traffic"] if pmc_k else None, args.specialize)
                    if pmc_k is None:
                        rec["roofline"]["pmc_unavailable"] = why_k
                rec["roofline_hbm"] = {"bound": "hbm", "achieved": round(Wk * Hk * 4 / (kms * 1e-3) / 1e9, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": round(Wk * Hk * 4 / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 6), "traffic": pmc_k["traffic"] if pmc_k else None}
                rec["cpu_baseline"] = cpu_baseline(a, pa)
                rec["oracle_check"] = oracle_check(a, pa, rr, torch, dev, stream, n=2048)
                others.append(rec)
                del rr, buf
            except Exception as e:  # the headline number does not depend on it
                print(f"[bench] workload {wname} unavailable: {e}", file=sys.stderr)
                others.append({"name": wname, "error": str(e)[:300]})

    # bounce-loop trips per frame (untimed, separate kernel variant with the counter compiled in)
    segments = None
    if args.full:
        try:
            if args.no_segments:
                raise RuntimeError("--no-segments")
            counting = pa.SceneRenderer(scene, device=local_rank, flags=pa.FLAG_COUNT_SEGMENTS | spec_flags, **scene_kw)
            configure(counting, args)
            seg = torch.zeros(1, dtype=torch.int64, device=dev)
            counting.draw_device(frame, out_rgba8=shard.data_ptr(), segments=seg.data_ptr(), stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            if world > 1:
                dist.all_reduce(seg)
            segments = int(seg.item())
            del counting
        except Exception as e:  # the headline number does not depend on it
            print(f"[bench] segment count unavailable: {e}", file=sys.stderr)

    # untimed, N = 1 only: the same frame with NO JIT specialisation (every scene uniform read at run time), for the record.
    # (Skipped together with the CPU baseline, i.e. in the profiling runs: their per-kernel statistics are about the timed launches.)
    # ... and with only the Bool / Int scene uniforms baked (FLAG_SPECIALIZE_INTS): what an animation whose float uniforms and matrices
    # move every frame runs on without a rebuild per frame.
    # ... and with NO value baked but the zero patterns of the matrices and the renderer's mode switches compiled in (FLAG_SPECIALIZE_PATTERNS):
    # valid while the patterns hold, i.e. for every frame of a clip whose portals move without leaving their planes' axes.
    dynamic_ms = ints_ms = patterns_ms = dynamic_build = ints_build = patterns_build = None
    if args.full and world == 1 and args.specialize != 0 and not args.no_cpu_baseline:
        try:
            for base_flags in (0, pa.FLAG_SPECIALIZE_INTS, pa.FLAG_SPECIALIZE_PATTERNS):
                timings = []
                # the two register budgets that matter for this kernel, at the JIT's optimisation level (-O3 without SLP) and at rounds 1-2's
                # -O1: the un-specialised headline kernel is the one measured case where -O1 is faster (kernel.cpp `opt_level`)
                for waves, opt in ((0, ""), (4, ""), (0, "-O1"), (4, "-O1")):
                    saved_opt = os.environ.get("PTL_JIT_OPT")
                    if opt:
                        os.environ["PTL_JIT_OPT"] = opt
                    try:
                        plain = pa.SceneRenderer(scene, device=local_rank, flags=base_flags | args.extra_flags | pa.flag_waves(waves), **scene_kw)
                    finally:
                        if opt:
                            if saved_opt is None:
                                os.environ.pop("PTL_JIT_OPT", None)
                            else:
                                os.environ["PTL_JIT_OPT"] = saved_opt
                    configure(plain, args)
                    for _ in range(8):
                        plain.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream)
                    ms = float(np.median([plain.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(16)]))
                    timings.append((plain.resources()["scratch_bytes"] > 0, ms, f"w{waves}{opt}"))
                    del plain
                if base_flags == 0:
                    dynamic_ms, dynamic_build = min(timings)[1:]  # a spill-free build first, then the faster
                elif base_flags == pa.FLAG_SPECIALIZE_INTS:
                    ints_ms, ints_build = min(timings)[1:]
                else:
                    patterns_ms, patterns_build = min(timings)[1:]
        except Exception as e:
            print(f"[bench] dynamic-uniform timing unavailable: {e}", file=sys.stderr)

    # untimed, N = 1 only: several frames per LAUNCH (FLAG_SLICES: grid.z = frame, one uniform block per slice in a device buffer -- what
    # `portal-amd render` does with the blur sub-frames of a clip frame).  The ramp and tail of one launch are shared by the frames in it,
    # which is what a small frame (C2: 50 us) loses most of its time to.  Same build otherwise, same frames (compared below).
    batched = None
    if args.full and world == 1 and not args.no_segments and args.specialize == 2:  # (--no-segments: the profiling passes, whose statistics are about the timed launches)
        try:
            nsl = 8 if W * H <= 1920 * 1080 else 4
            sl_r = pa.SceneRenderer(scene, device=local_rank, flags=spec_flags | pa.FLAG_SLICES, **scene_kw)
            configure(sl_r, args)
            big = torch.empty((nsl, H, W, 4), dtype=torch.uint8, device=dev)

            def one_batch(timed=False):
                for j in range(nsl):
                    sl_r.stage_slice(frame, j)
                return sl_r.draw_slices(frame, nsl, out_rgba8=big.data_ptr(), slice_pixels=W * H, stream=stream.cuda_stream, timed=timed)

            for _ in range(4):
                one_batch()
            ms_b = float(np.median([one_batch(True) for _ in range(12)])) / nsl
            one = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
            renderer.draw_device(frame, out_rgba8=one.data_ptr(), stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            same = bool(all(torch.equal(big[j], one) for j in range(nsl)))
            batched = {"frames_per_launch": nsl, "kernel_ms_per_frame": round(ms_b, 4), "value": round(W * H * args.aa / (ms_b * 1e-3) / 1e6, 3), "unit": "Mray/s",
                       "frames_identical_to_the_timed_build": same,
                       "note": "one launch, grid.z = frame, a uniform block per slice (FLAG_SLICES); kernel time only, NOT the measured value above"}
            del sl_r, big, one
        except Exception as e:
            print(f"[bench] batched-launch timing unavailable: {e}", file=sys.stderr)

    # untimed, N = 1 only: the tolerance mode (FLAG_FAST_MATH) on the same frame: kernel time and how far its picture is from the exact one
    fast = None
    if args.full and world == 1 and not args.no_cpu_baseline:
        try:
            f32 = torch.empty((2, H, W, 4), dtype=torch.float32, device=dev)
            exact_r = pa.SceneRenderer(scene, device=local_rank, flags=spec_flags, **scene_kw)
            fast_r = pa.SceneRenderer(scene, device=local_rank, flags=spec_flags | pa.FLAG_FAST_MATH, **scene_kw)
            for k, rr in enumerate((exact_r, fast_r)):
                configure(rr, args)
                rr.draw_device(frame, out_rgba8=shard.data_ptr(), out_rgba32f=f32[k].data_ptr(), stream=stream.cuda_stream)
            for _ in range(8):
                fast_r.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream)
            fast_ms = float(np.median([fast_r.draw_device(frame, out_rgba8=shard.data_ptr(), stream=stream.cuda_stream, timed=True) for _ in range(16)]))
            torch.cuda.synchronize(dev)
            err = (f32[0, :, :, :3] - f32[1, :, :, :3]).abs().amax(dim=2)
            fast = {"kernel_ms": round(fast_ms, 4), "pixels_beyond_1e-5": int((err > 1e-5).sum().item()), "pixels": W * H,
                    "median_abs_error": float(err.median().item()), "note": "hardware rcp/sqrt estimates, a/b = a*rcp(b), FMA contraction; NOT the measured value above"}
            del f32, exact_r, fast_r
        except Exception as e:
            print(f"[bench] fast-math timing unavailable: {e}", file=sys.stderr)

    # untimed, N = 1 only: what the JIT of the timed build costs on a cold cache (child process, private empty cache, comgr cache off)
    jit_seconds = None
    jit_detail = None
    if args.full and world == 1 and rank == 0 and not args.no_cpu_baseline:
        try:
            import subprocess
            import tempfile

            child = ("import sys, time; sys.path.insert(0, sys.argv[1]); import portal_amd as pa; s = pa.Scene.from_file(sys.argv[2]); t = time.perf_counter(); "
                     "r = pa.SceneRenderer(s, device=-1, flags=int(sys.argv[3])); a = time.perf_counter() - t; t = time.perf_counter(); r.prebuild_teleport(); "
                     "print(a, time.perf_counter() - t)")

            def cold(**env):
                with tempfile.TemporaryDirectory() as tmp:
                    done = subprocess.run([sys.executable, "-c", child, HERE, scene_path, str(spec_flags | pa.flag_waves(best_waves))],
                                          env=dict(os.environ, PTL_CACHE_DIR=tmp, AMD_COMGR_CACHE="0", **env), capture_output=True, text=True, timeout=300)
                return [round(float(x), 3) for x in done.stdout.strip().splitlines()[-1].split()]

            shipped = cold()
            jit_seconds = shipped[0]
            classic = cold(PTL_ONE_MODULE="1", PTL_MODULE_INLINER="0")
            jit_detail = {"render_module": shipped[0], "teleport_module_on_first_query": shipped[1],
                          "one_module_bottom_up_inliner_as_in_round_3": classic[0],
                          "note": "cold hiprtc builds of the timed kernel's source at the shipped -O3 (child process, empty code-object cache, comgr cache off).  jit_seconds = the render "
                                  "module: what a renderer waits for before its first frame; the camera-teleport entry is a module of its own, built when a query first asks "
                                  "(or ahead: prebuild_teleport).  Kernels whose intersection-material snippet loops -- this scene -- are built with LLVM's module inliner "
                                  "(kernel.cpp compile_options); PTL_ONE_MODULE=1 PTL_MODULE_INLINER=0 is round 3's build of the same source"}
        except Exception as e:
            print(f"[bench] jit timing unavailable: {e}", file=sys.stderr)

    if rank == 0:
        if args.save_png:
            pa.png_write(args.save_png, final_image)
        rays = W * H * args.aa
        ms_per_step = elapsed / args.steps * 1e3
        value = rays * args.steps / elapsed / 1e6
        out = {
            "metric": f"Mray/s (primary rays) + ms/frame at {W}x{H}, {args.scene} depth={args.depth}" + (f" aa={args.aa}" if args.aa != 1 else ""),
            "value": round(value, 3),
            "unit": "Mray/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic: the reference's shipped scene file, no stage applied, camera from the scene `cam` block",
            "config": {
                "workload": f"{args.scene_file or 'scenes/' + args.scene + '.ron'} {W}x{H} aa={args.aa} depth={args.depth}"
                            + (f" panini d={args.panini} fov={args.fov}" if args.panini >= 0 else "") + (f" camera look_at,alpha,beta,r={args.camera}" if args.camera else ""),
                "trips_per_primary_ray": None,
                "parallelism": f"row-block interleave x{world}" + ("" if world == 1 else {
                    "rccl-gather": " + one RCCL gather to rank 0 + de-interleave copy, double-buffered (gather n overlaps trace n+1)",
                    "p2p-stores": " + kernel stores straight into rank 0's frame over xGMI (HIP IPC mapping), fenced by a 1-element RCCL all-reduce",
                    "p2p-copy": " + packed shard per rank and ONE strided peer copy each into rank 0's frame (HIP IPC mapping), fenced by a 1-element RCCL all-reduce"}[transport.name]),
                "jit_specialisation": ["none", "int/bool scene uniforms baked", "all scene uniforms baked (camera dynamic)"][args.specialize],
                **(in_flight if in_flight is not None else {"frames_in_flight": 1, **({"frames_in_flight_unavailable": lanes_failed} if lanes_failed else {})}),
                "build": best, "waves_per_simd_hint": best_waves,
                "tuning_ms": tuning,
                # every candidate build drew the same bytes as the first one (compared on the device before timing); a build that did not is named here and was not eligible
                "candidate_frames_identical": not frames_differ, "candidate_frame_sha256_16": candidate_sha,
                **({"candidates_excluded": frames_differ} if frames_differ else {}),
                **({"transport": transport.name, "transport_ms_per_frame": transport_ms, "transport_notes": transport_notes} if world > 1 else {}),
            },
        }
        if kernel_ms is not None:  # (a plain run with frames in flight or N > 1 does not time the kernel's launches on their own)
            out.update({
                "kernel_ms": round(kernel_ms, 4),
                "kernel_ms_from": kernel_ms_from,
                # per rank: the interleave's load balance; ms_per_step - max(kernel_ms_per_rank) = what assembling the frame costs on top of tracing
                "kernel_ms_per_rank": [round(x, 4) for x in per_rank_ms],
                "kernel_ms_min_max": [round(min(per_rank_ms), 4), round(max(per_rank_ms), 4)],
                "transport_ms": round(max(0.0, ms_per_step - max(per_rank_ms)), 4),
            })
        if frame_check is not None:
            out["frame_check"] = frame_check
        if second is not None:
            out["second_workload"] = second
        if others or second is not None:
            # every BASELINE.json config, the Panini variant and the deep view in ONE list (the C5 entry is `second_workload`, timed through the gather)
            out["workloads"] = ([dict(second, name="c5")] if second is not None else []) + others
        if jit_seconds is not None:
            out["jit_seconds"] = jit_seconds  # cold compile of the timed build's render module (hiprtc, -O3); cached on disk by source + options + toolchain hash afterwards
            if jit_detail is not None:
                out["jit_seconds_detail"] = jit_detail
        if batched is not None:
            out["several_frames_per_launch"] = batched
        if fast is not None:
            out["fast_math_mode"] = fast
        if dynamic_ms is not None:
            out["kernel_ms_without_jit_specialisation"] = round(dynamic_ms, 4)
            out["kernel_ms_without_jit_specialisation_build"] = dynamic_build
        if ints_ms is not None:
            out["kernel_ms_with_only_int_uniforms_baked"] = round(ints_ms, 4)
            out["kernel_ms_with_only_int_uniforms_baked_build"] = ints_build
        if patterns_ms is not None:
            out["kernel_ms_with_only_zero_patterns_and_mode_switches"] = round(patterns_ms, 4)  # no scene VALUE compiled in (FLAG_SPECIALIZE_PATTERNS)
            out["kernel_ms_with_only_zero_patterns_and_mode_switches_build"] = patterns_build
        timed_sha = renderer.code_object_sha256()
        out["config"]["code_object_sha256"] = timed_sha  # of the binary the timed region launched: what ties this line to stored PMC passes
        out["config"]["affine_rays"] = renderer.affine_rays()
        out["config"]["toolchain"] = pa.version()
        out["config"]["kernel_source_sha256"] = source_sha256(renderer)
        if args.full:  # rooflines, CPU baselines and the checkers: --full only
            launch_bytes = rows * W * 4  # RGBA8 stored by this rank's launch
            achieved = launch_bytes / (kernel_ms * 1e-3) / 1e9
            pmc, pmc_why = stored_pmc(args, best, timed_sha, out["config"]["kernel_source_sha256"])
            hbm = {
                "bound": "hbm", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6),
                "traffic": pmc["traffic"] if pmc else None,
                "note": "algorithmic bytes = the RGBA8 framebuffer store (4 B/pixel); constants and textures are cache-resident",
            }
            if segments is not None:
                out["config"]["trips_per_primary_ray"] = round(segments / rays, 4)
                out["segments_per_frame"] = segments
                out["segment_mray_s"] = round(segments / (ms_per_step * 1e-3) / 1e6, 3)
            fl = flops_per_segment(args, renderer.affine_rays())
            if segments is not None and fl:
                roof = valu_roofline(fl, pmc, segments, world, kernel_ms, hbm["traffic"], args.specialize)
                if pmc is None:
                    roof["pmc_unavailable"] = pmc_why
                out["roofline"] = roof
                out["roofline_hbm"] = hbm
                if batched is not None:  # the same instructions in less time: fraction and ceiling scale alike
                    ratio = kernel_ms / batched["kernel_ms_per_frame"]
                    batched["frac"] = round(roof["frac"] * ratio, 5)
                    if "frac_ceiling_valu_plus_fma" in roof:
                        batched["frac_ceiling_valu_plus_fma"] = round(roof["frac_ceiling_valu_plus_fma"] * ratio, 4)
            else:
                out["roofline"] = hbm
            if world == 1 and not args.no_cpu_baseline:
                try:
                    out["cpu_baseline"] = cpu_baseline(args, pa)
                except Exception as e:
                    out["cpu_baseline"] = {"error": str(e)[:300]}
                kept = []
                try:
                    out["cpu_baseline_reference_text"] = reference_text_baseline(args, pa, keep=kept)
                except Exception as e:
                    out["cpu_baseline_reference_text"] = {"error": str(e)[:300]}
                try:
                    if kept:
                        out["reference_text_check_of_the_timed_build"] = reference_text_check(args, pa, renderer, torch, dev, stream, kept)
                except Exception as e:
                    out["reference_text_check_of_the_timed_build"] = {"error": str(e)[:300]}
                try:
                    which = {"headline": dict(scene=args.scene, width=W, height=H, depth=args.depth, aa=args.aa)} if not (args.scene_file or args.camera or args.panini >= 0) else {}
                    if workload_key(args) == "portal_in_portal_3840x2160_d40" and not args.no_second_workload:
                        which["c5"] = WORKLOADS["c5"]
                    if which and args.specialize == 2:
                        out["contract1_vs_contract2"] = contract_distance(args, pa, torch, dev, stream, local_rank, spec_flags, which)
                except Exception as e:
                    out["contract1_vs_contract2"] = {"error": str(e)[:300]}
                try:
                    out["oracle_check_of_the_timed_build"] = oracle_check(args, pa, renderer, torch, dev, stream)
                except Exception as e:
                    out["oracle_check_of_the_timed_build"] = {"error": str(e)[:300]}
        emit(out, full=args.full)
    transport.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
