"""The committed measurement records of the current round are self-consistent: no roofline object under profiles/r04/ claims
more than its own hardware ceiling, every workload whose roofline bench.py prints has stored PMC class counters, and the checks the bench line
carries about the build it timed are green in the record."""
import glob
import json
import os

import pytest

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R04 = os.path.join(HERE, "profiles", "r04")


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.startswith("{")]


def _rooflines():
    out = []
    for path in [os.path.join(R04, "bench_pip4k_1gpu.json"), os.path.join(R04, "bench_other_configs_1gpu.jsonl")]:
        for d in _lines(path):
            out.append((os.path.basename(path) + ": " + d["config"]["workload"], d["roofline"]))
            if "second_workload" in d and "roofline" in d["second_workload"]:
                out.append((os.path.basename(path) + ": second workload " + d["second_workload"]["workload"], d["second_workload"]["roofline"]))
    return out


def test_no_printed_roofline_exceeds_its_own_instruction_ceiling():
    found = _rooflines()
    assert len(found) >= 6  # headline + its second workload, C2, Panini, C3, C5
    for what, r in found:
        assert r["bound"] == "valu" and r["peak"] == 157.3 and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-4, what
        assert "pmc_source" in r and "frac_ceiling_valu_plus_fma" in r, f"{what}: no stored PMC class counters"
        assert r["frac"] <= r["frac_ceiling_valu_plus_fma"] + 1e-9, what
        assert r["hw_flops_frac"] <= r["frac_ceiling_valu_plus_fma"], what
        assert 0.9 < r["lane_utilisation"] <= 1.0, what


def test_pmc_files_cover_every_bench_workload_with_all_counter_classes():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(R04, "pmc_*.json")))
    for key in ("portal_in_portal_3840x2160_d40_spec", "monoportal_1920x1080_d20_spec", "triple_portal_3840x2160_d40_spec", "mobius_monoportal_7680x4320_d64_aa4_spec",
                "portal_in_portal_3840x2160_d40_panini_spec"):
        mine = [n for n in names if n.startswith("pmc_" + key + "_")]
        assert mine, key
        c = json.load(open(os.path.join(R04, mine[0])))["counters"]
        for k in ("SQ_INSTS_VALU", "SQ_INSTS_VALU_FMA_F32", "SQ_INSTS_VALU_MUL_F32", "SQ_INSTS_VALU_ADD_F32", "SQ_INSTS_VALU_TRANS_F32", "SQ_INSTS_VALU_INT32", "GRBM_GUI_ACTIVE",
                  "SQ_THREAD_CYCLES_VALU", "SQ_ACTIVE_INST_VALU", "FETCH_SIZE", "WRITE_SIZE"):
            assert c[k]["mean_per_launch"] > 0, (key, k)


def test_the_headline_record_carries_green_checks_of_the_timed_build():
    d = _lines(os.path.join(R04, "bench_pip4k_1gpu.json"))[-1]
    assert d["unit"] == "Mray/s" and d["dtype"] == "f32" and d["n_gpus"] == 1 and d["config"]["workload"].startswith("scenes/portal_in_portal.ron 3840x2160")
    assert d["kernel_ms"] <= d["ms_per_step"] and abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    assert d["config"]["candidate_frames_identical"]
    for key in ("oracle_check_of_the_timed_build", "reference_text_check_of_the_timed_build"):
        c = d[key]
        assert c["bit_exact"] and c["float_bits_equal"] == c["pixels"] == c["rgba8_equal"], key
    assert d["reference_text_check_of_the_timed_build"]["pixels"] >= 100_000
    dist = d["contract1_vs_contract2"]
    assert dist["headline"]["pixels"] == 3840 * 2160 and dist["headline"]["pixels_beyond_1e-5"] < 100
    assert dist["c5"]["pixels"] == 7680 * 4320 and dist["c5"]["pixels_beyond_1e-5"] / dist["c5"]["pixels"] < 0.01
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    # the rocprofv3 kernel trace of the same command agrees with the HIP-event kernel time (within 3 %)
    import csv

    rows = list(csv.DictReader(open(os.path.join(R04, "kernel_stats_pip4k_bench.csv"))))
    render = [r for r in rows if r["Name"] == "ptl_render_kernel"][0]
    assert abs(float(render["AverageNs"]) * 1e-6 - d["kernel_ms"]) / d["kernel_ms"] < 0.03


# ---- round 5 -----------------------------------------------------------------------------------------------------------------------------
R05 = os.path.join(HERE, "profiles", "r05")


def test_round5_rooflines_are_what_the_hardware_counted_for_the_timed_binary():
    """`frac` = min(the oracle's count, the hardware's FP32 arithmetic counters), the counters taken from PMC passes of the very
    code object the line timed (sha256 in the line and in the PMC file)."""
    d = _lines(os.path.join(R05, "bench_pip4k_1gpu.json"))[-1]
    found = [("headline", d["roofline"], d["config"]["code_object_sha256"])] + [(w["name"], w["roofline"], w["code_object_sha256"]) for w in d["workloads"]]
    assert {"c5", "c2", "c3", "c4-panini", "c4-deep", "recursive-room"} <= {name for name, _, _ in found}
    for name, r, sha in found:
        assert r["bound"] == "valu" and r["peak"] == 157.3 and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-4, name
        assert "pmc_unavailable" not in r and r["pmc_code_object_sha256"] == sha and len(sha) == 64, name
        pmc = json.load(open(os.path.join(HERE, r["pmc_source"].split(" ")[0])))
        assert pmc["code_object_sha256"] == sha, name
        assert r["frac"] <= r["hw_arith_frac"] + 1e-4 and r["frac"] <= r["frac_counted_by_the_oracle"] + 1e-9, name
        assert 0.85 < r["lane_utilisation"] <= 1.0, name


def test_round5_headline_record():
    d = _lines(os.path.join(R05, "bench_pip4k_1gpu.json"))[-1]
    start = _lines(os.path.join(R05, "bench_pip4k_start_of_round.json"))[-1]
    assert d["unit"] == "Mray/s" and d["dtype"] == "f32" and d["n_gpus"] == 1 and d["config"]["workload"].startswith("scenes/portal_in_portal.ron 3840x2160")
    assert d["kernel_ms"] <= d["ms_per_step"] <= 0.235 and d["ms_per_step"] < 0.8 * start["ms_per_step"]   # the round's target, and what the round bought
    assert abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    assert d["config"]["candidate_frames_identical"] and d["config"]["affine_rays"] is True
    for key in ("oracle_check_of_the_timed_build", "reference_text_check_of_the_timed_build"):
        c = d[key]
        assert c["bit_exact"] and c["float_bits_equal"] == c["pixels"] == c["rgba8_equal"], key
    assert d["reference_text_check_of_the_timed_build"]["pixels"] >= 100_000
    assert d["roofline"]["valu_insts_per_launch"] <= 140e6
    assert d["kernel_ms_with_only_int_uniforms_baked"] <= 0.28 and d["kernel_ms_with_only_zero_patterns_and_mode_switches"] <= 0.38   # VERDICT r4 #5 (the un-specialised kernel: DESIGN 7)
    # every workload of the line: timed, checked against the oracle on the frame of the build that was timed, with a CPU baseline beside it
    deep = 0.0
    for w in d["workloads"]:
        assert w["ms_per_step"] > 0 and w["oracle_check"]["bit_exact"] and w["oracle_check"]["pixels"] >= 2048, w["name"]
        assert w["cpu_baseline"]["value"] > 0 and w["cpu_baseline"]["kind"] == "port", w["name"]
        deep = max(deep, w["trips_per_primary_ray"])
    assert deep >= 5.0   # "depth = 40" exercised by a driver-timed number
    import csv

    rows = list(csv.DictReader(open(os.path.join(R05, "kernel_stats_pip4k_bench.csv"))))
    render = [r for r in rows if r["Name"] == "ptl_render_kernel"][0]
    # (the trace averages over the launches of ALL candidate builds of the run, a few per cent apart; the line's kernel_ms is the timed build's)
    assert abs(float(render["AverageNs"]) * 1e-6 - d["kernel_ms"]) / d["kernel_ms"] < 0.06


def test_round5_gpu_suite_and_clip_records():
    log = open(os.path.join(R05, "pytest_gpu.log")).read()
    assert " passed in " in log and "failed" not in log
    video = open(os.path.join(R05, "video_pip_intro1_4k_aa4_blur4.log")).read()
    assert video.count("0a12fb7adceb7b222b1550613d9e3123") == 2   # both builds write the frames of rounds 3 and 4
    import re

    per_subframe = [float(x) for x in re.findall(r"\((\d+\.\d+) ms each\)", video)]
    assert len(per_subframe) == 2 and per_subframe[0] < 0.7 and per_subframe[1] <= 1.4   # clip-specialised; the patterns kernel


# ---- round 6 -----------------------------------------------------------------------------------------------------------------------------
def test_the_stdout_line_stays_small_enough_for_the_driver():
    """round 5's line had grown to 32 KB and came back `parsed: null`.  bench.py now prints `compact_line(detail)`; fed round 5's
    own 32 KB record -- and the same record dressed up as an 8-rank run -- it stays under 4 KB and keeps every key of the contract."""
    import sys

    sys.path.insert(0, HERE)
    import bench

    d = _lines(os.path.join(R05, "bench_pip4k_1gpu.json"))[-1]
    assert len(json.dumps(d)) > 30_000
    eight = json.loads(json.dumps(d))
    eight.update(n_gpus=8, kernel_ms_per_rank=[0.0301 + 0.0001 * k for k in range(8)], frame_check={"last_timed_frame_equals_the_frame_rendered_by_rank0_alone": True})
    eight["config"].update(transport="rccl-gather", parallelism="row-block interleave x8 + one RCCL gather to rank 0 + de-interleave copy, double-buffered (gather n overlaps trace n+1)")
    eight["workloads"][0]["kernel_ms_per_rank"] = [1.6123 + 0.001 * k for k in range(8)]
    for rec in (d, eight):
        text = bench.compact_line(rec)
        assert len(text) <= bench.COMPACT_LINE_LIMIT and "\n" not in text
        line = json.loads(text)
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert key in line, key
        assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and line["roofline"]["pmc_code_object_sha256"] == line["config"]["code_object_sha256"]
        assert set(line["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"} and "workload" in line["config"] and "model" not in line["config"]
        assert line["parity"]["timed_build_vs_reference_text"] == {"pixels": 106496, "bit_exact": True, "max_abs_error": 0.0}
        assert [w["id"] for w in line["workloads"]] == ["c5", "c2", "c3", "c4-panini", "c4-deep", "recursive-room"] and all(w["bit_exact"] for w in line["workloads"])
        assert "dropped_for_size" not in line
    assert json.loads(bench.compact_line(eight))["kernel_ms_per_rank"] == eight["kernel_ms_per_rank"]
    # ... and a record that outgrows the limit anyway loses its extras, never its parseability
    fat = json.loads(json.dumps(d))
    fat["workloads"] = fat["workloads"] * 12
    text = bench.compact_line(fat)
    assert len(text) <= bench.COMPACT_LINE_LIMIT and "workloads" in json.loads(text)["dropped_for_size"] and "roofline" in json.loads(text)


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run's record (no --full: no roofline, no detail record) still gives the contract's keys and no pointer to a detail file; --dump-outputs
    writes a frame that fits in 64 MB of float32 whole and a 4K frame as the same seeded pixel sample every time, its values those of the frame."""
    import sys

    import numpy as np

    sys.path.insert(0, HERE)
    import bench

    plain = {"metric": "Mray/s (primary rays) + ms/frame at 3840x2160, portal_in_portal depth=40", "value": 46000.0, "unit": "Mray/s", "n_gpus": 1, "steps": 20,
             "warmup": 5, "ms_per_step": 0.18, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
             "config": {"workload": "scenes/portal_in_portal.ron 3840x2160 aa=1 depth=40", "build": "w0", "frames_in_flight": 2}}
    line = json.loads(bench.compact_line(plain, detail=False))
    assert {k: line[k] for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "steps")} == {k: plain[k] for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "steps")}
    assert "roofline" not in line and "detail" not in line and line["config"]["frames_in_flight"] == 2
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (720, 1280, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "small"), small)
    assert os.listdir(tmp_path / "small") == ["frame_rgba8.npy"] and np.array_equal(np.load(tmp_path / "small" / "frame_rgba8.npy"), small.astype(np.float32))
    big = rng.integers(0, 256, (2160, 3840, 4), dtype=np.uint8)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["frame_rgba8_sample.npy", "frame_rgba8_sample_pixels.npy"] and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got, pixels = np.load(tmp_path / "a" / files[0]), np.load(tmp_path / "a" / files[1])
    assert got.dtype == np.float32 and pixels.dtype == np.float64 and got.shape == (bench.DUMP_SAMPLE_PIXELS, 4) and len(np.unique(pixels)) == len(pixels)
    assert np.array_equal(got, big.reshape(-1, 4)[pixels.astype(np.int64)].astype(np.float32))
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in files)


R06 = os.path.join(HERE, "profiles", "r06")


def test_round6_records_of_the_driver_command_and_the_default_run():
    """The committed round-6 lines: what the driver reads (the compact stdout line: <= 4 KB, the contract's keys, `roofline` and `cpu_baseline` inside) and the
    detail record beside it -- two frames in flight in the timed region, compared inside the run with the frame drawn alone; `kernel_ms` from the one-stream
    pass right behind it, which is what the rocprofv3 trace of the one-stream command measures per dispatch; every workload bit-exact."""
    import csv

    for name in ("driver_command", "pip4k_1gpu"):
        text = open(os.path.join(R06, f"bench_{name}.json")).read().strip().splitlines()[-1]
        assert len(text) <= 4096, (name, len(text))
        line = json.loads(text)
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert key in line, (name, key)
        assert line["n_gpus"] == 1 and line["unit"] == "Mray/s" and line["dtype"] == "f32" and line["steps"] == (20 if name == "driver_command" else 400)
        assert abs(line["value"] - 3840 * 2160 / (line["ms_per_step"] * 1e-3) / 1e6) / line["value"] < 1e-3
        cfg = line["config"]
        assert cfg["frames_in_flight"] == 2 and cfg["frames_identical_to_one_in_flight"] is True
        assert line["ms_per_step"] < cfg["ms_per_step_one_frame_in_flight"] <= 0.20   # what two frames in flight buy (headline <= 0.183)
        assert line["ms_per_step"] <= 0.183
        r = line["roofline"]
        assert r["bound"] == "valu" and r["pmc_match"] == "code object" and r["pmc_code_object_sha256"] == cfg["code_object_sha256"] and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-4
        assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] >= 1 and line["cpu_baseline"]["value"] > 0
        assert line["parity"]["timed_build_vs_reference_text"]["bit_exact"] and line["parity"]["timed_build_vs_reference_text"]["pixels"] >= 100_000
        assert line["parity"]["timed_build_vs_oracle"]["bit_exact"]
        rows = {w["id"]: w for w in line["workloads"]}
        assert {"c5", "c2", "c3", "c4-panini", "c4-deep", "recursive-room"} <= set(rows)
        assert all(w["bit_exact"] and w["in_flight"] == (1 if w["id"] == "c5" else 2) for w in rows.values())   # (C5's 12.5 ms launches gain nothing from a second in flight)
        assert rows["c2"]["ms_per_step"] <= 0.033
        d = json.load(open(os.path.join(R06, f"bench_detail_{name}.json")))
        assert d["kernel_ms"] == line["kernel_ms"] and d["value"] == line["value"] and "one stream" in d["kernel_ms_from"]
        for w in d["workloads"]:
            if w["name"] != "c5":
                assert w["frames_identical_to_one_in_flight"] is True and w["ms_per_step"] <= w["ms_per_step_one_frame_in_flight"] * 1.01, w["name"]
        assert d["kernel_ms_without_jit_specialisation"] <= 0.65   # round 5: 0.676 (first-trip forms out of the un-specialised kernel)
    # the rocprofv3 per-dispatch average of the ONE-STREAM command agrees with the line's kernel_ms (the trace averages over the candidate builds too)
    line = json.loads(open(os.path.join(R06, "bench_pip4k_1gpu.json")).read().strip().splitlines()[-1])
    render = [r for r in csv.DictReader(open(os.path.join(R06, "kernel_stats_pip4k_bench_one_stream.csv"))) if r["Name"] == "ptl_render_kernel"][0]
    assert abs(float(render["AverageNs"]) * 1e-6 - line["kernel_ms"]) / line["kernel_ms"] < 0.04
    log = open(os.path.join(R06, "pytest_gpu.log")).read()
    assert " passed in " in log and "failed" not in log


def test_round6_store_pattern_reaches_the_north_star_target_with_two_launches_in_flight():
    """N-star: >= 60 % of 8 TB/s on the framebuffer write at 4K -- the store pattern alone, persistent grid, 16 B per lane, two launches in flight."""
    rows = _lines(os.path.join(R06, "fb_store_4k_in_flight.jsonl"))
    best = max(r["frac_of_8TB/s_two_in_flight"] for r in rows if r["bytes"] == 3840 * 2160 * 4)
    assert best >= 0.60
    assert all(r["frac_of_8TB/s_two_in_flight"] >= r["frac_of_8TB/s_queued_one_stream"] for r in rows if r["bytes"] > 0 and "workgroups" not in r)
