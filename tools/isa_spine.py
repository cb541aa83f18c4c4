#!/usr/bin/env python3
"""tools/isa_spine.py -- the SPINE of a scene snippet: the instructions every wave executes between the conditional regions of one stage.

    python tools/isa_spine.py [--scene portal_in_portal] [--flags 5] [--waves 5] [--stage intersect_material_0 | trace_segment | pack_rgba8 | shade_pixel]
                              [--hiprtc-flags=-DPTL_EARLY_RETURN_HITS] [--out profiles/r07/isa_spine_<tag>.json]

A snippet loop that the generator unrolls is a chain of candidates: per iteration a plane test, then `if (nearer(best, hit)) { ... }`, a
branch most waves skip (`s_cbranch_execz`).  What a wave pays for a candidate it does NOT take is the straight-line code up to that branch.
The tool builds the kernel a SceneRenderer with those flags would draw with, once more with `-gline-tables-only` (like tools/isa_lines.py: the
instruction stream is checked to be the shipped one), keeps the instructions whose inline chain passes through `--stage`, drops every
instruction that a forward branch of the stage jumps over (the conditional regions), and cuts what is left -- the code every wave executes --
at each remaining forward conditional branch.  Per segment: the source line of the closing branch (the `if` it belongs to) and the
instruction classes of tools/isa_hist.py.  Consecutive segments closing on the same line are the iterations of an unrolled loop; the summary
gives the median per closing line.  `--stage` also takes a function of the template itself (trace_segment, pack_rgba8, shade_pixel: what OUR
text makes every wave execute, whatever it inlines); the code after the last branch of a stage is its last segment, and the totals line gives
the stage's size and the sum of its always-executed segments.  STATIC counts, mnemonic classes only; no GPU needed."""
from __future__ import annotations

import argparse
import collections
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
from isa_hist import OBJDUMP, classify  # noqa: E402
from isa_lines import build, chains  # noqa: E402

CLASSES = ("valu_fp32_arith", "valu_transcendental", "valu_move", "valu_compare", "valu_select")


def instructions(code, kernel):
    """[(address, mnemonic, branch target or None)] of one kernel symbol, and the path of the temporary code object."""
    with tempfile.NamedTemporaryFile(suffix=".hsaco", delete=False) as f:
        f.write(code)
        path = f.name
    text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f"--disassemble-symbols={kernel}", path], capture_output=True, text=True, check=True).stdout
    base = next(int(m.group(1), 16) for m in (re.match(r"^([0-9a-f]+) <" + re.escape(kernel) + ">:", ln) for ln in text.splitlines()) if m)
    out = []
    for line in text.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)\b.*//\s*([0-9A-F]{8,}):", line)
        if not m:
            continue
        t = re.search(r"<" + re.escape(kernel) + r"\+0x([0-9a-f]+)>\s*$", line) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
        out.append((int(m.group(2), 16), m.group(1), base + int(t.group(1), 16) if t else None))
    return out, path


def spine(ins, where, stage, src_lines):
    """The segments of `stage`'s always-executed code: [{closing branch, its line, class counts}]."""
    def unit_line(adr):
        return next((ln for f, ln, _ in where.get(adr, []) if f == stage), 0)  # the line of the stage's OWN text (not of what it inlined)

    inside = [(a, m, t) for a, m, t in ins if any(f == stage for f, _, _ in where.get(a, []))]
    skipped = [(a, t) for a, m, t in inside if t is not None and t > a]  # forward branches of the stage: (a, t) may not execute
    segments, cur = [], collections.Counter()
    for a, m, t in inside:
        if any(b < a < e for b, e in skipped):
            continue
        if t is not None and t > a and m != "s_branch":
            ln = unit_line(a)
            valu = sum(c for k, c in cur.items() if k.startswith("valu_"))
            segments.append({"closing_branch": m, "line": ln, "text": src_lines[ln - 1].strip()[:110] if 0 < ln <= len(src_lines) else "", "valu": valu,
                             **{k[5:]: cur[k] for k in CLASSES}, "valu_other": valu - sum(cur[k] for k in CLASSES), "salu": cur["salu"]})
            cur = collections.Counter()
            continue
        cur[classify(m)] += 1
    if cur:  # what follows the last branch -- for a stage without a conditional region (the template's pack_rgba8, say) the whole stage
        valu = sum(c for k, c in cur.items() if k.startswith("valu_"))
        segments.append({"closing_branch": "(end of stage)", "line": 0, "text": "", "valu": valu, **{k[5:]: cur[k] for k in CLASSES},
                         "valu_other": valu - sum(cur[k] for k in CLASSES), "salu": cur["salu"]})
    return segments


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="portal_in_portal")
    ap.add_argument("--flags", type=int, default=5)
    ap.add_argument("--waves", type=int, default=5)
    ap.add_argument("--kernel", default="ptl_render_kernel")
    ap.add_argument("--stage", default="intersect_material_0")
    ap.add_argument("--hiprtc-flags", default="", help="extra compile options of BOTH builds (an A/B define such as -DPTL_EARLY_RETURN_HITS)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import portal_amd as pa

    flags = a.flags | pa.flag_waves(a.waves)
    scene_path = pa.scene_path(a.scene)
    with tempfile.TemporaryDirectory() as cache:  # caches of their own, as in isa_lines.py
        shipped, source = build(scene_path, flags, {"PTL_HIPRTC_FLAGS": a.hiprtc_flags, "PTL_CACHE_DIR": os.path.join(cache, "a")})
        lined, _ = build(scene_path, flags, {"PTL_HIPRTC_FLAGS": (a.hiprtc_flags + " -gline-tables-only").strip(), "PTL_CACHE_DIR": os.path.join(cache, "b")})
    ins_shipped, p0 = instructions(shipped, a.kernel)
    ins, path = instructions(lined, a.kernel)
    os.unlink(p0)
    same_stream = [m for _, m, _ in ins] == [m for _, m, _ in ins_shipped]
    where = chains(path, [adr for adr, _, _ in ins])
    os.unlink(path)
    segments = spine(ins, where, a.stage, source.splitlines())
    per_line = collections.defaultdict(list)
    for s in segments:
        per_line[s["line"]].append(s)
    summary = []
    for ln, ss in sorted(per_line.items(), key=lambda kv: -len(kv[1])):
        summary.append({"line": ln, "text": ss[0]["text"], "segments": len(ss), **{k: statistics.median(s[k] for s in ss) for k in ("valu", "fp32_arith", "move", "compare", "select", "salu")},
                        "valu_min": min(s["valu"] for s in ss), "valu_max": max(s["valu"] for s in ss)})
    in_stage = [m for adr, m, _ in ins if any(f == a.stage for f, _, _ in where.get(adr, []))]
    always = {"valu": sum(s["valu"] for s in segments), "salu": sum(s["salu"] for s in segments), "branches": sum(1 for s in segments if s["closing_branch"].startswith("s_"))}
    result = {"build": f"{os.path.relpath(scene_path, HERE)} flags={a.flags} waves={a.waves} {a.hiprtc_flags}".strip(), "kernel": a.kernel, "stage": a.stage, "instructions": len(ins),
              "stage_instructions": len(in_stage), "stage_branches": sum(1 for m in in_stage if classify(m) == "branch"), "always_executed": always,
              "same_instruction_stream_as_the_shipped_build": same_stream, "median_per_closing_line": summary, "segments": segments}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(f"{result['build']}: {len(ins)} instructions; same stream as the shipped build: {same_stream}; {len(segments)} always-executed segments of {a.stage}")
    print(f"  {a.stage}: {len(in_stage)} instructions, {result['stage_branches']} branches; always executed: {always['valu']} VALU, {always['salu']} SALU, {always['branches']} conditional branches")
    for s in summary:
        print(f"  line {s['line']:5d} x{s['segments']:2d}  median VALU {s['valu']:5.1f} ({s['valu_min']}..{s['valu_max']})  arith {s['fp32_arith']:4.1f}  mov {s['move']:4.1f}  cmp {s['compare']:4.1f}  "
              f"sel {s['select']:4.1f}  salu {s['salu']:4.1f} | {s['text']}")


if __name__ == "__main__":
    main()
