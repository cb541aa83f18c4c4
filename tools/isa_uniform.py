#!/usr/bin/env python3
"""tools/isa_uniform.py -- the VALU instructions of a generated kernel that compute the same value on all 64 lanes.

    python tools/isa_uniform.py [--scene portal_in_portal] [--flags 5] [--waves 5] [--out profiles/r26/isa_uniform_<tag>.json] [--top 25]

Builds the kernel like tools/isa_lines.py (the shipped build and the same source with `-gline-tables-only`; the instruction streams are
compared), disassembles `ptl_render_kernel` with its operands and walks every straight-line region forwards: a VALU instruction is
FRAME-UNIFORM when each of its source operands is an SGPR, a literal, an inline constant, or a VGPR (or lane mask) that an instruction
already classed uniform wrote earlier in the same region.  A region ends at a branch, at a branch target and wherever the exec mask is
written -- behind those a register may hold other values in lanes that were switched off when it was written.  Nothing the tile's
`threadIdx` feeds can qualify: no VGPR counts as uniform at the start of a region, and the instructions that read the lane number or move
values between lanes (v_mbcnt, DPP, SDWA, lane reads and writes) never do.  The walk is conservative: it misses uniform values that cross
a region boundary, it never claims a lane-varying one.

Each such instruction is booked -- as isa_lines.py books all of them -- to its stage, its innermost function and its line of the generated
unit, with the issue price of its class (profiles/r01/valu_rates.jsonl: fma / mul / add / mov / integer 2.3 cycles per wave instruction,
compares, `v_med3`, floor, min / max, conversions 4.3, `v_rcp` / `v_sqrt` / `v_rsq` 8.25).  Instructions inside the scene's snippets
(`intersect_material_N`, `is_inside_N`, `intersect_N` and what they call) are totalled apart: their uniform-only expressions belong to
host/glsl_hoist.h.  STATIC counts, JSON, no GPU needed."""
from __future__ import annotations

import argparse
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
from isa_hist import OBJDUMP, classify  # noqa: E402
from isa_lines import CARRIERS, build, chains  # noqa: E402

PRICE = {"valu_transcendental": 8.25, "valu_compare": 4.3, "valu_fp_other": 4.3}  # every other class: 2.3
SNIPPET = re.compile(r"^(intersect_material_\d+|is_inside_\d+|intersect_\d+)")
TWO_RESULTS = re.compile(r"^v_((add|sub|subrev|addc|subb|subbrev)_co_|div_scale_|mad_(u64_u32|i64_i32))")
MASK_LAST = re.compile(r"^v_(cndmask|addc_co|subb_co|subbrev_co)_")  # the last source is a lane mask
CROSS_LANE = re.compile(r"^v_(mbcnt|readlane|readfirstlane|writelane|permlane|swap|interp|mov_b32_dpp)|_dpp$|_sdwa$")
REG = re.compile(r"^([vs])(?:(\d+)|\[(\d+):(\d+)\])$")


def price(cls):
    return PRICE.get(cls, 2.3)


def listing(code, kernel):
    """[(address, mnemonic, operand text)] of one kernel symbol, and the addresses branches jump to."""
    with tempfile.NamedTemporaryFile(suffix=".hsaco", delete=False) as f:
        f.write(code)
        path = f.name
    text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f"--disassemble-symbols={kernel}", path], capture_output=True, text=True, check=True).stdout
    base = None
    out, targets = [], set()
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <" + re.escape(kernel) + ">:", line)
        if m:
            base = int(m.group(1), 16)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b(.*?)//\s*([0-9A-F]{8,}):(.*)$", line)
        if not m:
            continue
        out.append((int(m.group(3), 16), m.group(1), m.group(2).strip()))
        t = re.search(r"<" + re.escape(kernel) + r"\+0x([0-9a-f]+)>", m.group(4))
        if t and base is not None:
            targets.add(base + int(t.group(1), 16))
    return out, targets, path


def operands(text):
    """-> ([operand], trailing modifiers) of an instruction's operand text"""
    text = re.sub(r"\b\w+:\[[^\]]*\]", " ", text)  # op_sel:[0,1] and its kin: modifiers with commas inside
    parts = [p.strip() for p in text.split(",")] if text.strip() else []
    mods = ""
    if parts:
        words = parts[-1].split()
        parts[-1], mods = (words[0], " ".join(words[1:])) if words else ("", "")
    return parts, mods


def registers(op):
    """('v' | 's', {register numbers}) of a register operand, (None, set()) of anything else; sign and abs wrappers are looked through"""
    op = op.strip()
    op = re.sub(r"^(?:neg|abs|sext)\((.*)\)$", r"\1", op)
    op = op.lstrip("-").strip("|")
    op = re.sub(r"^(?:neg|abs|sext)\((.*)\)$", r"\1", op)
    m = REG.match(op)
    if not m:
        return None, set()
    if m.group(2) is not None:
        return m.group(1), {int(m.group(2))}
    return m.group(1), set(range(int(m.group(3)), int(m.group(4)) + 1))


def mask_name(op):
    return op.strip() if op.strip() in ("vcc", "vcc_lo", "vcc_hi") or op.strip().startswith("s") else None


def uniform_instructions(ins, targets):
    """The forward pass.  -> indices into `ins` of the frame-uniform VALU instructions."""
    uni_v, uni_mask = set(), set()  # VGPR numbers / lane-mask operands ("vcc", "s[4:5]") holding one value for the active lanes
    picked = []
    for k, (adr, mnem, text) in enumerate(ins):
        if adr in targets:
            uni_v.clear()
            uni_mask.clear()
        ops, mods = operands(text)
        cls = classify(mnem)
        if mnem.startswith("v_"):
            n_dst = 2 if TWO_RESULTS.match(mnem) else 1
            dsts, srcs = ops[:n_dst], ops[n_dst:]
            ok = not CROSS_LANE.search(mnem) and not re.search(r"\b(dpp|row_|quad_perm|wave_|bank_mask|src\d_sel|dst_sel)", mods) and bool(srcs)
            for j, s in enumerate(srcs):
                if not ok:
                    break
                kind, regs = registers(s)
                if MASK_LAST.match(mnem) and j == len(srcs) - 1:
                    ok = mask_name(s) in uni_mask
                elif kind == "v":
                    ok = regs <= uni_v
                elif kind is None and not re.match(r"^-?(0x[0-9a-f]+|\d+(\.\d+)?(e[-+]?\d+)?|lit\(.*\)|src_\w+|vcc|vcc_lo|vcc_hi|m0|scc)$", s.strip().strip("|").lstrip("-")):
                    ok = False  # exec, a symbol, anything this parser does not know: not claimed
            if mnem.startswith("v_div_fmas"):  # reads VCC without naming it
                ok = ok and "vcc" in uni_mask
            if mnem.startswith("v_cmpx") or any(d.strip().startswith("exec") for d in dsts):
                ok = False
            for d in dsts:
                kind, regs = registers(d)
                if kind == "v":
                    uni_v.difference_update(regs)
                    if ok:
                        uni_v.update(regs)
                else:
                    uni_mask.discard(d.strip())
                    if kind == "s":  # a scalar register (pair) rewritten: masks that overlap it are gone
                        for name in [n for n in uni_mask if registers(n)[1] & regs]:
                            uni_mask.discard(name)
                    if ok and cls == "valu_compare":
                        uni_mask.add(d.strip())
            if ok:
                picked.append(k)
        else:
            if ops:  # whatever a scalar or memory instruction names first may be its result
                kind, regs = registers(ops[0])
                if kind == "v":
                    uni_v.difference_update(regs)
                elif kind == "s":
                    for name in [n for n in uni_mask if registers(n)[1] & regs]:
                        uni_mask.discard(name)
                uni_mask.discard(ops[0].strip())
            if cls in ("vmem", "lds"):  # (loads with several results, returning atomics: every VGPR they name)
                for o in ops:
                    kind, regs = registers(o)
                    if kind == "v":
                        uni_v.difference_update(regs)
        writes_exec = "saveexec" in mnem or mnem.startswith("v_cmpx") or (bool(ops) and ops[0].strip().startswith("exec"))
        if cls == "branch" or writes_exec:
            uni_v.clear()
            uni_mask.clear()
    return picked


def analyse(scene_path, flags, kernel="ptl_render_kernel"):
    shipped, source = build(scene_path, flags, {})
    with tempfile.TemporaryDirectory() as cache:  # a cache of its own: the key does not know about PTL_HIPRTC_FLAGS of another process
        lined, _ = build(scene_path, flags, {"PTL_HIPRTC_FLAGS": "-gline-tables-only", "PTL_CACHE_DIR": cache})
    ins_shipped, _, p0 = listing(shipped, kernel)
    ins, targets, path = listing(lined, kernel)
    os.unlink(p0)
    same_stream = [(m, t) for _, m, t in ins] == [(m, t) for _, m, t in ins_shipped]
    picked = uniform_instructions(ins, targets)
    where = chains(path, [ins[k][0] for k in picked])
    os.unlink(path)
    src_lines = source.splitlines()

    def text_of(line_no):
        return src_lines[line_no - 1].strip()[:90] if 0 < line_no <= len(src_lines) else ""

    rows = []
    for k in picked:
        adr, mnem, text = ins[k]
        cls = classify(mnem)
        chain = where.get(adr) or [("?", 0, "?")]
        stage = next((f for f, _, _ in reversed(chain) if f not in CARRIERS), chain[-1][0])
        unit = next(((f, ln) for f, ln, file in chain if file.endswith("portal_scene.hip")), (chain[0][0], chain[0][1]))
        rows.append({"offset": adr - ins[0][0], "instruction": f"{mnem} {text}".strip(), "class": cls, "cycles": price(cls), "stage": stage, "line": unit[1],
                     "in_snippet": any(SNIPPET.match(f) for f, _, _ in chain),
                     # the inline chain through the generated unit, innermost first: which statement of which function the instruction serves
                     # (up to the pixel's shade_pixel: the entry around it is the same for every row)
                     "where": [f"{f}: {text_of(ln)}" for f, ln, file in chain if file.endswith("portal_scene.hip") and not text_of(ln).startswith(("return t.shade_pixel(", "if (live) c ="))]})

    def total(sel):
        by = collections.Counter(r["class"] for r in sel)
        return {"instructions": len(sel), "priced_cycles": round(sum(r["cycles"] for r in sel), 1), "by_class": dict(by.most_common())}

    def grouped(sel, key, extra=None):
        table = collections.defaultdict(list)
        for r in sel:
            table[r[key]].append(r)
        out = []
        for name, rs in sorted(table.items(), key=lambda kv: -sum(r["cycles"] for r in kv[1])):
            row = {key: name, **total(rs)}
            if extra:
                row.update(extra(name))
            out.append(row)
        return out

    outside = [r for r in rows if not r["in_snippet"]]
    valu = sum(1 for _, m, _ in ins if m.startswith("v_"))
    return {"build": f"{os.path.relpath(scene_path, HERE)} flags={flags}", "kernel": kernel, "code_object_sha256": hashlib.sha256(shipped).hexdigest(),
            "kernel_source_sha256": hashlib.sha256(source.encode("utf-8")).hexdigest(), "instructions": len(ins), "valu": valu,
            "same_instruction_stream_as_the_shipped_build": same_stream, "uniform_valu": total(rows), "uniform_valu_outside_snippets": total(outside),
            "uniform_valu_in_snippets": total([r for r in rows if r["in_snippet"]]), "outside_snippets_by_stage": grouped(outside, "stage"),
            "outside_snippets_by_line": grouped(outside, "line", lambda ln: {"text": text_of(ln)}),
            # moves of constants into registers are totalled above; what COMPUTES something is listed instruction by instruction
            "computing_outside_snippets": [{k: v for k, v in r.items() if k not in ("in_snippet", "line")} for r in outside if r["class"] != "valu_move"]}


def dump(result, f, top):
    """One line per scalar and per list element: a record a person can read and `diff` can compare."""
    result = dict(result, outside_snippets_by_line=result["outside_snippets_by_line"][:top])
    f.write("{\n")
    for n, (k, v) in enumerate(result.items()):
        end = ",\n" if n + 1 < len(result) else "\n"
        if isinstance(v, list):
            f.write(f" {json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(row) for row in v) + "\n ]" + end)
        else:
            f.write(f" {json.dumps(k)}: {json.dumps(v)}" + end)
    f.write("}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="portal_in_portal")
    ap.add_argument("--flags", type=int, default=5)
    ap.add_argument("--waves", type=int, default=5)
    ap.add_argument("--kernel", default="ptl_render_kernel")
    ap.add_argument("--out", default="")
    ap.add_argument("--top", type=int, default=25)
    a = ap.parse_args()
    import portal_amd as pa

    result = analyse(pa.scene_path(a.scene), a.flags | pa.flag_waves(a.waves), a.kernel)
    result["build"] += f" (= {a.flags} + waves {a.waves})"
    if a.out:
        with open(a.out, "w") as f:
            dump(result, f, a.top)
    u, o = result["uniform_valu"], result["uniform_valu_outside_snippets"]
    print(f"{result['build']}: {result['instructions']} instructions, {result['valu']} VALU; same stream as the shipped build: {result['same_instruction_stream_as_the_shipped_build']}")
    print(f"frame-uniform VALU: {u['instructions']} ({u['priced_cycles']} cycles), outside the scene's snippets {o['instructions']} ({o['priced_cycles']} cycles) {o['by_class']}")
    for r in result["outside_snippets_by_line"][: a.top]:
        print(f"  {r['line']:5d} {r['instructions']:4d} {r['priced_cycles']:7.1f} | {r['text']}")


if __name__ == "__main__":
    main()
