#!/usr/bin/env python3
"""tools/source_matrix.py -- what the kernel generator hands out, as a manifest of hashes (development aid, no GPU).

A change to the generator that is meant to leave the generated sources alone is shown to do so by running this tool on both
commits and comparing the two manifests with `diff`:

    python3 tools/source_matrix.py sources before.jsonl      (in a worktree of the parent, with this file copied in)
    python3 tools/source_matrix.py sources after.jsonl
    python3 tools/source_matrix.py objects before_obj.jsonl  (slow: twenty hiprtc builds; give each side an empty PTL_CACHE_DIR)

`sources`: for every scene of tests/corpus/scenes/*.ron, every base and every variant below, one JSON line with the sha256 of the
generated text and the sha256 of the text NORMALISED -- comments removed, every run of white space one space: two sources with the
same normalised hash are the same tokens in the same order -- or the message with which the generator refuses the combination.
Then one line per text of `ptl_device_source` that tests and tools paste into hand-written kernels.

`objects`: two scenes, the five flagged variants, FLAG_QUICK_JIT with and without baked values, compiled for gfx950 without a
device: sha256 of the disassembly (`llvm-objdump -d --no-show-raw-insn`) and the kernel's registers / scratch / LDS.  The bytes of
the code object are not compared: they hold an id the compiler derives from the text, comments and line breaks included.
"""
import glob, hashlib, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_STRIP = re.compile(r'"(?:[^"\\\n]|\\.)*"|/\*.*?\*/|//[^\n]*', re.S)


def normalised(text: str) -> str:
    text = _STRIP.sub(lambda m: m.group(0) if m.group(0)[0] == '"' else " ", text)
    return re.sub(r"\s+", " ", text).strip()


def sha(text) -> str:
    return hashlib.sha256(text if isinstance(text, bytes) else text.encode("utf-8")).hexdigest()


def bases(pa):
    return [("0", 0), ("ints", pa.FLAG_SPECIALIZE_INTS), ("ints|all", pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL), ("static", pa.FLAG_SPECIALIZE_STATIC),
            ("patterns", pa.FLAG_SPECIALIZE_PATTERNS)]  # (any specialisation switches KernelOptions::mask_zero_elements on; this is the one left)


def variants(pa):
    return [("none", 0), ("slices", pa.FLAG_SLICES), ("passes", pa.FLAG_PASSES), ("slices|passes", pa.FLAG_SLICES | pa.FLAG_PASSES), ("refine", pa.FLAG_REFINE),
            ("refine_slices", pa.FLAG_REFINE_SLICES)]


def sources(pa, out):
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "corpus", "scenes", "*.ron"))):
        name = os.path.splitext(os.path.basename(path))[0]
        for base_name, base in bases(pa):
            for variant_name, variant in variants(pa):
                line = {"scene": name, "base": base_name, "variant": variant_name, "flags": base | variant}
                try:
                    text = pa.Scene.from_file(path).generate_source(base | variant)
                    line.update(sha256=sha(text), normalised_sha256=sha(normalised(text)))
                except pa.PortalError as e:
                    line["error"] = str(e)
                out.write(json.dumps(line) + "\n")
    for which in ("glsl", "library", "entry", "refine_entry", "refine_slices_entry"):
        out.write(json.dumps({"device_source": which, "sha256": sha(pa.device_source(which))}) + "\n")


def objects(pa, out):
    objdump = next(p for p in ("/opt/rocm/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objdump", "llvm-objdump") if p == "llvm-objdump" or os.path.exists(p))
    for name in ("basics", "portal_in_portal"):
        for base_name, base in (("quick", pa.FLAG_QUICK_JIT), ("quick|ints|all", pa.FLAG_QUICK_JIT | pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL)):
            for variant_name, variant in variants(pa)[1:]:
                r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(name)), device=-1, flags=base | variant)
                with tempfile.NamedTemporaryFile(suffix=".co") as f:
                    f.write(r.code_object())
                    f.flush()
                    asm = subprocess.run([objdump, "-d", "--no-show-raw-insn", f.name], check=True, capture_output=True).stdout
                asm = b"\n".join(l for l in asm.split(b"\n") if b"file format" not in l)  # (the one line that names the temporary file)
                line = {"scene": name, "base": base_name, "variant": variant_name, "disassembly_sha256": sha(asm), "instructions": asm.count(b"\n"), **r.resources()}
                out.write(json.dumps(line) + "\n")
                out.flush()


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("sources", "objects"):
        sys.exit(__doc__)
    import portal_amd as pa

    with open(sys.argv[2], "w") as out:
        (sources if sys.argv[1] == "sources" else objects)(pa, out)
