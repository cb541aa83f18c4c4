#!/usr/bin/env python3
"""tools/source_matrix.py -- what the kernel generator hands out, as a manifest of hashes (development aid, no GPU).

A change to the generator that is meant to leave the generated sources alone is shown to do so by running this tool on both
commits and comparing the two manifests with `diff`:

    python3 tools/source_matrix.py sources before.jsonl      (in a worktree of the parent, with this file copied in)
    python3 tools/source_matrix.py sources after.jsonl
    python3 tools/source_matrix.py programs before_programs.jsonl   (likewise on both sides; a manifest of its own: each stays a file of moderate size)
    python3 tools/source_matrix.py objects before_obj.jsonl  (slow: twenty hiprtc builds; give each side an empty PTL_CACHE_DIR)
    python3 tools/source_matrix.py digest before.jsonl       (prints the short form of a manifest, the one to keep under profiles/)
    python3 tools/source_matrix.py hoist_golden tests/golden/hoist/programs.json   (on the PARENT only: what a refactor of the hoister must reproduce)

`sources`: for every scene of tests/corpus/scenes/*.ron, every base and every variant below, one JSON line with the sha256 of the
generated text and the sha256 of the text NORMALISED -- comments removed, every run of white space one space: two sources with the
same normalised hash are the same tokens in the same order -- or the message with which the generator refuses the combination.
The bases reach every snippet pass (glsl_translate / glsl_bound / glsl_hoist / glsl_affine) in both of its outcomes: each switch
that turns one of them on or off is a base of its own, on top of `0` and of `ints|all`, with the variant `none` alone.
Then one line per text of `ptl_device_source` that tests and tools paste into hand-written kernels.

`programs`: the snippet passes by themselves.  One line per statement template of tests/test_affine_guard_fuzz.py (and per random
program of its generator) with what `snippets_keep_rays_affine` says of it, verdict and message; one per program of the generators
of tests/test_glsl_fuzz.py / tests/test_bound_fuzz.py and per mutated corpus snippet with the hashes of what `translate_glsl`,
`translate_library_glsl`, `hoist_glsl` and `bound_glsl` make of it (or the message they refuse it with); `specialize` is the
translation through `specialize_translated` (the test entry ptl_specialize_translated; a parent that lacks it gets it patched into its
worktree) with the text's matrix names as masked and every identifier as an Int baked to 4; `hoist_origin_uniform` is
`hoist_glsl` once more with the ray parameter `r` given as `@r`, a ray whose origin is uniform (the first-trip variants).  Last, one line
per program of HOIST_PROGRAMS below: hand-written snippets, one for each thing the hoister does with loops, staged calls and functions.

`hoist_golden`: the programs of HOIST_PROGRAMS with what the commit it runs on makes of each, whole texts, as the fixture that
tests/test_host_logic.py::test_hoister_reproduces_the_pinned_programs compares with.  It records the hash of that commit.

`digest`: a manifest of `sources` or `programs` is a megabyte of hashes.  Its digest has one line per scene / per kind of program
with the number of lines and the sha256 of those lines as they stand in the manifest; the few lines that stand for themselves
(device sources, the affine guard's templates with their messages) are kept whole.  Equal digests are equal manifests; where two
digests differ, `diff` of the manifests shows the row.

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


def pass_bases(pa):
    switches = [("bounded", pa.FLAG_BOUNDED_SNIPPETS), ("no_deferred", pa.FLAG_NO_DEFERRED_UPDATES), ("no_hoist", pa.FLAG_NO_UNIFORM_HOIST),
                ("keep_dodges", pa.FLAG_KEEP_TRANSFORM_DODGES), ("no_affine", pa.FLAG_NO_AFFINE_RAYS), ("no_unroll", pa.FLAG_NO_UNROLL)]
    return [(f"{under_name}|{name}", under | flag) for under_name, under in (("0", 0), ("ints|all", pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL)) for name, flag in switches]


def variants(pa):
    return [("none", 0), ("slices", pa.FLAG_SLICES), ("passes", pa.FLAG_PASSES), ("slices|passes", pa.FLAG_SLICES | pa.FLAG_PASSES), ("refine", pa.FLAG_REFINE),
            ("refine_slices", pa.FLAG_REFINE_SLICES)]


HOIST_UNIFORMS = {"a_mat": "mat4", "a_mat_inv": "mat4", "b_mat": "mat4", "b_mat_inv": "mat4", "scale_u": "float", "n_u": "int", "dir_u": "vec3"}
_LOOP = "vec4 nb = b_mat * vec4(0., 0., 1., 0.);\nvec4 acc = r.o;\n%sfor (int i = 0; i < %s; i++) %s\nreturn acc;"
_STAGED = """{
	vec3 u0 = normalize_normal(nb.xyz, r.d.xyz);
	acc.y += plane_intersect(r, a_mat, nb.xyz);
	if (is_collinear(u0, nb.xyz) || is_collinear(nb.xyz, u0)) { acc.w += 1.; }
	nb = b_mat * (a_mat_inv * nb);
	vec3 u1 = normalize_normal(nb.xyz, r.d.xyz);
	acc.z += plane_intersect(r, a_mat, nb.xyz);
	if (is_collinear(u1, nb.xyz) || is_collinear(nb.xyz, u1)) { acc.w += 2.; }
}"""
# (name, text, keywords of pa.hoist_glsl besides the uniforms and the parameters ["hit", "r"])
HOIST_PROGRAMS = [
    ("uniform chain carried through a canonical loop", _LOOP % ("", "n_u", "{\n\tacc += nb * scale_u + vec4(normalize(nb.xyz) * r.d.x, 0.);\n\tnb = b_mat * (a_mat_inv * nb);\n\tacc += nb * length(dir_u);\n}"), {}),
    ("ray chain carried through a canonical loop", "Ray v = transform(a_mat, r);\nvec4 acc = vec4(0.);\nfor (int i = 0; i < n_u; i++) {\n\tacc += v.d * float(i) + v.o;\n"
     "\tv = transform(b_mat, transform(a_mat_inv, v));\n\tacc += b_mat * v.o;\n}\nreturn acc;", {}),
    ("ray chain that the body reads in a nested block only", "Ray v = transform(a_mat, r);\nvec4 acc = vec4(0.);\nfor (int i = 0; i < n_u; i++) {\n\tif (acc.x < 1.) { acc += v.d; }\n"
     "\tv = transform(b_mat, transform(a_mat_inv, v));\n}\nreturn acc;", {}),
    ("ray local written once, its origin read by a uniform expression", "Ray q = transform(a_mat, r);\nvec4 k = b_mat * (a_mat_inv * q.o);\nRay w = transform(b_mat_inv, q);\nreturn k + w.d + w.o;", {}),
    ("two chains, the first reads the second, the second fails", "vec4 p = a_mat * vec4(0., 0., 1., 0.);\nvec4 q = b_mat * vec4(1., 0., 0., 0.);\nvec4 acc = r.o;\nfor (int i = 0; i < n_u; i++) {\n"
     "\tacc += p * dot(q, r.d);\n\tp = a_mat_inv * (p + q);\n\tq = b_mat_inv * q + r.d;\n}\nreturn acc;", {}),
    ("two chains, the second reads the first, the first fails", "vec4 q = b_mat * vec4(1., 0., 0., 0.);\nvec4 p = a_mat * vec4(0., 0., 1., 0.);\nvec4 acc = r.o;\nfor (int i = 0; i < n_u; i++) {\n"
     "\tacc += p * dot(q, r.d);\n\tp = a_mat_inv * (p + q);\n\tq = b_mat_inv * q + r.d;\n}\nreturn acc;", {}),
    ("two chains, one reads the other, both hold; a ray chain reads one of them", "mat4 m = a_mat * b_mat;\nvec4 p = a_mat * vec4(0., 0., 1., 0.);\nRay v = transform(b_mat, r);\nvec4 acc = r.o;\n"
     "for (int i = 0; i < n_u; i++) {\n\tacc += p * dot(m[0], v.d) + v.o;\n\tv = transform(m, v);\n\tp = m * (a_mat_inv * p);\n\tm = m * b_mat_inv;\n}\nreturn acc;", {}),
    ("staged calls before and after the update", _LOOP % ("", "n_u", _STAGED), {}),
    ("staged calls outside any loop", "vec3 n = (a_mat * vec4(dir_u, 0.)).xyz;\nvec3 u = normalize_normal(n, r.d.xyz);\nfloat t = plane_intersect(r, b_mat, n);\n"
     "return vec4(u * t, is_collinear(u, n) ? 1. : (is_collinear(n, u) ? 2. : 0.));", {}),
    ("loop with a continue", _LOOP % ("", "n_u", "{\n\tif (acc.x > 1.) continue;\n\tacc += nb * scale_u;\n\tnb = b_mat * (a_mat_inv * nb);\n}"), {}),
    ("loop that is not braced", _LOOP % ("", "n_u", "nb = b_mat * (a_mat_inv * nb);\nacc += nb * scale_u * 2.;"), {}),
    ("loop whose bound is a local written twice", _LOOP % ("int n = n_u;\nn = n + 1;\n", "n", "{\n\tacc += nb * scale_u;\n\tnb = b_mat * (a_mat_inv * nb);\n}"), {}),
    ("loop whose bound is a local written once; a nested loop with a chain of its own is left alone",
     _LOOP % ("int n = n_u;\n", "n", "{\n\tacc += nb * scale_u;\n\tnb = b_mat * (a_mat_inv * nb);\n\tfor (int j = 0; j < 2; j++) { acc += a_mat * (b_mat * nb); }\n}"), {}),
    ("three functions, the second does not parse", "vec4 first(Ray r) {\n\tfloat k = length(dir_u) * scale_u;\n\treturn r.o * k;\n}\n"
     "vec4 second(Ray r, int m) {\n\tswitch (m) { case 0: return r.o; }\n\treturn r.d * (length(dir_u) * scale_u);\n}\n"
     "vec4 third(SurfaceIntersection hit, Ray r) {\n\t" + (_LOOP % ("", "n_u", "{\n\tacc += nb * scale_u;\n\tnb = b_mat * (a_mat_inv * nb);\n}")).replace("\n", "\n\t") + "\n}\n", {"body_only": False}),
    ("only rejected candidates while a chain is carried", "vec4 nb = vec4(dir_u, 0.);\nvec4 acc = r.o;\nfor (int i = 0; i < n_u; i++) {\n\tacc += nb * r.d.x + vec4(scale_u * 2.0);\n\tnb = a_mat_inv * nb;\n}\nreturn acc;", {}),
    ("a function with an out parameter writes a local", "vec3 n = normalize(dir_u);\nturn(n);\nvec3 m = normalize(dir_u) * scale_u;\nreturn vec4(n * length(dir_u) + m * length(m), 0.0);", {"out_functions": ["turn"]}),
]


def hoist_program(pa, code, origin_uniform, keywords):
    return pa.hoist_glsl(code, HOIST_UNIFORMS, params=["hit", "@r" if origin_uniform else "r"], **keywords)


def specialize(pa, cxx, masked, unroll_bounds):
    """pa has no wrapper for the test entry ptl_specialize_translated: called through the library itself"""
    import ctypes as C
    L = pa.lib()
    L.ptl_specialize_translated.restype = C.c_void_p
    L.ptl_specialize_translated.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    n = C.c_int()
    p = L.ptl_specialize_translated(cxx.encode("utf-8"), ";".join(masked).encode(), ";".join(f"{k}={v}" for k, v in unroll_bounds.items()).encode(), C.byref(n))
    if not p:
        raise pa.PortalError(L.ptl_last_error().decode())
    try:
        return "%s\0%d" % (C.string_at(p).decode("utf-8"), n.value)
    finally:
        L.ptl_free(C.c_void_p(p))


def snippet_passes(pa, code, uniforms=None, **hoist):
    """sha256 of what each snippet pass makes of `code`, or the message it refuses it with"""
    if uniforms is None:
        uniforms = {w: "mat4" for w in re.findall(r"\b\w+_mat(?:_inv|_teleport)?\b", code)} | {w: "float" for w in re.findall(r"\b\w+_u\b", code)}
    line = {}
    origin_uniform = dict(hoist, params=["@r" if p == "r" else p for p in hoist["params"]])
    for name, run in (("translate", lambda: pa.translate_glsl(code)), ("translate_library", lambda: pa.translate_library_glsl(code)),
                      ("hoist", lambda: "\0".join(pa.hoist_glsl(code, uniforms, **hoist))), ("hoist_origin_uniform", lambda: "\0".join(pa.hoist_glsl(code, uniforms, **origin_uniform))),
                      ("bound", lambda: "%s\0%d" % pa.bound_glsl(code, ("modf", "bump"))),
                      ("specialize", lambda: specialize(pa, pa.translate_glsl(code), sorted(set(re.findall(r"\b\w+_mat(?:_inv|_teleport)?\b", code))), {w: 4 for w in sorted(set(re.findall(r"\b[A-Za-z_]\w*\b", code)))}))):
        try:
            line[name] = sha(run())
        except pa.PortalError as e:
            line[name] = "error: " + str(e)
    return line


def programs(pa):
    """(label, snippet passes of it): the affine guard's templates, the fuzz generators' snippets, mutated corpus snippets"""
    import random
    from tests import test_affine_guard_fuzz as ag, test_bound_fuzz as bf, test_glsl_fuzz as gf

    for k, (text, _) in enumerate(ag.TEMPLATES):
        code = ag.instantiate(text, "r", random.Random(k))
        library = ag.LIBRARY_CLEAN + "".join(d for needle, d in ag.LIBRARY_DIRTY.items() if needle in code)
        ok, why = pa.snippets_keep_rays_affine(library + "void f(Ray r, SurfaceIntersection hit) {" + ag.PRELUDE + code + "}")
        yield {"affine_template": k, "code": code, "ok": ok, "why": why}
    rng = random.Random(24)
    for k in range(400):
        body, library, _ = ag.random_program(rng)
        ok, why = pa.snippets_keep_rays_affine(library + "MaterialProcessing bend(SurfaceIntersection hit, Ray r) {\n" + ag.PRELUDE + body + "\nreturn material_next(vec3(0.9), r);\n}\n")
        yield {"affine_program": k, "sha256": sha(library + body), "ok": ok, "why": why}
    snippet = re.compile(r'\(\("(.*?)"\)\)', re.S)
    for seed in range(1, 37):
        for label, make in (("glsl_fuzz", gf.fuzz_scene), ("glsl_fuzz_uniforms", gf.fuzz_scene_with_uniforms)):
            code = max(snippet.findall(make(seed)[0]), key=len)
            yield {"program": label, "seed": seed, **snippet_passes(pa, code, params=["hit", "r"])}
    for seed in range(7000, 7036):
        code = max(snippet.findall(bf.bound_fuzz_scene(seed)[0]), key=len).replace("\\n", "\n")
        yield {"program": "bound_fuzz", "seed": seed, **snippet_passes(pa, code, params=["r"])}
    texts = []  # as tests/test_glsl_fuzz.py::test_hoister_survives_mutated_corpus_snippets mutates them
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "corpus", "scenes", "*.ron"))):
        texts += [m.replace('\\"', '"') for m in snippet.findall(open(path).read()) if len(m) > 40]
    tok = re.compile(r"\s+|\w+|[^\w\s]")
    stray = ["(", ")", "{", "}", ";", ",", "for", "if", "else", "=", "++", "?", ":", "[", "]", "return", "continue", "break", ".", "*", "/", "/=", "out", "Ray"]
    rng = random.Random(2424)
    for k in range(600):
        text = rng.choice(texts)
        toks = tok.findall(text)
        for _ in range(rng.randrange(0, 6)):
            if not toks:
                break
            i, op = rng.randrange(len(toks)), rng.randrange(5)
            if op == 0:
                del toks[i]
            elif op == 1:
                toks.insert(i, toks[rng.randrange(len(toks))])
            elif op == 2:
                j = rng.randrange(len(toks))
                toks[i], toks[j] = toks[j], toks[i]
            elif op == 3:
                toks = toks[:i]
            else:
                toks.insert(i, rng.choice(stray))
        code = "".join(toks)
        ok, why = pa.snippets_keep_rays_affine(code)
        yield {"program": "mutated_corpus", "n": k, "sha256": sha(code), "ok": ok, "why": why,
               **snippet_passes(pa, code, body_only=not re.search(r"^\s*\w+\s+\w+\s*\(", text), params=["r", "pos", "x", "y", "back", "first", "hit", "i"])}
    for name, code, keywords in HOIST_PROGRAMS:
        yield {"program": "hoist_hand_written", "name": name, "hoist": sha("\0".join(hoist_program(pa, code, False, keywords))),
               "hoist_origin_uniform": sha("\0".join(hoist_program(pa, code, True, keywords)))}


def hoist_golden(pa):
    """the fixture: every program of HOIST_PROGRAMS with the whole texts this commit's hoister makes of it"""
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    entries = []
    for name, code, keywords in HOIST_PROGRAMS:
        entry = {"name": name, "code": code, "keywords": keywords}
        for label, origin_uniform in (("plain", False), ("origin_uniform", True)):
            glsl, prologue = hoist_program(pa, code, origin_uniform, keywords)
            members = [l for l in prologue.splitlines(True) if l.startswith("// member:")]
            entry[label] = {"glsl": glsl, "members": members, "prologue": prologue[len("".join(members)):]}
        entries.append(entry)
    return {"recorded_from_commit": commit, "uniforms": HOIST_UNIFORMS, "params": {"plain": ["hit", "r"], "origin_uniform": ["hit", "@r"]}, "programs": entries}


def sources(pa, out):
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "corpus", "scenes", "*.ron"))):
        name = os.path.splitext(os.path.basename(path))[0]
        rows = [(b, v) for b in bases(pa) for v in variants(pa)] + [(b, variants(pa)[0]) for b in pass_bases(pa)]
        for (base_name, base), (variant_name, variant) in rows:
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


def digest(manifest):
    groups = {}  # scene / kind of program -> its lines, in the manifest's order
    for text in manifest:
        line = json.loads(text)
        key = next((f"{k} {line[k]}" for k in ("scene", "program") if k in line), "affine_program" if "affine_program" in line else None)
        if key is None:
            groups[text] = None
        else:
            groups.setdefault(key, []).append(text)
    for key, lines in groups.items():
        yield key if lines is None else json.dumps({"group": key, "lines": len(lines), "sha256": sha("".join(lines))}) + "\n"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("sources", "programs", "objects", "digest", "hoist_golden"):
        sys.exit(__doc__)
    if sys.argv[1] == "digest":
        sys.stdout.writelines(digest(open(sys.argv[2])))
        sys.exit(0)
    import portal_amd as pa

    with open(sys.argv[2], "w") as out:
        if sys.argv[1] == "hoist_golden":
            json.dump(hoist_golden(pa), out, indent=1)
            out.write("\n")
        elif sys.argv[1] == "programs":
            out.writelines(json.dumps(line) + "\n" for line in programs(pa))
        else:
            (sources if sys.argv[1] == "sources" else objects)(pa, out)
