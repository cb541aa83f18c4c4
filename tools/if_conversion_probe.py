#!/usr/bin/env python3
"""tools/if_conversion_probe.py -- round 7: what a source-level if-conversion of the headline snippet's assign-only `if` would buy, measured by
hand-patching the generated source BEFORE writing a translator pass for it.

    python tools/if_conversion_probe.py            (GPU box: static counts, kernel ms alternating between the variants, frame hash)
    PTL_VARIANTS_PRECOMPILE=1 python tools/if_conversion_probe.py   (anywhere: static counts only; fills the code-object cache)

Variants of `if (hit_b.hit) { hit_b.t /= len; hit_b.n = normal3; }` in scenes/portal_in_portal.ron's intersection snippet (flags 5, w5):
  as_written        the `if`
  whole_values      { const bool c = (hit_b.hit); hit_b.t = c ? hit_b.t / len : hit_b.t; hit_b.n = c ? normal3 : hit_b.n; }
  scalar_fields     the same with hit_b.n spelled component by component
Result (profiles/r07/part2_probe.jsonl): scalar_fields is the instruction stream of as_written; whole_values keeps the record in scratch."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
import portal_amd as pa  # noqa: E402
from isa_hist import histogram, resources  # noqa: E402

OLD = """	if (hit_b.hit) {
	    ptl_div_assign(hit_b.t , len);
	    hit_b.n = normal3;
	}"""
WHOLE = """	{ const bool ptl_c = (hit_b.hit);
	    hit_b.t = ptl_c ? ptl_div(hit_b.t , len) : hit_b.t;
	    hit_b.n = ptl_c ? normal3 : hit_b.n;
	}"""
SCALAR = """	{ const bool ptl_c = (hit_b.hit);
	    hit_b.t = ptl_c ? ptl_div(hit_b.t , len) : hit_b.t;
	    hit_b.n = vec3(ptl_c ? normal3.x : hit_b.n.x, ptl_c ? normal3.y : hit_b.n.y, ptl_c ? normal3.z : hit_b.n.z);
	}"""


def code_object(k):
    data, size = C.c_void_p(), C.c_size_t()
    pa._check(pa.lib().ptl_kernel_code_object(k._h, C.byref(data), C.byref(size)), "code_object")
    return C.string_at(data, size.value)


def main():
    device = -1 if os.environ.get("PTL_VARIANTS_PRECOMPILE") else 0
    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    r = pa.SceneRenderer(scene, device=device, flags=pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL | pa.flag_waves(5))
    r.set_option("render_depth", 40)
    src = r.kernel_source()
    assert OLD in src
    layout, size = scene.uniform_layout()
    defines = list(scene.generated_defines())
    kernels = {name: pa.Kernel(text, layout, size, device=device, defines=defines)
               for name, text in (("as_written", src), ("whole_values", src.replace(OLD, WHOLE)), ("scalar_fields", src.replace(OLD, SCALAR)))}
    rows = {}
    for name, k in kernels.items():
        code = code_object(k)
        h, res = histogram(code), resources(code, "ptl_render_kernel")
        rows[name] = {"probe": "source-level if-conversion of `if (hit_b.hit) {..}`, hand-patched headline source (flags 5, w5)", "variant": name, "instructions": h["instructions"],
                      "valu": h["valu"], "vgprs": res.get("vgpr_count"), "scratch_bytes": res.get("private_segment_fixed_size"), "code_object_sha256": hashlib.sha256(code).hexdigest()}
    if device >= 0:
        W, H = 3840, 2160
        for k in kernels.values():
            for uname, typ, _ in layout:
                if typ == pa.PTL_SAMPLER:
                    continue
                v = r.uniform_value(uname, W, H)
                if v is not None:
                    k.set_uniform(uname, typ, v)
        times = {n: [] for n in kernels}
        for _ in range(12):  # alternating, so that a drift of the clocks meets every variant alike
            for n, k in kernels.items():
                o = k.render(W, H)
                times[n].append(o["ms"])
                rows[n]["frame_sha1"] = hashlib.sha1(o["rgba8"].tobytes()).hexdigest()[:12]
        for n, t in times.items():
            t = t[2:]
            rows[n].update(kernel_ms_median=round(float(np.median(t)), 4), kernel_ms_min=round(min(t), 4), kernel_ms_max=round(max(t), 4), launches=len(t))
    for row in rows.values():
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
