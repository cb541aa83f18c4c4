"""oracle/mesa.py -- the reference's shader compiled and run by Mesa (llvmpipe), headless.

TEST INFRASTRUCTURE ONLY: the product never imports this, `__graft_entry__.build()` builds none of it and
no test needs it.  `tests/golden/make_mesa_fixtures.py` is its one user: it stores what Mesa computed
under `tests/golden/mesa/`, and the tests compare against those files.

Every other oracle of this repository executes the reference's GLSL with code written here
(`oracle/glsl_interp.py` under the builtin contract of `oracle/glsl_math.py`).  This one hands the same
text to a GLSL compiler nobody here wrote: the fragment text is `ReferenceShader.build()`'s `.source`, the
vertex text is `VERTEX_SHADER_300`, cut out of the reference's `src/gui/scene.rs` at run time, and
`oracle/mesa_runner.c` (built on demand into `oracle/_build/`) draws the reference's two-triangle
rectangle into a float target through the DRI swrast interface.  Neither text is stored anywhere.
"""
from __future__ import annotations

import glob
import os
import re
import subprocess
import tempfile

import numpy as np

from . import reference_shader as RS
from .glsl_values import Mat, Vec

HERE = os.path.dirname(os.path.abspath(__file__))
RUNNER_SOURCE = os.path.join(HERE, "mesa_runner.c")
RUNNER = os.path.join(HERE, "_build", "mesa_runner")
VERTEX_SOURCE = os.path.join(os.path.dirname(RS.REFERENCE_SRC), "src", "gui", "scene.rs")
DRIVER_GLOBS = ("/usr/lib/*/dri/swrast_dri.so", "/usr/lib64/dri/swrast_dri.so", "/usr/lib/dri/swrast_dri.so")
GLAPI_GLOBS = ("/usr/lib/*/libglapi.so.0", "/usr/lib64/libglapi.so.0", "/usr/lib/libglapi.so.0")

_info = None


def _first(patterns):
    for p in patterns:
        hits = sorted(glob.glob(p))
        if hits:
            return hits[0]
    return None


def driver_path():
    return _first(DRIVER_GLOBS)


def vertex_text() -> str:
    """`VERTEX_SHADER_300` of the reference's src/gui/scene.rs (a Rust string literal without escapes)."""
    m = re.search(r'const VERTEX_SHADER_300: &str = "([^"]*)";', open(VERTEX_SOURCE, encoding="utf-8").read())
    if not m:
        raise FileNotFoundError("VERTEX_SHADER_300 not found in " + VERTEX_SOURCE)
    return m.group(1)


def runner() -> str:
    if not os.path.exists(RUNNER) or os.path.getmtime(RUNNER) < os.path.getmtime(RUNNER_SOURCE):
        os.makedirs(os.path.dirname(RUNNER), exist_ok=True)
        subprocess.run(["cc", "-O1", RUNNER_SOURCE, "-ldl", "-o", RUNNER], check=True)
    return RUNNER


def _hex(values, dtype):
    return " ".join(f"{int(b):08x}" for b in np.asarray(values, dtype).reshape(-1).view(np.uint32))


def uniform_line(name, value) -> str:
    """One job line; the value travels as its bits, so nothing is rounded on the way."""
    if isinstance(value, Mat):
        return f"uniform {name} mat4 " + _hex([np.asarray(c) for col in value.cols for c in col.c], np.float32)
    if isinstance(value, Vec):
        return f"uniform {name} vec{value.n} " + _hex([np.asarray(c) for c in value.c], np.float32)
    a = np.asarray(value)
    if a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer):
        return f"uniform {name} int " + _hex(a, np.int32)
    return f"uniform {name} float " + _hex(a, np.float32)


class Job:
    """One runner process: one program, any number of draws into one target."""

    def __init__(self, shader: RS.ReferenceShader, kind: str, width: int, height: int):
        from PIL import Image

        self.dir = tempfile.TemporaryDirectory(prefix="mesa_job_")
        self.kind, self.width, self.height, self.draws = kind, width, height, 0
        path = lambda n: os.path.join(self.dir.name, n)
        with open(path("vertex"), "w", encoding="utf-8") as f:
            f.write(vertex_text())
        with open(path("fragment"), "w", encoding="utf-8") as f:
            f.write(shader.source)
        self.lines = [f"program {path('vertex')} {path('fragment')}", f"target {kind} {width} {height}"]
        for k, (name, rel) in enumerate(shader.scene.textures):
            full = os.path.join(shader.asset_root, rel)
            if not os.path.exists(full):
                continue
            texels = np.ascontiguousarray(np.array(Image.open(full).convert("RGBA")), np.uint8)
            texels.tofile(path(f"texture{k}"))
            self.lines.append(f"texture {name}_tex {texels.shape[1]} {texels.shape[0]} {path(f'texture{k}')}")
        self.uniforms(shader.uniforms)
        self.uniforms({"_teleport_external_ray": np.int32(0)})

    def uniforms(self, values: dict):
        self.lines += [uniform_line(k, v) for k, v in values.items()]

    def draw(self):
        self.lines.append("draw " + os.path.join(self.dir.name, "out"))
        self.draws += 1

    def run(self) -> np.ndarray:
        """-> (draws, height, width, 4) float32 or uint8, row 0 = image row 0"""
        global _info
        job = os.path.join(self.dir.name, "job")
        with open(job, "w", encoding="utf-8") as f:
            f.write("\n".join(self.lines) + "\n")
        done = subprocess.run([runner(), driver_path(), job], capture_output=True, text=True)
        if done.returncode != 0:
            raise RuntimeError(f"mesa_runner exit {done.returncode}: {done.stderr.strip()[-2000:]}")
        _info = tuple(done.stdout.split("\n")[0].split("\t"))
        out = np.fromfile(os.path.join(self.dir.name, "out"), np.float32 if self.kind == "f32" else np.uint8)
        self.dir.cleanup()
        return out.reshape(self.draws, self.height, self.width, 4)


def available() -> bool:
    """True where the driver, libglapi and the reference tree all exist."""
    return bool(driver_path() and _first(GLAPI_GLOBS) and os.path.exists(VERTEX_SOURCE)
                and all(os.path.exists(os.path.join(RS.REFERENCE_SRC, n)) for n in RS.FILES))


def gl_info():
    """(GL_VERSION, GL_RENDERER) of the driver: of the last run, or of a context opened for the question."""
    global _info
    if _info is None and available():
        with tempfile.NamedTemporaryFile("w", prefix="mesa_job_") as empty:
            done = subprocess.run([runner(), driver_path(), empty.name], capture_output=True, text=True)
        if done.returncode == 0:
            _info = tuple(done.stdout.split("\n")[0].split("\t"))
    return _info


def render(shader: RS.ReferenceShader, width: int, height: int) -> np.ndarray:
    """The frame Mesa draws for `shader` (options, overrides and camera set as for `shader.render`): (h, w, 4) float32."""
    shader.build(width, height)
    job = Job(shader, "f32", width, height)
    job.draw()
    return job.run()[0]


def teleport_bytes(shader: RS.ReferenceShader, segments) -> np.ndarray:
    """The teleport query as the reference's host asks it (src/main.rs:1361-1393): `main()` with
    `_teleport_external_ray = 1` into a real 2x3 RGBA8 target.  -> (segments, 24) uint8 as read back."""
    shader.build(0, 0)
    job = Job(shader, "u8", 2, 3)
    if "teleport_light_u" in shader.uniforms:
        job.uniforms({"teleport_light_u": np.int32(1)})  # src/main.rs:1367
    job.uniforms({"_teleport_external_ray": np.int32(1)})
    for a, b in segments:
        job.uniforms({"_external_ray_a": Vec(np.asarray(a, np.float64).astype(np.float32)), "_external_ray_b": Vec(np.asarray(b, np.float64).astype(np.float32))})
        job.draw()
    return job.run().reshape(len(segments), 24)


def decode_teleport(arr):
    """src/main.rs:1394-1405 over the 24 bytes -> (teleported, hit, subspace, position bits (3,) uint32)"""
    arr = np.asarray(arr, np.uint8).reshape(-1)
    hit = bool(arr[5] == 255 or arr[13] == 255 or arr[21] == 255)
    sub = bool(arr[6] == 255 or arr[14] == 255 or arr[22] == 255)
    pos = np.array([np.frombuffer(bytes([arr[k], arr[k + 1], arr[k + 2], arr[k + 4]]), "<f4")[0] for k in (0, 8, 16)], np.float32)
    teleported = not (pos[0] == 0 and pos[1] == 0 and pos[2] == 0)
    return teleported, hit, sub, (pos.view(np.uint32) if teleported else np.zeros(3, np.uint32))
