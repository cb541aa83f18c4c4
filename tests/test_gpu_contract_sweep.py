"""The numerics contract on gfx950, swept: every probe function on the 2^20 stratified triples of tests/contract_sweep.py in three hiprtc
builds (shipped, -O1, contract 1) against the numpy restatement, bit for bit; texture() directed; every vector overload against its
scalar builtin.  The CPU legs of the same checks (host build) are in tests/test_math_contract.py."""
import numpy as np
import pytest

from tests import contract_sweep as cs
from tests import probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


_numpy = {}


def numpy_results(contract):
    """The numpy restatement on the whole sweep, once per contract and process, shared by the builds."""
    if contract not in _numpy:
        _numpy[contract] = cs.numpy_results(cs.sweep(), contract)
        _numpy[contract].setflags(write=False)
    return _numpy[contract]


@pytest.mark.parametrize("build", ["shipped", "O1", "contract1"])
def test_contract_sweep_on_gfx950(gpu, monkeypatch, build):
    """33 functions x 2^20 triples = 34 603 008 results per build: the hiprtc build on the GPU == numpy, bit for bit (NaN == NaN is the only
    equivalence).  `O1` is the level of the CLI's one-off frames and of every clip's first kernel (FLAG_QUICK_JIT), `contract1` the
    transcendentals over the other sqrt / reciprocal (PTL_CONTRACT_V1).  Four frames of 4096 x 576 pixels (36 MiB), four functions a pixel."""
    pa = gpu
    if build == "O1":
        monkeypatch.setenv("PTL_JIT_OPT", "-O1")
    else:
        monkeypatch.delenv("PTL_JIT_OPT", raising=False)
    samples = cs.sweep()
    contract = 1 if build == "contract1" else 2
    got = cs.run_gpu(pa, samples, defines=("PTL_CONTRACT_V1",) if contract == 1 else ())
    want = numpy_results(contract)
    assert got.shape == want.shape == (len(probe.functions()), 1 << 20)
    bad = cs.mismatches(got, want, samples, "gpu")
    print(f"{build}: {got.size} results compared")
    assert not bad, f"{build} build:\n" + "\n".join(bad)


def test_texture_directed_on_gfx950(gpu):
    """texture() on the GPU over tests/contract_sweep.texture_cases() (1x1, 2x3, 5x1, 4x4 textures and an unbound sampler; texel centres and
    edges, 0 and 1 +-1 ulp, outside [0, 1], +-1e30, +-inf, NaN, exactly W and H): == oracle.glsl_values.texture bit for bit, and within
    TEXTURE_TOLERANCE (twice the oracle's measured distance) of the binary64 bilinear clamp-to-edge filter."""
    pa = gpu
    k = pa.Kernel(cs.texture_source(pa), cs.TEXTURE_LAYOUT, cs.TEXTURE_BLOCK_SIZE, device=0)
    bad = cs.run_texture_cases(k.set_texture, lambda name, v: k.set_uniform(name, pa.PTL_I32, v), lambda w, h: k.render(w, h, rgba8=False, rgba32f=True)["rgba32f"])
    assert not bad, "\n".join(bad)


def test_vector_overloads_equal_the_scalar_builtins_on_gfx950(gpu):
    """The 342 (overload, component) rows of tests/contract_sweep.overload_rows() in the shipped build, on a 4096-triple slice of the sweep:
    component i of the vector overload == the scalar builtin on component i, bit for bit."""
    pa = gpu
    rows, samples = cs.overload_rows(), cs.overload_samples()
    assert len(rows) == 342 and samples.shape == (4096, 3)
    k = pa.Kernel(cs.overload_source(pa), cs.LAYOUT, cs.BLOCK_SIZE, device=0)
    assert k.set_texture("in_tex", probe.as_texture(samples)) == 0
    assert k.set_uniform("count_u", pa.PTL_I32, len(samples)) == 0 and k.set_uniform("base_u", pa.PTL_I32, 0) == 0
    frame = k.render(len(samples), len(rows), rgba8=False, rgba32f=True)["rgba32f"]
    bad = cs.check_overloads(samples, frame)
    print(f"{len(rows)} (overload, component) rows x {len(samples)} samples")
    assert not bad, "\n".join(bad)
    assert len(np.unique(frame[:, :, 1].view(np.uint32))) > 100000
