"""The numerics contract (portal_amd/csrc/device/ptl_glsl.h) against its numpy restatement
(oracle/glsl_math.py): bit-identical on the host build, and accurate against binary64."""
import numpy as np
import pytest

from tests import probe


@pytest.fixture(scope="module")
def host_results(pa):
    from oracle import host_build as hb

    samples = probe.inputs()
    hk = hb.HostKernel(probe.source(pa), probe.LAYOUT, probe.BLOCK_SIZE)
    hk.set_texture("in_tex", probe.as_texture(samples))
    hk.set_uniform("n_u", len(samples))
    out = hk.render(len(samples), len(probe.functions()), rgba8=False)["rgba32f"]
    assert np.array_equal(out[0, :, 1].view(np.uint32), samples[:, 0].view(np.uint32))  # inputs arrived intact
    return samples, out[:, :, 0]


def test_contract_cpp_equals_numpy_bit_for_bit(host_results):
    samples, got = host_results
    want = probe.numpy_results(samples)
    for k, (name, _, _) in enumerate(probe.functions()):
        ok = probe.same_bits(got[k], want[k])
        bad = np.nonzero(~ok)[0]
        assert ok.all(), f"{name}: {len(bad)} of {len(ok)} differ, e.g. inputs {samples[bad[0]]} -> c++ {got[k][bad[0]]!r} numpy {want[k][bad[0]]!r}"


# ---- the stratified sweep (tests/contract_sweep.py): 2^20 triples x every probe function ------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    from tests import contract_sweep as cs

    return cs.sweep()


def test_sweep_is_seeded_and_holds_what_it_promises(sweep):
    """Same triples on every call and in every process (the GPU leg and the CPU leg must look at the same inputs); the directed sets are in."""
    import zlib

    from tests import contract_sweep as cs

    assert sweep.shape == (1 << 20, 3) and sweep.dtype == np.float32 and not sweep.flags.writeable
    assert zlib.crc32(sweep.tobytes()) == zlib.crc32(cs._build.__wrapped__()[0].tobytes())      # built twice from the seed: identical
    a = set(sweep[:, 0].view(np.uint32).tolist())
    every = lambda values: all(int(np.float32(v).view(np.uint32)) in a for v in values)
    assert every(cs.from_bits(np.arange(512, dtype=np.int64) << 23)) and every(cs.from_bits((np.arange(512, dtype=np.int64) << 23) | 0x3504F3))   # every sign / exponent field
    consts = cs.header_comparison_constants()
    assert len(consts) >= 13 and every(cs.around(consts, 16))                                                 # every comparison constant of the header, +-16 ulp
    assert every(cs.around((np.arange(1, 4097) * (np.pi / 2)).astype(np.float32), 4)) and every(cs.around((np.arange(1, 4097) * (np.pi / 2) + np.pi / 4).astype(np.float32), 4))
    assert every(np.arange(-152, 131, dtype=np.float32)) and every(np.arange(-152, 131, dtype=np.float32) + np.float32(0.5))
    assert every([np.float32(p[0]) for _, p in cs.FIXED_POINTS])
    for name in ("atan2", "pow", "mod", "fma", "smoothstep", "vector", "equal"):
        assert len(cs.block(name)) >= 2000
    b = set(sweep[:, 1].view(np.uint32).tolist())
    assert len(a & b) > 900000                                                                                 # b is a permutation of a (beside block 2)


@pytest.mark.parametrize("contract", [2, 1])
def test_sweep_cpp_equals_numpy_bit_for_bit(pa, sweep, contract):
    """The host build (g++) == the numpy restatement on the whole sweep, every probe function, for the default contract and for contract 1
    (`PTL_CONTRACT_V1` / oracle.glsl_math.set_contract(1)).  NaN == NaN is the only equivalence: no tolerance, no input left out."""
    from tests import contract_sweep as cs

    got = cs.run_host(pa, sweep, defines=("PTL_CONTRACT_V1",) if contract == 1 else ())
    want = cs.numpy_results(sweep, contract)
    assert got.shape == want.shape == (len(probe.functions()), len(sweep))
    bad = cs.mismatches(got, want, sweep, "c++")
    assert not bad, f"contract {contract}:\n" + "\n".join(bad)


def ulp_error(got, exact):
    got64 = got.astype(np.float64)
    spacing = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return np.abs(got64 - exact) / np.maximum(spacing, 1e-45)


# name, binary64 reference, domain, bound in ulp.  Measured maxima over the sweep's points inside the domain (every value of the sweep's three
# columns) plus the 20 000 random ones, against binary64 libm (whose own error is ~1e-9 of a binary32 ulp):
#   sin 1.47  cos 1.47  asin 2.27  acos 1.18  exp 0.94  log 0.74  exp2 0.92  log2 1.09  sqrt 0.50  tan 3.24
#   atan 3.23 at x = 0.43229637 (the middle branch, (x - 1) / (x + 1), just above the tan(pi/8) knot: the worst of an exhaustive search of that
#     branch, kept as a named point of the sweep; 3.01 over the sweep's other points, 2.29 at the named point 0.41421542).
#     The bound was 2.0 while only uniform random points were drawn over (-1e6, 1e6), which never land there; the contract's bits are
#     frozen by the golden frames, so the bound states what the kernel does: the next half-ulp step above the measured maximum.
#   sqrt: 0.5 ulp holds from 2^-100 up.  Below, contract 2 DEFINES sqrt as +0 (ptl_glsl.h "CONTRACT 2"), which no ulp bound describes:
#     those swept points are asserted to give exactly +0, and contract 1 keeps 0.5 ulp on the whole of [0, 1e30], subnormals included.
ACCURACY = [
    ("sin", np.sin, (-100.0, 100.0), 2.0), ("cos", np.cos, (-100.0, 100.0), 2.0), ("atan", np.arctan, (-1e6, 1e6), 3.5),
    ("asin", np.arcsin, (-1.0, 1.0), 3.0), ("acos", np.arccos, (-1.0, 1.0), 3.0), ("exp", np.exp, (-80.0, 80.0), 2.0),
    ("log", np.log, (1e-30, 1e30), 2.0), ("exp2", np.exp2, (-120.0, 120.0), 2.0), ("log2", np.log2, (1e-30, 1e30), 3.0),
    ("sqrt", np.sqrt, (0.0, 1e30), 0.5), ("tan", np.tan, (-1.5, 1.5), 4.0),
]


@pytest.fixture(scope="module")
def swept_values(sweep):
    return np.unique(sweep.reshape(-1).view(np.uint32)).view(np.float32)


@pytest.mark.parametrize("name,ref,domain,max_ulp", ACCURACY)
def test_contract_accuracy_against_binary64(swept_values, name, ref, domain, max_ulp):
    """Every swept value inside the function's domain -- the branch knots, the trig cancellation points, integers and half-integers, every
    exponent field -- and 20 000 random ones, against binary64 libm.  (The table above holds the measured maxima.)"""
    from oracle import glsl_math as M

    rng = np.random.default_rng(5)
    lo, hi = domain
    x = (np.exp(rng.uniform(np.log(lo), np.log(hi), 20000)) if lo > 0 else rng.uniform(lo, hi, 20000)).astype(np.float32)
    x = np.concatenate([x, swept_values[(swept_values >= lo) & (swept_values <= hi)]])
    assert len(x) > 300000
    if name == "atan":
        knots = np.abs(x[:, None] - np.array([0.4142135623730950, 2.414213562373095], np.float32)[None, :]) < 1e-5
        assert knots.any(axis=0).all() and np.float32(0.41421542) in x
    if name == "sqrt":
        flushed = x < np.float32(2.0 ** -100)
        assert flushed.sum() > 10000 and (M.sqrt(x[flushed]).view(np.uint32) == 0).all()          # the contract's definition below 2^-100: +0
        previous = M.set_contract(1)
        try:
            err = ulp_error(M.sqrt(x[flushed]), np.sqrt(x[flushed].astype(np.float64)))
        finally:
            M.set_contract(previous)
        assert err.max() <= max_ulp, f"sqrt, contract 1: {err.max():.2f} ulp at x={x[flushed][err.argmax()]!r}"
        x = x[~flushed]
    got = getattr(M, name)(x)
    err = ulp_error(got, ref(x.astype(np.float64)))
    print(f"{name}: max {err.max():.4f} ulp at x={x[err.argmax()]!r} over {len(x)} points (bound {max_ulp})")
    assert err.max() <= max_ulp, f"{name}: {err.max():.2f} ulp at x={x[err.argmax()]!r}"


def test_contract_exact_identities():
    from oracle import glsl_math as M

    f = np.float32
    assert M.acos(f(-1.0)) == f(np.pi)                 # `#define PI acos(-1.)` (src/library.glsl:15)
    assert M.sin(f(0.0)) == 0 and M.cos(f(0.0)) == 1 and M.atan(f(0.0)) == 0 and M.exp(f(0.0)) == 1 and M.log(f(1.0)) == 0
    assert M.atan2(f(1.0), f(0.0)) == f(np.pi / 2) and M.atan2(f(0.0), f(-1.0)) == f(np.pi)
    assert M.mod(f(5.5), f(2.0)) == f(1.5) and M.mod(f(-0.5), f(2.0)) == f(1.5)   # x - y*floor(x/y)
    assert M.step(f(0.5), f(0.5)) == 1 and M.step(f(0.5), f(0.25)) == 0
    assert M.sign(f(-3.0)) == -1 and M.sign(f(0.0)) == 0
    assert M.exp2(f(10.0)) == 1024 and M.log2(f(1024.0)) == 10 and M.pow(f(2.0), f(0.5)) == pytest.approx(2 ** 0.5, rel=3e-7)
    assert np.isnan(M.fmin(f(np.nan), f(1.0))) and M.fmin(f(1.0), f(np.nan)) == 1   # min(a,b) = b < a ? b : a


def test_fma_emulation_is_a_single_rounding():
    """Cross-check the numpy fma emulation against exact rational arithmetic."""
    from fractions import Fraction

    from oracle import glsl_math as M

    rng = np.random.default_rng(11)
    a = rng.standard_normal(300).astype(np.float32)
    b = rng.standard_normal(300).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.uniform(-1e-7, 1e-7, 300))).astype(np.float32)  # heavy cancellation
    got = M.fma(a, b, c)
    for k in range(300):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        near = np.float32(float(exact))  # float(Fraction) rounds correctly to binary64; then to binary32:
        lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
        best = min((lo, near, hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[k] == best, (a[k], b[k], c[k])


def exact_round_to_binary32(q):
    """The binary32 number nearest to the Fraction q != 0 (ties to even, subnormals, overflow to infinity), in integer arithmetic."""
    from fractions import Fraction

    negative, q = q < 0, abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    scaled = q / quantum
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    value = n * quantum
    out = np.float32(np.inf) if value >= Fraction(2) ** 128 else np.float32(float(value))   # (value has at most 24 bits: float() is exact)
    return -out if negative else out


def test_fma_emulation_against_exact_arithmetic_on_the_sweep():
    """The oracle's fma (binary64 product, TwoSum, round-to-odd, one rounding to binary32) against exact rational arithmetic on every third row
    of the sweep's fma block: products that cancel c, results in the subnormal range, at the overflow boundary, exact ties of the sum and
    ties missed by a tail that binary64 cannot hold.  Zero results keep IEEE's sign (+0 unless both addends are -0)."""
    from fractions import Fraction

    from oracle import glsl_math as M
    from tests import contract_sweep as cs

    rows = cs.block("fma")[::3]
    assert len(rows) >= 5000
    a, b, c = (np.ascontiguousarray(rows[:, k]) for k in range(3))
    got = M.fma(a, b, c)
    kinds = {"subnormal": 0, "overflow": 0, "tie": 0, "zero": 0}
    for k in range(len(rows)):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        if exact == 0:
            want = np.float32(float(a[k]) * float(b[k]) + float(c[k]))     # both exact in binary64: the sum of two zeros, or x + (-x) = +0
            kinds["zero"] += 1
        else:
            want = exact_round_to_binary32(exact)
            kinds["overflow"] += bool(np.isinf(want))
            kinds["subnormal"] += bool(abs(float(want)) < 2.0 ** -126)
            if np.isfinite(want) and exact != Fraction(float(want)):
                with np.errstate(over="ignore"):
                    toward = np.nextafter(want, np.float32(np.inf if exact > Fraction(float(want)) else -np.inf))
                gap = abs(Fraction(float(toward)) - Fraction(float(want))) if np.isfinite(toward) else Fraction(2) ** 104
                kinds["tie"] += abs(exact - Fraction(float(want))) * 2 == gap
        assert got[k].view(np.uint32) == want.view(np.uint32), (k, a[k], b[k], c[k], got[k], want)
    assert min(kinds.values()) >= 100, kinds


# ---- texture() and the vector overloads in the host build -------------------------------------------------------------------------------
def test_texture_directed_in_the_host_build(pa):
    """texture() on 1x1, 2x3, 5x1 and 4x4 random textures and an unbound sampler, at every texel centre and edge, 0 and 1 +-1 ulp, outside
    [0, 1], +-1e30, +-inf, NaN and exactly W and H in either coordinate: the host build == oracle.glsl_values.texture bit for bit, and within
    TEXTURE_TOLERANCE of a binary64 bilinear clamp-to-edge filter written on its own (a transposed or flipped fetch shared by both
    restatements would show there).  The tolerance is twice the oracle's measured distance from binary64, asserted here."""
    from oracle import host_build as hb
    from tests import contract_sweep as cs

    measured = max(float(np.abs(cs.texture_oracle(tex, uv).astype(np.float64) - cs.texture_binary64(tex, uv)).max()) for tex, uv in cs.texture_cases())
    print(f"numpy oracle vs binary64 bilinear: {measured:.3g}")
    assert 0.5 * cs.TEXTURE_MEASURED <= measured <= cs.TEXTURE_MEASURED
    hk = hb.HostKernel(cs.texture_source(pa), cs.TEXTURE_LAYOUT, cs.TEXTURE_BLOCK_SIZE)
    bad = cs.run_texture_cases(hk.set_texture, hk.set_uniform, lambda w, h: hk.render(w, h, rgba8=False)["rgba32f"])
    assert not bad, "\n".join(bad)
    # the binary64 filter is no restatement of a shared mistake: it tells a transposed and a flipped texture apart from the right one
    tex, uv = cs.texture_cases()[1]
    inside = np.isfinite(uv).all(axis=1)
    for wrong in (tex[::-1], tex[:, ::-1]):
        assert np.abs(cs.texture_oracle(np.ascontiguousarray(wrong), uv)[inside] - cs.texture_binary64(tex, uv)[inside]).max() > 1e-3


def test_vector_overloads_equal_the_scalar_builtins_in_the_host_build(pa):
    """Every vec2 / vec3 / vec4 overload of the component-wise builtins that ptl_glsl.h spells by hand (342 (overload, component) rows: 22 one-argument
    builtins, min max mod pow atan step, the vector-scalar forms of min max mod step clamp mix smoothstep, the all-vector clamp mix
    smoothstep), on a 4096-triple slice of the sweep: component i == the scalar builtin on component i, bit for bit."""
    from oracle import host_build as hb
    from tests import contract_sweep as cs

    rows, samples = cs.overload_rows(), cs.overload_samples()
    assert len(rows) == 342 and samples.shape == (4096, 3)
    hk = hb.HostKernel(cs.overload_source(pa), cs.LAYOUT, cs.BLOCK_SIZE)
    hk.set_texture("in_tex", probe.as_texture(samples))
    hk.set_uniform("count_u", len(samples))
    hk.set_uniform("base_u", 0)
    frame = hk.render(len(samples), len(rows), rgba8=False)["rgba32f"]
    bad = cs.check_overloads(samples, frame)
    print(f"{len(rows)} (overload, component) rows x {len(samples)} samples")
    assert not bad, "\n".join(bad)
    assert len(np.unique(frame[:, :, 1].view(np.uint32))) > 100000      # the rows computed something
