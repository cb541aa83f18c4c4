"""The prelude (portal_amd/csrc/device/ptl_library.h) function by function on the CPU: the host build of the probe units of
tests/prelude_sweep.py against tests/golden/reference_text/functions.npz (the reference text's own values), against the numpy restatement
on committed, random and directed lanes, the product-only forms against the restatement of their base forms, the accuracy leg, and the
coverage every directed family must reach.  The same checks on gfx950: tests/test_gpu_prelude_sweep.py."""
import warnings

import numpy as np
import pytest

from tests import prelude_sweep as ps


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def test_case_table_covers_the_prelude_share_of_the_committed_vectors():
    """Every function of functions.npz that lives in ptl_library.h has a case (a function added to the prelude and to the vectors fails here
    until it gets one); the keys left out are the trace template's, which the header does not define."""
    keys = set(ps.committed_vectors())
    table = {c.key for c in ps.cases() if c.group in ("library", "template")}
    assert table == keys - ps.TEMPLATE_KEYS
    assert ps.TEMPLATE_KEYS <= keys
    defined = ps.prelude_reference_functions()
    assert {c.name for c in ps.cases() if c.group == "library"} <= defined
    assert not {c.name for c in ps.cases() if c.group == "template"} & defined
    assert not {k.split("(")[0] for k in ps.TEMPLATE_KEYS} & defined
    forms = {"plane_intersect_derived", "plane_intersect_o", "plane_intersect_derived_o", "ptl_plane_intersect_unit", "ptl_normalize_normal_unit", "ptl_is_collinear_len",
             "ptl_is_collinear_len0", "ptl_transform_m", "ptl_mul_m", "ptl_row_m", "ptl_mul_origin", "ptl_cannot_be_nearer", "ptl_plane_cull"}
    text = "\n".join(c.body for c in ps.cases())
    assert all(f + "(" in text or f + "<" in text for f in forms)
    assert len([c for c in ps.cases() if c.group == "masks" and not c.name.startswith("derived_m_")]) == len(ps.MASKS) * 4
    assert len([c for c in ps.cases() if c.name.startswith("derived_m_")]) == 3


def test_directed_lanes_reach_every_listed_branch():
    """Counted with the restatement's arithmetic, never with the code under test: MIN_BRANCH lanes through every branch, MIN_EDGE on every equality
    and NaN edge."""
    low = []
    for key, branch, lanes, minimum in ps.coverage_lines():
        print(f"{key.split('(')[0]:28s} {branch:45s} {lanes:6d} >= {minimum}")
        if lanes < minimum:
            low.append((key, branch, lanes, minimum))
    assert not low, low
    required = {"cylinder(Ray,vec3,vec3,float)": 8, "cap(Ray,vec3,vec3,float)": 7, "triangle(Ray,vec3,vec3,vec3)": 16, "plane_intersect(Ray,mat4,vec3)": 10,
                "my_refract(vec3,vec3,float)": 8, "is_collinear(vec3,vec3)": 8, "color_grid3(vec3,vec2)": 7}
    for key, count in required.items():
        assert len(ps.directed(key)[2]) >= count, key


# (contract 1 never gets a mask other than 0xffff: no such leg)
HOST_LEGS = [(b, g) for b in ("shipped", "contract1", "affine") for g in ps.groups_of_cases() if not (b != "shipped" and g == "template") and not (b == "contract1" and g == "masks")]


@pytest.mark.parametrize("build,group", HOST_LEGS)
def test_host_build_of_the_probe(pa, build, group):
    """g++ build of the probe unit: functions.npz on the committed lanes, the restatement on committed + 16 384 random + directed lanes, every
    product-only form against its base form's restatement, the cull on the device function, the accuracy leg -- zero differing leaves."""
    shipped = ps.Runner(pa, group, "host") if build == "affine" else None
    lines, counts = ps.run_build(pa, "host", build, group, shipped)
    for key, lanes in counts:
        print(f"{build}: {key}: {lanes} lanes compared")
    assert counts and not lines, "\n".join(lines[:40])


def test_accuracy_constants_are_the_restatements_residuals():
    """ACCURACY_MEASURED is what the restatement gives today on the well-conditioned lanes (never what a build gives), on enough lanes."""
    for name in ps.ACCURACY_FUNCTIONS:
        worst, n = ps.restatement_residual(name)
        print(f"{name}: restatement residual {worst:.4g} on {n} lanes (constant {ps.ACCURACY_MEASURED[name]:.4g})")
        assert n >= 256
        assert 0.9 * ps.ACCURACY_MEASURED[name] <= worst <= ps.ACCURACY_MEASURED[name]


@pytest.mark.parametrize("group", ps.groups_of_cases())
def test_probe_unit_compiles_for_gfx950(pa, group):
    """hiprtc, no device: what tests/test_gpu_prelude_sweep.py runs builds for the target."""
    src, layout, size, defines = ps.template_unit(pa) if group == "template" else (ps.source(pa, group), ps.LAYOUT, ps.BLOCK_SIZE, ())
    k = pa.Kernel(src, layout, size, device=-1, defines=defines)
    assert k._h
