"""The prelude (portal_amd/csrc/device/ptl_library.h) function by function on gfx950: the probe units of tests/prelude_sweep.py through layer 1
in four hiprtc builds -- shipped, -O1, contract 1, PTL_AFFINE_RAYS + PTL_DROP_ZERO_TERMS -- with the checks of tests/test_prelude_contract.py
(the host-build legs): functions.npz, the numpy restatement on committed, random and directed lanes, the product-only forms, the cull and its
ballot, the accuracy leg.  Bit for bit; NaN == NaN is the only equivalence."""
import warnings

import numpy as np
import pytest

from tests import prelude_sweep as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


CASES = [(b, g) for b in ("shipped", "O1", "contract1", "affine") for g in ps.groups_of_cases() if not (b == "contract1" and g == "masks") and not (g == "template" and b not in ("shipped", "O1"))]


@pytest.mark.parametrize("build,group", CASES)
def test_prelude_sweep_on_gfx950(gpu, monkeypatch, build, group):
    """One probe kernel per (build, group): every case of the group over its lanes, zero differing leaves.  `O1` is the level of the CLI's one-off
    frames (PTL_JIT_OPT), `contract1` compares with the restatement under contract 1 (no functions.npz leg, no masks), `affine` with the shipped
    build's results on affine matrices, rays with o.w = 1 and d.w = 0, finite values."""
    pa = gpu
    if build == "O1":
        monkeypatch.setenv("PTL_JIT_OPT", "-O1")
    else:
        monkeypatch.delenv("PTL_JIT_OPT", raising=False)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        shipped = ps.Runner(pa, group, "gpu") if build == "affine" else None
        lines, counts = ps.run_build(pa, "gpu", build, group, shipped)
    for key, lanes in counts:
        print(f"{build}: {key}: {lanes} lanes compared")
    assert counts and not lines, "\n".join(lines[:40])
