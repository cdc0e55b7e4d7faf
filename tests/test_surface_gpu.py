"""The surface-distance kernels (csrc/kernels/surface.hip) against the brute-force fp64 reference of
tests/surface_ref.py on its table of cases, the two logit layouts and two runs bit for bit, and the refusals.
Tolerances (derived in surface_ref.check): counts and the Hausdorff column exact, the percentile and ASSD columns
within one fp32 ulp of the rounded fp64 reference."""
import pytest
import torch

import surface_ref as R
from deeplearning_mpi_amd.ops import make_backend, surface_distances

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_matches_brute_force(case):
    assert make_backend(DEV).surface_tile == R.TILE
    x, t = R.device_inputs(case, DEV)
    R.check(*surface_distances(x, t, R.IGNORE, case[5]), case)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2]], ids=str)
def test_layouts_and_runs_give_equal_bits(case):
    x, t = R.device_inputs(case, DEV)
    xv, _ = R.device_inputs(case, DEV, "nhwc_view")
    assert not xv.is_contiguous()
    a, b, c = (surface_distances(v, t, R.IGNORE, case[5]) for v in (x, x, xv))
    for o in (b, c):
        assert torch.equal(a[0].view(torch.int32), o[0].view(torch.int32)) and torch.equal(a[1], o[1])
    R.check(*c, case)


@pytest.mark.parametrize("shape, percentile, error, text", [
    ((1, 2, 4097, 8), 95.0, RuntimeError, "surface_distances: served shapes"),
    ((1, 2, 8, 8), 0.0, ValueError, "percentile"),
])
def test_refusals(shape, percentile, error, text):
    x = torch.zeros(shape, device=DEV)
    with pytest.raises(error, match=text):
        surface_distances(x, torch.zeros(shape[0], *shape[2:], dtype=torch.int64, device=DEV), percentile=percentile)
