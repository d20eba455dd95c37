"""GPU: the headline instance of step_kernel_duo (LEAN feature set, fp64, forcing read from the knots, no history
score) at bench.py's launch shape against the one-point-per-lane flavour, bit for bit.

8 192 random points x 48 h in launches of 60 indices; every one of the six outputs of every point at every index
must carry the same bit pattern in both flavours.  Twice: with the plan re-sorted by forecast before every launch
(bench.py's plan order: wavefronts of like points, where the kernel's wave-uniform shortcuts - frozen / thawed
layers, bare roads, no precipitation - are taken), and with the re-sort switched off, so that the same instance
steps wavefronts of unlike neighbours in natural order.

Both flavours compile the same physics and walk the same 64 slots per wavefront, so a shortcut that is wrong only
for some make-up of a wavefront would be wrong in both alike.  What tells it is the third comparison: the points
are independent of one another, so a point's series may not depend on who shares its wavefront - each flavour's
plan-order result must equal its own natural-order result bit for bit."""
import numpy as np
import pytest

from roadsurf_amd import abi

pytestmark = pytest.mark.gpu
SPK = 120
N, HOURS, CHUNK = 8192, 48, 60


def _series(variant, resort):
    import torch
    from roadsurf_amd import device, workload
    L = HOURS * SPK + 1
    s = abi.default_settings(L); p = abi.default_parameters()
    plan = device.Plan(N, s, p, 0)
    plan.set_variant(variant)
    run = workload.SyntheticRun(plan, 2024, HOURS, CHUNK, point_offset=777_000, plan_order=True, resort=resort)
    assert run.fused == (variant == 3)  # variant 3: rs_hip_step_knots, the knot-reading two-wavefront kernel
    out = {k: torch.full((L, N), float("nan"), dtype=torch.float64, device=plan.device) for k in device.OUT_FIELDS}
    moved = []

    def on_launch(c, t0, ns):
        o = run.orders[c][:N].long()
        moved.append(int((o != torch.arange(N, device=plan.device)).sum()))
        for k in device.OUT_FIELDS:
            out[k][t0 - 1:t0 - 1 + ns, o] = run.out.tensors[k][:ns, :N]

    run.run_pass(on_launch)
    plan.sync()
    assert plan.failed_count() == 0
    assert len(moved) == -(-L // CHUNK)
    assert (max(moved) > 0) == resort  # re-sorted launches moved points; without the re-sort nobody moved
    res = {k: v.cpu().numpy() for k, v in out.items()}
    del run
    plan.close()
    return res


@pytest.fixture(scope="module")
def series():
    return {(variant, resort): _series(variant, resort) for variant in (1, 3) for resort in (True, False)}


def _same_bits(a, b, what):
    assert len(a) == 6 and len(b) == 6
    for k in a:
        assert not np.isnan(a[k]).any() and not np.isnan(b[k]).any(), (what, k)
        ndiff = int((a[k].view(np.uint64) != b[k].view(np.uint64)).sum())
        print(f"{what}: {k}: {ndiff} of {a[k].size} values differ in their bits")
        assert ndiff == 0, (what, k)


@pytest.mark.parametrize("resort", [True, False], ids=["plan_order", "natural_order"])
def test_headline_instance_matches_one_point_per_lane_bit_for_bit(series, resort):
    _same_bits(series[(1, resort)], series[(3, resort)], "one point per lane against two wavefronts")


@pytest.mark.parametrize("variant", [3, 1], ids=["two_wavefronts", "one_point_per_lane"])
def test_a_point_does_not_depend_on_who_shares_its_wavefront(series, variant):
    _same_bits(series[(variant, False)], series[(variant, True)], "natural order against plan order")
