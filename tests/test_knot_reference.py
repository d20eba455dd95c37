"""CPU: the references tests/test_hip_knots.py holds the knot-reading kernels to.

1. golden_helpers.expand_knots - the plain numpy statement of `k0 + (r * (k1 - k0)) / spk` - reproduces the host
   twin of the generator bit for bit, so the rule the kernels are compared with IS the rule the suite's synthetic
   weather is made by.
2. The division by the reciprocal of the uniform span (rs_math.hpp rs_div_u), restated with an exactly rounded
   fused multiply-add, equals the IEEE quotient inside a band of |k1 - k0| - the band in which knot_forcing and
   expand_kernel may take it (rs_kernels.hip knot_interval_fast names the same two edges) - and does not outside."""
import math
import random

import numpy as np

import golden_helpers as gh
import knot_helpers as kh
from roadsurf_amd import synth


def test_numpy_rule_equals_the_host_generator():
    spk, n, L = 120, 64, 6 * 120 + 1
    for start_hour in (0, 17):
        f = synth.synth_forcing(n, L, seed=20240110, steps_per_knot=spk, start_hour=start_hour)
        K = {k: np.ascontiguousarray(f[k][:, ::spk]) for k in gh.KNOT_FIELDS}
        K["phase"] = np.ascontiguousarray(f["precphase"][:, ::spk])
        K["tsurf0"] = f["tsurfobs"][:, 0].copy()
        assert K["tair"].shape == (n, 7)
        g = kh.expand(K, L, spk, start_hour)
        for k in gh.KNOT_FIELDS + ("tsurfobs", "precphase", "hour"):
            assert g[k].dtype == f[k].dtype and g[k].shape == f[k].shape, k
            assert np.array_equal(g[k].view(np.int64 if g[k].itemsize == 8 else np.int32),
                                  f[k].view(np.int64 if f[k].itemsize == 8 else np.int32)), k
        # what the generator's knots never hold - the reason the crafted atlas of tests/test_hip_knots.py exists
        for k in gh.KNOT_FIELDS:
            assert not np.signbit(K[k][K[k] == 0.0]).any()
            d = np.abs(np.diff(K[k], axis=1))
            assert np.isfinite(K[k]).all() and (d[d > 0] > 1e-6).all() and d.max() < 1e3


def _bits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def test_reciprocal_division_is_the_ieee_quotient_inside_the_band_and_not_outside():
    """a / b for a = r * dv, b the uniform span (60 or 120 indices per knot), r = 0 .. b - 1.

    Why the band: q0 = RN(a * rb) is within an ulp of a / b, rem = a - b * q0 is exact in the fused multiply-add
    (b is a small integer: rem is a multiple of ulp(q0) below 2^7 ulp(q0)), and RN(q0 + rem * rb) is the correctly
    rounded quotient as long as a / b cannot lie within |rem / b| 2^-53 of a rounding boundary - which the quotient
    of two 53-bit numbers never does while it is a NORMAL number (Markstein).  So:
      lower edge: |a / b| >= 2^-1022 for every r >= 1 and b <= 128 is |dv| >= 2^7 2^-1022 = 2^-1015 = DV_MIN.  Below,
        a / b is subnormal, can be an exact tie (a = (b / 2) * odd * 2^-1074) and the perturbed sum rounds the other
        way; the largest such numerator lies just under 2^-1019, four binades under the edge.
      upper edge: r * dv must stay finite for r <= b - 1 < 2^7: |dv| < 2^1024 / 2^7 = 2^1017 = DV_MAX.  In the same
        binade, from 2^1024 / 119 = 1.51e306 on, 119 * dv is infinite, q0 = inf and rem = fma(-b, inf, inf) is NaN
        where a / b is inf.
      dv = 0 gives +-0, and k0 + (+-0) = k0 for every k0 but -0.0 (r = 0 with a falling series: a = -0.0, the
        sequence returns +0.0 where -0.0 / b is -0.0 - which is why an interval whose k0 is -0.0 is outside the domain).
    """
    assert kh.DV_MIN == 2.0 ** -1015 and kh.DV_MAX == 2.0 ** 1017
    rnd = random.Random(20240110)
    edge_lo = [kh.DV_MIN, math.nextafter(kh.DV_MIN, 1.0)]
    edge_hi = [math.nextafter(kh.DV_MAX, 0.0), kh.DV_MAX / 2]
    exps = [-1015, -1014, -1013, -1000, -970, -500, -60, -10, -1, 0, 1, 7, 60, 500, 1000, 1015, 1016]
    for b in (60.0, 120.0):
        rb = 1.0 / b
        dvs = edge_lo + edge_hi + [0.1, 1.0 / 3.0, 5e-324 * 2.0 ** 59]
        dvs += [rnd.uniform(1.0, 2.0) * 2.0 ** e for e in exps for _ in range(3)]
        dvs += [float(int(rnd.uniform(1.0, 2.0) * 2 ** 52) | 1) * 2.0 ** (e - 52) for e in exps[:4]]  # full mantissas
        for dv in dvs:
            assert kh.DV_MIN <= dv < kh.DV_MAX
            for sign in (1.0, -1.0):
                for r in range(int(b)):
                    a = float(r) * (sign * dv)
                    assert math.isfinite(a)
                    got, want = kh.div_u(a, b, rb), a / b
                    if r == 0:  # +-0: equal as numbers, the sign of the zero is the sequence's own
                        assert got == 0.0 and want == 0.0
                        assert 1.5 + got == 1.5 and 0.0 + got == 0.0 and _bits(0.0 + got) == _bits(0.0 + want)
                    else:
                        assert _bits(got) == _bits(want), (b, r, sign * dv, got, want)
        # dv = 0: +0.0 for every r
        for r in range(int(b)):
            assert _bits(kh.div_u(float(r) * 0.0, b, rb)) == _bits(0.0)

    # outside, below: an exact tie in the subnormal range comes out on the wrong side (for RN(1 / b) != 1 / b)
    wrong = 0
    for b in (60.0, 120.0):
        for _ in range(40):
            odd = 2 * rnd.randrange(1 << 40, 1 << 44) + 1
            dv = (b / 2) * odd * 2.0 ** -1074
            assert 0.0 < dv < kh.DV_MIN
            wrong += kh.div_u(dv, b, 1.0 / b) != dv / b
    assert wrong > 0
    # ... the largest numerator that can be such a tie is (b/2) * odd * 2^-1074 < 2^53 * 2^-1072: under 2^-1019
    top = 15.0 * float((2 ** 53 // 15 - 1) | 1) * 2.0 ** -1072
    assert 2.0 ** -1020 < top < 2.0 ** -1019
    # outside, above: the numerator overflows for the largest r of the longer span within DV_MAX's own binade
    assert math.isfinite(127.0 * math.nextafter(kh.DV_MAX, 0.0)) and math.isinf(119.0 * (kh.DV_MAX * 1.08))
    assert math.isnan(math.inf * (1.0 / 120.0) - math.inf)  # rem = fma(-b, q0 = inf, a = inf)
    # outside, -0.0: a falling series at the knot itself
    a = 0.0 * -1.0
    assert _bits(a) == _bits(-0.0) and _bits(a / 120.0) == _bits(-0.0)
    assert _bits(kh.div_u(a, 120.0, 1.0 / 120.0)) == _bits(0.0)
    assert _bits(-0.0 + kh.div_u(a, 120.0, 1.0 / 120.0)) != _bits(-0.0 + a / 120.0)
