"""The driver's inputs at the kept rows and the dew-point deficit: the definition, in numpy.

``rs_driver_run`` gives the six output series at every ``step``-th simulation index (``save_output``,
roadrunner.cpp:303).  What the reference's operational program stores beside them per point and output time
(examples/example2/src/QueryDataTools.cpp:323-347) are the INPUTS the model saw there - air temperature and dew
point as ``read_input`` hands them to ``runsimulation``: merged over the sources, interpolated, Tdew / RH completed -
and the difference between the surface temperature and the dew point, the hoar-frost and condensation indicator
(``calc_difference``, QueryDataTools.cpp:285-296).  ``kept_rows`` and ``dew_point_deficit`` are the specification;
the device side (``rs_driver_run_kept``: include/roadsurf.h, roadsurf_amd/csrc/rs_driver.hip) is held to it bit for
bit by the tests.
"""
from __future__ import annotations

import numpy as np

#: order of ``RsDriverKept::merged`` (that of rs_driver_expand's ``merged``)
FIELDS = ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "sw_dir", "lw_net", "tsurfobs")
#: what a deficit without both operands reads
NO_DEFICIT = -9999.0
#: an operand counts only above this - strictly: -9000.0 itself is missing here (this is calc_difference's rule,
#: not roadrunner.cpp's is_missing, which keeps -9000.0)
PRESENT_ABOVE = -9000.0


def kept_rows(merged, step: int) -> np.ndarray:
    """``merged[..., ::step]``: kept row r is the 0-based simulation index r*step."""
    step = int(step)
    if step < 1:
        raise ValueError("step >= 1")
    return np.asarray(merged)[..., ::step]


def dew_point_deficit(tsurf, tdew) -> np.ndarray:
    """Element-wise ``tsurf - tdew`` (one float64 subtraction) where both operands are not NaN and > -9000, else
    exactly -9999.0.  An infinite operand above the threshold is an operand like any other (inf - inf is NaN)."""
    a = np.asarray(tsurf, np.float64)
    b = np.asarray(tdew, np.float64)
    a, b = np.broadcast_arrays(a, b)
    with np.errstate(invalid="ignore"):
        ok = (a > PRESENT_ABOVE) & (b > PRESENT_ABOVE)  # a NaN compares false
        out = np.full(a.shape, NO_DEFICIT)
        np.subtract(a, b, out=out, where=ok)
    return out
