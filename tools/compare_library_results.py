#!/usr/bin/env python3
"""Do two builds of the library compute the same bytes?  The sibling of tools/compare_device_code.py for kernels whose
machine code was allowed to change: the general fp32 kernel (step_kernel_f32_coupled) and step_kernel_f32_lds are held
to the reference by distribution gates only (tests/test_hip_f32.py), so a changed bit would pass the suite.

For each library one fresh child process (ROADSURF_HIP_LIB set, one after the other, each under its own time limit)
runs the cases below through device.run_points and saves the six output series and the number of failed points; this
process compares them as raw bytes - NaN and -0.0 count - prints one line per case and exits 1 on any difference.
The cases are built by the tests' own builders (tests/test_hip_coupling.py, test_hip_skyview.py, test_hip_f32.py):
  coupling        the four configurations of test_hip_coupling._cases(300, 1441, 77) in fp32, configuration 1 in fp64 too
  coupling + sky  test_hip_f32._coupling_sky_case on _sky_case(200, 1441, 7, summer=True), NLayers 15 and 12
  general, no coupling   test_hip_f32._depth_cases(300, 1441, nl, 701): both depth configurations, (NLayers, chunk) =
                  (15, 0) and (12, 97) - state through store and load in mid-series, a failure inside a launch
  step_kernel_f32_lds    LEAN, NLayers 8, 300 x 1441, launches of 97 indices

usage: compare_library_results.py <libA.so> <libB.so>"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900  # seconds per library


def cases():
    """(name, forcing, settings, parameters, local parameters, run_points keywords)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import oracle_helpers as oh
    from roadsurf_amd import abi
    from test_hip_coupling import _cases
    from test_hip_f32 import _coupling_sky_case, _depth_cases
    from test_hip_skyview import _sky_case
    n, L = 300, 1441
    for k, (f, s, p, ls) in enumerate(_cases(n, L, 77)[0]):
        yield f"coupling {k} fp32", f, s, p, ls, dict(precision=32)
        if k == 1:
            yield f"coupling {k} fp64", f, s, p, ls, dict(precision=64)
    f, ls = _sky_case(200, L, 7, summer=True)
    for nl in (15, 12):
        g, s, p, ls2 = _coupling_sky_case(f, ls, L, nl)
        yield f"coupling + sky view NLayers {nl} fp32", g, s, p, ls2, dict(precision=32)
    for nl, chunk in ((15, 0), (12, 97)):
        _, p, ls, depth = _depth_cases(n, L, nl, 701)
        for what, g, s in depth:
            yield f"general {what} NLayers {nl} chunk {chunk} fp32", g, s, p, ls, dict(precision=32, chunk=chunk)
    s = abi.default_settings(L); s.NLayers = 8
    l = abi.default_local(); l.InitLenI = 1
    yield "lean NLayers 8 chunk 97 fp32", oh.synth_forcing(n, L, seed=3), s, abi.default_parameters(), l, \
        dict(precision=32, chunk=97)


def child(out_path):
    import numpy as np
    todo = list(cases())
    from roadsurf_amd import device
    saved = {}
    for name, f, s, p, ls, kw in todo:
        res, nfail = device.run_points(f, s, p, ls, **kw)
        for k in ("tsurf", "snow", "water", "ice", "deposit", "ice2"):
            saved[f"{name}|{k}"] = res[k]
        saved[f"{name}|nfail"] = np.array([nfail], np.int64)
    np.savez(out_path, **saved)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for tag, so in zip("AB", sys.argv[1:3]):
            out = os.path.join(tmp, tag + ".npz")
            env = dict(os.environ, ROADSURF_HIP_LIB=os.path.abspath(so))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, check=True,
                           timeout=CHILD_TIMEOUT)
            with np.load(out) as z:
                runs.append({k: z[k] for k in z.files})
    a, b = runs
    names = []
    for key in a:
        if key.split("|")[0] not in names:
            names.append(key.split("|")[0])
    bad = 0
    for name in names:
        diff = []
        for key in (k for k in a if k.split("|")[0] == name):
            x, y = a[key], b[key]
            if x.dtype != y.dtype or x.shape != y.shape:
                diff.append(f"{key.split('|')[1]}: {x.dtype}{x.shape} / {y.dtype}{y.shape}")
            elif x.tobytes() != y.tobytes():
                ne = x.view(f"u{x.itemsize}") != y.view(f"u{y.itemsize}")
                diff.append(f"{key.split('|')[1]}: {int(ne.sum())} of {ne.size} values")
        bad += bool(diff)
        print(f"{name}: " + ("DIFFERENT - " + "; ".join(diff) if diff else "equal"))
    print(f"{len(names) - bad} of {len(names)} cases equal")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
