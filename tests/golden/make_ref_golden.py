#!/usr/bin/env python3
"""Regenerates tests/golden/ref_*.npz.  REFERENCE-GENERATED: every number in these files was computed by the
reference's own solver core, compiled unchanged against the stand-in headers of oracle/ref_standin/
(`make -C oracle ref`, which needs a checkout of the reference; see oracle/Makefile).  The golden_*.npz,
sweeps22_*.npz and fields_*.npz files next to them are oracle-generated (make_golden.py).

    make -C oracle ref && python tests/golden/make_ref_golden.py

Per case (tests/reference_cases.py: the three domains of make_golden.py and one with partial tiles on every level):
the sha256 of every input array; the sha256 of every per-cell operator output on every level (labels, band lists,
apply, residual, Jacobi, each of three band passes, each of the four Gauss-Seidel passes in V-cycle order, both
transfers, the vector operations, the expansion); the reductions as numbers; full fp64 arrays for one and four
chained V-cycles per smoother; PCG iteration counts and residual histories.

`coarse_sensitivity` is the largest relative max-norm difference, over all cases and all V-cycle / PCG results,
between the build that carries the coarse Cholesky factorisation in double and the one that carries it in long
double: what a cycle can differ by through its direct solve alone.  test_reference_parity.py allows another direct
solver `tolerance_factor` times that.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import reference_cases as R  # noqa: E402
from oracle.mg_ref import Reference  # noqa: E402

TOLERANCE_FACTOR = 10.0
ARRAYS = ("vcycle1_jacobi", "vcycle4_jacobi", "vcycle1_gs", "vcycle4_gs")


def key(name):
    return name.replace("/", ".")


def build_case(ref, ref_ld, name):
    lab, w, off, lev, dx = R.solver_domain(name)
    out = {"offset": off, "levels_requested": lev, "dx": dx, "shape": np.array(lab.shape)}
    for group in (R.input_hashes(lab, w, dx), R.per_cell(ref, lab, w, lev, dx), R.expansion(ref, name), R.structure_checks(ref, lab, w, lev)):
        for k, v in group.items():
            out[key(k)] = np.array(v)
    for k, v in R.reductions(ref, lab).items():
        out["reduce." + k] = v
    cyc, cyc_ld = R.cycles(ref, lab, w, lev, dx), R.cycles(ref_ld, lab, w, lev, dx)
    sens = 0.0
    for k, v in cyc.items():
        if isinstance(v, np.ndarray):
            assert v.shape == cyc_ld[k].shape, k
            sens = max(sens, R.rel_max(cyc_ld[k], v))
            if k in ARRAYS or k.endswith("_history"):
                out[k] = v
            else:
                out[k + "_sha"] = np.array(R.sha(v))
        else:
            assert v == cyc_ld[k], k
            out[k] = v
    out["case_sensitivity"] = sens
    return out


def main():
    ref, ref_ld = Reference(), Reference(long_double=True)
    cases = {name: build_case(ref, ref_ld, name) for name in R.CASES}
    sensitivity = max(c["case_sensitivity"] for c in cases.values())
    for name, data in cases.items():
        data["coarse_sensitivity"] = sensitivity
        data["tolerance_factor"] = TOLERANCE_FACTOR
        path = os.path.join(HERE, f"ref_{name}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path) // 1024, "KiB, sensitivity of this case", data["case_sensitivity"])
    print("coarse_sensitivity", sensitivity, "tolerance", TOLERANCE_FACTOR * sensitivity)


if __name__ == "__main__":
    main()
