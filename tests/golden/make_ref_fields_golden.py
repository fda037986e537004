#!/usr/bin/env python3
"""Regenerates tests/golden/ref_fields_*.npz.  REFERENCE-GENERATED: every number in these files but the `device.*` ones was
computed by the reference's own plugin (HDK_GeometricFreeSurfacePressureSolver.cpp, HDK_Utilities.*) and solver core,
compiled unchanged against the stand-in headers of oracle/ref_standin/ (`make -C oracle ref`, which needs a checkout of
the reference; see oracle/Makefile).

    make -C oracle ref && python tests/golden/make_ref_fields_golden.py

Per scene (tests/reference_fields_cases.py): the sha256 of every input and of every per-pass output; the divergence
report's three numbers; the layout the reference chose; two whole solveGasSubclass runs with the multigrid
preconditioner, `tight.*` (tolerance 1e-10) and `loose.*` (the device test's tolerance), each as the float32 pressure on
the cells it is non-zero on, the float32 velocity on the valid faces, the valid faces and the iteration count; the
iteration count of the diagonal preconditioner at the device test's tolerance; and the measured numbers:

`case_sensitivity`: the largest relative max-norm difference of the solution grid (double; the plugin's own passes chained
with its own CG) between the build with the coarse Cholesky factorisation in double and the one in long double, over both
tolerances.  `sensitivity` is the maximum over the scenes; test_reference_fields_parity.py allows the oracle pipeline
`oracle_factor` times that.
`short_{mg,diag}_{p,v}`: the relative max-norm distance of pressure / velocity from the tight run to the reference's own run
at the device test's tolerance capped at the iteration count it converges with, that is one update short of convergence:
an iterate the reference itself rejects.  The device is allowed `device_factor` times that.
`device.{mg,diag}_{p,v}`: the distance the device was observed at (MI355X), for the record; MEASURED below.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import reference_fields_cases as F  # noqa: E402
from oracle.mg_ref import Reference, ReferenceFields  # noqa: E402

# device against the tight run, as tests/test_reference_fields_parity.py printed it on one MI355X: scene -> (mg_p, mg_v, diag_p, diag_v)
MEASURED = {
    "pool": (7.724e-06, 1.273e-06, 2.312e-05, 2.561e-06),
    "pool_solid": (9.859e-06, 1.530e-06, 1.604e-05, 2.480e-06),
    "edge": (3.141e-06, 1.064e-06, 2.378e-06, 2.742e-07),
}


def key(name):
    return name.replace("/", ".")


def distance(run, tight):
    """relative max-norm distance of the pressure and of the three velocity grids taken together"""
    flat = lambda r: np.concatenate([v.ravel() for v in r["velocity"]])  # noqa: E731
    return F.rel_max(run["pressure"], tight["pressure"]), F.rel_max(flat(run), flat(tight))


def build_scene(name, rf, rf_ld, core, core_ld):
    sc = F.scene(name)
    passes = F.reference_passes(rf, sc)
    out = {key(k): np.array(v) for k, v in {**F.hashes(F.inputs(sc)), **F.hashes(passes)}.items()}
    (eshape, off, levels), report = passes["layout"], passes["report"]
    out.update(expanded=np.array(eshape), offset=off, levels=levels, report=np.array(report), shape=np.array(sc["liquid_phi"].shape))
    tight = F.reference_solve(rf, sc, F.TIGHT_TOL)
    loose = F.reference_solve(rf, sc, F.DEVICE_TOL)
    for tag, run in (("tight.", tight), ("loose.", loose)):
        for k, v in F.pack_run(run, sc).items():
            out[tag + k] = v
    diag = F.reference_solve(rf, sc, F.DEVICE_TOL, use_mg=False)
    out["diag_iterations"] = diag["iterations"]
    # one update short of convergence: the cap is the iteration index the converging run leaves its loop at
    for tag, run, use_mg in (("mg", loose, True), ("diag", diag, False)):
        short = F.reference_solve(rf, sc, F.DEVICE_TOL, max_iterations=run["iterations"], use_mg=use_mg)
        assert short["iterations"] == run["iterations"] and short["info"]["rel_residual"] >= F.DEVICE_TOL > run["info"]["rel_residual"]
        out[f"short_{tag}_p"], out[f"short_{tag}_v"] = distance(short, tight)
        converged = distance(run, tight)
        assert converged[0] <= out[f"short_{tag}_p"] and converged[1] <= out[f"short_{tag}_v"], "a converged run lies no farther than the rejected one"
    sens = 0.0
    for tol in (F.TIGHT_TOL, F.DEVICE_TOL):
        x, it, p = F.reference_solution64(rf, core, sc, tol)
        x_ld, it_ld, _ = F.reference_solution64(rf_ld, core_ld, sc, tol)
        run = tight if tol == F.TIGHT_TOL else loose
        assert it == it_ld == run["iterations"] and np.array_equal(p, run["pressure"]), "the chained passes are the whole call"
        sens = max(sens, F.rel_max(x_ld, x))
    out["case_sensitivity"] = sens
    for k, v in zip(("mg_p", "mg_v", "diag_p", "diag_v"), MEASURED[name]):
        out["device." + k] = v
    return out


def main():
    rf, rf_ld, core, core_ld = ReferenceFields(), ReferenceFields(long_double=True), Reference(), Reference(long_double=True)
    assert rf.parameter_count() == 12
    scenes = {name: build_scene(name, rf, rf_ld, core, core_ld) for name in F.SCENES}
    sensitivity = max(s["case_sensitivity"] for s in scenes.values())
    for name, data in scenes.items():
        data.update(sensitivity=sensitivity, oracle_factor=F.ORACLE_FACTOR, device_factor=F.DEVICE_FACTOR, device_tolerance=F.DEVICE_TOL,
                    tight_tolerance=F.TIGHT_TOL)
        path = os.path.join(HERE, f"ref_fields_{name}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path) // 1024, "KiB; iterations", int(data["tight.iterations"]), int(data["loose.iterations"]), int(data["diag_iterations"]),
              "sensitivity", data["case_sensitivity"], "short", {k: float(data[k]) for k in data if k.startswith("short_")})
    print("sensitivity", sensitivity, "oracle tolerance", F.ORACLE_FACTOR * sensitivity)


if __name__ == "__main__":
    main()
