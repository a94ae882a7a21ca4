#!/usr/bin/env python3
"""Write tests/golden/fracture_p1_{name}.npz: example 03 (phase-field fracture, P1 on the native crack mesh) run by the numpy /
scipy restatement tests/fracture_reference.py with the reference's solver options: the mesh parameters and the mesh itself, the
log of attempts (step, k, alpha, its, reason, increment), the per-step counts, the largest c_conform per step and the final
z and z_prev.

Each run is repeated twice from an initial state perturbed by 1e-13 and 1e-11 (standard normal, absolute).  `sensitivity` is the
largest difference of the final state per field (u, c absolute; psi relative to max |psi|) between the run and the reruns.  A
golden is WRITTEN only if both reruns reproduce its log under the comparison rule (fracture_reference.logs_agree: failed attempts
compare on (step, k, alpha) and the fact of failure only); the tool refuses otherwise.  The committed files:

    python tools/make_fracture_golden.py A    # h 0.2, T 0 -> 1.2 in 7 points, write_frequency 2: damage localises (c_conform 0.98)
    python tools/make_fracture_golden.py B    # h 0.1, T 0 -> 1.0 in 6 points, write_frequency 1: diffuse damage only
    python tools/make_fracture_golden.py C    # h 0.2, T 0 -> 1.0 in 6 points, write_frequency 1: one natural failed attempt
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from proximalgalerkin_amd.mesh_generation import create_crack_mesh  # noqa: E402
from tests import fracture_reference as R  # noqa: E402

RUNS = {"A": dict(h=0.2, num_load_steps=7, Tmax=1.2, write_frequency=2),
        "B": dict(h=0.1, num_load_steps=6, Tmax=1.0, write_frequency=1),
        "C": dict(h=0.2, num_load_steps=6, Tmax=1.0, write_frequency=1),
        "D": dict(h=0.1, num_load_steps=9, Tmax=1.6, write_frequency=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name", choices=sorted(RUNS))
    ap.add_argument("--dry-run", action="store_true", help="measure and report, write nothing")
    a = ap.parse_args()
    p = RUNS[a.name]
    mesh, (edges, tags), names = create_crack_mesh(p["h"])
    P = R.Fracture(mesh.geometry, mesh.cells, R.boundary_vertices(edges, tags, names["topleft"]),
                   R.boundary_vertices(edges, tags, names["topright"]))
    kw = dict(num_load_steps=p["num_load_steps"], Tmin=0.0, Tmax=p["Tmax"], write_frequency=p["write_frequency"])
    run = R.solve(P, **kw)
    log = run["log"]
    failed = int(np.isnan(log[:, 5]).sum())
    print(f"{a.name}: {mesh.num_vertices} vertices, {len(log)} attempts, {int(run['newton_its'].sum())} Newton steps, {failed} failed, "
          f"max c_conform per step {np.round(run['max_conform'], 4).tolist()}", flush=True)
    sens = np.zeros(3)
    rng = np.random.default_rng(3)
    for scale in (1e-13, 1e-11):
        rerun = R.solve(P, z0=scale * rng.standard_normal(P.ndofs), **kw)
        ok = R.logs_agree(log, rerun["log"])
        d = R.field_differences(P.nv, rerun["z"], run["z"])
        print(f"  perturbed by {scale:g}: log {'agrees' if ok else 'DIFFERS'}, final state moved by u {d[0]:.2e} c {d[1]:.2e} psi(rel) {d[2]:.2e}",
              flush=True)
        if not ok:
            raise SystemExit(f"golden {a.name} is not reproducible under perturbation: not written")
        sens = np.maximum(sens, d)
    if a.dry_run:
        return
    out = ROOT / "tests" / "golden" / f"fracture_p1_{a.name}.npz"
    np.savez_compressed(out, h=p["h"], num_load_steps=p["num_load_steps"], Tmin=0.0, Tmax=p["Tmax"],
                        write_frequency=p["write_frequency"], coords=mesh.geometry, cells=mesh.cells, log=log,
                        newton_its=run["newton_its"], lvpp_its=run["lvpp_its"], max_conform=run["max_conform"], z=run["z"],
                        z_prev=run["z_prev"], sensitivity=sens)
    print("wrote", out, "sensitivity", sens)


if __name__ == "__main__":
    main()
