#!/usr/bin/env python3
"""CPU study behind the degree-2 patch cycle on refined general meshes: Krylov iterations per Newton system of
the settings-B run with the twin of tests/p2_umg_reference.py as preconditioner - vertex-star smoother (nu = 2, omega = 0.8) over a
V(6,6), omega = 0.75 cycle of tests/umg_reference.py on (K1, M1, T^T D_P2 T) - against the same with an exact coarse solve, and
against the cycle WITHOUT the zeroing of the restricted residual on the u rows of Dirichlet vertices.  numpy / scipy only.

    python3 tools/p2_umg_proto.py [MESH ...] [--first K] [--no-mask]

MESH: disk:H:L = create_disk(H, refinements=L); x:NX:NY:L = the crossed NX x NY rectangle refined L times.  Default: disk:0.4:2
disk:0.34:2 x:3:2:3 disk:0.2:2.  --first K: systems K and later only (disk:0.2:3 has 5 149 vertices: --first 15)."""
import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def build(spec):
    from proximalgalerkin_amd import fem

    kind, *a = spec.split(":")
    if kind == "disk":
        return fem.create_disk(float(a[0]), refinements=int(a[1]))
    if kind == "x":
        msh = fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), (int(a[0]), int(a[1])), diagonal="crossed")
        for _ in range(int(a[2])):
            msh = fem.refine(msh)
        return msh
    raise SystemExit(f"unknown mesh {spec}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("meshes", nargs="*", default=["disk:0.4:2", "disk:0.34:2", "x:3:2:3", "disk:0.2:2"])
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--no-mask", action="store_true", help="also run the cycle without the Dirichlet zeroing of the restriction")
    a = ap.parse_args()
    from oracle import pg_oracle as O
    from tests import p2_umg_reference as Q

    for spec in a.meshes:
        msh = build(spec)
        prob = O.ObstacleLagrange(msh.geometry, msh.cells, 2)
        deg = Q.vertex_degrees(prob.edges, prob.nv)
        t0 = time.perf_counter()
        systems, hist = Q.record_systems(prob)
        print(f"{spec}: {prob.nv} vertices ({len(msh.hierarchy) + 1} levels), largest degree {deg.max()} ({int((deg >= 8).sum())} wide stars), "
              f"Newton {hist['Newton steps']}, {len(systems)} systems ({time.perf_counter() - t0:.1f} s)", flush=True)
        for k, (J, b, alpha) in enumerate(systems):
            if k < a.first:
                continue
            its = Q.krylov_count(prob, J, b, msh.hierarchy)[0]
            exact = Q.krylov_count(prob, J, b, msh.hierarchy, coarse="exact")[0]
            line = f"  system {k:2d} alpha {alpha:8.3f}: cycle {its:3d}  exact coarse solve {exact:3d}"
            if a.no_mask:
                line += f"  without the zeroing {Q.krylov_count(prob, J, b, msh.hierarchy, zero_dirichlet=False)[0]:3d}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
