"""The notched plate with a hole of example 03, meshed natively.  Counterpart of the reference's
examples/03_fracture/generate_mesh.py (netgen): same polygon, same disk, same boundary names; the triangulation itself is this
package's (proximalgalerkin_amd.mesh_generation.create_crack_mesh), not netgen's.  Run as a script it writes mesh.vtu, and
facets.npz with the tagged boundary edges."""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd.mesh_generation import create_crack_mesh  # noqa: E402,F401


def main(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--res", "-r", type=float, default=0.05, help="Resolution of the mesh")
    parser.add_argument("--out", type=Path, default=Path("output"), help="Directory to write to")
    a = parser.parse_args(argv)
    from proximalgalerkin_amd import io

    mesh, (edges, tags), names = create_crack_mesh(max_res=a.res)
    a.out.mkdir(parents=True, exist_ok=True)
    io.write_vtu(a.out / "mesh.vtu", mesh.geometry, mesh.cells)
    np.savez(a.out / "facets.npz", edges=edges, tags=tags, names=list(names), values=list(names.values()))
    print(f"{mesh.num_vertices} vertices, {mesh.num_cells} cells, {len(edges)} boundary edges -> {a.out}", flush=True)


if __name__ == "__main__":
    main()
