"""Generate the half sphere for the contact problem - counterpart of the reference's examples/02_signorini/generate_mesh.py
(`lvpp.mesh_generation.create_half_sphere(res=0.04)` + XDMFFile.write_mesh / write_meshtags).  Then:

    python examples/02_signorini/signorini.py --filename meshes/half_sphere.xdmf --contact-tag 2 --displacement-tag 1

`--half-disk`: the plane geometry, `lvpp.mesh_generation.create_half_disk(c_y, R, res)` -> meshes/half_disk.xdmf (triangles, curved
boundary tagged 2, flat top tagged 1).  Then:

    python examples/02_signorini/signorini.py --alpha_0 0.005 --disp -0.1 --filename meshes/half_disk.xdmf
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd import io, mesh_generation  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=float, default=None, help="surface edge length (the reference's `res`; default 0.04, half disk 0.05)")
    ap.add_argument("--output", type=Path, default=None, help="default meshes/half_sphere.xdmf (meshes/half_disk.xdmf with --half-disk)")
    ap.add_argument("--half-disk", dest="half_disk", action="store_true", help="the 2-D half disk instead of the half sphere")
    ap.add_argument("--c-y", dest="c_y", type=float, default=0.4, help="half disk: y coordinate of the flat top")
    ap.add_argument("--R", type=float, default=0.4, help="half disk: radius")
    a = ap.parse_args()
    if a.half_disk:
        out = a.output or Path("meshes/half_disk.xdmf")
        mesh, _, edge_marker = mesh_generation.create_half_disk(c_y=a.c_y, R=a.R, res=0.05 if a.res is None else a.res)
        io.write_xdmf_tri(out, mesh, edge_marker)
        print(f"{out}: {mesh.geometry.shape[0]} vertices, {mesh.cells.shape[0]} triangles, "
              f"{len(edge_marker[2])} contact edges (tag 2), {len(edge_marker[1])} displacement edges (tag 1)")
        sys.exit(0)
    a.res = 0.04 if a.res is None else a.res
    a.output = a.output or Path("meshes/half_sphere.xdmf")
    mesh, cell_marker, facet_marker = mesh_generation.create_half_sphere(res=a.res)
    io.write_xdmf_tet(a.output, mesh, facet_marker)
    print(f"{a.output}: {mesh.geometry.shape[0]} vertices, {mesh.cells.shape[0]} tetrahedra, "
          f"{len(facet_marker.find(2))} contact facets (tag 2), {len(facet_marker.find(1))} displacement facets (tag 1)")
