"""Example 02 - Signorini contact of a linear-elastic body with a rigid plane - on the HIP backend.

Host-side mirror of /root/reference/examples/02_signorini/signorini_dolfinx.py: `solve_contact_problem` keeps the
reference's signature (:156-174) and loop (:317-358); `SignoriniProblem` stands where the script builds the blocked
`dolfinx.fem.petsc.NonlinearProblem(F, [u, psi], bcs=bcs, entity_maps=..., petsc_options=...)` (:281-291) and exposes
`.solve()`, `.solver.setTolerances(atol=, rtol=)`, `.solver.getIterationNumber()`, `.solver.getConvergedReason()`
(:331-335).  Everything below `.solve()` runs in libpgx.so (include/pgx_sg.h).  No CPU fallback.

Degrees 1 (BASELINE.json config 5) and 2 (the reference's default, :68-73) on tetrahedra (`TetMesh`) and on the reference's native
hexahedral box grid (`HexMesh`, :376-383; Q1 / Q2 elements).  The forms-driven `NonlinearProblem` below takes both degrees.

PLANE problems (the script with gdim = 2: `native --dim 2`, the half disk of `mesh_generation.create_half_disk`): a triangular
`fem.Mesh` or a `fem.QuadMesh` instead of `TetMesh` / `HexMesh`; facets are then EDGES given as vertex pairs, the state is
[u_x | u_y | psi], the rigid line is y = gap (include/pgx_sg.h: pgx_sg_create_2d).  Declarative driver only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Literal

import numpy as np

from . import _lib, fem
from ._mixed import _MixedHandle
from .problem import _SNES

AlphaScheme = Literal["constant", "linear", "doubling"]


_TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_TRI_EDGES = ((0, 1), (0, 2), (1, 2))


@dataclass
class TetMesh:
    geometry: np.ndarray  # (nv,3)
    cells: np.ndarray  # (nc,4)
    # ORDER-2 GEOMETRY (round 5): the geometry's mid-edge node of every edge, edges ordered by their (min, max) vertex pair - the
    # numbering of `edges()` and of p2_nodes - as a mesh of 10-node tetrahedra carries them (the reference's half sphere:
    # lvpp/mesh_generation.py:88,158).  None, or every node at its edge's midpoint: affine cells.
    midside: np.ndarray | None = None

    def __post_init__(self):
        if self.midside is not None:
            self.midside = np.ascontiguousarray(self.midside, dtype=np.float64)
            e = self.edges()
            if self.midside.shape != (len(e), 3):
                raise ValueError(f"midside must be (n_edges, 3) = {(len(e), 3)}")
            straight = 0.5 * (self.geometry[e[:, 0]] + self.geometry[e[:, 1]])
            length = np.linalg.norm(self.geometry[e[:, 0]] - self.geometry[e[:, 1]], axis=1)
            if not np.any(np.linalg.norm(self.midside - straight, axis=1) > 1e-13 * length):
                self.midside = None

    @property
    def curved(self):
        return self.midside is not None

    def flattened(self):
        """the same mesh with affine cells (what a degree-1 run uses)"""
        return TetMesh(self.geometry, self.cells) if self.curved else self

    def edges(self):
        """(ne, 2) sorted unique (min, max) vertex pairs - the edge numbering of p2_nodes and of `midside`"""
        c = self.cells.astype(np.int64)
        nv = self.geometry.shape[0]
        pairs = np.sort(np.concatenate([c[:, list(e)] for e in _TET_EDGES]), axis=1)
        ukey = np.unique(pairs[:, 0] * nv + pairs[:, 1])
        return np.stack([ukey // nv, ukey % nv], axis=1)

    def facets_where(self, pred):
        """Exterior triangles (vertex triples) whose three vertices satisfy pred(x) (locate_entities_boundary, :369-373)."""
        on = pred(self.geometry.T)
        c = self.cells
        faces = np.concatenate([c[:, [1, 2, 3]], c[:, [0, 2, 3]], c[:, [0, 1, 3]], c[:, [0, 1, 2]]])
        sel = faces[on[faces].all(axis=1)]
        key = np.sort(sel, axis=1)
        _, idx, cnt = np.unique(key, axis=0, return_index=True, return_counts=True)
        idx = idx[cnt == 1]  # exterior: the face belongs to exactly one cell
        return np.ascontiguousarray(sel[np.sort(idx)], dtype=np.int32)


class MeshTags:
    """facet_tag of the reference (:384-385): tag -> facets (vertex triples; `width` = 2: the vertex pairs of a plane mesh's edges);
    `.find(tag)` as dolfinx.mesh.MeshTags."""

    def __init__(self, tagged: dict, width: int = 3):
        self._t = {int(k): np.ascontiguousarray(v, dtype=np.int32) for k, v in tagged.items()}
        self._width = int(width)

    def find(self, tag):
        return self._t.get(int(tag), np.zeros((0, self._width), dtype=np.int32))


def _tagged(facet_tag, tags, width):
    """facets of all `tags`: from a MeshTags or from the {marker: facets} dict `mesh_generation.create_half_disk` returns"""
    find = facet_tag.find if hasattr(facet_tag, "find") else (lambda t: facet_tag.get(int(t), np.zeros((0, width), dtype=np.int32)))
    return np.concatenate([np.asarray(find(t), dtype=np.int32).reshape(-1, width) for t in tags])


def p2_nodes_tri(mesh: fem.Mesh, *edge_sets):
    """Degree-2 node numbering of a triangular mesh (include/pgx_sg.h, plane problems): the vertices, then one node per edge in
    `Mesh.edges()` order, at the edge midpoint.  Returns (node_coords, cells6 - vertices, then the edge nodes of (0,1) (0,2) (1,2) -,
    [edges3 - the two vertices, then the midpoint node - for every set of edges given as vertex pairs])."""
    nv = mesh.num_vertices
    edges, cell_edges = mesh.edges()  # local edge i is OPPOSITE local vertex i
    cells6 = np.ascontiguousarray(np.concatenate([mesh.cells, nv + cell_edges[:, [2, 1, 0]]], axis=1), dtype=np.int32)
    coords = np.ascontiguousarray(np.concatenate([mesh.geometry, 0.5 * (mesh.geometry[edges[:, 0]] + mesh.geometry[edges[:, 1]])]))
    key = edges[:, 0].astype(np.int64) * nv + edges[:, 1]
    out = []
    for e in edge_sets:
        e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
        k = e.min(axis=1) * nv + e.max(axis=1)
        pos = np.searchsorted(key, k)
        if len(e) and not np.array_equal(key[np.minimum(pos, len(key) - 1)], k):
            raise ValueError("a facet is not an edge of the mesh")
        out.append(np.ascontiguousarray(np.concatenate([e, (nv + pos)[:, None]], axis=1), dtype=np.int32))
    return coords, cells6, out


def quad_lattice(mesh: fem.QuadMesh, d: int):
    """(node coordinates, cells [nc][(d+1)^2]) of the Q_d discretisation of a structured quadrilateral grid: the vertex lattice refined
    d times, nodes and local nodes lexicographic (x fastest)"""
    nx, ny = mesh.structured
    (x0, y0), (x1, y1) = mesh.box
    Nx, Ny = d * nx + 1, d * ny + 1
    coords = np.ascontiguousarray(np.stack([np.tile(np.linspace(x0, x1, Nx), Ny), np.repeat(np.linspace(y0, y1, Ny), Nx)], axis=1))
    cy, cx = np.repeat(np.arange(ny), nx), np.tile(np.arange(nx), ny)
    cells = np.stack([(d * cy + iy) * Nx + d * cx + ix for iy in range(d + 1) for ix in range(d + 1)], axis=1)
    return coords, np.ascontiguousarray(cells, dtype=np.int32)


def quad_edge_nodes(mesh: fem.QuadMesh, edges, d: int):
    """Q_d nodes (lexicographic along the edge) of grid edges given by their two corner vertices"""
    nx, ny = mesh.structured
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    Nx = d * nx + 1
    i, j = e % (nx + 1), e // (nx + 1)
    n = (d * j) * Nx + d * i  # the corners on the refined lattice
    lo, hi = n.min(axis=1), n.max(axis=1)
    if len(e) and not np.all((np.abs(i[:, 0] - i[:, 1]) + np.abs(j[:, 0] - j[:, 1])) == 1):
        raise ValueError("a facet is not an edge of the grid")
    return np.ascontiguousarray(np.stack([lo + k * (hi - lo) // d for k in range(d + 1)], axis=1), dtype=np.int32)


def boundary_edges_where(mesh, pred):
    """Exterior edges (vertex pairs) of a triangular fem.Mesh or a fem.QuadMesh whose two vertices satisfy pred(x)
    (locate_entities_boundary, :369-373)."""
    c = mesh.cells
    loc = ((0, 1), (1, 3), (3, 2), (2, 0)) if isinstance(mesh, fem.QuadMesh) else ((0, 1), (1, 2), (2, 0))
    e = np.concatenate([c[:, list(ab)] for ab in loc])
    on = pred(mesh.geometry.T)
    sel = e[on[e].all(axis=1)]
    _, idx, cnt = np.unique(np.sort(sel, axis=1), axis=0, return_index=True, return_counts=True)
    return np.ascontiguousarray(sel[np.sort(idx[cnt == 1])], dtype=np.int32)



def p2_nodes(mesh: TetMesh, *facet_sets):
    """Degree-2 node numbering of include/pgx_sg.h: the mesh vertices, then one node per edge (edges ordered by their (min, max)
    vertex pair), at the edge midpoint (a curved mesh: at the geometry's mid-edge node).  Returns (node_coords, cells10, [facets6 for every facet set])."""
    cells = mesh.cells.astype(np.int64)
    nv = mesh.geometry.shape[0]
    pairs = np.sort(np.concatenate([cells[:, list(e)] for e in _TET_EDGES]), axis=1)
    key = pairs[:, 0] * nv + pairs[:, 1]
    ukey, inv = np.unique(key, return_inverse=True)
    nc = len(cells)
    cells10 = np.ascontiguousarray(np.concatenate([cells, nv + inv.reshape(6, nc).T], axis=1), dtype=np.int32)
    e0, e1 = ukey // nv, ukey % nv
    mid = mesh.midside if getattr(mesh, "midside", None) is not None else 0.5 * (mesh.geometry[e0] + mesh.geometry[e1])
    coords = np.ascontiguousarray(np.concatenate([mesh.geometry, mid]))  # order-2 geometry: an edge node sits on the mid-edge node
    out = []
    for f in facet_sets:
        f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
        fp = np.sort(np.concatenate([f[:, list(e)] for e in _TRI_EDGES]), axis=1) if len(f) else np.zeros((0, 2), dtype=np.int64)
        pos = np.searchsorted(ukey, fp[:, 0] * nv + fp[:, 1])
        if len(f) and not np.array_equal(ukey[pos], fp[:, 0] * nv + fp[:, 1]):
            raise ValueError("a facet edge is not an edge of the mesh")
        out.append(np.ascontiguousarray(np.concatenate([f, nv + pos.reshape(3, len(f)).T], axis=1), dtype=np.int32))
    return coords, cells10, out


@dataclass
class HexMesh:
    """dolfinx.mesh.create_unit_cube(comm, nx, ny, nz, CellType.hexahedron) - the reference's NATIVE mesh (signorini_dolfinx.py:376-383):
    a structured grid of boxes.  `geometry` / `cells` are the vertex lattice (nv, 3) and the 8 corner vertices per cell, numbered
    lexicographically (x fastest); the Q_d nodes of include/pgx_sg.h are the lattice refined d times (`lattice(d)`)."""
    nx: int
    ny: int
    nz: int

    def _lat(self, d):
        Nx, Ny, Nz = d * self.nx + 1, d * self.ny + 1, d * self.nz + 1
        Z, Y, X = np.meshgrid(np.linspace(0, 1, Nz), np.linspace(0, 1, Ny), np.linspace(0, 1, Nx), indexing="ij")
        return np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)), (Nx, Ny, Nz)

    @property
    def geometry(self):
        return self._lat(1)[0]

    @property
    def cells(self):
        return self.lattice(1)[1]

    def lattice(self, d):
        """(node coordinates, cells [nc][(d+1)^3]) of the Q_d discretisation, local nodes lexicographic"""
        coords, (Nx, Ny, Nz) = self._lat(d)
        cz, cy, cx = np.meshgrid(np.arange(self.nz), np.arange(self.ny), np.arange(self.nx), indexing="ij")
        cx, cy, cz = cx.ravel(), cy.ravel(), cz.ravel()
        cells = np.stack([((d * cz + iz) * Ny + d * cy + iy) * Nx + d * cx + ix
                          for iz in range(d + 1) for iy in range(d + 1) for ix in range(d + 1)], axis=1)
        return coords, np.ascontiguousarray(cells, dtype=np.int32)

    def facets_where(self, pred):
        """Exterior faces (4 corner vertices of the vertex lattice, lexicographic within the face) whose corners satisfy pred(x)."""
        nx, ny, nz = self.nx, self.ny, self.nz
        Nx, Ny = nx + 1, ny + 1
        vid = lambda gx, gy, gz: (gz * Ny + gy) * Nx + gx  # noqa: E731
        out = []
        j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        for gz in (0, nz):
            out.append(np.stack([vid(i, j, gz), vid(i + 1, j, gz), vid(i, j + 1, gz), vid(i + 1, j + 1, gz)], axis=-1).reshape(-1, 4))
        k, i = np.meshgrid(np.arange(nz), np.arange(nx), indexing="ij")
        for gy in (0, ny):
            out.append(np.stack([vid(i, gy, k), vid(i + 1, gy, k), vid(i, gy, k + 1), vid(i + 1, gy, k + 1)], axis=-1).reshape(-1, 4))
        k, j = np.meshgrid(np.arange(nz), np.arange(ny), indexing="ij")
        for gx in (0, nx):
            out.append(np.stack([vid(gx, j, k), vid(gx, j + 1, k), vid(gx, j, k + 1), vid(gx, j + 1, k + 1)], axis=-1).reshape(-1, 4))
        faces = np.concatenate(out)
        on = pred(self.geometry.T)
        return np.ascontiguousarray(faces[on[faces].all(axis=1)], dtype=np.int32)

    def facet_nodes(self, faces, d):
        """Q_d nodes (lexicographic within the face) of faces given by their 4 corner vertices"""
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 4)
        Nx1, Ny1 = self.nx + 1, self.ny + 1
        Nx, Ny = d * self.nx + 1, d * self.ny + 1

        def ijk(v):
            return np.stack([v % Nx1, (v // Nx1) % Ny1, v // (Nx1 * Ny1)], axis=-1)

        c0, e1, e2 = ijk(faces[:, 0]), ijk(faces[:, 1]) - ijk(faces[:, 0]), ijk(faces[:, 2]) - ijk(faces[:, 0])
        nodes = []
        for iy in range(d + 1):
            for ix in range(d + 1):
                g = d * c0 + ix * e1 + iy * e2
                nodes.append((g[:, 2] * Ny + g[:, 1]) * Nx + g[:, 0])
        return np.ascontiguousarray(np.stack(nodes, axis=1), dtype=np.int32)


def create_unit_cube_hex(nx, ny, nz) -> HexMesh:
    return HexMesh(int(nx), int(ny), int(nz))


def create_unit_cube(nx, ny, nz) -> TetMesh:
    """nx x ny x nz cubes, six tetrahedra each around the diagonal v0-v7 (dolfinx.mesh.create_unit_cube with
    CellType.tetrahedron [split pattern recalled, not verifiable offline])."""
    xs, ys, zs = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), np.linspace(0, 1, nz + 1)
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    coords = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1))
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v0 = (iz * (ny + 1) * (nx + 1) + iy * (nx + 1) + ix).ravel()
    v1, v2 = v0 + 1, v0 + (nx + 1)
    v3 = v1 + (nx + 1)
    off = (nx + 1) * (ny + 1)
    v4, v5, v6, v7 = v0 + off, v1 + off, v2 + off, v3 + off
    tets = [(v0, v1, v3, v7), (v0, v1, v7, v5), (v0, v5, v7, v4), (v0, v3, v2, v7), (v0, v6, v4, v7), (v0, v2, v6, v7)]
    cells = np.stack([np.stack(t, axis=1) for t in tets], axis=1).reshape(-1, 4)
    return TetMesh(coords, np.ascontiguousarray(cells, dtype=np.int32))


def native_tags(mesh: TetMesh) -> tuple[MeshTags, dict]:
    """The `native` branch of the reference's __main__ (:365-386): top (z = 1; the unit square: y = 1) tagged 1, bottom (z = 0; y = 0)
    tagged 2."""
    if isinstance(mesh, (fem.Mesh, fem.QuadMesh)):
        top = boundary_edges_where(mesh, lambda x: np.isclose(x[1], 1.0))
        bottom = boundary_edges_where(mesh, lambda x: np.isclose(x[1], 0.0))
        return MeshTags({1: top, 2: bottom}, width=2), {"contact": (2,), "displacement": (1,)}
    top = mesh.facets_where(lambda x: np.isclose(x[2], 1.0))
    bottom = mesh.facets_where(lambda x: np.isclose(x[2], 0.0))
    return MeshTags({1: top, 2: bottom}), {"contact": (2,), "displacement": (1,)}


def curved_tables(node_coords, cells10, facets6, cell_qpts, facet_qpts):
    """The two geometry tables of include/pgx_sg.h `pgx_sg_curved` for a mesh of 10-node tetrahedra: per cell and cell quadrature
    point |det J| and J^-1 (row-major, d xi_k / d x_d) of x(xi) = sum_a X_a N2_a(xi); per contact facet and facet quadrature point the
    surface element |x_xi x x_eta| of the 6-node triangle and its z coordinate.  Node orders of p2_nodes."""
    gref3 = np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    L = np.concatenate([1.0 - cell_qpts.sum(axis=1, keepdims=True), cell_qpts], axis=1)
    dN = np.empty((len(L), 10, 3))
    for a in range(4):
        dN[:, a] = (4 * L[:, a] - 1)[:, None] * gref3[a][None]
    for k, (a, b) in enumerate(_TET_EDGES):
        dN[:, 4 + k] = 4 * (L[:, a][:, None] * gref3[b][None] + L[:, b][:, None] * gref3[a][None])
    J = np.einsum("cad,qak->cqdk", node_coords[cells10], dN)
    det = np.linalg.det(J)
    if np.any(det.min(axis=1) * det.max(axis=1) <= 0):  # (a cell may be negatively oriented as a whole: |det J| is what enters)
        raise ValueError("order-2 geometry: the cell map is not orientation preserving at every quadrature point")
    cgeo = np.ascontiguousarray(np.concatenate([np.abs(det)[..., None], np.linalg.inv(J).reshape(len(cells10), len(L), 9)], axis=2))
    gref2 = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]])
    L3 = np.stack([1.0 - facet_qpts[:, 0] - facet_qpts[:, 1], facet_qpts[:, 0], facet_qpts[:, 1]], axis=1)
    N6 = np.concatenate([L3 * (2 * L3 - 1), np.stack([4 * L3[:, a] * L3[:, b] for a, b in _TRI_EDGES], axis=1)], axis=1)
    dT = np.empty((len(L3), 6, 2))
    for a in range(3):
        dT[:, a] = (4 * L3[:, a] - 1)[:, None] * gref2[a][None]
    for k, (a, b) in enumerate(_TRI_EDGES):
        dT[:, 3 + k] = 4 * (L3[:, a][:, None] * gref2[b][None] + L3[:, b][:, None] * gref2[a][None])
    X6 = node_coords[facets6]
    t = np.einsum("fad,qak->fqdk", X6, dT)
    ds = np.linalg.norm(np.cross(t[..., 0], t[..., 1]), axis=2)
    zq = np.einsum("qa,fa->fq", N6, X6[:, :, 2])
    return cgeo, np.ascontiguousarray(np.stack([ds, zq], axis=2))


class SignoriniProblem(_MixedHandle):
    """x = [u_x | u_y | u_z | psi (contact vertices ordered by vertex id)]; on a plane mesh (fem.Mesh / fem.QuadMesh) x = [u_x | u_y | psi]."""

    _prefix = "pgx_sg"

    def __init__(self, mesh: TetMesh, contact_facets, bc_vertices, E, nu, gap, disp, quadrature_degree=4, device=0, comm=None, degree=1,
                 bc_facets=None, cell_quadrature_degree=None):
        """degree 2 (the reference's default): the Dirichlet NODES come from `bc_vertices` if given (node ids of p2_nodes), else from
        `bc_facets` (the displacement facets: vertices and edge nodes).  State layout [u_x | u_y | u_z | psi] over the P2 nodes.
        A CURVED TetMesh (order-2 geometry, `mesh.midside`) is integrated on its quadratic cells and facets (pgx_sg_create_curved):
        degree 2 isoparametrically, degree 1 with P1 fields on the curved cells; the cell integrals then use a Gauss-Jacobi rule of
        degree `cell_quadrature_degree` - the reference leaves that degree to UFL's estimator: 2 (degree - 1) for the integrand + 3 for
        det J of a quadratic tetrahedron, the default here."""
        self._lib = lib = _lib.load()
        self.mesh = mesh
        self.degree = int(degree)
        self.gdim = 2 if isinstance(mesh, (fem.Mesh, fem.QuadMesh)) else 3
        if self.gdim == 2:
            if comm is not None:
                raise NotImplementedError("plane problems: single handle only (include/pgx_sg.h: pgx_sg_create_dist is 3-D)")
            self._create_2d(contact_facets, bc_vertices, bc_facets, E, nu, gap, disp, quadrature_degree, device)
            self._finish()
            return
        pts, wts = fem.quadrature_rule("triangle", quadrature_degree)
        self.cell_type = 1 if isinstance(mesh, HexMesh) else 0
        if self.cell_type == 1:  # the reference's native mesh: Q_d on the structured box grid
            if self.degree not in (1, 2):
                raise NotImplementedError("HIP backend: degrees 1 and 2")
            if bc_facets is None:
                raise ValueError("hexahedral meshes need the displacement FACETS")
            coords, cells = mesh.lattice(self.degree)
            facets = mesh.facet_nodes(contact_facets, self.degree)
            bv = np.unique(mesh.facet_nodes(bc_facets, self.degree).ravel()).astype(np.int64)
            g, w1 = np.polynomial.legendre.leggauss(3)  # 3 x 3 Gauss-Legendre on the unit square (degree 5 >= quadrature_degree 4)
            g, w1 = 0.5 * (g + 1.0), 0.5 * w1
            pts = np.ascontiguousarray([(g[a], g[b]) for b in range(3) for a in range(3)])
            wts = np.ascontiguousarray([w1[a] * w1[b] for b in range(3) for a in range(3)])
        elif self.degree == 2:
            if bc_facets is None and bc_vertices is None:
                raise ValueError("degree 2 needs the Dirichlet nodes or the displacement FACETS (their edge nodes are constrained as well)")
            coords, cells, (facets, bf6) = p2_nodes(mesh, contact_facets, bc_facets if bc_vertices is None else np.zeros((0, 3), np.int32))
            bv = (np.unique(bf6.ravel()) if bc_vertices is None else np.asarray(bc_vertices)).astype(np.int64)
        elif self.degree == 1:
            coords, cells = mesh.geometry, mesh.cells
            facets = np.ascontiguousarray(contact_facets, dtype=np.int32)
            bv = np.asarray(bc_vertices, dtype=np.int64)
        else:
            raise NotImplementedError("HIP backend: degrees 1 and 2")
        self.node_coords = coords
        self.cells, self.facets = cells, facets  # node ids, the orders of include/pgx_sg.h
        self.E, self.nu, self.gap = float(E), float(nu), float(gap)
        self.facet_quadrature = (pts, wts)
        nv = coords.shape[0]
        bc = np.ascontiguousarray(np.concatenate([bv, nv + bv, 2 * nv + bv]), dtype=np.int32)  # all components (:267)
        vals = np.ascontiguousarray(np.concatenate([np.zeros(len(bv)), np.zeros(len(bv)), np.full(len(bv), float(disp))]))
        self._keep = (coords, cells, facets, pts, wts, bc, vals)
        pm = _lib.pgx_sg_mesh(nv, cells.shape[0], _lib.dptr(coords), _lib.iptr(cells), facets.shape[0], _lib.iptr(facets), self.degree,
                              self.cell_type)
        pp = _lib.pgx_sg_problem(float(E), float(nu), float(gap), len(wts), _lib.dptr(pts), _lib.dptr(wts), len(bc),
                                 _lib.iptr(bc), _lib.dptr(vals))
        self._h = C.c_void_p()
        curved = self.cell_type == 0 and getattr(mesh, "curved", False)
        if curved and comm is not None:
            raise NotImplementedError("order-2 geometry: single handle only (include/pgx_sg.h pgx_sg_create_curved)")
        if curved:
            # isoparametric P2 on the 10-node tetrahedra: the library takes the geometry as tables over the quadrature points
            qdeg = 2 * (self.degree - 1) + 3 if cell_quadrature_degree is None else int(cell_quadrature_degree)
            qp3, qw3 = fem.quadrature_rule("tetrahedron", qdeg)
            if self.degree == 2:
                cgeo, fgeo = curved_tables(coords, cells, facets, qp3, pts)
            else:  # P1 fields: the geometry tables come from the 10-node cells / 6-node facets, the mesh arrays stay the vertices'
                gcoords, g10, (g6,) = p2_nodes(mesh, facets)
                cgeo, fgeo = curved_tables(gcoords, g10, g6, qp3, pts)
            self._keep_curved = (qp3, qw3, cgeo, fgeo)
            cv = _lib.pgx_sg_curved(len(qw3), _lib.dptr(qp3), _lib.dptr(qw3), _lib.dptr(cgeo), _lib.dptr(fgeo))
            rc = lib.pgx_sg_create_curved(C.byref(pm), C.byref(pp), C.byref(cv), int(device), C.byref(self._h))
        elif comm is None:
            rc = lib.pgx_sg_create(C.byref(pm), C.byref(pp), int(device), C.byref(self._h))
        else:  # one handle per GPU, distributed sparse LU (include/pgx_sg.h); every call below is collective
            self._comm = comm
            rc = lib.pgx_sg_create_dist(C.byref(pm), C.byref(pp), comm._c, int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_sg_last_error(None)
            raise _lib.PgxError(f"pgx_sg_create failed (code {rc}): {msg.decode() if msg else ''}")
        self._finish()

    def _create_2d(self, contact_edges, bc_vertices, bc_edges, E, nu, gap, disp, quadrature_degree, device):
        """pgx_sg_create_2d: triangles (P1 / P2) or the structured quadrilateral grid (Q1 / Q2); contact and displacement facets are
        edges given as vertex pairs; Dirichlet data (0, disp) at the nodes of the displacement edges (edge nodes included)."""
        lib, mesh, d = self._lib, self.mesh, self.degree
        if d not in (1, 2):
            raise NotImplementedError("HIP backend: degrees 1 and 2")
        if bc_edges is None and bc_vertices is None:
            raise ValueError("plane problems need the Dirichlet nodes or the displacement EDGES")
        none = np.zeros((0, 2), np.int32)
        self.cell_type = 1 if isinstance(mesh, fem.QuadMesh) else 0
        if self.cell_type == 1:
            coords, cells = quad_lattice(mesh, d)
            facets = quad_edge_nodes(mesh, contact_edges, d)
            be = quad_edge_nodes(mesh, none if bc_edges is None else bc_edges, d)
        else:
            if mesh.curved:
                raise NotImplementedError("plane contact on curved (order-2 geometry) triangles is not implemented: pass mesh.flattened()")
            if d == 2:
                coords, cells, (facets, be) = p2_nodes_tri(mesh, contact_edges, none if bc_edges is None else bc_edges)
            else:
                coords, cells = mesh.geometry, mesh.cells
                facets = np.ascontiguousarray(np.asarray(contact_edges, dtype=np.int32).reshape(-1, 2))
                be = np.asarray(none if bc_edges is None else bc_edges, dtype=np.int32).reshape(-1, 2)
        bv = (np.unique(be.ravel()) if bc_vertices is None else np.asarray(bc_vertices)).astype(np.int64)
        pts, wts = fem.interval_quadrature(quadrature_degree)  # basix's default on the interval (:211-218 metadata)
        self.node_coords = coords
        self.cells, self.facets = cells, facets  # node ids, the orders of include/pgx_sg.h
        self.E, self.nu, self.gap = float(E), float(nu), float(gap)
        self.facet_quadrature = (pts, wts)
        nv = coords.shape[0]
        bc = np.ascontiguousarray(np.concatenate([bv, nv + bv]), dtype=np.int32)  # all components (:267)
        vals = np.ascontiguousarray(np.concatenate([np.zeros(len(bv)), np.full(len(bv), float(disp))]))
        self._keep = (coords, cells, facets, pts, wts, bc, vals)
        pm = _lib.pgx_sg_mesh2d(nv, cells.shape[0], _lib.dptr(coords), _lib.iptr(cells), facets.shape[0], _lib.iptr(facets), d, self.cell_type)
        pp = _lib.pgx_sg_problem2d(float(E), float(nu), float(gap), len(wts), _lib.dptr(pts), _lib.dptr(wts), len(bc), _lib.iptr(bc),
                                   _lib.dptr(vals))
        self._h = C.c_void_p()
        rc = lib.pgx_sg_create_2d(C.byref(pm), C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_sg_last_error(None)
            raise _lib.PgxError(f"pgx_sg_create_2d failed (code {rc}): {msg.decode() if msg else ''}")

    def _finish(self):
        lib, nv = self._lib, self.node_coords.shape[0]
        nt, npsi = C.c_int64(0), C.c_int64(0)
        lib.pgx_sg_num_dofs(self._h, C.byref(nt), C.byref(npsi))
        self.ndofs, self.npsi, self.nv = nt.value, npsi.value, nv
        self.contact_vertices = np.zeros(self.npsi, dtype=np.int32)
        lib.pgx_sg_contact_vertices(self._h, _lib.iptr(self.contact_vertices))
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))  # PETSc defaults: stol 1e-8, max_it 50 (the script sets atol/rtol only)
        self._opts.ksp_max_it = 6
        self._flags = {"snes_error_if_not_converged": True}  # :278
        self.solver = _SNES(self._opts)

    def u_increment(self):
        return self._scalar("u_increment")

    # -- what the script reports about an iterate (signorini_dolfinx.py:293-321, 346-350), evaluated on the device state -------------
    def penetration(self):
        """|| max(u.n_g - g, 0) ||_L2(Gamma) with the facet rule of the residual (:307-314)"""
        return self._scalar("penetration")

    def violation(self):
        """u.n_g - g at every node (:307-308, 349)"""
        out = np.empty(self.nv)
        self._call("violation", _lib.dptr(out))
        return out

    def von_mises(self):
        """(n_cells, nodes per cell): the von-Mises stress at each cell's own nodes - its DG_degree interpolant (:296-302, 346).  Affine
        cells only (include/pgx_sg.h)."""
        out = np.empty(self.cells.shape)
        self._call("von_mises", _lib.dptr(out))
        return out

    def partition_info(self):
        """(cells whose element matrices this rank assembled, cells of the mesh): equal on a single handle; a distributed handle
        assembles its slab only (include/pgx_sg.h: pgx_sg_create_dist)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._call("partition_info", C.byref(a), C.byref(b))
        return a.value, b.value

    def lu_stats(self) -> dict:
        st = _lib.pgx_nd_stats()
        self._call("lu_stats", C.byref(st))
        out = {k: getattr(st, k) for k, _ in st._fields_}
        out["symmetric"] = bool(self._lib.pgx_sg_lu_is_symmetric(self._h))  # L D L^T in LU clothing: about half of `flops` executed
        return out


def solve_contact_problem(mesh: TetMesh, facet_tag: MeshTags, boundary_conditions: dict, degree: int = 1, E: float = 2.0e4,
                          nu: float = 0.3, gap: float = 0.0, disp: float = -0.25, newton_max_its: int = 250,
                          newton_tol: float = 1e-6, max_iterations: int = 25, alpha_scheme: AlphaScheme = "doubling",
                          alpha_0: float = 1.0, alpha_c: float = 1.0, tol: float = 1e-6, output: Path | None = None,
                          quadrature_degree: int = 4, verbose: bool = True, return_solution: bool = False, device: int = 0,
                          comm=None, penetration_history: list | None = None):
    """signorini_dolfinx.solve_contact_problem (:156-360): returns (it, iterations) [, final state, problem data].  A list given as
    `penetration_history` receives the penetration norm the reference prints before every proximal step (:318-321); it is evaluated
    only when printed (`verbose`) or collected."""
    if degree not in (1, 2):
        raise NotImplementedError("HIP backend: degrees 1 (BASELINE.json config 5) and 2 (the reference's default)")
    plane = isinstance(mesh, (fem.Mesh, fem.QuadMesh))  # gdim = 2 (:204): facets are edges, tagged as vertex pairs
    width = 2 if plane else (4 if isinstance(mesh, HexMesh) else 3)
    contact = _tagged(facet_tag, boundary_conditions["contact"], width)  # :186-189
    bc_facets = _tagged(facet_tag, boundary_conditions["displacement"], width)  # :265-266
    bc_vertices = np.unique(bc_facets.ravel())
    problem = SignoriniProblem(mesh, contact, bc_vertices if degree == 1 and not plane and not isinstance(mesh, HexMesh) else None, E, nu, gap, disp,
                               quadrature_degree, device=device, comm=comm, degree=degree, bc_facets=bc_facets)
    iterations = []
    normed_diff = -1.0
    it = 0
    for it in range(1, max_iterations + 1):
        if verbose or penetration_history is not None:
            penetration = problem.penetration()  # :312-314
            if penetration_history is not None:
                penetration_history.append(penetration)
            if verbose:
                print(f"{it=}/{max_iterations} {normed_diff:.2e} Penetration L2(Gamma):", f" {penetration:.2e}")  # :318-321
        alpha = alpha_0
        if alpha_scheme == "linear":
            alpha = alpha_0 + alpha_c * it
        elif alpha_scheme == "doubling":
            alpha = alpha_0 * 2**it
        problem.set_alpha(alpha)
        solver_tol = 10 * newton_tol if it < 2 else newton_tol  # :330
        problem.solver.setTolerances(atol=solver_tol, rtol=solver_tol)  # :331-332
        problem.solve()  # :333
        num_its = problem.solver.getIterationNumber()
        converged = problem.solver.getConvergedReason() > 0
        iterations.append(num_its)
        normed_diff = problem.u_increment()  # :336-339
        if normed_diff <= tol:
            if verbose:
                print(f"Converged at {it=} with increment norm {normed_diff:.2e}<{tol:.2e}")
            break
        problem.advance_prev()  # :342-343
        if not converged:
            break
    if output is not None:
        output = Path(output)
        output.mkdir(parents=True, exist_ok=True)
        np.savetxt(output / "lvpp_history.csv", np.asarray(iterations, dtype=np.int64), header="newton")
        from .io import write_vtu  # displacement for ParaView - the reference writes uh.bp with VTXWriter (:293-294)

        xs = problem.get_state()
        nv = problem.nv
        viol = problem.violation()  # the reference's `violation` Function next to u in uh.bp (:293-294, 349)
        u3 = np.stack([xs[k * nv:(k + 1) * nv] for k in range(problem.gdim)], axis=1)
        cell_name = None
        if isinstance(mesh, fem.QuadMesh):  # all Q_d nodes, first-order cells on the refined lattice (VTK corner order)
            co, _ = quad_lattice(mesh, degree)
            sub = fem.QuadMesh(mesh.box, (degree * mesh.structured[0], degree * mesh.structured[1]))
            cell_name = "quad"
            write_vtu(output / "uh.vtu", co, sub.cells[:, [0, 1, 3, 2]], {"displacement": u3, "violation": viol}, cell_type=cell_name)
            n1 = degree + 1
            corners = [0, degree, degree * n1 + degree, degree * n1]
        elif isinstance(mesh, fem.Mesh):
            nvert = mesh.geometry.shape[0]
            write_vtu(output / "uh.vtu", mesh.geometry, mesh.cells, {"displacement": u3[:nvert], "violation": viol[:nvert]})
            corners = [0, 1, 2]
        elif isinstance(mesh, HexMesh):  # all Q_d nodes as a point cloud of first-order cells on the refined lattice
            co, ce = mesh.lattice(degree)
            sub = HexMesh(degree * mesh.nx, degree * mesh.ny, degree * mesh.nz)
            write_vtu(output / "uh.vtu", co, sub.cells[:, [0, 1, 3, 2, 4, 5, 7, 6]], {"displacement": u3, "violation": viol},
                      cell_type="hexahedron")
            n1 = degree + 1
            corners = [0, degree, degree * n1 + degree, degree * n1]  # VTK corner order, bottom then top
            corners += [c + degree * n1 * n1 for c in corners]
        else:
            nvert = mesh.geometry.shape[0]  # degree 2: the vertex values (the edge nodes follow them in every component)
            write_vtu(output / "uh.vtu", mesh.geometry, mesh.cells, {"displacement": u3[:nvert], "violation": viol[:nvert]})
            corners = [0, 1, 2, 3]
        if not getattr(mesh, "curved", False):  # (von Mises needs affine cells: include/pgx_sg.h)
            # von_mises.bp of the reference (:296-299, 346-348): DG fields on a discontinuous mesh - points duplicated per cell, the
            # corner nodes of every cell as uh.vtu uses them
            cn = problem.cells[:, corners]
            nc, k = cn.shape
            write_vtu(output / "von_mises.vtu", problem.node_coords[cn.ravel()], np.arange(nc * k, dtype=np.int32).reshape(nc, k),
                      {"VonMises": problem.von_mises()[:, corners].ravel(), "u": u3[cn.ravel()]},
                      cell_type="hexahedron" if isinstance(mesh, HexMesh) else cell_name)
    if verbose:
        print(f"num_dofs_u={problem.gdim * problem.nv}, num_cells={mesh.cells.shape[0]}")
    if return_solution:
        x = problem.get_state()
        cv = problem.contact_vertices.copy()
        problem.close()
        return it, iterations, x, cv
    problem.close()
    return it, iterations


class NonlinearProblem:
    """dolfinx.fem.petsc.NonlinearProblem(F, [u, psi], bcs=bcs, petsc_options=..., entity_maps=entity_maps, kind="mpi") as
    signorini_dolfinx.py:283-291 builds it, for the blocked residual FORM of :244-252 stated in proximalgalerkin_amd.ufl (tensor
    algebra sym / tr / Identity, the `ds` measure over the contact tags, MixedFunctionSpace(V, W) with W on the contact
    sub-mesh).  The front end recognises the family, reads mu and lambda off the coefficients, the gap off g, the contact facets
    off the measure; `.solve()` / `.solver` behave like the reference's.  u, psi, psi_k are host Functions."""

    def __init__(self, F, u, bcs=None, petsc_options=None, petsc_options_prefix="", entity_maps=None, kind="mpi", device=0):
        from . import ufl

        spec = ufl.compile_signorini(F, u)
        V = spec.u.function_space
        mesh = V.mesh
        W = spec.psi.function_space
        if V.degree not in (1, 2) or V.dim != 3 or W.degree != V.degree:
            raise NotImplementedError("HIP backend, forms front end: equal degrees 1 or 2 for displacement and latent variable, in 3-D "
                                      "(signorini_dolfinx.py:221-222); plane problems run through the declarative driver "
                                      "proximalgalerkin_amd.signorini.solve_contact_problem on a fem.Mesh / fem.QuadMesh")
        if not bcs or len(bcs) != 1:
            raise NotImplementedError("one Dirichlet condition on the displacement surface (signorini_dolfinx.py:255-269)")
        bc = bcs[0]
        vals = np.asarray(bc.values)
        if vals.shape[0] != 3 or np.any(vals[:2] != 0.0) or np.any(vals[2] != vals[2, 0]):
            raise NotImplementedError("Dirichlet data (0, 0, disp) (signorini_dolfinx.py:257-262)")
        mu, lam = spec.mu, spec.lmbda
        E, nu = mu * (3.0 * lam + 2.0 * mu) / (lam + mu), lam / (2.0 * (lam + mu))
        self.spec = spec
        self._p = SignoriniProblem(mesh, spec.contact_facets, bc.dofs, E, nu, spec.gap, float(vals[2, 0]), spec.quadrature_degree,
                                   device=device, degree=V.degree)
        assert np.array_equal(self._p.contact_vertices, W.nodes())
        self.solver = self._p.solver
        self._nu3 = V.num_dofs

    def solve(self):
        p, sp = self._p, self.spec
        p.set_alpha(sp.alpha.value)
        p.set_state(np.concatenate([sp.u.x.array, sp.psi.x.array]))
        p.set_prev(np.concatenate([np.zeros(self._nu3), sp.psi_k.x.array]))  # only psi_k enters the residual (:246)
        p.solve()
        if p.solver.getConvergedReason() > 0:
            x = p.get_state()
            sp.u.x.array[:] = x[: self._nu3]
            sp.psi.x.array[:] = x[self._nu3:]

    def close(self):
        self._p.close()


def solve_contact_problem_forms(mesh: TetMesh, facet_tag: MeshTags, boundary_conditions: dict, E: float = 2.0e4, nu: float = 0.3,
                                gap: float = 0.0, disp: float = -0.25, newton_tol: float = 1e-6, max_iterations: int = 25,
                                alpha_0: float = 1.0, tol: float = 1e-6, quadrature_degree: int = 4, device: int = 0, degree: int = 1):
    """signorini_dolfinx.solve_contact_problem (:156-360) with the problem stated as the reference states it: spaces, sub-mesh,
    measures, the residual form, NonlinearProblem - through the UFL-subset front end.  alpha doubling.  Returns
    (it, iterations, u Function)."""
    from . import ufl

    if isinstance(mesh, (fem.Mesh, fem.QuadMesh)):
        raise NotImplementedError("HIP backend, forms front end: 3-D only; plane problems run through the declarative driver "
                                  "proximalgalerkin_amd.signorini.solve_contact_problem on a fem.Mesh / fem.QuadMesh")

    def epsilon(w):  # :146-147
        return ufl.sym(ufl.grad(w))

    def sigma(w, mu, lmbda):  # :150-153
        return 2.0 * mu * epsilon(w) + lmbda * ufl.tr(ufl.grad(w)) * ufl.Identity(gdim)

    contact_facets = np.concatenate([facet_tag.find(m) for m in boundary_conditions["contact"]])  # :199-202
    gdim, fdim = 3, 2
    submesh, submesh_to_mesh = fem.create_submesh(mesh, fdim, contact_facets)  # :207
    ds = ufl.Measure("ds", domain=mesh, subdomain_data=facet_tag, subdomain_id=boundary_conditions["contact"],
                     metadata={"quadrature_degree": quadrature_degree})  # :211-218
    V = fem.functionspace(mesh, ("Lagrange", degree, (gdim,)))  # :221
    W = fem.functionspace(submesh, ("Lagrange", degree))  # :222
    Q = ufl.MixedFunctionSpace(V, W)  # :225
    v, w = ufl.TestFunctions(Q)
    u, psi, psi_k = fem.Function(V, name="displacement"), fem.Function(W), fem.Function(W)
    mu = E / (2.0 * (1.0 + nu))
    lmbda = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    n_g = fem.Constant(mesh, np.zeros(gdim))
    n_g.value[-1] = -1
    alpha = fem.Constant(mesh, alpha_0)
    f = fem.Constant(mesh, np.zeros(gdim))
    x = ufl.SpatialCoordinate(mesh)
    g = x[gdim - 1] + fem.Constant(mesh, -gap)
    residual = alpha * ufl.inner(sigma(u, mu, lmbda), epsilon(v)) * ufl.dx(domain=mesh) - alpha * ufl.inner(f, v) * ufl.dx(domain=mesh)
    residual += -ufl.inner(psi - psi_k, ufl.dot(v, n_g)) * ds
    residual += ufl.inner(ufl.dot(u, n_g), w) * ds
    residual += ufl.inner(ufl.exp(psi), w) * ds - ufl.inner(g, w) * ds
    F = ufl.extract_blocks(residual)  # :252
    u_bc = fem.Function(V)

    def disp_func(xx):  # :257-260
        values = np.zeros((gdim, xx.shape[1]))
        values[gdim - 1, :] = disp
        return values

    u_bc.interpolate(disp_func)
    bc_facets = np.concatenate([facet_tag.find(d) for d in boundary_conditions["displacement"]])  # :265-266
    bc = fem.dirichletbc(u_bc, fem.locate_dofs_topological(V, fdim, bc_facets))  # :267
    solver = NonlinearProblem(F, [u, psi], bcs=[bc], petsc_options={"snes_type": "newtonls", "snes_linesearch_type": "none"},
                              petsc_options_prefix="signorini_", entity_maps=[submesh_to_mesh], kind="mpi", device=device)
    u_prev = np.zeros_like(u.x.array)
    iterations = []
    it = 0
    for it in range(1, max_iterations + 1):  # :317-358
        alpha.value = alpha_0 * 2**it
        solver_tol = 10 * newton_tol if it < 2 else newton_tol
        solver.solver.setTolerances(atol=solver_tol, rtol=solver_tol)
        solver.solve()
        iterations.append(solver.solver.getIterationNumber())
        normed_diff = float(np.linalg.norm(u.x.array - u_prev))  # :336-339
        if normed_diff <= tol:
            break
        u_prev[:] = u.x.array
        psi_k.x.array[:] = psi.x.array
        if solver.solver.getConvergedReason() <= 0:
            break
    solver.close()
    return it, iterations, u
