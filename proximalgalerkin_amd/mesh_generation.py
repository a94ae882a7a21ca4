"""Native stand-ins for the reference's gmsh-based mesh generators (`src/lvpp/mesh_generation.py`: `create_half_disk` :11-83,
`create_half_sphere` :86-168; driven by `examples/02_signorini/generate_mesh.py:12`).  gmsh is not available offline, so the same
GEOMETRIES - same centre, radius and surface markers, same return shape `(mesh, cell_tags, facet_tags)` - are meshed by mapping a
structured simplicial grid of the (half) cube onto the (half) ball: `p -> c + r p |p|_inf / |p|_2` sends the cube's faces to the
sphere and keeps the plane z = 0 (y = 0 in 2-D) flat.  The meshes are conforming, shape-regular away from the images of the cube's
edges, and linear (order 1): the reference's default order 2 is a curved-geometry refinement this package reduces to its vertices on
input anyway (`io.py`).  `res` is the edge length on the surface near the pole, as in the reference; the grading towards the pole
(gmsh Threshold field, lc from `res` to `2 res`) is not reproduced - the grid is quasi-uniform at `res`.
"""
from __future__ import annotations

import numpy as np

from . import fem
from .signorini import MeshTags, TetMesh

__all__ = ["create_half_disk", "create_half_sphere", "create_crack_mesh", "CRACK_BOUNDARIES", "create_mobius_strip", "MobiusMesh"]


class MobiusMesh:
    """nu x nv quadrilaterals of geometry order `order` embedded in R^3, the last column of cells glued to the first one upside down.
    `cell_nodes` (nc, (order+1)^2, 3): the geometry nodes of cell cy nu + cx, local node b (order+1) + a, each cell sampled at its own
    unwrapped parameters.  The dof numberings on it come from `lagrange.numbering_mobius`."""

    def __init__(self, nu, nv, order, scale, cell_nodes):
        self.nu, self.nv, self.order, self.scale = int(nu), int(nv), int(order), float(scale)
        self.cell_nodes = np.ascontiguousarray(cell_nodes, dtype=np.float64)
        self.num_cells = self.nu * self.nv

    def cell_name(self):
        return "quadrilateral"


def mobius_map(s, t, scale=1.0):
    """x(s, t) = scale ((1 + rho cos(s / 2)) cos s, (1 + rho cos(s / 2)) sin s, rho sin(s / 2)), rho = (t - 1/2) / 2: the strip of
    half-width scale / 4 around the circle of radius scale, s in [0, 2 pi], t in [0, 1]; (s + 2 pi, t) and (s, 1 - t) are one point."""
    rho = 0.5 * (np.asarray(t, dtype=np.float64) - 0.5)
    a = 1.0 + rho * np.cos(0.5 * s)
    return scale * np.stack([a * np.cos(s), a * np.sin(s), rho * np.sin(0.5 * s)], axis=-1)


def create_mobius_strip(nu: int, nv: int, order: int = 3, scale: float = 1.0) -> MobiusMesh:
    """The Moebius strip of example 09 meshed natively: the parameter cells [2 pi cx / nu, 2 pi (cx + 1) / nu] x [cy / nv, (cy + 1) / nv]
    mapped by `mobius_map`, every cell's (order+1)^2 equispaced geometry nodes sampled at its own unwrapped parameters (the nodes two
    cells share across the seam are one point of R^3 reached through two parameter pairs).  The reference reads a mesh written by MFEM
    (examples/09_eikonal/eikonal_dolfinx.py:27); this parametrisation is the package's own."""
    nu, nv, order = int(nu), int(nv), int(order)
    if nu < 3 or nv < 1:
        raise ValueError("create_mobius_strip: nu >= 3 (no cell may meet itself or one neighbour twice) and nv >= 1")
    if order not in (1, 2, 3):
        raise ValueError("create_mobius_strip: geometry order 1, 2 or 3")
    if not (scale > 0.0) or not np.isfinite(scale):
        raise ValueError("create_mobius_strip: scale must be positive")
    cx, cy = np.tile(np.arange(nu), nv), np.repeat(np.arange(nv), nu)
    lat = np.arange(order + 1) / order
    S = 2.0 * np.pi * (cx[:, None] + np.tile(lat, order + 1)[None, :]) / nu
    T = (cy[:, None] + np.repeat(lat, order + 1)[None, :]) / nv
    return MobiusMesh(nu, nv, order, scale, mobius_map(S, T, float(scale)))


def _ball_map(p):
    """cube [-1,1]^d -> unit ball, radial: p |p|_inf / |p|_2 (0 -> 0)"""
    n2 = np.linalg.norm(p, axis=1)
    ninf = np.abs(p).max(axis=1)
    s = np.divide(ninf, n2, out=np.zeros_like(n2), where=n2 > 0)
    return p * s[:, None]


def _untangle(coords, cells, edges, curved, ratio=0.2):
    """Mid-edge nodes of a valid order-2 tetrahedral mesh: `curved` where the quadratic cell maps allow it.  Where the cube's faces meet,
    the map to the ball opens a 90 degree dihedral angle to 180 degrees: a tetrahedron with two faces on the surface keeps a positive
    volume, but its QUADRATIC map can fold once the surface edges bulge outward (33 of 648 cells at res = 0.15).  gmsh untangles such
    cells by optimisation; here the offset of every edge of an offending cell is halved until det J, sampled at the vertices, the edge
    midpoints and the degree-5 quadrature points, stays within `ratio` of its maximum over the cell (the mesh stays conforming: an
    edge has ONE node)."""
    from . import fem
    from .signorini import _TET_EDGES

    nv = len(coords)
    key = edges[:, 0] * nv + edges[:, 1]
    c = cells.astype(np.int64)
    ce = np.stack([np.searchsorted(key, np.minimum(c[:, a], c[:, b]) * nv + np.maximum(c[:, a], c[:, b])) for a, b in _TET_EDGES], axis=1)
    pts = np.concatenate([fem.quadrature_rule("tetrahedron", 5)[0], np.eye(4)[:, 1:], 0.5 * (np.eye(4)[[a for a, _ in _TET_EDGES]] + np.eye(4)[[b for _, b in _TET_EDGES]])[:, 1:]])
    L = np.concatenate([1.0 - pts.sum(axis=1, keepdims=True), pts], axis=1)
    gref = np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    dN = np.empty((len(L), 10, 3))
    for a in range(4):
        dN[:, a] = (4 * L[:, a] - 1)[:, None] * gref[a][None]
    for k, (a, b) in enumerate(_TET_EDGES):
        dN[:, 4 + k] = 4 * (L[:, a][:, None] * gref[b][None] + L[:, b][:, None] * gref[a][None])
    straight = 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])
    x = coords[cells]
    sgn = np.sign(np.linalg.det(np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]], axis=2)))
    theta = np.ones(len(edges))
    for _ in range(12):
        mid = straight + theta[:, None] * (curved - straight)
        X10 = np.concatenate([x, mid[ce]], axis=1)
        det = np.linalg.det(np.einsum("cad,qak->cqdk", X10, dN)) * sgn[:, None]
        bad = det.min(axis=1) < ratio * det.max(axis=1)
        if not bad.any():
            break
        theta[np.unique(ce[bad])] *= 0.5
    else:
        theta[np.unique(ce[bad])] = 0.0
    return straight + theta[:, None] * (curved - straight)


def create_half_sphere(model_name=None, order: int = 2, center=(0.0, 0.0, 0.5), res: float = 0.02, r: float = 0.4, comm=None, rank: int = 0,
                       sphere_surface: int = 2, flat_surface: int = 1):
    """Half ball of radius `r` below the plane z = center[2] (the reference's geometry, `mesh_generation.py:86-168`): tetrahedra,
    curved surface tagged `sphere_surface` (the potential contact surface of example 02), flat top tagged `flat_surface` (where the
    displacement is prescribed).  Returns (TetMesh, None, MeshTags): the reference's (mesh, cell_tags, facet_tags); the cell tags
    (one physical volume) carry no information and are not modelled.  order = 2 (the reference's default, :88): the mid-edge nodes
    of the 10-node tetrahedra are the images of the grid's edge midpoints under the same map (`mesh.midside`; on the curved surface they
    lie ON the sphere) - isoparametric P2 in example 02 since round 5; order = 1: vertices only."""
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    n = max(2, 2 * int(np.ceil(np.pi * r / (4.0 * res))))  # a quarter circle of the surface spans n/2 cells of length ~res; even
    nz = n // 2
    xs = np.linspace(-1.0, 1.0, n + 1)
    zs = np.linspace(-1.0, 0.0, nz + 1)
    Z, Y, X = np.meshgrid(zs, xs, xs, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(n), np.arange(n), indexing="ij")
    v0 = (iz * (n + 1) * (n + 1) + iy * (n + 1) + ix).ravel()
    v1, v2 = v0 + 1, v0 + (n + 1)
    v3 = v1 + (n + 1)
    off = (n + 1) * (n + 1)
    v4, v5, v6, v7 = v0 + off, v1 + off, v2 + off, v3 + off
    tets = [(v0, v1, v3, v7), (v0, v1, v7, v5), (v0, v5, v7, v4), (v0, v3, v2, v7), (v0, v6, v4, v7), (v0, v2, v6, v7)]
    cells = np.ascontiguousarray(np.stack([np.stack(t, axis=1) for t in tets], axis=1).reshape(-1, 4), dtype=np.int32)
    coords = np.ascontiguousarray(np.asarray(center, dtype=float)[None, :] + r * _ball_map(P))
    mesh = TetMesh(coords, cells)
    if order == 2:
        e = mesh.edges()
        curved = np.asarray(center, dtype=float)[None, :] + r * _ball_map(0.5 * (P[e[:, 0]] + P[e[:, 1]]))
        mesh = TetMesh(coords, cells, _untangle(coords, cells, e, curved))
    # exterior facets: flat <=> all three vertices come from the plane z = 0 of the cube (mapped to z = center[2] exactly)
    on_top = np.isclose(P[:, 2], 0.0)
    ext = mesh.facets_where(lambda x: np.ones(x.shape[1], dtype=bool))
    flat = on_top[ext].all(axis=1)
    return mesh, None, MeshTags({flat_surface: ext[flat], sphere_surface: ext[~flat]})


def create_half_disk(c_y: float, R: float, res: float, order: int = 1, refinement_level: int = 1, disk_marker: int = 2, top_marker: int = 1):
    """Half disk of radius `R` below the line y = c_y (`mesh_generation.py:11-83`): triangles; curved boundary tagged
    `disk_marker`, flat top `top_marker`.  Returns (fem.Mesh, None, {marker: boundary edges as vertex pairs})."""
    n = max(2, 2 * int(np.ceil(np.pi * R / (4.0 * res)))) * max(1, int(refinement_level))
    ny = n // 2
    xs = np.linspace(-1.0, 1.0, n + 1)
    ys = np.linspace(-1.0, 0.0, ny + 1)
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel()], axis=1)
    jy, ix = np.meshgrid(np.arange(ny), np.arange(n), indexing="ij")
    a = (jy * (n + 1) + ix).ravel()
    b, c = a + 1, a + (n + 1)
    d = c + 1
    cells = np.ascontiguousarray(np.stack([np.stack([a, b, d], axis=1), np.stack([a, d, c], axis=1)], axis=1).reshape(-1, 3), dtype=np.int32)
    coords = np.ascontiguousarray(np.array([0.0, float(c_y)])[None, :] + R * _ball_map(P))
    mesh = fem.Mesh(coords, cells)
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    key = np.sort(e, axis=1)
    _, idx, cnt = np.unique(key, axis=0, return_index=True, return_counts=True)
    ext = e[np.sort(idx[cnt == 1])]
    top = np.isclose(P[:, 1], 0.0)[ext].all(axis=1)
    return mesh, None, {int(top_marker): ext[top].astype(np.int32), int(disk_marker): ext[~top].astype(np.int32)}


# examples/03_fracture/generate_mesh.py:15-37: the polygon's segments in order, then the circle; tag = position + 1
CRACK_BOUNDARIES = ("bottom", "right", "topright", "crackright", "crackleft", "topleft", "left", "hole")
_CRACK_POLYGON = ((0.0, 0.0), (2.0, 0.0), (2.0, 2.0), (1.01, 2.0), (1.0, 1.5), (0.99, 2.0), (0.0, 2.0))
_CRACK_HOLE = ((0.3, 0.3), 0.2)


def _in_polygon(P, poly):
    """even-odd rule, vectorised over the points P (n, 2)"""
    x, y = P[:, 0], P[:, 1]
    inside = np.zeros(len(P), dtype=bool)
    for (x0, y0), (x1, y1) in zip(poly, np.roll(poly, -1, axis=0)):
        cross = (y0 > y) != (y1 > y)
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = x0 + (y - y0) * (x1 - x0) / (y1 - y0)
        inside ^= cross & (x < xi)
    return inside


def _segment_distance(P, a, b):
    ab = b - a
    t = np.clip(((P - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(P - (a + t[:, None] * ab), axis=1)


def create_crack_mesh(max_res: float = 0.05):
    """The notched plate with a hole of example 03 (`examples/03_fracture/generate_mesh.py:15-37`): the polygon (0,0), (2,0), (2,2),
    (1.01,2), (1,1.5), (0.99,2), (0,2) minus the disk of centre (0.3,0.3) and radius 0.2, with the reference's boundary names.
    Returns (fem.Mesh, (edges (ne,2) int32, tags (ne,) int32), {name: tag}).

    netgen is not available offline, so the geometry is meshed natively: boundary points at spacing <= h = max_res on every
    polygon segment, m = max(8, ceil(2 pi r / h)) points on the circle, a staggered lattice (spacing h, rows h sqrt(3)/2 apart)
    of the points inside the domain and farther than 0.6 h from every boundary, then scipy's Delaunay triangulation, of which the
    triangles with their centroid inside the domain are kept (counter-clockwise).  The clearance keeps the diametral circle of
    every boundary piece free of lattice points, and the two sides of the notch carry their points at equal heights, so the
    boundary is recovered without constraints; the function checks that, and raises otherwise:
    every boundary piece is a mesh edge, the cell areas sum to 4 - 0.005 - (m/2) r^2 sin(2 pi / m), and the exterior edges are
    exactly the tagged ones.  This is NOT netgen's mesh: iterate-for-iterate parity of example 03 with FEniCSx stays unpinned, as
    for every other example."""
    from scipy.spatial import Delaunay

    h = float(max_res)
    if not (h > 0.0) or not np.isfinite(h):
        raise ValueError("max_res must be positive")
    poly = np.array(_CRACK_POLYGON)
    (cx, cy), r = _CRACK_HOLE
    pts, pieces, tags = [], [], []  # boundary points; pieces = index pairs into pts
    first = 0
    for k, (a, b) in enumerate(zip(poly, np.roll(poly, -1, axis=0))):
        n = max(1, int(np.ceil(np.linalg.norm(b - a) / h - 1e-12)))
        start = len(pts)
        for i in range(n):
            pts.append(a + (b - a) * (i / n))
        for i in range(n):
            nxt = start + i + 1
            pieces.append((start + i, nxt if (k < len(poly) - 1 or i < n - 1) else first))
            tags.append(k + 1)
    m = max(8, int(np.ceil(2.0 * np.pi * r / h)))
    start = len(pts)
    th = 2.0 * np.pi * np.arange(m) / m
    circle = np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], axis=1)
    pts.extend(circle)
    for i in range(m):
        pieces.append((start + i, start + (i + 1) % m))
        tags.append(len(poly) + 1)
    B = np.array(pts)
    pieces = np.array(pieces, dtype=np.int64)
    dy = h * np.sqrt(3.0) / 2.0
    rows = np.arange(0, int(np.floor(2.0 / dy)) + 1)
    L = np.concatenate([np.stack([np.arange(0, int(np.floor(2.0 / h)) + 2) * h - (0.5 * h if j % 2 else 0.0),
                                  np.full(int(np.floor(2.0 / h)) + 2, j * dy)], axis=1) for j in rows])
    keep = _in_polygon(L, poly) & (np.hypot(L[:, 0] - cx, L[:, 1] - cy) > r + 0.6 * h)
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        keep &= _segment_distance(L, a, b) > 0.6 * h
    P = np.concatenate([B, L[keep]])
    tri = Delaunay(P).simplices.astype(np.int64)
    x = P[tri]
    cen = x.mean(axis=1)
    det = (x[:, 1, 0] - x[:, 0, 0]) * (x[:, 2, 1] - x[:, 0, 1]) - (x[:, 2, 0] - x[:, 0, 0]) * (x[:, 1, 1] - x[:, 0, 1])
    ok = _in_polygon(cen, poly) & ~_in_polygon(cen, circle) & (np.abs(det) > 1e-10 * h * h)
    tri, det = tri[ok], det[ok]
    tri[det < 0] = tri[det < 0][:, [0, 2, 1]]
    used = np.unique(tri)
    if len(used) < len(B) or not np.array_equal(used[:len(B)], np.arange(len(B))):
        raise RuntimeError("create_crack_mesh: a boundary point belongs to no cell")
    new = np.full(len(P), -1, dtype=np.int64)
    new[used] = np.arange(len(used))
    cells = new[tri]
    coords = P[used]
    mesh = fem.Mesh(coords, cells.astype(np.int32))
    nv = len(coords)
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    e.sort(axis=1)
    uk, cnt = np.unique(e[:, 0] * nv + e[:, 1], return_counts=True)
    bkey = np.sort(pieces, axis=1)
    bkey = bkey[:, 0] * nv + bkey[:, 1]
    if not np.all(np.isin(bkey, uk)):
        raise RuntimeError(f"create_crack_mesh({h}): the triangulation does not recover the boundary")
    if not np.array_equal(np.sort(bkey), uk[cnt == 1]):
        raise RuntimeError(f"create_crack_mesh({h}): the exterior edges are not the tagged boundary pieces")
    area = 0.5 * np.abs(det).sum()
    exact = 4.0 - 0.005 - 0.5 * m * r * r * np.sin(2.0 * np.pi / m)
    if abs(area - exact) > 1e-12 * exact:
        raise RuntimeError(f"create_crack_mesh({h}): cell areas sum to {area!r}, the domain has {exact!r}")
    names = {name: k + 1 for k, name in enumerate(CRACK_BOUNDARIES)}
    return mesh, (np.ascontiguousarray(pieces, dtype=np.int32), np.array(tags, dtype=np.int32)), names
