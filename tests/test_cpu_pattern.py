"""The host pattern builders of the mixed-matrix families (proximalgalerkin_amd/csrc/pgx_pattern.h) without a GPU: a stand-alone
driver (tests/csrc/pattern_check.cpp, g++ only) is fed small meshes and its rowptr / col / sptr / scol / kind are compared with a
numpy restatement - the boolean union of the per-entity dof outer products, rows ascending."""
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pattern") / "pattern_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "csrc" / "pattern_check.cpp")],
                   check=True)
    return exe


def _run(driver, tmp_path, text):
    f = tmp_path / "request.txt"
    f.write_text(text)
    out = subprocess.run([str(driver), str(f)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        name, _, rest = line.partition(" ")
        res[name] = rest if name == "error" else np.array(rest.split(), dtype=np.int64)
    return res


def _triangles(nx, ny):
    """vertex-major (ny + 1) x (nx + 1) lattice, two triangles per square (right diagonal)"""
    v = lambda i, j: j * (nx + 1) + i  # noqa: E731
    cells = []
    for j in range(ny):
        for i in range(nx):
            cells += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
    return (nx + 1) * (ny + 1), np.array(cells, dtype=np.int64)


def _union_pattern(n, entities):
    """rowptr, col of the boolean union of the outer products of the entities' dof lists, rows ascending"""
    A = np.zeros((n, n), dtype=bool)
    for d in entities:
        A[np.ix_(d, d)] = True
    rows = [np.flatnonzero(A[r]) for r in range(n)]
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]), (np.concatenate(rows) if n else np.zeros(0, np.int64))


def _kinds(nu, mask, rowptr, col):
    kind = np.empty(len(col), dtype=np.int64)
    for r in range(len(rowptr) - 1):
        for k in range(rowptr[r], rowptr[r + 1]):
            c = col[k]
            if r < nu and c < nu:
                kind[k] = (3 if (r == c and mask[r]) else 4) if (mask[r] or mask[c]) else 0
            elif r < nu:
                kind[k] = 4 if mask[r] else 1
            elif c < nu:
                kind[k] = 4 if mask[c] else 1
            else:
                kind[k] = 2
    return kind


def _entities_request(ntot, nu, entities, mask):
    lines = [f"entities {ntot} {nu} {len(entities)}"]
    lines += [" ".join(map(str, [len(d), *d])) for d in entities]
    lines.append(" ".join(str(int(b)) for b in mask))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("keep", [1, 0])
def test_p1_adjacency_with_an_isolated_vertex(driver, tmp_path, keep):
    nv, cells = _triangles(5, 4)  # nx != ny: a transposed lattice would show
    iso = nv  # one extra vertex that no cell touches
    res = _run(driver, tmp_path, f"p1 {nv + 1} {len(cells)} {keep}\n" + " ".join(map(str, cells.ravel())) + "\n")
    sptr, scol = _union_pattern(nv + 1, list(cells) + ([[iso]] if keep else []))
    assert np.array_equal(res["sptr"], sptr) and np.array_equal(res["scol"], scol)
    assert res["sptr"][iso + 1] - res["sptr"][iso] == (1 if keep else 0)
    for v in range(nv):  # every vertex of a cell has its diagonal either way
        assert v in res["scol"][res["sptr"][v]:res["sptr"][v + 1]]


def test_builders_on_their_threaded_path(driver, tmp_path):
    """more than 20000 rows: the builders split the rows over host threads; the result is the same union, here through scipy"""
    import scipy.sparse as sp

    nv, cells = _triangles(160, 130)  # 21091 vertices
    assert nv > 20000

    def union(n, ents):
        e = np.asarray(ents)
        k = e.shape[1]
        A = sp.coo_matrix((np.ones(e.shape[0] * k * k, dtype=np.int8), (np.repeat(e, k, axis=1).ravel(), np.tile(e, (1, k)).ravel())),
                          shape=(n, n)).tocsr()
        A.sum_duplicates()
        A.sort_indices()
        return A.indptr, A.indices

    res = _run(driver, tmp_path, f"p1 {nv} {len(cells)} 0\n" + " ".join(map(str, cells.ravel())) + "\n")
    sptr, scol = union(nv, cells)
    assert np.array_equal(res["sptr"], sptr) and np.array_equal(res["scol"], scol)
    nu = 2 * nv
    ents = np.concatenate([cells, nv + cells], axis=1)  # (u_x, u_y) of a cell's vertices, all of them primal rows
    mask = np.zeros(nu, dtype=bool)
    mask[:161] = True
    res = _run(driver, tmp_path, _entities_request(nu, nu, ents.tolist(), mask))
    rowptr, col = union(nu, ents)
    assert np.array_equal(res["rowptr"], rowptr) and np.array_equal(res["col"], col) and res["find"][0] == 1
    r = np.repeat(np.arange(nu), np.diff(rowptr))
    dirichlet = mask[r] | mask[col]
    assert np.array_equal(res["kind"], np.where(dirichlet, np.where((r == col) & mask[r], 3, 4), 0))


def test_out_of_range_cell_vertex_is_refused(driver, tmp_path):
    nv, cells = _triangles(2, 1)
    for bad in (nv, -1):
        c = cells.copy()
        c[1, 2] = bad
        res = _run(driver, tmp_path, f"p1 {nv} {len(c)} 1\n" + " ".join(map(str, c.ravel())) + "\n")
        assert res == {"error": "cell vertex out of range"}


def test_three_field_pattern_from_cells(driver, tmp_path):
    """the numbering of pgx_gc on a 3 x 2 rectangle: 6 P2 dofs of u (vertices, then edges), 3 + 3 P1 dofs of (psi_x, psi_y)"""
    nv, cells = _triangles(3, 2)
    edges = sorted({tuple(sorted((c[a], c[b]))) for c in cells for a, b in ((1, 2), (0, 2), (0, 1))})
    eid = {e: nv + k for k, e in enumerate(edges)}
    n2 = nv + len(edges)
    ntot = n2 + 2 * nv
    ents = []
    for c in cells:
        u = list(c) + [eid[tuple(sorted((c[a], c[b])))] for a, b in ((1, 2), (0, 2), (0, 1))]
        ents.append(u + [n2 + v for v in c] + [n2 + nv + v for v in c])
    assert all(len(d) == 12 for d in ents)
    mask = np.zeros(n2, dtype=bool)
    mask[[0, 3, eid[edges[0]]]] = True
    res = _run(driver, tmp_path, _entities_request(ntot, n2, ents, mask))
    rowptr, col = _union_pattern(ntot, ents)
    assert np.array_equal(res["rowptr"], rowptr) and np.array_equal(res["col"], col)
    assert np.array_equal(res["kind"], _kinds(n2, mask, rowptr, col)) and set(res["kind"]) == {0, 1, 2, 3, 4}
    assert res["find"][0] == 1


def test_cells_and_facets_as_one_entity_range(driver, tmp_path):
    """the numbering of pgx_sg_create_2d: cells carry (u_x, u_y) of their vertices, two contact edges carry u_y and psi of theirs"""
    nv, cells = _triangles(3, 2)
    nu = 2 * nv
    facets = [[0, 1], [1, 2]]  # two edges of the bottom side
    cverts = sorted({v for f in facets for v in f})
    psi = {v: nu + k for k, v in enumerate(cverts)}
    ntot = nu + len(cverts)
    ents = [[i * nv + v for v in c for i in range(2)] for c in cells]
    ents += [[nv + v for v in f] + [psi[v] for v in f] for f in facets]
    mask = np.zeros(nu, dtype=bool)
    top = [v for v in range(nv) if v // 4 == 2]
    mask[top] = True  # u_x and u_y on the top side
    mask[[nv + v for v in top]] = True
    res = _run(driver, tmp_path, _entities_request(ntot, nu, ents, mask))
    rowptr, col = _union_pattern(ntot, ents)
    assert np.array_equal(res["rowptr"], rowptr) and np.array_equal(res["col"], col)
    assert np.array_equal(res["kind"], _kinds(nu, mask, rowptr, col)) and set(res["kind"]) == {0, 1, 2, 3, 4}
    assert res["find"][0] == 1
    # a psi row couples to the u_y and psi dofs of its edges only
    r = psi[0]
    assert list(res["col"][res["rowptr"][r]:res["rowptr"][r + 1]]) == [nv + 0, nv + 1, psi[0], psi[1]]
