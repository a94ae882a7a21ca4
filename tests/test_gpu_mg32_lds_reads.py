"""The single-precision V-cycle bit for bit against the library before its LDS neighbour reads were unmerged.

csrc/pgx_mg32.hip reads the seven neighbours of an image vertex - row sweeps, residual rows of the fused epilogue, restriction gathers -
as single 8-byte LDS reads (F32_LDS_SINGLE, f_lds) where the compiler used to merge pairs of them.  A read returns the same value
either way and the source's arithmetic and its order are untouched - but the file is compiled with FMA contraction left to the
compiler, and which products it contracts can move with the form of the loads: with f_lds in the residual rows of k_f_resid_restrict
the twelve cases below without the fused restriction differed from the parent in the last bits (those rows keep the plain reads),
and same-row neighbours by DPP (tools/experiments/r12_lds_dpp_row.patch) changed all of them.  So bit-for-bit equality is a property
of the compiled library, and this test is what pins it.  Here one V-cycle is
applied through pgx_vcycle_apply to two seeded right-hand sides - a random one, and impulses on both sides of every tile seam and next
to the frame - under every launch form, entered on level 0 and on level 1, and the result is compared with goldens that were recorded
ONCE on an MI355X with the library of the commit before the change (tools/make_golden_lds_reads.py):
  golden/mg32_lds_reads_parent_n200x72.npz  the full outputs of the main form (K = 6, 20-row tiles, whole boundary tiles, fused
                                            restriction) on (200, 72): a difference is located, not only detected
  golden/mg32_lds_reads_parent_sha256.json  SHA-256 of the fp64 result of every case
Grids: (200, 72) and (130, 260), the smallest on which every kind of boundary tile exists (test_gpu_mg32_bnd_tiles.py, whose K6 keys
force the six-sweep launches onto them).  Keys the library does not report are set explicitly, as in test_gpu_vcycle_operator.py."""
import hashlib
import json
import pathlib

import numpy as np
import pytest

from tests.test_gpu_structured_kernels import _state

DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
OMEGA = 0.75
ALPHA = 2.5
EXPLICIT = {"PGX_NU_COARSE": 0, "PGX_COARSE_SWEEPS": 10, "PGX_TAIL_VERTS": 1100, "PGX_MG_MIN_NX": 4}
K6 = {"PGX_F32_K6_MAX": 2 ** 30, "PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500, "PGX_F32_BND_FULL_MIN": 0}
GRIDS = [(200, 72), (130, 260)]
NORR = {"PGX_F32_RR_MAX": 0}
# name -> (tuning keys, nu).  K = 6 with whole boundary tiles and with four-row sub-tiles, restriction fused and on its own, tiles of
# 8 and 20 rows; K = 3 (two launches per leg); K = 2 (nu = 4); the float4 form of D
FORMS = {
    "K6-ty20-full-rr": (dict(K6, PGX_F32_TY=20), 6),
    "K6-ty20-sub-rr": (dict(K6, PGX_F32_TY=20, PGX_F32_BND_FULL=0), 6),
    "K6-ty20-full-norr": (dict(K6, PGX_F32_TY=20, **NORR), 6),
    "K6-ty20-sub-norr": (dict(K6, PGX_F32_TY=20, PGX_F32_BND_FULL=0, **NORR), 6),
    "K6-ty8-full-rr": (dict(K6, PGX_F32_TY=8), 6),
    "K6-ty8-sub-rr": (dict(K6, PGX_F32_TY=8, PGX_F32_BND_FULL=0), 6),
    "K6-ty8-full-norr": (dict(K6, PGX_F32_TY=8, **NORR), 6),
    "K3-rr": (dict(K6, PGX_F32_K6_MAX=0), 6),
    "K3-norr": (dict(K6, PGX_F32_K6_MAX=0, **NORR), 6),
    "K2-nu4-rr": (dict(K6), 4),
    "K2-nu4-norr": (dict(K6, **NORR), 4),
    "K6-ty20-float4-rr": (dict(K6, PGX_F32_TY=20, PGX_F32_DBF16=0), 6),
    "K6-ty20-float4-norr": (dict(K6, PGX_F32_TY=20, PGX_F32_DBF16=0, **NORR), 6),
}
MAIN = "K6-ty20-full-rr"  # its outputs on GRIDS[0] are stored in full
LEVELS = (0, 1)
GOLDEN = pathlib.Path(__file__).parent / "golden"
FULL, SHA = GOLDEN / "mg32_lds_reads_parent_n200x72.npz", GOLDEN / "mg32_lds_reads_parent_sha256.json"
TILE_COLUMNS, TILE_ROWS = (52, 58, 60), (4, 8, 16, 20)  # tile widths at six, three and two sweeps per launch; the PGX_F32_TY heights
_rhs_cache, _golden = {}, {}


def rhs(nx, ny, coarse):
    """name -> [u | psi] on the (nx, ny) grid, shared and read-only.  Below the finest level the u part is 0 on the frame (what every
    restriction delivers; pgx_vcycle_apply refuses anything else) and the values are floats, which is how the hook hands them over."""
    if (nx, ny, coarse) in _rhs_cache:
        return _rhs_cache[(nx, ny, coarse)]
    sx, n = nx + 1, (nx + 1) * (ny + 1)
    rng = np.random.default_rng(7000 * nx + ny)
    v = []
    for w in TILE_COLUMNS:  # both sides of every seam column, on every third row
        for k, c in enumerate(range(w, nx, w)):
            v += [j * sx + c + d for j in range(1 + k % 3, ny, 3) for d in (-1, 0)]
    for t in TILE_ROWS:
        for k, r in enumerate(range(t, ny, t)):
            v += [(r + d) * sx + i for i in range(1 + k % 3, nx, 3) for d in (-1, 0)]
    v += [j * sx + i for j in range(1, ny) for i in range(1, nx) if i in (1, nx - 1) or j in (1, ny - 1)]  # next to the frame
    v = np.unique(np.asarray(v, dtype=np.int64))
    imp = np.zeros(2 * n)
    imp[v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
    imp[n + v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
    out = {"random": rng.standard_normal(2 * n), "impulses": imp}
    for name, b in out.items():
        if coarse:
            j, i = np.divmod(np.arange(n), sx)
            b[:n][(i == 0) | (i == nx) | (j == 0) | (j == ny)] = 0.0
            b[:] = b.astype(np.float32)
        b.setflags(write=False)
    _rhs_cache[(nx, ny, coarse)] = out
    return out


def run_case(cells, form):
    """{(level, right-hand side name): z} of one handle: one Jacobian (the state of test_gpu_vcycle_operator.py), one cycle per entry."""
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import setup_problem

    keys, nu = FORMS[form]
    keys = dict(EXPLICIT, **keys)
    nx, ny = cells
    for k, v in keys.items():
        _lib.tuning_set(k, v)
    problem = None
    try:
        problem, sol, sol_k, a = setup_problem(fem.create_rectangle(DOMAIN, cells))
        n2 = sol.function_space.num_dofs
        x, xk = _state(n2, 11)
        x[n2 // 2:].reshape(ny + 1, nx + 1)[ny // 3: ny // 3 + 6, nx // 3: nx // 3 + 7] -= 800.0  # exp(psi) underflows: exact zeros in D
        sol_k.x.array[:] = xk
        a.value = ALPHA
        problem.assemble_jacobian(x)
        out = {}
        for level in LEVELS:
            info = problem.mg_level_export(level)
            # (130, 260) coarsens once (65 is odd): its level 1 is the coarsest level, in fp64 - level 0 then hands its right-hand side
            # down and takes its correction back in fp64 (the CB64 and CADD = 2 forms of the launches)
            assert bool(info["f32"]) == (level == 0 or cells == GRIDS[0]), (cells, form, level)
            assert not info["f32"] or bool(info["dbf16"]) == bool(keys.get("PGX_F32_DBF16", 1)), (cells, form, level)
            for name, b in rhs(info["nx"], info["ny"], level > 0).items():
                z = problem.vcycle_apply(level, b, nu=nu, omega=OMEGA)
                assert np.isfinite(z).all() and np.abs(z).max() > 0.0
                out[(level, name)] = z
        return out
    finally:
        if problem is not None:
            problem.close()
        for k in keys:
            _lib.tuning_set(k, None)


def case_id(cells, form, level, name):
    return f"{cells[0]}x{cells[1]}/{form}/level{level}/{name}"


def digest(z):
    return hashlib.sha256(np.ascontiguousarray(z, dtype="<f8").tobytes()).hexdigest()


def _goldens():
    if not _golden:
        _golden["sha"] = json.loads(SHA.read_text())["sha256"]
        _golden["full"] = dict(np.load(FULL))
    return _golden


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cells", GRIDS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_vcycle_is_bitwise_the_parent_library(require_gpu, cells, form):
    g = _goldens()
    got = run_case(cells, form)
    assert len(got) == 2 * len(LEVELS)
    for (level, name), z in got.items():
        cid = case_id(cells, form, level, name)
        if cells == GRIDS[0] and form == MAIN:
            want = g["full"][f"level{level}_{name}"].astype(np.float64)
            d = np.abs(z - want)
            print(f"{cid}: max |z - z_parent| = {d.max():.3e} at entry {int(d.argmax())} of {len(z)} (max |z| {np.abs(want).max():.3e}), "
                  f"{int((z != want).sum())} entries differ")
            assert np.array_equal(z, want), cid
        print(f"{cid}: sha256 {digest(z)[:16]} parent {g['sha'][cid][:16]}")
        assert digest(z) == g["sha"][cid], cid


def test_goldens_cover_every_case():
    """(no GPU) one digest per grid, form, level and right-hand side, and the full outputs of the main form"""
    g = _goldens()
    want = {case_id(c, f, l, n) for c in GRIDS for f in FORMS for l in LEVELS for n in ("random", "impulses")}
    assert set(g["sha"]) == want
    assert set(g["full"]) == {f"level{l}_{n}" for l in LEVELS for n in ("random", "impulses")}
    for l in LEVELS:
        for n in ("random", "impulses"):
            assert digest(g["full"][f"level{l}_{n}"].astype(np.float64)) == g["sha"][case_id(GRIDS[0], MAIN, l, n)]
