"""The P1 multigrid V-cycle as an OPERATOR, level by level and launch form by launch form, against tests/vcycle_reference.py.

No solves: a case creates a handle under one set of tuning keys, fills ONE Jacobian, reads the stored level operators
(pgx_mg_level_export) or applies one cycle entered on one level (pgx_vcycle_apply) and compares with the numpy cycle built from the
exported blocks (K, M, D, alpha, the frame as Dirichlet set).  FGMRES is flexible and its residual is fp64, so a cycle that is subtly
wrong - a link dropped at a tile seam, a frame-adjacent row with the interior formula, a coarse correction one column off - still
delivers the Newton counts and the u the solve tests assert; here it changes z at the vertices it touches, and every comparison is
per vertex in the MAXIMUM norm, relative to max |z_ref|, separately on the u half and the psi half.

State: `_state` of test_gpu_structured_kernels.py (psi mostly negative, exp(psi) over several orders of magnitude) with a 6 x 7 patch
inside the grid pushed down by 800, where exp(psi) underflows to exact zeros; alpha in {2.5, 100}.

Right-hand sides of every case (on the level entered): a random vector; unit impulses at the four corners; impulses on both sides of
every tile seam in x (tiles of 52 columns at six sweeps per launch, 58 at three, 60 at two and in the residual + restriction kernel,
32 in the tile-mapped fp64 kernels, inside images of 64 columns) and in y (4, 8, 12, 16, 20 rows: the PGX_F32_TY values); impulses at
the vertices next to the frame.  Below the finest level the u part is zeroed on the frame: a coarse right-hand side is a restricted
residual, every restriction masks those rows, the fused tail relies on it and the hook refuses anything else.

Bounds.  fp64 forms: 1e-12, the project's bar for a kernel against its twin (summation order is the only difference).  Single-precision
forms: the reference runs the same cycle twice, in float64 and with float32 stencils, vectors and arithmetic on the levels the handle
runs in single precision (both with the STORED D of those levels); E = their maximum-norm distance on the same input is the reference
measured against itself, and the device must be within 16 E of the float64 cycle (4 for the device's other summation order - pair-summed
links, FMA contraction -, 4 for the maximum over 1e4 vertices being a tail statistic).  Every case prints its ratio device / E
(`RATIO ...` lines; DESIGN.md section 5b tabulates the largest per form).

Tuning keys the library does not report are set explicitly (PGX_NU_COARSE, PGX_COARSE_SWEEPS, PGX_TAIL_VERTS, PGX_MG_MIN_NX), and the
forms are forced onto these small grids as in test_gpu_mg32_bnd_tiles.py (K6 below), whose table the grids come from."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import vcycle_reference as VR
from tests.test_gpu_structured_kernels import _state

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
OMEGA = 0.75
ALPHAS = (2.5, 100.0)
EXPLICIT = {"PGX_NU_COARSE": 0, "PGX_COARSE_SWEEPS": 10, "PGX_TAIL_VERTS": 1100, "PGX_MG_MIN_NX": 4}
K6 = {"PGX_F32_K6_MAX": 2 ** 30, "PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500, "PGX_F32_BND_FULL_MIN": 0}
GRIDS32 = [(200, 72), (130, 260), (110, 60), (104, 46), (40, 90), (90, 30)]
GRIDS64 = [(96, 48), (72, 150)]
PGX_EINVAL, PGX_EHIP, PGX_ESTATE = -1, -2, -5
TOL64 = 1e-12
MARGIN32 = 16.0

_live = None  # ONE live handle: several tuning keys are process-wide and read at every launch
_blocks, _refs, _zref, _rhs_cache = {}, {}, {}, {}


class _Handle:
    def __init__(self, cells, alpha, keys):
        from proximalgalerkin_amd import _lib

        self.cells, self.alpha, self.keys = cells, alpha, dict(EXPLICIT, **keys)
        self.key = (cells, alpha, tuple(sorted(keys.items())))
        self.problem = None
        for k, v in self.keys.items():
            _lib.tuning_set(k, v)
        try:
            self._create()
        except BaseException:
            self.close()
            raise

    def _create(self):
        from proximalgalerkin_amd import fem
        from proximalgalerkin_amd.obstacle import setup_problem

        cells, alpha = self.cells, self.alpha
        nx, ny = cells
        msh = fem.create_rectangle(DOMAIN, cells)
        self.problem, sol, sol_k, a = setup_problem(msh)
        n2 = sol.function_space.num_dofs
        x, xk = _state(n2, 11)
        psi = x[n2 // 2:].reshape(ny + 1, nx + 1)
        psi[ny // 3: ny // 3 + 6, nx // 3: nx // 3 + 7] -= 800.0  # exp(psi) underflows: exact zeros in D, away from the frame
        sol_k.x.array[:] = xk
        a.value = alpha
        self.problem.assemble_jacobian(x)
        self.nlev = self.problem.mg_levels()
        self.info = [self.problem.mg_level_export(l) for l in range(self.nlev)]
        shapes = VR.coarse_shapes(nx, ny, self.keys["PGX_MG_MIN_NX"])
        assert [(i["nx"], i["ny"]) for i in self.info] == shapes, (shapes, [(i["nx"], i["ny"]) for i in self.info])
        # the fused tail: from the first level below the finest with at most PGX_TAIL_VERTS vertices, at most 8 levels
        self.tail_start = next((l for l in range(1, self.nlev) if self.info[l]["Dh"].shape[1] <= self.keys["PGX_TAIL_VERTS"] and self.nlev - l <= 8), None)
        self.last_entry = self.tail_start if self.tail_start is not None else self.nlev - 1
        self.f32_levels = tuple(l for l in range(self.nlev) if self.info[l]["f32"])

    def blocks(self):
        """(K, M, D) of the finest level as scipy matrices, exported once per grid and alpha."""
        k = (self.cells, self.alpha)
        if k not in _blocks:
            rowptr, col, K, M, D = self.problem.export_blocks()
            n = len(rowptr) - 1
            _blocks[k] = tuple(sp.csr_matrix((v, col, rowptr), shape=(n, n)) for v in (K, M, D))
        return _blocks[k]

    def reference(self, f32_levels=None):
        f32_levels = self.f32_levels if f32_levels is None else tuple(f32_levels)
        dbf16 = bool(self.info[f32_levels[0]]["dbf16"]) if f32_levels else True
        k = (self.cells, self.alpha, self.nlev, self.keys["PGX_MG_MIN_NX"], f32_levels, dbf16, self.keys["PGX_COARSE_SWEEPS"])
        if k not in _refs:
            K, M, D = self.blocks()
            nx, ny = self.cells
            _refs[k] = VR.VCycleReference(K, M, D, self.alpha, nx, ny, VR.frame_mask(nx, ny), n_levels=self.nlev, min_nx=self.keys["PGX_MG_MIN_NX"],
                                          coarse_sweeps=self.keys["PGX_COARSE_SWEEPS"], f32_levels=f32_levels, dbf16=dbf16)
        return k, _refs[k]

    def close(self):
        from proximalgalerkin_amd import _lib

        if self.problem is not None:
            self.problem.close()
        for k in self.keys:
            _lib.tuning_set(k, None)


def _handle(cells, alpha, keys):
    global _live
    key = (cells, alpha, tuple(sorted(keys.items())))
    if _live is not None and _live.key == key:
        return _live
    _drop()
    _live = _Handle(cells, alpha, keys)
    return _live


def _drop():
    global _live
    if _live is not None:
        live, _live = _live, None
        live.close()


def _apply(h, level, b, **kw):
    """pgx_vcycle_apply; a HIP runtime error ends the session (nothing more is launched on a device that reported one)."""
    from proximalgalerkin_amd._lib import PgxError

    try:
        return h.problem.vcycle_apply(level, b, **kw)
    except PgxError as e:
        if getattr(e, "code", 0) == PGX_EHIP:
            pytest.exit(f"HIP error in pgx_vcycle_apply: {e}", returncode=3)
        raise


@pytest.fixture(scope="module", autouse=True)
def _close_last_handle():
    yield
    _drop()


# ---------------------------------------------------------------------------------------------------------------------
# right-hand sides
# ---------------------------------------------------------------------------------------------------------------------
TILE_COLUMNS, TILE_ROWS = (52, 58, 60, 32), (4, 8, 12, 16, 20)


def _rhs(nx, ny, coarse=False):
    """name -> [u | psi] on the (nx, ny) grid; shared, read-only.  coarse: the grid is entered below the finest level, where a
    right-hand side is a restricted residual: its u part is 0 on the frame (every restriction masks it, and the fused tail relies on
    it - pgx_vcycle_apply refuses anything else)."""
    if (nx, ny, coarse) in _rhs_cache:
        return _rhs_cache[(nx, ny, coarse)]
    sx, n = nx + 1, (nx + 1) * (ny + 1)
    rng = np.random.default_rng(1000 * nx + ny)

    def impulses(vertices):
        v = np.unique(np.asarray(vertices, dtype=np.int64))
        b = np.zeros(2 * n)
        b[v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
        b[n + v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
        return b

    seams = []
    for w in TILE_COLUMNS:  # vertices (c - 1, j) and (c, j) of every seam column c, on every third row (offset by the seam's number)
        for k, c in enumerate(range(w, nx, w)):
            seams += [j * sx + c + d for j in range(1 + k % 3, ny, 3) for d in (-1, 0)]
    for t in TILE_ROWS:
        for k, r in enumerate(range(t, ny, t)):
            seams += [(r + d) * sx + i for i in range(1 + k % 3, nx, 3) for d in (-1, 0)]
    ring = [j * sx + i for j in range(1, ny) for i in range(1, nx) if i in (1, nx - 1) or j in (1, ny - 1)]
    out = {"random": rng.standard_normal(2 * n), "corners": impulses([0, nx, ny * sx, ny * sx + nx]), "frame-adjacent": impulses(ring)}
    if seams:
        out["seams"] = impulses(seams)
    for b in out.values():
        if coarse:
            b[:n][VR.frame_mask(nx, ny)] = 0.0
        b.setflags(write=False)
    _rhs_cache[(nx, ny, coarse)] = out
    return out


def _to_float(b):
    return b.astype(np.float32).astype(np.float64)


def _zr(refkey, ref, level, nu, mode, name, b, tag=""):
    k = (refkey, level, nu, mode, name, tag)
    if k not in _zref:
        z = ref.vcycle(b, level, nu=nu, omega=OMEGA, mode=mode)
        z.setflags(write=False)
        _zref[k] = z
    return _zref[k]


def _halves(z, zref):
    """max-norm deviation relative to max |zref|, on the u half and on the psi half"""
    n = len(z) // 2
    return tuple(np.abs(z[s] - zref[s]).max() / np.abs(zref[s]).max() for s in (slice(0, n), slice(n, 2 * n)))


def _check64(h, level, nu, label):
    """The device cycle entered on `level` against the float64 reference at 1e-12, for every right-hand side."""
    refkey, ref = h.reference(())
    info = h.info[level]
    worst = 0.0
    for name, b in _rhs(info["nx"], info["ny"], level > 0).items():
        z = _apply(h, level, b, nu=nu, omega=OMEGA)
        eu, ep = _halves(z, _zr(refkey, ref, level, nu, "f64", name, b))
        print(f"FP64 {label} {h.cells} alpha {h.alpha} level {level} nu {nu} {name}: u {eu:.2e} psi {ep:.2e}")
        worst = max(worst, eu, ep)
        assert eu <= TOL64 and ep <= TOL64, (label, h.cells, h.alpha, level, nu, name, eu, ep)
    return worst


def _check32(h, level, nu, label, names=None, in_form=0, out_form=0, scale=1.0):
    """The device cycle entered on single-precision `level` against the float64 reference with stored D, within 16 E; returns the
    device results by right-hand side."""
    assert level in h.f32_levels, (label, h.cells, level, h.f32_levels)
    refkey, ref = h.reference()
    info = h.info[level]
    res = {}
    for name, b in _rhs(info["nx"], info["ny"], level > 0).items():
        if names is not None and name not in names:
            continue
        tag = ""
        if level > 0:  # the hook hands these over as floats: both sides start from the same numbers.  (Level 0, in_form 1: the float
            b, tag = _to_float(b), "float"  # pair is what FGMRES's float basis stores of b, a rounding of the device path like IO = 1's)
        bref = b
        if scale != 1.0:
            bref, tag = scale * b, tag + f"*{scale}"
        z = _apply(h, level, b, nu=nu, omega=OMEGA, in_form=in_form, out_form=out_form, scale=scale)
        z64 = _zr(refkey, ref, level, nu, "f64", name, bref, tag)
        z32 = _zr(refkey, ref, level, nu, "f32", name, bref, tag)
        E, dev = _halves(z32, z64), _halves(z, z64)
        ratios = tuple(d / e for d, e in zip(dev, E))
        print(f"RATIO {label} {h.cells} alpha {h.alpha} level {level} nu {nu} {name}: E u {E[0]:.2e} psi {E[1]:.2e}  device/E u {ratios[0]:.2f} "
              f"psi {ratios[1]:.2f}")
        assert E[0] > 0.0 and E[1] > 0.0
        assert dev[0] <= MARGIN32 * E[0] and dev[1] <= MARGIN32 * E[1], (label, h.cells, h.alpha, level, nu, name, dev, E, ratios)
        res[name] = z
    return res


# ---------------------------------------------------------------------------------------------------------------------
# a. coarse operators
# ---------------------------------------------------------------------------------------------------------------------
def _check_operators(h):
    _, ref = h.reference(())
    K, M, D0 = h.blocks()
    for l, info in enumerate(h.info):
        L = ref.levels[l]
        want = VR.half_stencil(L["D"], L["nx"], L["ny"])
        err = np.abs(info["Dh"] - want).max() / np.abs(want).max()
        print(f"OPER {h.cells} alpha {h.alpha} {h.key[2]} level {l}: |Dh - P^T D P| / max |D| = {err:.2e}")
        assert err <= 1e-13, (h.cells, l, err)
        assert np.array_equal(info["mask"], VR.frame_mask(L["nx"], L["ny"])) and np.array_equal(info["mask"], L["mask"])
        if l == 0:
            assert np.array_equal(info["Dh"] == 0.0, want == 0.0)  # exp(psi) underflows in the same entries ...
            assert (want[0] == 0.0).sum() >= 6  # ... and the state has some
        if info["f32"]:
            got = info["Dq"].T  # [4, n], decoded
            stored = VR.stored_d(info["Dh"], bool(info["dbf16"]))
            assert np.array_equal(got.view(np.uint32), stored.view(np.uint32)), (h.cells, l, "Dq is not the packing of Dh")


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("cells", GRIDS32 + GRIDS64)
def test_level_operators_are_galerkin_and_dq_is_the_packing_of_dh(require_gpu, cells, direct):
    """Dh of every level = P^T D P to 1e-13 of the level's max |D|; the mask = the frame; the exact zeros of level 0 = the underflow
    set; Dq decoded = pack_d(Dh) bit for bit (bf16) - with D(psi) stored by the kernels that compute it (PGX_D_DIRECT=1) and by the
    separate conversion and packing launches (0)."""
    for alpha in ALPHAS:
        _check_operators(_handle(cells, alpha, dict(K6, PGX_D_DIRECT=direct)))


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("cells", GRIDS32 + GRIDS64)
def test_level_operators_with_float4_dq(require_gpu, cells, direct):
    """PGX_F32_DBF16=0: Dq = float(min(Dh, 1e30)), bit for bit."""
    h = _handle(cells, ALPHAS[0], dict(K6, PGX_D_DIRECT=direct, PGX_F32_DBF16=0))
    assert h.f32_levels and not any(h.info[l]["dbf16"] for l in h.f32_levels)
    _check_operators(h)


@pytest.mark.parametrize("dbf16", [1, 0])
@pytest.mark.parametrize("cells", [(200, 72), (130, 260)])
def test_level_operators_from_lds_staged_coarsening(require_gpu, cells, dbf16):
    """PGX_RAP_LDS_MIN=0: k_rap7h_lds coarsens onto every level, the small ones included."""
    for alpha in ALPHAS:
        _check_operators(_handle(cells, alpha, dict(K6, PGX_D_DIRECT=1, PGX_RAP_LDS_MIN=0, PGX_F32_DBF16=dbf16)))


# ---------------------------------------------------------------------------------------------------------------------
# b. the plain fp64 cycle: one launch per sweep, residual, restriction and prolongation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [1, 2, 6])
@pytest.mark.parametrize("cells", GRIDS32 + GRIDS64)
def test_plain_fp64_cycle_on_every_level(require_gpu, cells, nu):
    """level_apply sweeps, pgxk_restrict, pgxk_prolong_add (PGX_MG_F32=0, PGX_FUSED_LEGS=0), entered on every level down to the
    coarsest: the anchor of the reference on the simplest kernels.  PGX_TAIL_VERTS=0: no fused tail, every level is entered."""
    for alpha in ALPHAS:
        h = _handle(cells, alpha, {"PGX_MG_F32": 0, "PGX_FUSED_LEGS": 0, "PGX_TAIL_VERTS": 0})
        assert h.tail_start is None and not h.f32_levels
        for level in range(h.nlev):
            _check64(h, level, nu, "plain")


# ---------------------------------------------------------------------------------------------------------------------
# c. the fused fp64 forms
# ---------------------------------------------------------------------------------------------------------------------
F64 = {"PGX_MG_F32": 0, "PGX_FUSED_MIN": 500}
FORMS64 = {
    "K2-nu2": (F64, 2), "K2-nu4": (F64, 4),                        # pgxk_st_smooth2, pgxk_st_resid_restrict
    "K3-nu3": (F64, 3), "K3-nu6": (dict(F64, PGX_K6_MAX=0), 6),    # k_st_smoothR, three sweeps per launch
    "K3-tiles-nu3": (dict(F64, PGX_SMOOTH_ROWMAP=0), 3),           # k_st_smoothK, the tile-mapped kernel
    "K3-ty8-nu6": (dict(F64, PGX_K6_MAX=0, PGX_ROWMAP_TY=8), 6), "K3-ty16-nu3": (dict(F64, PGX_ROWMAP_TY=16), 3),
    "K6": (dict(F64, PGX_K6_MAX=2 ** 30), 6), "K6-ty16": (dict(F64, PGX_K6_MAX=2 ** 30, PGX_K6_TY=16), 6),
    "tail-old-nu6": (dict(F64, PGX_TAIL2=0), 6), "tail-old-nu2": (dict(F64, PGX_TAIL2=0), 2),   # the round-2 tail kernels
    "min-nx-2": (dict(F64, PGX_MG_MIN_NX=2), 6),                   # a deeper hierarchy inside the tail
    "tail-deep": (dict(F64, PGX_MG_MIN_NX=2, PGX_TAIL_VERTS=5000), 6),  # the tail entered one level higher
}


@pytest.mark.parametrize("form", list(FORMS64))
@pytest.mark.parametrize("cells", GRIDS64 + [(200, 72), (40, 90)])
def test_fused_fp64_forms_on_every_level(require_gpu, cells, form):
    """k_st_smoothK with 2, 3 and 6 sweeps per launch, pgxk_st_resid_restrict, k_mg_tail2 and the older tail: entered on every level
    down to and including the first level of the tail, against the float64 reference at 1e-12."""
    keys, nu = FORMS64[form]
    for alpha in ALPHAS:
        h = _handle(cells, alpha, keys)
        assert not h.f32_levels
        for level in range(h.last_entry + 1):
            _check64(h, level, nu, form)
        if h.last_entry + 1 < h.nlev:  # levels inside the tail are not entry points
            with pytest.raises(Exception) as e:
                _apply(h, h.last_entry + 1, np.zeros(2 * h.info[h.last_entry + 1]["Dh"].shape[1]), nu=nu)
            assert e.value.code == PGX_EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# d. the single-precision forms
# ---------------------------------------------------------------------------------------------------------------------
def _run32(cells, keys, nu, label, **kw):
    for alpha in ALPHAS:
        h = _handle(cells, alpha, keys)
        assert h.f32_levels and h.f32_levels[0] == 0, (cells, keys, h.f32_levels)
        for level in h.f32_levels:
            _check32(h, level, nu, label, **kw)


@pytest.mark.parametrize("rr", ["default", 0])
@pytest.mark.parametrize("full", [1, 0])
@pytest.mark.parametrize("ty", [8, 12, 16, 20])
@pytest.mark.parametrize("cells", GRIDS32)
def test_six_sweep_single_precision_launches(require_gpu, cells, ty, full, rr):
    """K = 6 at every tile height, with whole boundary tiles and four-row sub-tiles, with the restriction fused into the
    pre-smoothing launch and launched on its own."""
    keys = dict(K6, PGX_F32_TY=ty, PGX_F32_BND_FULL=full)
    if rr != "default":
        keys["PGX_F32_RR_MAX"] = rr
    _run32(cells, keys, 6, f"K6-ty{ty}-{'full' if full else 'sub'}-{'rr' if rr == 'default' else 'norr'}")


SMALL = {"PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500}
K32 = {"K3-nu3": (SMALL, 3), "K3-nu6": (dict(SMALL, PGX_F32_K6_MAX=0), 6), "K2-nu2": (SMALL, 2), "K2-nu4": (SMALL, 4)}


@pytest.mark.parametrize("rr", ["default", 0])
@pytest.mark.parametrize("ty", [4, 8, 16])
@pytest.mark.parametrize("form", list(K32))
@pytest.mark.parametrize("cells", [(200, 72), (130, 260), (40, 90)])
def test_three_and_two_sweep_single_precision_launches(require_gpu, cells, form, ty, rr):
    keys, nu = K32[form]
    keys = dict(keys, PGX_F32_TY=ty)
    if rr != "default":
        keys["PGX_F32_RR_MAX"] = rr
    _run32(cells, keys, nu, f"{form}-ty{ty}-{'rr' if rr == 'default' else 'norr'}")


@pytest.mark.parametrize("form", ["K6", "K3-nu3", "K2-nu2"])
def test_single_precision_launches_with_float4_dq(require_gpu, form):
    """PGX_F32_DBF16=0 once per sweep count (the float4 instantiations of every kernel)."""
    keys, nu = (K6, 6) if form == "K6" else K32[form]
    _run32((200, 72), dict(keys, PGX_F32_DBF16=0), nu, f"{form}-float4")
    _run32((200, 72), dict(keys, PGX_F32_DBF16=0, PGX_F32_RR_MAX=0), nu, f"{form}-float4-norr")


@pytest.mark.parametrize("rr", ["default", 0])
@pytest.mark.parametrize("nu", [6, 3, 2])
def test_single_precision_level_above_an_unfused_fp64_level(require_gpu, nu, rr):
    """A single-precision level that hands its right-hand side down, and takes its correction back, in fp64 (the CB64 and CADD = 2
    forms) from a level that is NOT the fused tail: PGX_F32_MIN = 10000 keeps level 1 of (200, 72) (3737 vertices) in fp64 while
    level 0 (14673) stays single precision.  (Every grid whose level 1 is the tail or the coarsest level runs these forms too.)"""
    keys = dict(K6, PGX_F32_MIN=10000)
    if rr != "default":
        keys["PGX_F32_RR_MAX"] = rr
    for alpha in ALPHAS:
        h = _handle((200, 72), alpha, keys)
        assert h.f32_levels == (0,) and h.tail_start == 2
        _check32(h, 0, nu, f"K{nu}-over-fp64-{'rr' if rr == 'default' else 'norr'}")


def test_f32_min_above_the_grid_runs_the_fp64_cycle(require_gpu):
    """PGX_F32_MIN = 20000 on (200, 72): more than the 14673 vertices of its finest level, so no level is single precision and the
    cycle is the fused fp64 one - at the fp64 bound."""
    for alpha in ALPHAS:
        h = _handle((200, 72), alpha, dict(K6, PGX_F32_MIN=20000))
        assert not h.f32_levels
        for level in range(h.last_entry + 1):
            _check64(h, level, 6, "f32-min-20000")


LEVEL0_FORMS = [("K6-ty8", dict(K6, PGX_F32_TY=8), 6), ("K6-ty20-full", dict(K6, PGX_F32_TY=20), 6), ("K6-ty12-norr", dict(K6, PGX_F32_TY=12, PGX_F32_RR_MAX=0), 6),
                ("K6-ty16-sub", dict(K6, PGX_F32_TY=16, PGX_F32_BND_FULL=0), 6), ("K3-nu3", dict(SMALL, PGX_F32_TY=8), 3), ("K2-nu4", dict(SMALL, PGX_F32_TY=4), 4)]


@pytest.mark.parametrize("label,keys,nu", LEVEL0_FORMS, ids=[f[0] for f in LEVEL0_FORMS])
@pytest.mark.parametrize("cells", [(200, 72), (130, 260), (40, 90)])
def test_level0_input_and_output_forms(require_gpu, cells, label, keys, nu):
    """The finest level's first launch reading the float pair of FGMRES's float basis (in_form 1: IO = 3) and the lazily normalised
    fp64 pair (scale 0.37), its last launch leaving the float2 field FGMRES keeps as Z_j (out_form 1)."""
    for alpha in ALPHAS:
        h = _handle(cells, alpha, keys)
        z0 = _check32(h, 0, nu, label + "-io1")
        zf = _check32(h, 0, nu, label + "-io3", in_form=1)
        zs = _check32(h, 0, nu, label + "-scale", scale=0.37)
        for name, b in _rhs(*cells).items():
            # the factor is applied in fp64 as the right-hand side is read: the cycle of 0.37 b, bit for bit
            assert np.array_equal(zs[name], _apply(h, 0, 0.37 * b, nu=nu, omega=OMEGA)), (label, name)
            # the float2 result is the float cast of the fp64 one, bit for bit
            z2 = _apply(h, 0, b, nu=nu, omega=OMEGA, out_form=1)
            assert np.array_equal(z2.astype(np.float32).view(np.uint32), z0[name].astype(np.float32).view(np.uint32)), (label, name)
            assert np.array_equal(z2, z2.astype(np.float32).astype(np.float64))
            same = np.array_equal(zf[name], _apply(h, 0, _to_float(b), nu=nu, omega=OMEGA))
            print(f"{label} {cells} {name}: float-pair input bitwise equal to the fp64 pair holding the same floats: {same}")
        # both forms at once, as FGMRES's lean path runs them
        _check32(h, 0, nu, label + "-io3-out2", in_form=1, out_form=1)


# ---------------------------------------------------------------------------------------------------------------------
# e. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refused(problem, code, level=0, n2=None, **kw):
    from proximalgalerkin_amd._lib import PgxError

    with pytest.raises(PgxError) as e:
        problem.mg_level_export(level)
    assert e.value.code == (code if code == PGX_ESTATE else PGX_EINVAL)
    if n2 is not None:
        with pytest.raises(PgxError) as e:
            problem.vcycle_apply(level, np.ones(n2), **kw)
        assert e.value.code == code


def _spmv_works(problem, n2):
    v = np.random.default_rng(3).standard_normal(n2)
    y = problem.spmv(v)
    assert np.isfinite(y).all() and np.abs(y).max() > 0.0
    return y


def test_refusals_leave_the_handle_usable(require_gpu):
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd._lib import PgxError
    from proximalgalerkin_amd.obstacle import setup_problem

    _drop()
    lib = _lib.load()
    cells = (48, 32)

    def state(problem, sol, sol_k, alpha, fill=True):
        n2 = sol.function_space.num_dofs
        x, xk = _state(n2, 13)
        sol_k.x.array[:] = xk
        alpha.value = 2.5
        if fill:
            problem.assemble_jacobian(x)
        return n2, x

    def raw_apply(problem, level, n2, **kw):
        """the C call itself: the Python method asks pgx_mg_level_export for the level's size first"""
        b, z = np.ones(n2), np.empty(n2)
        return lib.pgx_vcycle_apply(problem._h, level, kw.get("nu", 6), OMEGA, kw.get("in_form", 0), kw.get("out_form", 0), kw.get("scale", 1.0),
                                    _lib.dptr(b), _lib.dptr(z))

    # a P2 handle: the export serves the P1 hierarchy below its P2 level (tests/test_gpu_p2_cycle_operator.py compares it), the
    # V-cycle hook keeps its P1 precondition
    problem, sol, sol_k, alpha = setup_problem(fem.create_rectangle(DOMAIN, (16, 16)), 2)
    n2, _ = state(problem, sol, sol_k, alpha)
    assert problem.mg_levels() == 3 and problem.mg_level_export(0)["Dh"].shape == (4, 17 * 17)  # (16, 16), (8, 8), (4, 4)
    with pytest.raises(PgxError) as e:
        problem.vcycle_apply(0, np.ones(2 * 17 * 17))
    assert e.value.code == PGX_ESTATE
    assert raw_apply(problem, 0, n2) == PGX_ESTATE and raw_apply(problem, 0, 2 * 17 * 17) == PGX_ESTATE
    _spmv_works(problem, n2)
    problem.close()
    # an unstructured mesh (the same triangles without the grid structure: single-level smoother, no hierarchy)
    grid = fem.create_rectangle(DOMAIN, cells)
    problem, sol, sol_k, alpha = setup_problem(fem.Mesh(grid.geometry, grid.cells))
    n2, _ = state(problem, sol, sol_k, alpha)
    _refused(problem, PGX_ESTATE)
    assert raw_apply(problem, 0, n2) == PGX_ESTATE
    _spmv_works(problem, n2)
    problem.close()
    # a structured handle: unfilled Jacobian, then levels out of range, forms the level cannot run
    problem, sol, sol_k, alpha = setup_problem(grid)
    n2, x = state(problem, sol, sol_k, alpha, fill=False)
    _refused(problem, PGX_ESTATE)
    assert raw_apply(problem, 0, n2) == PGX_ESTATE
    problem.assemble_jacobian(x)
    y = _spmv_works(problem, n2)
    nlev = problem.mg_levels()
    assert nlev == 4  # (48, 32), (24, 16), (12, 8), (6, 4); the tail starts on level 1 (425 vertices)
    for level in (-1, nlev, 2):
        assert raw_apply(problem, level, n2) == PGX_EINVAL, level
    for level in (-1, nlev):
        with pytest.raises(PgxError) as e:
            problem.mg_level_export(level)
        assert e.value.code == PGX_EINVAL
    assert raw_apply(problem, 0, n2, in_form=2) == PGX_EINVAL and raw_apply(problem, 0, n2, nu=0) == PGX_EINVAL
    assert raw_apply(problem, 1, 2 * 25 * 17) == PGX_EINVAL  # b_u = 1 on the coarse frame: no restricted residual looks like that
    assert raw_apply(problem, 1, 2 * 25 * 17, scale=0.5) == PGX_EINVAL and raw_apply(problem, 1, 2 * 25 * 17, out_form=1) == PGX_EINVAL
    # level 0 of this grid (1617 vertices) is below PGX_F32_MIN: the fp64 cycle reads neither a float pair nor a factor
    assert problem.mg_level_export(0)["f32"] == 0
    assert raw_apply(problem, 0, n2, in_form=1) == PGX_EINVAL and raw_apply(problem, 0, n2, scale=0.5) == PGX_EINVAL
    assert raw_apply(problem, 0, n2, out_form=1) == PGX_ESTATE
    assert np.array_equal(problem.spmv(np.random.default_rng(3).standard_normal(n2)), y)
    problem.close()
    # out_form 1 without the float2 Z storage, and a sweep count the single-precision legs do not run
    for k, v in dict(SMALL, PGX_Z_F32=0).items():
        _lib.tuning_set(k, v)
    try:
        problem, sol, sol_k, alpha = setup_problem(grid)
        n2, x = state(problem, sol, sol_k, alpha)
        assert problem.mg_level_export(0)["f32"] == 1
        assert raw_apply(problem, 0, n2, out_form=1) == PGX_ESTATE
        assert raw_apply(problem, 0, n2, nu=5) == PGX_EINVAL
        assert raw_apply(problem, 0, n2, in_form=1) == 0 and raw_apply(problem, 0, n2) == 0
        assert np.array_equal(problem.spmv(np.random.default_rng(3).standard_normal(n2)), y)
        problem.close()
    finally:
        for k in dict(SMALL, PGX_Z_F32=0):
            _lib.tuning_set(k, None)
