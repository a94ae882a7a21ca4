"""The first launch of a six-sweep leg with a halo of five: k_f_smooth<..., HF = 1> of csrc/pgx_mg32.hip.

A leg's first launch starts from x = 0, so its first sweep reads no neighbour and is exact on the whole 64 x 32 image; sweep s is then
exact s - 1 rings in and the image owns 54 x 22 vertices instead of 52 x 20.  The library takes the form from 1 000 000 vertices up
(PGX_F32_FIRST_HALO_MIN), on levels with whole boundary tiles, where no restriction is fused into the launch and PGX_F32_TY is unset or
20.  Here PGX_F32_FIRST_HALO_MIN=0 forces it onto small grids and PGX_F32_RR_MAX=0 keeps the restriction out of the first launches, so
that they qualify on every single-precision level; the K6 keys of test_gpu_vcycle_operator.py put the six-sweep launches and whole
boundary tiles there.

Grids: (200, 72) and (130, 260) - 4 x 4 and 3 x 12 tiles of 54 x 22 with interior tiles, a partial last tile column and row, every
kind of whole boundary tile; (130, 260) has its fp64 coarsest level right below level 0 - and (40, 90), which has no interior tile.

1. the cycle as an operator against tests/vcycle_reference.py, with that file's bound (_check32: within MARGIN32 x the float
   reference's own error E of the float64 cycle), for the three input forms of level 0 and entered on level 1;
2. the new form against the 52 x 20 form (PGX_F32_FIRST_HALO=0) of the same library on right-hand sides that sit on the seams of
   both tilings;
3. PGX_F32_FIRST_HALO=0 against the defaults on a full solve: below the threshold the key changes nothing."""
import numpy as np
import pytest

from tests.test_gpu_mg32_bnd_tiles import _solve
from tests.test_gpu_vcycle_operator import ALPHAS, K6, MARGIN32, OMEGA, _apply, _check32, _drop, _handle, _rhs

pytestmark = pytest.mark.gpu
FORCED = dict(K6, PGX_F32_FIRST_HALO_MIN=0, PGX_F32_RR_MAX=0)
GRIDS = [(200, 72), (130, 260), (40, 90)]
NU = 6
_seam_cache = {}


@pytest.fixture(autouse=True)
def _close_the_live_handle():
    """The handle of test_gpu_vcycle_operator.py stays open, with its tuning keys set, until the next one is asked for: every test
    here starts and ends without one, so that the solves below and the modules after this one run under their own keys only."""
    _drop()
    yield
    _drop()


@pytest.mark.parametrize("ty", ["unset", 20])
@pytest.mark.parametrize("cells", GRIDS)
def test_halo_five_first_launch_as_an_operator(require_gpu, cells, ty):
    """One cycle per right-hand side of test_gpu_vcycle_operator.py: entered on level 0 with the fp64 pair, the float pair of
    FGMRES's float basis (IO = 3) and a lazily applied factor, and on every lower single-precision level (IO = 0)."""
    keys = dict(FORCED) if ty == "unset" else dict(FORCED, PGX_F32_TY=ty)
    for alpha in ALPHAS:
        h = _handle(cells, alpha, keys)
        assert h.f32_levels and h.f32_levels[0] == 0, (cells, h.f32_levels)
        _check32(h, 0, NU, f"first-halo-ty{ty}-io1")
        _check32(h, 0, NU, f"first-halo-ty{ty}-io3", in_form=1)
        _check32(h, 0, NU, f"first-halo-ty{ty}-scale", scale=0.37)
        for level in h.f32_levels[1:]:
            _check32(h, level, NU, f"first-halo-ty{ty}-level{level}")
    if cells == (200, 72):
        assert 1 in h.f32_levels  # the new form below the finest level, too


def _seam_rhs(nx, ny):
    """name -> [u | psi]: the random right-hand side of test_gpu_vcycle_operator.py, and impulses on both sides of every seam of
    the new tiling (columns at multiples of 54, rows at multiples of 22), of the old one (52, 20) and next to the frame - built as in
    tests/test_gpu_mg32_lds_reads.py:rhs.  Shared and read-only."""
    if (nx, ny) in _seam_cache:
        return _seam_cache[(nx, ny)]
    sx, n = nx + 1, (nx + 1) * (ny + 1)
    rng = np.random.default_rng(5400 * nx + ny)

    def impulses(v):
        v = np.unique(np.asarray(v, dtype=np.int64))
        b = np.zeros(2 * n)
        b[v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
        b[n + v] = rng.choice([-1.0, 1.0], len(v)) * rng.uniform(0.5, 1.5, len(v))
        return b

    def seams(w, t):
        v = []
        for k, c in enumerate(range(w, nx, w)):  # both sides of every seam column, on every third row
            v += [j * sx + c + d for j in range(1 + k % 3, ny, 3) for d in (-1, 0)]
        for k, r in enumerate(range(t, ny, t)):
            v += [(r + d) * sx + i for i in range(1 + k % 3, nx, 3) for d in (-1, 0)]
        return v

    ring = [j * sx + i for j in range(1, ny) for i in range(1, nx) if i in (1, nx - 1) or j in (1, ny - 1)]
    out = {"random": _rhs(nx, ny)["random"], "seams-54x22": impulses(seams(54, 22)), "seams-52x20": impulses(seams(52, 20)),
           "frame-adjacent": impulses(ring)}
    for b in out.values():
        b.setflags(write=False)
    _seam_cache[(nx, ny)] = out
    return out


@pytest.mark.parametrize("cells", GRIDS)
def test_halo_five_against_the_halo_six_form(require_gpu, cells):
    """Level 0 entered under the same keys with PGX_F32_FIRST_HALO=1 and =0.  Every vertex takes the same six sweeps from the same
    numbers in both tilings; both results are within MARGIN32 x E of the float64 reference, and their distance and whether they are
    bitwise equal is printed."""
    nx, ny = cells
    rhs = _seam_rhs(nx, ny)
    for alpha in ALPHAS:
        z = {}
        for on in (1, 0):
            h = _handle(cells, alpha, dict(FORCED, PGX_F32_TY=20, PGX_F32_FIRST_HALO=on))  # (20: the 52 x 20 tiles on the other side)
            z[on] = {name: _apply(h, 0, b, nu=NU, omega=OMEGA) for name, b in rhs.items()}
        _, ref = h.reference()
        n = (nx + 1) * (ny + 1)
        halves = (slice(0, n), slice(n, 2 * n))
        for name, b in rhs.items():
            z64 = ref.vcycle(b, 0, nu=NU, omega=OMEGA, mode="f64")
            z32 = ref.vcycle(b, 0, nu=NU, omega=OMEGA, mode="f32")
            E = [np.abs(z32[s] - z64[s]).max() / np.abs(z64[s]).max() for s in halves]
            assert E[0] > 0.0 and E[1] > 0.0
            d = np.abs(z[1][name] - z[0][name])
            print(f"FIRST-HALO {cells} alpha {alpha} {name}: max |z_5 - z_6| = {d.max():.3e} (max |z| {np.abs(z[0][name]).max():.3e}), "
                  f"{int((z[1][name] != z[0][name]).sum())} entries differ, bitwise equal: {np.array_equal(z[1][name], z[0][name])}")
            for on in (1, 0):
                dev = [np.abs(z[on][name][s] - z64[s]).max() / np.abs(z64[s]).max() for s in halves]
                print(f"FIRST-HALO {cells} alpha {alpha} {name} halo {6 - on}: E u {E[0]:.2e} psi {E[1]:.2e}  device/E u {dev[0] / E[0]:.2f} "
                      f"psi {dev[1] / E[1]:.2f}")
                assert dev[0] <= MARGIN32 * E[0] and dev[1] <= MARGIN32 * E[1], (cells, alpha, name, on, dev, E)


def test_key_at_zero_changes_nothing_below_the_threshold(require_gpu):
    """(200, 72) has 14 673 vertices: with the default threshold no launch takes the new form, and the full Newton solve with
    PGX_F32_FIRST_HALO=0 is the default library's, bit for bit, with the same Newton and Krylov counts."""
    a, na, la = _solve((200, 72), {})
    b, nb, lb = _solve((200, 72), {"PGX_F32_FIRST_HALO": 0})
    assert na == nb and la == lb
    assert np.array_equal(a, b)


def test_full_solve_with_the_halo_five_form_forced(require_gpu):
    """The LVPP run of (200, 72) with the new form on both single-precision levels: the Newton counts of the fp64 cycle, u to 1e-10."""
    x64, n64, _ = _solve((200, 72), {"PGX_MG_F32": 0})
    x, newton, _ = _solve((200, 72), FORCED)
    n = 201 * 73
    err = np.linalg.norm(x[:n] - x64[:n]) / np.linalg.norm(x64[:n])
    print(f"(200, 72) forced halo five: newton {newton} rel-L2(u) vs fp64 cycle {err:.2e}")
    assert newton == n64
    assert err <= 1e-10

