"""The evidence behind the bf16 storage of the single-precision V-cycle's D(psi) stencil (csrc/pgx_mg32.hip, PGX_F32_DBF16), on
the numpy twin of the Newton linear solver (tools/mg32_study.py on oracle/krylov_proto.py): with D stored as bf16 - rounded to
nearest even after the clamp at 1e30, arithmetic still float - the Krylov count of EVERY linear solve of a settings-B run equals
the float cycle's, and the Newton counts are the exact-Newton oracle's.  Equality is the condition: the cycle is a preconditioner
inside FGMRES and D carries eight bits it does not use."""
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import pg_oracle as O

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def study():
    spec = importlib.util.spec_from_file_location("mg32_study", ROOT / "tools" / "mg32_study.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_bf16_rounding_helper(study):
    r = study.bf16_round
    # ties to even: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 -> 1 (even); 1 + 3 * 2^-8 halfway between 1 + 2^-7 and 1 + 2^-6 ->
    # 1 + 2^-6 (even); anything above a tie goes up, anything below goes down
    got = r(_f32([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF])).view(np.uint32)
    assert got.tolist() == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000]
    # the result always has an empty low half and is at most half a bf16 ulp away (8 significand bits: 2^-8 relative)
    x = np.random.default_rng(0).standard_normal(10000).astype(np.float32) * np.float32(1e3)
    y = r(x)
    assert not (y.view(np.uint32) & 0xFFFF).any()
    assert np.all(np.abs(y - x) <= np.abs(x) * 2.0 ** -8)
    assert np.array_equal(r(y), y)  # idempotent: a bf16 value is stored exactly
    # +-0 stay +-0 (the det != 0 tests and the underflow set of exp(psi) depend on exact zeros)
    z = r(_f32([0x00000000, 0x80000000])).view(np.uint32)
    assert z.tolist() == [0x00000000, 0x80000000]
    # the clamp of k_f_pack_d comes first: anything above 1e30, infinity included, is stored as the bf16 nearest to 1e30 - finite
    big = study.pack_d(np.array([3e38, np.inf, 2e30, 1e30], dtype=np.float32))
    assert np.all(np.isfinite(big)) and np.all(big == r(np.array([1e30], dtype=np.float32))[0])
    assert abs(float(big[0]) / 1e30 - 1.0) <= 2.0 ** -8
    # float denormals: the same bit arithmetic - the upper seven mantissa bits survive, what lies below half of the last one is +0
    d = r(_f32([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF])).view(np.uint32)
    assert d.tolist() == [0x00000000, 0x00000000, 0x00000000, 0x00010000, 0x00020000, 0x00800000]


def test_bf16_stencil_storage_keeps_every_krylov_count_of_the_twin(study):
    N = 64
    coords, cells = O.create_rectangle(N, N)
    prob = O.ObstacleP1(coords, cells, O.boundary_vertices_rectangle(N, N))
    _, h_ref = O.solve_problem(prob, 500, "double_exponential", 1e2, 1e-4)  # exact Newton steps (sparse LU)
    runs = {}
    for name, narrow in (("float", {}), ("bf16 D", dict(narrow="D"))):
        stats = []
        x, h = O.solve_problem(prob, 500, "double_exponential", 1e2, 1e-4, linear_solve=study.make(prob, N, 0, stats, 0.75, **narrow))
        print(f"{name}: Newton {h['Newton steps']} Krylov per solve {stats} total {sum(stats)}")
        assert h["Newton steps"] == h_ref["Newton steps"], name
        runs[name] = (x, stats)
    (xf, kf), (xb, kb) = runs["float"], runs["bf16 D"]
    assert len(kf) == sum(h_ref["Newton steps"])
    assert kb == kf  # every linear solve, not only the total
    assert np.linalg.norm(xb[: prob.n] - xf[: prob.n]) <= 1e-10 * np.linalg.norm(xf[: prob.n])
