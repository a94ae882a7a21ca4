"""The export order of the mixed CSR patterns, pinned: for each create path of the sparse-LU families, at the smallest mesh its
front end accepts that is not square or cubic, `csr_export` returns the rowptr / col arrays whose sha256 and nnz
tests/golden/mixed_patterns.json records.  The arrays are integers built on the host (csrc/pgx_pattern.h and the block layouts of
the families), so equality is exact; the fixture was recorded before the pattern builders were shared and pins the order for good."""
import ctypes as C
import hashlib
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "mixed_patterns.json"


def _gc(general):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.gradient_constraint import GradientConstraintProblem, f_default, phi_default

    return GradientConstraintProblem(fem.create_unit_square(5, 4), phi_default, f_default, general=general)


def _sg():
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(3, 2, 2)
    mt, _ = G.native_tags(mesh)
    return G.SignoriniProblem(mesh, mt.find(2), np.unique(mt.find(1).ravel()), 2.0e4, 0.3, 0.0, -0.25)


def _sg2d():
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import signorini as G

    mesh = fem.create_unit_square(5, 4)
    mt, _ = G.native_tags(mesh)
    return G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.0, -0.25, degree=1, bc_facets=mt.find(1))


def _qvi():
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.thermoforming import ThermoformingProblem

    return ThermoformingProblem(fem.create_unit_square(5, 4))


def _qmy():
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.thermoforming_comparison import PenalisedThermoformingProblem

    return PenalisedThermoformingProblem(fem.create_unit_square(5, 4))


def _ic():
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import intersecting as I

    return I.IntersectingProblem(fem.IntervalMesh(np.array([0.0, 0.1, 0.25, 0.4, 0.5, 0.7, 0.85, 1.0])), I.phi0_bump, I.phi_bound(0.5))


def _mp():
    from proximalgalerkin_amd import fem, multiphase

    return multiphase.MultiphaseProblem(fem.create_unit_square(5, 4, diagonal="crossed"))


def _fr():
    from proximalgalerkin_amd import fracture
    from proximalgalerkin_amd.mesh_generation import create_crack_mesh

    mesh, ft, names = create_crack_mesh(0.4)
    return fracture.FractureProblem(mesh, fracture.boundary_vertices(ft, "topleft", names), fracture.boundary_vertices(ft, "topright", names))


def _ev():
    from proximalgalerkin_amd import eigenvalue, fem

    return eigenvalue.EigenvalueProblem(fem.QuadMesh(((0.0, 0.0), (1.0, 1.0)), (5, 4)), 2, 8)


CASES = {
    "gc_structured": lambda: _gc(False),
    "gc_general": lambda: _gc(True),
    "sg_p1_tets": _sg,
    "sg2d_p1_triangles": _sg2d,
    "qvi": _qvi,
    "qmy": _qmy,
    "ic": _ic,
    "mp": _mp,
    "fr": _fr,
    "ev": _ev,
}


def pattern_pin(problem):
    """{"nnz", "rowptr_sha256", "col_sha256"} of the handle's csr_export (the pattern alone: no Jacobian needs to be filled)"""
    from proximalgalerkin_amd import _lib

    nr, nnz = C.c_int64(0), C.c_int64(0)
    problem._call("csr_export", C.byref(nr), C.byref(nnz), None, None, None)
    rp, col = np.empty(nr.value + 1, np.int32), np.empty(nnz.value, np.int32)
    problem._call("csr_export", None, None, _lib.iptr(rp), _lib.iptr(col), None)
    assert nr.value == problem.ndofs and rp[0] == 0 and rp[-1] == nnz.value
    return {"nnz": int(nnz.value), "rowptr_sha256": hashlib.sha256(rp.tobytes()).hexdigest(),
            "col_sha256": hashlib.sha256(col.tobytes()).hexdigest()}


@pytest.mark.parametrize("name", list(CASES))
def test_exported_pattern_is_the_recorded_one(require_gpu, name):
    problem = CASES[name]()
    try:
        assert pattern_pin(problem) == json.loads(GOLDEN.read_text())[name]
    finally:
        problem.close()
