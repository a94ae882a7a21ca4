"""The handle layer the mixed-matrix families share: examples 06 (`pgx_gc_*`), 02 (`pgx_sg_*`), 05 (`pgx_qvi_*`),
08 (`pgx_ic_*`), 04 (`pgx_mp_*`), 03 (`pgx_fr_*`), 07 (`pgx_ev_*`), 09 (`pgx_ek_*`) and 10 (`pgx_ma_*`, which has no previous iterate and no alpha).  Each family exports the same entry points under its own prefix, all of them forwards to the shared driver
(csrc/pgx_mixed.hip).  A subclass names its prefix in `_prefix`; its constructor creates `self._h` and sets `_lib`, `_opts`,
`solver` and `ndofs` (and `_flags` where its options take `snes_error_if_not_converged`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .problem import ConvergenceError


def _vec(x):
    return _lib.dptr(np.ascontiguousarray(x, dtype=np.float64))


class _MixedHandle:
    _prefix = ""  # "pgx_gc", "pgx_sg", "pgx_qvi", "pgx_ic", "pgx_mp", "pgx_fr", "pgx_ev" or "pgx_ek"
    _flags: dict = {}  # {"snes_error_if_not_converged": bool}: solve() raises ConvergenceError only where it is set
    alpha = 1.0  # the value last given to set_alpha (the library's initial value)

    def _fn(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _check(self, rc, what):
        if rc:
            msg = self._fn("last_error")(self._h)
            raise _lib.PgxError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def _call(self, name, *args):
        self._check(self._fn(name)(self._h, *args), f"{self._prefix}_{name}")

    def _scalar(self, name):
        out = C.c_double(0)
        self._call(name, C.byref(out))
        return out.value

    # -- state -------------------------------------------------------------------------------------------------
    def get_state(self):
        x = np.empty(self.ndofs)
        self._call("get_state", _lib.dptr(x))
        return x

    def set_state(self, x):
        self._call("set_state", _vec(x))

    def get_prev(self):
        x = np.empty(self.ndofs)
        self._call("get_prev", _lib.dptr(x))
        return x

    def set_prev(self, x):
        self._call("set_prev", _vec(x))

    def advance_prev(self):
        """previous iterate <- current state, on the device"""
        self._call("advance_prev")

    def set_alpha(self, a):
        self.alpha = float(a)
        self._call("set_alpha", self.alpha)

    # -- the call the scripts make once per proximal step ------------------------------------------------------------
    def solve(self):
        reason, its, lin = C.c_int(0), C.c_int(0), C.c_int(0)
        self._call("newton_solve", C.byref(self._opts), C.byref(reason), C.byref(its), C.byref(lin))
        s = self.solver
        s._reason, s._its = reason.value, its.value
        s.ksp._its, s.ksp._reason = lin.value, (-3 if reason.value == -3 else 4)
        if reason.value <= 0 and self._flags.get("snes_error_if_not_converged"):
            raise ConvergenceError(f"SNES did not converge: reason {reason.value} after {its.value} iterations")
        return reason.value, its.value

    # -- fine-grained probes (tests) -----------------------------------------------------------------------------------
    def residual(self, x=None):
        out = np.empty(self.ndofs)
        nrm = C.c_double(0)
        self._call("residual", None if x is None else _vec(x), _lib.dptr(out), C.byref(nrm))
        return out, nrm.value

    def jacobian(self, x=None):
        import scipy.sparse as sp

        self._call("jacobian_fill", None if x is None else _vec(x))
        nr, nnz = C.c_int64(0), C.c_int64(0)
        self._call("csr_export", C.byref(nr), C.byref(nnz), None, None, None)
        rp, col, val = np.empty(nr.value + 1, np.int32), np.empty(nnz.value, np.int32), np.empty(nnz.value)
        self._call("csr_export", None, None, _lib.iptr(rp), _lib.iptr(col), _lib.dptr(val))
        return sp.csr_matrix((val, col, rp), shape=(nr.value, nr.value))

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._call("spmv", _lib.dptr(x), _lib.dptr(y))
        return y

    def profile(self, enable=True):
        ms = (C.c_double * 6)()
        self._call("profile", int(enable), ms)
        return dict(zip(("residual", "jacobian", "lu_factor", "lu_solve", "spmv", "newton_total"), ms))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
