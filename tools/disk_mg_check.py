#!/usr/bin/env python3
"""Example 01 on the reference's disk family with the multilevel cycle of refined general meshes.

    python3 tools/disk_mg_check.py [--levels 3 4 5 6] [--modes mg single lu] [--trace-level 5] [--out profiles/umg_disk_scaling.json]
    python3 tools/disk_mg_check.py --degree 2 [--levels 3 4 5] [--modes mg lu auto]          (-> profiles/p2_umg_disk_scaling.json)
    python3 tools/disk_mg_check.py --built [--levels 3 4] [--build {host,device}]             (-> profiles/amg_disk_scaling.json)

For every L: create_disk(0.1, refinements=L) - the construction of generate_mesh_gmsh.py's disk_L - solved with settings B
(double_exponential, alpha_max 100, tol 1e-4) under "pgx_mg" (the cycle), "pgx_mg" with PGX_UMG=0 (the single-level smoother) and
"pgx_lu".  Recorded: vertices per level, Newton counts, Krylov iterations per Newton step (read from the solver's monitor lines in a
second, untimed run), and per LVPP solve the host clock around pgx_newton_solve (which ends in a synchronisation).  What the times
include: the first solve of a handle carries its one-time work - under "pgx_lu" the symbolic analysis of the factorisation - so the
mean over all solves, the first solve and the mean without it are recorded separately; the cycle's one-time host pass
(pgx_set_hierarchy) runs when the handle is created and is recorded as set_hierarchy_seconds.  Each mode is run once untimed on
the first mesh before anything is timed (code objects loaded); one timed run per entry, so no spread.  --trace-level L runs the "mg" solve of that L once more under rocprofv3 --kernel-trace
and adds the per-launch times of the k_umg_* kernels per grid size, with the achieved bandwidth of k_umg_rap and
k_umg_resid_restrict on the finest transfer against their algorithmic bytes.  A mode that fails (the single-level smoother runs into
the Krylov iteration cap on the large meshes) is recorded with its message.  Needs an MI355X.

--degree 2: the same family at degree 2 (obstacle_pg.py -p 2).  "mg" is the two-level patch cycle over the hierarchy, "lu" the sparse
LU, "auto" pc_type auto forced onto the cycle at every size (PGX_UMG_MIN_P2=0): the cycle first, the sparse LU for a Newton solve in
which it stagnates.  Recorded in addition: create_seconds (the handle, pgx_set_hierarchy included), fallbacks (Newton solves rescued
by the LU) and nw (wide stars).  setup_and_solve_seconds - handle creation plus every solve, rescues included - of "auto" against
"lu" is what PGX_UMG_MIN_P2's default is taken from.

--built: the hierarchy built from the matrix (pgx_build_hierarchy) on meshes that carry none.  Per L three meshes: "attached" - the
refined disk with its hierarchy, the comparator; "renumbered" - the same mesh with its vertices renumbered by a fixed random permutation
and the hierarchy stripped; "unrefined" - create_disk(h / 2^L), a mesh of about as many vertices that no refinement produced.  The last
two run "built" ("pgx_mg"; the constructor builds the hierarchy, PGX_UMG_BUILD_MIN=0) and "lu".  Recorded in addition:
build_hierarchy_seconds = (host pass, device work and copies) of pgx_build_hierarchy and the vertices per built level.  Each mode
is warmed by ONE untimed run on the first mesh it meets (code objects loaded), not once per mesh; one timed run per entry.  The section
"twin" of the output file is kept as it is (CPU figures of tests/amg_reference.py).  --build host / device pins the pass that computes
the split and the patterns (tuning key PGX_AMG_BUILD = 0 / 1; without the option no key is set and the library's default, the device
pass, runs) and files the results under "build_host" / "build_device" instead of "device", so that two runs into one --out file
(profiles/amg_device_build.json) hold both passes side by side; build_pass and split_launches (pgx_amg_build_info) are recorded
either way."""
import argparse
import contextlib
import csv
import ctypes
import glob
import json
import os
import pathlib
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
BASE = {"ksp_type": "preonly", "ksp_error_if_not_converged": True, "snes_error_if_not_converged": True, "snes_linesearch_type": "none",
        "snes_rtol": 1e-6, "snes_max_it": 100}
MODES = {"built": ("pgx_mg", {"PGX_UMG_BUILD_MIN": 0}), "mg": ("pgx_mg", {}), "single": ("pgx_mg", {"PGX_UMG": 0}), "lu": ("pgx_lu", {}), "auto": ("lu", {"PGX_UMG_MIN_P2": 0})}


@contextlib.contextmanager
def c_stdout_to(path):
    """The library prints its monitor lines with printf: redirect file descriptor 1."""
    sys.stdout.flush()
    libc = ctypes.CDLL(None)
    saved = os.dup(1)
    with open(path, "w") as f:
        os.dup2(f.fileno(), 1)
        try:
            yield
        finally:
            libc.fflush(None)
            os.dup2(saved, 1)
            os.close(saved)


def solve(msh, mode, monitor_file=None, degree=1):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    from proximalgalerkin_amd.problem import NonlinearProblem

    pc, keys = MODES[mode]
    for k, v in keys.items():
        _lib.tuning_set(k, v)
    hier_s, set_hierarchy = [], NonlinearProblem.set_hierarchy

    def timed_set_hierarchy(self, *args, **kw):  # pgx_set_hierarchy returns after a synchronisation
        t0 = time.perf_counter()
        r = set_hierarchy(self, *args, **kw)
        hier_s.append(time.perf_counter() - t0)
        return r

    NonlinearProblem.set_hierarchy = timed_set_hierarchy
    try:
        opts = dict(BASE, pc_type=pc)
        if monitor_file:
            opts["snes_monitor"] = None
        t_create = time.perf_counter()
        problem, sol, sol_k, alpha = setup_problem(msh, degree, petsc_options=opts)
        t_create = time.perf_counter() - t_create
        extra = {}
        if getattr(problem, "build_seconds", None):  # the constructor built the hierarchy (pgx_build_hierarchy)
            info = problem.build_info()
            extra = dict(build_hierarchy_seconds=[round(v, 4) for v in problem.build_seconds], build_pass=info["mode"],
                         split_launches=info["split_launches"])
        try:
            lin, ms, inner = [], [], problem.solve

            def counted():
                t0 = time.perf_counter()
                r = inner()  # pgx_newton_solve returns after a synchronisation of its stream
                ms.append(1e3 * (time.perf_counter() - t0))
                lin.append(problem.solver.getLinearSolveIterations())
                return r

            problem.solve = counted
            with (c_stdout_to(monitor_file) if monitor_file else contextlib.nullcontext()):
                hist = run_outer_loop(problem, sol, sol_k, alpha, 500, "double_exponential", 1e2, 1e-4)
            u = sol.x.array[: sol.function_space.block_size].copy()
            if "build_hierarchy_seconds" in extra:
                problem.assemble_jacobian()
                extra["built_levels"] = [problem.umg_level_export(l)["n"] for l in range(problem.umg_levels())]
            if degree == 2:
                problem.assemble_jacobian()
                extra.update(fallbacks=problem.p2_cycle_info()["fallbacks"], nw=int(len(problem.p2_wide_export()[0])))
        finally:
            problem.close()
    finally:
        NonlinearProblem.set_hierarchy = set_hierarchy
        for k in keys:
            _lib.tuning_set(k, None)
    rec = dict(newton=[int(v) for v in hist["Newton steps"]], krylov_per_lvpp_solve=lin, ms_per_lvpp_solve=[round(v, 3) for v in ms],
               ms_per_lvpp_solve_mean=round(float(np.mean(ms)), 3), ms_first_solve=round(ms[0], 3),
               ms_per_lvpp_solve_mean_without_first=round(float(np.mean(ms[1:])), 3) if len(ms) > 1 else None,
               ms_total=round(float(np.sum(ms)), 3), set_hierarchy_seconds=round(hier_s[0], 4) if hier_s else None,
               create_seconds=round(t_create, 3), **extra)
    if monitor_file:
        steps = [int(m) for m in re.findall(r"KSP its (\d+)", pathlib.Path(monitor_file).read_text())]
        rec = dict(krylov_per_newton_step=steps, krylov_per_newton_step_range=[min(steps), max(steps)] if steps else None)
    return rec, u


def transfer_bytes(parents, rowptr, col):
    """Algorithmic bytes of one k_umg_rap launch and one k_umg_resid_restrict launch on the transfer `parents` from the level with
    the pattern (rowptr, col): every operand once."""
    nf = len(parents)
    nc = int(np.count_nonzero(parents[:, 0] == parents[:, 1]))
    npar = np.where(np.arange(nf) < nc, 1, 2)
    rows = np.repeat(np.arange(nf), np.diff(rowptr))
    plan = int(np.sum(npar[rows] * npar[col]))
    import scipy.sparse as sp

    P = sp.csr_matrix((np.ones(2 * nf), (np.repeat(np.arange(nf), 2), parents.ravel())), shape=(nf, nc))
    A = sp.csr_matrix((np.ones(len(col)), col, rowptr), shape=(nf, nf))
    nnz_c = int((P.T @ A @ P).nnz)
    rap = 4 * plan + 4 * (nnz_c + 1) + 8 * len(col) + 8 * nnz_c
    children = nc + 2 * (nf - nc)
    restrict = 16 * nf + 4 * children + 4 * (nc + 1) + nc + 16 * nc
    return dict(n_fine=nf, n_coarse=nc, nnz_fine=int(len(col)), nnz_coarse=nnz_c, plan_items=plan, plan_row_mean=round(plan / nnz_c, 2),
                rap_bytes=rap, resid_restrict_bytes=restrict)


def kernel_times(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f, newline="")):
            name = r["Kernel_Name"]
            if "k_umg_" not in name and "k_bspmv" not in name:
                continue
            short = re.sub(r"^void ", "", name.split("(")[0])
            acc.setdefault((short, int(r.get("Grid_Size", r.get("Grid_Size_X", 0)))), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [dict(kernel=k, grid=g, launches=len(v), us_mean=round(float(np.mean(v)), 2), us_min=round(float(np.min(v)), 2),
                 us_max=round(float(np.max(v)), 2)) for (k, g), v in sorted(acc.items(), key=lambda kv: (kv[0][0], -kv[0][1]))]


def main_built(a):
    from proximalgalerkin_amd import fem
    from tests.amg_reference import permuted as renumbered  # fixed random permutation of the vertex numbers, hierarchy stripped

    path = pathlib.Path(a.out or str(ROOT / "profiles" / "amg_disk_scaling.json"))
    out = json.loads(path.read_text()) if path.exists() else {}
    out.update(h=a.h, settings="B: double_exponential, alpha_max 100, tol 1e-4; V(6,6), omega 0.75, 60 coarse sweeps; one timed run per entry; "
               "each mode is run once untimed on the first mesh it meets, not once per mesh, so a first-solve figure still carries what is "
               "first-use per mesh size")
    section = "device" if a.build is None else f"build_{a.build}"
    out[section] = {}
    if a.build is not None:
        MODES["built"] = ("pgx_mg", dict(MODES["built"][1], PGX_AMG_BUILD=1 if a.build == "device" else 0))
    warm = set()
    for L in a.levels:
        refined = fem.create_disk(a.h, refinements=L)
        meshes = {"attached": (refined, ["mg"]), "renumbered": (renumbered(refined), ["built", "lu"]),
                  "unrefined": (fem.create_disk(a.h / 2 ** L), ["built", "lu"])}
        rec = {}
        for tag, (msh, modes) in meshes.items():
            rec[tag] = dict(vertices=int(msh.num_vertices))
            u_ref = {}
            for mode in modes:
                if mode == "lu" and L > a.lu_max_level:
                    rec[tag][mode] = "not run at this size"
                    continue
                try:
                    if mode not in warm:
                        solve(msh, mode)
                        warm.add(mode)
                    t0 = time.perf_counter()
                    r, u_ref[mode] = solve(msh, mode)
                    r["setup_and_solve_seconds"] = round(time.perf_counter() - t0, 2)
                    if mode != "lu":
                        with tempfile.TemporaryDirectory() as tmp:
                            r.update(solve(msh, mode, os.path.join(tmp, "monitor.txt"))[0])
                        r["krylov_per_newton_step_mean"] = round(float(np.mean(r["krylov_per_newton_step"])), 2)
                    rec[tag][mode] = r
                    print(f"L={L} {tag} {msh.num_vertices} {mode}: Newton {r['newton']}, Krylov per Newton step mean {r.get('krylov_per_newton_step_mean')}, "
                          f"ms per LVPP solve without the first {r['ms_per_lvpp_solve_mean_without_first']}, build {r.get('build_hierarchy_seconds')} s, "
                          f"levels {r.get('built_levels')}, {r.get('build_pass')} pass, split launches {r.get('split_launches')}, "
                          f"creation plus all solves {r['setup_and_solve_seconds']} s", flush=True)
                except Exception as e:
                    rec[tag][mode] = f"failed: {type(e).__name__}: {e}"
                    print(f"L={L} {tag} {mode}: {rec[tag][mode]}", flush=True)
            if "lu" in u_ref and "built" in u_ref:
                rec[tag]["rel_l2_u_built_vs_lu"] = float(np.linalg.norm(u_ref["built"] - u_ref["lu"]) / np.linalg.norm(u_ref["lu"]))
        out[section][str(L)] = rec
        path.write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--built", action="store_true", help="meshes without a hierarchy: the hierarchy built from the matrix (-> profiles/amg_disk_scaling.json)")
    ap.add_argument("--build", choices=["host", "device"], default=None,
                    help="with --built: the pass of pgx_build_hierarchy (PGX_AMG_BUILD); results under build_host / build_device")
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 4, 5, 6])
    ap.add_argument("--degree", type=int, default=1, choices=[1, 2])
    ap.add_argument("--modes", nargs="+", default=None, choices=sorted(MODES), help="default: mg single lu; degree 2: mg lu auto")
    ap.add_argument("--h", type=float, default=0.1)
    ap.add_argument("--lu-max-level", type=int, default=5, help="largest L solved under pgx_lu")
    ap.add_argument("--single-max-level", type=int, default=5, help="largest L solved with the single-level smoother")
    ap.add_argument("--trace-level", type=int, default=None)
    ap.add_argument("--trace-timeout", type=float, default=300.0, help="seconds the traced child process may take")
    ap.add_argument("--out", default=None, help="default: profiles/umg_disk_scaling.json; degree 2: profiles/p2_umg_disk_scaling.json")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.built:
        if a.degree != 1 or a.trace_level is not None:
            ap.error("--built runs degree 1 without a kernel trace")
        return main_built(a)
    if a.build is not None:
        ap.error("--build goes with --built")
    a.modes = a.modes or (["mg", "single", "lu"] if a.degree == 1 else ["mg", "lu", "auto"])
    a.out = a.out or str(ROOT / "profiles" / ("umg_disk_scaling.json" if a.degree == 1 else "p2_umg_disk_scaling.json"))
    if a.degree == 2 and (a.trace_level is not None or "single" in a.modes):
        ap.error("--degree 2 has the modes mg, lu, auto and no kernel trace")
    from proximalgalerkin_amd import fem

    if a.child:  # under rocprofv3: one "mg" run of one mesh, nothing else
        solve(fem.create_disk(a.h, refinements=a.levels[0]), "mg")
        return
    out = dict(h=a.h, degree=a.degree, settings="B: double_exponential, alpha_max 100, tol 1e-4; V(6,6), omega 0.75, 60 coarse sweeps", levels={})
    warm = set()
    for L in a.levels:
        t0 = time.perf_counter()
        msh = fem.create_disk(a.h, refinements=L)
        sizes = [len(p) for p in msh.hierarchy] + [int(np.count_nonzero(msh.hierarchy[-1][:, 0] == msh.hierarchy[-1][:, 1]))]
        rec = dict(vertices=sizes, mesh_seconds=round(time.perf_counter() - t0, 2))
        print(f"L={L}: vertices {sizes}", flush=True)
        u_ref = {}
        for mode in a.modes:
            if (mode == "lu" and L > a.lu_max_level) or (mode == "single" and L > a.single_max_level):
                rec[mode] = "not run at this size"
                continue
            try:
                if mode not in warm:  # once per process and mode: code objects, first-use allocations
                    solve(msh, mode, degree=a.degree)
                    warm.add(mode)
                t0 = time.perf_counter()
                r, u = solve(msh, mode, degree=a.degree)
                r["setup_and_solve_seconds"] = round(time.perf_counter() - t0, 2)
                u_ref[mode] = u
                if mode != "lu":
                    with tempfile.TemporaryDirectory() as tmp:
                        r.update(solve(msh, mode, os.path.join(tmp, "monitor.txt"), degree=a.degree)[0])
                rec[mode] = r
                print(f"  {mode}: Newton {r['newton']}, Krylov per Newton step {r.get('krylov_per_newton_step_range')}, "
                      f"ms per LVPP solve: mean {r['ms_per_lvpp_solve_mean']}, first {r['ms_first_solve']}, without the first "
                      f"{r['ms_per_lvpp_solve_mean_without_first']}; set_hierarchy {r['set_hierarchy_seconds']} s", flush=True)
            except Exception as e:  # e.g. the single-level smoother at the Krylov iteration cap
                rec[mode] = f"failed: {type(e).__name__}: {e}"
                print(f"  {mode}: {rec[mode]}", flush=True)
        if "lu" in u_ref:
            for mode in ("mg", "single", "auto"):
                if mode in u_ref:
                    rec[f"rel_l2_u_{mode}_vs_lu"] = float(np.linalg.norm(u_ref[mode] - u_ref["lu"]) / np.linalg.norm(u_ref["lu"]))
        out["levels"][str(L)] = rec
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")  # after every size: a later failure keeps what was measured
    if a.trace_level is not None:
        L = a.trace_level
        msh = fem.create_disk(a.h, refinements=L)
        from proximalgalerkin_amd.obstacle import setup_problem

        problem = setup_problem(msh, 1)[0]
        rowptr, col = problem.export_blocks(with_D=False)[:2]
        problem.close()
        tb = transfer_bytes(msh.hierarchy[0], rowptr, col)
        with tempfile.TemporaryDirectory() as tmp:
            child = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, __file__,
                                    "--child", "--levels", str(L), "--h", str(a.h)], timeout=a.trace_timeout, stdout=subprocess.DEVNULL,
                                   stderr=subprocess.PIPE, text=True)  # a child that hangs ends here, and the script with it
            if child.returncode:
                sys.exit(f"the traced run ended with status {child.returncode}:\n{child.stderr[-2000:]}")
            kt = kernel_times(tmp)
        for k in kt:
            # the launches of the finest transfer, by their grid (threads or blocks; k_umg_rap runs 1, 4 or 8 lanes per coarse entry)
            blocks = {"k_umg_rap": [-(-tb["nnz_coarse"] * lanes // 256) for lanes in (1, 4, 8)], "k_umg_resid_restrict": [-(-tb["n_coarse"] // 256)]}
            for name, by in (("k_umg_rap", tb["rap_bytes"]), ("k_umg_resid_restrict", tb["resid_restrict_bytes"])):
                if k["kernel"].startswith(name) and any(k["grid"] in (b * 256, b) for b in blocks[name]):
                    k["algorithmic_bytes"] = by
                    k["gb_per_s_mean"] = round(by / k["us_mean"] / 1e3, 1)
        out["kernel_trace"] = dict(level=L, finest_transfer=tb, kernels=kt)
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
        for k in kt:
            print(k, flush=True)


if __name__ == "__main__":
    main()
