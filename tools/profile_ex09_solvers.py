"""Example 09, dense against banded LU in ONE session: a warm-up solve, then `--linear-solver dense` and `banded` alternating, twice each,
timed with the handle's device events (pgx_ek_profile), and one run of a strip the dense LU cannot take.  Writes the JSON that
DESIGN.md section 12h quotes.

    python tools/profile_ex09_solvers.py [--out profiles/ex09_nu64_nv8_banded.json] [--big 200 13]
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from proximalgalerkin_amd.eikonal import solve_problem  # noqa: E402


def run(solver, nu, nv):
    prof = {}
    t0 = time.perf_counter()
    fields, log = solve_problem(nu=nu, nv=nv, profile=prof, linear_solver=solver)
    wall = time.perf_counter() - t0
    steps = int(log[:, 2].sum())
    ms = {k: v for k, v in prof.items() if k not in ("lu", "band")}
    n = prof["lu"]["n"]
    out = dict(linear_solver=solver, unknowns=n, lvpp_iterations=len(log), newton_iterations=steps, wall_s=wall, ms=ms,
               lu_factor_ms_per_newton_step=ms["lu_factor"] / steps, lu_factor_share_of_newton=ms["lu_factor"] / ms["newton_total"],
               lu=prof["lu"], max_u=float(fields["u"].max()))
    if solver == "banded":
        b = prof["band"]
        out["band"] = b
        flops = 2.0 * b["n"] * b["kl"] * (b["kl"] + b["ku"])  # per factorisation, one per Newton step
    else:
        flops = 2.0 * n ** 3 / 3.0
    out["lu_factor_flops_each"] = flops
    out["lu_factor_gflops"] = flops * steps / (ms["lu_factor"] * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=64)
    ap.add_argument("--nv", type=int, default=8)
    ap.add_argument("--big", type=int, nargs=2, default=[200, 13], help="a strip for the banded solver alone (0 0: none)")
    ap.add_argument("--out", type=pathlib.Path, default=None)
    a = ap.parse_args()
    run("banded", 8, 2)  # warm-up: library load, first launches
    runs = [run(s, a.nu, a.nv) for s in ("dense", "banded", "dense", "banded")]
    best = {s: min((r for r in runs if r["linear_solver"] == s), key=lambda r: r["ms"]["newton_total"]) for s in ("dense", "banded")}
    out = dict(nu=a.nu, nv=a.nv, runs=runs,
               factor_speedup=best["dense"]["ms"]["lu_factor"] / best["banded"]["ms"]["lu_factor"],
               solve_speedup=best["dense"]["ms"]["lu_solve"] / best["banded"]["ms"]["lu_solve"],
               newton_speedup=best["dense"]["ms"]["newton_total"] / best["banded"]["ms"]["newton_total"])
    if a.big[0] > 0:
        out["big"] = dict(nu=a.big[0], nv=a.big[1], **run("banded", *a.big))
    text = json.dumps(out, indent=1) + "\n"
    path = a.out or ROOT / "profiles" / f"ex09_nu{a.nu}_nv{a.nv}_banded.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(text)
    for r in runs + ([out["big"]] if "big" in out else []):
        print(f"{r['linear_solver']:7s} n={r['unknowns']} newton {r['newton_iterations']} factor {r['ms']['lu_factor']:.1f} ms solve {r['ms']['lu_solve']:.1f} ms "
              f"total {r['ms']['newton_total']:.1f} ms, {r['lu_factor_gflops']:.1f} GF/s, max u {r['max_u']:.6f}")
    print(f"factor x{out['factor_speedup']:.1f} solve x{out['solve_speedup']:.2f} newton x{out['newton_speedup']:.1f} -> {path}")


if __name__ == "__main__":
    main()
