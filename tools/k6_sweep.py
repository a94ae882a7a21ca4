"""Sweep of the single-precision cycle's six-sweep keys on the headline workload: which levels run a whole smoothing leg as ONE
launch (PGX_F32_K6_MAX: levels of at most that many vertices) times the tile height of those launches (PGX_F32_TY; 0 = by level
size):
python tools/k6_sweep.py [cells]"""
import json
import os
os.environ.setdefault("PGX_TUNING_FROM_ENV", "1")  # PGX_* switches reach the library through the loader's opt-in bridge
import subprocess
import sys

n = sys.argv[1] if len(sys.argv) > 1 else "2048"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# PGX_F32_K6_MAX: no level | 513^2 and below | + 1025^2 | + 2049^2
for k6 in (0, 300000, 1100000, 4300000):
    for ty in (0, 8, 12, 16, 20):
        e = dict(os.environ, PGX_F32_K6_MAX=str(k6), PGX_F32_TY=str(ty))
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--cells", n, "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                           env=e, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if not lines or r.returncode != 0 or "Memory access fault" in r.stderr:
            print(k6, ty, "FAILED", r.stderr[-300:])
            sys.exit(1)  # never run on after a failed GPU step
        d = json.loads(lines[-1])
        print(f"cells {n} PGX_F32_K6_MAX={k6:8d} PGX_F32_TY={ty:2d}: {d['ms_per_step']:8.2f} ms/solve  "
              f"{d['value']:.2f} Newton it/s  newton {d['config']['newton_iterations_per_step']}  "
              f"last lin its {d['last_newton_linear_iterations']}", flush=True)
