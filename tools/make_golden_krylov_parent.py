#!/usr/bin/env python3
"""Records the golden of tests/test_gpu_krylov_parent.py: every case of that test, solved twice with the library given.

    PGX_LIB=<libpgx.so built from the parent commit by the same toolchain> python3 tools/make_golden_krylov_parent.py <parent commit id> [outdir]

The cases and the solve helper are the test module's own (imported, not copied).  A case whose two runs differ in the final iterate
is recorded with its counts only ("reproducible": false); one whose counts differ, or a structured P1 case that does not reproduce, is
an error.  Writes krylov_driver_parent.json into outdir (default tests/golden).  Needs an MI355X."""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import test_gpu_krylov_parent as T  # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "the full id of the commit the library was built from"
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else T.GOLDEN
    out.mkdir(parents=True, exist_ok=True)
    cases = {}
    for case in T.CASES:
        a, b = T.solve(case, keep=False), T.solve(case, keep=False)
        assert (a["newton"], a["linear"], a["stopped"]) == (b["newton"], b["linear"], b["stopped"]), (case, a, b)
        same = a["sha256"] == b["sha256"]
        assert same or case not in T.MUST_REPRODUCE, (case, a, b)
        cases[case] = dict(a, sha256=a["sha256"] if same else None, reproducible=same)
        print(f"{case}: Newton {a['newton']}, linear {a['linear']}, stopped: {a['stopped']}, reproducible: {same}", flush=True)
    (out / T.RECORD.name).write_text(json.dumps({"parent_commit": commit, "cases": cases}, indent=1) + "\n")
    print(f"wrote {len(cases)} cases to {out / T.RECORD.name}")


if __name__ == "__main__":
    main()
