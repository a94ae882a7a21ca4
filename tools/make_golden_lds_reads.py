#!/usr/bin/env python3
"""Records the goldens of tests/test_gpu_mg32_lds_reads.py: one V-cycle per grid, launch form, level and right-hand side of that test.

    PGX_LIB=<libpgx.so of the commit the test compares against> python3 tools/make_golden_lds_reads.py [outdir [what that library is]]

The cases, the state and the right-hand sides are the test module's own (imported, not copied).  Writes
mg32_lds_reads_parent_n200x72.npz (the main form's outputs in full; as float32 where that is lossless - the single-precision cycle
returns floats) and mg32_lds_reads_parent_sha256.json into outdir (default tests/golden).  Needs an MI355X."""
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import test_gpu_mg32_lds_reads as T  # noqa: E402


def main():
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
    out.mkdir(parents=True, exist_ok=True)
    sha, full = {}, {}
    for cells in T.GRIDS:
        for form in T.FORMS:
            for (level, name), z in T.run_case(cells, form).items():
                sha[T.case_id(cells, form, level, name)] = T.digest(z)
                if cells == T.GRIDS[0] and form == T.MAIN:
                    z32 = z.astype(np.float32)
                    full[f"level{level}_{name}"] = z32 if np.array_equal(z32.astype(np.float64), z) else z
            print(f"{cells} {form}: recorded", flush=True)
    np.savez_compressed(out / T.FULL.name, **full)
    (out / T.SHA.name).write_text(json.dumps({"library": sys.argv[2] if len(sys.argv) > 2 else "not stated", "sha256": sha}, indent=1) + "\n")
    print(f"wrote {len(sha)} digests and {len(full)} full outputs ({(out / T.FULL.name).stat().st_size} bytes) to {out}")


if __name__ == "__main__":
    main()
