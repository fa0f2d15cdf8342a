"""Record f and g of func_grad(x, 2) at the shapes of tests/test_gpu_plan_parity.py: one per upload path of build_plans.

Needs the GPU.  Run it with the library of the commit whose bits are to be kept (ACCBPG_HIP_LIB selects a build of
another commit than the tree's):
    ACCBPG_HIP_LIB=/path/to/parent/libaccbpg_hip.so python tools/gen_plan_parity_golden.py [out.npz]
Per case and instance the file holds f, the SHA-256 of g's bytes and g's first and last 16 entries
(tests/plan_cases.py: parity_record); tests/golden/plan_parity_parent.npz was written this way from the commit before
the launch plans moved into csrc/dopt_plan.hpp."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd import _lib  # noqa: E402
import plan_cases as P  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_parity_parent.npz")
    lib = _lib.load()
    rec = {}
    for case in P.PARITY_CASES:
        results = P.parity_evaluate(acc, lib, case)
        rec.update(P.parity_record(case, results))
        print(P.parity_name(case), [r[0] for r in results])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
