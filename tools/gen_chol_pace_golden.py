"""Record value and gradient of the one-launch Cholesky path at the shapes of tests/test_gpu_chol_pace.py.

Needs the GPU.  Run it with the library of the commit whose bits are to be kept (ACCBPG_HIP_LIB selects a build of
another commit than the tree's):
    ACCBPG_HIP_LIB=/path/to/parent/libaccbpg_hip.so python tools/gen_chol_pace_golden.py [out.npz]
The file holds, per shape, the seeds, f(x) from a value-only evaluation (no inverse blocks), and f and g from
func_grad(x, 2); tests/golden/chol_pace_parent.npz was written this way from the commit before the chain's panel solve
was rescheduled."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd import _lib  # noqa: E402

SHAPES = [130, 192, 200, 256, 320, 333]


def instance(m):
    """V and x as test_tile_cholesky_matches_step_kernels draws them (first trial)."""
    n = m + 200 + (m % 7)
    seed_v, seed_x = 40 + m % 13, m
    np.random.seed(seed_v)
    V = np.random.randn(m, n)
    rng = np.random.RandomState(seed_x)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    return n, seed_v, seed_x, V, x


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chol_pace_parent.npz")
    lib = _lib.load()
    rec = {"m": np.array(SHAPES, dtype=np.int64)}
    for m in SHAPES:
        n, seed_v, seed_x, V, x = instance(m)
        f = acc.DOptimalObj(V)
        lib.accbpg_dopt_value_reuse(f._h, 0)                # every evaluation runs its factorisation
        fv = f(x)
        fg, g = f.func_grad(x, 2)
        rec["n_%d" % m] = np.int64(n)
        rec["seed_v_%d" % m] = np.int64(seed_v)
        rec["seed_x_%d" % m] = np.int64(seed_x)
        rec["f_value_%d" % m] = np.float64(fv)
        rec["f_%d" % m] = np.float64(fg)
        rec["g_%d" % m] = np.asarray(g, dtype=np.float64)
        print("m=%d n=%d f=%r (value-only %r)" % (m, n, fg, fv))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
