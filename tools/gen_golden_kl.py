"""Generate tests/golden/kl.npz by running the real reference (KL-divergence nonnegative regression with the
Shannon-entropy kernels, ipynb/ex_KL_regr_L1.ipynb).

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference
package is imported read-only through oracle/gen_golden.load_reference and called on seeded inputs; only numbers
are written.  A is not stored: the tests rebuild it with the legacy NumPy RNG call sequence of the factory
(accbpg/applications.py:197-203) and compare the checksum.

Usage:  python tools/gen_golden_kl.py        (about a minute)
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.gen_golden import load_reference, save  # noqa: E402

SIZES = [("s1", 1000, 100), ("s2", 100, 1000)]
ARGS = dict(noise=0.01, lamdaL1=0.001, normalizeA=True, randseed=1)
NTRAJ = 2000
NROWS = 5000
ROWS = [0, 1000, 2000, 3000, 4000]


def calls(accbpg, f, h, L, x0, maxitrs):
    """The six solver calls of ex_KL_regr_L1.ipynb cells 3 and 5: name -> (x, F, G or Ls)."""
    out = {}
    x, F, G, _ = accbpg.BPG(f, h, L, x0, maxitrs=maxitrs, linesearch=False, verbose=False)
    out["bpg"] = (x, F, G)
    x, F, G, _ = accbpg.BPG(f, h, L, x0, maxitrs=maxitrs, linesearch=True, ls_ratio=1.2, verbose=False)
    out["bpgls"] = (x, F, G)
    x, F, G, _ = accbpg.ABPG(f, h, L, x0, gamma=2.0, maxitrs=maxitrs, theta_eq=True, restart=False, verbose=False)
    out["abpg"] = (x, F, G)
    x, F, G, _ = accbpg.ABPG(f, h, L, x0, gamma=2.0, maxitrs=maxitrs, theta_eq=True, restart=True, verbose=False)
    out["abpgrs"] = (x, F, G)
    x, F, G, _, _, _ = accbpg.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=maxitrs, G0=0.1, theta_eq=True,
                                        restart=False, verbose=False)
    out["gain"] = (x, F, G)
    x, F, G, _, _, _ = accbpg.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=maxitrs, G0=0.1, theta_eq=True,
                                        restart=True, restart_rule='f', verbose=False)
    out["gainrs"] = (x, F, G)
    return out


def main():
    accbpg = load_reference()
    out = {}
    for tag, m, n in SIZES:
        f, h, L, x0 = accbpg.KL_nonneg_regr(m, n, **ARGS)
        out[tag + "_cfg"] = np.array([m, n, ARGS["noise"], ARGS["lamdaL1"], ARGS["randseed"]])
        out[tag + "_A_checksum"] = np.array([f.A.sum(), np.abs(f.A).max(), (f.A ** 2).sum()])
        out[tag + "_b"] = f.b
        out[tag + "_L"] = L
        out[tag + "_x0"] = x0
        rng = np.random.RandomState(78)
        x = rng.rand(n) + 0.01
        y = rng.rand(n) + 0.01
        xz, yz = x.copy(), y.copy()
        xz[::7] = 0.0                     # exact zeros in x (the delta path), some where y is zero too
        yz[::5] = 0.0
        fx, g = f.func_grad(x, 2)
        out.update({tag + "_x": x, tag + "_y": y, tag + "_xz": xz, tag + "_yz": yz, tag + "_f": fx, tag + "_g": g,
                    tag + "_f0": f(x0), tag + "_g0": f.gradient(x0), tag + "_psi": h.extra_Psi(x)})
        kernels = {"sh": accbpg.ShannonEntropy(), "l1": accbpg.ShannonEntropyL1(ARGS["lamdaL1"]),
                   "sx": accbpg.ShannonEntropySimplex()}
        for kname, hk in kernels.items():
            for idx, Lc in enumerate([L, 0.37 * L, 5.0]):
                out["%s_%s_prox%d" % (tag, kname, idx)] = hk.prox_map(g, Lc)
                out["%s_%s_divprox%d" % (tag, kname, idx)] = hk.div_prox_map(y, g, Lc)
            out["%s_%s_div_xy" % (tag, kname)] = hk.divergence(x, y)
            out["%s_%s_div_zero" % (tag, kname)] = hk.divergence(xz, yz)
        out[tag + "_prox_L"] = np.array([L, 0.37 * L, 5.0])
        for name, (xs, F, G) in calls(accbpg, f, h, L, x0, NTRAJ).items():
            out.update({"%s_%s_x" % (tag, name): xs, "%s_%s_F" % (tag, name): F, "%s_%s_G" % (tag, name): G})
        for name, (xs, F, G) in calls(accbpg, f, h, L, x0, NROWS).items():
            out["%s_%s_rows" % (tag, name)] = np.array([F[k] if k < len(F) else np.nan for k in ROWS])
            out["%s_%s_len" % (tag, name)] = len(F)
    save("kl", **out)


if __name__ == "__main__":
    main()
