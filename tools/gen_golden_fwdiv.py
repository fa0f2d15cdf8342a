"""Generate tests/golden/fwdiv.npz by running the real reference: Frank-Wolfe with the Bregman step and with the
classical step 2/(k+2) on the D-optimal objective with the simplex LMO (frank_wolfe_wtih_rs/ex_Dopt_design.py,
parameters_free_fw/ipynb/ex_Dopt_Full_Adapt_and_descent_step.ipynb).

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference
package is imported read-only through oracle/gen_golden.load_reference and called on seeded inputs; only numbers
are written.  The design matrices are not stored: the tests rebuild them (D_opt_design is seeded, housing is a
committed data file).

Usage:  python tools/gen_golden_fwdiv.py        (a few seconds)
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import REF, load_reference, save  # noqa: E402

ITERS = 600


def main():
    accbpg = load_reference()
    out = {}
    # the classical step on (80,200) seed 10 and on housing
    f, h, L, x0 = accbpg.D_opt_design(80, 200, randseed=10)
    x, F, T, G = accbpg.FW_alg_descent_step(f, h, x0, ITERS, accbpg.lmo_simplex(), verbose=False)
    out.update(r_desc_x=x, r_desc_F=F)
    f, h, L, x0 = accbpg.D_opt_libsvm(os.path.join(REF, "parameters_free_fw", "data", "housing.txt"))
    x, F, T, G = accbpg.FW_alg_descent_step(f, h, x0, ITERS, accbpg.lmo_simplex(), verbose=False)
    out.update(h_desc_x=x, h_desc_F=F)
    # the Bregman step at (64,512) seed 3: another line-search ratio, and no line search
    f, h, L, x0 = accbpg.D_opt_design(64, 512, randseed=3)
    out["s_L"] = L
    x, F, Ls, T = accbpg.FW_alg_div_step(f, h, L, x0, lmo=accbpg.lmo_simplex(), maxitrs=ITERS, gamma=2.0,
                                         ls_ratio=1.5, verbose=False)
    out.update(s_ls15_x=x, s_ls15_F=F, s_ls15_Ls=Ls)
    x, F, Ls, T = accbpg.FW_alg_div_step(f, h, L, x0, lmo=accbpg.lmo_simplex(), maxitrs=ITERS, gamma=2.0,
                                         linesearch=False, verbose=False)
    out.update(s_nols_x=x, s_nols_F=F, s_nols_Ls=Ls)
    save("fwdiv", **out)


if __name__ == "__main__":
    main()
