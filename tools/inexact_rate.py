"""Iterations per second and launches per line-search try of AIBM, AdaptFGM and UniversalGM on Poisson regression
over the simplex, at the drivers' size (2000,1000) and at one size where A no longer fits in cache, in three variants:
the fused kernels (combine_ls_terms, prox_map_acc), the same loops composed from the package's public kernels
(algorithms.FUSED_INEXACT = False), and the NumPy restatement of tests/inexact_numpy.py on the host cores.

Launches are counted, not timed: every C-ABI entry a run makes is tallied and weighted by the kernels it launches at
that n (read off the sources); a try is one evaluation of f alone (flag 0), which each try of each method makes once.

Usage:  python tools/inexact_rate.py --out profiles/inexact_rate.json        (needs the GPU)
"""
import argparse
import json
import os
import sys
import time

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd import _lib, algorithms  # noqa: E402
import inexact_numpy as R  # noqa: E402


def launches_of(name, args, n):
    """kernels launched by one call of a C-ABI entry on a length-n vector"""
    two_stage = 2 if n > 1024 else 1
    if name == "accbpg_combine_ls_terms":
        return two_stage if args[7].value else 1                # x_dev NULL: the elementwise pass alone
    if name == "accbpg_burg_simplex_prox_acc":
        return 1 if n <= 32768 else 2
    if name == "accbpg_poisson_func_grad":
        return 1 if args[2] == 0 else 2
    return {"accbpg_ls_terms": 2, "accbpg_vec_dot_diff": 2, "accbpg_vec_dot": 2, "accbpg_burg_divergence": 2,
            "accbpg_vec_axpby": 1, "accbpg_vec_div_scalar": 1, "accbpg_burg_simplex_div_prox": 1}.get(name, 0)


class Tally:
    """wraps the library's entries with counters for the length of one run"""

    def __init__(self, n):
        self.n, self.launches, self.tries, self.calls = n, 0, 0, 0
        self.lib = _lib.load()
        self.saved = {}

    def __enter__(self):
        for name in _lib.EXPORTS:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def counted(*args, _fn=fn, _name=name):
                k = launches_of(_name, args, self.n)
                self.launches += k
                self.calls += 1 if k else 0
                if _name == "accbpg_poisson_func_grad" and args[2] == 0:
                    self.tries += 1
                return _fn(*args)
            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def device_run(call, fused, n):
    algorithms.FUSED_INEXACT = fused
    try:
        call(3)                                                 # warm-up: allocations, first launches
        torch.cuda.synchronize()
        with Tally(n) as t:
            res = call(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call(None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        algorithms.FUSED_INEXACT = True
    its = len(res[1]) - 1
    return {"it_per_s": round(its / dt, 2), "launches_per_try": round(t.launches / max(t.tries, 1), 2),
            "tries_per_it": round(t.tries / max(its, 1), 2), "F_last": float(res[1][-1])}


def host_run(call, iters):
    t0 = time.perf_counter()
    res = call(iters)
    dt = time.perf_counter() - t0
    return {"it_per_s": round((len(res[1]) - 1) / dt, 3), "F_last": float(res[1][-1])}


def instance(m, n, on_device):
    """Poisson_regr_simplex_acc's instance; at the large size A is drawn on the device (plumbing only)"""
    if not on_device:
        np.random.seed(7)
        f, hs, L, x0 = acc.Poisson_regr_simplex_acc(m, n, noise=0.001)
        return f, hs[0], L, x0, R.PoissonOracle(f.A, f.b)
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=gen)
    A /= A.sum(dim=0)
    np.random.seed(7)
    x0 = acc.random_point_on_simplex(n)
    sol = torch.from_numpy(acc.random_point_on_simplex(n)).cuda()
    b = A @ sol + 0.001 * torch.rand(m, dtype=torch.float64, device="cuda", generator=gen)
    f = acc.PoissonRegression(A, b)
    return f, acc.BurgEntropySimplex(eps=1e-7), float(b.abs().sum()), x0, R.PoissonOracle(A.cpu().numpy(), b.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--large", default="8192x65536")
    ap.add_argument("--large-iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=12)
    ap.add_argument("--large-host-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lm, ln = (int(v) for v in a.large.split("x"))
    rec = {"device": torch.cuda.get_device_name(0), "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
           "sizes": {}}
    for (m, n, iters, hiters, on_dev) in [(2000, 1000, a.iters, a.host_iters, False),
                                          (lm, ln, a.large_iters, a.large_host_iters, True)]:
        f, h, L, x0, fr = instance(m, n, on_dev)
        xd = torch.from_numpy(x0).cuda()
        hr = R.BurgSimplexOracle(eps=1e-7)
        solvers = {
            "AIBM": (lambda k: acc.AIBM(f, h, L, xd, gamma=1.4, maxitrs=k or iters, verbose=False),
                     lambda k: R.AIBM(fr, hr, L, x0, gamma=1.4, maxitrs=k)),
            "AdaptFGM": (lambda k: acc.AdaptFGM(f, h, L, xd, maxitrs=k or iters, verbose=False),
                         lambda k: R.AdaptFGM(fr, hr, L, x0, maxitrs=k)),
            "UniversalGM": (lambda k: acc.UniversalGM(f, h, L, xd, maxitrs=k or iters, verbose=False),
                            lambda k: R.UniversalGM(fr, hr, L, x0, maxitrs=k)),
        }
        out = {}
        for name, (dev_call, host_call) in solvers.items():
            out[name] = {"fused": device_run(dev_call, True, n), "composed": device_run(dev_call, False, n),
                         "numpy_host": host_run(host_call, hiters + 1)}
            out[name]["fused_over_composed"] = round(out[name]["fused"]["it_per_s"] / out[name]["composed"]["it_per_s"], 3)
            print(m, n, name, json.dumps(out[name]), flush=True)
        rec["sizes"]["%dx%d" % (m, n)] = out
        del f, fr
    rec["method"] = ("wall clock of one run of --iters outer iterations after a 3-iteration warm-up, device x0; launches "
                     "tallied per C-ABI entry over a run of the same length; NumPy restatement on the host for "
                     "--host-iters iterations")
    s = json.dumps(rec)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
