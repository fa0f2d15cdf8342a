"""SymNMF rates: FrobeniusSymLoss.func_grad and value-only evaluation at (400,50), (700,50), (8192,64), (16384,64)
and (16384,128), with the M X product's TFLOP/s and fraction of the 78.6 TFLOP/s fp64 MFMA peak and the NumPy host
time beside each; and Frank-Wolfe iterations per second (FW_alg_div_step with line search, l-infinity ball) on the
notebook instance and at (16384,64), against the NumPy restatement on the host.

Large instances are built directly (M = (A + A^T)/2 on the device), not through the factories, whose host SVD for
sigma is out of reach at these sizes.  GPU times are medians of rounds of back-to-back calls (each call returns a
value or is synchronised), so they include the launch and readback costs.

Usage:  python tools/symnmf_rate.py [--out FILE.json] [--quick]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402
import symnmf_numpy as S  # noqa: E402

PEAK = 78.6


def med_ms(fn, reps, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / reps * 1e3)
    return float(np.median(out))


def host_ms(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def sym(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(n, n, dtype=torch.float64, device="cuda", generator=g)
    M = (A + A.T) * 0.5
    del A
    return M


def evals(n, r, host):
    M = sym(n, n)
    X = torch.rand(n, r, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(r))
    f = acc.FrobeniusSymLoss(M, X)
    reps = 50 if n <= 1000 else 10
    fg = med_ms(lambda: f.func_grad(X, 2), reps, 7)
    v = med_ms(lambda: f.func_grad(X, 0), reps, 7)
    flop = 2.0 * n * n * r
    rec = {"n": n, "r": r, "plan": list(f.plan()), "func_grad_ms": fg, "value_ms": v,
           "func_grad_tflops": flop / (fg * 1e-3) / 1e12, "func_grad_peak_frac": flop / (fg * 1e-3) / 1e12 / PEAK}
    if host:
        Mh, Xh = M.cpu().numpy(), X.cpu().numpy()
        fh = S.FrobeniusSymLoss(Mh, Xh)
        hreps = 10 if n <= 1000 else 2
        rec["host_func_grad_ms"] = host_ms(lambda: fh.func_grad(Xh, 2), hreps)
        rec["host_value_ms"] = host_ms(lambda: fh.func_grad(Xh, 0), hreps)
    del f, M
    torch.cuda.empty_cache()
    return rec


def fw_rate(n, r, iters, host_iters):
    center = np.ones((n, r)) * 500.0
    if n <= 1000:
        np.random.seed(2)
        f, h, L, X0, M = acc.FrobeniusSymLossExLInfBall(n, r, center, radius=500.0, on_boundary=False)
        Mh = M
    else:
        Md = sym(n, 7)
        f = acc.FrobeniusSymLoss(Md, np.zeros((n, r)))
        h = acc.SumOf2nd4thPowers(6, 2.0 * n)          # ||M||_2 of a uniform (0,1) matrix is about n/2
        L, X0 = 1, np.ones((n, r)) * 500.005
        Mh = Md.cpu().numpy() if host_iters else None
    lmo = acc.lmo_linf_ball(500.0, center=center)
    Xd = torch.from_numpy(X0).cuda()
    acc.FW_alg_div_step(f, h, L, Xd, 2, 2.0, lmo, epsilon=1e-300, verbose=False)
    torch.cuda.synchronize()
    t = time.perf_counter()
    x, F, Ls, T = acc.FW_alg_div_step(f, h, L, Xd, iters, 2.0, lmo, epsilon=1e-300, verbose=False)
    torch.cuda.synchronize()
    rec = {"n": n, "r": r, "iters": len(F), "gpu_it_per_s": len(F) / (time.perf_counter() - t)}
    if host_iters:
        fh = S.FrobeniusSymLoss(Mh, X0)
        hh = S.SumOf2nd4thPowers(h.alpha, h.sigma)
        t = time.perf_counter()
        _, Fh, _ = S.FW_alg_div_step(fh, hh, L, X0, host_iters, 2.0, S.lmo_linf_ball(500.0, center), epsilon=1e-300)
        rec["host_iters"] = len(Fh)
        rec["host_it_per_s"] = len(Fh) / (time.perf_counter() - t)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="no host NumPy timings at n >= 8192")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "peak_tflops": PEAK, "evals": [], "fw": []}
    for n, r in ((400, 50), (700, 50), (8192, 64), (16384, 64), (16384, 128)):
        res["evals"].append(evals(n, r, host=not (a.quick and n >= 8192)))
        print(json.dumps(res["evals"][-1]), file=sys.stderr, flush=True)
    res["fw"].append(fw_rate(400, 50, 200, 200))
    res["fw"].append(fw_rate(16384, 64, 40, 0 if a.quick else 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
