"""The decisions of one Bregman-step Frank-Wolfe iteration as the device predicts them are plain C++
(accbpg_and_fw_amd/csrc/fw_div_decide.hpp).  The header is compiled alone with the host compiler behind a small main that
reads records and writes decisions, and is held against the one Python copy of the same decisions --
``_DivStepRun.decide`` / ``_DescentRun`` of D_opt_alg.py -- on 120 000 random records.  On the host both sides call the
same libm, so the bar is equality bit for bit of (L, trials, a, hcoef, hdiv, ld1, q1, f1, F[k], stop) and of the
hand-back reason, with no case left out.  No GPU, nothing loaded into Python."""
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")
TRIALS_MAX = 64
NONE, BUDGET, L_INF, SLOPE, MIN_X, PIVOT, CAP, ARITH = range(8)
APPLIED, STOPPED, HANDED_BACK = 0, 1, 2

# one row in: i n k mode (int64) | w_i x_i sum_w sum_w2 slope div min_x sum_u2 ld q m radius F_prev L gamma ls_ratio eps
# one row out: status reason trials dstop (int64) | L a hcoef hdiv ld1 q1 f1 fx | da dhcoef dhdiv dld1 dq1 dF (descent)
MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "fw_div_decide.hpp"
using namespace accbpg;
struct Rec { long long i; double w_i, x_i, sum_w, sum_w2, slope, div, min_x, sum_u2; };
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t iv[4];
    double dv[17];
    while (fread(iv, sizeof(iv), 1, in) == 1 && fread(dv, sizeof(dv), 1, in) == 1) {
        Rec r{iv[0], dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], dv[7]};
        const FwdBook b0{dv[8], dv[9], dv[10], dv[11], 1e-15, dv[12]};
        FwdBook b = b0;
        double L = dv[13];
        FwdOut o;
        fw_div_decide(r, iv[1], &b, &L, (int)iv[3], dv[14], dv[15], dv[16], iv[2], &o);
        // the classical step of iteration max(k, 1) from the same record and book, then the stop test on it
        FwdBook d = b0;
        FwdOut s;
        const long long kd = iv[2] > 0 ? iv[2] : 1;
        fw_descent_step(r, iv[1], &d, kd, &s);
        double Fk = 0.0;
        const bool dstop = fw_descent_probed(r, &d, dv[16], &Fk);
        const int64_t io[4] = {o.status, o.reason, o.trials, (s.status == FWD_HANDED_BACK ? 2 : 0) + (dstop ? 1 : 0)};
        const double dout[14] = {o.L, o.a, o.hcoef, o.hdiv, o.ld1, o.q1, o.f1, o.fx, s.a, s.hcoef, s.hdiv, s.ld1, s.q1, Fk};
        fwrite(io, sizeof(io), 1, out);
        fwrite(dout, sizeof(dout), 1, out);
    }
    fclose(out);
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(rocm), "no host C++ compiler found"
    return rocm


@pytest.fixture(scope="module")
def decide_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fwdiv")
    (d / "main.cpp").write_text(MAIN)
    exe = d / "decide"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", HEADER_DIR,
                           str(d / "main.cpp"), "-o", str(exe)])

    def run(iv, dv):
        iv = np.ascontiguousarray(iv, dtype=np.int64)
        dv = np.ascontiguousarray(dv, dtype=np.float64)
        rows = np.zeros(len(iv), dtype=[("i", np.int64, 4), ("d", np.float64, 17)])
        rows["i"], rows["d"] = iv, dv
        rows.tofile(str(d / "in.bin"))
        subprocess.check_call([str(exe), str(d / "in.bin"), str(d / "out.bin")])
        out = np.fromfile(str(d / "out.bin"), dtype=[("i", np.int64, 4), ("d", np.float64, 14)])
        assert len(out) == len(iv)
        return out["i"], out["d"]
    return run


def test_header_stands_alone():
    """<cmath> only: the fixture compiles the header with the host compiler alone."""
    includes = [ln.strip() for ln in open(os.path.join(HEADER_DIR, "fw_div_decide.hpp")) if ln.startswith("#include")]
    assert includes == ["#include <cmath>"]


def _cases(N, seed):
    """The record, book and parameter columns of N random iterations (see the module docstring for the layout)."""
    g = np.random.default_rng(seed)
    m = g.choice([8, 13, 30, 100, 2048], N).astype(np.float64)
    n = 1000
    i = g.integers(0, n, N)
    i[g.random(N) < 0.005] = -1
    i[g.random(N) < 0.005] = n
    w_i = m * g.uniform(1.0, 5.0, N)
    w_i[g.random(N) < 0.02] = np.nan
    x_i = g.uniform(1e-4, 0.5, N)
    sum_w = m * g.uniform(0.5, 2.0, N) * n / 10
    sum_w2 = sum_w * g.uniform(0.5, 3.0, N) * m
    sum_w2[g.random(N) < 0.02] = 10.0 ** g.uniform(-40, -20)
    slope = -10.0 ** g.uniform(-9, math.log10(50.0), N)
    band = g.random(N) < 0.03
    slope[band] = g.uniform(0, 1e-6, band.sum())
    slope[g.random(N) < 0.003] = 1e-6
    slope[g.random(N) < 0.01] = 1.5e-6
    slope[g.random(N) < 0.02] = np.nan
    div = 10.0 ** g.uniform(-3, 3, N)
    div[g.random(N) < 0.03] = 0.0
    min_x = 10.0 ** g.uniform(-16, -3, N)
    min_x[g.random(N) < 0.005] = 0.0
    min_x[g.random(N) < 0.005] = np.nan
    sum_u2 = w_i * w_i * g.uniform(0.2, 3.0, N)
    ld = g.uniform(-50, 50, N)
    q = np.where(g.random(N) < 0.5, 0.0, 1e-15 * g.uniform(0, 1, N))
    radius = g.choice([1.0, 2.5], N)
    L = 10.0 ** g.uniform(-2, 3, N)
    tiny = g.random(N) < 0.05                                   # forces the cap
    L[tiny] = 10.0 ** g.uniform(-14, -9, tiny.sum())
    gamma = g.choice([2.0, 1.5, 3.0], N)
    ls_ratio = g.choice([1.2, 1.5, 2.0], N)
    huge = g.random(N) < 0.02                                   # never accepts, and L reaches inf within the budget
    L[huge] = 10.0 ** g.uniform(300, 308, huge.sum())
    ls_ratio[huge] = 2.0
    sum_u2[huge] = np.nan
    neg = g.random(N) < 0.01                                    # a negative base: ** leaves the reals at gamma == 3
    div[neg] = -div[neg]
    L[g.random(N) < 0.005] = 5e-324                             # 2 * L * div == 0: a zero divisor
    mode = (g.random(N) < 0.2).astype(np.int64)
    eps = g.choice([1e-14, 1e-6], N)
    k = g.choice([0, 1, 57], N)
    fx = -ld - q * sum_w
    F_prev = fx + g.choice([0.0, 1e-15, -3e-15, 1e-7, 1e-3], N)
    iv = np.stack([i, np.full(N, n), k, mode], axis=1)
    dv = np.stack([w_i, x_i, sum_w, sum_w2, slope, div, min_x, sum_u2, ld, q, m, radius, F_prev, L, gamma, ls_ratio,
                   eps], axis=1)
    return iv, dv


class _Cap(Exception):
    pass


class _Budget(Exception):
    pass


def _python_side(iv, dv):
    """What ``_DivStepRun.decide`` and ``_DescentRun`` make of one row: the output row of the compiled text."""
    from accbpg_and_fw_amd.D_opt_alg import _DescentRun, _DivBook, _DivStepRun
    i, n, k, mode = (int(v) for v in iv)
    (w_i, x_i, sum_w, sum_w2, slope, div, min_x, sum_u2, ld, q, m, radius, F_prev, L, gamma, ls_ratio,
     eps) = (float(v) for v in dv)
    rec = types.SimpleNamespace(i=i, w_i=w_i, x_i=x_i, sum_w=sum_w, sum_w2=sum_w2, slope=slope, div=div, min_x=min_x,
                                sum_u2=sum_u2)
    calls = [0]

    class Book(_DivBook):
        def scalars(self, a, r):
            if calls[0] == TRIALS_MAX:
                raise _Budget()
            calls[0] += 1
            self.last = _DivBook.scalars(self, a, r)
            return self.last

    def capped(r):
        raise (_Budget if calls[0] == TRIALS_MAX else _Cap)()

    def book():
        b = Book(int(m), radius, 0, ld)
        b.q = q
        return b

    b = book()
    run = _DivStepRun(b, L, k + 1, gamma, eps, mode == 0, ls_ratio)
    if k > 0:
        run.F[k - 1] = F_prev
    status, reason, out = HANDED_BACK, NONE, None
    fx = b.value(rec)
    if not 0 <= i < n:
        reason = PIVOT                                          # (the sequential solver's probe raises)
    else:
        try:
            step, trial, stop = run.decide(k, rec, 0.0, capped)
            assert trial is None
            status = STOPPED if stop else APPLIED
            out = (run.L, step[1], step[2], step[3], b.ld, b.q, b.last[4])
            assert step[0] == i and run.Ls[k] == run.L
        except _Cap:
            reason = CAP
        except _Budget:
            reason = BUDGET
        except ValueError as e:
            reason = SLOPE if "grad_d_prod must be non-positive" in str(e) else ARITH
            assert reason == SLOPE or "math domain error" in str(e)
        except AssertionError as e:
            reason = {"Entries of x or y not positive.": MIN_X, "L is infinite": L_INF}[str(e)]
        except (ZeroDivisionError, OverflowError, TypeError):
            reason = ARITH
    trials = calls[0]
    # the classical step from the same record and book
    calls[0] = 0
    d = book()
    drun = _DescentRun(d, max(k, 1) + 1, eps)
    drun.rec = rec
    drun.F[max(k, 1) - 1] = F_prev
    dflag, dout = 0, None
    if not 0 <= i < n:
        dflag = 2
    else:
        try:
            _, a, hcoef, hdiv = drun.step(max(k, 1))
            dout = (a, hcoef, hdiv, d.ld, d.q)
        except (ZeroDivisionError, ValueError):
            dflag = 2
    dstop = drun.probed(max(k, 1), rec, 0.0)
    return status, reason, trials, out, fx, dflag + int(dstop), dout, float(drun.F[max(k, 1)])


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def test_compiled_text_equals_the_python_text(decide_exe):
    N = 120000
    iv, dv = _cases(N, 20240607)
    oi, od = decide_exe(iv, dv)
    seen = {}
    trials_seen = set()
    for r in range(N):
        status, reason, trials, out, fx, dflag, dout, dF = _python_side(iv[r], dv[r])
        where = "row %d: %r %r" % (r, iv[r].tolist(), dv[r].tolist())
        assert (oi[r, 0], oi[r, 1]) == (status, reason), where
        seen[(status, reason)] = seen.get((status, reason), 0) + 1
        assert _bits(od[r, 7]) == _bits(fx), where
        assert oi[r, 2] == trials, where                        # the trials that reached _DivBook.scalars, every reason
        if status != HANDED_BACK:
            assert np.array_equal(_bits(od[r, :7]), _bits(out)), where
            trials_seen.add(trials)
        elif reason == BUDGET:
            assert oi[r, 2] == TRIALS_MAX, where
        assert oi[r, 3] == dflag, where
        if dout is not None:
            assert np.array_equal(_bits(od[r, 8:13]), _bits(dout)), where
        assert _bits(od[r, 13]) == _bits(dF), where
    print("status/reason counts:", sorted(seen.items()), "trial counts seen:", sorted(trials_seen))
    # the table cannot quietly stop covering a branch
    for key in [(APPLIED, NONE), (STOPPED, NONE), (HANDED_BACK, L_INF), (HANDED_BACK, SLOPE), (HANDED_BACK, MIN_X),
                (HANDED_BACK, PIVOT), (HANDED_BACK, CAP), (HANDED_BACK, BUDGET), (HANDED_BACK, ARITH)]:
        assert seen.get(key, 0) >= 50, (key, seen)
    assert len(trials_seen) >= 8


def test_trial_bound(decide_exe):
    """A record that never accepts (NaN sum_u2 makes every f1 a NaN) hands back after exactly the bound, at every
    ls_ratio; L stays finite, so nothing else ends the loop."""
    rows_i, rows_d = [], []
    for ls_ratio in (1.2, 1.5, 2.0):
        rows_i.append([3, 1000, 5, 0])
        rows_d.append([40.0, 0.01, 900.0, 4000.0, -2.0, 3.0, 1e-6, math.nan, 7.0, 0.0, 13.0, 1.0, -7.0, 1.0, 2.0, ls_ratio,
                       1e-14])
    oi, od = decide_exe(rows_i, rows_d)
    for r in range(3):
        assert oi[r].tolist()[:3] == [HANDED_BACK, BUDGET, TRIALS_MAX]
        status, reason, trials, *_ = _python_side(np.array(rows_i[r]), np.array(rows_d[r]))
        assert (status, reason, trials) == (HANDED_BACK, BUDGET, TRIALS_MAX)


def test_arithmetic_that_raises_is_handed_back(decide_exe):
    """Where Python's arithmetic raises -- a zero divisor, ** overflowing, ** leaving the reals, log of a non-positive --
    the compiled text hands back with reason 7 instead of deciding."""
    base = [40.0, 0.01, 900.0, 4000.0, -2.0, 3.0, 1e-6, 50.0, 7.0, 0.0, 13.0, 1.0, -7.0, 1.0, 2.0, 2.0, 1e-14]
    rows = []
    for col, val in [(13, 5e-324), (14, 1.0), (5, -3.0), (0, -1e30)]:      # 2*L*div == 0; gamma == 1; div < 0; den < 0
        row = list(base)
        row[col] = val
        if col == 5:
            row[14] = 1.5 + 1e-3                                # a negative base to a fractional power
        if col == 0:
            row[13] = 1e3
        rows.append(row)
    rows.append(list(base))
    rows[-1][4], rows[-1][13], rows[-1][14] = -1e200, 1e-3, 1.5            # (1e200-ish) ** 2 overflows
    iv = [[3, 1000, 5, 0]] * len(rows)
    oi, od = decide_exe(iv, rows)
    for r in range(len(rows)):
        status, reason, *_ = _python_side(np.array(iv[r]), np.array(rows[r]))
        assert (status, reason) == (HANDED_BACK, ARITH), (r, status, reason)
        assert oi[r].tolist()[:2] == [HANDED_BACK, ARITH], r
