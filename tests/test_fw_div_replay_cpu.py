"""The host's replay of the records of accbpg_fw_div_run in C (accbpg_and_fw_amd/csrc/fw_div_replay.hpp).  The header is
compiled alone with the host compiler behind a small main (the method of test_fw_div_decide_cpu.py, -ffp-contract=off),
and once more with -fsanitize=address,undefined as a stand-alone program (the way test_guard_cpu.py runs its own).  It is
fed chains of records made by the predictor of tests/fwdiv_batch_fake.py and held against the Python replay loop -- the
agreement rules of ``_div_device_steps`` / ``_descent_device_steps`` over the package's one copy of the decisions
(``_DivStepRun.decide``, ``_DescentRun.step`` / ``.probed``): the agreed count, the verdict, F, Ls / alpha and the
returned book, bit for bit (both sides call the same libm).  No GPU, nothing of the library loaded into Python."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import fwdiv_batch_fake as FB
from fwdiv_batch_fake import (AGREED_STOP, APPLIED, BAD_PIVOT, CLASSICAL, DEVICE_HB, DISAGREE, END, FIXED_L, HANDED_BACK,
                              HOST_HB, LINESEARCH, PIVOT, STOPPED)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")
N = 1000

# one chain in: mode n m nrun k0 (int64) | L gamma ls_ratio eps ld q F_prev fill value | nrun (+1: mode 2) records
# one chain out: rc agreed verdict k0 mode (int64) | L gamma ls_ratio eps ld q F_prev | F[nrun] | L_or_alpha[nrun]
MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "fw_div_replay.hpp"
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t iv[5];
    double dv[9];
    while (fread(iv, sizeof(iv), 1, in) == 1 && fread(dv, sizeof(dv), 1, in) == 1) {
        const int nrun = (int)iv[3];
        const size_t count = (size_t)nrun + (iv[0] == 2 ? 1 : 0);
        std::vector<accbpg_fw_div_step> steps(count);            // exactly as many as the call may read
        if (count && fread(steps.data(), sizeof(accbpg_fw_div_step), count, in) != count) return 3;
        std::vector<double> F((size_t)nrun, -777.0), LA((size_t)nrun, -777.0);   // ... and may write
        accbpg_fw_div_params prm{(int32_t)iv[0], 0, iv[4], dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6]};
        accbpg_fw_div_params book{};
        int agreed = -1, verdict = -1;
        const int rc = accbpg::fw_div_replay(&prm, iv[1], iv[2], dv[7], dv[8], steps.data(), nrun, F.data(), LA.data(),
                                             &book, &agreed, &verdict);
        const int64_t io[5] = {rc, agreed, verdict, book.k0, book.mode};
        const double dout[7] = {book.L, book.gamma, book.ls_ratio, book.epsilon, book.ld, book.q, book.F_prev};
        fwrite(io, sizeof(io), 1, out);
        fwrite(dout, sizeof(dout), 1, out);
        if (nrun) {
            fwrite(F.data(), sizeof(double), (size_t)nrun, out);
            fwrite(LA.data(), sizeof(double), (size_t)nrun, out);
        }
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


def _records_bytes(recs, lead):
    from accbpg_and_fw_amd import _lib
    arr = FB.to_ctypes(recs, lead)
    return bytes(arr)[:(len(recs) + (0 if lead is None else 1)) * C.sizeof(_lib.FwDivStep)]


def _runner(tmp_path_factory, name, extra):
    d = tmp_path_factory.mktemp(name)
    (d / "main.cpp").write_text(MAIN)
    exe = d / "replay"
    cmd = [_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", HEADER_DIR,
           str(d / "main.cpp"), "-o", str(exe)] + extra
    if extra and subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.DEVNULL,
                                stderr=subprocess.DEVNULL).returncode == 0:
        pass                    # the sanitizer runtimes linked into the program itself where the compiler knows the switches
    else:
        subprocess.check_call(cmd)

    def run(chains):
        """chains: [(mode, m, k0, (L, gamma, ls_ratio, eps, ld, q, F_prev), radius, recs, pending)]"""
        with open(str(d / "in.bin"), "wb") as fh:
            for mode, m, k0, book, radius, recs, pending in chains:
                fh.write(struct.pack("5q", mode, N, m, len(recs), k0))
                fh.write(struct.pack("9d", *(tuple(book) + (FB.FILL, float(radius)))))
                fh.write(_records_bytes(recs, pending if mode == CLASSICAL else None))
        done = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout
        assert "runtime error" not in done.stdout and "AddressSanitizer" not in done.stdout, done.stdout
        raw = open(str(d / "out.bin"), "rb").read()
        out, at = [], 0
        for mode, m, k0, book, radius, recs, pending in chains:
            io = struct.unpack_from("5q", raw, at)
            dv = struct.unpack_from("7d", raw, at + 40)
            at += 96
            F = np.frombuffer(raw, dtype=np.float64, count=len(recs), offset=at)
            LA = np.frombuffer(raw, dtype=np.float64, count=len(recs), offset=at + 8 * len(recs))
            at += 16 * len(recs)
            assert io[0] == 0 and io[4] == mode and dv[1:4] == tuple(book[1:4])
            assert np.all(F[io[1]:] == -777.0) and np.all(LA[io[1]:] == -777.0)     # nothing written past `agreed`
            out.append(SimpleNamespace(agreed=io[1], verdict=io[2], k0=io[3], L=dv[0], ld=dv[4], q=dv[5], F_prev=dv[6],
                                       F=F[:io[1]].copy(), LA=LA[:io[1]].copy()))
        assert at == len(raw)
        return out
    return run


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    return _runner(tmp_path_factory, "replay", [])


@pytest.fixture(scope="module")
def replay_sanitized(tmp_path_factory):
    return _runner(tmp_path_factory, "replay_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_header_stands_alone():
    """<cmath>, <cstdint>, the decisions and the C struct definitions: nothing of HIP."""
    includes = [ln.split()[1] for ln in open(os.path.join(HEADER_DIR, "fw_div_replay.hpp")) if ln.startswith("#include")]
    assert includes == ["<cmath>", "<cstdint>", '"../../include/accbpg_hip.h"', '"fw_div_decide.hpp"']
    api = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    assert [ln for ln in api.splitlines() if ln.startswith("#include")] == ["#include <stdint.h>"]


# ---- the Python replay loop: the agreement rules of the device solvers over the package's decisions -------------------
RAISES = (ValueError, AssertionError, ZeroDivisionError, OverflowError, TypeError)


def _same_bits(mine, theirs):
    return all(struct.pack("d", a) == struct.pack("d", b) or (a != a and b != b) for a, b in zip(mine, theirs))


def python_replay(mode, m, k0, book0, radius, recs, pending):
    from accbpg_and_fw_amd import D_opt_alg as D
    L, gamma, ls_ratio, eps, ld, q, F_prev = book0
    book = D._DivBook(m, radius, 0, ld)
    book.q = q
    F, LA, verdict, agreed = [], [], END, len(recs)
    size = k0 + len(recs) + 1
    if mode == CLASSICAL:
        run = D._DescentRun(book, size, eps)
        run.rec = pending
    else:
        run = D._DivStepRun(book, L, size, gamma, eps, mode == LINESEARCH, ls_ratio)
    if k0:
        run.F[k0 - 1] = F_prev
    for j, r in enumerate(recs):
        k = k0 + j
        in_range = 0 <= r.probe.i < N
        saved = (book.ld, book.q, book.since, getattr(run, "L", None), getattr(run, "rec", None))
        if r.status == HANDED_BACK:
            verdict = BAD_PIVOT if mode != CLASSICAL and (r.reason == PIVOT or not in_range) else DEVICE_HB
        elif r.status not in (APPLIED, STOPPED):
            verdict = DISAGREE
        elif mode != CLASSICAL:
            if not in_range:
                verdict = BAD_PIVOT
            else:
                try:
                    step, _, stop = run.decide(k, r.probe, 0.0, D._replay_capped)
                except (D._Capped,) + RAISES:
                    verdict = HOST_HB
                else:
                    if stop == (r.status == STOPPED) and _same_bits(step[1:] + (run.Ls[k],), (r.a, r.hcoef, r.hdiv, r.L)):
                        F.append(run.F[k])
                        LA.append(run.Ls[k])
                        if stop:
                            verdict, agreed = AGREED_STOP, j + 1
                            break
                        continue
                    verdict = DISAGREE
        else:
            try:
                step = run.step(k)
            except RAISES:
                verdict = HOST_HB
            else:
                if not _same_bits(step[1:], (r.a, r.hcoef, r.hdiv)):
                    verdict = DISAGREE
                elif not in_range:
                    verdict = BAD_PIVOT
                else:
                    try:
                        stop = run.probed(k, r.probe, 0.0)
                    except RAISES:
                        verdict = HOST_HB
                    else:
                        if stop == (r.status == STOPPED):
                            F.append(run.F[k])
                            LA.append(step[1])
                            if stop:
                                verdict, agreed = AGREED_STOP, j + 1
                                break
                            continue
                        verdict = DISAGREE
        book.ld, book.q, book.since = saved[:3]                 # not an agreed step: the book stays BEFORE this record
        if mode == CLASSICAL:
            run.rec = saved[4]
        else:
            run.L = saved[3]
        agreed = j
        break
    k = k0 + agreed
    return SimpleNamespace(agreed=agreed, verdict=verdict, k0=k, L=(L if mode == CLASSICAL else run.L), ld=book.ld,
                           q=book.q, F_prev=(run.F[k - 1] if agreed else F_prev), F=np.array(F), LA=np.array(LA))


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64).tolist()


def _hold(got, want, what):
    assert (got.agreed, got.verdict, got.k0) == (want.agreed, want.verdict, want.k0), (what, vars(got), vars(want))
    for name in ("L", "ld", "q", "F_prev", "F", "LA"):
        assert _bits(getattr(got, name)) == _bits(getattr(want, name)), (what, name)


# ---- chains -----------------------------------------------------------------------------------------------------------
def _probe(g, m, **over):
    w_i = m * g.uniform(1.05, 5.0)
    d = dict(i=int(g.integers(0, N)), w_i=w_i, x_i=g.uniform(1e-4, 0.5), sum_w=m * g.uniform(0.5, 2.0) * N / 10,
             sum_w2=m * m * g.uniform(1.0, 50.0) * N, slope=-10.0 ** g.uniform(-4, 0.5), div=10.0 ** g.uniform(0, 3),
             min_x=10.0 ** g.uniform(-12, -3), sum_u2=w_i * w_i * g.uniform(0.2, 3.0))
    d.update(over)
    return SimpleNamespace(**d)


def chain(seed, mode, nrun, over=None, flips=None, **kw):
    """(mode, m, k0, book, radius, recs, pending): ``nrun`` iterations of the predictor on random probes from a random
    book; over[j]: fields planted into probe j; flips[j]: falsify the prediction of record j."""
    g = np.random.default_rng(seed)
    m = int(g.choice([8, 30, 100]))
    radius = float(g.choice([1.0, 2.5]))
    k0 = kw.get("k0", int(g.choice([0, 1, 57])) if mode != CLASSICAL else int(g.choice([1, 2, 57])))
    gamma = kw.get("gamma", 2.0)
    ls_ratio = kw.get("ls_ratio", float(g.choice([1.2, 1.5, 2.0])))
    eps = kw.get("eps", 1e-14)
    ld, q = float(g.uniform(-50, 50)), float(g.choice([0.0, 1e-16]))
    L0 = kw.get("L", float(10.0 ** g.uniform(0.5, 3)))
    pending = _probe(g, m)
    F_prev = -ld - q * pending.sum_w + float(g.choice([1e-3, -1e-7, 1.0]))
    book0 = (L0 if mode != CLASSICAL else 0.0, gamma if mode != CLASSICAL else 0.0, ls_ratio if mode != CLASSICAL else 0.0,
             eps, ld, q, F_prev)
    bk = SimpleNamespace(ld=ld, q=q, m=m, radius=radius, F_prev=F_prev, L=L0)
    over, flips, recs, prev = over or {}, flips or {}, [], pending
    for j in range(nrun):
        probe = _probe(g, m, **over.get(j, {}))
        if mode == CLASSICAL:
            r = FB.predict_classical(prev, lambda a, hcoef, hdiv: probe, N, bk, eps, k0 + j, flips.get(j))
        else:
            r = FB.predict(probe, N, bk, mode, gamma, ls_ratio, eps, k0 + j, flips.get(j))
        recs.append(r)
        if r.status != APPLIED and not kw.get("run_on"):
            break
        prev = r.probe
    return mode, m, k0, book0, radius, recs, pending


def _both(replay, chains, what):
    got = replay(chains)
    for c, g in zip(chains, got):
        _hold(g, python_replay(*c), (what, c[0], c[2]))
    return got


@pytest.mark.parametrize("mode", [LINESEARCH, FIXED_L, CLASSICAL])
def test_random_chains(replay, mode):
    chains = [chain(1000 * mode + s, mode, int(1 + s % 40)) for s in range(300)]
    chains += [chain(5000 + s, mode, 30, gamma=g) for s, g in enumerate([1.5, 3.0, 1.5, 3.0])]
    chains.append(chain(77, mode, FB.RUN_MAX))                  # the longest a call holds
    got = _both(replay, chains, "random")
    verdicts = [g.verdict for g in got]
    print("mode", mode, "verdicts", {v: verdicts.count(v) for v in sorted(set(verdicts))},
          "agreed records", sum(g.agreed for g in got))
    assert verdicts.count(END) >= 100 and sum(g.agreed for g in got) >= 3000


@pytest.mark.parametrize("mode,fields", [(LINESEARCH, ("a", "hcoef", "hdiv", "L", "status")),
                                         (FIXED_L, ("a", "hcoef", "hdiv", "L", "status")),
                                         (CLASSICAL, ("a", "hcoef", "hdiv", "status"))])
def test_one_ulp_in_each_compared_field(replay, mode, fields):
    for at in (0, 6, 11):
        base = chain(31 + mode, mode, 12, L=50.0, k0=3)
        assert len(base[5]) == 12 and all(r.status == APPLIED for r in base[5])
        chains = []
        for f in fields:
            c = chain(31 + mode, mode, 12, L=50.0, k0=3)
            r = c[5][at]
            if f == "status":
                r.status = STOPPED
            else:
                setattr(r, f, float(np.nextafter(getattr(r, f), math.inf)))
            chains.append(c)
        for f in ("ld1", "q1", "f1", "trials"):                  # fields the replay does not compare
            c = chain(31 + mode, mode, 12, L=50.0, k0=3)
            setattr(c[5][at], f, getattr(c[5][at], f) + 1)
            chains.append(c)
        got = _both(replay, chains, ("ulp", at))
        for f, g in zip(fields, got):
            assert (g.verdict, g.agreed, g.k0) == (DISAGREE, at, 3 + at), (f, at, vars(g))
        for g in got[len(fields):]:
            assert (g.verdict, g.agreed) == (END, 12)
        whole = replay([base])[0]
        for g in got[:len(fields)]:                             # the book BEFORE the record: that of the agreed prefix
            assert _bits(g.F) == _bits(whole.F[:at]) and _bits(g.LA) == _bits(whole.LA[:at])


@pytest.mark.parametrize("reason", list(range(1, 8)))
def test_device_hand_back_reasons(replay, reason):
    chains = []
    for mode in (LINESEARCH, FIXED_L, CLASSICAL):
        c = chain(41 + mode, mode, 9, L=50.0, k0=2)
        assert len(c[5]) == 9
        c[5][5].status, c[5][5].reason = HANDED_BACK, reason
        chains.append(c)
    got = _both(replay, chains, ("hand-back", reason))
    want = BAD_PIVOT if reason == PIVOT else DEVICE_HB
    assert [(g.verdict, g.agreed) for g in got] == [(want, 5), (want, 5), (DEVICE_HB, 5)]


def test_host_side_hand_backs(replay):
    """Records that claim an applied step where the host's own decision is a hand-back: the cap (a tiny L in the book, a
    huge slope in one probe), a failed check of the sequential solver, an arithmetic error; verdict 3 at that record."""
    chains = []
    for mode in (LINESEARCH, FIXED_L):
        c = chain(51, mode, 8, L=50.0, k0=1, over={4: dict(slope=-1e12)}, run_on=True)
        assert c[5][4].status == HANDED_BACK and c[5][4].reason == FB.CAP
        c[5][4].status, c[5][4].a, c[5][4].hdiv = APPLIED, 0.5, 0.5
        chains.append(c)
        for fields in (dict(slope=2e-6), dict(min_x=0.0), dict(min_x=math.nan), dict(div=5e-324)):
            c = chain(52, mode, 8, L=0.5, k0=1, over={4: fields}, run_on=True)
            assert c[5][4].status == HANDED_BACK
            c[5][4].status = APPLIED
            chains.append(c)
    c = chain(53, CLASSICAL, 8, k0=1, over={3: dict(w_i=-1e6)}, run_on=True)   # log of a negative number in step 4
    assert c[5][4].status == HANDED_BACK
    c[5][4].status = APPLIED
    chains.append(c)
    c = chain(54, CLASSICAL, 8, k0=1, over={4: dict(sum_w2=-1.0)})           # math.sqrt of a negative sum
    assert len(c[5]) == 8
    chains.append(c)
    got = _both(replay, chains, "host hand-back")
    assert [(g.verdict, g.agreed) for g in got] == [(HOST_HB, 4)] * len(chains)


def test_pivots_nans_stops_and_empty_chains(replay):
    chains = []
    for mode in (LINESEARCH, CLASSICAL):
        for p in (-1, N):
            c = chain(61, mode, 7, L=50.0, k0=1, over={3: dict(i=p)}, run_on=True)
            chains.append(c)                                    # as the device records it: handed back / probed
            c = chain(61, mode, 7, L=50.0, k0=1, over={3: dict(i=p)}, run_on=True)
            c[5][3].status = APPLIED                            # ... and with the hand-back painted over
            chains.append(c)
    got = _both(replay, chains, "pivot")
    assert [(g.verdict, g.agreed) for g in got] == [(BAD_PIVOT, 3)] * len(chains)
    chains = []
    for mode in (LINESEARCH, FIXED_L, CLASSICAL):
        for fields in (dict(w_i=math.nan), dict(slope=math.nan), dict(sum_w=math.nan), dict(sum_u2=math.nan)):
            chains.append(chain(62, mode, 7, L=50.0, k0=1, over={2: fields}, run_on=True))
    got = _both(replay, chains, "NaN")
    assert all(g.agreed >= 2 for g in got)
    print("NaN chains", [(g.verdict, g.agreed) for g in got])
    chains = [chain(63, mode, 9, L=50.0, k0=k0, eps=math.inf) for mode in (LINESEARCH, FIXED_L, CLASSICAL) for k0 in (0, 1, 5)
              if k0 or mode != CLASSICAL]
    got = _both(replay, chains, "stop")
    for c, g in zip(chains, got):                               # k > 0 in the div step's test
        assert (g.verdict, g.agreed) == (AGREED_STOP, 2 if c[0] != CLASSICAL and c[2] == 0 else 1), (c[0], c[2], vars(g))
    c = chain(64, LINESEARCH, 9, L=50.0, k0=4)
    c[5][6].status = STOPPED if c[5][6].status == APPLIED else APPLIED
    chains = [c, chain(65, LINESEARCH, 0), chain(65, CLASSICAL, 0)]
    got = _both(replay, chains, "mid-chain and empty")
    assert (got[0].verdict, got[0].agreed) == (DISAGREE, 6)
    for c, g in zip(chains[1:], got[1:]):
        assert (g.verdict, g.agreed, g.k0) == (END, 0, c[2]) and _bits([g.L, g.ld, g.q, g.F_prev]) == _bits(
            [c[3][0], c[3][4], c[3][5], c[3][6]])


def test_under_address_and_undefined_behaviour_sanitizers(replay, replay_sanitized):
    """The same chains through the stand-alone program built with -fsanitize=address,undefined: the output arrays hold
    exactly nrun entries and the record array exactly what the call may read, so one entry too far is a report."""
    chains = [chain(7000 + s, s % 3, 1 + s % 25) for s in range(60)]
    chains += [chain(77, mode, FB.RUN_MAX) for mode in (LINESEARCH, CLASSICAL)]
    chains += [chain(65, LINESEARCH, 0), chain(65, CLASSICAL, 0)]
    c = chain(61, LINESEARCH, 7, L=50.0, k0=1, over={3: dict(i=-1)}, run_on=True)
    chains.append(c)
    for a, b in zip(replay(chains), replay_sanitized(chains)):
        _hold(b, a, "sanitized")
