"""Guard bands around the library's OWN device buffers (accbpg_debug_guard_bands / accbpg_debug_guard_check): every
scenario below is run twice, first with the switch off and then with every buffer of the handles it makes between two
bands of sentinel, max(65536, round_up(64 * m * 8, 4096)) bytes wide -- a whole stray tile row of an m x m buffer.
With the bands on, (i) the number of live banded buffers is at least what the scenario's handles own, so that the switch
cannot silently do nothing, (ii) no band is damaged behind the scenario -- the tile stores of the MFMA engine, the
double2 stores, the slab writes of the stream-K Gram kernel, the workspace layouts of the length-n kernels all stay
inside their buffers -- and (iii) the results equal those of the unbanded run bit for bit: the band width is a multiple
of 4096, the buffers keep the alignment hipMalloc gives, so every kernel runs in the same form.
The scenarios run in a worker thread whose thread-local scratch of the length-n kernels was allocated with the bands on
(the main thread's may be older than the switch)."""
import ctypes as C
import gc
import os
import queue
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_numpy as T  # noqa: E402

pytestmark = pytest.mark.gpu

DOPT_HANDLE_BUFFERS = 10     # Lbuf Wbuf Tbuf dscal vws slabs Pbuf chol_op + the tile list and the ranges of the Gram plan
DOPT_SHAPES = [(13, 506), (64, 271), (65, 267), (130, 334), (333, 537), (520, 723), (1100, 3000), (300, 900),
               (256, 1024), (64, 65537)]
TWO_LEVEL = 2048 | (1 << 12)            # as test_two_level_cholesky_forced_at_small_sizes


def band_bytes(m):
    return max(65536, -(-64 * m * 8 // 4096) * 4096)


class Worker(threading.Thread):
    """a thread that runs the callables handed to it (the library keeps scratch per thread)"""

    def __init__(self):
        super().__init__(daemon=True)
        self.tasks = queue.Queue()
        self.start()

    def run(self):
        while True:
            fn, box, done = self.tasks.get()
            if fn is None:
                return
            try:
                box.append(("ok", fn()))
            except BaseException as e:      # handed to the caller
                box.append(("error", e))
            done.set()

    def call(self, fn):
        box, done = [], threading.Event()
        self.tasks.put((fn, box, done))
        done.wait()
        kind, value = box[0]
        if kind == "error":
            raise value
        return value

    def stop(self):
        self.tasks.put((None, None, None))
        self.join()


def guard_check(lib):
    from accbpg_and_fw_amd import _lib
    out = (C.c_int64 * 3)()
    assert lib.accbpg_debug_guard_check(out) == 0, _lib.last_error()
    return out[0], out[1], out[2], (_lib.last_error() if out[1] else "")


def _touch_scratch(lib):
    x = torch.ones(8, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.accbpg_vec_workspace_doubles(8), dtype=torch.float64, device="cuda")
    out = (C.c_double * 2)()
    assert lib.accbpg_vec_min_sum(C.c_void_p(x.data_ptr()), 8, out, C.c_void_p(ws.data_ptr()), None) == 0
    assert list(out) == [1.0, 8.0]


@pytest.fixture(scope="module")
def env():
    """(acc, lib, worker): the bands are off on entry and on exit; `worker` owns banded thread-local scratch.

    The switch does not stay on for the whole module: every scenario needs its unbanded reference run in the same
    process, so run_both turns the bands on around the banded run only, before that run makes its first handle, and off
    behind it.  What cannot be made anew per scenario is the scratch of the length-n kernels, which the library keeps
    per thread and hands from a thread that ended to the next one that asks; the loop below starts threads, with the
    bands on, until one of them had to allocate its block (two more banded buffers are live), and that thread then
    runs every scenario."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    assert lib.accbpg_debug_guard_bands(100) == _lib.ERR_ARG and lib.accbpg_debug_guard_bands(-4096) == _lib.ERR_ARG
    assert lib.accbpg_debug_guard_bands(65536) == 0
    workers, owner = [], None
    try:
        for _ in range(8):          # a new thread may be handed an older thread's (unbanded) block from the pool
            before = guard_check(lib)[0]
            w = Worker()
            workers.append(w)
            w.call(lambda: _touch_scratch(lib))
            if guard_check(lib)[0] >= before + 2:
                owner = w
                break
        assert owner is not None, "no thread received freshly allocated scratch"
        assert lib.accbpg_debug_guard_bands(0) == 0
        yield acc, lib, owner
    finally:
        lib.accbpg_debug_guard_bands(0)
        for w in workers:
            w.stop()


def run_both(env, scenario, m, min_buffers):
    """scenario() -> (results, keep): unbanded, then banded with the handles in `keep` still alive at the check.
    The process-wide switch is set per run (see `env`): on before the banded run's first handle, off behind its check;
    buffers made while it was on keep their bands until they are freed, whatever the switch says then."""
    acc, lib, worker = env

    def once(width):
        assert lib.accbpg_debug_guard_bands(width) == 0
        try:
            before = guard_check(lib)[0]
            results, keep = scenario()
            torch.cuda.synchronize()
            live, bands, nbytes, msg = guard_check(lib)
        finally:
            lib.accbpg_debug_guard_bands(0)
        del keep
        gc.collect()
        return results, live - before, bands, nbytes, msg

    want, extra, bands, _, _ = worker.call(lambda: once(0))
    assert extra == 0 and bands == 0
    got, extra, bands, nbytes, msg = worker.call(lambda: once(band_bytes(m)))
    assert bands == 0, "%d damaged band(s), %d byte(s): %s" % (bands, nbytes, msg)
    assert extra >= min_buffers, "only %d banded buffers are live (expected at least %d)" % (extra, min_buffers)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        same = a.view(np.int64) == b.view(np.int64) if a.dtype == np.float64 else a == b
        assert np.all(same), "%s: %d of %d entries differ from the unbanded run" % (name, int(np.sum(~same)), same.size)


def gaussian(m, n, seed):
    return np.random.RandomState(seed).randn(m, n)


def simplex_point(n, seed):
    x = np.random.RandomState(seed).rand(n) + 0.01
    return x / x.sum()


def arr(*v):
    return np.array(v, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- the switch itself
def test_switch_bands_every_buffer_of_a_handle_and_frees_in_any_order(env):
    acc, lib, worker = env

    def body():
        V = torch.from_numpy(gaussian(64, 300, 1)).cuda()
        base = guard_check(lib)[0]
        plain = acc.DOptimalObj(V)                              # made with the switch off
        assert guard_check(lib)[0] == base
        assert lib.accbpg_debug_guard_bands(65536) == 0
        banded = acc.DOptimalObj(V)
        live = guard_check(lib)
        assert live[0] - base >= DOPT_HANDLE_BUFFERS and live[1:3] == (0, 0)
        assert lib.accbpg_debug_guard_bands(0) == 0             # ... they keep their bands with the switch off again
        x = simplex_point(300, 2)
        assert banded.func_grad(x, 2)[0] == plain.func_grad(x, 2)[0]
        assert guard_check(lib)[:3] == (live[0], 0, 0)
        del plain
        gc.collect()
        assert guard_check(lib)[0] == live[0]
        del banded
        gc.collect()
        assert guard_check(lib)[0] == base
    worker.call(body)


# ------------------------------------------------------------------------------------------------- D-optimal handles
@pytest.mark.parametrize("variant", [0, 64])
@pytest.mark.parametrize("m,n", DOPT_SHAPES)
def test_dopt_evaluation_paths(env, m, n, variant):
    acc, lib, _ = env
    V = torch.from_numpy(gaussian(m, n, m * 1000 + n)).cuda()
    x = torch.from_numpy(simplex_point(n, m)).cuda()

    def scenario():
        f = acc.DOptimalObj(V)
        bits = variant | (TWO_LEVEL if (m, n) == (300, 900) else 0)
        assert lib.accbpg_debug_chol_variant(f._h, bits) == 0
        fx, g = f.func_grad(x, 2)
        f0 = f(x)
        gram = torch.empty(m, m, dtype=torch.float64, device="cuda")
        f.gram_into(x, gram)
        fe, ge = C.c_double(), torch.empty(n, dtype=torch.float64, device="cuda")
        assert lib.accbpg_dopt_eval_gram(f._h, C.c_void_p(gram.data_ptr()), 2, C.byref(fe), C.c_void_p(ge.data_ptr())) == 0
        torch.cuda.synchronize()
        return [("f", arr(fx, f0, fe.value)), ("g", g.cpu().numpy()), ("g_eval", ge.cpu().numpy()),
                ("gram_lower", np.tril(gram.cpu().numpy()))], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS)


@pytest.mark.parametrize("m,n", [(130, 334), (520, 723)])
def test_abpg_gain_iterations(env, m, n):
    """the side handle of the value evaluations, the trial's status block, the value record"""
    acc, lib, _ = env
    V = gaussian(m, n, m + n)

    def scenario():
        f = acc.DOptimalObj(V)
        h = acc.BurgEntropySimplex()
        x, F, G, Gdiv, Gavg, _ = acc.ABPG_gain(f, h, 1.0, np.ones(n) / n, gamma=2, maxitrs=20, verbose=False)
        return [("x", x), ("F", F), ("G", G)], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS + 1)


def test_fw_away_with_logdet_ring(env):
    """the ring's auxiliary handles and the rank-one updates of fw_H"""
    acc, lib, _ = env
    m, n = 64, 512
    V = gaussian(m, n, 5)

    def scenario():
        f = acc.DOptimalObj(V)
        x, F, SP, SN, _ = acc.D_opt_FW_away(f, np.ones(n) / n, 1e-12, 50, verbose=False, logdet_refresh=1, logdet_ring=3)
        return [("x", x), ("F", F), ("SP", SP), ("SN", SN)], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS + 4)


def test_fw_away_device_steps(env):
    acc, lib, _ = env
    m, n = 64, 512
    V = gaussian(m, n, 6)

    def scenario():
        f = acc.DOptimalObj(V)
        x, F, SP, SN, _ = acc.D_opt_FW_away_device(f, np.ones(n) / n, 1e-12, 40, verbose=False, sync_every=8)
        return [("x", x), ("F", F), ("SP", SP), ("SN", SN)], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS + 5)


def test_kyinit_device(env):
    acc, lib, _ = env
    m, n = 65, 267
    V = gaussian(m, n, 7)

    def scenario():
        f = acc.DOptimalObj(V)
        np.random.seed(11)
        x0, picked = acc.D_opt_KYinit_device(f, return_picked=True)
        return [("x0", x0), ("picked", np.asarray(picked, dtype=np.int64))], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS)


@pytest.mark.parametrize("K,m,n,fused", [(3, 256, 1024, True), (4, 96, 640, False)])
def test_batches(env, K, m, n, fused):
    acc, lib, _ = env
    from accbpg_and_fw_amd.batched import ABPG_batch, DOptimalBatch
    Vs = [torch.from_numpy(gaussian(m, n, 77 * i + m)).cuda() for i in range(K)]

    def scenario():
        batch = DOptimalBatch(Vs)
        assert batch.fused == fused
        x0 = np.ones(n) / n
        res = []
        for i, (x, F, G, _) in enumerate(ABPG_batch(batch, acc.BurgEntropySimplex(), 1.0, x0, 2.0, 5)):
            res += [("abpg_x%d" % i, x), ("abpg_F%d" % i, F)]
        for i, out in enumerate(acc.D_opt_FW_batch(batch, x0, 1e-12, 10)):
            res += [("fw_x%d" % i, np.asarray(out[0])), ("fw_F%d" % i, np.asarray(out[1]))]
        return res, batch

    run_both(env, scenario, m, K * DOPT_HANDLE_BUFFERS)


def test_shards(env):
    acc, lib, _ = env
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.sharded import LogicalShards, NativeShardedDOptimalObj, native_unique_id
    m = 96
    V0, V1 = gaussian(m, 1000, 12), gaussian(m, 1001, 13)
    x0, x1 = simplex_point(1000, 1), simplex_point(1001, 2)

    def scenario():
        ls = LogicalShards(V0, 3)
        f0, g0 = ls.func_grad(x0, 2)
        fs = NativeShardedDOptimalObj(torch.from_numpy(V1).cuda(), 1001, 1, 0, native_unique_id())
        f1, g1 = fs.func_grad(x1, 2)
        _lib.check(lib.accbpg_debug_shard_pad(fs._s, 3), "accbpg_debug_shard_pad")
        f2, g2 = fs.func_grad(x1, 2)
        return [("f", arr(f0, f1, f2)), ("g_logical", g0), ("g_native", g1), ("g_padded", g2)], (ls, fs)

    run_both(env, scenario, m, 4 * DOPT_HANDLE_BUFFERS + 3)


# ------------------------------------------------------------------------------------------------- the other objectives
@pytest.mark.parametrize("m,n", [(37, 51), (5, 4096), (1000, 3), (513, 130)])
@pytest.mark.parametrize("kind", ["PoissonRegression", "KLdivRegression"])
def test_regression_objectives(env, kind, m, n):
    acc, lib, _ = env
    rng = np.random.RandomState(m * 31 + n)
    A, b, x = rng.rand(m, n), rng.rand(m) + 0.2, rng.rand(n) / n + 1e-4

    def scenario():
        f = getattr(acc, kind)(A, b)
        fx, g = f.func_grad(x, 2)
        return [("f", arr(fx, f(x))), ("g", g), ("g1", f.gradient(x))], f

    run_both(env, scenario, m, 5)             # Ax r t upart dout


@pytest.mark.parametrize("n,r", [(1, 1), (17, 3), (400, 50), (257, 64), (300, 70), (513, 130)])
def test_symnmf_objective(env, n, r):
    """the split slabs P, spart and red"""
    acc, lib, _ = env
    rng = np.random.RandomState(n * 7 + r)
    W = rng.rand(n, r)
    M, X = W @ W.T, rng.rand(n, r)

    def scenario():
        f = acc.FrobeniusSymLoss(M, X)
        fx, g = f.func_grad(X, 2)
        return [("f", arr(fx, f(X))), ("g", np.asarray(g)), ("g1", np.asarray(f.gradient(X)))], f

    run_both(env, scenario, n, 5)             # P S spart red dout


# ------------------------------------------------------------------------------------------------- length-n families
@pytest.mark.parametrize("n", [32769, 2048 * 256 + 1])
def test_length_n_families_on_banded_scratch(env, n):
    """the thread-local flags / out scratch (the worker's is banded) and a batch's vws: every family once"""
    acc, lib, _ = env
    from accbpg_and_fw_amd import functions as Fn
    from accbpg_and_fw_amd.batched import DOptimalBatch
    g, x, y, z, w = (torch.from_numpy(T.draw(n, k)).cuda() for k in range(5))
    px, py, pz, pw = (v.abs() + 0.05 for v in (x, y, z, w))
    sx = px / px.sum()
    K, mb = 2, 16
    Vs = [torch.from_numpy(gaussian(mb, n, 3 + i)).cuda() for i in range(K)]

    def host(v):
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)

    def scenario():
        res = []
        burg, shannon = acc.BurgEntropySimplex(), acc.ShannonEntropySimplex()
        res.append(("burg_prox", host(burg.div_prox_map(sx, g, 1.5))))
        res.append(("burg_ls_terms", arr(*Fn.ls_terms(g, px, py, pz, pw))))
        res.append(("vec", arr(Fn.vec_dot(x, y), Fn.vec_dot_diff(g, x, y), *Fn.vec_min_sum(x), *Fn.vec_argminmax(x))))
        res.append(("shannon_prox", host(shannon.div_prox_map(sx, g, 1.5))))
        res.append(("shannon_ls_terms", arr(*Fn.shannon_ls_terms(g, px, py, pz, pw))))
        res.append(("quartic_ls_terms", arr(*Fn.quartic_ls_terms(g, x, y, z, w))))
        wv, lin, dist = Fn.combine_ls_terms(acc.BurgEntropy(), 0.3, px, 0.7, py, 1.3, g, pz)
        res += [("combine_w", host(wv)), ("combine", arr(lin, dist))]
        batch = DOptimalBatch(Vs)
        X = torch.stack([sx, sx]).contiguous()
        G = torch.stack([g, -g]).contiguous()
        res.append(("batch_prox", host(batch.prox(X, G, [1.5, 2.5], 1e-8))))
        res.append(("batch_ls_terms", batch.ls_terms(G, torch.stack([px, py]), torch.stack([py, pz]))))
        return res, batch

    run_both(env, scenario, mb, K * DOPT_HANDLE_BUFFERS + 3)
