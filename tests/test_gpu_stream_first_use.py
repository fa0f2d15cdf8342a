"""First use and ordering of every handle family on non-default streams.

The rest of the suite builds its handles and makes its calls on the default stream behind a synchronisation, where
everything is ordered for free; the package itself works on non-blocking streams (solve_batch, BatchStepper, the side
handle of DOptimalObj, the twin batch of DOptimalBatch.value_async, the auxiliary handles of the away-step log-det
ring).  Here every subject -- ``make()`` builds fresh objects from device inputs, ``use()`` runs a fixed list of entry
points and returns every result as host bytes -- is run quietly on the default stream (mode Q, the reference) and then
with gates (tests/stream_gate.py) that make any misplaced fill, copy or launch land late:

  A  first use on a fresh non-blocking stream with the default stream gated (re-gated before ``use()`` when the
     blocking uploads of ``create`` have drained the first gate), then again after ``s.synchronize()`` only, then after
     a device synchronisation;
  B  inputs poisoned, then written late on the call's own stream behind a gate on that stream -- once before
     ``make()`` and, since create waits for its stream, once more before ``use()``;
  C  ``make()`` on a gated stream s1, ``use()`` on a second fresh stream with the default stream gated as well (the
     caller orders its own inputs with an event recorded before ``make()``; nothing of ``create`` is waited for);
  D  host threads on fresh objects (solve_batch, BatchStepper) with the default stream gated (the gate holds every
     worker at the blocking uploads of its side handle's create: it delays, it does not race).

Every comparison is bit for bit against mode Q of the same subject (bytes, so NaNs by pattern).  A gate lasts ten times
the longest quiet ``use()`` of the module (both times are printed), and every gated case asserts that its gate is still
pending immediately before the call under test.  The streams of a gated case are chosen so that they do not share a
hardware queue with the gated stream (``stream_gate.independent_stream``); the streams the package creates itself
cannot be chosen, and one that shares the gated queue merely waits.  No case is repeated: the gates make the ordering
deterministic."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stream_gate as sg

GATE_FACTOR = 10


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


# ---------------------------------------------------------------------------------------------------------------------
# results as host bytes
def _bytes(v):
    """A result as host bytes.  A device tensor is consumed with a clone on the current stream before any host wait
    (an entry point may return it without having waited)."""
    if isinstance(v, torch.Tensor):
        return v.clone().cpu().numpy().tobytes()
    if isinstance(v, (tuple, list)):
        return b"".join(_bytes(e) for e in v)
    if isinstance(v, (int, np.integer)):
        return np.int64(v).tobytes()
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes()


class _Out:
    def __init__(self):
        self.items = []

    def add(self, label, value):
        self.items.append((label, _bytes(value)))
        return value


def _same(got, ref, what):
    assert [l for l, _ in got] == [l for l, _ in ref], what
    for (label, a), (_, b) in zip(got, ref):
        if a != b:
            x, y = np.frombuffer(a, dtype=np.uint64), np.frombuffer(b, dtype=np.uint64)
            bad = np.flatnonzero(x != y) if x.size == y.size else np.arange(0)
            pytest.fail("%s: %s differs from the quiet run (%d of %d words; first at %s: %r against %r)"
                        % (what, label, bad.size, y.size, bad[:1], x.view(np.float64)[bad[:1]], y.view(np.float64)[bad[:1]]))


def _simplex_point(rng, *shape):
    x = rng.rand(*shape) + 0.05
    return x / x.sum(axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# subjects
class S1:
    """DOptimalObj (96, 640), one-launch Cholesky; ABPG_gain is the first accbpg_dopt_burg_trial (allocates the status
    block) and the first value_async (creates the side handle)."""
    m, n = 96, 640
    held = ("H",)                                               # inputs the objects of make() keep reading

    def host(self):
        rng = np.random.RandomState(9600 + self.n)
        return {"H": rng.randn(self.m, self.n), "x": _simplex_point(rng, self.n), "x0": np.full(self.n, 1.0 / self.n)}

    def make(self, acc, inp):
        return acc.DOptimalObj(inp["H"]), acc.BurgEntropySimplex()

    def use(self, acc, objs, inp):
        f, h = objs
        o = _Out()
        o.add("func_grad(x,2)", f.func_grad(inp["x"], 2))
        o.add("f(x)", f(inp["x"]))
        o.add("gradient(x)", f.gradient(inp["x"]))
        x, F, Gain = acc.ABPG_gain(f, h, 1.0, inp["x0"], gamma=2, maxitrs=6, verbose=False)[:3]
        o.add("ABPG_gain x", x); o.add("ABPG_gain F", F); o.add("ABPG_gain Gain", Gain)
        return o.items


class S2(S1):
    """DOptimalObj (768, 2048), big tile."""
    m, n = 768, 2048

    def use(self, acc, objs, inp):
        f, _ = objs
        o = _Out()
        o.add("func_grad(x,2)", f.func_grad(inp["x"], 2))
        o.add("f(x)", f(inp["x"]))
        return o.items


class S3(S1):
    """DOptimalObj (1536, 4096): the side handle factors in small launches for m > 1408."""
    m, n = 1536, 4096

    def use(self, acc, objs, inp):
        f, h = objs
        o = _Out()
        x, F, G = acc.ABPG(f, h, 1.0, inp["x0"], gamma=2, maxitrs=3, verbose=False)[:3]
        o.add("ABPG x", x); o.add("ABPG F", F); o.add("ABPG G", G)
        return o.items


class S4:
    """DOptimalBatch, K = 3 at (96, 640); ABPG_gain_batch with overlap creates the twin batch and the side stream."""
    K, m, n = 3, 96, 640
    held = ("H",)

    def host(self):
        rng = np.random.RandomState(396640)
        return {"H": rng.randn(self.K, self.m, self.n), "X": _simplex_point(rng, self.K, self.n),
                "X0": np.full((self.K, self.n), 1.0 / self.n)}

    def make(self, acc, inp):
        return acc.DOptimalBatch([inp["H"][i] for i in range(self.K)]), acc.BurgEntropySimplex()

    def use(self, acc, objs, inp):
        batch, h = objs
        K, X = self.K, inp["X"]
        o = _Out()
        fv, G = o.add("func_grad(X,2)", batch.func_grad(X, 2))
        Z = o.add("prox", batch.prox(X, G, [1.0, 1.5, 2.0], h.eps))
        o.add("ls_terms", batch.ls_terms(G, Z, X))
        o.add("axpby", batch.axpby([0.25] * K, X, [0.75] * K, Z))
        o.add("avg_prox", batch.avg_prox(G, G, [0.5, 1.0, 1.5], [1.5, 2.0, 2.5], [1 / 1.5, 1 / 2.0, 1 / 2.5], h.eps))
        for i, res in enumerate(acc.ABPG_gain_batch(batch, h, 1.0, inp["X0"], gamma=2, maxitrs=5, overlap=True)):
            o.add("ABPG_gain_batch[%d] x, F, Gain" % i, res[:3])
        np.random.seed(77)                                      # D_opt_KYinit_batch draws its directions on the host
        o.add("D_opt_KYinit_batch", acc.D_opt_KYinit_batch(batch, return_picked=True))
        return o.items


class S5(S1):
    """Frank-Wolfe at (64, 512): the pipelined log-det form of the away-step solver with a ring of depth 2 (auxiliary
    handles on streams of their own), then the two solvers that decide their steps on the device."""
    m, n = 64, 512

    def make(self, acc, inp):
        return acc.DOptimalObj(inp["H"])

    def use(self, acc, f, inp):
        o = _Out()
        o.add("D_opt_FW_away x, F, SP, SN",
              acc.D_opt_FW_away(f, inp["x0"], 1e-8, 40, verbose=False, logdet_refresh=1, logdet_ring=2)[:4])
        o.add("D_opt_FW_device x, F, SP, SN", acc.D_opt_FW_device(f, inp["x0"], 1e-8, 64, verbose=False)[:4])
        o.add("D_opt_FW_div_step_device x, F, Ls",
              acc.D_opt_FW_div_step_device(f, 1.0, inp["x0"], 20, 2.0, verbose=False)[:3])
        return o.items


class S6:
    """The other handle families: func_grad(x, 2), then flag 0, then flag 1, and the prox maps that go with them."""
    held = ("A", "b_p", "b_k", "As", "ys", "M")

    def host(self):
        rng = np.random.RandomState(3751)
        A = rng.rand(37, 51)
        A = A / A.sum(axis=0)
        xs = rng.rand(51)
        W = rng.rand(400, 50)
        M = W @ W.T
        As = rng.randn(33, 130)
        return {"A": A, "b_p": A @ (np.maximum(xs - xs.mean(), 0) * 10 / 51) + 0.01 * (rng.rand(37) + 0.5),
                "b_k": A @ xs + 0.01 * (rng.rand(37) + 0.5), "x_p": np.full(51, 10.0 / 51), "x_k": np.full(51, 0.5),
                "As": As, "ys": np.sign(As @ rng.randn(130) + 0.1), "x_s": 0.1 * rng.randn(130),
                "M": 0.5 * (M + M.T), "X": rng.rand(400, 50)}

    def make(self, acc, inp):
        return {"poisson": acc.PoissonRegression(inp["A"], inp["b_p"]), "kl": acc.KLdivRegression(inp["A"], inp["b_k"]),
                "svm": acc.SVM_fun(0.1, inp["As"], inp["ys"]), "sym": acc.FrobeniusSymLoss(inp["M"], inp["X"]),
                "h_p": acc.BurgEntropyL1(0.0), "h_k": acc.ShannonEntropy(),
                "h_s": acc.SumOf2nd4thPowersPositiveOrthant(6.0, 2.0), "lmo": acc.lmo_l2_ball(5.0)}

    def use(self, acc, d, inp):
        o = _Out()
        grads = {}
        for name, x in (("poisson", inp["x_p"]), ("kl", inp["x_k"]), ("svm", inp["x_s"]), ("sym", inp["X"])):
            grads[name] = o.add(name + " func_grad(x,2)", d[name].func_grad(x, 2))[1]
            o.add(name + " flag 0", d[name].func_grad(x, 0))
            o.add(name + " flag 1", d[name].func_grad(x, 1))
        o.add("BurgEntropyL1.div_prox_map", d["h_p"].div_prox_map(inp["x_p"], grads["poisson"], 40.0))
        z = o.add("ShannonEntropy.div_prox_map", d["h_k"].div_prox_map(inp["x_k"], grads["kl"], 1.0))
        o.add("ShannonEntropy.divergence", d["h_k"].divergence(z, inp["x_k"]))
        o.add("SumOf2nd4thPowersPositiveOrthant.div_prox_map", d["h_s"].div_prox_map(inp["X"], grads["sym"], 1.0e4))
        o.add("lmo_l2_ball", d["lmo"](grads["sym"]))
        return o.items


class S7:
    """Handle-free vector kernels: the Burg simplex prox at n = 1000 and n = 40000 (the multi-workgroup form), and the
    length-n reductions at n = 4097."""
    held = ()

    def host(self):
        rng = np.random.RandomState(4097)
        out = {}
        for n in (1000, 40000):
            out["y%d" % n] = _simplex_point(rng, n)
            out["g%d" % n] = rng.randn(n)
        out["g"] = rng.randn(4097)
        out["x"] = _simplex_point(rng, 4097)
        out["y"] = _simplex_point(rng, 4097)
        return out

    def make(self, acc, inp):
        return acc.BurgEntropySimplex()

    def use(self, acc, h, inp):
        from accbpg_and_fw_amd.functions import ls_terms, shannon_ls_terms, vec_argminmax
        o = _Out()
        for n in (1000, 40000):
            o.add("BurgEntropySimplex.div_prox_map n=%d" % n, h.div_prox_map(inp["y%d" % n], inp["g%d" % n], 1.0))
        o.add("ls_terms", ls_terms(inp["g"], inp["x"], inp["y"]))
        o.add("vec_argminmax", vec_argminmax(inp["g"]))
        o.add("shannon_ls_terms", shannon_ls_terms(inp["g"], inp["x"], inp["y"]))
        return o.items


SUBJECTS = {c.__name__: c() for c in (S1, S2, S3, S4, S5, S6, S7)}
NAMES = sorted(SUBJECTS)


def _fresh(masters):
    """The inputs of a run, produced by device copies on the current stream (the last thing enqueued before make())."""
    return {k: torch.empty_like(v).copy_(v) for k, v in masters.items()}


def _run_quiet(acc, subj, masters, timed):
    torch.cuda.synchronize()
    inp = _fresh(masters)
    objs = subj.make(acc, inp)
    runs, times = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        runs.append(subj.use(acc, objs, inp))
        times.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    return (runs, times) if timed else None


@pytest.fixture(scope="module")
def quiet(acc):
    """Mode Q of every subject -- its three use() calls as bytes, computed once and never changed -- the longest quiet
    use() of the module and the gate length that follows from it.  Every subject is run through once beforehand on
    objects that are thrown away, so that the times are those of the calls (first use of a fresh handle included) and
    not of loading the kernels' code objects."""
    torch.cuda.set_device(0)
    masters, ref, times = {}, {}, {}
    for name in NAMES:
        masters[name] = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
                         for k, v in SUBJECTS[name].host().items()}
    torch.cuda.synchronize()
    for name in NAMES:
        _run_quiet(acc, SUBJECTS[name], masters[name], False)
    for name in NAMES:
        ref[name], times[name] = _run_quiet(acc, SUBJECTS[name], masters[name], True)
    longest = max(max(t) for t in times.values())
    gate_ms = GATE_FACTOR * longest
    measured = sg.measure_gate(gate_ms)
    print("\nquiet use() times in ms (three calls each): "
          + "; ".join("%s %s" % (n, " ".join("%.2f" % t for t in times[n])) for n in NAMES))
    print("longest quiet use(): %.2f ms; gate asked for: %.1f ms; gate measured on an idle device: %.1f ms"
          % (longest, gate_ms, measured))
    probe = sg.independent_stream(_default())
    print("a stream that runs beside the gated default stream: found after passing over %d" % len(sg.rejected))
    del probe
    assert measured >= GATE_FACTOR * longest, (measured, longest)
    return {"masters": masters, "ref": ref, "gate_ms": gate_ms, "times": times}


def _default():
    return torch.cuda.default_stream()


# ---------------------------------------------------------------------------------------------------------------------
def test_gate_self_check_default_stream(acc, quiet):
    sg.check_default_stream_gate(quiet["gate_ms"])


def test_gate_self_check_own_stream(acc, quiet):
    sg.check_own_stream_gate(quiet["gate_ms"])


@pytest.mark.parametrize("name", NAMES)
def test_mode_q_quiet(acc, quiet, name):
    """The reference of A-D.  Its agreement with the oracle is what the other suites test; here: nothing of it is NaN,
    and a warm handle answers as the fresh one did (the kernels are deterministic)."""
    r1, r2, r3 = quiet["ref"][name]
    for label, b in r1:
        assert not np.isnan(np.frombuffer(b, dtype=np.float64)).any(), label    # (indices are small: no NaN pattern)
    _same(r2, r1, "%s second quiet use" % name)
    _same(r3, r1, "%s third quiet use" % name)


@pytest.mark.parametrize("name", NAMES)
def test_mode_a_fresh_stream_default_gated(acc, quiet, name):
    subj, masters, ref, ms = SUBJECTS[name], quiet["masters"][name], quiet["ref"][name], quiet["gate_ms"]
    s = sg.independent_stream(_default())
    end = sg.gate(_default(), ms)
    with torch.cuda.stream(s):
        inp = _fresh(masters)
        assert sg.pending(end), "the gate drained before make()"
        objs = subj.make(acc, inp)
        if not sg.pending(end):                                 # (create's blocking uploads wait for the null stream)
            end = sg.gate(_default(), ms)
        assert sg.pending(end), "the gate drained before use()"
        r1 = subj.use(acc, objs, inp)
        s.synchronize()                                         # ... and no device synchronisation
        r2 = subj.use(acc, objs, inp)
        torch.cuda.synchronize()
        r3 = subj.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "%s mode A first use" % name)
    _same(r2, ref[1], "%s mode A second use" % name)
    _same(r3, ref[2], "%s mode A third use" % name)


@pytest.mark.parametrize("name", NAMES)
def test_mode_b_inputs_late_on_own_stream(acc, quiet, name):
    """Two gates on s, one for each call under test.  create waits for its stream before it returns, so the first gate
    and the copies behind it have drained when make() is back; the inputs that use() reads (all but the ones the
    handles hold: ``held``) are therefore poisoned again and written again behind a second gate, which is pending when
    use() starts."""
    subj, masters, ref, ms = SUBJECTS[name], quiet["masters"][name], quiet["ref"][name], quiet["gate_ms"]
    late = [k for k in masters if k not in subj.held]
    assert late, name
    inp = {k: sg.poisoned(v.shape) for k, v in masters.items()}
    torch.cuda.synchronize()
    s = sg.independent_stream(_default())                       # (work that strays to the null stream runs ahead)
    end = sg.gate(s, ms)
    with torch.cuda.stream(s):
        for k, v in masters.items():
            inp[k].record_stream(s)
            inp[k].copy_(v)                                     # the real inputs, behind the gate
        assert sg.pending(end), "the gate drained before make()"
        objs = subj.make(acc, inp)
        s.synchronize()
        for k in late:
            sg.poison_(inp[k])
        s.synchronize()
        end = sg.gate(s, ms)
        for k in late:
            inp[k].copy_(masters[k])                            # ... and once more for use()
        assert sg.pending(end), "the gate drained before use()"
        r1 = subj.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "%s mode B" % name)


@pytest.mark.parametrize("name", NAMES)
def test_mode_c_create_on_one_stream_use_on_another(acc, quiet, name):
    subj, masters, ref, ms = SUBJECTS[name], quiet["masters"][name], quiet["ref"][name], quiet["gate_ms"]
    s1 = sg.independent_stream(_default())
    s2 = sg.independent_stream(s1, _default())
    end1 = sg.gate(s1, ms)
    with torch.cuda.stream(s1):
        inp = _fresh(masters)
        ready = torch.cuda.Event()
        ready.record(s1)                                        # the caller's own inputs, nothing of create
        assert sg.pending(end1), "the gate on s1 drained before make()"
        objs = subj.make(acc, inp)
    # twice as long: where make() did not wait for s1, the work of use() starts only when the gate on s1 has drained
    end0 = sg.gate(_default(), 2 * ms)
    with torch.cuda.stream(s2):
        s2.wait_event(ready)
        for v in inp.values():
            v.record_stream(s2)
        assert sg.pending(end0), "the default-stream gate drained before use()"
        r1 = subj.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "%s mode C" % name)


# ---------------------------------------------------------------------------------------------------------------------
# D: host threads, first use
def _thread_gate(quiet, quiet_ms):
    """The default-stream gate of a host-thread check: ten times the sequential leg, at least the module's gate."""
    return sg.gate(_default(), max(quiet["gate_ms"], GATE_FACTOR * quiet_ms))


def _report_beside(beside, what):
    """How many workers had their results on the host while the gate was still pending: printed, not asserted.  It is
    none, and by the code (not traced) not because of hardware queues: the first thing ABPG_gain does on a fresh objective is value_async, which
    creates the side handle, and create's blocking uploads of its plan tables wait for the null stream as every
    blocking hipMemcpy does.  So the gate holds each worker at its first create and the solver proper runs when the
    gate has drained: in mode D the gate delays, it does not race.  What D pins is first use from host threads on the
    package's own streams, bit for bit; the ordering cases are A, B and C."""
    print("\n%s: %d of %d workers finished while the default-stream gate was pending" % (what, sum(beside), len(beside)))


def test_mode_d_solve_batch_fresh_problems(acc, quiet):
    from accbpg_and_fw_amd.batched import solve_batch
    seq_probs = [acc.D_opt_design(96, 640, randseed=50 + j) for j in range(6)]
    t0 = time.perf_counter()
    seq = [acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=40, verbose=False) for f, h, L, x0 in seq_probs]
    quiet_ms = 1e3 * (time.perf_counter() - t0)
    probs = [acc.D_opt_design(96, 640, randseed=50 + j) for j in range(6)]      # never evaluated
    gate_end, beside = [], []

    def solver(f, h, L, x0, **kwargs):
        out = acc.ABPG_gain(f, h, L, x0, **kwargs)              # (NumPy x0: the results are on the host when it returns)
        beside.append(sg.pending(gate_end[0]))
        return out

    torch.cuda.synchronize()
    gate_end.append(_thread_gate(quiet, quiet_ms))
    assert sg.pending(gate_end[0]), "the gate drained before solve_batch"
    par = solve_batch(probs, solver, threads=6, gamma=2, maxitrs=40, verbose=False)
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(seq, par)):
        for k, what in enumerate(("x", "F", "Gain")):
            assert _bytes(a[k]) == _bytes(b[k]), "instance %d: %s differs from the sequential run" % (j, what)
    _report_beside(beside, "solve_batch (sequential leg %.1f ms)" % quiet_ms)


def test_mode_d_batch_stepper_fresh_generators(acc, quiet):
    from accbpg_and_fw_amd.algorithms import ABPG_gain_steps
    from accbpg_and_fw_amd.batched import BatchStepper

    def two_steps(prob, box, j, done):
        """Two outer iterations in two steps; the second step also ends the run (maxitrs = 2) and keeps its result."""
        gen = ABPG_gain_steps(*prob, gamma=2, maxitrs=2, verbose=False)
        yield next(gen)
        next(gen)
        try:
            next(gen)
        except StopIteration as stop:
            box[j] = stop.value
        else:
            raise AssertionError("the generator went on past maxitrs")
        done(j)
        yield None

    def problems():
        return [acc.D_opt_design(96, 640, randseed=60 + j) for j in range(4)]

    seq = [None] * 4
    t0 = time.perf_counter()
    for j, prob in enumerate(problems()):
        gen = two_steps(prob, seq, j, lambda j: None)
        next(gen); next(gen)
    quiet_ms = 1e3 * (time.perf_counter() - t0)

    par, gate_end, beside = [None] * 4, [], []
    makers = [(lambda p=p, j=j: two_steps(p, par, j, lambda j: beside.append(sg.pending(gate_end[0]))))
              for j, p in enumerate(problems())]
    stepper = BatchStepper(makers, torch.device("cuda", torch.cuda.current_device()), threads=4)
    torch.cuda.synchronize()
    gate_end.append(_thread_gate(quiet, quiet_ms))
    assert sg.pending(gate_end[0]), "the gate drained before the first step()"
    try:
        stepper.step()
        stepper.step()
    finally:
        stepper.close()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(seq, par)):
        for k, what in enumerate(("x", "F", "Gain")):
            assert _bytes(a[k]) == _bytes(b[k]), "instance %d: %s differs from sequential stepping" % (j, what)
    _report_beside(beside, "BatchStepper (sequential leg %.1f ms)" % quiet_ms)
    print("streams passed over in this module because they stood still behind a gated stream: %d" % len(sg.rejected))
