"""First use and ordering of accbpg_fw_direction and of the carried-margin entries of the logistic handle
(line_begin, line_value, line_accept, func_grad_carried) on non-default streams, and of a whole carried solve, on the
model of tests/test_gpu_stream_logistic.py with the gates of tests/stream_gate.py.

``make()`` builds fresh objects from device inputs, ``use()`` runs the entry points and returns every result as host
bytes.  The subject is run quietly on the default stream (mode Q, the reference) and then

  A  first use on a fresh non-blocking stream with the default stream gated, then again after ``s.synchronize()`` only,
     then after a device synchronisation;
  B  inputs poisoned, then written late on the call's own stream behind a gate on that stream, before ``make()`` and once
     more before ``use()``;
  C  ``make()`` on a gated stream s1, ``use()`` on a second fresh stream with the default stream gated as well.

Every comparison is bit for bit against mode Q.  A gate lasts ten times the longest quiet ``use()``, and every gated
case asserts that its gate is still pending immediately before the call under test."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_gate as sg  # noqa: E402

GATE_FACTOR = 10


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _bytes(v):
    """A result as host bytes.  A device tensor is consumed with a clone on the current stream before any host wait."""
    if isinstance(v, torch.Tensor):
        return v.clone().cpu().numpy().tobytes()
    if isinstance(v, (tuple, list)):
        return b"".join(_bytes(e) for e in v)
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes()


def _same(got, ref, what):
    assert [l for l, _ in got] == [l for l, _ in ref], what
    for (label, a), (_, b) in zip(got, ref):
        if a != b:
            x, y = np.frombuffer(a, dtype=np.uint64), np.frombuffer(b, dtype=np.uint64)
            bad = np.flatnonzero(x != y) if x.size == y.size else np.arange(0)
            pytest.fail("%s: %s differs from the quiet run (%d of %d words)" % (what, label, bad.size, y.size))


class Subject:
    """fw_direction with the three oracles at n = 4097 (an array centre for the l2 ball), the line entries of
    LogisticRegression at (33, 130) (a wavefront per row) and (5, 4097) (a workgroup per row), and six iterations of
    FW_l0l1_log_and_linear_step with carried margins"""
    held = ("A1", "y1", "A2", "y2", "c")                        # inputs the objects keep reading

    def host(self):
        rng = np.random.RandomState(4131)
        A1, A2 = rng.randn(33, 130), rng.randn(5, 4097)
        return {"A1": A1, "y1": np.sign(A1 @ rng.randn(130) + 0.1), "x1": 0.1 * rng.randn(130),
                "d1": 0.1 * rng.randn(130), "A2": A2, "y2": np.sign(A2 @ rng.randn(4097) + 0.1),
                "x2": 0.02 * rng.randn(4097), "d2": 0.02 * rng.randn(4097), "g": rng.randn(4097),
                "c": 0.3 * rng.randn(4097)}

    def make(self, acc, inp):
        return {"f1": acc.LogisticRegression(inp["A1"], inp["y1"]), "f2": acc.LogisticRegression(inp["A2"], inp["y2"]),
                "l2": acc.lmo_l2_ball(1.5, inp["c"]), "linf": acc.lmo_linf_ball(0.5), "simplex": acc.lmo_simplex()}

    def use(self, acc, d, inp):
        items = []

        def add(label, value):
            items.append((label, _bytes(value)))
            return value

        for name in ("l2", "linf", "simplex"):
            add("fw_direction " + name, acc.fw_direction(d[name], inp["g"], inp["x2"])[:6])
        for k in ("1", "2"):
            f, x, dv = d["f" + k], inp["x" + k], inp["d" + k]
            add("f%s func_grad(x,2)" % k, f.func_grad(x, 2))
            f.line_begin(dv)
            add("f%s line_value" % k, (f.line_value(1.0), f.line_value(0.25)))
            f.line_accept(0.25)
            add("f%s rows" % k, (f.fitted(), f.losses(), f.weights()))
            add("f%s carried" % k, f.func_grad_carried(2))
            add("f%s carried flags" % k, (f.func_grad_carried(0), f.func_grad_carried(1)))
        out = acc.FW_l0l1_log_and_linear_step(d["f1"], acc.SquaredL2Norm(), 1e-3, 10.0, inp["x1"], 6, d["linf"], 2.0,
                                              verbose=False, carry=True, refresh=4)
        add("carried solve", (out[0], out[1], out[2], out[3].astype(np.float64)))
        return items


SUBJ = Subject()


def _fresh(masters):
    return {k: torch.empty_like(v).copy_(v) for k, v in masters.items()}


def _default():
    return torch.cuda.default_stream()


def _run_quiet(acc, masters, timed):
    torch.cuda.synchronize()
    inp = _fresh(masters)
    objs = SUBJ.make(acc, inp)
    runs, times = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        runs.append(SUBJ.use(acc, objs, inp))
        times.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    return (runs, times) if timed else None


@pytest.fixture(scope="module")
def quiet(acc):
    torch.cuda.set_device(0)
    masters = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda() for k, v in SUBJ.host().items()}
    torch.cuda.synchronize()
    _run_quiet(acc, masters, False)                             # (loads the kernels' code objects)
    ref, times = _run_quiet(acc, masters, True)
    gate_ms = GATE_FACTOR * max(times)
    measured = sg.measure_gate(gate_ms)
    print("\nquiet use() times in ms: %s; gate asked for %.1f ms, measured %.1f ms"
          % (" ".join("%.2f" % t for t in times), gate_ms, measured))
    assert measured >= gate_ms, (measured, gate_ms)
    return {"masters": masters, "ref": ref, "gate_ms": gate_ms}


def test_mode_q_quiet(acc, quiet):
    r1, r2, r3 = quiet["ref"]
    for label, b in r1:
        assert not np.isnan(np.frombuffer(b, dtype=np.float64)).any(), label
    _same(r2, r1, "second quiet use")
    _same(r3, r1, "third quiet use")


def test_mode_a_fresh_stream_default_gated(acc, quiet):
    masters, ref, ms = quiet["masters"], quiet["ref"], quiet["gate_ms"]
    s = sg.independent_stream(_default())
    end = sg.gate(_default(), ms)
    with torch.cuda.stream(s):
        inp = _fresh(masters)
        assert sg.pending(end), "the gate drained before make()"
        objs = SUBJ.make(acc, inp)
        if not sg.pending(end):
            end = sg.gate(_default(), ms)
        assert sg.pending(end), "the gate drained before use()"
        r1 = SUBJ.use(acc, objs, inp)
        s.synchronize()
        r2 = SUBJ.use(acc, objs, inp)
        torch.cuda.synchronize()
        r3 = SUBJ.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "mode A first use")
    _same(r2, ref[1], "mode A second use")
    _same(r3, ref[2], "mode A third use")


def test_mode_b_inputs_late_on_own_stream(acc, quiet):
    masters, ref, ms = quiet["masters"], quiet["ref"], quiet["gate_ms"]
    late = [k for k in masters if k not in SUBJ.held]
    inp = {k: sg.poisoned(v.shape) for k, v in masters.items()}
    torch.cuda.synchronize()
    s = sg.independent_stream(_default())
    end = sg.gate(s, ms)
    with torch.cuda.stream(s):
        for k, v in masters.items():
            inp[k].record_stream(s)
            inp[k].copy_(v)                                     # the real inputs, behind the gate
        assert sg.pending(end), "the gate drained before make()"
        objs = SUBJ.make(acc, inp)
        s.synchronize()
        for k in late:
            sg.poison_(inp[k])
        s.synchronize()
        end = sg.gate(s, ms)
        for k in late:
            inp[k].copy_(masters[k])                            # ... and once more for use()
        assert sg.pending(end), "the gate drained before use()"
        r1 = SUBJ.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "mode B")


def test_mode_c_create_on_one_stream_use_on_another(acc, quiet):
    masters, ref, ms = quiet["masters"], quiet["ref"], quiet["gate_ms"]
    s1 = sg.independent_stream(_default())
    s2 = sg.independent_stream(s1, _default())
    end1 = sg.gate(s1, ms)
    with torch.cuda.stream(s1):
        inp = _fresh(masters)
        ready = torch.cuda.Event()
        ready.record(s1)                                        # the caller's own inputs, nothing of create
        assert sg.pending(end1), "the gate on s1 drained before make()"
        objs = SUBJ.make(acc, inp)
    end0 = sg.gate(_default(), 2 * ms)
    with torch.cuda.stream(s2):
        s2.wait_event(ready)
        for v in inp.values():
            v.record_stream(s2)
        assert sg.pending(end0), "the default-stream gate drained before use()"
        r1 = SUBJ.use(acc, objs, inp)
    torch.cuda.synchronize()
    _same(r1, ref[0], "mode C")
