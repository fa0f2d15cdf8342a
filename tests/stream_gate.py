"""Gates: work put on a chosen stream that keeps it busy for a known time (torch only, no library code).

A test that wants to know whether a call orders its own work cannot wait for a race to happen; it makes the race
certain.  ``gate(stream, ms)`` enqueues one spin kernel (``torch.cuda._sleep``: a single thread that watches the
clock, so the gate takes no compute units or bandwidth away from the work under test) on ``stream`` and returns an
event recorded behind it.  Whatever is enqueued on that stream afterwards runs only when the gate has drained, while
every other non-blocking stream goes on: a fill, copy or launch that the call under test puts on the gated stream by
mistake lands late, after the kernels that needed it (or that it then overwrites), and the result differs by far more
than a bit.  ``pending(end)`` is the condition every gated case asserts immediately before the call under test: a gate
that has already drained proves nothing, and such a case fails instead of passing vacuously.  The streams of a gated
case come from ``independent_stream``: streams share the few hardware queues of a process, and one that shares its
queue with the gated stream would stand still behind the gate.

The two self-checks at the bottom are what tests/test_gpu_stream_first_use.py runs first: they touch no library code
and show that the gates model the two hazards (a stream that does not wait for the null stream; a reader on another
stream that does not wait for the writer's)."""
import numpy as np
import torch

POISON_BITS = 0x7FF8DEADBEEF0BAD            # a quiet NaN with a payload nobody computes by accident
POISON = np.array([POISON_BITS], dtype=np.uint64).view(np.float64)[0]

_cycles_per_ms = {}


def poison_(t):
    """Fill the fp64 tensor t with the poison pattern, on the current stream."""
    t.view(torch.int64).fill_(POISON_BITS)
    return t


def poisoned(shape, device="cuda"):
    return poison_(torch.empty(shape, dtype=torch.float64, device=device))


def is_poison(host_array):
    a = np.ascontiguousarray(host_array, dtype=np.float64).view(np.uint64)
    return bool(np.all(a == np.uint64(POISON_BITS)))


def calibrate(device=None):
    """Spin-kernel cycles per millisecond on this device, measured once with events (two lengths, so that the launch
    overhead cancels)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    if dev not in _cycles_per_ms:
        with torch.cuda.device(dev):
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)                             # (first launch: code object load)
            times = []
            for cycles in (2_000_000, 10_000_000):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            slope = (times[1] - times[0]) / 8_000_000           # ms per cycle
            assert slope > 0, times
            _cycles_per_ms[dev] = 1.0 / slope
    return _cycles_per_ms[dev]


def gate(stream, ms):
    """Keep `stream` busy for at least `ms` milliseconds from the moment the gate starts to run; returns the event
    recorded behind it."""
    cycles = int(ms * calibrate(stream.device) * 1.05) + 1      # (5% over: the calibration is a measurement)
    end = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        end.record(stream)
    return end


def pending(end):
    """The gate has not drained yet (a condition, not a measurement)."""
    return not end.query()


rejected = []          # streams independent_stream() passed over, as (candidate, busy stream) handles: for the test output


def independent_stream(*busy, probe_ms=10.0, tries=32):
    """A stream whose work demonstrably runs while each of the streams `busy` is held by a gate.

    A process has far fewer hardware queues than streams (four by default), the runtime deals its streams out over
    them, and a hardware queue runs its packets in order: a stream that shares its queue with a gated stream stands
    still behind the gate although nothing orders the two.  Work under test on such a stream would be ordered by
    accident and every case would pass without testing anything (it can never fail for it).  So the streams of a gated
    case are chosen: each candidate (torch hands its pool out in turn) gets one tiny kernel while a short probe gate
    holds a busy stream, and is taken when that kernel has finished with the probe still pending."""
    dev = torch.device("cuda", torch.cuda.current_device())
    word = torch.zeros(1, dtype=torch.float64, device=dev)
    for _ in range(tries):
        cand = torch.cuda.Stream()
        if any(cand.cuda_stream == b.cuda_stream for b in busy):
            continue
        free = True
        for b in busy:
            torch.cuda.synchronize()
            end = gate(b, probe_ms)
            with torch.cuda.stream(cand):
                word.add_(1.0)
            cand.synchronize()
            free = pending(end)
            end.synchronize()
            if not free:
                rejected.append((cand.cuda_stream, b.cuda_stream))
                break
        if free:
            torch.cuda.synchronize()
            return cand
    raise AssertionError("no stream of %d runs while %s is gated" % (tries, [hex(b.cuda_stream) for b in busy]))


def measure_gate(ms):
    """How long a gate of `ms` lasts on an idle device, in ms by events (what the tests print beside the quiet time)."""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    start.record(s)
    end = gate(s, ms)
    end.synchronize()
    return start.elapsed_time(end)


# ---------------------------------------------------------------------------------------------------------------------
# self-checks (pure torch)
def check_default_stream_gate(ms):
    """(a) A side stream does not wait for the null stream, and the gate delays the null stream: poison written on s,
    the default stream gated and then told to clear the tensor, a clone taken on s still holds the poison."""
    dev = torch.device("cuda", torch.cuda.current_device())
    s = independent_stream(torch.cuda.default_stream())
    with torch.cuda.stream(s):
        t = poisoned(4096, dev)
    s.synchronize()
    torch.cuda.synchronize()
    end = gate(torch.cuda.default_stream(), ms)
    assert pending(end), "the default-stream gate drained before the clear was issued"
    t.zero_()                                                   # on the default stream, behind the gate
    with torch.cuda.stream(s):
        seen = t.clone()
    s.synchronize()
    still = pending(end)
    seen_host = seen.cpu().numpy()
    torch.cuda.synchronize()
    after = t.cpu().numpy()
    assert still, "the default-stream gate drained before the side stream had read"
    assert is_poison(seen_host), "the side stream waited for the null stream (or the gate did not hold the clear back)"
    assert np.all(after == 0.0), "the clear never ran"


def check_own_stream_gate(ms):
    """(b) A gate on s delays a write issued on s: a second non-blocking stream that does not wait reads the poison,
    a read on s sees the written values."""
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.Stream()
    other = independent_stream(s)
    x = poisoned(4096, dev)
    src = torch.arange(4096, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    end = gate(s, ms)
    assert pending(end), "the gate on s drained before the write was issued"
    with torch.cuda.stream(s):
        x.copy_(src)                                            # behind the gate
    with torch.cuda.stream(other):
        early = x.clone()                                       # no wait for s
    other.synchronize()
    still = pending(end)
    with torch.cuda.stream(s):
        ordered = x.clone()
    s.synchronize()
    early_host, ordered_host = early.cpu().numpy(), ordered.cpu().numpy()
    torch.cuda.synchronize()
    assert still, "the gate on s drained before the other stream had read"
    assert is_poison(early_host), "a stream that did not wait saw the write behind the gate"
    assert np.array_equal(ordered_host, np.arange(4096, dtype=np.float64)), "a read on s did not see the write on s"
