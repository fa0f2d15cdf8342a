"""``ABPG_expo_batch`` and ``ABDA_batch``: the K instances of a ``DOptimalBatch`` in lock-step.  Every instance's run --
iterates, F, the exponent sequence with its lowerings, the gains -- is bit-identical (T apart) to the sequential solver
on ``batch.instance(i)``: the host decisions are one copy (solver_runs._ExpoRun / _ABDARun), the kernels are the
instance's own, and ABDA's three launches per step (sum, quotient, prox) are one launch of ``avg_prox`` with the same
roundings.  Instances lower their exponents and stop at different iterations, so the passes do run on proper subsets."""
import numpy as np
import pytest

from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


_BATCHES = {}


def batch_of(acc, m, n, K, seed, stride):
    key = (m, n, K, seed, stride)
    if key not in _BATCHES:
        _BATCHES.clear()                                        # (the cases of one batch follow each other)
        _BATCHES[key] = acc.DOptimalBatch([gaussian_design(m, n, seed + stride * i) for i in range(K)])
    return _BATCHES[key]


def expo_batch(acc, m, n, K):
    return batch_of(acc, m, n, K, 700, 13)


def abda_batch(acc, m, n, K):
    return batch_of(acc, m, n, K, 900, 17)


def same_as_sequential(outs, refs, records):
    assert len(outs) == len(refs)
    for out, ref in zip(outs, refs):
        assert len(out) == len(ref) == records + 2
        for got, want in zip(out[:-1], ref[:-1]):
            np.testing.assert_array_equal(got, want)
        assert len(out[-1]) == len(ref[-1])


def run_expo(acc, batch, gamma0, iters, **opts):
    h = acc.BurgEntropySimplex()
    x0 = np.ones(batch.n) / batch.n
    outs = acc.ABPG_expo_batch(batch, h, 1.0, x0, gamma0, iters, **opts)
    opts.pop("overlap", None)
    refs = [acc.ABPG_expo(batch.instance(i), h, 1.0, x0, gamma0, iters, verbose=False, **opts) for i in range(batch.K)]
    same_as_sequential(outs, refs, 3)
    return outs


def run_abda(acc, batch, gamma, iters, **opts):
    h = acc.BurgEntropySimplex()
    x0 = np.ones(batch.n) / batch.n
    outs = acc.ABDA_batch(batch, h, 1.0, x0, gamma, iters, **opts)
    opts.pop("overlap", None)
    refs = [acc.ABDA(batch.instance(i), h, 1.0, x0, gamma, iters, verbose=False, **opts) for i in range(batch.K)]
    same_as_sequential(outs, refs, 2)
    return outs


@pytest.mark.parametrize("shape,K,gamma0,opts,differ", [
    ((256, 1024), 5, 3, dict(theta_eq=True), True),
    ((256, 1024), 3, 3, dict(theta_eq=False, delta=0.5, restart=True), True),
    ((256, 1024), 4, 3, dict(checkdiv=True, Gmargin=3), True),
    # three lowerings inside one outer iteration; every instance lowers alike (2.5 -> 1.9 at k = 2)
    ((256, 2048), 4, 2.5, dict(theta_eq=False, checkdiv=True, Gmargin=1, restart=True, restart_rule='f'), False)])
def test_lockstep_expo_matches_sequential(acc, shape, K, gamma0, opts, differ):
    batch = expo_batch(acc, *shape, K)
    assert batch.fused
    outs = run_expo(acc, batch, gamma0, 45, **opts)
    patterns = {tuple(out[2]) for out in outs}
    if differ:
        assert len(patterns) > 1                                # the instances did not all lower alike


@pytest.mark.parametrize("theta_eq", [True, False])
def test_lockstep_abda_matches_sequential(acc, theta_eq):
    batch = abda_batch(acc, 256, 1024, 4)
    assert batch.fused
    outs = run_abda(acc, batch, 2, 30, theta_eq=theta_eq)
    assert all(len(out[1]) == 30 for out in outs)
    assert len({tuple(out[1]) for out in outs}) == 4            # four different problems


def test_early_stops_expo(acc):
    """epsilon = 2e-2: every instance stops where its sequential run stops, and not all at one iteration -- the later
    passes run without the instances that are done."""
    outs = run_expo(acc, expo_batch(acc, 256, 1024, 5), 3, 60, epsilon=2e-2)
    lengths = [len(out[1]) for out in outs]
    assert len(set(lengths)) > 1, lengths


def test_early_stops_abda(acc):
    outs = run_abda(acc, abda_batch(acc, 256, 1024, 4), 2, 60, epsilon=2e-2)
    lengths = [len(out[1]) for out in outs]
    assert len(set(lengths)) > 1, lengths


def test_overlap_off_gives_the_same_bits(acc):
    batch = expo_batch(acc, 256, 1024, 3)
    on = run_expo(acc, batch, 3, 20, theta_eq=False, delta=0.5, restart=True)
    off = run_expo(acc, batch, 3, 20, theta_eq=False, delta=0.5, restart=True, overlap=False)
    same_as_sequential(off, on, 3)
    batch = abda_batch(acc, 256, 1024, 4)
    on = run_abda(acc, batch, 2, 20)
    off = run_abda(acc, batch, 2, 20, overlap=False)
    same_as_sequential(off, on, 2)


@pytest.mark.parametrize("shape,K,iters,fused", [((96, 640), 4, 30, False),      # outside the fused path
                                                 ((8, 40000), 2, 5, False),      # long rows: the composition, per instance
                                                 ((256, 512), 1, 30, True)])
def test_other_paths_both_solvers(acc, shape, K, iters, fused):
    batch = expo_batch(acc, *shape, K)
    assert batch.fused == fused
    run_expo(acc, batch, 3, iters)
    batch = abda_batch(acc, *shape, K)
    run_abda(acc, batch, 2, iters)


def test_device_iterates_stay_on_the_device(acc):
    batch = abda_batch(acc, 256, 1024, 4)
    h = acc.BurgEntropySimplex()
    x0 = torch.full((batch.n,), 1.0 / batch.n, dtype=torch.float64, device="cuda")
    for out in acc.ABDA_batch(batch, h, 1.0, x0, 2, 3) + acc.ABPG_expo_batch(batch, h, 1.0, x0, 3, 3):
        assert isinstance(out[0], torch.Tensor) and out[0].is_cuda and out[0].shape == (batch.n,)
