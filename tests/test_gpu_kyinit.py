"""GPU tests of the device Kumar-Yildirim start (accbpg_dopt_kyinit, D_opt_KYinit_device).

Free of tolerance and of margin: the call is replayed by tests/ky_numpy.py with the device's own accbpg_dopt_vt_times as
the pass over V.  The replay's q is then bit-identical to the device's at every step (same summation order of the dots,
same order of the subtractions), its w are the device's bits, and np.argmax / np.argmin on them are the device's
decisions: `picked` must be equal step by step and Q bit for bit, ties or not.

The comparison with D_opt_KYinit (np.dot coefficients on the host) holds only where no decision is within rounding of a
tie; it is made on the four instances whose smallest gap tests/test_kyinit_cpu.py pins (>= 3.8e-6)."""
import ctypes as C

import numpy as np
import pytest

import ky_numpy
from conftest import golden, gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (m, n): smallest sizes (step 0 alone; a deflation loop of one) | wave seam of the dots | 256-thread block seam over
# rows | arg-extremum one-block / two-block seam at 1024 entries | its 128-block cap (131072 entries) | general
SHAPES = [(1, 3), (2, 5), (63, 200), (64, 200), (65, 200), (257, 2100), (8, 1024), (8, 1025), (8, 132100), (130, 1030)]
INSTANCES = [(30, 1000, 4, 99), (65, 700, 6, 8), (130, 1030, 3, 11), (257, 2100, 2, 12)]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _data(m, n):
    rng = np.random.RandomState(1000 * m + n)
    return rng.randn(m, n), rng.rand(m, m)


def _padded_obj(acc, V, pad):
    """a DOptimalObj over V stored with row stride n + pad (handles are created that way through the C-ABI only)"""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n = V.shape
    store = torch.full((m, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    store[:, :n] = torch.from_numpy(V).cuda()
    h = C.c_void_p()
    rc = lib.accbpg_dopt_create(C.c_void_p(store.data_ptr()), m, n, n + pad, None, C.byref(h), 0)
    assert rc == 0, _lib.last_error()

    class Owner:
        def __del__(self, lib=lib, h=h, store=store):
            lib.accbpg_dopt_destroy(h)
    return acc.DOptimalObj(V, _borrowed=(h, Owner()))


def _run_and_replay(acc, f, V, B):
    m = V.shape[0]
    Qd = torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda")
    picked = f.kyinit_picks(B, Q_out=Qd)
    Q = Qd.cpu().numpy().T                                      # row j of the device array = Q[:, j]
    steps = []
    rp, rQ, rx0 = ky_numpy.kyinit(V, B, vt_times=lambda q: f.vt_times(q).cpu().numpy(), steps=steps)
    return picked, Q, rp, rQ, steps


def _check(picked, Q, rp, rQ):
    bad = np.nonzero(picked != rp)[0]
    assert bad.size == 0, "first differing pick at step %d (%s): device %d, replay %d" % (
        bad[0] // 2, "kmin" if bad[0] & 1 else "kmax", picked[bad[0]], rp[bad[0]])
    np.testing.assert_array_equal(Q, rQ)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_replay_is_bit_identical(acc, shape):
    m, n = shape
    V, B = _data(m, n)
    f = acc.DOptimalObj(V)
    picked, Q, rp, rQ, steps = _run_and_replay(acc, f, V, B)
    _check(picked, Q, rp, rQ)
    assert np.all(np.isfinite(Q))
    if m >= 2:
        assert np.max(np.abs(Q.T @ Q - np.eye(m))) < 1e-10      # the directions are orthonormal (sanity, not the check)


def test_replay_with_padded_rows(acc):
    """ldv > n, with aligned rows (the vector-load path of the pass over V) under an odd n; the padding holds NaN and
    must never be read"""
    m, n = 33, 777
    V, B = _data(m, n)
    f = _padded_obj(acc, V, 5)
    picked, Q, rp, rQ, steps = _run_and_replay(acc, f, V, B)
    _check(picked, Q, rp, rQ)
    assert np.all(np.isfinite(Q))


@pytest.mark.parametrize("layout", ["halves", "interleaved"])
def test_planted_ties_pick_the_first_of_a_pair(acc, layout):
    """every column twice: each arg-extremum is an exact tie, and the first index must win at every stage of the merge"""
    m, n0 = 16, 1030
    V0, B = _data(m, n0)
    V = np.concatenate([V0, V0], axis=1) if layout == "halves" else np.repeat(V0, 2, axis=1)
    V = np.ascontiguousarray(V)
    f = acc.DOptimalObj(V)
    picked, Q, rp, rQ, steps = _run_and_replay(acc, f, V, B)
    _check(picked, Q, rp, rQ)
    for q, w in steps:                                          # the ties are exact on the device too
        twin = w.reshape(2, n0) if layout == "halves" else w.reshape(n0, 2).T
        np.testing.assert_array_equal(twin[0], twin[1])
    if layout == "halves":
        assert np.all(picked < n0)
    else:
        assert np.all(picked % 2 == 0)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def starts(acc):
    """per instance: the objective, the host start and the device start under the same seed, the generator after each"""
    out = {}
    for m, n, seed, rs in INSTANCES:
        V = gaussian_design(m, n, seed)
        f = acc.DOptimalObj(V)
        np.random.seed(rs)
        x_host = acc.D_opt_KYinit(f)
        s_host = np.random.get_state()
        np.random.seed(rs)
        x_dev, picked = acc.D_opt_KYinit_device(f, return_picked=True)
        s_dev = np.random.get_state()
        out[(m, n)] = dict(V=V, f=f, x_host=x_host, x_dev=x_dev, picked=picked, s_host=s_host, s_dev=s_dev, rs=rs)
    return out


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda t: "%dx%d" % t[:2])
def test_device_start_equals_host_start(acc, starts, inst):
    c = starts[inst[:2]]
    np.testing.assert_array_equal(c["x_dev"], c["x_host"])
    assert c["s_dev"][0] == c["s_host"][0] and np.array_equal(c["s_dev"][1], c["s_host"][1]) \
        and c["s_dev"][2:] == c["s_host"][2:]
    assert c["picked"].shape == (2 * inst[0],)
    np.testing.assert_array_equal(c["x_dev"], ky_numpy.x0_from_picked(c["picked"], inst[1]))


def test_device_start_equals_reference_golden_and_feeds_fw_away(acc, starts):
    gd = golden("next_rows")
    c = starts[(30, 1000)]
    np.testing.assert_array_equal(c["x_dev"], gd["ky_x"])
    np.random.seed(c["rs"])
    np.testing.assert_array_equal(acc.D_opt_KYinit_device(c["V"]), gd["ky_x"])      # an array as well as the objective
    xs, F, SP, SN, T = acc.D_opt_FW_away(c["V"], c["x_dev"], 1e-8, 2000, verbose=False)
    k = min(len(F), len(gd["ky_away_F"]))
    assert abs(len(F) - len(gd["ky_away_F"])) <= 2
    np.testing.assert_allclose(F[:k], gd["ky_away_F"][:k], rtol=1e-8, atol=1e-8)
    assert np.max(np.abs(xs - gd["ky_away_x"])) < 1e-8


def test_repeated_calls_are_bit_identical_and_leave_the_objective_alone(acc, starts):
    c = starts[(65, 700)]
    f, n = c["f"], 700
    x = np.random.RandomState(2).rand(n)
    x /= x.sum()
    f0, g0 = f.func_grad(x, 2)
    m = 65
    B = np.random.RandomState(3).rand(m, m)
    Q1 = torch.empty((m, m), dtype=torch.float64, device="cuda")
    Q2 = torch.empty((m, m), dtype=torch.float64, device="cuda")
    p1 = f.kyinit_picks(B, Q_out=Q1)
    f1, g1 = f.func_grad(x, 2)
    p2 = f.kyinit_picks(B, Q_out=Q2)
    p3 = f.kyinit_picks(B)                                      # the call's own Q
    np.testing.assert_array_equal(p1, p2)
    np.testing.assert_array_equal(p1, p3)
    assert torch.equal(Q1, Q2)
    assert f1 == f0
    np.testing.assert_array_equal(g1, g0)
    np.random.seed(c["rs"])
    np.testing.assert_array_equal(acc.D_opt_KYinit_device(f), c["x_dev"])
    np.testing.assert_array_equal(acc.D_opt_KYinit_device(np.zeros((30, 60))), np.ones(60) / 60)


def test_null_arguments_are_refused(acc, starts):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    f = starts[(30, 1000)]["f"]
    m = 30
    B = torch.zeros((m, m), dtype=torch.float64, device="cuda")
    picked = (C.c_int64 * (2 * m))()
    assert lib.accbpg_dopt_kyinit(None, C.c_void_p(B.data_ptr()), picked, None) == _lib.ERR_ARG
    assert lib.accbpg_dopt_kyinit(f._h, None, picked, None) == _lib.ERR_ARG
    assert lib.accbpg_dopt_kyinit(f._h, C.c_void_p(B.data_ptr()), None, None) == _lib.ERR_ARG
    with pytest.raises(AssertionError):
        f.kyinit_picks(np.zeros((m, m + 1)))
