"""build_plans plans on the host (csrc/dopt_plan.hpp) and uploads what the planners return.  One evaluation per upload
path -- small tiles with edges, the D-stride XCD order, aligned ranges, whole tiles, two column blocks of a long row,
and a batch with its capped grid and its op tables -- gives f and g of func_grad(x, 2) bit for bit as the commit before
the planner moved did (tests/golden/plan_parity_parent.npz, written from that commit's library by
tools/gen_plan_parity_golden.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import plan_cases as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def lib(acc):
    from accbpg_and_fw_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "plan_parity_parent.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", P.PARITY_CASES, ids=[P.parity_name(c) for c in P.PARITY_CASES])
def test_func_grad_bits_equal_the_parents(acc, lib, parent, case):
    mine = P.parity_record(case, P.parity_evaluate(acc, lib, case))
    assert len(mine) == 4 * case[2]
    for k in sorted(mine):
        print(k, mine[k] if mine[k].size <= 1 else mine[k][:2])
        assert np.array_equal(mine[k], parent[k]), k
