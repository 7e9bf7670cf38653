"""The cases of tests/_handover_cases.py without a GPU: does every case do what the GPU tests rely on?  From the
oracle alone (the pattern of tests/test_gcp_truth_cpu.py), so that tests/test_gpu_handover.py cannot pass on walks that
cross nothing:

  * along the oracle's trajectory at least `served` iterations have a walk that crosses 1 .. 16 breakpoints
    (1 <= nseg - 1 <= 16: short enough for the hand-over's list), at least `served7` of them with col >= 7, where the
    free-row layout sends the update pass to the pair-shared instantiation.  (`served` is what a CPU model of the
    host's rule predicts to be handed over; the crossing iterations are a superset of those.)
  * every row such a walk fixed (iwhere 0 -> 1 / 2 across the call) is one of the case's bounded rows, and where
    n % 128 != 0 lies behind the last whole layout tile of its rank -- the rows a hand-over from whole tiles alone
    would miss.
"""
import numpy as np
import pytest

import _handover_cases as hc


@pytest.mark.parametrize("case", hc.CASES, ids=[c.name for c in hc.CASES])
def test_walks_cross_breakpoints_in_the_chosen_rows(oracle_built, case):
    walks = hc.oracle_walks(oracle_built, case)
    short = [w for w in walks if 1 <= w[2] - 1 <= 16]
    print("\n%-10s walks %2d crossing 1..16: %2d (col >= 7: %2d) at iterations %s"
          % (case.name, len(walks), len(short), sum(w[1] >= 7 for w in short), [w[0] for w in short]))
    assert len(short) >= case.served, (len(short), case.served)
    assert sum(w[1] >= 7 for w in short) >= case.served7
    seen = 0
    for it, col, nseg, rows in short:
        assert np.all(case.bounded[rows]), (it, rows)
        if case.tail:
            assert np.all(rows >= case.tile0[rows]), (it, rows)
        seen += rows.size > 0
    # (a row that the previous walk had fixed and the line search took off its bound again goes 1 -> 1 and is not
    # seen, so not every crossing shows; the check above must not be empty, though)
    assert seen >= 1


def test_sharded_cases_bound_each_ranks_last_rows():
    """the two sharded cases use the partition of lbfgsb_amd.block_partition, and bound n_loc % 128 rows per rank"""
    from lbfgsb_amd import block_partition
    for case in hc.CASES:
        for r in range(case.world):
            assert hc.block_rows(case.n, case.world, r) == tuple(block_partition(case.n, case.world, r))
    assert hc.BY_NAME["n510_w2"].bounded.sum() == 2 * 127
    assert hc.BY_NAME["n700_w3"].bounded.sum() == 106 + 105 + 105
