"""The inputs of tests/test_gpu_routines_real32.py are well posed and its bars bite -- shown with no GPU, on the REAL32
oracle alone (tests/_r32_truth.py builds the cases, the truth and the magnitudes).

Per case and routine the table printed here records how many states were examined, rho_ref (the REAL32 oracle's error
against the truth in units of eps32 M, over the states whose decisions agree) and how often the REAL32 oracle's integers
(nseg, info, iwhere; iword, info; ifun, iback, nfgv, info, task, csave, isave of dcsrch) equal the truth's.  Asserted:
  * the integers differ from the truth's in at most 1 examined state in 4 per case and 1 in 10 over all cases -- so the
    GPU test's rule "equal to the truth's or the REAL32 oracle's, left out at most that often" can be met;
  * every routine is examined in at least 3 states of every case with n >= 63, at least once in the three smallest;
  * the bounded branch of subsm (iword = 1) is reached in at least 4 cases;
  * the class (b) bar, |got - exact| <= 1e-12 M, rejects two deliberately wrong sums in every case with n >= 63: the sum
    with its last row left out (a lost tail: in at least one examined state -- a last row that does not move adds 0 to
    every sum of that state) and the sum accumulated in float32 (in every examined state).  The sums are those the doors
    return as doubles: y'y = theta dr of matupd, dtd and gd of the line search's set-up call.
Seeds: 201 ... 212 in the order of the table, and 215 for the last case -- with 213 its last row never moves, so that
leaving it out changes no sum and the lost tail is not rejected there.
"""
import numpy as np
import pytest

import _r32_truth as rt
from _r32_truth import F32, F64, LD, SUM_BAR

DECIDING = ("cauchy", "subsm", "lnsrlb", "lnsrlb2")


def _passes(got, exact, M):
    return abs(LD(got) - exact) <= SUM_BAR * M


def _wrong_sums(a, b):
    """a'b with the last row left out, and accumulated in float32 one term after the other"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    lost = rt.xdot(a[:-1], b[:-1])[0]
    acc = np.add.accumulate(a.astype(F32) * b.astype(F32), dtype=F32)[-1]     # (accumulate is sequential)
    return lost, acc


@pytest.fixture(scope="module")
def survey(oracle_built):
    out = []
    for case in rt.CASES:
        p, sts = rt.states(case)
        T = rt.Tally(rt.case_id(case))
        sep = dict(states=0, lost_rejected=0, fp32_rejected=0)
        for s in sts:
            ch = rt.chain(p, s)
            for k, rec in ch.items():
                same = not hasattr(getattr(rec, "ref", None), "ints") or rec.ref.ints == rec.tru.ints
                rr = rt.rho_ref(rec) if same and hasattr(rec, "units") else {}
                T.add(k, max(rr.values(), default=0.0), ints_equal=same)
            T.bounded += int("subsm" in ch and ch["subsm"].bounded)
            if "lnsrlb" in ch:
                sums = [(ch["lnsrlb"].z.astype(F64) - s.x.astype(F64),) * 2 + ch["lnsrlb"].dtd,
                        (s.g, ch["lnsrlb"].z.astype(F64) - s.x.astype(F64)) + ch["lnsrlb"].gd]
                if "matupd" in ch:
                    sums.append((ch["matupd"].y,) * 2 + rt.xdot(ch["matupd"].y, ch["matupd"].y))
                wrong = [_wrong_sums(a, b) + (e, M) for (a, b, e, M) in sums if M > 0]
                sep["states"] += 1
                sep["lost_rejected"] += int(any(not _passes(lost, e, M) for (lost, _, e, M) in wrong))
                sep["fp32_rejected"] += int(all(not _passes(acc, e, M) for (_, acc, e, M) in wrong))
        out.append((case, T, sep))
        print("\n" + T.table(gpu=False))
        print("   wrong sums: %(states)d states, lost tail rejected in %(lost_rejected)d, fp32 accumulator in "
              "%(fp32_rejected)d" % sep)
    return out


def test_states_and_decisions(survey):
    tot = diff = 0
    for case, T, _ in survey:
        n = case[1]
        st = sum(T.rows[r]["states"] for r in DECIDING)
        df = st - sum(T.rows[r]["ints_equal"] for r in DECIDING)
        assert 4 * df <= st, "%s: the REAL32 oracle's integers differ from the truth's in %d of %d" % (T.name, df, st)
        tot, diff = tot + st, diff + df
        for r in rt.ROUTINES[:-1]:
            assert T.rows[r]["states"] >= (3 if n >= 63 else 1), (T.name, r, T.rows[r])
    assert 10 * diff <= tot, (diff, tot)
    assert sum(1 for _, T, _ in survey if T.bounded) >= 4, "the bounded branch of subsm"


def test_class_b_bar_rejects_a_lost_tail_and_an_fp32_accumulator(survey):
    for case, T, sep in survey:
        if case[1] >= 63:
            assert sep["states"] >= 3, (T.name, sep)
            assert sep["lost_rejected"] >= 1, "%s: a sum without its last row passes the class (b) bar" % T.name
            assert sep["fp32_rejected"] == sep["states"], "%s: an fp32 accumulator passes the class (b) bar" % T.name
