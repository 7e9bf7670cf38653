"""The rank launcher of the sharded GPU tests (tests/_sharded.py) on children that need no GPU: `python -c`
one-liners.  Whenever launch_ranks raises, no child is left running -- the partners of a failed rank, a rank that
ignores SIGTERM, a rank past the deadline -- and after a rank that died by signal nothing more is started.  And the
two pieces of index arithmetic that every sharded test leans on: the uneven split `cut` and `glue`, which puts the
ranks' exported states together."""
import os
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

import _sharded as sh
from _mr_common import cut

MARGIN_S = 5.0   # starting and reaping a few interpreters on a loaded box
OK = [sys.executable, "-c", "pass"]
SLEEP = [sys.executable, "-c", "import time; time.sleep(60)"]


@pytest.fixture
def started(monkeypatch):
    """every child that the launcher starts during the test; the stop-after-a-fault flag is clear before and restored
    after"""
    monkeypatch.setattr(sh, "_faulted", None)
    made, popen = [], subprocess.Popen

    def recording(*args, **kwargs):
        made.append(popen(*args, **kwargs))
        return made[-1]
    monkeypatch.setattr(subprocess, "Popen", recording)
    return made


def _gone(p):
    if p.poll() is None:
        return False
    with pytest.raises(ProcessLookupError):
        os.kill(p.pid, 0)
    return True


def test_all_ranks_succeed(started):
    assert sh.launch_ranks([OK, OK, OK]) is None
    assert [p.returncode for p in started] == [0, 0, 0]


def test_a_failed_rank_ends_its_partners(started):
    t0 = time.monotonic()
    with pytest.raises(RuntimeError) as e:
        sh.launch_ranks([[sys.executable, "-c", "import sys; sys.exit(3)"], SLEEP, SLEEP])
    assert time.monotonic() - t0 <= sh.GRACE_S + sh.TERM_TO_KILL_S + MARGIN_S
    msg = str(e.value)
    assert "rank 0: 3 (on its own)" in msg, msg
    assert msg.count("stopped by the launcher") == 2, msg
    assert len(started) == 3 and all(_gone(p) for p in started)
    assert sh._faulted is None                      # a plain non-zero exit is no fault
    sh.launch_ranks([OK])


def test_a_rank_that_ignores_sigterm_is_killed_at_the_deadline(started, tmp_path):
    ready = tmp_path / "ready"
    code = ("import signal, time; signal.signal(signal.SIGTERM, signal.SIG_IGN); open(%r, 'w').close(); time.sleep(60)"
            % str(ready))
    t0 = time.monotonic()
    with pytest.raises(RuntimeError) as e:
        sh.launch_ranks([[sys.executable, "-c", code]], timeout=2.0)
    assert time.monotonic() - t0 <= 2.0 + sh.TERM_TO_KILL_S + MARGIN_S
    assert ready.exists()                           # (the handler was in place when terminate() came)
    assert _gone(started[0]) and started[0].returncode == -signal.SIGKILL
    assert "no end after 2 s" in str(e.value) and "stopped by the launcher" in str(e.value)
    assert sh._faulted is not None                  # a hang: nothing more is started


def test_nothing_starts_after_a_rank_died_by_signal(started, tmp_path):
    with pytest.raises(RuntimeError) as e:
        sh.launch_ranks([[sys.executable, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGABRT)"], OK])
    assert "rank 0: %d (on its own)" % -signal.SIGABRT in str(e.value)
    assert all(_gone(p) for p in started)
    marker = tmp_path / "started"
    with pytest.raises(RuntimeError) as later:
        sh.launch_ranks([[sys.executable, "-c", "open(%r, 'w').close()" % str(marker)]])
    assert str(e.value) in str(later.value)         # it names the earlier launch
    assert len(started) == 2 and not marker.exists()


@pytest.mark.parametrize("world", [2, 3])
def test_glue_undoes_a_split_at_the_cuts(world):
    n, m = 37, 3
    blocks = [cut(n, world, r) for r in range(world)]
    assert blocks[0][0] == 0 and sum(k for _, k in blocks) == n
    assert all(blocks[r][0] + blocks[r][1] == blocks[r + 1][0] for r in range(world - 1))   # they tile [0, n)
    assert len({k for _, k in blocks}) == world and min(k for _, k in blocks) > 0           # unevenly
    rng = np.random.default_rng(5)
    ws, wy = rng.standard_normal((2, m, n))
    fixed = rng.standard_normal(11 * m * m)
    rows = rng.standard_normal((5, n))      # z, r, d, t, xp
    tail = rng.standard_normal(8 * m)
    wa = np.concatenate([ws.ravel(), wy.ravel(), fixed, rows.ravel(), tail])
    parts = [dict(n_loc=k, wa=np.concatenate([ws[:, a:a + k].ravel(), wy[:, a:a + k].ravel(), fixed,
                                              rows[:, a:a + k].ravel(), tail])) for a, k in blocks]
    got = sh.glue(parts, n, m)
    assert got.dtype == wa.dtype and got.tobytes() == wa.tobytes()
