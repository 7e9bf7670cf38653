"""One sequence of curvature pairs and the oracle's state after each of them, for the tests of the pairs in and out
(lbfgsb_hip_qn_pairs_set / _push): tests/_qn_synth.py's recipe -- pairs (s, y = D s [+ noise]) of its two families,
Routines.matupd per pair, Routines.formt for a state -- but with ONE random stream for the whole sequence, so that the
state after j pairs is the state after j - 1 pairs plus pair j.  (synth(n, m, j) seeds its generator with j: its
states for different j hold unrelated pairs, which no sequence of pushes can reproduce.)"""
import numpy as np

from oracle import pyoracle as po

from _qn_synth import QnSynth


def sequence(n, m, npairs, family="dyadic", real=np.float64, seed=0):
    """-> (pairs, states): pairs[j - 1] = (s_j, y_j) as float64 arrays (fp32 numbers for real = float32),
    states[j] = the QnSynth after the first j of them, j = 0 .. npairs (import_state takes each)"""
    assert family in ("dyadic", "generic")
    rng = np.random.default_rng(2000003 * seed + 7919 * n + 31 * m + (0 if family == "dyadic" else 500))
    D = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), n)
    R = po.Routines()
    ws, wy = np.zeros(m * n), np.zeros(m * n)
    sy, ss = np.zeros(m * m), np.zeros(m * m)
    col, head, itail = (np.array([v], np.int32) for v in (0, 1, 0))
    theta = np.array([1.0])
    off = po.wa_offsets(n, m)

    def state(j):
        wt, info = np.zeros(m * m), np.zeros(1, np.int32)
        c, h = int(col[0]), int(head[0])
        if c:
            R.formt(m, wt, sy, ss, c, float(theta[0]), info)
        wa = np.zeros(po.wa_len(n, m), np.float64)
        for name, arr in (("ws", ws), ("wy", wy), ("sy", sy), ("ss", ss), ("wt", wt)):
            o, sz = off[name]
            wa[o:o + sz] = arr
        isave = np.zeros(44, np.int32)
        isave[26], isave[27], isave[28], isave[30] = h, c, int(itail[0]), j
        M = lambda a: a.reshape(m, m).T.copy()  # noqa: E731
        st = QnSynth(n, m, c, h, j, real, family, float(theta[0]), int(info[0]), np.zeros(c), wa.astype(real),
                     np.zeros(3 * n, np.int32), isave, M(sy), M(ss), M(wt))
        st.sty_diag = np.diag(st.sy)[:c].copy()
        st.itail = int(itail[0])
        assert st.info == 0 and np.all(st.sty_diag > 0.0)
        return st

    pairs, states = [], [state(0)]
    for it in range(1, npairs + 1):
        if family == "dyadic":
            s = np.zeros(n)
            while not s.any():  # (n = 1: a zero draw is no pair)
                s = rng.integers(-4, 5, n).astype(np.float64) / 8.0
            y = D * s
        else:
            s = rng.standard_normal(n)
            y = D * s + 0.05 * rng.standard_normal(n)
            if real == np.float32:
                s, y = s.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
        dot = lambda a, b: float(R.lib.lbo_ddot(n, po._ptr(a), po._ptr(b)))  # noqa: E731
        rr, dr, dtd = dot(y, y), dot(s, y), dot(s, s)
        assert dr > 0.0, "a pair with s'y <= 0"
        R.matupd(n, m, ws, wy, sy, ss, s, y, itail, it, col, head, theta, rr, dr, 1.0, dtd)
        pairs.append((s.copy(), y.copy()))
        states.append(state(it))
    return pairs, states
