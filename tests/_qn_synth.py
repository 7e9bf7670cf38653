"""Curvature-model states with a chosen col, head, real kind and data, made on the CPU with the oracle's own routines
(the way tests/test_gpu_routines.py calls them): `npairs` calls of Routines.matupd with pairs (s, y = D s [+ noise]),
one Routines.formt, then ws, wy, sy, ss, wt packed at pyoracle.wa_offsets -- the rest of wa and all of iwa zero,
isave[26] = head, isave[27] = col, isave[30] = iupdat.  DeviceSolver.import_state takes such a state as it takes an
exported one; npairs > m wraps the ring, so head != 1.

Two data families:
  dyadic   s has entries in {-4 ... 4} / 8, D is diagonal with entries in {1/2, 1, 2, 4}: every entry of S'S, S'Y and
           Y'Y is a multiple of 2^-7 below 2^24 for n <= 2000, so it is exact in fp32 and fp64 in any order of
           summation, and a REAL32 context's imported sy and ss carry no rounding;
  generic  s has normal entries, y = D s + 0.05 noise: the rounding of every product is exercised.
REAL32 states make the pairs in fp32 (exact in the dyadic family), compute sy, ss, wt from them with the fp64 oracle
and round those for the import: in the dyadic family only wt carries fp32 rounding."""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle as po


@dataclass
class QnSynth:
    n: int
    m: int
    col: int
    head: int
    iupdat: int
    real: type
    family: str
    theta: float        # the oracle's theta of the newest pair (1.0 with no pair)
    info: int           # formt's info
    sty_diag: np.ndarray  # s'y of every stored pair, oldest first
    wa: np.ndarray      # in `real`, as import_state takes it
    iwa: np.ndarray
    isave: np.ndarray
    sy: np.ndarray      # the fp64 oracle's m x m matrices (column-major storage viewed as [i, j])
    ss: np.ndarray
    wt: np.ndarray

    def mats(self, name):
        """the imported sy / ss / wt (in `real`, as stored in wa) as an m x m float64 array [i, j]"""
        o, sz = po.wa_offsets(self.n, self.m)[name]
        return self.wa[o:o + sz].astype(np.float64).reshape(self.m, self.m).T

    def pairs(self):
        """S, Y (n x col float64, oldest pair first) as stored in wa"""
        return ring_pairs(self.wa, self.n, self.m, self.col, self.head)


def ring_pairs(wa, n, m, col, head):
    """S, Y (n x col float64, oldest pair first) from a wa in the reference's layout and the 1-based head"""
    wa = np.asarray(wa)
    Ws = wa[:m * n].astype(np.float64).reshape(m, n).T
    Wy = wa[m * n:2 * m * n].astype(np.float64).reshape(m, n).T
    cols = [(head - 1 + j) % m for j in range(col)]
    return Ws[:, cols].copy(), Wy[:, cols].copy()


def synth(n, m, npairs, family="dyadic", real=np.float64, seed=0):
    """the state after `npairs` accepted pairs in a ring of m"""
    assert family in ("dyadic", "generic") and npairs >= 0
    rng = np.random.default_rng(1000003 * seed + 7919 * n + 31 * m + npairs + (0 if family == "dyadic" else 500))
    D = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), n)
    R = po.Routines()  # (fp64: the small matrices are rounded for the import, not summed in fp32)
    ws, wy = np.zeros(m * n), np.zeros(m * n)
    sy, ss, wt = np.zeros(m * m), np.zeros(m * m), np.zeros(m * m)
    col, head, itail = (np.array([v], np.int32) for v in (0, 1, 0))
    theta = np.array([1.0])
    for it in range(1, npairs + 1):
        if family == "dyadic":
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
    info = np.zeros(1, np.int32)
    c, h = int(col[0]), int(head[0])
    if c:
        R.formt(m, wt, sy, ss, c, float(theta[0]), info)
    wa = np.zeros(po.wa_len(n, m), np.float64)
    off = po.wa_offsets(n, m)
    for name, arr in (("ws", ws), ("wy", wy), ("sy", sy), ("ss", ss), ("wt", wt)):
        o, sz = off[name]
        wa[o:o + sz] = arr
    wa_r = wa.astype(real)
    if real == np.float32:  # (the pairs are fp32 numbers: nothing of W is rounded here)
        assert np.array_equal(wa_r[:2 * m * n].astype(np.float64), wa[:2 * m * n])
    isave = np.zeros(44, np.int32)
    isave[26], isave[27], isave[28], isave[30] = h, c, int(itail[0]), npairs
    M = lambda a: a.reshape(m, m).T.copy()  # noqa: E731
    st = QnSynth(n, m, c, h, npairs, real, family, float(theta[0]), int(info[0]), np.zeros(c), wa_r,
                 np.zeros(3 * n, np.int32), isave, M(sy), M(ss), M(wt))
    st.sty_diag = np.diag(st.sy)[:c].copy()
    assert st.info == 0 and np.all(st.sty_diag > 0.0)
    return st
