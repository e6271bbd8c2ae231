"""Batches, the host twin's wrapper and the numpy oracle of the service trips (fcpp_trip_solve / fcpp_debug_trip_solve; the rule:
include/fcpp.h), shared by tests/test_trips_host.py and the device tests (a helper, not a test file).

  Batch        n fields' synthetic tables in the entries' layout: swath and block offsets, T, length, E, X, In, Out, C candidate tours,
               capacities.  batch() draws one; the tables are random numbers, not connectors: the rule does not care.
  poisoned     a batch of three fields whose middle one is bad in one of the ways KINDS names -> (batch, expected status).
  twin         fcpp_debug_trip_solve on a Batch -> {output: array}; OUTPUTS names them in the entries' order.
  variant      the tour of variant v of a field, as the rule forms it.
  tables       (P, d, base) of a tour, added as the rule adds them, in Python floats (IEEE double, one rounding per operation).
  brute        the least cost over EVERY stop set of a tour (2^(m - 1) of them), each summed left to right as the rule sums.
  cost_of      the cost of given trip starts, or None where a trip is infeasible.
"""
import itertools
from dataclasses import dataclass

import numpy as np

from tests.support import p

INF = float('inf')
MAX_SWATHS = 512
OUT_I32 = ('tour', 'trip', 'n_trips', 'overfull', 'winner', 'status')
OUT_F64 = ('cost', 'base', 'extra', 'costs')
OUTPUTS = OUT_I32 + OUT_F64
EINVAL, EUNSUPPORTED = -1, -3


@dataclass
class Batch:
    soff: object                # (n + 1) int64
    toff: object                # (n + 1) int64
    T: object                   # (toff[-1]) float64
    length: object              # (n_total) float64
    E: object                   # (2 n_total) float64 or None
    X: object
    In: object                  # (2 n_total) float64
    Out: object
    tours: object               # (C, n_total) int32
    Q: object                   # (n) float64
    Q0: object                  # (n) float64 or None
    stop: float = 0.0
    both_ways: int = 1

    @property
    def n(self):
        return len(self.soff) - 1

    @property
    def n_total(self):
        return int(self.soff[-1])

    @property
    def C(self):
        return int(self.tours.shape[0])

    def m(self, f):
        return int(self.soff[f + 1] - self.soff[f])

    def field(self, f):
        """field f's own tables: (T as N x N or None, length, E, X, In, Out, tours as C x m)"""
        s0, s1, m = int(self.soff[f]), int(self.soff[f + 1]), self.m(f)
        T = self.T[int(self.toff[f]):int(self.toff[f + 1])].reshape(2 * m, 2 * m) if m <= MAX_SWATHS else None
        ends = [None if a is None else a[2 * s0:2 * s1] for a in (self.E, self.X, self.In, self.Out)]
        return T, self.length[s0:s1], *ends, self.tours[:, s0:s1]


def block_offsets(soff):
    m = np.diff(soff)
    return np.concatenate([[0], np.cumsum(np.where(m > MAX_SWATHS, 0, 4 * m * m))]).astype(np.int64)


def batch(rng, ms, C, capacity, first=None, ends=True, stop=0.0, both_ways=1, swath=None, metric=False):
    """fields of ms swaths with random tables.  capacity, first: per field, in MEAN SWATHS of the field (first: a share of the capacity,
    None = no Q0); swath: every swath's length (None: random in [5, 60]); metric: the ways to and from the service point are at least 15
    each, so that no detour over it is shorter than a transit (at most 30) and no stop has a negative price -- what connector lengths
    give by the triangle inequality; without it some stops pay, which the rule allows"""
    ms = np.asarray(ms, dtype=np.int64)
    n = len(ms)
    soff = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    toff = block_offsets(soff)
    total = int(soff[-1])
    T = rng.uniform(3.0, 30.0, int(toff[-1]))
    for f in range(n):
        m = int(ms[f])
        if m <= MAX_SWATHS and m > 0:
            blk = T[int(toff[f]):int(toff[f + 1])].reshape(2 * m, 2 * m)
            for s in range(m):
                blk[2 * s:2 * s + 2, 2 * s:2 * s + 2] = INF
    length = rng.uniform(5.0, 60.0, total) if swath is None else np.full(total, float(swath))
    E, X = (rng.uniform(0.0, 80.0, 2 * total) for _ in range(2))
    In, Out = (rng.uniform(15.0 if metric else 0.0, 80.0, 2 * total) for _ in range(2))
    tours = np.zeros((C, total), dtype=np.int32)
    for f in range(n):
        m, s0 = int(ms[f]), int(soff[f])
        for c in range(C):
            tours[c, s0:s0 + m] = 2 * rng.permutation(m) + rng.integers(0, 2, m)
    cap = np.broadcast_to(np.asarray(capacity, dtype=np.float64), (n,))
    mean = np.array([length[int(soff[f]):int(soff[f + 1])].mean() if ms[f] else 1.0 for f in range(n)])
    Q = np.ascontiguousarray(cap * mean)
    Q0 = None if first is None else np.ascontiguousarray(Q * np.broadcast_to(np.asarray(first, dtype=np.float64), (n,)))
    return Batch(soff, toff, T, length, E if ends else None, X if ends else None, In, Out, tours, Q, Q0, float(stop), int(both_ways))


def out_sizes(b):
    return dict(tour=b.n_total, trip=b.n_total, n_trips=b.n, overfull=b.n, winner=b.n, status=b.n, cost=b.n, base=b.n, extra=b.n, costs=b.n * 2 * b.C)


def out_dtype(name):
    return np.int32 if name in OUT_I32 else np.float64


def twin_call(lib, b, outs):
    """fcpp_debug_trip_solve with the output pointers `outs` (a dict; a missing name is NULL) -> the return code"""
    return lib.fcpp_debug_trip_solve(b.n, p(b.soff), b.n_total, p(b.toff), int(b.toff[-1]), p(b.T), p(b.length), p(b.E), p(b.X), p(b.In), p(b.Out), b.C,
                                     p(b.tours), b.both_ways, p(b.Q), p(b.Q0), b.stop, *[p(outs.get(k)) for k in OUTPUTS])


def twin(lib, b):
    sizes = out_sizes(b)
    outs = {k: np.full(sizes[k], -7, dtype=out_dtype(k)) for k in OUTPUTS}
    rc = twin_call(lib, b, outs)
    assert rc == 0, rc
    outs['costs'] = outs['costs'].reshape(b.n, 2 * b.C)
    return outs


# ---- one bad field among good ones -------------------------------------------------------------------------------------------------------
def poisoned(kind):
    """a batch of three fields whose middle one is bad in the way `kind` says -> (batch, expected status)"""
    rng = np.random.default_rng(8)
    ms = [6, 513 if kind == 'too many' else 7, 5]
    b = batch(rng, ms, 2, 2.5, first=0.6)
    s0 = int(b.soff[1])
    if kind == 'too many':
        return b, EUNSUPPORTED
    if kind == 'twice':
        b.tours[1, s0 + 3] = b.tours[1, s0 + 2] ^ 1
    elif kind == 'beyond':
        b.tours[1, s0 + 3] = 14
    elif kind == 'negative':
        b.tours[0, s0] = -1
    elif kind in ('length < 0', 'length nan', 'length inf'):
        b.length[s0 + 2] = {'length < 0': -1.0, 'length nan': np.nan, 'length inf': INF}[kind]
    elif kind in ('Q nan', 'Q 0', 'Q < 0'):
        b.Q[1] = {'Q nan': np.nan, 'Q 0': 0.0, 'Q < 0': -3.0}[kind]
    elif kind in ('Q0 nan', 'Q0 0'):
        b.Q0[1] = np.nan if kind == 'Q0 nan' else 0.0
    elif kind == 'base':
        t = b.tours[0, s0:s0 + 7]
        b.T[int(b.toff[1]):int(b.toff[2])].reshape(14, 14)[t[2], t[3]] = INF
    return b, EINVAL


KINDS = ['too many', 'twice', 'beyond', 'negative', 'length < 0', 'length nan', 'length inf', 'Q nan', 'Q 0', 'Q < 0', 'Q0 nan', 'Q0 0', 'base']


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def plus(a, b):
    s = a + b
    return s if s < INF else INF


def variant(cand, r):
    t = np.asarray(cand, dtype=np.int64)
    return (t[::-1] ^ 1) if r else t


def tables(t, T, length, E, X, In, Out, stop):
    """(P, d, base) of the tour t"""
    m = len(t)
    P = [0.0]
    for k in range(m):
        P.append(P[k] + float(length[t[k] >> 1]))
    d = [0.0] * m
    for j in range(1, m):
        a, c = t[j - 1], t[j]
        d[j] = plus((float(Out[a]) + float(In[c])) - float(T[a, c]), stop)
    base = 0.0
    if m:
        base = 0.0 if E is None else float(E[t[0]])
        for k in range(m - 1):
            base += float(T[t[k], t[k + 1]])
        base = base + (0.0 if X is None else float(X[t[-1]]))
    return P, d, base


def feasible(P, i, j, Q, Q0):
    return j == i + 1 or P[j] - P[i] <= (Q0 if i == 0 else Q)


def cost_of(starts, P, d, Q, Q0):
    """the left-to-right rounded sum of the stops at `starts` (ascending, starts[0] == 0), None where a trip is infeasible"""
    m = len(P) - 1
    ends = list(starts[1:]) + [m]
    if any(not feasible(P, i, j, Q, Q0) for i, j in zip(starts, ends)):
        return None
    c = 0.0
    for j in starts[1:]:
        c = plus(d[j], c)
    return c


def brute(P, d, Q, Q0):
    """the least cost over all 2^(m - 1) stop sets"""
    m = len(P) - 1
    if m == 0:
        return 0.0
    best = INF
    for mask in itertools.product((0, 1), repeat=m - 1):
        c = cost_of([0] + [j for j in range(1, m) if mask[j - 1]], P, d, Q, Q0)
        if c is not None and c < best:
            best = c
    return best


def field_costs(b, f):
    """the oracle's cost row of field f: every variant's total, NaN for the variants that do not exist"""
    T, length, E, X, In, Out, tours = b.field(f)
    Q, Q0 = float(b.Q[f]), float(b.Q[f] if b.Q0 is None else b.Q0[f])
    row = np.full(2 * b.C, np.nan)
    for v in range(2 * b.C):
        if (v & 1) and not b.both_ways:
            continue
        P, d, base = tables(variant(tours[v >> 1], v & 1), T, length, E, X, In, Out, b.stop)
        row[v] = plus(base, brute(P, d, Q, Q0))
    return row
