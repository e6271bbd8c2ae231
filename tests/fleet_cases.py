"""Batches, the host twin's wrapper and the Python-float oracle of the vehicle shares (fcpp_fleet_solve / fcpp_debug_fleet_solve; the rule:
include/fcpp.h), shared by tests/test_fleet_host.py and the device tests (a helper, not a test file).

  Batch        n fields' synthetic tables in the entries' layout: swath and block offsets, T, length, In, Out, C candidate tours, K per field,
               the row length of the per-share outputs, omega.  batch() draws one; the tables are random numbers, not connectors: the rule
               does not care.
  poisoned     a batch of three fields whose middle one is bad in one of the ways KINDS names -> (batch, expected status).
  twin         fcpp_debug_fleet_solve on a Batch -> {output: array}; OUTPUTS names them in the entries' order.
  variant      the tour of variant v of a field, as the rule forms it.
  tables       (P, S) of a tour, added as the rule adds them, in Python floats (IEEE double, one rounding per operation).
  share_cost   c(i, j) of the rule.
  brute        (M, sum) over EVERY composition of a tour into at most K shares: M the least largest share cost, sum the least left-to-right
               rounded sum among the compositions whose largest share cost is <= M.
  field_rows   the oracle's (makespans, totals) rows of a field.
"""
import itertools
from dataclasses import dataclass

import numpy as np

from tests.support import p

INF = float('inf')
MAX_SWATHS = 512
MAX_VEHICLES = 16
OUT_I32 = ('tour', 'share', 'n_used', 'winner', 'status', 'share_first')
OUT_F64 = ('makespan', 'total', 'makespans', 'totals', 'share_cost')
OUTPUTS = ('tour', 'share', 'n_used', 'winner', 'status', 'makespan', 'total', 'makespans', 'totals', 'share_first', 'share_cost')
EINVAL, EUNSUPPORTED = -1, -3


@dataclass
class Batch:
    soff: object                # (n + 1) int64
    toff: object                # (n + 1) int64
    T: object                   # (toff[-1]) float64
    length: object              # (n_total) float64
    In: object                  # (2 n_total) float64
    Out: object
    tours: object               # (C, n_total) int32
    K: object                   # (n) int32
    k_stride: int = MAX_VEHICLES
    omega: float = 1.0
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
        """field f's own tables: (T as N x N or None, length, In, Out, tours as C x m)"""
        s0, s1, m = int(self.soff[f]), int(self.soff[f + 1]), self.m(f)
        T = self.T[int(self.toff[f]):int(self.toff[f + 1])].reshape(2 * m, 2 * m) if m <= MAX_SWATHS else None
        return T, self.length[s0:s1], self.In[2 * s0:2 * s1], self.Out[2 * s0:2 * s1], self.tours[:, s0:s1]


def block_offsets(soff):
    m = np.diff(soff)
    return np.concatenate([[0], np.cumsum(np.where(m > MAX_SWATHS, 0, 4 * m * m))]).astype(np.int64)


def batch(rng, ms, C, K, omega=1.0, both_ways=1, k_stride=MAX_VEHICLES, integer=False, blocked=False):
    """fields of ms swaths with random tables; K: the vehicles, a scalar or one per field.  integer: every table entry a small whole number,
    so that equal costs -- ties -- are common and every sum is exact; blocked: one transit of every field of two swaths or more is +inf,
    one that candidate 0 as given does not drive (the field stays valid) but candidate 0 driven backwards (both_ways) or candidate 1
    (C >= 2) does"""
    ms = np.asarray(ms, dtype=np.int64)
    n = len(ms)
    soff = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    toff = block_offsets(soff)
    total = int(soff[-1])
    draw = (lambda lo, hi, k: rng.integers(int(lo), int(hi), k).astype(np.float64)) if integer else (lambda lo, hi, k: rng.uniform(lo, hi, k))
    T = draw(3, 30, int(toff[-1]))
    length = draw(5, 60, total)
    In, Out = draw(0, 80, 2 * total), draw(0, 80, 2 * total)
    tours = np.zeros((C, total), dtype=np.int32)
    for f in range(n):
        m, s0 = int(ms[f]), int(soff[f])
        for c in range(C):
            tours[c, s0:s0 + m] = 2 * rng.permutation(m) + rng.integers(0, 2, m)
        if m > MAX_SWATHS or m == 0:
            continue
        blk = T[int(toff[f]):int(toff[f + 1])].reshape(2 * m, 2 * m)
        for s in range(m):
            blk[2 * s:2 * s + 2, 2 * s:2 * s + 2] = INF
        if blocked and m >= 2:
            t = variant(tours[0, s0:s0 + m], 1) if both_ways else (tours[1, s0:s0 + m] if C >= 2 else None)
            k = int(rng.integers(0, m - 1))
            if t is not None and not consecutive(tours[0, s0:s0 + m], t[k], t[k + 1]):
                blk[t[k], t[k + 1]] = INF
    Kf = np.broadcast_to(np.asarray(K, dtype=np.int32), (n,)).copy()
    return Batch(soff, toff, T, length, In, Out, tours, Kf, int(k_stride), float(omega), int(both_ways))


def consecutive(t, a, b):
    return any(int(t[k]) == a and int(t[k + 1]) == b for k in range(len(t) - 1))


def out_sizes(b):
    return dict(tour=b.n_total, share=b.n_total, n_used=b.n, winner=b.n, status=b.n, makespan=b.n, total=b.n, makespans=b.n * 2 * b.C,
                totals=b.n * 2 * b.C, share_first=b.n * b.k_stride, share_cost=b.n * b.k_stride)


def out_dtype(name):
    return np.int32 if name in OUT_I32 else np.float64


def shaped(b, outs):
    """the flat outputs with their rows"""
    for k, cols in (('makespans', 2 * b.C), ('totals', 2 * b.C), ('share_first', b.k_stride), ('share_cost', b.k_stride)):
        if k in outs:
            outs[k] = outs[k].reshape(b.n, cols)
    return outs


def twin_call(lib, b, outs):
    """fcpp_debug_fleet_solve with the output pointers `outs` (a dict; a missing name is NULL) -> the return code"""
    return lib.fcpp_debug_fleet_solve(b.n, p(b.soff), b.n_total, p(b.toff), int(b.toff[-1]), p(b.T), p(b.length), p(b.In), p(b.Out), b.C, p(b.tours),
                                      b.both_ways, p(b.K), b.k_stride, b.omega, *[p(outs.get(k)) for k in OUTPUTS])


def twin(lib, b):
    sizes = out_sizes(b)
    outs = {k: np.full(sizes[k], -7, dtype=out_dtype(k)) for k in OUTPUTS}
    rc = twin_call(lib, b, outs)
    assert rc == 0, rc
    return shaped(b, outs)


# ---- one bad field among good ones -------------------------------------------------------------------------------------------------------
def poisoned(kind):
    """a batch of three fields whose middle one is bad in the way `kind` says -> (batch, expected status)"""
    rng = np.random.default_rng(8)
    ms = [6, 513 if kind == 'too many' else 7, 5]
    b = batch(rng, ms, 2, [3, 4, 2], omega=1.5, k_stride=4 if kind == 'K beyond the rows' else MAX_VEHICLES)
    s0 = int(b.soff[1])
    if kind == 'too many':
        return b, EUNSUPPORTED
    if kind == 'K 17':
        b.K[1] = 17
        return b, EUNSUPPORTED
    if kind in ('K 0', 'K < 0', 'K beyond the rows'):
        b.K[1] = {'K 0': 0, 'K < 0': -2, 'K beyond the rows': 5}[kind]
    elif kind == 'twice':
        b.tours[1, s0 + 3] = b.tours[1, s0 + 2] ^ 1
    elif kind == 'beyond':
        b.tours[1, s0 + 3] = 14
    elif kind == 'negative':
        b.tours[0, s0] = -1
    elif kind in ('length < 0', 'length nan', 'length inf'):
        b.length[s0 + 2] = {'length < 0': -1.0, 'length nan': np.nan, 'length inf': INF}[kind]
    elif kind in ('S inf', 'S nan'):
        t = b.tours[0, s0:s0 + 7]
        b.T[int(b.toff[1]):int(b.toff[2])].reshape(14, 14)[t[2], t[3]] = INF if kind == 'S inf' else np.nan
    return b, EINVAL


KINDS = ['too many', 'K 17', 'K 0', 'K < 0', 'K beyond the rows', 'twice', 'beyond', 'negative', 'length < 0', 'length nan', 'length inf', 'S inf',
         'S nan']


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def plus(a, b):
    s = a + b
    return s if s < INF else INF


def variant(cand, r):
    t = np.asarray(cand, dtype=np.int64)
    return (t[::-1] ^ 1) if r else t


def tables(t, T, length):
    """(P, S) of the tour t"""
    m = len(t)
    P = [0.0]
    for k in range(m):
        P.append(P[k] + float(length[t[k] >> 1]))
    S = [0.0] * max(m, 1)
    for k in range(1, m):
        S[k] = S[k - 1] + float(T[t[k - 1], t[k]])
    return P, S


def share_cost(t, P, S, In, Out, omega, i, j):
    """c(i, j): the positions i .. j - 1 from the depot and back"""
    return plus((float(In[t[i]]) + (S[j - 1] - S[i])) + float(Out[t[j - 1]]), omega * (P[j] - P[i]))


def split_costs(t, P, S, In, Out, omega, firsts):
    """the costs of the shares that start at `firsts` (ascending, firsts[0] == 0)"""
    ends = list(firsts[1:]) + [len(t)]
    return [share_cost(t, P, S, In, Out, omega, i, j) for i, j in zip(firsts, ends)]


def rounded_sum(costs):
    s = 0.0
    for c in costs:
        s = plus(c, s)
    return s


def brute(t, P, S, In, Out, omega, K):
    """(M, sum) over every composition of the tour into at most K non-empty contiguous shares"""
    m = len(t)
    if m == 0:
        return 0.0, 0.0
    splits = []
    for k in range(1, min(K, m) + 1):
        for cuts in itertools.combinations(range(1, m), k - 1):
            costs = split_costs(t, P, S, In, Out, omega, [0] + list(cuts))
            splits.append((max(costs), rounded_sum(costs)))
    M = min(s[0] for s in splits)
    return M, min(s[1] for s in splits if s[0] <= M)


def field_rows(b, f, K=None):
    """the oracle's (makespans, totals) rows of field f: every variant's (M, sum), NaN for the variants that do not exist"""
    T, length, In, Out, tours = b.field(f)
    K = int(b.K[f]) if K is None else K
    Ms, sums = np.full(2 * b.C, np.nan), np.full(2 * b.C, np.nan)
    for v in range(2 * b.C):
        if (v & 1) and not b.both_ways:
            continue
        t = variant(tours[v >> 1], v & 1)
        P, S = tables(t, T, length)
        Ms[v], sums[v] = brute(t, P, S, In, Out, b.omega, K)
    return Ms, sums
