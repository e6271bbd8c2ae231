"""Fields for the field cell tests (tests/test_cells_host.py, tests/test_gpu_cells*.py) and the host-side caller of fcpp_debug_cells.

NAMED: the shapes whose cell counts at cut angle 0 are known by hand (COUNTS: reflex, extrema), each also rotated by 0.5 rad.
DEVICE: what a device loop can get wrong -- stars at the sizes where the kernels change shape (64 edges: one wavefront / four) or a lane
takes a second item (256, 257), the cap and one beyond it, fields of every status, and fields of 260 rings for loops that stride over rings."""
import numpy as np

from field_coverage_path_planning_amd import _lib as L
from tests.support import p as _p
from tests.test_swaths_host import pack, rings_of, rotated

MAX_EDGES = 1024
EINVAL, EUNSUPPORTED = -1, -3
REFLEX, EXTREMA = 0, 1

RECT = [(0, 0), (10, 0), (10, 4), (0, 4)]
ELL = [(0, 0), (60, 0), (60, 20), (25, 20), (25, 50), (0, 50)]
TEE = [(10, 0), (20, 0), (20, 20), (30, 20), (30, 30), (0, 30), (0, 20), (10, 20)]
PLUS = [(10, 0), (20, 0), (20, 10), (30, 10), (30, 20), (20, 20), (20, 30), (10, 30), (10, 20), (0, 20), (0, 10), (10, 10)]
# two 12 x 60 m legs on a 72 x 12 m bar
YOU = [(0, 0), (72, 0), (72, 72), (60, 72), (60, 12), (12, 12), (12, 72), (0, 72)]
AITCH = [(0, 0), (10, 0), (10, 15), (30, 15), (30, 0), (40, 0), (40, 40), (30, 40), (30, 25), (10, 25), (10, 40), (0, 40)]
SQUARE = [(0, 0), (40, 0), (40, 40), (0, 40)]
POND_MID = [(12, 12), (28, 12), (28, 28), (12, 28)]


def diamond(cx, cy, rx, ry):
    return [(cx + rx, cy), (cx, cy + ry), (cx - rx, cy), (cx, cy - ry)]


def sym_star(m, r_out=30.0, r_in=14.0, centre=(35.0, 33.0)):
    """m vertices alternating between two radii: symmetric, so at cut angle 0 reflex vertices face each other on levels an ulp apart"""
    a = 2.0 * np.pi * np.arange(m) / m
    r = np.where(np.arange(m) % 2 == 0, r_out, r_in)
    return np.column_stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)])


def rnd_star(seed, m, r_lo=40.0, r_hi=120.0, centre=(300.0, -120.0)):
    """m vertices at sorted random angles and random radii: a simple ring that is star-shaped about its centre"""
    rng = np.random.default_rng(seed)
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, m))
    while np.any(np.diff(a) == 0.0):
        a = np.sort(rng.uniform(0.0, 2.0 * np.pi, m))
    r = rng.uniform(r_lo, r_hi, m)
    return np.column_stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)])


def star_pond(seed, m=32):
    """a random star with one diamond pond about its centre (the radii start at 40, the pond reaches 12)"""
    rng = np.random.default_rng(seed + 1000)
    return [rnd_star(seed, m), np.asarray(diamond(300.0 + rng.uniform(-3, 3), -120.0 + rng.uniform(-3, 3), rng.uniform(4, 12), rng.uniform(4, 12)))]


def ponds_field(n_ponds=259, cols=17, pitch=10.0, kind='diamond'):
    """a rectangle with n_ponds small ponds on a lattice: 260 rings, a second round for a loop that strides over rings by 256.  Diamond ponds:
    4 + 4 x 259 = 1040 edges, over the cap; triangular ponds: 781 edges, under it.  Every pond sits a little higher than the one before,
    so no two corners share a level."""
    rows = -(-n_ponds // cols)
    rings = [np.array([(0.0, 0.0), (cols * pitch, 0.0), (cols * pitch, rows * pitch), (0.0, rows * pitch)])]
    for k in range(n_ponds):
        cx, cy = (k % cols + 0.5) * pitch, (k // cols + 0.5) * pitch + 0.011 * (k % cols) + 0.0007 * k
        if kind == 'diamond':
            rings.append(np.asarray(diamond(cx, cy, 1.4, 1.1)))
        else:
            rings.append(np.array([(cx - 1.3, cy - 0.9), (cx + 1.4, cy - 0.8), (cx + 0.1, cy + 1.6)]))
    return rings


NAMED = {
    'rect': RECT, 'ell': ELL, 'tee': TEE, 'plus': PLUS, 'you': YOU, 'aitch': AITCH,
    'holed_square': [SQUARE, POND_MID],
    'diamond_pond': [SQUARE, diamond(20, 21, 7, 9)],
    'two_diamonds': [[(0, 0), (80, 0), (80, 40), (0, 40)], diamond(22, 20, 6, 8), diamond(55, 20, 6, 8)],
}
# cells at cut angle 0: (reflex, extrema)
COUNTS = {'rect': (1, 1), 'ell': (2, 1), 'tee': (2, 1), 'plus': (3, 1), 'you': (3, 3), 'aitch': (5, 5), 'holed_square': (4, 4),
          'diamond_pond': (6, 4), 'two_diamonds': (8, 5)}
STAR32 = sym_star(32)
TILT = 0.5


def named_cases():
    """(name, field, cut angle): every named shape and the star at angle 0, and its copy rotated by TILT at cut angle TILT"""
    out = []
    for name, f in list(NAMED.items()) + [('star32', STAR32)]:
        out.append((name, rings_of(f), 0.0))
        out.append((name + '_tilt', rotated(f, TILT), TILT))
    return out


# two touching rings: the pond stands with its lowest corner on the outline (FCPP_EUNSUPPORTED at every cut angle of the tests); and two
# ponds that share the corner (28, 20), which a cut along angle 0 runs into
TOUCHING = [[(0, 0), (80, 0), (80, 40), (0, 40)], diamond(20, 8, 6, 8)]
TOUCHING_PONDS = [[(0, 0), (80, 0), (80, 40), (0, 40)], diamond(22, 20, 6, 8), diamond(34, 20, 6, 8)]
NAN_FIELD = [(0.0, 0.0), (10.0, 0.0), (np.nan, 5.0), (0.0, 10.0)]
ZERO_EDGE = [(0.0, 0.0), (10.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0)]
SHORT_RING = [SQUARE, [(5.0, 5.0), (6.0, 6.0)]]
EMPTY = []

DEVICE_STARS = {m: rnd_star(m, m) for m in (3, 63, 64, 65, 256, 257, 1024, 1025)}


def device_cases():
    """name -> field: the named cases (cut angles come with the batch), the stars, the statuses, the ring loops"""
    out = {name: f for name, f, _ in named_cases()}
    out.update({'star%d' % m: [s] for m, s in DEVICE_STARS.items()})
    out.update({'star_pond%d' % k: star_pond(k) for k in range(4)})
    out.update({'nan': rings_of(NAN_FIELD), 'empty': EMPTY, 'zero_edge': rings_of(ZERO_EDGE), 'short_ring': rings_of(SHORT_RING),
                'touching': rings_of(TOUCHING), 'touching_ponds': rings_of(TOUCHING_PONDS), 'ponds259': ponds_field(259, kind='diamond'), 'tri_ponds259': ponds_field(259, kind='triangle')})
    return out


class HostCells:
    """fcpp_debug_cells on a batch: sizes with caps of 0, then the cells"""

    def __init__(self, fields, angles, events, min_area=0.0):
        lib = L.load()
        ro, vo, x, y = pack(fields)
        self.n = len(ro) - 1
        ang = np.ascontiguousarray(np.broadcast_to(np.asarray(angles, dtype=np.float64), (self.n,)))
        self.angle = ang
        self.co, self.cvo = np.zeros(self.n + 1, np.int64), np.zeros(self.n + 1, np.int64)
        self.status, self.n_cuts, self.dropped = (np.full(self.n, -7, np.int32) for _ in range(3))
        self.dropped_area = np.full(self.n, np.nan)
        head = (self.n, _p(ro), len(vo) - 1, _p(vo), len(x), _p(x), _p(y), _p(ang), int(events), float(min_area))
        rc = lib.fcpp_debug_cells(*head, _p(self.co), _p(self.cvo), _p(self.status), _p(self.n_cuts), _p(self.dropped), _p(self.dropped_area),
                                  0, 0, None, None, None, None, None, None)
        assert rc == 0, lib.fcpp_last_error()
        C, V = int(self.co[-1]), int(self.cvo[-1])
        self.ovo = np.full(C + 1, -1, np.int64)
        self.x, self.y, self.src = np.full(V, np.nan), np.full(V, np.nan), np.full(V, -9, np.int32)
        self.field, self.area = np.full(C, -9, np.int32), np.full(C, np.nan)
        co2, cvo2 = np.zeros(self.n + 1, np.int64), np.zeros(self.n + 1, np.int64)
        rc = lib.fcpp_debug_cells(*head, _p(co2), _p(cvo2), None, None, None, None, C, V, _p(self.ovo), _p(self.x), _p(self.y), _p(self.src),
                                  _p(self.field), _p(self.area))
        assert rc == 0 and np.array_equal(co2, self.co) and np.array_equal(cvo2, self.cvo)

    def cells(self, i, with_src=False):
        out = []
        for k in range(self.co[i], self.co[i + 1]):
            sl = slice(self.ovo[k], self.ovo[k + 1])
            xy = np.column_stack([self.x[sl], self.y[sl]])
            out.append((xy, self.src[sl]) if with_src else xy)
        assert self.ovo[self.co[i]] == self.cvo[i] and self.ovo[self.co[i + 1]] == self.cvo[i + 1]
        return out
