"""GPU: the GA's and the scheduler inputs' C entries through the guarded arena (tests/guarded.py), in the style of tests/test_gpu_guarded.py.

fcpp_ga_evolve, fcpp_ga_fitness, fcpp_distance_matrix and fcpp_best_connections are called directly (ctx.lib) on slots carved out of one
uint8 CUDA tensor: 256 guard bytes around every slot, outputs pre-filled, every pointer only naturally aligned (the int32 population at an
address that is 4 mod 8, doubles at 8 mod 16).  After each call the guards are intact, the inputs have the bits that were put in, every
output element has the expected bits, and the optional outputs (hist; dist or fit) may be NULL.  The population of fcpp_ga_evolve is an
in-out slot: it holds the initial population, and the final one afterwards.  Expected values: the oracle, and plain numpy for the tree sum."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from field_coverage_path_planning_amd import _lib as L
from tests import ga_cases as G
from tests.guarded import Arena
from tests.test_gpu_guarded import gpu  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _plan_one_launch(gpu, n, pop):
    out = np.zeros(6, dtype=np.int32)
    gpu.ok(gpu.lib.fcpp_debug_ga_launch_plan(gpu.h, n, pop, C.c_void_p(out.ctypes.data)))
    return bool(out[0])


@pytest.mark.parametrize('with_hist', [True, False], ids=['hist', 'hist_null'])
@pytest.mark.parametrize('n,pop', [(24, 20), (520, 12)], ids=['one_launch', 'two_streams'])
def test_ga_evolve(gpu, n, pop, with_hist):
    assert _plan_one_launch(gpu, n, pop) == (n == 24)
    D, routes = G.problem(700 + n, n, pop)
    cfg = G.config(max_generations=5, elite_size=3, tournament_size=4)
    seed = 4242
    ofinal, obest, ohb, oha, ores = G.oracle_run(D, routes, cfg, seed)
    assert ores.generations == cfg['max_generations'] and not np.array_equal(ofinal, routes)          # every hist element is written
    A = Arena().input('D', D).inout('routes', routes).output('best_route', np.int32, n)
    if with_hist:
        A.output('hist', np.float64, 2 * cfg['max_generations'])
    A.build(gpu.dev)
    assert A.address('routes') % 8 == 4
    c = L.GaConfig(pop, cfg['max_generations'], cfg['crossover_rate'], cfg['mutation_rate'], cfg['elite_size'], cfg['tournament_size'],
                   cfg['convergence_threshold'], 0, seed)
    res = L.GaResult()
    gpu.ok(gpu.lib.fcpp_ga_evolve(gpu.h, n, C.byref(c), A.ptr('D'), A.ptr('routes'), A.ptr('best_route'), A.ptr('hist'), C.byref(res)))
    want = {'routes': ofinal.reshape(-1), 'best_route': obest}
    if with_hist:
        want['hist'] = np.concatenate([ohb, oha])
    A.check(want)
    assert (res.generations, res.convergence_gen, res.best_distance, res.best_fitness) == \
        (ores.generations, ores.convergence_gen, ores.best_distance, ores.best_fitness)


def _tree_sum(terms):
    """fcpp_ga_fitness' order_mode 1: lane l adds the terms l, l + 64, ... in order, then a butterfly over the 64 lanes (xor 32, 16, .. 1)"""
    t = np.zeros(64)
    for k, v in enumerate(terms):
        t[k % 64] += v
    for o in (32, 16, 8, 4, 2, 1):
        t = t + t[np.arange(64) ^ o]
    return t[0]


@pytest.mark.parametrize('order_mode', [0, 1], ids=['left_to_right', 'tree'])
@pytest.mark.parametrize('n', [1, 64, 65])
def test_ga_fitness(gpu, n, order_mode):
    pop = 7          # the kernel takes four chromosomes a workgroup: the second workgroup has three
    rng = np.random.default_rng(800 + n)
    D = rng.uniform(1.0, 1000.0, size=(n, n))          # (no zero diagonal: a tour of one node has the length D[0, 0])
    routes = np.array([rng.permutation(n) for _ in range(pop)], dtype=np.int32)
    terms = [D[r, np.roll(r, -1)] for r in routes]
    if order_mode == 0:
        dist = np.array([G.tour_length(r, D) for r in routes])
        if n > 1:
            assert np.array_equal(dist, orc.ga_distance(routes, D))
    else:
        dist = np.array([_tree_sum(t) for t in terms])
    want = {'dist': dist, 'fit': 1.0 / (dist + 1e-6)}
    for outs in (('dist', 'fit'), ('fit',), ('dist',)):
        A = Arena().input('D', D).input('routes', routes)
        for k in outs:
            A.output(k, np.float64, pop)
        A.build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_ga_fitness(gpu.h, n, pop, A.ptr('D'), A.ptr('routes'), A.ptr('dist'), A.ptr('fit'), order_mode))
        A.check({k: want[k] for k in outs})


def test_distance_matrix(gpu):
    n = 257          # one column over the 256-thread block
    xy = np.random.default_rng(257).uniform(-500.0, 500.0, size=(n, 2))
    A = Arena().input('x', xy[:, 0]).input('y', xy[:, 1]).output('D', np.float64, n * n).build(gpu.dev)
    gpu.ok(gpu.lib.fcpp_distance_matrix(gpu.h, n, A.ptr('x'), A.ptr('y'), A.ptr('D')))
    want = orc.distance_matrix(xy)
    assert np.array_equal(want, np.sqrt((xy[:, None, 0] - xy[None, :, 0]) ** 2 + (xy[:, None, 1] - xy[None, :, 1]) ** 2))
    A.check({'D': want.reshape(-1)})


def test_best_connections(gpu):
    rng = np.random.default_rng(31)
    pts = lambda k: rng.uniform(-500.0, 500.0, size=(k, 2))
    # an empty exit list, an empty entry list, one candidate each, more products than lanes (9 x 8 and 65 x 1), every distance twice
    fl = [pts(0), pts(3), pts(1), pts(9), pts(65), pts(2)]
    tl = [pts(4), pts(0), pts(1), pts(8), pts(1), pts(3)]
    tl[5] = np.vstack([tl[5], tl[5][::-1]])
    assert [len(a) * len(b) for a, b in zip(fl, tl)] == [0, 0, 1, 72, 65, 12]
    fo = np.concatenate([[0], np.cumsum([len(a) for a in fl])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(a) for a in tl])]).astype(np.int64)
    fxy, txy = np.vstack(fl), np.vstack(tl)
    bf, bt, bd = [], [], []
    for p in range(len(fl)):
        a, b, d = orc.best_connection(fl[p], tl[p])
        bf.append(-1 if a < 0 else fo[p] + a); bt.append(-1 if b < 0 else to[p] + b); bd.append(d)
    assert bf[0] == bt[1] == -1 and np.isinf(bd[:2]).all() and bt[5] - to[5] < 3          # the first of two equal products wins
    A = Arena().input('fo', fo).input('to', to).input('fx', fxy[:, 0]).input('fy', fxy[:, 1]).input('tx', txy[:, 0]).input('ty', txy[:, 1])
    A.output('bf', np.int32, len(fl)).output('bt', np.int32, len(fl)).output('bd', np.float64, len(fl)).build(gpu.dev)
    gpu.ok(gpu.lib.fcpp_best_connections(gpu.h, len(fl), *[A.ptr(k) for k in ('fo', 'to', 'fx', 'fy', 'tx', 'ty', 'bf', 'bt', 'bd')]))
    A.check({'bf': np.array(bf, dtype=np.int32), 'bt': np.array(bt, dtype=np.int32), 'bd': np.array(bd)})
