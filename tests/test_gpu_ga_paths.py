"""GPU: every device path and size edge of the GA evolution loop (fcpp_ga_evolve, fcpp_ga.hip) against the oracle, bit for bit.

tests/test_gpu_ga.py pins eight configurations; fcpp_ga.hip chooses between code paths by tour length, population, elite count, tournament
size, compute units and by the data.  Each group below names the path it pins and PROVES it takes it: through fcpp_debug_ga_launch_plan
(what the launcher will do for (n, pop) on this device) or through a condition tests/test_ga_paths_host.py shows on the CPU for the same
rows of tests/ga_cases.py.  Every row compares the final population, the best route, both histories, generations, convergence_gen, best
distance and fitness with the oracle's replay exactly, and checks that every final row is a permutation; rows of one generation are also
held against the numpy predictions of tests/ga_cases.py, which share no code with the oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import ga_cases as G

pytestmark = pytest.mark.gpu

PLAN_FIELDS = ('one_launch', 'groups', 'base', 'extra', 'per_wg', 'lds')
SEARCH_N = 32          # tour length of the pair-spreading rows


def plan(n, pop):
    """what fcpp_ga_evolve launches for (n, pop) on this device"""
    ctx = E.get_context(None)
    out = np.full(6, -1, dtype=np.int32)
    L.check(ctx.lib.fcpp_debug_ga_launch_plan(ctx.handle, n, pop, C.c_void_p(out.ctypes.data)))
    return SimpleNamespace(**dict(zip(PLAN_FIELDS, (int(v) for v in out))))


def run(D, routes, cfg, seed):
    """device against oracle, everything exact -> (final population, the oracle's result)"""
    n = D.shape[0]
    final, best, hb, ha, res = E.ga_evolve(D, routes, SimpleNamespace(**cfg), seed=seed)
    ofinal, obest, ohb, oha, ores = G.oracle_run(D, routes, cfg, seed)
    final = final.cpu().numpy()
    assert (res.generations, res.convergence_gen) == (ores.generations, ores.convergence_gen)
    assert res.best_distance == ores.best_distance and res.best_fitness == ores.best_fitness
    assert np.array_equal(final, ofinal) and np.array_equal(best.cpu().numpy(), obest)
    assert np.array_equal(hb, ohb) and np.array_equal(ha, oha)
    assert np.array_equal(np.sort(final, axis=1), np.broadcast_to(np.arange(n, dtype=np.int32), final.shape))
    return final, ores


# ---- size edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rounded', [False, True], ids=['plain', 'rounded'])
@pytest.mark.parametrize('n', G.SIZE_EDGES)
def test_size_edges(n, rounded):
    """both bodies of ga_pair (n <= 256: terms of both children at once; longer: child by child) inside k_ga_generation's per-wavefront LDS
    slices, up to the last n of the one-launch path and the first of the two-stream path; an odd elite count splits the last pair's rows"""
    p = plan(n, G.SIZE_POP)
    assert p.one_launch == (n <= G.ONE_LAUNCH_MAX_N)
    if p.one_launch:
        assert (p.groups, p.base, p.extra, p.per_wg) == ((G.SIZE_POP // 2 + 7) // 8, 8, 0, 8)
    else:
        assert (p.groups, p.per_wg) == (G.SIZE_POP // 2, 1)
    if n == G.ONE_LAUNCH_MAX_N:
        assert p.lds == 60 * 1024          # the most dynamic LDS the launcher ever asks for, beside the kernel's static arrays
    D, routes = G.problem(300 + n, n, G.SIZE_POP, rounded=rounded)
    assert G.SIZE_CFG['elite_size'] % 2 == 1
    run(D, routes, G.SIZE_CFG, 1000 + n)


def test_asymmetric_matrix_long_tour():
    D, routes = G.problem(557, 257, G.SIZE_POP, asym=True)
    assert not np.array_equal(D, D.T) and plan(257, G.SIZE_POP).one_launch
    run(D, routes, G.SIZE_CFG, 557)


# ---- pair spreading (ga_pair_groups) ----------------------------------------------------------------------------------------------------------
def _search(want, what):
    """the first even population <= 6144 whose plan satisfies `want`"""
    for pop in range(16, 6145, 2):
        p = plan(SEARCH_N, pop)
        if p.one_launch and want(p):
            return pop, p
    pytest.fail('no population <= 6144 has %s on this device (too few compute units?)' % what)


def _spread_case(kind):
    if kind == 'extra':
        return (SEARCH_N,) + _search(lambda p: p.extra > 0 and p.per_wg > 8, 'uneven workgroups of more than 8 pairs')
    if kind == 'even':
        return (SEARCH_N,) + _search(lambda p: p.extra == 0 and p.base > 8, 'even workgroups of more than 8 pairs')
    n = SEARCH_N if kind == 'pop6144' else 240
    return n, 6144, plan(n, 6144)


@pytest.mark.parametrize('kind', ['extra', 'even', 'pop6144', 'lds_fallback'])
def test_pair_spreading(kind):
    n, pop, p = _spread_case(kind)
    print('launch plan', kind, dict(n=n, pop=pop, **vars(p)))
    pairs = pop // 2
    assert p.one_launch and p.groups * p.base + p.extra == pairs and p.per_wg == p.base + (p.extra > 0)
    if kind == 'lds_fallback':
        # the tours' LDS does not fit more than eight pairs: eight a workgroup, though the same population of short tours is spread
        assert (p.groups, p.base, p.extra, p.per_wg) == (pairs // 8, 8, 0, 8)
        q = plan(SEARCH_N, pop)
        if q.per_wg <= 8:
            pytest.fail('population 6144 is not spread over more than 8 pairs a workgroup on this device: %r' % vars(q))
        pair_lds = plan(n, 16).lds // 8          # (eight pairs in one workgroup, a population too small to matter: 8 x a pair's LDS)
        assert pair_lds * 8 <= 60 * 1024 < pair_lds * q.per_wg
    else:
        if p.per_wg <= 8:
            pytest.fail('population %d is not spread over more than 8 pairs a workgroup on this device: %r' % (pop, vars(p)))
        assert p.per_wg <= 16 and p.lds <= 60 * 1024
        assert kind == 'pop6144' or (p.extra > 0) == (kind == 'extra')
        # the plan is made for the context's own device: the pairs go to (its compute units - 2) workgroups
        ctx = E.get_context(None)
        cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
        assert p.groups == min(pairs, cu - 2)
    D, routes = G.problem(pop, n, pop)
    run(D, routes, G.config(max_generations=3, elite_size=7, tournament_size=5), pop)


# ---- tournaments --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pop,k,seed,generations', G.FALLBACK_ROWS)
def test_tournament_fallback(pop, k, seed, generations):
    """k <= 8 with fewer than k distinct values among a tournament's 16 draws: the wavefront leaves its fast path for the sequential draw
    (both kinds of pair occur in these runs: tests/test_ga_paths_host.py)"""
    D, routes, cfg = G.fallback_problem(pop, k, seed, generations)
    _, res = run(D, routes, cfg, seed)
    assert res.generations == generations


@pytest.mark.parametrize('k', [9, 33, 63, 64])
def test_sequential_tournaments(k):
    D, routes = G.problem(80 + k, 17, 64)
    run(D, routes, G.config(elite_size=4, tournament_size=k), 900 + k)


# ---- elites -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', G.ELITE_ROWS)
def test_elites(row):
    D, routes, cfg, seed = G.elite_problem(row)
    n, pop, E_ = D.shape[0], len(routes), cfg['elite_size']
    assert plan(n, pop).one_launch == (pop <= 6144)
    run(D, routes, cfg, seed)
    # one generation: the last E rows are the numpy elites of the initial population
    final, _ = run(D, routes, dict(cfg, max_generations=1), seed)
    assert np.array_equal(final[pop - E_:], G.elite_rows(routes, G.fitness(routes, D), E_))


def test_identical_rows():
    """every fitness equal: every tie-break at once (first arg-max, tournaments' first maximum, elites by the larger index, 300 candidates)"""
    D, routes = G.problem(90, 20, 300)
    routes[:] = routes[0]
    cfg = G.config(max_generations=5, elite_size=10)
    final, _ = run(D, routes, cfg, 90)
    assert len(np.unique(final, axis=0)) > 1          # (mutations: the later generations are not all ties)
    final, _ = run(D, routes, dict(cfg, max_generations=1, crossover_rate=0.0, mutation_rate=0.0), 90)
    assert np.array_equal(final, routes)


# ---- children that do not depend on the random stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize('pop,E_', [(2, 1), (8, 3), (64, 5)])
def test_children_without_philox(pop, E_):
    D, routes = G.problem(60 + pop, 9, pop)
    cfg = G.config(max_generations=1, crossover_rate=0.0, mutation_rate=0.0, elite_size=E_, tournament_size=pop)
    final, _ = run(D, routes, cfg, 77)
    assert np.array_equal(final, G.whole_population_children(D, routes, E_))


# ---- edges of the loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [24, 520])
@pytest.mark.parametrize('generations', [0, 1])
def test_no_and_one_generation(n, generations):
    D, routes = G.problem(70, n, 16)
    assert plan(n, 16).one_launch == (n == 24)
    final, res = run(D, routes, G.config(max_generations=generations), 9)
    assert res.generations == generations
    if generations == 0:
        assert np.array_equal(final, routes) and res.convergence_gen == -1
    else:
        assert np.array_equal(final[-3:], G.elite_rows(routes, G.fitness(routes, D), 3))


@pytest.mark.parametrize('n', [24, 520])
@pytest.mark.parametrize('generations', [31, 32, 33])
def test_stop_around_the_pipelined_check(n, generations):
    """the host looks at the run's progress after every 32nd launch ((g & 31) == 31): a run that stops just before, at and just after it"""
    D, routes, cfg, seed = G.stop_problem(n, generations)
    assert plan(n, len(routes)).one_launch == (n == 24)
    _, res = run(D, routes, cfg, seed)
    assert res.generations == generations


def test_seed_with_bit_63():
    D, routes = G.problem(95, 30, 40)
    seed = (1 << 63) | 0x1234_5678_9ABC
    final, _ = run(D, routes, G.config(), seed)
    other, _ = run(D, routes, G.config(), seed ^ (1 << 63))
    assert not np.array_equal(final, other)          # the top bit is part of the key
