"""CPU: the inputs of tests/test_gpu_ga_paths.py take the paths they are named after, and the oracle agrees with plain numpy.

Everything here runs on the reference side alone (the oracle's replay, the Philox stream, numpy): the rows of tests/ga_cases.py whose
device path depends on the DATA -- a tournament with fewer than k distinct values among its 16 draws, more than 256 candidates for the short
elite selection in mid-run, all elites in one key class, a wavefront's exhausted list, the generation a run stops in -- are shown to have
that property, so the device tests need not take it on trust.  Then the oracle itself is held against the independent predictions in the
one setting where the outcome does not depend on its random stream: one generation."""
import numpy as np
import pytest

from tests import ga_cases as G


@pytest.mark.parametrize('pop,k,seed,generations', G.FALLBACK_ROWS)
def test_fallback_rows_take_both_tournament_paths(pop, k, seed, generations):
    D, routes, cfg = G.fallback_problem(pop, k, seed, generations)
    assert k <= 8 and G.oracle_run(D, routes, cfg, seed)[4].generations == generations          # (every counted generation is run)
    paths = G.tournament_paths(seed, generations, pop, k)
    assert paths['fast'] > 0 and paths['sequential'] > 0, paths
    assert paths['fast_pairs'] > 0 and paths['sequential_pairs'] > 0, paths
    assert paths['fast'] + paths['sequential'] == generations * pop


def test_tournament_counter_on_known_streams():
    # k = 1: one draw is one distinct value; k = 16 of 16 draws from a population of 64: a repeat among them is all but certain somewhere
    assert G.tournament_paths(1, 3, 8, 1) == dict(fast=24, sequential=0, fast_pairs=12, sequential_pairs=0)
    p = G.tournament_paths(1, 3, 64, 16)
    assert p['sequential'] > 0 and p['fast'] + p['sequential'] == 3 * 64


@pytest.mark.parametrize('row', ['midrun_E20', 'midrun_E64'])
def test_midrun_rows_leave_the_short_selection_after_generation_0(row):
    D, routes, cfg, seed = G.elite_problem(row)
    C, _ = G.elite_candidates(D, routes, cfg, seed, cfg['max_generations'])
    print(row, 'C_g =', C)
    assert C[0] == len(routes)
    late = [g for g in range(1, len(C)) if C[g] > G.ELITE_CAND]
    assert late, C                                                        # the per-wavefront lists with a non-zero threshold behind them
    assert any(C[g] <= G.ELITE_CAND for g in range(late[-1] + 1, len(C))), C          # and the short way again afterwards
    assert all(c >= cfg['elite_size'] for c in C)


@pytest.mark.parametrize('row,E', [('deeper', 20), ('deeper_ties', 20), ('E64_pop1024_one_class', 64)])
def test_one_class_rows_hold_every_elite_in_one_key_class(row, E):
    D, routes, cfg, seed = G.elite_problem(row)
    fit = G.fitness(routes, D)
    assert cfg['elite_size'] == E and G.class_count(fit, E) == E
    assert sorted(G.elite_order(fit, E)) == [5 + 16 * q for q in range(E)]
    assert G.ELITE_CAND < len(routes) <= 6144                             # generation 0 ranks through the per-wavefront lists
    if row == 'deeper_ties':                                               # exact duplicates among the best rows: the larger index first
        order = G.elite_order(fit, E)
        ties = [(a, b) for a, b in zip(order[:-1], order[1:]) if fit[a] == fit[b]]
        assert len(ties) >= 10 and all(a > b and np.array_equal(routes[a], routes[b]) for a, b in ties)


def test_exhausted_lists_row():
    """pop 258, E 64: a wavefront owns 16 or 17 members, one key class holds 6 or more of the elites, so the lists are continued to 64"""
    D, routes, cfg, seed = G.elite_problem('E64_pop258')
    assert len(routes) == 258 and cfg['elite_size'] == 64
    assert G.class_count(G.fitness(routes, D), 64) >= G.ELITE_FIRST
    assert -(-258 // G.KEY_CLASSES) == 17 < 64


@pytest.mark.parametrize('row', G.ELITE_ROWS)
def test_oracle_elites_are_the_numpy_elites(row):
    D, routes, cfg, seed = G.elite_problem(row)
    E = cfg['elite_size']
    final = G.oracle_run(D, routes, dict(cfg, max_generations=1), seed)[0]
    assert np.array_equal(final[len(routes) - E:], G.elite_rows(routes, G.fitness(routes, D), E))


@pytest.mark.parametrize('pop,E', [(2, 1), (8, 3), (64, 5)])
def test_oracle_children_without_philox(pop, E):
    D, routes = G.problem(60 + pop, 9, pop)
    cfg = G.config(max_generations=1, crossover_rate=0.0, mutation_rate=0.0, elite_size=E, tournament_size=pop)
    final, best, hb, _, res = G.oracle_run(D, routes, cfg, 77)
    assert np.array_equal(final, G.whole_population_children(D, routes, E))
    fit = G.fitness(routes, D)
    assert np.array_equal(best, routes[int(np.argmax(fit))]) and hb.tolist() == [fit.max()] and res.best_fitness == fit.max()


@pytest.mark.parametrize('n', [24, 520])
def test_oracle_runs_no_generation(n):
    D, routes = G.problem(70, n, 16)
    final, best, hb, ha, res = G.oracle_run(D, routes, G.config(max_generations=0), 9)
    fit = G.fitness(routes, D)
    assert (res.generations, res.convergence_gen) == (0, -1) and len(hb) == len(ha) == 0
    assert np.array_equal(final, routes) and np.array_equal(best, routes[int(np.argmax(fit))])
    assert res.best_fitness == fit.max() and res.best_distance == G.tour_length(best, D)


@pytest.mark.parametrize('n', [24, 520])
@pytest.mark.parametrize('generations', [31, 32, 33])
def test_stop_rows_stop_where_they_say(n, generations):
    D, routes, cfg, seed = G.stop_problem(n, generations)
    res = G.oracle_run(D, routes, cfg, seed)[4]
    assert res.generations == generations < cfg['max_generations']
    assert res.convergence_gen == generations - 1 - cfg['convergence_threshold']


def test_launch_plan_entry_refuses_bad_arguments():
    import ctypes as C

    from field_coverage_path_planning_amd import _lib as L
    out = np.zeros(6, dtype=np.int32)
    assert L.load().fcpp_debug_ga_launch_plan(None, 24, 16, C.c_void_p(out.ctypes.data)) == L.EINVAL          # (no context: nothing is asked of a device)
    assert not out.any()


def test_predictions_on_hand_cases():
    D = np.array([[0.0, 1.0, 4.0], [2.0, 0.0, 8.0], [16.0, 32.0, 0.0]])
    assert G.tour_length([0, 1, 2], D) == 1.0 + 8.0 + 16.0 and G.tour_length([2, 1, 0], D) == 32.0 + 2.0 + 4.0
    # a sum whose value depends on the order: left to right 1e16 + 1 + 1 stays 1e16
    assert G.tour_length([0, 1, 2], np.array([[0, 1e16, 0], [0, 0, 1.0], [1.0, 0, 0]])) == 1e16
    fit = np.array([3.0, 5.0, 5.0, 1.0, 5.0])
    assert G.elite_order(fit, 4) == [4, 2, 1, 0]
    assert G.tournament_winner(fit, [3, 2, 4, 1]) == 2 and G.tournament_winner(fit, [0]) == 0
    rows = np.arange(10).reshape(5, 2)
    assert G.elite_rows(rows, fit, 2).tolist() == [[4, 5], [8, 9]] and len(G.elite_rows(rows, fit, 0)) == 0
    assert G.threshold_for([1.0, 2.0, 2.0, 2.0, 2.0], 1.0, 4) == 2 and G.threshold_for([1.0] * 5, 1.0, 3) == 3
