"""The inputs of the GA path tests and what can be said about them without a GPU (a helper, not a test file).

fcpp_ga_evolve chooses between code paths by sizes (tour length, population, elite count, tournament size, compute units) and by DATA:
fitness ties, how many of a tournament's 16 first draws are distinct, how many members beat the last elite of the generation before, how
many of the elites sit in one key class i % 16.  A test that names a data-dependent path has to show that its input takes it.  That is done
once, here and on the CPU (tests/test_ga_paths_host.py), from the oracle and the Philox stream alone; tests/test_gpu_ga_paths.py imports
the same rows and relies on it.  Three pieces:

  predictions   tour length, fitness, elites and tournament winners restated in plain numpy, sharing no code with the oracle: what a
                run of ONE generation must give (the only setting in which the final population is a pure function of the initial one).
  tournaments   the 16 draws per tournament replayed with orc.philox4x32: how many tournaments have k distinct values among them (the
                wavefront's fast path) and how many fall back to the sequential draw.
  candidates    C_g, the number of candidates the short elite selection gathers in generation g, and the largest number of the top E
                members in one key class, from the oracle's populations after g = 0 .. G - 1 generations (a prefix run is the same run:
                every decision is a function of (seed, generation, pair)).
"""
import numpy as np

import oracle as orc

CFG_KEYS = ('max_generations', 'crossover_rate', 'mutation_rate', 'elite_size', 'tournament_size', 'convergence_threshold')
NEVER = 1 << 20          # a convergence threshold no run reaches
ELITE_CAND = 256         # candidates the short elite selection ranks (GA_ELITE_CAND, fcpp_ga.hip)
ELITE_FIRST = 6          # depth of the per-wavefront lists before they are continued (ELITE_FIRST, fcpp_ga.hip)
KEY_CLASSES = 16         # member i belongs to wavefront i % 16 of the bookkeeping workgroup


def config(**kw):
    c = dict(max_generations=4, crossover_rate=0.85, mutation_rate=0.3, elite_size=3, tournament_size=5, convergence_threshold=NEVER)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def problem(seed, n, pop, asym=False, rounded=False):
    """-> D (n x n), routes (pop x n int32).  rounded: integer distances, so that different tours tie in fitness exactly"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1000, size=(n, 2))
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    if asym:
        D = D + rng.uniform(0, 5, size=D.shape)
    if rounded:
        D = np.round(D)
    routes = np.array([rng.permutation(n) for _ in range(pop)], dtype=np.int32)
    return D, routes


def oracle_run(D, routes, cfg, seed):
    """-> (final population, best route, best history, mean history, result) of the oracle"""
    return orc.ga_evolve(D, routes, population_size=len(routes), seed=seed, **{k: cfg[k] for k in CFG_KEYS})


# ---- independent predictions (no oracle) ------------------------------------------------------------------------------------------------
def tour_length(route, D):
    """GA:174-181: the left-to-right float64 sum (np.cumsum adds in order; np.sum's pairwise order differs)"""
    r = np.asarray(route)
    return float(np.cumsum(D[r, np.roll(r, -1)])[-1])


def fitness(routes, D):
    return np.array([1.0 / (tour_length(r, D) + 1e-6) for r in routes])          # GA:172


def elite_order(fit, E):
    """the E best members in the order (fitness descending, index descending)"""
    return sorted(range(len(fit)), key=lambda i: (-fit[i], -i))[:E]


def elite_rows(routes, fit, E):
    """-> the last E rows of the next population: the t-th best goes to row pop - 1 - t (GA:254-268)"""
    return routes[elite_order(fit, E)[::-1]] if E else routes[:0]


def tournament_winner(fit, cand):
    """np.argmax over the candidates' fitness: the FIRST maximum wins (GA:189-194)"""
    cand = np.asarray(cand)
    return int(cand[int(np.argmax(fit[cand]))])


def whole_population_children(D, routes, E):
    """The population after ONE generation with both rates 0 and tournament_size = population_size: every tournament sees every member, so
    -- the maximum being unique, which is asserted -- every child is the fittest member whatever order the draws come in."""
    fit = fitness(routes, D)
    assert (fit == fit.max()).sum() == 1
    w = tournament_winner(fit, np.arange(len(routes)))
    pop = len(routes)
    return np.vstack([np.repeat(routes[w][None, :], pop - E, axis=0), elite_rows(routes, fit, E)]).astype(np.int32)


# ---- the tournaments' path ----------------------------------------------------------------------------------------------------------------
def tournament_paths(seed, generations, pop, k):
    """-> dict(fast, sequential: (generation, pair, slot) tournaments with / without k distinct values among their first 16 draws;
    fast_pairs, sequential_pairs: pairs whose two tournaments both have them / do not -- a wavefront leaves the fast path for BOTH its
    tournaments when either lacks them)"""
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    out = dict(fast=0, sequential=0, fast_pairs=0, sequential_pairs=0)
    for g in range(generations):
        for p in range(pop // 2):
            ok = []
            for slot in range(2):
                draws = [w % pop for blk in range(4) for w in orc.philox4x32((g, p, 1 + slot, blk), key)]
                ok.append(len(set(draws)) >= k)
                out['fast' if ok[-1] else 'sequential'] += 1
            out['fast_pairs' if all(ok) else 'sequential_pairs'] += 1
    return out


# ---- the elite selection's path -----------------------------------------------------------------------------------------------------------
def class_count(fit, E):
    """the largest number of the top E members in one key class"""
    return int(np.bincount(np.array(elite_order(fit, E), dtype=np.int64) % KEY_CLASSES, minlength=KEY_CLASSES).max()) if E else 0


def elite_candidates(D, routes, cfg, seed, G):
    """-> (C, classes): for g = 0 .. G - 1 the candidates the short selection gathers among population g --
    C_g = #{f > thr_(g-1)} + #{i >= pop - E, f <= thr_(g-1)}, thr_g = the fitness of the last elite of population g, thr_(-1) = 0 -- and the
    largest number of population g's elites in one key class.  The run must not converge within G generations."""
    E, pop = cfg['elite_size'], len(routes)
    C, classes, thr = [], [], 0.0
    for g in range(G):
        P, _, _, _, res = oracle_run(D, routes, dict(cfg, max_generations=g, convergence_threshold=NEVER), seed)
        assert res.generations == g
        f = fitness(P, D)
        i = np.arange(pop)
        C.append(int((f > thr).sum() + ((i >= pop - E) & (f <= thr)).sum()))
        classes.append(class_count(f, E))
        thr = f[elite_order(f, E)[-1]]
    return C, classes


def into_one_class(D, routes, E, cls=5):
    """the same rows permuted so that the E best of them sit at the indices cls + 16 q: ONE wavefront of the bookkeeping workgroup owns all"""
    pop = len(routes)
    assert cls + KEY_CLASSES * (E - 1) < pop
    best = elite_order(fitness(routes, D), E)
    slots = [cls + KEY_CLASSES * q for q in range(E)]
    rest_rows = [i for i in range(pop) if i not in set(best)]
    rest_slots = [i for i in range(pop) if i not in set(slots)]
    out = np.empty_like(routes)
    out[slots] = routes[best]
    out[rest_slots] = routes[rest_rows]
    return out


def with_duplicates(D, routes, copies=(7, 5, 3)):
    """the worst rows replaced by copies of the best, the second best, ...: exact fitness ties among the elites"""
    order = elite_order(fitness(routes, D), len(routes))
    out = routes.copy()
    worst = len(order) - 1
    for rank, m in enumerate(copies):
        for _ in range(m):
            out[order[worst]] = routes[order[rank]]
            worst -= 1
    return out


def threshold_for(best_history, first_best, generations):
    """the convergence threshold with which a run whose best-fitness history (threshold NEVER) is best_history stops after exactly
    `generations` generations: the count of generations without improvement there, which no earlier generation may have reached (GA:94-113)"""
    gwi, trace, best = 0, [], first_best
    for b in best_history:
        gwi = 0 if b > best else gwi + 1
        best = max(best, b)
        trace.append(gwi)
    T = trace[generations - 1]
    assert T >= 1 and all(t < T for t in trace[:generations - 1]), trace
    return T


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
# tours: both sides of the 64-lane chunk edges, of the long-tour body (n > 256, nchunk 4 -> 5) and of the one-launch limit (398 / 399)
SIZE_EDGES = (3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 320, 398, 399)
SIZE_POP, SIZE_CFG = 34, config(max_generations=5, elite_size=3, tournament_size=5)
ONE_LAUNCH_MAX_N = 398

# small k in a tiny population: fewer than k distinct values among 16 draws happens, and does not always happen.  The seeds were searched
# for; tests/test_ga_paths_host.py asserts that both kinds occur with them.
FALLBACK_ROWS = [            # (pop, k, seed, generations)
    (8, 8, 101, 6),
    (10, 8, 102, 6),
    (16, 7, 102, 6),         # (one sequential pair among 48)
]


def fallback_problem(pop, k, seed, generations):
    D, routes = problem(seed, 12, pop)
    return D, routes, config(max_generations=generations, elite_size=1, tournament_size=k)


def midrun_problem(E, k):
    """both rates 0: the population collapses into copies, so many members EQUAL the last elite's fitness -- more than 256 beat the threshold
    of the generation before at first, none does in the end"""
    rng = np.random.default_rng(3)
    n, pop = 24, 1024
    pts = rng.uniform(0, 1000, size=(n, 2))
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    routes = np.array([rng.permutation(n) for _ in range(pop)], dtype=np.int32)
    return D, routes, config(max_generations=6, crossover_rate=0.0, mutation_rate=0.0, elite_size=E, tournament_size=k)


MIDRUN_ROWS = [(20, 32), (64, 64)]          # (E, k)
MIDRUN_SEED = 11


def deeper_problem(duplicates, pop=512, E=20):
    D, routes = problem(40 + int(duplicates), 24, pop)
    if duplicates:
        routes = with_duplicates(D, routes)
    return D, into_one_class(D, routes, E), config(max_generations=4, elite_size=E, tournament_size=5)


ELITE_ROWS = ('E0', 'E1', 'E64_pop258', 'E64_pop1024_one_class', 'E65_pop66', 'E129_pop130', 'deeper', 'deeper_ties', 'midrun_E20', 'midrun_E64',
              'pop6146_E5', 'pop6146_E64')
ELITE_SEED = 5


def elite_problem(row):
    """-> D, routes, cfg, seed of a row of ELITE_ROWS"""
    return _elite_problem(row) + (MIDRUN_SEED if row.startswith('midrun') else ELITE_SEED,)


def _elite_problem(row):
    """-> D, routes, cfg of a row of ELITE_ROWS.  Short way: E0 (nothing to do), E1; per-wavefront lists at generation 0 of every row with
    256 < pop <= 6144 and E <= 64, exhausted in E64_pop258, continued past their first depth where a key class holds 6 or more of the elites
    (E64_pop258, E64_pop1024_one_class, deeper*), entered again in mid-run by midrun_*; the general path for E >= 65 and for pop > 6144."""
    if row in ('E0', 'E1'):
        D, routes = problem(50, 20, 40)
        return D, routes, config(elite_size=int(row[1:]))
    if row == 'E64_pop258':
        D, routes = problem(7, 20, 258)
        return D, routes, config(elite_size=64)
    if row == 'E64_pop1024_one_class':
        D, routes = problem(52, 24, 1024)
        return D, into_one_class(D, routes, 64), config(elite_size=64)
    if row in ('E65_pop66', 'E129_pop130'):
        E, pop = (65, 66) if row == 'E65_pop66' else (129, 130)
        D, routes = problem(53, 20, pop)
        return D, routes, config(elite_size=E)
    if row in ('deeper', 'deeper_ties'):
        return deeper_problem(row == 'deeper_ties')
    if row in ('midrun_E20', 'midrun_E64'):
        return midrun_problem(*MIDRUN_ROWS[row == 'midrun_E64'])
    D, routes = problem(54, 16, 6146)
    return D, routes, config(max_generations=3, elite_size=int(row.split('_E')[1]))


def stop_problem(n, generations, seed=21):
    """both rates 0: a run that stops after exactly `generations` generations, the threshold read off the oracle's own trace"""
    D, routes = problem(seed, n, 16)
    cfg = config(max_generations=70, crossover_rate=0.0, mutation_rate=0.0, elite_size=2, tournament_size=3)
    hb = oracle_run(D, routes, cfg, seed)[2]
    assert len(hb) == 70
    return D, routes, dict(cfg, convergence_threshold=threshold_for(hb, fitness(routes, D).max(), generations)), seed
