"""Host checks of the transdimensional Voronoi-cell step (no
GPU): the library's host helpers against the restatement tests/_vor.py, the
raster's rules, and the exact reversibility of the four moves under the stated
prior, which is the claim that no Hastings factor is needed."""
import itertools
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import _vor as V
from mceik_amd import mcmc


def test_free_cell_is_a_bijection_onto_the_free_cells():
    ncell = 12
    g = np.random.default_rng(3)
    for k in range(ncell):
        for _ in range(4):
            cells = [int(c) for c in g.permutation(ncell)[:k]]      # unsorted: list order must not matter
            free = [c for c in range(ncell) if c not in cells]
            got = [V.free_cell(cells, f) for f in range(ncell - k)]
            assert got == free
            assert [mcmc.vor_free_cell(cells, ncell, f) for f in range(ncell - k)] == free
    for bad in ((lambda: mcmc.vor_free_cell([0, 1], 12, 10)), (lambda: mcmc.vor_free_cell([12], 12, 0)),
                (lambda: mcmc.vor_free_cell([], 12, -1))):
        with pytest.raises(ValueError):
            bad()


def test_draw_equals_the_restatement():
    for seed, g, gs, k in itertools.product((1, 2016), (0, 7), (0, 5, (1 << 32) + 3), (1, 3, 64)):
        want = V.draw(seed, g, gs, k, 64, 25, 1000, 9000, (1, 2, 0))
        got = mcmc.vor_draw(seed, g, gs, k, 64, 25, 1000, 9000, (1, 2, 0))
        for key in ("type", "j", "f", "delta", "wnew", "d"):
            assert got[key] == want[key], key
        assert np.float64(got["logu"]).view(np.uint64) == np.float64(want["logu"]).view(np.uint64)
    assert V.start_cells(5, 3, 0, 12, 12) != V.start_cells(5, 4, 0, 12, 12)
    assert sorted(V.start_cells(5, 3, 1, 12, 12)) == list(range(12))     # distinct cells, here all of them


GRIDS = ((4, 4, 4), (6, 4, 3))


@pytest.mark.parametrize("grid", GRIDS)
def test_raster_rules(grid):
    ncell = grid[0] * grid[1] * grid[2]
    for name, cells, vals, metric in V.raster_cases(grid):
        want = V.raster(grid, cells, vals, metric)
        got = mcmc.vor_raster(grid, cells, vals, metric)
        assert np.array_equal(got, want), name
        perm = np.random.default_rng(9).permutation(len(cells))      # list order never changes the model
        assert np.array_equal(mcmc.vor_raster(grid, np.asarray(cells)[perm], np.asarray(vals)[perm], metric), want), name
        if name == "k1":
            assert (got == vals[0]).all()
        if name == "kmax" and len(cells) == ncell:
            assert np.array_equal(got[np.asarray(cells)], np.asarray(vals))
        if name == "ties":
            assert got[1] == vals[1] and got[0] == vals[1] and got[2] == vals[0]     # the tie on cell 1 goes to the nucleus in cell 0
    # every nucleus owns its own cell
    name, cells, vals, metric = V.raster_cases(grid)[1]
    assert np.array_equal(mcmc.vor_raster(grid, cells, vals, metric)[np.asarray(cells)], np.asarray(vals))
    # the metric matters: doubling z moves a boundary
    a = mcmc.vor_raster((1, 4, 4), [0, 15], [1, 2], (1, 1, 1))
    b = mcmc.vor_raster((1, 4, 4), [0, 15], [1, 2], (1, 1, 2))
    assert np.array_equal(a, V.raster((1, 4, 4), [0, 15], [1, 2])) and not np.array_equal(a, b)
    with pytest.raises(ValueError):
        mcmc.vor_raster(grid, [ncell], [1])
    with pytest.raises(ValueError):
        mcmc.vor_raster((40000, 1, 1), [0], [1], (2, 1, 1))          # 79998^2 does not fit 31 bits


def test_the_four_moves_leave_the_prior_invariant():
    """2 x 2 x 1 cells, two admissible values, 1 <= k <= 3: the transition matrix
    of the proposal under a flat likelihood (every valid move accepted: log u <
    0 always), built from the exact share of 32-bit words behind every outcome,
    has the stated prior as a stationary distribution -- uniform on k, on sets
    of k distinct cells and on values -- to 1e-9 (floor(r n / 2^32) is uniform
    only to n 2^-32)."""
    grid, ncell, kmin, kmax, vlo, vhi, dv, dmax = (2, 2, 1), 4, 1, 3, 5, 6, 1, (1, 1, 0)
    nv = vhi - vlo + 1
    states = []
    for k in range(kmin, kmax + 1):
        for cells in itertools.combinations(range(ncell), k):
            for vals in itertools.product(range(vlo, vhi + 1), repeat=k):
                states.append(tuple(zip(cells, vals)))
    index = {s: i for i, s in enumerate(states)}
    assert len(states) == sum(comb(ncell, k) * nv ** k for k in range(kmin, kmax + 1)) == 64
    pi = np.array([1.0 / ((kmax - kmin + 1) * comb(ncell, len(s)) * nv ** len(s)) for s in states])
    assert abs(pi.sum() - 1.0) < 1e-15
    P = np.zeros((len(states), len(states)))
    seen = set()
    for s in states:
        draws = V.draws_with_probability(len(s), ncell, dv, vlo, vhi, dmax)
        assert sum(pr for pr, _ in draws) == Fraction(1)             # every word is counted once
        for pr, d in draws:
            reason, _, _, _, prop = V.apply(list(s), d, kmin, kmax, vlo, vhi, grid)
            seen.add((d["type"], reason))
            P[index[s], index[tuple(sorted(prop))]] += float(pr)
    assert seen == set(V.OUTCOMES)                                   # every move type and rejection reason took part
    assert np.abs(P.sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(pi @ P - pi).max() < 1e-9
    # detailed balance too (each move is its own reverse's partner), and the chain is irreducible: pi is THE answer
    F = pi[:, None] * P
    assert np.abs(F - F.T).max() < 1e-9
    reach = np.linalg.matrix_power((P > 0).astype(np.float64) + np.eye(len(states)), len(states)) > 0
    assert reach.all()
    # the control: a birth that did not draw its value from the prior's whole box would need a Hastings factor
    Q = np.zeros_like(P)
    for s in states:
        for pr, d in V.draws_with_probability(len(s), ncell, dv, vlo, vhi, dmax):
            if d["type"] == V.BIRTH:
                d = dict(d, wnew=vlo)
            prop = V.apply(list(s), d, kmin, kmax, vlo, vhi, grid)[4]
            Q[index[s], index[tuple(sorted(prop))]] += float(pr)
    assert np.abs(pi @ Q - pi).max() > 1e-3
