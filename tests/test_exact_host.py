"""The exact-posterior harness without a GPU (tests/_exact.py):
the statistic and its pooling, the properties every enumerated toy is chosen by,
and the harness fed by the oracle's own chains, so that it can be debugged on a
CPU-only machine."""
import math

import numpy as np
import pytest

import _exact as X
import _oracle as O


def _skewed(n=40):
    return X.normalise(-0.15 * np.arange(n, dtype=np.float64))


def test_statistic_accepts_pi_and_rejects_a_tenth_off():
    pi = _skewed()
    wrong = X.normalise(0.9 * np.log(pi))
    rng = np.random.default_rng(24)
    ps = []
    for _ in range(20):
        t = X.chi2_test(rng.multinomial(X.N_FLOOR, pi), pi)
        assert t.dof == pi.size - 1 and t.pooled == 0.0
        ps.append(t.p)
    assert min(ps) >= X.P_PASS and 0.2 < np.mean(ps) < 0.8, ps        # p is uniform under the null
    for _ in range(5):
        assert X.chi2_test(rng.multinomial(X.N_FLOOR, wrong), pi).p <= X.P_REJECT
        assert X.chi2_test(rng.multinomial(X.N_FLOOR, pi), wrong).p <= X.P_REJECT


def test_pooling_and_closed_forms():
    # three bins, dof 2: Q(1, x / 2) = exp(-x / 2)
    for counts in ([30, 50, 20], [334, 333, 333], [10, 80, 10], [500, 300, 200]):
        q = np.array([0.3, 0.5, 0.2])
        n = sum(counts)
        x2 = sum((c - n * qi) ** 2 / (n * qi) for c, qi in zip(counts, q))
        t = X.chi2_test(counts, q)
        assert t.dof == 2 and abs(t.x2 - x2) <= 1e-12 * max(1.0, x2)
        assert abs(t.p - math.exp(-x2 / 2.0)) <= 1e-12 * math.exp(-x2 / 2.0) + 1e-300
    # dof 4: Q(2, y) = exp(-y) (1 + y)
    for y in (0.1, 3.0, 40.0, 300.0):
        assert abs(X.upper_gamma_q(2.0, y) - math.exp(-y) * (1.0 + y)) <= 1e-11 * math.exp(-y) * (1.0 + y)
    # states below MIN_EXPECTED share one bin; its mass is reported
    q = np.array([0.5, 0.4, 0.0993, 0.0004, 0.0002, 0.0001])
    bins, nb, pooled = X.pool_bins(10000 * q)
    assert nb == 4 and bins.tolist() == [0, 1, 2, 3, 3, 3] and abs(pooled - 0.0007) < 1e-12
    t = X.chi2_test([5000, 4000, 993, 4, 2, 1], q)
    assert t.dof == 3 and t.x2 == 0.0 and t.p == 1.0
    # nothing to pool: every state a bin of its own
    assert X.pool_bins([8.0, 9.0, 100.0])[1:] == (3, 0.0)
    # a toy past the cap is reported as such (the GPU tests assert the cap)
    assert X.pool_bins(100 * np.array([0.9, 0.05, 0.05]))[2] > X.POOL_CAP
    # a count where the target has no mass rejects outright
    assert X.chi2_test([10, 10, 1], np.array([0.5, 0.5, 0.0])).p == 0.0


_STATES = {"single": 64, "single_wide": 64, "multi_step": 128, "ps": 81, "fp64": 64, "block_prior": 256, "temper": 64,
           "hypo": 324, "nuis": 1225, "joint": 504, "single_l1": 64, "hypo_l1": 324, "lang": 25, "de": 64, "vor": 66}


@pytest.mark.parametrize("name", X.CASES)
def test_enumerated_toys(name):
    cs = X.case(name)
    assert cs.toy.nstates == _STATES[name]
    nt = len(cs.betas) if cs.betas is not None else 1
    assert cs.N % nt == 0 and cs.N // nt >= X.N_FLOOR
    assert cs.K_first <= cs.K <= 4 * cs.K_first and 0 < cs.K_inv <= cs.K_first
    for r, pi in enumerate(X.rung_targets(cs)):
        pr = X.properties(pi, cs.N // nt)
        print(f"{name} rung {r}: states {pr.states} pooled {pr.pooled:.2e} effective {pr.effective:.1f} "
              f"max/min {pr.ratio:.3g}")
        assert abs(pi.sum() - 1.0) < 1e-12 and (pi > 0).all()
        assert pr.pooled <= X.POOL_CAP
        assert pr.effective >= 0.25 * pr.states
        if r == 0:
            assert 10.0 <= pr.ratio <= 1e12
        # the controls are other distributions than the target, on the same states
        for cname, q in X.controls(cs, r).items():
            assert q.shape == pi.shape and abs(q.sum() - 1.0) < 1e-9, cname
            assert np.abs(q - pi).max() > 1e-4, cname


def test_fp64_target_differs_from_fp32():
    a, b = X.case("single").toy.target(), X.case("fp64").toy.target()
    assert a.shape == b.shape and 0 < np.abs(a - b).max() < 1e-2


def test_state_index_round_trip():
    for name in ("ps", "hypo", "nuis", "joint"):
        toy = X.case(name).toy
        idx = np.random.default_rng(3).integers(0, toy.nstates, 200)
        v, xyz, kn, kc = toy.states(idx)
        assert (toy.index(v, xyz if toy.hyp is not None else None,
                          *((kn, kc) if toy.nuis is not None else (None, None))) == idx).all()
    toy = X.case("vor").toy
    idx = np.arange(toy.nstates)
    c, w, k = toy.nuclei(idx)
    assert (toy.index(c, w, k) == idx).all()
    assert (toy.index(c[:, :, ::-1][k[:, 0] == 2], w[:, :, ::-1][k[:, 0] == 2], k[k[:, 0] == 2])
            == idx[k[:, 0] == 2]).all()               # a state is a set: the order of the nuclei does not enter


def test_plumbing_with_the_oracle_chains():
    """The harness on the oracle's own single-cell chains (case 1, 2048 chains, 32
    steps, starts drawn from pi): only p >= 1e-6 is asked -- the power needs the
    GPU tests' N."""
    cs = X.case("single")
    toy, p = cs.toy, cs.toy.p
    pi = toy.target()
    n = 2048
    idx = X.draw_states(pi, n, 7)
    v0 = toy.states(idx)[0]
    P = O.make_problem(p)
    logl0 = toy.data.ravel()[idx]
    v, logl, acc, _ = O.mcmc_run(P, v0, logl0, 0, 0, 32)
    fin = toy.index(v)
    assert (toy.data.ravel()[fin] == logl).all()        # the enumerated logL is the chains' own, bit for bit
    assert acc.any() and (fin != idx).any()
    t = X.chi2_test(np.bincount(fin, minlength=toy.nstates), pi)
    print(f"oracle chains: X2 {t.x2:.1f} dof {t.dof} p {t.p:.3e} pooled {t.pooled:.2e}")
    assert t.p >= X.P_PASS
