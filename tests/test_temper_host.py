"""Parallel tempering, host side (no GPU): the geometric ladder
(mceik_temper_ladder) and the cold chains' global ids under mcmc.shard."""
import ctypes as C

import numpy as np
import pytest


def _ladder(ntemps, tmax, n=None):
    from mceik_amd import _lib
    beta = np.full(n if n is not None else max(ntemps, 1), -7.0)
    rc = _lib.lib().mceik_temper_ladder(ntemps, tmax, beta.ctypes.data_as(C.c_void_p))
    return rc, beta


@pytest.mark.parametrize("ntemps,tmax", [(2, 2.0), (4, 50.0), (8, 1000.0), (5, 3.7), (16, 1e6)])
def test_ladder(ntemps, tmax):
    rc, beta = _ladder(ntemps, tmax)
    assert rc == 0
    assert beta[0] == 1.0
    assert (np.diff(beta) < 0.0).all() and (beta > 0.0).all()
    last = 1.0 / tmax
    assert abs(beta[-1] - last) <= np.spacing(last)
    # geometric: constant ratio between neighbours, to rounding
    ratio = beta[1:] / beta[:-1]
    assert np.allclose(ratio, tmax ** (-1.0 / (ntemps - 1)), rtol=1e-14, atol=0.0)


def test_ladder_one_rung_and_flat():
    rc, beta = _ladder(1, 50.0)
    assert rc == 0 and beta[0] == 1.0
    rc, beta = _ladder(3, 1.0)
    assert rc == 0 and (beta == 1.0).all()


@pytest.mark.parametrize("ntemps,tmax", [(0, 10.0), (-1, 10.0), (4, 0.5), (4, 0.0), (4, -3.0), (4, float("nan")),
                                         (4, float("inf"))])
def test_ladder_bad_arguments(ntemps, tmax):
    rc, beta = _ladder(ntemps, tmax, n=4)
    assert rc == 1 and (beta == -7.0).all()


def test_ladder_null():
    from mceik_amd import _lib, mcmc
    assert _lib.lib().mceik_temper_ladder(4, 10.0, None) == 1
    assert mcmc.temper_ladder(4, 10.0).tobytes() == _ladder(4, 10.0)[1].tobytes()
    with pytest.raises(ValueError):
        mcmc.temper_ladder(4, 0.5)


def test_cold_chain_ids():
    from mceik_amd import mcmc
    # one rank: 12 chains, 4 rungs -> G = 3
    assert mcmc.cold_chain_ids(12, 1, 4).tolist() == [0, 1, 2]
    # two ranks of 12: shards [0, 12), [12, 24); 3 rungs -> G = 4 each
    assert mcmc.cold_chain_ids(24, 2, 3).tolist() == [0, 1, 2, 3, 12, 13, 14, 15]
    # three ranks of 6: shards [0, 6), [6, 12), [12, 18); 3 rungs -> G = 2 each
    assert [mcmc.shard(18, r, 3) for r in range(3)] == [(0, 6), (6, 12), (12, 18)]
    assert mcmc.cold_chain_ids(18, 3, 3).tolist() == [0, 1, 6, 7, 12, 13]
    # one rung: every chain is cold, also under an uneven split
    assert mcmc.cold_chain_ids(7, 3, 1).tolist() == list(range(7))
    assert mcmc.cold_chain_ids(18, 3, 3).dtype == np.int64
    # shards that do not hold whole groups: 20 over 3 ranks is 7, 7, 6
    assert [mcmc.shard(20, r, 3) for r in range(3)] == [(0, 7), (7, 14), (14, 20)]
    with pytest.raises(ValueError):
        mcmc.cold_chain_ids(20, 3, 2)
