"""The kept-state hook (csrc/sampler.hip kept_queue / kept_counted) where the
cold-chain boundary falls inside a pipe, for six of its seven consumers at
once: the four accumulators of csrc/kept.h (posterior, covariances, batch
means, data fit) and the hypocentre and nuisance moments (the seventh, the
Voronoi moments, has tests/test_gpu_vor.py).

9 chains on the three-rung ladder: the cold chains are 0-2.  Two pipes split
the chains 4 + 5, so pipe 0 holds chains 0-3, of which only 0-2 are cold, and
pipe 1 holds none.  Every accumulator is an exact integer sum, so the run must
equal the one-pipe run byte for byte, and the hot chains' rows stay zero."""
import numpy as np
import pytest

import test_gpu_hypo as TH
import test_gpu_nuis as TN
import test_gpu_posterior as TP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NCH, G, NSTEPS = 9, 3, 24


def _run(env, monkeypatch):
    from mceik_amd import mcmc
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    p = TP._problem("P", n=24, nburn=2, keepk=2)
    smp = mcmc.Sampler(p, nchains=NCH, max_samples=16)
    try:
        smp.temper_enable(betas=TH.LADDER3, swap_every=2)
        smp.hypo_enable(3, dmax=(1, 1, 1))
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        smp.posterior_enable(per_chain=True, nbins=16)
        probes = [("model", 100), ("hypo", 0, 2), ("static", 0, 1), ("noise", 0)]
        smp.cov_enable(probes, within=True)
        smp.ess_enable(3, probes=probes)
        smp.fit_enable()
        info = smp.info()
        smp.run(NSTEPS)
        return {"info": info, "state": smp.state(), "samples": smp.samples(), "posterior": smp.posterior_raw(),
                "cov": smp.cov_raw(), "ess": smp.ess_raw(), "fit": smp.fit_raw(), "hypo": smp.hypo_moments(), "nuis": smp.nuis_moments()}
    finally:
        smp.close()


def _flat(x):
    """(name, value) of every leaf of a tuple / dict result."""
    items = x.items() if isinstance(x, dict) else enumerate(x)
    return [(k, v) for k, v in items]


def test_cold_boundary_inside_a_pipe(monkeypatch):
    TP._dev()
    one = _run({"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, monkeypatch)
    two = _run({"MCEIK_PIPES": "2"}, monkeypatch)
    assert one["info"]["npipe"] == 1 and two["info"]["npipe"] == 2, (one["info"], two["info"])
    assert two["info"]["chains"] == [4, 5]
    for what in ("state", "samples", "posterior", "cov", "ess", "fit", "hypo", "nuis"):
        for (k, a), (k2, b) in zip(_flat(one[what]), _flat(two[what])):
            assert k == k2
            if isinstance(a, np.ndarray):
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)
            else:
                assert a == b, (what, k)
    nkept = len(two["samples"][0])
    assert nkept == 11                           # kept steps 2, 4, ..., 22
    for r in (one, two):
        assert r["posterior"]["n"] == r["cov"]["n"] == r["ess"]["n"] == r["fit"]["n"] == nkept
        for rows in (r["posterior"]["sum"], r["cov"]["Sc"], r["ess"]["Sc"]):
            assert rows.shape[0] == NCH and not rows[G:].any() and rows[:G].any(1).all()
        assert r["hypo"]["n"] == G * nkept and r["nuis"]["n"] == G * nkept
