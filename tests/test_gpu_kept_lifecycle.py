"""The lifecycle of the four accumulators of kept states (csrc/kept.h, DESIGN.md
s.25; the shared host code in csrc/sampler_api.hip and Sampler._kept_*):
covariances, batch means and data fit keep their sums over a disable, resume
with the same options, refuse other options while they hold states and start
over after a clear; the posterior starts over at every enable and is dropped
by its disable; a mismatching posterior in a checkpoint is refused before the
chains are restored; and the likelihood's norm cannot change under an enabled
accumulator that holds states.

24^3 nodes, 4 stations, 6 events, 4 chains, no burn-in, keepK 1: every step
is a kept step, runs of 6 steps."""
import numpy as np
import pytest

import test_gpu_posterior as TP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NCH, R = 4, 6
# the options a stream is enabled with, and other ones
OPTS = {"posterior": (dict(per_chain=True, nbins=8), dict(per_chain=False, nbins=4)),
        "cov": (dict(probes=[("model", 100), ("model", 7)], within=True), dict(probes=[("model", 101)], within=False)),
        "ess": (dict(nlevels=3), dict(nlevels=2, probes=[("model", 5)])),
        "fit": (dict(), dict(nbins=32, zmax=512.0))}
SUMS = ("cov", "ess", "fit")


class _Stream:
    """Sampler.<name>_* by their last word."""

    def __init__(self, smp, name):
        for what in ("enable", "disable", "accumulate", "raw", "partials") + (("clear",) if name in SUMS else ()):
            setattr(self, what, getattr(smp, f"{name}_{what}"))


def _sampler():
    from mceik_amd import mcmc
    TP._dev()
    return mcmc.Sampler(TP._problem("P", n=24, nburn=0, keepk=1), nchains=NCH)


def _arrays(raw):
    return {k: v for k, v in raw.items() if isinstance(v, np.ndarray) and k != "t0_ref"}


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _assert_empty(raw, what):
    assert raw["n"] == 0 and _arrays(raw), what
    for k, v in _arrays(raw).items():
        assert not v.any(), (what, k)


@pytest.mark.parametrize("name", SUMS)
def test_sums_over_disable_enable_clear(name):
    opts, other = OPTS[name]
    smp = _sampler()
    try:
        s = _Stream(smp, name)
        s.enable(**opts)
        smp.run(R)
        first = s.raw()
        assert first["n"] == R and any(v.any() for v in _arrays(first).values())
        # disabled: the sums stay as they are, and nothing can be added by hand
        s.disable()
        with pytest.raises(RuntimeError):
            s.accumulate()
        smp.run(R)
        _assert_same(first, s.raw(), "after a disabled run")
        # the same options resume the count
        s.enable(**opts)
        smp.run(R)
        held = s.raw()
        assert held["n"] == first["n"] + R
        # other options are refused while states are held, and nothing changes
        with pytest.raises(ValueError):
            s.enable(**other)
        _assert_same(held, s.raw(), "after a refused enable")
        assert s.partials().nkept == held["n"]
        # cleared: nothing to read; then other options start from zero
        s.clear()
        with pytest.raises(RuntimeError):
            s.raw()
        s.enable(**other)
        _assert_empty(s.raw(), "after clear and enable")
        smp.run(R)
        assert s.raw()["n"] == R
    finally:
        smp.close()


def test_posterior_resets_and_drops():
    opts, other = OPTS["posterior"]
    smp = _sampler()
    try:
        smp.posterior_enable(**opts)
        smp.run(R)
        raw = smp.posterior_raw()
        assert raw["n"] == R and raw["sum"].any() and raw["hist"].any()
        smp.posterior_enable(**opts)                 # the same options: from zero
        _assert_empty(smp.posterior_raw(), "enabled again")
        smp.run(R)
        assert smp.posterior_raw()["n"] == R
        smp.posterior_enable(**other)                # other options: new arrays, from zero
        raw = smp.posterior_raw()
        _assert_empty(raw, "enabled with other options")
        assert raw["sum"].shape == smp.model_shape[1:] and raw["hist"].shape[-1] == other["nbins"]
        smp.posterior_disable()
        with pytest.raises(RuntimeError):
            smp.posterior_raw()
        with pytest.raises(RuntimeError):
            smp.posterior_accumulate()
    finally:
        smp.close()


def test_posterior_mismatch_refused_before_the_restore():
    opts, other = OPTS["posterior"]
    smp = _sampler()
    try:
        smp.posterior_enable(**opts)
        smp.run(R)
        ck = smp.checkpoint()
        smp.run(R)
        smp.posterior_enable(**other)
        smp.run(R)
        before, praw = smp.state(), smp.posterior_raw()
        assert before[3] == 3 * R and not np.array_equal(before[0], ck["v"])
        with pytest.raises(ValueError):
            smp.restore(ck)
        after = smp.state()
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
        _assert_same(praw, smp.posterior_raw(), "after a refused restore")
        smp.posterior_enable(**opts)                 # with the checkpoint's options it restores
        smp.restore(ck)
        assert smp.state()[3] == R and smp.posterior_raw()["n"] == R
    finally:
        smp.close()


@pytest.mark.parametrize("name", ("posterior",) + SUMS)
def test_likelihood_refused_while_holding_states(name):
    smp = _sampler()
    try:
        s = _Stream(smp, name)
        s.enable(**OPTS[name][0])
        smp.likelihood_set(1)                        # enabled, no states yet: accepted
        smp.likelihood_set(2)
        smp.run(R)
        with pytest.raises(ValueError):
            smp.likelihood_set(1)
        assert smp.likelihood == 2
        s.disable()                                  # (the posterior is dropped; the others keep their sums, switched off)
        smp.likelihood_set(1)
        assert smp.likelihood == 1
    finally:
        smp.close()
