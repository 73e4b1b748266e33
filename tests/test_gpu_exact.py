"""The GPU sampler's moves against exactly enumerated posteriors (tests/_exact.py,
DESIGN.md s.24).  Every other sampler test compares the kernels with a CPU
restatement of the same rule, which cannot show that the rule samples the target
DESIGN.md states; here mcmc.Sampler -- its real forward solves, step plan and
launch paths -- runs on toy problems whose posterior is enumerated from the
definition of the target alone, and the histogram of the chains' final states is
held against it.

Per case two runs of N chains and K steps: *invariance* (starts drawn from the
exact target: if the step leaves it invariant the final states are N independent
draws of it) and *mixing* (every chain starts in one corner state, and every move
type of the step plan must have accepted something).  Pearson's X^2 must accept
the exact target at p >= 1e-6 and reject every wrong target of the power controls
at p <= 1e-12.  The mixing run's K is four times the smallest K at which the
corner start first passed on an MI355X, less where that would run past about
10 s (the numbers stand at the cases in tests/_exact.py, K_first and K, and in
DESIGN.md s.24's table, with the time, X^2 and p of every case).  Every figure is
printed before it is asserted (pytest -s).
"""
import numpy as np
import pytest

import _exact as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("mode", ["invariance", "mixing"])
@pytest.mark.parametrize("name", X.CASES)
def test_exact_posterior(name, mode, monkeypatch):
    _dev()
    cs = X.case(name)
    X.set_path(cs, monkeypatch)
    counts, stats, wall = X.run_gpu(name, cs, mode)
    print(f"{name} {mode}: {wall:.2f} s for {cs.K_inv if mode == 'invariance' else cs.K} steps of {cs.N} chains; accepts "
          + ", ".join(f"{k} {np.asarray(v).tolist()}" for k, v in stats.items()))
    X.check(name, cs, counts, mode)
    if mode == "mixing":
        assert stats, name
        for move, acc in stats.items():
            assert (np.asarray(acc) > 0).all(), (name, move, acc)
