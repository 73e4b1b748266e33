"""bench.py on the GPU: --dump-outputs writes what the timed path computed and
writes the same arrays on every run; a plain run prints the headline only and
--full adds the CPU baseline and the fp64 record.

The command-line cases run C2's geometry with 8 chains (64^3, 16 stations):
the smallest workload bench.py's own options reach.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"v": np.float32, "posterior": np.float32, "chains": np.float64, "logl": np.float64, "naccept": np.float64,
         "ttab": np.float32, "niter": np.float32, "accept": np.float32}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    for n, a in out.items():
        assert a.dtype == NAMES[n], n
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def _steps_and_dump(out_dir, nchains=4, nsteps=3):
    """bench.py's timed path at 24^3: nsteps steps (keepK = nsteps keeps the
    first one's state), the kept states copied to `post` on the device, then
    dump_outputs."""
    import bench
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", n=24, nstat=3, nev=4, picks="analytic")
    mcmc.bench_picks(p, 5e-4, 0)
    p.nburn, p.keepk = 0, nsteps
    smp = mcmc.Sampler(p, nchains=nchains, max_samples=1)
    post = torch.empty((nchains, p.ncell), dtype=torch.int32, device="cuda:0")
    smp.run(1)
    first = smp.state()[0]
    smp.run(nsteps - 1)
    assert smp.samples(max_states=1, device_ptr=post.data_ptr()) == 1
    torch.cuda.synchronize()
    bench.dump_outputs(str(out_dir), post, smp)
    state = smp.state()
    last = smp.last()
    smp.close()
    return p, first, state, last


def test_dump_outputs_are_the_last_steps_arrays_and_repeat(tmp_path):
    _dev()
    p, first, (v, logl, nacc, step), (ttab, niter, acc) = _steps_and_dump(tmp_path / "a")
    a = _load(tmp_path / "a")
    assert step == 3
    assert np.array_equal(a["chains"], np.arange(4))
    assert np.array_equal(a["v"], v.astype(np.float32))
    assert np.array_equal(a["posterior"], first.astype(np.float32))
    assert not np.array_equal(v, first)                               # later steps were accepted
    assert np.array_equal(a["logl"], logl) and np.array_equal(a["naccept"], nacc)
    assert a["ttab"].shape == (4, p.nstat, p.nevents) and np.array_equal(a["ttab"], ttab)
    assert np.array_equal(a["niter"], niter) and np.array_equal(a["accept"], acc)
    assert np.all(np.isfinite(a["ttab"])) and np.all(a["ttab"] > 0)
    _steps_and_dump(tmp_path / "b")
    b = _load(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2", "--chains", "8",
                        "--steps", "3", "--warmup", "1"] + args, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(tmp_path):
    _dev()
    line = _bench(["--dump-outputs", str(tmp_path / "o")])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "proposals/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(8 * 1e3 / line["ms_per_step"], rel=1e-2)
    assert line["cpu_baseline"] is None and "f64" not in line and "speedup_vs_cpu" not in line
    assert line["roofline"]["kernel"]
    o = _load(tmp_path / "o")
    assert o["v"].shape == o["posterior"].shape == (8, 16 ** 3) and o["ttab"].shape == (8, 16, 16)
    assert o["logl"].shape == (8,) and np.all(np.isfinite(o["logl"]))


def test_full_run_adds_the_cpu_baseline_and_the_f64_record():
    _dev()
    line = _bench(["--full", "--cpu-cores", "2", "--cpu-rounds", "1", "--f64-steps", "1", "--f64-warmup", "0"])
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] == 2
    assert line["speedup_vs_cpu"] > 0
    assert line["f64"]["dtype"] == "f64" and line["f64"]["steps"] == 1 and line["f64"]["value"] > 0
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
