"""Host-side pieces of the hypocentre moves (include/mceik.h mceik_mcmc_hypo_*,
mceik_eikonal.h mceik_fsm_batch.ev_stride): no GPU needed.

The draw of event e of global chain g at step gs is restated from the oracle's
Philox4x32-10 and det_log:

    r = philox(counter {gs lo, gs hi, 2, e}, key {g, seed})
    d[a] = ((r[a] * (2 dmax[a] + 1)) >> 32) - dmax[a];  log u = det_log((r[3] + 0.5) / 2^32)
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def restated_draw(seed, gid, gs, e, dmax):
    r = [int(x) for x in O.philox([gs & 0xFFFFFFFF, gs >> 32, 2, e], [gid, seed])]
    d = [((r[a] * (2 * dmax[a] + 1)) >> 32) - dmax[a] for a in range(3)]
    return d, O.lib().oracle_det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))


@pytest.mark.parametrize("seed,gid,gs,e,dmax", [
    (2016, 0, 0, 0, (1, 1, 1)),
    (2016, 3, 1, 5, (1, 1, 1)),
    (7, 1023, 11, 31, (2, 3, 4)),
    (7, 5, (1 << 32) + 9, 2, (1, 0, 7)),            # a step past 2^32: the counter's high word
    (0xFFFFFFFF, 0xFFFFFFFF, (1 << 40) - 1, 63, (100, 1, 1000)),
])
def test_draw_equals_the_philox_restatement(seed, gid, gs, e, dmax):
    from mceik_amd import mcmc
    d, logu = mcmc.hypo_draw(seed, gid, gs, e, dmax)
    dr, lr = restated_draw(seed, gid, gs, e, dmax)
    assert d.tolist() == dr
    assert np.float64(logu).tobytes() == np.float64(lr).tobytes()
    assert all(-m <= x <= m for x, m in zip(dr, dmax)) and logu < 0.0


def test_draw_covers_the_whole_range_and_no_more():
    """Over many (chain, step, event) every offset of [-dmax, dmax] turns up on every axis."""
    from mceik_amd import mcmc
    seen = [set(), set(), set()]
    for g in range(8):
        for gs in range(8):
            for e in range(4):
                d, _ = mcmc.hypo_draw(11, g, gs, e, (1, 2, 3))
                for a in range(3):
                    seen[a].add(int(d[a]))
    assert [sorted(s) for s in seen] == [[-1, 0, 1], [-2, -1, 0, 1, 2], [-3, -2, -1, 0, 1, 2, 3]]


def test_dmax_zero_does_not_move():
    from mceik_amd import mcmc
    for g, gs, e in ((0, 0, 0), (4, 9, 3), (77, 12345, 17)):
        d, logu = mcmc.hypo_draw(2016, g, gs, e, (0, 0, 0))
        assert d.tolist() == [0, 0, 0]
        assert logu == restated_draw(2016, g, gs, e, (0, 0, 0))[1]
    d, _ = mcmc.hypo_draw(2016, 1, 2, 3, (0, 5, 0))
    assert d[0] == 0 and d[2] == 0


def test_draw_refuses_bad_arguments():
    from mceik_amd import mcmc
    with pytest.raises(ValueError):
        mcmc.hypo_draw(1, 0, 0, -1, (1, 1, 1))
    with pytest.raises(ValueError):
        mcmc.hypo_draw(1, 0, 0, 0, (1, -1, 1))
    with pytest.raises(ValueError):
        mcmc.hypo_draw(1, 0, 0, 0, (1, 1))


def _offsets_c(header, ctype, fields):
    body = "".join(f'  printf("{f} %zu\\n", offsetof({ctype}, {f}));\n' for f in fields)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\n'
           f'int main(void) {{\n  printf("sizeof %zu\\n", sizeof({ctype}));\n{body}  return 0;\n}}\n')
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "o.c")
        open(p, "w").write(src)
        exe = os.path.join(td, "o")
        subprocess.run(["gcc", "-I", INC, p, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(out[0::2], map(int, out[1::2])))


@pytest.mark.parametrize("header,ctype,pyname", [("mceik.h", "mceik_hypo_opts", "HypoOpts"),
                                                 ("mceik_eikonal.h", "mceik_fsm_batch", "FsmBatch")])
def test_struct_layouts_match_the_headers(header, ctype, pyname):
    from mceik_amd import _lib
    cls = getattr(_lib, pyname)
    names = [f[0] for f in cls._fields_]
    c = _offsets_c(header, ctype, names)
    assert C.sizeof(cls) == c["sizeof"]
    for n in names:
        assert getattr(cls, n).offset == c[n], n
    if pyname == "FsmBatch":
        assert names[-1] == "ev_stride" and c["ev_stride"] > c["solve_count"]      # appended: older callers' layout holds
    else:
        assert names == ["every", "dmax", "lo", "hi"] and c["sizeof"] == 40


def _batch(**kw):
    from mceik_amd import _lib
    b = _lib.FsmBatch()
    b.nx, b.ny, b.nz, b.h = 24, 20, 17, 100.0
    b.maxit, b.tol, b.precision = 50, 1e-8, 32
    b.nmodel, b.nstat, b.nsrc = 3, 2, 1
    b.slow_mode, b.nrx, b.nry, b.nrz = 1, 4, 4, 4
    b.fast_sqrt, b.max_sweeps, b.nev = 1, -1, 5
    for k, v in kw.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("kw", [dict(), dict(precision=64), dict(step_z=8), dict(nrx=3, nry=3, nrz=3), dict(slow_mode=0)])
def test_check_and_kernel_name_do_not_depend_on_ev_stride(kw):
    """The per-model event lists change which nodes a finished field is read at, nothing
    about the launch: same geometry check, kernel instance, LDS and step size."""
    from mceik_amd import _lib
    L = _lib.lib()
    ref = None
    for stride in (0, 5, 10, 1 << 20):
        b = _batch(ev_stride=stride, **kw)
        got = (L.mceik_fsm_check(C.byref(b)), L.mceik_fsm_kernel_name(C.byref(b)), L.mceik_fsm_lds_bytes(C.byref(b)),
               L.mceik_fsm_step_z(C.byref(b)))
        assert got[0] == 0 and got[1]
        ref = ref or got
        assert got == ref, (stride, got, ref)
