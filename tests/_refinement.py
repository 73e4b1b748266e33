"""The inversion-cell refinements the suite pins beside nref = (4, 4, 4):
which sweep-kernel instance serves each (tests/test_fsm_instances.py, host
only) and that the instance computes the twin's tables bit for bit
(tests/test_gpu_refinement.py).

A case is (id, (nx, ny, nz), nref, precision, fast_sqrt, step_z, kernel name).
The names are mceik_fsm_kernel_name's; step_z = 8 forces the 8-z kernel where
the launch would pick the 16-z one.  Cells per z-block (ccb) in the comments
are fill_launch's sizing; MCEIK_CC_MAX = 256 is the cell cache's capacity.
"""

F32 = "fsm_solve_kernel<float, %s>"
F64 = "fsm_solve_kernel<double, %s>"
UNCACHED32, UNCACHED64 = F32 % "1, false, -1, 1, 0", F64 % "1, false, -1, 1, 0"
GEN32, GEN32_EXACT = F32 % "2, true, -1, 4, 0", F32 % "2, false, -1, 4, 0"
GEN64 = F64 % "2, false, -1, 4, 0"
Z4_RT32, Z4_RT64 = F32 % "2, true, 2, 1, 0", F64 % "2, false, 2, 1, 0"
Z4_KB32 = F32 % "2, true, 2, 1, 4"
Z4_KB64, Z4_KB64_EXACT = F64 % "2, true, 2, 1, 4", F64 % "2, false, 2, 1, 4"
FSM16_FT, FSM16_1, FSM16_4 = ("fsm16_solve_kernel<2, 1>", "fsm16_solve_kernel<0, 1>", "fsm16_solve_kernel<0, 4>")

# every slow_mode 1 name of fsm_launch_name (fsm_kernel.hip)
CELL_MODE_NAMES = {UNCACHED32, UNCACHED64, GEN32, GEN32_EXACT, GEN64, Z4_RT32, Z4_RT64, Z4_KB32, Z4_KB64,
                   Z4_KB64_EXACT, FSM16_FT, FSM16_1, FSM16_4}

G = (30, 26, 34)
_ROWS = [
    # (row id, geometry, nref, [(precision, fast_sqrt, step_z, name)...])
    # ccb 2048: the library default, uncached (load_f's multiply per lane)
    ("n1", G, (1, 1, 1), [(32, True, 0, UNCACHED32), (32, False, 0, UNCACHED32),
                          (64, True, 0, UNCACHED64), (64, False, 0, UNCACHED64)]),
    # ccb 512: the first geometry past MCEIK_CC_MAX
    ("n221", G, (2, 2, 1), [(32, True, 0, UNCACHED32), (64, True, 0, UNCACHED64)]),
    # ccb 256: exactly MCEIK_CC_MAX, four cache registers per lane all used
    ("n2", G, (2, 2, 2), [(32, True, 0, GEN32), (64, True, 0, GEN64)]),
    # ccb 176 = 4 x 4 x 11 cells (a tile's 8 nodes touch 3 or 4 cells, the first z-block's 32 nodes 11)
    ("n3", G, (3, 3, 3), [(32, True, 0, GEN32), (32, False, 0, GEN32_EXACT),
                          (64, True, 0, GEN64), (64, False, 0, GEN64)]),
    # ccb 66: anisotropic, all three odd
    ("n573", G, (5, 7, 3), [(32, True, 0, GEN32), (64, True, 0, GEN64)]),
    # kb 3 (nz = 20), ccb 60: the runtime-kb nrz = 4 instances
    ("n534_kb3", (30, 26, 20), (5, 3, 4), [(32, True, 0, Z4_RT32), (64, True, 0, Z4_RT64)]),
    # ccb 32: 2 x 2 x 8 cells as at nref 4, but cells straddle tile edges
    ("n664", G, (6, 6, 4), [(32, True, 0, FSM16_FT), (32, True, 8, Z4_KB32),
                            (64, True, 0, Z4_KB64), (64, False, 0, Z4_KB64_EXACT)]),
    # ccb 8: a cell spans two tiles; ragged last z-block
    ("n16_16_4", (30, 26, 67), (16, 16, 4), [(32, True, 0, FSM16_FT)]),
    # ccb 64: past the fixed layout's 32, one cache register
    ("n344", G, (3, 4, 4), [(32, True, 0, FSM16_1)]),
    # ccb 96: two cache registers (of the instance's four)
    ("n534", G, (5, 3, 4), [(32, True, 0, FSM16_4), (32, True, 8, GEN32)]),
    # one cell for the whole grid
    ("n40", G, (40, 40, 40), [(32, True, 0, GEN32)]),
]

CASES = [("%s-f%d%s%s" % (rid, prec, "" if fast else "-exact", "-z8" if step_z else ""),
          geo, nref, prec, fast, step_z, name)
         for rid, geo, nref, cells in _ROWS for prec, fast, step_z, name in cells]
CASE_IDS = [c[0] for c in CASES]
