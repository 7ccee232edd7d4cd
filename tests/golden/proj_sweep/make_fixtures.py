"""Writes tests/golden/proj_sweep/<name>.npz for the cases of tests/proj_sweep_cases.py: the seeded inputs (97 rows), the
fp64 reference of tests/proj_reference.py (``conic.solve`` per row, KKT Jacobian) and the host mirror's runs in fp32 and,
where the wave kernel serves the case, fp64; and for r32_k4 of tests/proj_lmi_reference.py that module's reference and fp64
mirror.  10 to 60 s a case.  Run from the repository root:
python tests/golden/proj_sweep/make_fixtures.py [name ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import proj_lmi_reference as plr                             # noqa: E402
import proj_reference as pr                                  # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402
import proj_sweep_cases as sw                                # noqa: E402


def lmi(name):
    """The LMI case of the stride test: proj_lmi_reference's own reference and fp64 mirror."""
    ref = getattr(plr.reference, "inner", plr.reference)(name)
    run = getattr(plr.mirror_run, "inner", plr.mirror_run)(name, sw.F64)
    print(f"{name}: kink rows {int(np.count_nonzero(ref.kink))}, fp64 mirror iters {int(run.iters.max())}", flush=True)
    ptc.save_fixture(sw.fixture_path(name), ref, {sw.F64: run}, nullity=ref.nullity)


def main(names):
    for name in names:
        if name == sw.LMI_STRIDE:
            lmi(name)
            continue
        ref = pr.reference(name, B=sw.BATCH)
        runs = {dtype_name: pr.mirror_run(name, dtype_name, B=sw.BATCH) for dtype_name in sw.dtype_names(name)}
        prog = pr.module_for(name).program
        ok = ~ref.kink
        print(f"{name}: program (n, m, cones) = {(prog.n, prog.m, len(prog.soc_rows))}, rho {prog.rho}, "
              f"kink rows {int(np.count_nonzero(ref.kink))}, interior {int(np.count_nonzero(ref.interior))}; " + "; ".join(
                  f"{d} fwd {pr.row_gap(r.z, ref.z).max():.1e} bwd {pr.row_gap(r.grad_q, ref.grad_q)[ok].max():.1e} "
                  f"iters {int(r.iters.max())} / {r.iters.mean():.0f}" for d, r in runs.items()), flush=True)
        ptc.save_fixture(sw.fixture_path(name), ref, runs)


if __name__ == "__main__":
    main(sys.argv[1:] or sw.NAMES + [sw.LMI_STRIDE])
