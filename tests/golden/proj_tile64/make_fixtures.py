"""Writes tests/golden/proj_tile64/<name>.npz for the cases of tests/proj_tile64_cases.py: the fp64 host mirror's run
(``z``, ``grad_q``, ``iters`` at eps = 1e-9, 2048 iterations at most) on the seeded batch whose inputs and fp64 reference the
fixtures of tests/golden/proj_tile and tests/golden/proj_sweep already hold.  Up to 50 s a case.  Run from the repository
root:  python tests/golden/proj_tile64/make_fixtures.py [name ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import proj_reference as pr                                  # noqa: E402
import proj_sweep_cases as psc                               # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402
import proj_tile64_cases as p64                              # noqa: E402


def main(names):
    for name in names:
        if name in psc.BY_NAME:
            psc.install(name)
        else:
            ptc.install(name)
        ref = pr.reference(name)
        run = pr.mirror_run(name, p64.F64, B=p64.rows_of(name))
        ok = ~ref.kink
        prog = pr.module_for(name).program
        print(f"{name}: program (n, m, cones) = {(prog.n, prog.m, len(prog.soc_rows))}, rho {prog.rho}, kink rows "
              f"{int(np.count_nonzero(ref.kink))}, fp64 mirror fwd {pr.row_gap(run.z, ref.z).max():.1e} bwd "
              f"{pr.row_gap(run.grad_q, ref.grad_q)[ok].max():.1e} iters {int(run.iters.max())} / {run.iters.mean():.0f}")
        np.savez_compressed(p64.fixture_path(name), mirror64_z=run.z, mirror64_grad_q=run.grad_q, mirror64_iters=run.iters)


if __name__ == "__main__":
    main(sys.argv[1:] or p64.RECORDED)
