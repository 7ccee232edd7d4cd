"""Writes tests/golden/proj_tile/<name>.npz for the cases of tests/proj_tile_cases.py: the seeded inputs, the fp64
reference of tests/proj_reference.py (``conic.solve`` per row, KKT Jacobian) and the fp32 host mirror's run.  25 to 70 s a
case.  Run from the repository root:  python tests/golden/proj_tile/make_fixtures.py [name ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import proj_reference as pr                                  # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402


def main(names):
    for name in names:
        ref = pr.reference.__wrapped__(name) if hasattr(pr.reference, "__wrapped__") else pr.reference(name)
        run = pr.mirror_run(name, "float32")
        prog = pr.module_for(name).program
        print(f"{name}: program (n, m, cones) = {(prog.n, prog.m, len(prog.soc_rows))}, rho {prog.rho}, "
              f"kink rows {int(np.count_nonzero(ref.kink))}, mirror iters {int(run.iters.max())} / {run.iters.mean():.0f}")
        ptc.save_fixture(ptc.fixture_path(name), ref, {"float32": run})


if __name__ == "__main__":
    main(sys.argv[1:] or ptc.NAMES)
