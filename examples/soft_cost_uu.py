#!/usr/bin/env python
"""The reference's unconstrained baseline (method='UU') trained with the soft cost as its penalty, on an MI355X: the network's
output is NOT projected, the loss adds weight * sum relu(g)^2 over the set's constraints -- with ``fused=True`` loss and
gradient of that term are one launch of rayen_cost.hip (rayen_amd/soft_cost.py) instead of a chain of torch ops.

    python examples/soft_cost_uu.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import constraint_module, workloads  # noqa: E402
from rayen_amd.cost_computer import CostComputer  # noqa: E402
from rayen_amd.soft_cost import SoftCost  # noqa: E402


def main():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=16, m=24, n_quad=2, n_soc=2, seed=0))
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.ReLU(),
                                constraint_module.ConstraintModule(cs, input_dim=64, method='UU', create_map=True)).cuda()
    cost = CostComputer(cs, fused=True).cuda()
    judge = SoftCost(cs).cuda()
    x = torch.randn(4096, 4, device="cuda")
    target = torch.full((1, cs.k, 1), 0.4, device="cuda")          # outside the set
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    for step in range(300):
        opt.zero_grad()
        y = model(x)
        loss = ((y - target) ** 2).sum() + 100.0 * cost.getSumSoftCostAllSamples(y)
        loss.backward()
        opt.step()
        if step % 100 == 0 or step == 299:
            worst, which = judge.violation(y.detach())
            print(f"step {step:3d}  loss/row {loss.item() / len(x):.5f}  worst violation {worst.max().item():.3e} "
                  f"(constraint {int(which[worst.argmax()])}), rows inside {(worst <= 0).float().mean().item():.1%}")


if __name__ == "__main__":
    main()
