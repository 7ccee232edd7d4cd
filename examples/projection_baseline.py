"""The PP baseline (project always) next to RAYEN on one small set: train a two-layer network whose output is forced
into the set, once through ``ProjectionModule(mode='PP')`` and once through ``ConstraintModule(method='RAYEN')``.

    python examples/projection_baseline.py            # on 'cuda' when there is one, else on the host
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import constraint_module, projection, workloads       # noqa: E402


def main():
    device = "cuda" if torch.cuda.is_available() else "cpu"
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(8, 12, 1, 1, seed=2))
    torch.manual_seed(0)
    x = torch.randn(256, 5, device=device)
    target = 0.5 * torch.randn(256, cs.k, device=device)
    for name, head in (("PP", projection.ProjectionModule(cs, input_dim=16, mode='PP')),
                       ("RAYEN", constraint_module.ConstraintModule(cs, input_dim=16, method='RAYEN'))):
        net = torch.nn.Sequential(torch.nn.Linear(5, 16), torch.nn.ReLU(), head).to(device)
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        for step in range(60):
            opt.zero_grad()
            loss = ((net(x)[:, :, 0] - target) ** 2).mean()
            loss.backward()
            opt.step()
        y = net(x)[:, :, 0].detach().double().cpu().numpy()
        print(f"{name:6s} loss {float(loss.detach()):.4f}   worst residual {float(np.max(cs.getViolationRows(y))):+.2e}")


if __name__ == "__main__":
    main()
