"""``ProjectionModule``: the reference's ``PP`` (project always) and ``UP`` (project at test time only) baselines
(rayen/constraint_module.py:76-96 and :488-504) as a module of their own, on a batched Euclidean projection.

The core is ``Pi(q) = argmin ||z - q||^2`` subject to ``A_p z <= b_p`` and the quadratics and cones evaluated at
``y = NA_E z + yp`` -- the reference's program, which it hands to cvxpylayers + ECOS one sample at a time.  Here it is the
operator-splitting iteration of ``rayen_amd/conic.py`` specialised to ``P = 2I, c = -2q``: the cone rows ``G z + h in K``
(slack of ``A_p`` as orthant rows, every quadratic and SOC as a second-order cone, the LMI as a PSD block) are the same for
the whole batch, so
the rows are assembled and equilibrated, ``rho`` is chosen and ``K^-1 = ((2 + sigma) I + rho G'G)^-1`` is formed ONCE per
set, in fp64 on the host (:func:`build_program`).  With ``v = z_r + y / rho + h`` the splitting variables are
``z = Pi_K(v) - h`` and ``y = rho (v - Pi_K(v))`` (Moreau), so the state of a sample is ``(x, v)`` and one iteration is

    p  = Pi_K(v)
    xt = K^-1 (sigma x + 2 q - rho G'h + rho G'(2 p - v))
    r  = G xt + h - p
    x <- x + alpha (xt - x),     v <- v + alpha r

A sample stops when ``max|r| <= eps (1 + max|p|)`` and ``max|xt - x| <= eps (1 + max|xt|)`` (both vanish exactly at the
fixed point, where ``(xt, p, y)`` satisfies the KKT conditions of the program) and returns ``xt``; the stop is PER ROW.  A
row with ``G q + h in K`` takes 0 iterations and returns ``q``; a row that reaches ``max_iters`` reports
``iters == max_iters`` and is not an error.

The backward is implicit: the Jacobian of a Euclidean projection is symmetric, so ``grad_q = J g``, and ``J g`` is the fixed
point of the LINEARISED iteration -- every ``Pi_K`` replaced by its derivative at the saved ``v*``, ``h`` dropped, ``2 g`` in
place of ``2 q`` -- run to the same stop rule on ``g`` scaled to unit maximum.

Tensors on a HIP device run ``rayen_amd/csrc/rayen_proj.hip`` through ``rayen_amd::euclid_project``; host tensors, and sets
the kernel does not stage (one ``RuntimeWarning``; an error under ``RAYEN_STRICT_HIP=1``), run the mirror below: the same
iteration in plain torch ops.  It is the eager path, not the test reference (tests/proj_reference.py).

``kernel='tile'`` sends fp32 device tensors to ``rayen_amd/csrc/rayen_proj_tile.hip`` instead (tiles of 32 samples on the
matrix cores: no LDS image, so programs beyond the wave kernel's 576 rows and 32 cones; no fp64, no LMI), ``kernel='auto'``
does so only where the wave kernel refuses the set; what the chosen kernel refuses takes the same loud detour.  The default
``'wave'`` is what every call ran before.

A set with an LMI is served on request (``lmi=True``; the default still raises ``NotImplementedError``).  Its PSD block
comes LAST in ``G z + h in K`` and is stored as svec: ``r (r + 1) / 2`` rows, one per ``(i, j)`` with ``i <= j``, row-major
(``(0,0), (0,1), .., (0,r-1), (1,1), ..``), the off-diagonal rows scaled by ``sqrt(2)``.  The Euclidean norm of the block
is then the Frobenius norm of the matrix and ``Pi_K`` on it is the Euclidean projection onto the PSD cone
(``V max(lambda, 0) V'``); the block is equilibrated by ONE scale, like a second-order cone.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib, conic, utils

SIGMA, ALPHA = 1e-6, 1.6
RHO_CANDIDATES = (0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0)
DEFAULT_MAX_ITERS, DEFAULT_EPS = 512, 1e-6


# ------------------------------------------------------------------------------------------------------------------
# the program of a set (host, fp64, once)
# ------------------------------------------------------------------------------------------------------------------

def svec_index(r):
    """``(i [rows], j [rows], scale [rows])`` of the svec storage of a symmetric ``r x r`` block: ``i <= j``, row-major;
    ``scale`` is 1 on the diagonal and ``sqrt(2)`` off it."""
    i, j = np.triu_indices(r)
    return i, j, np.where(i == j, 1.0, np.sqrt(2.0))


def cone_rows(cs, lmi=False):
    """``(G [m, n], h [m], m_lin, soc_rows, psd_dim)`` of ``G z + h in K``, unscaled: ``m_lin`` orthant rows first (the
    slack of ``A_p``; rows of zeros are dropped), then one second-order cone per quadratic and per SOC (``t`` stored
    last), then, with ``lmi=True``, the LMI's ``psd_dim x psd_dim`` block in svec storage (0: the set has none)."""
    if cs.has_lmi_constraints and not lmi:
        raise NotImplementedError("the Euclidean projection serves linear, quadratic and second-order-cone constraints by "
                                  "default; a set with an LMI needs a PSD projection per iteration and is served on request: "
                                  "pass lmi=True")
    prog = conic.ConeProgram(cs.n)
    keep = np.any(cs.A_p != 0.0, axis=1)
    prog.add(conic.NONNEG, -cs.A_p[keep], cs.b_p[keep, 0])
    m_lin = int(np.count_nonzero(keep))
    cs._nonlinear_cone_rows(prog, cs.NA_E, cs.yp)
    G, h = prog.stacked()
    soc_rows = [rows for kind, rows, _ in prog.cones if kind == conic.SOC]
    psd_dim = 0
    if cs.has_lmi_constraints:                # the rows of cs._nonlinear_cone_rows (full r x r storage) folded to svec
        psd_dim = int(prog.cones[-1][2])
        full = G.shape[0] - psd_dim * psd_dim
        i, j, scale = svec_index(psd_dim)
        fold = lambda a: 0.5 * scale.reshape((-1,) + (1,) * (a.ndim - 1)) * (a[full + i * psd_dim + j] + a[full + j * psd_dim + i])   # noqa: E731
        G, h = np.concatenate((G[:full], fold(G)), axis=0), np.concatenate((h[:full], fold(h)))
    return G, h, m_lin, soc_rows, psd_dim


def _equilibrate(G, h, m_lin, soc_rows, psd_dim=0):
    """One scale per orthant row and per cone block, the PSD block included (``conic.solve``'s rule: a cone stays a
    cone)."""
    scale = np.ones(G.shape[0])
    Gh = np.concatenate((G, h[:, None]), axis=1)
    rn = np.linalg.norm(Gh[:m_lin], axis=1)
    scale[:m_lin] = 1.0 / np.where(rn > 0, rn, 1.0)
    at = m_lin
    for rows in list(soc_rows) + ([psd_dim * (psd_dim + 1) // 2] if psd_dim else []):
        nrm = float(np.linalg.norm(Gh[at:at + rows])) / np.sqrt(rows)
        if nrm > 0:
            scale[at:at + rows] = 1.0 / nrm
        at += rows
    return G * scale[:, None], h * scale


class Program:
    """The per-set constants of the iteration, fp64 numpy (picklable)."""

    def __init__(self, G, h, m_lin, soc_rows, n, rho, psd_dim=0):
        self.G, self.h, self.m_lin, self.soc_rows, self.n = G, h, int(m_lin), [int(r) for r in soc_rows], int(n)
        self.m = int(G.shape[0])
        self.psd_dim = int(psd_dim)              # the PSD block: the last psd_dim (psd_dim + 1) / 2 rows, svec
        self.psd_row0 = self.m - self.psd_dim * (self.psd_dim + 1) // 2
        self.set_rho(rho)

    def set_rho(self, rho):
        self.rho = float(rho)
        K = (2.0 + SIGMA) * np.eye(self.n) + self.rho * (self.G.T @ self.G)
        Kinv = np.linalg.inv(K)
        self.Kinv = 0.5 * (Kinv + Kinv.T)
        self.w0 = -self.rho * (self.G.T @ self.h)

    def arrays(self):
        """What ``ops.ProjPack`` uploads."""
        c = np.ascontiguousarray
        return dict(G=c(self.G), h=c(self.h), Kinv=c(self.Kinv), w0=c(self.w0), m_lin=self.m_lin,
                    soc_rows=np.asarray(self.soc_rows, dtype=np.int32), n=self.n, m=self.m, rho=self.rho,
                    sigma=SIGMA, alpha=ALPHA, psd_row0=self.psd_row0, psd_dim=self.psd_dim)


def probe_points(cs, count=8, seed=0):
    """Seeded points around ``z0`` for the choice of ``rho``: ``z0 + s N(0, I)`` with ``s = 1 + max|z0|``."""
    rng = np.random.default_rng(seed)
    z0 = np.asarray(cs.z0, dtype=np.float64).reshape(1, cs.n)
    return z0 + (1.0 + float(np.max(np.abs(z0)))) * rng.standard_normal((count, cs.n))


def build_program(cs, rho=None, probe_eps=1e-8, probe_iters=2000, lmi=False):
    """Assemble, equilibrate and pick ``rho``: the candidate with the fewest iterations (worst probe row, fp64 mirror at
    ``probe_eps``) wins; ties go to the value nearest 1.  ``rho`` given: taken as is.  ``lmi=True``: a set with an LMI is
    served (its PSD block last, svec); the default raises ``NotImplementedError`` on one."""
    G, h, m_lin, soc_rows, psd_dim = cone_rows(cs, lmi=lmi)
    G, h = _equilibrate(G, h, m_lin, soc_rows, psd_dim)
    prog = Program(G, h, m_lin, soc_rows, cs.n, 1.0 if rho is None else rho, psd_dim)
    if rho is not None:
        return prog
    q0, z0 = probe_points(cs), np.asarray(cs.z0, dtype=np.float64).reshape(1, cs.n)
    for spread in (1.0, 4.0, 16.0, 64.0):
        q = torch.from_numpy(z0 + spread * (q0 - z0))
        best = None
        for cand in RHO_CANDIDATES:
            prog.set_rho(cand)
            _, iters, _ = mirror_forward(Constants(prog, torch.float64, q.device), q, probe_iters, probe_eps)
            key = (int(iters.max()), abs(np.log(cand)))
            if best is None or key < best[0]:
                best = (key, cand)
        # a set with an LMI is often wide around z0 (F_k dominates): probes that all fall inside say nothing about rho,
        # so they are spread further until one leaves (sets without an LMI keep the one round they have always had)
        if best[0][0] > 0 or not psd_dim:
            break
    prog.set_rho(best[1])
    prog.probe_iters = best[0][0]
    return prog


# ------------------------------------------------------------------------------------------------------------------
# the mirror: the same iteration in plain torch ops (host tensors, and the loud detour on a device)
# ------------------------------------------------------------------------------------------------------------------

class Constants:
    """A :class:`Program` as torch tensors of one dtype on one device."""

    def __init__(self, prog, dtype, device):
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype, device=device)          # noqa: E731
        self.G, self.h, self.Kinv, self.w0 = t(prog.G), t(prog.h), t(prog.Kinv), t(prog.w0)
        self.rho, self.m_lin, self.n, self.m = prog.rho, prog.m_lin, prog.n, prog.m
        idx_x, cid_x, idx_t, at = [], [], [], prog.m_lin
        for c, rows in enumerate(prog.soc_rows):
            idx_x += list(range(at, at + rows - 1))
            cid_x += [c] * (rows - 1)
            idx_t.append(at + rows - 1)
            at += rows
        i64 = lambda a: torch.as_tensor(a, dtype=torch.int64, device=device)              # noqa: E731
        self.idx_x, self.cid_x, self.idx_t = i64(idx_x), i64(cid_x), i64(idx_t)
        self.n_soc = len(prog.soc_rows)
        self.psd_dim, self.psd_row0 = getattr(prog, "psd_dim", 0), getattr(prog, "psd_row0", prog.m)
        if self.psd_dim:
            i, j, scale = svec_index(self.psd_dim)
            self.psd_i, self.psd_j, self.psd_scale = i64(i), i64(j), t(scale)


def smat(c, block):
    """``[B, r (r + 1) / 2]`` svec rows -> ``[B, r, r]`` symmetric matrices."""
    M = block.new_zeros(block.shape[0], c.psd_dim, c.psd_dim)
    w = block / c.psd_scale
    M[:, c.psd_i, c.psd_j] = w
    M[:, c.psd_j, c.psd_i] = w
    return M


def svec(c, M):
    return M[:, c.psd_i, c.psd_j] * c.psd_scale


def psd_eig(c, v):
    """``(lambda [B, r] ascending, V [B, r, r], finite [B])`` of the PSD block of ``v``; a row with a NaN or an infinity is
    decomposed as zeros and answers NaN in its own block only."""
    block = v[:, c.psd_row0:]
    finite = torch.isfinite(block).all(dim=1)
    lam, V = torch.linalg.eigh(smat(c, torch.where(finite[:, None], block, torch.zeros_like(block))))
    return lam, V, finite


def _psd_project(c, v):
    """The block of ``Pi_K(v)``: ``svec(V max(lambda, 0) V')``, computed as ``v - svec(V min(lambda, 0) V')`` -- the same
    matrix, but the rounding of the decomposition then multiplies the negative part alone and not ``||A||``: with the sum
    over the positive part the fp32 iteration at ``r >= 20`` jitters about its stop rule (one host took 614 iterations on
    a row of the 32 x 32 test case, another 3759; the kernel ran to ``max_iters``).  A block with every eigenvalue ``>= 0``
    is handed back as it is, bit for bit (an interior row's ``p == v_raw`` rests on it)."""
    lam, V, finite = psd_eig(c, v)
    block = v[:, c.psd_row0:]
    rebuilt = block + svec(c, (V * torch.clamp_min(-lam, 0.0)[:, None, :]) @ V.transpose(1, 2))
    out = torch.where((lam >= 0).all(dim=1)[:, None], block, rebuilt)
    return torch.where(finite[:, None], out, torch.full_like(out, float("nan")))


def _psd_weights(lam):
    """``B_ij`` of ``D Pi(M)[H] = V (B o (V'HV)) V'``: 1 where both eigenvalues are ``> 0``, 0 where both are ``<= 0``,
    ``lambda_+ / (lambda_+ - lambda_-)`` on a mixed pair (an eigenvalue of exactly 0 counts as ``<= 0``)."""
    li, lj = lam[:, :, None], lam[:, None, :]
    pi, pj = li > 0, lj > 0
    hi, lo = torch.maximum(li, lj), torch.minimum(li, lj)
    mixed = hi / torch.where(pi ^ pj, hi - lo, torch.ones_like(hi))
    return torch.where(pi & pj, torch.ones_like(hi), torch.where(pi ^ pj, mixed, torch.zeros_like(hi)))


def _psd_derivative(c, eig, dv):
    lam, V, finite = eig
    T = V.transpose(1, 2) @ smat(c, dv[:, c.psd_row0:]) @ V
    out = svec(c, V @ (_psd_weights(lam) * T) @ V.transpose(1, 2))
    return torch.where(finite[:, None], out, torch.full_like(out, float("nan")))


def _soc_parts(c, v):
    x, t = v[:, c.idx_x], v[:, c.idx_t]
    s = torch.sqrt(torch.zeros_like(t).index_add_(1, c.cid_x, x * x))
    return x, t, s


def cone_project(c, v):
    """``Pi_K(v)`` row by row of the batch."""
    out = torch.clamp_min(v, 0.0)
    if c.n_soc:
        x, t, s = _soc_parts(c, v)
        inside, zero = s <= t, s <= -t
        a = 0.5 * (s + t)
        coef = torch.where(inside, torch.ones_like(s), torch.where(zero, torch.zeros_like(s), a / s))
        out[:, c.idx_x] = x * coef[:, c.cid_x]
        out[:, c.idx_t] = torch.where(inside, t, torch.where(zero, torch.zeros_like(t), a))
    if c.psd_dim:
        out[:, c.psd_row0:] = _psd_project(c, v)
    return out


def cone_derivative(c, v, dv, eig=None):
    """``D Pi_K(v) dv`` (an element of the generalised Jacobian on a kink).  ``eig``: ``psd_eig(c, v)`` when the caller
    has it (the backward decomposes ``v*`` once)."""
    out = torch.where(v > 0, dv, torch.zeros_like(dv))
    if c.n_soc:
        x, t, s = _soc_parts(c, v)
        dx, dt = dv[:, c.idx_x], dv[:, c.idx_t]
        inside, zero = s <= t, s <= -t
        safe = torch.where(s > 0, s, torch.ones_like(s))
        xh = x / safe[:, c.cid_x]
        xd = torch.zeros_like(t).index_add_(1, c.cid_x, xh * dx)
        da = 0.5 * (xd + dt)
        ratio = 0.5 * (s + t) / safe
        mid_x = da[:, c.cid_x] * xh + ratio[:, c.cid_x] * (dx - xh * xd[:, c.cid_x])
        ins_x, zer_x = inside[:, c.cid_x], zero[:, c.cid_x]
        out[:, c.idx_x] = torch.where(ins_x, dx, torch.where(zer_x, torch.zeros_like(dx), mid_x))
        out[:, c.idx_t] = torch.where(inside, dt, torch.where(zero, torch.zeros_like(dt), da))
    if c.psd_dim:
        out[:, c.psd_row0:] = _psd_derivative(c, psd_eig(c, v) if eig is None else eig, dv)
    return out


def _rowmax(t):
    return t.abs().amax(dim=1) if t.shape[1] else t.new_zeros(t.shape[0])


def _iterate(c, rhs2, x, v, done, max_iters, eps, cone_op, h, w0):
    """The shared loop.  ``rhs2`` is ``2 q`` (forward) or ``2 g`` (backward); ``cone_op(v)`` is ``Pi_K`` or its
    derivative.  Returns ``(xt at the stop, v at the stop, iters)``; rows in ``done`` are left as they are."""
    B = x.shape[0]
    out, vstop = x.clone(), v.clone()
    iters = torch.zeros(B, dtype=torch.int32, device=x.device)
    done = done.clone()
    for t in range(1, max_iters + 1):
        if bool(done.all()):
            break
        p = cone_op(v)
        xt = (SIGMA * x + rhs2 + w0 + c.rho * ((2.0 * p - v) @ c.G)) @ c.Kinv
        r = xt @ c.G.T + h - p
        dx = xt - x
        conv = (_rowmax(r) <= eps * (1.0 + _rowmax(p))) & (_rowmax(dx) <= eps * (1.0 + _rowmax(xt)))
        act = ~done
        stop = act & (conv | (t == max_iters))
        out = torch.where(stop[:, None], xt, out)
        vstop = torch.where(stop[:, None], v, vstop)
        iters = torch.where(act, torch.full_like(iters, t), iters)
        go = (act & ~stop)[:, None]
        v = torch.where(go, v + ALPHA * r, v)
        x = torch.where(go, x + ALPHA * dx, x)
        done = done | stop
    return out, vstop, iters


def mirror_forward(c, q, max_iters, eps):
    """``(z [B, n], iters [B] int32, v* [B, m])``."""
    v_raw = q @ c.G.T + c.h
    p = cone_project(c, v_raw)
    interior = (p == v_raw).all(dim=1)
    z, vstop, iters = _iterate(c, 2.0 * q, q, p, interior, int(max_iters), eps, lambda v: cone_project(c, v), c.h, c.w0)
    return (torch.where(interior[:, None], q, z), torch.where(interior, torch.zeros_like(iters), iters),
            torch.where(interior[:, None], v_raw, vstop))


def mirror_backward(c, g, vstar, iters, max_iters, eps):
    """``J g`` row by row: the linearised iteration at ``v*`` (rows with ``iters == 0`` have ``J = I``)."""
    interior = iters == 0
    scale = _rowmax(g)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))[:, None]
    gn = g / scale
    eig = psd_eig(c, vstar) if c.psd_dim else None
    D = lambda dv: cone_derivative(c, vstar, dv, eig)           # noqa: E731
    out, _, _ = _iterate(c, 2.0 * gn, gn, D(gn @ c.G.T), interior, int(max_iters), eps, D, 0.0, 0.0)
    return torch.where(interior[:, None], g, out * scale)


class _MirrorProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, c, max_iters, eps):
        z, iters, vstar = mirror_forward(c, q, max_iters, eps)
        ctx.c, ctx.max_iters, ctx.eps = c, max_iters, eps
        ctx.save_for_backward(vstar, iters)
        ctx.mark_non_differentiable(iters)
        return z, iters

    @staticmethod
    def backward(ctx, grad_z, grad_iters):
        vstar, iters = ctx.saved_tensors
        if grad_z is None:
            return None, None, None, None
        return mirror_backward(ctx.c, grad_z.to(vstar.dtype), vstar, iters, ctx.max_iters, ctx.eps), None, None, None


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------

class ProjectionModule(torch.nn.Module):
    """``mode='PP'``: ``y = NA_E Pi(q) + yp`` in training and eval.  ``mode='UP'``: ``z = q`` while ``self.training``,
    ``Pi(q)`` otherwise (rayen/constraint_module.py:488-504).  Same mapper contract and buffer names as
    ``ConstraintModule``; ``project(q)`` returns ``(z, iters)``.  ``lmi=True`` serves a set with an LMI (the default
    raises ``NotImplementedError`` on one).  ``kernel``: ``'wave'`` (rayen_proj.hip, the default), ``'tile'``
    (rayen_proj_tile.hip on fp32 input, rayen_proj_tile64.hip on fp64 input) or ``'auto'`` (the wave kernel where it serves
    the set at the input's precision, that precision's tile kernel where only it does)."""

    KERNELS = ('wave', 'tile', 'auto')

    def __init__(self, cs, input_dim=None, mode='PP', create_map=True, max_iters=DEFAULT_MAX_ITERS, eps=DEFAULT_EPS,
                 rho=None, lmi=False, kernel='wave'):
        super().__init__()
        if mode not in ('PP', 'UP'):
            raise ValueError(f"mode must be 'PP' or 'UP', got {mode!r}")
        if kernel not in self.KERNELS:
            raise ValueError(f"kernel must be one of {self.KERNELS}, got {kernel!r}")
        self.kernel = kernel
        if isinstance(max_iters, bool) or int(max_iters) != max_iters or int(max_iters) < 1:
            raise ValueError(f"max_iters must be an integer >= 1, got {max_iters!r}")
        if not float(eps) >= 0.0:
            raise ValueError(f"eps must be >= 0, got {eps!r}")
        self.program = build_program(cs, rho=rho, lmi=lmi)          # (raises NotImplementedError on an LMI without lmi=True)
        self.mode, self.max_iters, self.eps = mode, int(max_iters), float(eps)
        self.cs = cs
        self.k, self.n = cs.k, cs.n

        all_P, all_q, all_r = utils.getAllPqrFromQcs(cs.qcs)
        all_M, all_s, all_c, all_d = utils.getAllMscdFromSocs(cs.socs)
        for name, value in (("A_p", cs.A_p), ("b_p", cs.b_p), ("yp", cs.yp), ("NA_E", cs.NA_E), ("z0", cs.z0),
                            ("y0", cs.y0), ("all_P", np.array(all_P)), ("all_q", np.array(all_q)),
                            ("all_r", np.array(all_r)), ("all_M", np.array(all_M)), ("all_s", np.array(all_s)),
                            ("all_c", np.array(all_c)), ("all_d", np.array(all_d))):
            self.register_buffer(name, torch.Tensor(value))

        self.dim_after_map = self.n
        if create_map:
            utils.verify(input_dim is not None, "input_dim needs to be provided")
            self.mapper = nn.Linear(input_dim, self.dim_after_map)
        else:
            self.mapper = nn.Sequential()
        self._invalidate_packs()

    # ------------------------------------------------------------------ packs (rebuilt, never pickled)
    def _invalidate_packs(self):
        self.__dict__["_proj_packs"] = {}
        self.__dict__["_constants"] = {}
        self.__dict__["_unsupported"] = set()
        self.__dict__["_auto_kernel"] = {}

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate_packs()
        return out

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_proj_packs"], state["_constants"], state["_unsupported"], state["_auto_kernel"] = {}, {}, set(), {}
        state.pop("proj_iters", None)
        return state

    def proj_pack(self, device):
        """(pack, pack_id) of the program on ``device`` (built on first use)."""
        from . import ops
        index = device.index if device.index is not None else torch.cuda.current_device()
        entry = self._proj_packs.get(index)
        if entry is None:
            pack = ops.ProjPack(self.program.arrays(), index)
            entry = self._proj_packs[index] = (pack, ops.register_pack(pack))
        return entry

    def constants(self, dtype, device):
        key = (dtype, str(device))
        c = self._constants.get(key)
        if c is None:
            c = self._constants[key] = Constants(self.program, dtype, device)
        return c

    def getDimAfterMap(self):
        return self.dim_after_map

    # ------------------------------------------------------------------ the projection
    def _mirror(self, q2, max_iters, eps):
        return _MirrorProject.apply(q2, self.constants(q2.dtype, q2.device), max_iters, eps)

    def _device_kernel(self, kernel, pack, dtype):
        """``'wave'``, ``'tile'`` or ``'tile64'`` for this call.  ``'tile'`` is the tile kernel of the input's precision
        (``'tile64'`` on fp64).  ``'auto'``: the wave kernel wherever it serves the set at this precision (asked of the
        library with an empty batch: nothing is launched), else that precision's tile kernel where it does, else the wave
        kernel, whose refusal is the one reported.  No timing enters.  (The fp64 tile images are uploaded when first
        asked for: make one call before capturing a graph.)"""
        if kernel == 'tile':
            return 'tile64' if dtype == torch.float64 else 'tile'
        if kernel != 'auto':
            return kernel
        from . import ops
        key = (pack.device_index, dtype)
        cache = self.__dict__.setdefault("_auto_kernel", {})
        chosen = cache.get(key)                              # (fixed per pack and precision: asked once)
        if chosen is None:
            chosen = 'wave'
            if not ops.proj_wave_served(pack, dtype):
                if dtype == torch.float32 and ops.proj_tile_served(pack):
                    chosen = 'tile'
                elif dtype == torch.float64 and ops.proj_tile64_served(pack):
                    chosen = 'tile64'
            cache[key] = chosen
        return chosen

    def project(self, q, max_iters=None, eps=None, kernel=None):
        """``q [B, n]`` (or ``[B, n, 1]``) -> ``(z [B, n], iters [B] int32)``: the projection in the subspace and the
        iterations each row took (0: ``q`` was inside; ``max_iters``: the row did not meet the stop rule).
        ``max_iters`` / ``eps`` / ``kernel``: this call's, in place of the module's."""
        max_iters = self.max_iters if max_iters is None else int(max_iters)
        eps = self.eps if eps is None else float(eps)
        kernel = getattr(self, "kernel", "wave") if kernel is None else kernel      # (a module pickled before `kernel` existed)
        if kernel not in self.KERNELS:
            raise ValueError(f"kernel must be one of {self.KERNELS}, got {kernel!r}")
        q2 = torch.flatten(q, 1)[:, :self.n]
        if q2.dtype not in (torch.float32, torch.float64):
            z, iters = self.project(q2.float(), max_iters, eps, kernel)         # 16-bit activations: computed in fp32
            return z.to(q2.dtype), iters
        if not q2.is_cuda or (q2.device.index, q2.dtype, kernel) in self._unsupported:
            return self._mirror(q2, max_iters, eps)
        try:
            from . import ops
            pack, pack_id = self.proj_pack(q2.device)
            chosen = self._device_kernel(kernel, pack, q2.dtype)
            if not (torch.is_grad_enabled() and q2.requires_grad):
                z, iters, _ = ops.proj_forward_raw(q2, pack, max_iters, eps, kernel=chosen)
            elif chosen == 'tile':
                z, iters, _ = torch.ops.rayen_amd.euclid_project_tile(q2, pack_id, max_iters, eps)
            elif chosen == 'tile64':
                z, iters, _ = torch.ops.rayen_amd.euclid_project_tile64(q2, pack_id, max_iters, eps)
            else:
                z, iters, _ = torch.ops.rayen_amd.euclid_project(q2, pack_id, max_iters, eps)
            return z, iters
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                raise
            warnings.warn(f"rayen_amd: no HIP kernel serves this projection ({err}); this module now runs the same "
                          "iteration in torch ops (rayen_amd/projection.py) on " + str(q2.device), RuntimeWarning,
                          stacklevel=3)
            self._unsupported.add((q2.device.index, q2.dtype, kernel))
            return self._mirror(q2, max_iters, eps)

    def forward(self, x):
        nsib = x.shape[0]
        q = self.mapper(x.view(nsib, -1))
        if self.mode == 'UP' and self.training:
            z = q[:, :self.n]
        else:
            z, iters = self.project(q)
            self.__dict__["proj_iters"] = iters
        NA_E, yp = self.NA_E.to(z.dtype), self.yp.to(z.dtype)
        y = torch.addmm(yp.reshape(1, -1), z, NA_E.T)
        return y.unsqueeze(2)
