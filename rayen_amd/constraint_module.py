"""``ConstraintModule``: the RAYEN layer, drop-in for ``rayen.constraint_module.ConstraintModule``.

Same constructor, same ``forward`` contract (any ``[B, ...]`` tensor in, ``[B, k, 1]`` out,
rayen/constraint_module.py:520-533), same buffer names (so ``state_dict``s and
pickles written with the reference load here) and the same helper methods
(``getDimAfterMap, gety0, getyFromz, getzFromy, computeKappa``; :351, :506-518).

What differs is how ``forwardForRAYEN`` (:468-474) is executed: instead of ~165
PyTorch ops and 10 host syncs per call, one hand-written gfx950 kernel computes
``kappa`` for every constraint family and writes ``y = y0 + NA_E v / max(1, kappa(v))``
(the homogeneity identity of SURVEY.md §0, equal to :468-474 for every ``v``).
Tensors on a HIP device go to those kernels (a missing ``librayen_hip.so`` is a loud error, never a detour);
tensors on the host -- the reference's own smoke test runs there -- and constraint sets no kernel serves
(with a one-time ``RuntimeWarning``; ``RAYEN_STRICT_HIP=1`` makes it an error) are evaluated from the same packed
constants with plain torch ops on the caller's device (``rayen_amd/eager.py``; this is not the test oracle).

``method='RAYEN'`` (the default) is the hot path this package accelerates; its older step rule
``'RAYEN_old'`` (:460-466) runs on the same kernels; ``'UU'`` is the identity and kept because it
is free; ``'Bar'`` (the barycentric baseline, :124-132 and :479-486) converts the linear part of the set to
vertices and rays once (``rayen_amd/vrep.py``, no cddlib) and runs one HIP kernel per direction
(``rayen_amd/csrc/rayen_bar.hip``, or with the keyword ``bar_kernel='stream' | 'auto'`` ``rayen_bar_stream.hip``, which
needs no LDS proportional to the number of generators); ``'DC3'`` (completion + gradient correction, :134-228 and :265-336, linear and
quadratic sets only) needs ``args_DC3`` and runs its fixed iteration, batch-global stop included, on
``rayen_amd/csrc/rayen_dc3.hip`` or, with ``args_DC3['kernel'] = 'tile' | 'auto'``, ``rayen_dc3_tile.hip`` (fp32 input) or
``rayen_dc3_tile64.hip`` (fp64 input) (host side: ``rayen_amd/dc3.py``).  The other paper baselines (``UP, PP``) raise
``NotImplementedError`` here: they are served by a module of their own, ``rayen_amd.projection.ProjectionModule``.

Documented deviation: for an SOC whose ray never meets the cone (negative
discriminant with ``c' < 0``) the reference's assert at :342 fires (or NaN under
``python -O``); here that constraint contributes ``kappa_j = 0``, its mathematical value.
"""
from __future__ import annotations

import copy
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib, dc3 as _dc3, eager, ops, pack as _pack, utils


class ConstraintModule(torch.nn.Module):
    _fast = {}                    # (replaced per instance; a pickle written before round 4 has no such attribute)

    # Which (device index, dtype, old_head) combinations the HIP kernels refused (RAYEN_E_UNSUPPORTED, announced with a
    # warning): those calls -- and only those -- run rayen_amd/eager.py.  Forgotten whenever the packs are rebuilt
    # (.to(), load_state_dict) and never pickled.  ``_hip_unsupported`` is the any-of view the tests read.
    @property
    def _hip_unsupported(self):
        return bool(self.__dict__.get("_unsupported"))

    @_hip_unsupported.setter
    def _hip_unsupported(self, value):
        if value:
            self.__dict__.setdefault("_unsupported", set()).add(None)     # (None: every combination)
        else:
            self.__dict__["_unsupported"] = set()

    def _refused(self, v, old_head=False):
        refused = self.__dict__.get("_unsupported")
        return bool(refused) and (None in refused or (v.device.index, v.dtype, self._route_key(old_head)) in refused)

    def _route_key(self, old_head=False):
        """Third part of a refusal's key: the old head of RAYEN_old, the kernel ``args_DC3`` asks for (``False`` for the
        default, ``'lane'``), the kernel ``bar_kernel`` asks for (``False`` for the default, ``'resident'``), the kernel
        ``wide_kernel`` asks for under method 'RAYEN' (``False`` for the default, ``'products'``; with a ``wide_backward``
        other than the default, ``'<wide_kernel>+bwd_<wide_backward>'``), ``False`` otherwise."""
        if self.method == 'DC3':
            kernel = _dc3.kernel_choice(self.args_DC3)
            return False if kernel == 'lane' else kernel
        if self.method == 'Bar':
            kernel = getattr(self, 'bar_kernel', 'resident')
            return False if kernel == 'resident' else kernel
        if self.method == 'RAYEN' and getattr(self, 'wide_backward', 'products') != 'products':
            return getattr(self, 'wide_kernel', 'products') + '+bwd_' + self.wide_backward
        if self.method == 'RAYEN' and getattr(self, 'wide_kernel', 'products') != 'products':
            return self.wide_kernel          # (method 'RAYEN' has no old head)
        return bool(old_head)

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if name == "mapper":
            self.__dict__["_fast"] = {}       # (the fast path caches "the mapper is the identity" per device and dtype)

    BAR_KERNELS = ('resident', 'stream', 'auto')
    WIDE_KERNELS = ops.WIDE_KERNELS
    WIDE_BACKWARDS = ops.WIDE_BACKWARDS

    def __init__(self, cs, input_dim=None, method='RAYEN', create_map=True, args_DC3=None, *, bar_kernel='resident',
                 bar_window_bytes=0, wide_kernel='products', wide_backward='products', fuse_mapper64=False):
        super().__init__()

        self.method = method
        if fuse_mapper64 and method != 'RAYEN':
            raise ValueError(f"fuse_mapper64={fuse_mapper64!r} chooses a kernel of method 'RAYEN'; this module's method is {method!r}")
        # fp64 input behind an nn.Linear mapper: True evaluates the mapper inside the fp64 matrix-core forward (the MAPPED
        # instances of rayen_mfma_f64.hip: one launch, v written only for the backward) where ops.mapper_fusable64 serves
        # the call, and runs the two ops otherwise, silently, as fuse_mapper does in fp32.  Off by default: no timing
        # enters a dispatch here.  fuse_mapper = False switches both precisions off.
        self.fuse_mapper64 = bool(fuse_mapper64)
        if wide_kernel not in self.WIDE_KERNELS:
            raise ValueError(f"wide_kernel must be one of {self.WIDE_KERNELS}, got {wide_kernel!r}")
        if wide_kernel != 'products' and method != 'RAYEN':
            raise ValueError(f"wide_kernel={wide_kernel!r} chooses a kernel of method 'RAYEN'; this module's method is {method!r}")
        # method='RAYEN' on wide sets (n beyond the register-resident kernels, ops._WIDE_MIN_N): 'products' (the default: a
        # library GEMM and rayen_wide.hip over its products) or 'fused' (rayen_wide_fused.hip: one launch, no products
        # matrix; fp32, no LMI, n <= 1024 -- anything else takes the module's loud path) or 'fused64' (its fp64 twin,
        # rayen_wide_fused64.hip: fp64 input, no LMI, n <= 1024 -- anything else likewise).  No effect on narrower sets.  The
        # backward is chosen by `wide_backward` below (the products route by default).  There is no 'auto': both serve the same sets, and no timing
        # enters a dispatch here.
        self.wide_kernel = wide_kernel
        if wide_backward not in self.WIDE_BACKWARDS:
            raise ValueError(f"wide_backward must be one of {self.WIDE_BACKWARDS}, got {wide_backward!r}")
        if wide_backward != 'products' and method != 'RAYEN':
            raise ValueError(f"wide_backward={wide_backward!r} chooses a kernel of method 'RAYEN'; this module's method is {method!r}")
        # the backward of the same sets, chosen independently (it consumes kappa and active of whichever forward made them):
        # 'products' (the default: two library GEMMs around the coefficient kernel of rayen_wide.hip) or 'fused'
        # (rayen_wide_fused_bwd.hip: one launch over the active constraints' rows; fp32, no LMI, n <= 1024 -- anything else
        # takes the backward's loud path, ops._bwd_or_detour) or 'fused64' (its fp64 twin, rayen_wide_fused_bwd64.hip: fp64
        # input, no LMI, n <= 1024 -- anything else likewise).  No 'auto' here either.
        self.wide_backward = wide_backward
        if bar_kernel not in self.BAR_KERNELS:
            raise ValueError(f"bar_kernel must be one of {self.BAR_KERNELS}, got {bar_kernel!r}")
        if bar_kernel != 'resident' and method != 'Bar':
            raise ValueError(f"bar_kernel={bar_kernel!r} chooses a kernel of method 'Bar'; this module's method is {method!r}")
        if isinstance(bar_window_bytes, bool) or not isinstance(bar_window_bytes, int) or bar_window_bytes < 0 \
                or bar_window_bytes % 16:
            raise ValueError(f"bar_window_bytes must be 0 (the default window) or a positive multiple of 16, got {bar_window_bytes!r}")
        if bar_window_bytes and bar_kernel == 'resident':
            raise ValueError("bar_window_bytes is the window of the streamed kernels: it needs bar_kernel='stream' or 'auto'")
        # method='Bar' on a HIP device: 'resident' (rayen_bar.hip, the image of G in LDS), 'stream' (rayen_bar_stream.hip, the
        # image streamed through LDS in windows: no limit on the number of generators) or 'auto' (resident where it serves
        # the pack at the input's dtype, else stream).  bar_window_bytes: the streamed kernels' window for tests and
        # measurements, 0 = the default; the library refuses (RAYEN_E_BAD_ARG) one beyond the default or below one group of
        # four generators at the pack's K.
        self.bar_kernel = bar_kernel
        self.bar_window_bytes = bar_window_bytes
        if method == 'Bar' and cs.has_quadratic_constraints:
            raise Exception(f"Method {method} cannot be used with quadratic constraints")     # (:24-25)
        if method == 'DC3':
            if cs.has_soc_constraints or cs.has_lmi_constraints:
                raise NotImplementedError("method 'DC3' serves linear and quadratic constraints only")     # (:27-28)
            _dc3.check_args(args_DC3)        # (None: NotImplementedError, a RuntimeError like the reference's verify, :31)
        elif method not in ('RAYEN', 'RAYEN_old', 'UU', 'Bar'):
            if method in ('UP', 'PP'):
                raise NotImplementedError(
                    f"method '{method}' is one of the reference's comparison baselines; rayen_amd "
                    "implements the RAYEN projection only")
            raise NotImplementedError
        self.args_DC3 = args_DC3

        self.cs = cs
        self.k = cs.k  # dimension of the ambient space
        self.n = cs.n  # dimension of the embedded space

        # every row of A_p divided by its slack at z0 (rayen/constraint_module.py:38)
        D = cs.A_p / ((cs.b_p - cs.A_p @ cs.z0) @ np.ones((1, cs.n)))

        all_P, all_q, all_r = utils.getAllPqrFromQcs(cs.qcs)
        all_M, all_s, all_c, all_d = utils.getAllMscdFromSocs(cs.socs)

        if cs.has_lmi_constraints:
            # H = F_k + sum_i y0_i F_i,  H^-1 = L L'  (:43-52); like the reference, the
            # last slot of the all_F buffer ends up holding H
            all_F = copy.deepcopy(cs.lmic.all_F)
            H = np.array(all_F[-1], dtype=np.float64)
            for i in range(cs.lmic.dim()):
                H = H + cs.y0[i, 0] * cs.lmic.all_F[i]
            all_F[-1] = H
            Hinv = np.linalg.inv(H)
            self.register_buffer("mHinv", torch.Tensor(-Hinv))
            self.register_buffer("L", torch.Tensor(np.linalg.cholesky(Hinv)))
        else:
            all_F = []

        # buffers follow .to(device) and appear in state_dict under the reference's names (:59-74)
        self.register_buffer("D", torch.Tensor(D))
        self.register_buffer("all_P", torch.Tensor(np.array(all_P)))
        self.register_buffer("all_q", torch.Tensor(np.array(all_q)))
        self.register_buffer("all_r", torch.Tensor(np.array(all_r)))
        self.register_buffer("all_M", torch.Tensor(np.array(all_M)))
        self.register_buffer("all_s", torch.Tensor(np.array(all_s)))
        self.register_buffer("all_c", torch.Tensor(np.array(all_c)))
        self.register_buffer("all_d", torch.Tensor(np.array(all_d)))
        self.register_buffer("all_F", torch.Tensor(np.array(all_F)))
        self.register_buffer("A_p", torch.Tensor(cs.A_p))
        self.register_buffer("b_p", torch.Tensor(cs.b_p))
        self.register_buffer("yp", torch.Tensor(cs.yp))
        self.register_buffer("NA_E", torch.Tensor(cs.NA_E))
        self.register_buffer("z0", torch.Tensor(cs.z0))
        self.register_buffer("y0", torch.Tensor(cs.y0))

        if cs.has_quadratic_constraints:
            # sigma, phi, delta per quadratic, evaluated at the default dtype like the reference (:99-122)
            all_delta, all_phi = [], []
            y0 = self.y0
            for i in range(self.all_P.shape[0]):
                P, q, r = self.all_P[i, :, :], self.all_q[i, :, :], self.all_r[i, :, :]
                g_y0 = 0.5 * y0.T @ P @ y0 + q.T @ y0 + r
                sigma = 2 * g_y0
                grad_row = y0.T @ P + q.T
                all_phi.append(-grad_row / sigma)
                all_delta.append((grad_row.T @ grad_row - 4 * g_y0 * 0.5 * P) / torch.square(sigma))
            self.register_buffer("all_delta", torch.stack(all_delta))
            self.register_buffer("all_phi", torch.stack(all_phi))

        if self.method == 'Bar':
            # vertices and rays of the linear part {z : A_p z <= b_p} (:124-132); cones and LMIs are not imposed
            if cs.has_soc_constraints or cs.has_lmi_constraints:
                warnings.warn("method 'Bar' imposes the linear constraints only: the second-order-cone and LMI "
                              "constraints of this set are not imposed", UserWarning, stacklevel=2)
            from .vrep import H_to_V
            V, R = H_to_V(cs.A_p, cs.b_p)
            self.register_buffer("V", torch.Tensor(V))
            self.register_buffer("R", torch.Tensor(R))
            self.num_vertices = self.V.shape[1]
            self.num_rays = self.R.shape[1]
            assert (self.num_vertices + self.num_rays) > 0
            self._bar_packs = {}

        if self.method == 'DC3':
            _dc3.setup(self, cs)
            self._dc3_packs = {}

        if self.method == 'RAYEN':
            self.forwardForMethod = self.forwardForRAYEN
            self.dim_after_map = self.n
        elif self.method == 'DC3':
            self.forwardForMethod = self.forwardForDC3
            self.dim_after_map = self.k - self.neq_DC3
            assert self.dim_after_map == self.n
        elif self.method == 'RAYEN_old':
            self.forwardForMethod = self.forwardForRAYENOld
            self.dim_after_map = self.n + 1
        elif self.method == 'Bar':
            self.forwardForMethod = self.forwardForBar
            self.dim_after_map = self.num_vertices + self.num_rays
        else:  # 'UU'
            self.forwardForMethod = self.forwardForUU
            self.dim_after_map = self.k

        if create_map:
            utils.verify(input_dim is not None, "input_dim needs to be provided")
            self.mapper = nn.Linear(input_dim, self.dim_after_map)
        else:
            self.mapper = nn.Sequential()  # mapper does nothing

        # fused NaN check: the kernel raises a device flag instead of re-reading y (:531)
        self.check_nan = True
        # evaluate the mapper inside the projection kernel when the shapes allow it (one launch, v
        # never written to memory in inference); False = always run nn.Linear as its own GEMM
        self.fuse_mapper = True
        # True: clipped samples stop 2^-20 of their step short of the boundary in fp32 instead of ON it, where half of the fp32
        # roundings fall outside (the fp32 kernels evaluate (1 + 2^-20) kappa, RAYEN_PREPARE_INWARD_BIAS in include/rayen_hip.h;
        # fp64 and interior samples untouched).  Measured on 65 536 rows of config 3 (profiles/bench/r06_inward_bias.txt): rows
        # with a positive fp64 residual 31 594 -> 1, outputs moved by at most 1.3e-6 of a row.  OFF by default: the shift is
        # 2^-20 of the STEP y - y0, and on a row whose y is small against its step (the reference's example sets: a point near the
        # origin reached from y0 = (0.5, 0.5)) that is more than the 1e-5 of the row the parity bar allows -- the golden vectors
        # fail with it on (round 6, gpurun_out/r06d).  Read when a device's constants are packed (first forward on that device).
        self.inward_bias = False
        self._device_packs = {}
        self._consts = None
        self._fast = {}

    # ------------------------------------------------------------------ constant packs
    def _invalidate_packs(self):
        self._device_packs = {}
        self._consts = None
        self._fast = {}
        self.__dict__["_unsupported"] = set()
        self.__dict__.pop("_eager", None)
        self.__dict__["_bar_packs"] = {}
        self.__dict__["_dc3_packs"] = {}

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate_packs()  # buffers moved or changed dtype
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._invalidate_packs()
        return out

    def packed_constants(self):
        """Host-side (fp64) row matrix + segment table derived from the buffers."""
        if self._consts is None:
            names = ("D", "NA_E", "z0", "yp", "y0", "all_phi", "all_delta", "all_M", "all_s",
                     "all_c", "all_d", "all_F", "L", "all_P")
            exact = ([(qc.P, qc.q, qc.r) for qc in self.cs.qcs], self.cs.y0) if self.cs.qcs else None
            self._consts = _pack.pack_constants({n: getattr(self, n) for n in names if hasattr(self, n)},
                                                exact_quadratics=exact)
        return self._consts

    def device_pack(self, device):
        """(pack, pack_id) with the constants resident on ``device`` (built on first use)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        entry = self._device_packs.get(index)
        if entry is None:
            # (inward_bias: RAYEN_PREPARE_INWARD_BIAS, include/rayen_hip.h -- set the attribute before the first forward)
            dp = _pack.DevicePack(self.packed_constants(), index,
                                  prepare=_lib.PREPARE_INWARD_BIAS if getattr(self, "inward_bias", False) else 0)
            entry = (dp, ops.register_pack(dp))
            self._device_packs[index] = entry
        return entry

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_device_packs"] = {}   # device handles are not picklable; rebuilt lazily
        state["_consts"] = None
        state["_fast"] = {}
        state["_unsupported"] = set()
        state.pop("_eager", None)
        state["_bar_packs"] = {}
        state["_dc3_packs"] = {}
        state.pop("dc3_steps", None)
        state.pop("forwardForMethod", None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._fast = {}
        self.__dict__.setdefault("bar_kernel", 'resident')       # (pickles from before the streamed Bar kernels)
        self.__dict__.setdefault("bar_window_bytes", 0)
        self.__dict__.setdefault("wide_kernel", 'products')      # (pickles from before the fused wide forward)
        self.__dict__.setdefault("wide_backward", 'products')    # (pickles from before the fused wide backward)
        self.__dict__.setdefault("fuse_mapper64", False)         # (pickles from before the fused fp64 mapper)
        self.forwardForMethod = {'RAYEN': self.forwardForRAYEN, 'RAYEN_old': self.forwardForRAYENOld,
                                 'UU': self.forwardForUU, 'Bar': self.forwardForBar,
                                 'DC3': self.forwardForDC3}[self.method]

    # ------------------------------------------------------------------ the projection
    def _project(self, q, old_head=False):
        """``q [B, >=n, 1]`` (or ``[B, >=n]``) -> ``(y [B,k], kappa [B])`` through the fused HIP op."""
        v = torch.flatten(q, 1)
        if not v.is_cuda:
            # tensors on the host (the reference's own smoke runs there, examples/test_layer.py:70-117): the packed form
            # in plain torch ops on the caller's device, differentiable through autograd -- rayen_amd/eager.py
            return eager.project(self, v, old_head=old_head)
        if v.dtype not in (torch.float32, torch.float64):
            y, kappa = self._project(v.float(), old_head=old_head)       # 16-bit activations: computed in fp32
            return y.to(v.dtype), (None if kappa is None else kappa.to(v.dtype))
        if self._refused(v, old_head):
            return eager.project(self, v, old_head=old_head)
        try:
            dp, pack_id = self.device_pack(v.device)
            need_active = torch.is_grad_enabled() and v.requires_grad
            wide = 'products' if old_head else getattr(self, "wide_kernel", 'products')
            fused = wide == 'fused'
            if not need_active and type(v) is torch.Tensor and not torch.compiler.is_compiling():
                # plain inference call: straight to the C ABI (the same code the registered op runs; the dispatcher
                # layers around a custom op cost ~10 us per call, as much as the kernel at small batches)
                y, _, _ = ops.project_raw(v, dp, want_active=False, old_head=old_head, want_kappa=False, wide_kernel=wide)
                return y, None
            if not old_head and (getattr(self, "wide_backward", 'products') != 'products' or wide == 'fused64'):
                # (the op that carries both strings: 'fused64' has no op of its own)
                y, kappa, _ = torch.ops.rayen_amd.ray_project_wide(v, pack_id, need_active, wide,
                                                                   getattr(self, "wide_backward", 'products'))
            elif fused:
                y, kappa, _ = torch.ops.rayen_amd.ray_project_wide_fused(v, pack_id, need_active)
            else:
                y, kappa, _ = torch.ops.rayen_amd.ray_project(v, pack_id, need_active, old_head)
            return y, kappa
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                raise
            # a shape no HIP kernel serves: say so ONCE, then evaluate the packed form with torch ops on
            # the same device.  Never silent, never for a missing library (that raises in _lib.load), and
            # RAYEN_STRICT_HIP=1 turns it back into the error.
            warnings.warn(f"rayen_amd: no HIP kernel serves this constraint set ({err}); this module now runs the "
                          "packed torch evaluator (rayen_amd/eager.py) on " + str(v.device), RuntimeWarning, stacklevel=3)
            self.__dict__.setdefault("_unsupported", set()).add((v.device.index, v.dtype, self._route_key(old_head)))
            return eager.project(self, v, old_head=old_head)

    def computeKappa(self, v_bar):
        """``kappa [B,1,1]`` of directions ``v_bar [B,n,1]`` (rayen/constraint_module.py:351-458)."""
        v = torch.flatten(v_bar, 1)
        if not v.is_cuda or self._refused(v) or v.dtype not in (torch.float32, torch.float64):
            return eager.evaluator_for(self, v).kappa(v[:, :self.n]).reshape(-1, 1, 1)
        dp, _ = self.device_pack(v.device)
        wide = self.wide_kernel if self.method == 'RAYEN' else 'products'
        try:
            _, kappa, _ = ops.project_raw(v, dp, want_y=False, want_active=False, wide_kernel=wide)
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED:
                raise
            # the kernels that always write y (an LMI on the workgroup-per-sample kernels, alone, next to quadratics / cones
            # or behind the products GEMM; rayen_abi.hip::mixed_forward) decline y == NULL: same kernels, a scratch y
            try:
                _, kappa, _ = ops.project_raw(v, dp, want_y=True, want_active=False, wide_kernel=wide)
            except _lib.RayenError as err2:
                if err2.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                    raise
                return eager.evaluator_for(self, v).kappa(v[:, :self.n]).reshape(-1, 1, 1)
        return kappa.reshape(-1, 1, 1)

    def forwardForRAYEN(self, q):
        y, _ = self._project(q)
        return y.unsqueeze(2)

    def forwardForRAYENOld(self, q):
        # step 1/(exp(beta) + kappa) with beta = q[:, n] (rayen/constraint_module.py:460-466)
        y, _ = self._project(q, old_head=True)
        return y.unsqueeze(2)

    def forwardForUU(self, q):
        return q

    # ------------------------------------------------------------------ method='Bar'
    def bar_pack(self, device):
        """(pack, pack_id): ``G = NA_E [V R]`` and ``yp`` of the CURRENT buffers resident on ``device`` (built on first
        use; forgotten by ``.to()`` and ``load_state_dict``, so a loaded ``V`` / ``R`` is what the kernels read)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        packs = self.__dict__.setdefault("_bar_packs", {})
        entry = packs.get(index)
        if entry is None:
            NA_E = self.NA_E.detach().double().cpu()
            G = torch.cat([NA_E @ self._bar_generators(self.V), NA_E @ self._bar_generators(self.R)], dim=1)
            bp = ops.BarPack(G.numpy(), self.yp.detach().double().cpu().numpy(), self.num_vertices, self.num_rays, index)
            entry = packs[index] = (bp, ops.register_pack(bp))
        return entry

    def _bar_generators(self, X):
        return X.detach().double().cpu().reshape(self.n, -1) if X.numel() else torch.zeros((self.n, 0), dtype=torch.float64)

    def _bar_reference(self, q):
        """The reference formula (:479-486) in plain torch ops on ``q``'s device and dtype."""
        nv, nr = self.num_vertices, self.num_rays
        lambdas = nn.functional.softmax(q[:, 0:nv, 0:1], dim=1)
        mus = torch.abs(q[:, nv:nv + nr, 0:1])
        z = (self.V.to(q.dtype) @ lambdas if nv else 0) + (self.R.to(q.dtype) @ mus if nr else 0)
        return self.NA_E.to(q.dtype) @ z + self.yp.to(q.dtype)

    def _bar_kernel_for(self, bp, dtype):
        """The kernel a call at ``dtype`` runs.  ``'auto'``: the resident kernel wherever it serves the pack at ``dtype``,
        else the streamed one (which serves every pack).  No timing enters the choice."""
        kernel = self.bar_kernel
        if kernel != 'auto':
            return kernel
        return 'resident' if bp.resident_served(dtype) else 'stream'

    def forwardForBar(self, q):
        if not q.is_cuda:
            return self._bar_reference(q)        # host tensors: the reference's formula, differentiable by autograd
        q2 = torch.flatten(q, 1)
        if q2.dtype not in (torch.float32, torch.float64):
            return self.forwardForBar(q2.float().unsqueeze(2)).to(q2.dtype)     # 16-bit activations: computed in fp32
        if self._refused(q2):
            return self._bar_reference(q2.unsqueeze(2))
        try:
            bp, pack_id = self.bar_pack(q2.device)
            kernel = self._bar_kernel_for(bp, q2.dtype)
            window = int(self.bar_window_bytes)
            if not (torch.is_grad_enabled() and q2.requires_grad) and not torch.compiler.is_compiling():
                # plain inference: straight to the C ABI
                y, _ = ops.bar_forward_raw(q2, bp, want_rowstat=False, kernel=kernel, window_bytes=window)
            elif kernel == 'stream':
                y, _ = torch.ops.rayen_amd.bar_project_stream(q2, pack_id, window)
            else:
                y, _ = torch.ops.rayen_amd.bar_project(q2, pack_id)
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                raise
            warnings.warn(f"rayen_amd: no HIP kernel serves this Bar layer ({err}); this module now runs the reference "
                          "formula with torch ops on " + str(q2.device), RuntimeWarning, stacklevel=3)
            self.__dict__.setdefault("_unsupported", set()).add((q2.device.index, q2.dtype, self._route_key()))
            return self._bar_reference(q2.unsqueeze(2))
        return y.unsqueeze(2)

    # ------------------------------------------------------------------ method='DC3'
    def dc3_pack(self, device):
        """(pack, pack_id): the effective forms of the CURRENT buffers resident on ``device`` (built on first use;
        forgotten by ``.to()`` and ``load_state_dict``)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        packs = self.__dict__.setdefault("_dc3_packs", {})
        entry = packs.get(index)
        if entry is None:
            dp = ops.Dc3Pack(_dc3.pack_arrays(self), index)
            entry = packs[index] = (dp, ops.register_pack(dp))
            # what 'tile' / 'auto' need from the device is settled here, with the pack's own uploads (like them, not while
            # a stream is capturing): the calls after the first only look the answers up
            # (under 'tile' the fp64 image waits for the first fp64 call: that call must precede a capture)
            kernel = self.dc3_kernel
            if kernel == 'tile':
                dp.tile_images()
            elif kernel == 'auto':
                for dtype in (torch.float32, torch.float64):
                    self._dc3_kernel_for(dp, dtype)
        return entry

    @property
    def dc3_kernel(self):
        """What ``args_DC3['kernel']`` asks for: ``'lane'`` (the default, rayen_dc3.hip), ``'tile'`` (rayen_dc3_tile.hip
        for fp32 input, rayen_dc3_tile64.hip for fp64 input) or ``'auto'``."""
        return _dc3.kernel_choice(self.args_DC3)

    def _dc3_kernel_for(self, dp, dtype):
        """The kernel of ``ops`` a call at ``dtype`` runs.  ``'tile'``: the tile kernel of that dtype (``'tile'`` in fp32,
        ``'tile64'`` in fp64).  ``'auto'``: the lane kernel wherever it serves the pack at ``dtype``, else the tile kernel
        of that dtype where it does, else the lane kernel, whose refusal is then the one reported.  No timing enters the
        choice."""
        kernel = self.dc3_kernel
        if kernel == 'tile':
            return 'tile64' if dtype == torch.float64 else 'tile'
        if kernel != 'auto':
            return kernel
        if ops.dc3_lane_served(dp, dtype):
            return 'lane'
        if dtype == torch.float32 and ops.dc3_tile_served(dp):
            return 'tile'
        if dtype == torch.float64 and ops.dc3_tile64_served(dp):
            return 'tile64'
        return 'lane'

    def obtainyoFromypDC3(self, yp):
        return self.A2oi @ (self.b2_DC3 - self.A2p @ yp)

    def _dc3_reference(self, q):
        """The reference iteration (:269-336) in plain torch ops on ``q``'s device and dtype; ``dc3_steps`` receives the
        number of steps it took, as on the kernel path."""
        y, steps = _dc3.reference_forward(self, q, return_steps=True)
        self.__dict__["dc3_steps"] = torch.tensor([steps], dtype=torch.int32, device=q.device)
        return y

    def forwardForDC3(self, q):
        if not q.is_cuda:
            return self._dc3_reference(q)        # host tensors: the reference's formula, differentiable by autograd
        q2 = torch.flatten(q, 1)
        if q2.dtype not in (torch.float32, torch.float64):
            return self.forwardForDC3(q2.float().unsqueeze(2)).to(q2.dtype)     # 16-bit activations: computed in fp32
        if self._refused(q2):
            return self._dc3_reference(q2.unsqueeze(2))
        args = self.args_DC3
        lr, momentum, eps = float(args['lr']), float(args['momentum']), float(args['eps_converge'])
        limit = _dc3.max_steps(self)
        try:
            dp, pack_id = self.dc3_pack(q2.device)
            kernel = self._dc3_kernel_for(dp, q2.dtype)
            if not (torch.is_grad_enabled() and q2.requires_grad) and not torch.compiler.is_compiling():
                y, steps = ops.dc3_forward_raw(q2, dp, lr, momentum, eps, limit, kernel)      # plain inference: straight to the C ABI
            elif kernel == 'tile':
                y, steps = torch.ops.rayen_amd.dc3_project_tile(q2, pack_id, lr, momentum, eps, limit)
            elif kernel == 'tile64':
                y, steps = torch.ops.rayen_amd.dc3_project_tile64(q2, pack_id, lr, momentum, eps, limit)
            else:
                y, steps = torch.ops.rayen_amd.dc3_project(q2, pack_id, lr, momentum, eps, limit)
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                raise
            warnings.warn(f"rayen_amd: no HIP kernel serves this DC3 layer ({err}); this module now runs the reference "
                          "formula with torch ops on " + str(q2.device), RuntimeWarning, stacklevel=3)
            self.__dict__.setdefault("_unsupported", set()).add((q2.device.index, q2.dtype, self._route_key()))
            return self._dc3_reference(q2.unsqueeze(2))
        self.__dict__["dc3_steps"] = steps      # [1] int32 on q's device: the steps this call took (every route sets it)
        return y.unsqueeze(2)

    # ------------------------------------------------------------------ reference helper surface
    def getDimAfterMap(self):
        return self.dim_after_map

    def gety0(self):
        return self.getyFromz(self.z0)

    def getyFromz(self, z):
        return self.NA_E @ z + self.yp

    def getzFromy(self, y):
        return self.NA_E.T @ (y - self.yp)

    def _forward_fused_mapper(self, x2):
        """mapper + projection as ONE kernel launch (``rayen_amd::ray_project_mapped``; fp64 input with
        ``fuse_mapper64``: ``rayen_amd::ray_project_mapped64``) or ``None`` when
        the fused kernel does not serve this layer/input (then the two-op path below runs)."""
        if (self.method != 'RAYEN' or not getattr(self, "fuse_mapper", True)
                or not isinstance(self.mapper, nn.Linear) or not x2.is_cuda
                or x2.dtype not in (torch.float32, torch.float64)
                or (x2.dtype == torch.float64 and not getattr(self, "fuse_mapper64", False))
                or self._refused(x2)):
            return None
        try:
            dp, pack_id = self.device_pack(x2.device)
        except _lib.RayenError:
            return None           # (the two-op path below reports it)
        weight, bias = self.mapper.weight, self.mapper.bias
        f64 = x2.dtype == torch.float64
        if not (ops.mapper_fusable64 if f64 else ops.mapper_fusable)(x2, weight, bias, dp):
            return None
        need_grad = torch.is_grad_enabled() and (x2.requires_grad or weight.requires_grad
                                                 or (bias is not None and bias.requires_grad))
        op = torch.ops.rayen_amd.ray_project_mapped64 if f64 else torch.ops.rayen_amd.ray_project_mapped
        y, _, _, _ = op(x2, weight, bias, pack_id, need_grad)
        return y.unsqueeze(2)

    # ------------------------------------------------------------------ small-batch inference fast path
    def _fast_entry(self, x):
        """Per-(device, dtype) prebuilt call of the C ABI for plain inference with the identity mapper: pack handle,
        ctypes entry point, NaN-flag address and sizes looked up ONCE (round 4: the generic route -- flatten, the empty
        nn.Sequential, unsqueeze, _project, ops.project_raw and their re-validation -- cost ~13 us of Python per call in
        front of a 4.5 us kernel at config 1).  ``None`` when the layer has a mapper, another method, or no HIP kernel."""
        key = (x.device.index, x.dtype)
        entry = self._fast.get(key, False)
        if entry is False:
            entry = None
            if (self.method == 'RAYEN' and isinstance(self.mapper, nn.Sequential) and len(self.mapper) == 0
                    and not self._refused(x) and x.dtype in (torch.float32, torch.float64)
                    and self.n < ops._WIDE_MIN_N[x.dtype]      # (wide sets: GEMM + products epilogue, ops.project_raw)
                    # (a set with an LMI may take the wide route earlier: wide_kernel='fused' gets its refusal there)
                    and not (getattr(self, "wide_kernel", 'products') in ('fused', 'fused64') and self.cs.has_lmi_constraints)):
                try:
                    dp, _ = self.device_pack(x.device)
                    fn = ops._entry(ops._FWD[(x.dtype, False)])
                    entry = (fn, dp.handle, dp.nan_flag.data_ptr(), self.k, self.n, x.device.index, dp)
                except _lib.RayenError:
                    entry = None           # (the generic route reports it)
            self._fast[key] = entry
        return entry

    def forward(self, x):
        # x: [nsib, numel_input_mapper, 1]; after the mapper q is [nsib, numel_output_mapper, 1]
        if (type(x) is torch.Tensor and x.is_cuda and x.dim() >= 2 and x.is_contiguous()
                and not (x.requires_grad and torch.is_grad_enabled()) and not torch.compiler.is_compiling()):
            entry = self._fast_entry(x)
            if entry is not None:
                fn, handle, nan_ptr, k, n, index, dp = entry
                B = x.shape[0]
                width = x.numel() // B if B else n
                if width >= n and dp.handle is not None:
                    y = torch.empty((B, k, 1), dtype=x.dtype, device=x.device)
                    if torch.cuda.current_device() == index:
                        code = fn(handle, x.data_ptr(), B, width, y.data_ptr(), k, None, None, nan_ptr,
                                  ops._stream(index))
                    else:
                        with torch.cuda.device(index):
                            code = fn(handle, x.data_ptr(), B, width, y.data_ptr(), k, None, None, nan_ptr,
                                      ops._stream(index))
                    if code == 0:
                        if __debug__ and self.check_nan and not torch.cuda.is_current_stream_capturing():
                            if int(dp.nan_flag.item()) != 0:      # the flag read is a host sync (CM:531 is one too)
                                dp.nan_flag.zero_()
                                raise AssertionError("the projection produced NaN (NaN in the input?)")
                        return y
                    if code != _lib.E_UNSUPPORTED:
                        _lib.check(code, "rayen_ray_project")
                    self._fast[(x.device.index, x.dtype)] = None     # no kernel for this set: the route below says so
        x2 = torch.flatten(x, 1)  # == x.view(B, -1), and defined for B = 0
        y = self._forward_fused_mapper(x2)
        if y is None:
            q = torch.unsqueeze(self.mapper(x2), dim=2)
            y = self.forwardForMethod(q)

        if __debug__ and self.check_nan and self.method in ('RAYEN', 'RAYEN_old', 'Bar', 'DC3'):
            what = "the projection produced NaN (NaN in the input?)"
            if self.method == 'DC3':      # (the reference's words, CM:531)
                what = f"If you are using DC3, try reducing args_DC3['lr']. Right now it's {self.args_DC3['lr']}"
            if not y.is_cuda or self._refused(y, self.method == 'RAYEN_old'):
                assert not torch.isnan(y).any(), what     # CM:531
            elif not torch.cuda.is_current_stream_capturing():  # the flag read is a host sync
                dp, _ = (self.bar_pack(y.device) if self.method == 'Bar' else
                         self.dc3_pack(y.device) if self.method == 'DC3' else self.device_pack(y.device))
                if int(dp.nan_flag.item()) != 0:
                    dp.nan_flag.zero_()
                    raise AssertionError(what)
        return y
