"""ctypes binding of the C ABI in ``include/rayen_hip.h`` (``librayen_hip.so``).

There is deliberately no fallback: if the shared library is missing or an entry
point fails, the error is raised to the caller.
"""
from __future__ import annotations

import ctypes
import os

from ._build import LIBRARY

ABI_VERSION = 15

SEG_LIN, SEG_QUAD_SYM, SEG_QUAD_FAC, SEG_SOC, SEG_LMI = range(5)
E_UNSUPPORTED = -6      # RAYEN_E_UNSUPPORTED (include/rayen_hip.h)
PREPARE_ALL, PREPARE_F32, PREPARE_F64, PREPARE_FWD_ONLY, PREPARE_INWARD_BIAS = 0, 1, 2, 4, 8

# every symbol include/rayen_hip.h declares
EXPORTS = (
    "rayen_abi_version", "rayen_strerror", "rayen_pack_create", "rayen_pack_destroy",
    "rayen_pack_info", "rayen_ray_project_f32", "rayen_ray_project_f64",
    "rayen_ray_project_generic_f32", "rayen_ray_project_generic_f64", "rayen_ray_project_bwd_f32",
    "rayen_ray_project_bwd_f64", "rayen_ray_project_old_f32", "rayen_ray_project_old_f64",
    "rayen_ray_project_old_bwd_f32", "rayen_ray_project_old_bwd_f64",
    "rayen_mapper_fusable", "rayen_ray_project_mapped_f32", "rayen_ray_project_bwd_generic_f32",
    "rayen_ray_project_bwd_generic_f64", "rayen_mapper_image_bytes", "rayen_mapper_prepare_f32",
    "rayen_ray_project_mapped_image_f32", "rayen_bwd_workspace_bytes_f32", "rayen_ray_project_bwd_ws_f32",
    "rayen_bwd_workspace_bytes_f64", "rayen_ray_project_bwd_ws_f64", "rayen_last_forward_kernel",
    "rayen_pair_schedule", "rayen_reserve_cus",
    "rayen_products_rows", "rayen_products_served", "rayen_ray_project_from_products_f32", "rayen_ray_project_from_products_f64",
    "rayen_ray_project_bwd_coefficients_f32", "rayen_ray_project_bwd_coefficients_f64",
    "rayen_bar_pack_create", "rayen_bar_pack_destroy", "rayen_bar_forward_f32", "rayen_bar_forward_f64",
    "rayen_bar_backward_f32", "rayen_bar_backward_f64",
    "rayen_dc3_pack_create", "rayen_dc3_pack_destroy", "rayen_dc3_workspace_bytes", "rayen_dc3_forward_f32",
    "rayen_dc3_forward_f64", "rayen_dc3_backward_f32", "rayen_dc3_backward_f64",
    "rayen_proj_pack_create", "rayen_proj_pack_set_psd", "rayen_proj_pack_destroy", "rayen_proj_workspace_bytes", "rayen_proj_forward_f32",
    "rayen_proj_forward_f64", "rayen_proj_backward_f32", "rayen_proj_backward_f64",
    "rayen_cost_pack_create", "rayen_cost_pack_set_lmi", "rayen_cost_pack_destroy", "rayen_cost_served", "rayen_soft_cost_f32", "rayen_soft_cost_f64",
    "rayen_pair_screen", "rayen_pair_screen_counters", "rayen_pair_drain",
)
# ABI v15, declared in include/rayen_hip_tile.h (which rayen_hip.h includes); tests/test_proj_tile_host.py holds the two
# against each other
EXPORTS_TILE = ("rayen_proj_tile_layout", "rayen_proj_tile_served", "rayen_proj_tile_workspace_bytes",
                "rayen_proj_tile_forward_f32", "rayen_proj_tile_backward_f32")
# additive to ABI v15, declared in include/rayen_hip_tile64.h (which rayen_hip.h includes): the fp64 twins on tiles of 16
# samples; tests/test_proj_tile64_host.py holds the two against each other
EXPORTS_TILE64 = ("rayen_proj_tile64_layout", "rayen_proj_tile64_pack_set", "rayen_proj_tile64_served",
                  "rayen_proj_tile64_workspace_bytes", "rayen_proj_tile64_forward_f64", "rayen_proj_tile64_backward_f64")
# additive to ABI v15, declared in include/rayen_hip_dc3_tile.h (which rayen_hip.h includes, like rayen_hip_tile.h);
# tests/test_dc3_tile_host.py holds the two against each other
EXPORTS_DC3_TILE = ("rayen_dc3_tile_shape_served", "rayen_dc3_tile_pack_set", "rayen_dc3_tile_served",
                    "rayen_dc3_tile_workspace_bytes", "rayen_dc3_tile_forward_f32", "rayen_dc3_tile_backward_f32")
# additive to ABI v15, declared in include/rayen_hip_dc3_tile64.h (which rayen_hip.h includes): the fp64 twins of the six
# above; tests/test_dc3_tile64_host.py holds the two against each other
EXPORTS_DC3_TILE64 = ("rayen_dc3_tile64_shape_served", "rayen_dc3_tile64_pack_set", "rayen_dc3_tile64_served",
                      "rayen_dc3_tile64_workspace_bytes", "rayen_dc3_tile64_forward_f64", "rayen_dc3_tile64_backward_f64")
# additive to ABI v15, declared in include/rayen_hip_cost_stream.h (which rayen_hip.h includes, like the two above);
# tests/test_cost_stream_host.py holds the two against each other
EXPORTS_COST_STREAM = ("rayen_cost_stream_set", "rayen_cost_stream_served", "rayen_soft_cost_stream_f32",
                       "rayen_soft_cost_stream_f64")
# additive to ABI v15, declared in include/rayen_hip_bar_stream.h (which rayen_hip.h includes, like the three above);
# tests/test_bar_stream_host.py holds the two against each other
EXPORTS_BAR_STREAM = ("rayen_bar_resident_served", "rayen_bar_stream_forward_f32", "rayen_bar_stream_forward_f64",
                      "rayen_bar_stream_backward_f32", "rayen_bar_stream_backward_f64")
# additive to ABI v15, declared in include/rayen_hip_wide_fused.h (which rayen_hip.h includes, like the four above);
# tests/test_wide_fused_host.py holds the two against each other
EXPORTS_WIDE_FUSED = ("rayen_wide_fused_served", "rayen_ray_project_wide_fused_f32")
# additive to ABI v15, declared in include/rayen_hip_wide_fused_bwd.h (which rayen_hip.h includes, like the five above);
# tests/test_wide_fused_bwd_host.py holds the two against each other
EXPORTS_WIDE_FUSED_BWD = ("rayen_wide_fused_bwd_served", "rayen_wide_fused_bwd_workspace_bytes",
                          "rayen_ray_project_wide_fused_bwd_f32")
# additive to ABI v15, declared in include/rayen_hip_wide_fused64.h (which rayen_hip.h includes, like the six above);
# tests/test_wide_fused64_host.py holds the two against each other
EXPORTS_WIDE_FUSED64 = ("rayen_wide_fused64_served", "rayen_wide_fused64_plan", "rayen_ray_project_wide_fused64_f64")
# additive to ABI v15, declared in include/rayen_hip_wide_fused_bwd64.h (which rayen_hip.h includes, like the seven above);
# tests/test_wide_fused_bwd64_host.py holds the two against each other
EXPORTS_WIDE_FUSED_BWD64 = ("rayen_wide_fused_bwd64_served", "rayen_wide_fused_bwd64_plan",
                            "rayen_wide_fused_bwd64_workspace_bytes", "rayen_ray_project_wide_fused_bwd_f64")
# additive to ABI v15, declared in include/rayen_hip_cost_tile64.h (which rayen_hip.h includes, like the eight above);
# tests/test_cost_tile64_host.py holds the two against each other
EXPORTS_COST_TILE64 = ("rayen_cost_tile64_set", "rayen_cost_tile64_served", "rayen_soft_cost_tile64_f64")
# additive to ABI v15, declared in include/rayen_hip_mapped64.h (which rayen_hip.h includes, like the nine above);
# tests/test_mapped64_host.py holds the two against each other
EXPORTS_MAPPED64 = ("rayen_mapper_fusable_f64", "rayen_ray_project_mapped_f64")
KERNEL_NONE, KERNEL_LANE, KERNEL_MFMA, KERNEL_TRIPLE, KERNEL_PAIR, KERNEL_PAIR_IO, KERNEL_LMI_QUAD, KERNEL_LMI_WAVE, KERNEL_PAIR_WS, KERNEL_PRODUCTS, KERNEL_LMI_BLOCK, KERNEL_PAIR_WL = range(12)
KERNEL_WIDE_FUSED = 12
KERNEL_WIDE_FUSED64 = 13


class RayenSegment(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("row0", ctypes.c_int32), ("nrows", ctypes.c_int32),
                ("aux_row", ctypes.c_int32), ("dim", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("f0", ctypes.c_double), ("f1", ctypes.c_double)]


class RayenPackDesc(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("k", ctypes.c_int32), ("n", ctypes.c_int32),
                ("n_rows", ctypes.c_int32), ("n_segments", ctypes.c_int32),
                ("out_identity", ctypes.c_int32),
                ("W", ctypes.POINTER(ctypes.c_double)),
                ("segments", ctypes.POINTER(RayenSegment)),
                ("NA_E", ctypes.POINTER(ctypes.c_double)),
                ("y0", ctypes.POINTER(ctypes.c_double)),
                ("prepare", ctypes.c_int32), ("fp32_mode", ctypes.c_int32)]


class RayenPackInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("n", ctypes.c_int32), ("n_rows", ctypes.c_int32),
                ("n_segments", ctypes.c_int32), ("device", ctypes.c_int32),
                ("mfma_f32", ctypes.c_int32), ("generic_block", ctypes.c_int32),
                ("mfma_f64", ctypes.c_int32), ("device_bytes", ctypes.c_int64),
                ("prepared", ctypes.c_int32), ("bwd_f32", ctypes.c_int32),
                ("fp32_check_split", ctypes.c_double), ("fp32_check_exact", ctypes.c_double),
                ("fp32_check_pair", ctypes.c_double),
                ("bwd32_check_pair", ctypes.c_double), ("bwd32_check_exact", ctypes.c_double)]


class RayenError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed with code {code}: {strerror(code)}")
        self.code = code


_lib = None


def library_path():
    return LIBRARY


def load():
    """Load ``librayen_hip.so`` (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBRARY):
        raise RuntimeError(
            f"{LIBRARY} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). Tensors on a HIP device are never routed anywhere else.")
    lib = ctypes.CDLL(LIBRARY)
    p, i64, i32p = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p
    lib.rayen_abi_version.restype = ctypes.c_int
    lib.rayen_abi_version.argtypes = []
    lib.rayen_last_forward_kernel.restype = ctypes.c_int
    lib.rayen_last_forward_kernel.argtypes = []
    lib.rayen_pair_schedule.restype = ctypes.c_int
    lib.rayen_pair_schedule.argtypes = [ctypes.c_int]
    # (mode: 1 spectral test and leading-product probe (default) | 2 spectral test only | 0 off | anything else queries)
    lib.rayen_pair_screen.restype = ctypes.c_int
    lib.rayen_pair_screen.argtypes = [ctypes.c_int]
    lib.rayen_pair_screen_counters.restype = ctypes.c_int
    lib.rayen_pair_screen_counters.argtypes = [ctypes.c_void_p]
    # (mode: 1 progress-ordered issue priority in schedule 3 | 0 off (default) | anything else queries)
    lib.rayen_pair_drain.restype = ctypes.c_int
    lib.rayen_pair_drain.argtypes = [ctypes.c_int]
    lib.rayen_reserve_cus.restype = ctypes.c_int
    lib.rayen_reserve_cus.argtypes = [ctypes.c_int]
    lib.rayen_strerror.restype = ctypes.c_char_p
    lib.rayen_strerror.argtypes = [ctypes.c_int]
    lib.rayen_pack_create.restype = ctypes.c_int
    lib.rayen_pack_create.argtypes = [ctypes.POINTER(RayenPackDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.rayen_pack_destroy.restype = None
    lib.rayen_pack_destroy.argtypes = [p]
    lib.rayen_pack_info.restype = ctypes.c_int
    lib.rayen_pack_info.argtypes = [p, ctypes.POINTER(RayenPackInfo)]
    fwd = [p, p, i64, i64, p, i64, p, i32p, i32p, p]
    for name in ("rayen_ray_project_f32", "rayen_ray_project_f64", "rayen_ray_project_generic_f32",
                 "rayen_ray_project_generic_f64", "rayen_ray_project_old_f32", "rayen_ray_project_old_f64",
                 "rayen_ray_project_wide_fused_f32"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = fwd
    for name in ("rayen_ray_project_from_products_f32", "rayen_ray_project_from_products_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, p, i64, i64, p, i64, p, i32p, i32p, p]
    for name in ("rayen_ray_project_bwd_coefficients_f32", "rayen_ray_project_bwd_coefficients_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, p, i64, i64, p, i32p, p, i64, p, i64, p, p]
    lib.rayen_wide_fused_served.restype = ctypes.c_int
    lib.rayen_wide_fused_served.argtypes = [p, ctypes.c_int32]
    lib.rayen_wide_fused64_served.restype = ctypes.c_int
    lib.rayen_wide_fused64_served.argtypes = [p]
    lib.rayen_wide_fused64_plan.restype = ctypes.c_int
    lib.rayen_wide_fused64_plan.argtypes = [p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    lib.rayen_ray_project_wide_fused64_f64.restype = ctypes.c_int
    lib.rayen_ray_project_wide_fused64_f64.argtypes = [p, p, i64, i64, p, i64, p, i32p, i32p, ctypes.c_int32, p]
    lib.rayen_wide_fused_bwd_served.restype = ctypes.c_int
    lib.rayen_wide_fused_bwd_served.argtypes = [p, ctypes.c_int32]
    lib.rayen_wide_fused_bwd_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_wide_fused_bwd_workspace_bytes.argtypes = [p, i64]
    lib.rayen_ray_project_wide_fused_bwd_f32.restype = ctypes.c_int
    lib.rayen_ray_project_wide_fused_bwd_f32.argtypes = [p, p, i64, i64, p, i32p, p, i64, p, i64, p, i64, p]
    lib.rayen_wide_fused_bwd64_served.restype = ctypes.c_int
    lib.rayen_wide_fused_bwd64_served.argtypes = [p]
    lib.rayen_wide_fused_bwd64_plan.restype = ctypes.c_int
    lib.rayen_wide_fused_bwd64_plan.argtypes = [p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    lib.rayen_wide_fused_bwd64_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_wide_fused_bwd64_workspace_bytes.argtypes = [p, i64]
    lib.rayen_ray_project_wide_fused_bwd_f64.restype = ctypes.c_int
    lib.rayen_ray_project_wide_fused_bwd_f64.argtypes = [p, p, i64, i64, p, i32p, p, i64, p, i64, p, i64, ctypes.c_int32, p]
    lib.rayen_products_rows.restype = ctypes.c_int64
    lib.rayen_products_rows.argtypes = [p]
    lib.rayen_products_served.restype = ctypes.c_int
    lib.rayen_products_served.argtypes = [p, ctypes.c_int]
    bwd = [p, p, i64, i64, p, i32p, p, i64, p, i64, p]
    for name in ("rayen_ray_project_bwd_f32", "rayen_ray_project_bwd_f64", "rayen_ray_project_bwd_generic_f32",
                 "rayen_ray_project_bwd_generic_f64",
                 "rayen_ray_project_old_bwd_f32", "rayen_ray_project_old_bwd_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = bwd
    lib.rayen_mapper_fusable.restype = ctypes.c_int
    lib.rayen_mapper_fusable.argtypes = [p, ctypes.c_int32]
    lib.rayen_ray_project_mapped_f32.restype = ctypes.c_int
    lib.rayen_ray_project_mapped_f32.argtypes = [p, p, i64, i64, ctypes.c_int32, p, i64, p, p, i64, p, i64,
                                                 p, i32p, i32p, p]
    lib.rayen_mapper_fusable_f64.restype = ctypes.c_int
    lib.rayen_mapper_fusable_f64.argtypes = [p, ctypes.c_int32]
    lib.rayen_ray_project_mapped_f64.restype = ctypes.c_int
    lib.rayen_ray_project_mapped_f64.argtypes = [p, p, i64, i64, ctypes.c_int32, p, i64, p, p, i64, p, i64,
                                                 p, i32p, i32p, p]
    for name in ("rayen_bwd_workspace_bytes_f32", "rayen_bwd_workspace_bytes_f64"):
        getattr(lib, name).restype = ctypes.c_int64
        getattr(lib, name).argtypes = [p, i64]
    for name in ("rayen_ray_project_bwd_ws_f32", "rayen_ray_project_bwd_ws_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i32p, p, i64, p, i64, p, i64, p]
    lib.rayen_mapper_image_bytes.restype = ctypes.c_int64
    lib.rayen_mapper_image_bytes.argtypes = [p, ctypes.c_int32]
    lib.rayen_mapper_prepare_f32.restype = ctypes.c_int
    lib.rayen_mapper_prepare_f32.argtypes = [p, p, i64, ctypes.c_int32, p, p, p]
    lib.rayen_ray_project_mapped_image_f32.restype = ctypes.c_int
    lib.rayen_ray_project_mapped_image_f32.argtypes = [p, p, i64, i64, ctypes.c_int32, p, p, i64, p, i64,
                                                       p, i32p, i32p, p]
    lib.rayen_bar_pack_create.restype = ctypes.c_int
    lib.rayen_bar_pack_create.argtypes = [p, p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(ctypes.c_void_p)]
    lib.rayen_bar_pack_destroy.restype = None
    lib.rayen_bar_pack_destroy.argtypes = [p]
    for name in ("rayen_bar_forward_f32", "rayen_bar_forward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i64, p, i32p, p]
    for name in ("rayen_bar_backward_f32", "rayen_bar_backward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, p, p, i64, p, p]
    lib.rayen_bar_resident_served.restype = ctypes.c_int
    lib.rayen_bar_resident_served.argtypes = [p, ctypes.c_int32]
    for name in ("rayen_bar_stream_forward_f32", "rayen_bar_stream_forward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i64, p, i32p, i64, p]
    for name in ("rayen_bar_stream_backward_f32", "rayen_bar_stream_backward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, p, p, i64, p, i64, p]
    i32, f64 = ctypes.c_int32, ctypes.c_double
    lib.rayen_dc3_pack_create.restype = ctypes.c_int
    lib.rayen_dc3_pack_create.argtypes = [p, p, i32, p, p, p, i32, p, p, p, p, i32, i32, ctypes.POINTER(ctypes.c_void_p)]
    lib.rayen_dc3_pack_destroy.restype = None
    lib.rayen_dc3_pack_destroy.argtypes = [p]
    lib.rayen_dc3_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_dc3_workspace_bytes.argtypes = [p, i64, i32, i32, i32]
    for name in ("rayen_dc3_forward_f32", "rayen_dc3_forward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i64, f64, f64, f64, i32, i32p, p, i64, i32p, p]
    for name in ("rayen_dc3_backward_f32", "rayen_dc3_backward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i64, p, i64, f64, f64, i32, i32p, p, i64, p]
    for tile, dt in (("tile", "f32"), ("tile64", "f64")):           # the twin entry points of the two DC3 tile geometries
        for name, restype, argtypes in (
                ("shape_served", ctypes.c_int, [i32, i32, i32, i32]),
                ("pack_set", ctypes.c_int, [p, p, p, p, p, p, p, p]),
                ("served", ctypes.c_int, [p]),
                ("workspace_bytes", ctypes.c_int64, [p, i64, i32, i32]),
                ("forward_" + dt, ctypes.c_int, [p, p, i64, i64, p, i64, f64, f64, f64, i32, i32p, p, i64, i32p, p]),
                ("backward_" + dt, ctypes.c_int, [p, p, i64, i64, p, i64, p, i64, f64, f64, i32, i32p, p, i64, p])):
            fn = getattr(lib, f"rayen_dc3_{tile}_{name}")
            fn.restype, fn.argtypes = restype, argtypes
    lib.rayen_proj_pack_create.restype = ctypes.c_int
    lib.rayen_proj_pack_create.argtypes = [p, p, p, p, i32, i32, i32, p, i32, f64, f64, f64, ctypes.POINTER(ctypes.c_void_p)]
    lib.rayen_proj_pack_set_psd.restype = ctypes.c_int
    lib.rayen_proj_pack_set_psd.argtypes = [p, i32, i32]
    lib.rayen_proj_pack_destroy.restype = None
    lib.rayen_proj_pack_destroy.argtypes = [p]
    lib.rayen_proj_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_proj_workspace_bytes.argtypes = [p, i64, i32, i32]
    for name in ("rayen_proj_forward_f32", "rayen_proj_forward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i64, i32p, p, f64, i32, p, i64, p]
    for name in ("rayen_proj_backward_f32", "rayen_proj_backward_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, i32p, p, i64, f64, i32, p, i64, p]
    lib.rayen_proj_tile_layout.restype = ctypes.c_int
    lib.rayen_proj_tile_layout.argtypes = [i32, p, i32, i32p, p, p]
    lib.rayen_proj_tile_served.restype = ctypes.c_int
    lib.rayen_proj_tile_served.argtypes = [p]
    lib.rayen_proj_tile_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_proj_tile_workspace_bytes.argtypes = [p, i64, i32]
    lib.rayen_proj_tile_forward_f32.restype = ctypes.c_int
    lib.rayen_proj_tile_forward_f32.argtypes = [p, p, i64, i64, p, i64, i32p, p, f64, i32, p, i64, p]
    lib.rayen_proj_tile_backward_f32.restype = ctypes.c_int
    lib.rayen_proj_tile_backward_f32.argtypes = [p, p, i64, i64, p, i32p, p, i64, f64, i32, p, i64, p]
    lib.rayen_proj_tile64_layout.restype = ctypes.c_int
    lib.rayen_proj_tile64_layout.argtypes = [i32, i32, p, i32, i32p, p, p, p]
    lib.rayen_proj_tile64_pack_set.restype = ctypes.c_int
    lib.rayen_proj_tile64_pack_set.argtypes = [p, p, p, p, p, p, i32]
    lib.rayen_proj_tile64_served.restype = ctypes.c_int
    lib.rayen_proj_tile64_served.argtypes = [p]
    lib.rayen_proj_tile64_workspace_bytes.restype = ctypes.c_int64
    lib.rayen_proj_tile64_workspace_bytes.argtypes = [p, i64, i32]
    lib.rayen_proj_tile64_forward_f64.restype = ctypes.c_int
    lib.rayen_proj_tile64_forward_f64.argtypes = [p, p, i64, i64, p, i64, i32p, p, f64, i32, p, i64, p]
    lib.rayen_proj_tile64_backward_f64.restype = ctypes.c_int
    lib.rayen_proj_tile64_backward_f64.argtypes = [p, p, i64, i64, p, i32p, p, i64, f64, i32, p, i64, p]
    lib.rayen_cost_pack_create.restype = ctypes.c_int
    lib.rayen_cost_pack_create.argtypes = [p, p, i32, p, p, p, i32, p, p, p, p, p, i32, p, p, i32, i32,
                                           ctypes.POINTER(ctypes.c_void_p)]
    lib.rayen_cost_pack_set_lmi.restype = ctypes.c_int
    lib.rayen_cost_pack_set_lmi.argtypes = [p, p, i32]
    lib.rayen_cost_pack_destroy.restype = None
    lib.rayen_cost_pack_destroy.argtypes = [p]
    lib.rayen_cost_served.restype = ctypes.c_int
    lib.rayen_cost_served.argtypes = [p, i32]
    for name in ("rayen_soft_cost_f32", "rayen_soft_cost_f64", "rayen_soft_cost_stream_f32", "rayen_soft_cost_stream_f64",
                 "rayen_soft_cost_tile64_f64"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [p, p, i64, i64, p, p, i32p, p, i64, p]
    lib.rayen_cost_stream_set.restype = ctypes.c_int
    lib.rayen_cost_stream_set.argtypes = [p, i64]
    lib.rayen_cost_stream_served.restype = ctypes.c_int
    lib.rayen_cost_stream_served.argtypes = [p, i32]
    lib.rayen_cost_tile64_set.restype = ctypes.c_int
    lib.rayen_cost_tile64_set.argtypes = [p, i64]
    lib.rayen_cost_tile64_served.restype = ctypes.c_int
    lib.rayen_cost_tile64_served.argtypes = [p]
    if lib.rayen_abi_version() != ABI_VERSION:
        raise RuntimeError(f"librayen_hip.so ABI {lib.rayen_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def strerror(code):
    return load().rayen_strerror(int(code)).decode()


def check(code, what):
    if code != 0:
        raise RayenError(code, what)
