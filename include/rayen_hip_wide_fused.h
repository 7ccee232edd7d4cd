/*
 * rayen_hip_wide_fused.h -- C ABI v15 (additive): the forward of wide sets in one launch (rayen_amd/csrc/rayen_wide_fused.hip).
 * Included by rayen_hip.h (which declares RayenPack and the error codes); not meant to be included alone.
 */
#ifndef RAYEN_HIP_WIDE_FUSED_H
#define RAYEN_HIP_WIDE_FUSED_H

/* The forward of rayen_ray_project_f32 for sets beyond the n the other matrix-core kernels keep in registers, WITHOUT the
 * products matrix T = v W_ext' of the ABI v7 route (rayen_ray_project_from_products_*): a workgroup owns 32 consecutive rows
 * of the batch, stages them in LDS once, streams the rows of W_ext = [W ; NA_E] past them in blocks of 32 on
 * v_mfma_f32_32x32x2_f32 and reduces every block while its products are in registers.  Exact fp32 arithmetic (another
 * summation order than the GEMM's).  Selected only by calling this entry point; every other entry runs what it ran before.
 *
 * rayen_wide_fused_served(pack, f64): 1 where the kernel serves the pack at that precision -- fp32 (f64 = 0) only, no LMI
 *   segment, n <= 1024, and the 32 x n tile (padded) with the segments' per-sample scratch within 160 KiB - 256 B of LDS
 *   (rayen_amd/csrc/rayen_wide_fused_layout.h); pure host code.  Any n >= 1 inside that is served: the caller decides where
 *   the route pays.
 * rayen_ray_project_wide_fused_f32: arguments, null-pointer rules (y, kappa, active, nan_flag optional; y == NULL computes
 *   kappa alone) and error codes of rayen_ray_project_f32; a pack that is not served answers RAYEN_E_UNSUPPORTED.  The FIRST
 *   call on a pack uploads the kernel's image of W_ext (rows padded to 32, fp32) -- it allocates and synchronises, and while
 *   `stream` is capturing it answers RAYEN_E_NOT_PREPARED instead: make one call before the capture.  Later calls are
 *   asynchronous and allocate nothing.  A pack that never calls this allocates nothing for it.  The image holds the set's
 *   own W: RAYEN_PREPARE_INWARD_BIAS does not enter (as on the products route, whose W_ext the caller builds).
 *   rayen_last_forward_kernel() answers RAYEN_KERNEL_WIDE_FUSED after it. */
int rayen_wide_fused_served(const RayenPack* pack, int32_t f64);
int rayen_ray_project_wide_fused_f32(const RayenPack* pack, const float* v, int64_t B, int64_t ldv, float* y, int64_t ldy,
                                     float* kappa, int32_t* active, int32_t* nan_flag, void* stream);

#endif /* RAYEN_HIP_WIDE_FUSED_H */
