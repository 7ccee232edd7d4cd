/*
 * rayen_hip_wide_fused_bwd.h -- C ABI v15 (additive): the backward of wide sets in one launch
 * (rayen_amd/csrc/rayen_wide_fused_bwd.hip).  Included by rayen_hip.h (which declares RayenPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_WIDE_FUSED_BWD_H
#define RAYEN_HIP_WIDE_FUSED_BWD_H

/* The backward of rayen_ray_project_bwd_f32 for sets beyond the n the other matrix-core kernels keep in registers, WITHOUT
 * the products matrix T = v W_ext' and the coefficient matrix C of the ABI v7 route (rayen_ray_project_bwd_coefficients_*
 * between two GEMMs): a workgroup owns 32 rows of the batch and multiplies only the rows of W that belong to the constraint
 * that set kappa for some of them, on v_mfma_f32_32x32x2_f32.  Exact fp32 arithmetic (another summation order than the
 * GEMMs').  It consumes kappa and active of ANY forward of the pack.  Selected only by calling this entry point.
 *
 * rayen_wide_fused_bwd_served(pack, f64): 1 where the kernel serves the pack at that precision -- fp32 (f64 = 0) only, no LMI
 *   segment, 1 <= n <= 1024, and max(the 32 x k tile of grad_y when NA_E != I, the 32 x n tile of v + the 32 x r tile of the
 *   widest low-rank quadratic or cone) with the per-sample scratch within 160 KiB - 256 B of LDS
 *   (rayen_amd/csrc/rayen_wide_fused_bwd_layout.h); pure host code.
 * rayen_wide_fused_bwd_workspace_bytes(pack, B): bytes of device scratch with which the call groups the rows of the batch by
 *   active constraint before it deals them to workgroups (a tile then walks one constraint's rows, not several); 0 for a
 *   pack with fewer than two non-linear segments, a pack that is not served, or B == 0.
 * rayen_ray_project_wide_fused_bwd_f32: v [B, ldv], kappa [B], active [B, 2] and grad_y [B, ldg] as for
 *   rayen_ray_project_bwd_f32; grad_v [B, ldgv] receives its first n columns.  `workspace` NULL or smaller than asked for:
 *   batch order (the same bits: a row's gradient depends on the pack and that row's inputs alone).  A pack that is not
 *   served answers RAYEN_E_UNSUPPORTED; B == 0 is RAYEN_OK.  The FIRST call on a pack uploads the kernel's images (the
 *   forward's image of W_ext is shared where rayen_ray_project_wide_fused_f32 has built it) -- it allocates and synchronises,
 *   and while `stream` is capturing it answers RAYEN_E_NOT_PREPARED instead: make one call before the capture.  Later calls
 *   are asynchronous and allocate nothing. */
int rayen_wide_fused_bwd_served(const RayenPack* pack, int32_t f64);
int64_t rayen_wide_fused_bwd_workspace_bytes(const RayenPack* pack, int64_t B);
int rayen_ray_project_wide_fused_bwd_f32(const RayenPack* pack, const float* v, int64_t B, int64_t ldv, const float* kappa,
                                         const int32_t* active, const float* grad_y, int64_t ldg, float* grad_v, int64_t ldgv,
                                         void* workspace, int64_t workspace_bytes, void* stream);

#endif /* RAYEN_HIP_WIDE_FUSED_BWD_H */
