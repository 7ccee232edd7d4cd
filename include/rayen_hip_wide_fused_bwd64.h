/*
 * rayen_hip_wide_fused_bwd64.h -- C ABI v15 (additive): the fp64 backward of wide sets in one launch
 * (rayen_amd/csrc/rayen_wide_fused_bwd64.hip).  Included by rayen_hip.h (which declares RayenPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_WIDE_FUSED_BWD64_H
#define RAYEN_HIP_WIDE_FUSED_BWD64_H

/* The backward of rayen_ray_project_bwd_f64 for sets beyond the n the fp64 matrix-core kernels keep in registers (n > 64),
 * WITHOUT the products matrix T = v W_ext' and the coefficient matrix C of the ABI v7 route
 * (rayen_ray_project_bwd_coefficients_f64 between two GEMMs): the fp64 twin of rayen_hip_wide_fused_bwd.h.  A workgroup owns
 * S rows of the batch (S = 32 where its LDS fits, else 16) and multiplies only the rows of W that belong to the constraint
 * that set kappa for some of them, on v_mfma_f64_16x16x4_f64.  Exact fp64 arithmetic (another summation order than the
 * GEMMs').  It consumes kappa and active of ANY forward of the pack.  Selected only by calling this entry point.
 *
 * rayen_wide_fused_bwd64_served(pack): 1 where the kernel serves the pack -- no LMI segment, 1 <= n <= 1024, and at S = 16
 *   max(the S x k tile of grad_y when NA_E != I, the S x n tile of v + the S x r tile of the widest low-rank quadratic or
 *   cone) with the per-sample scratch within 160 KiB - 256 B of LDS (rayen_amd/csrc/rayen_wide_fused_bwd64_layout.h); pure
 *   host code.
 * rayen_wide_fused_bwd64_plan(pack, samples, out): the LDS plan for a tile of `samples` samples (0: the plan's own choice,
 *   16 or 32: forced) as eleven integers -- kp, ks, ke, gs, rp, ts, np, samples, region_words (8-byte words), lds_bytes,
 *   served; pure host code.  They are the pack's own plan (its widest low-rank quadratic or cone included) also where a
 *   shape condition of the segment table fails: then served and region_words are 0.  RAYEN_E_BAD_ARG for a null argument or another `samples`, RAYEN_E_UNSUPPORTED for a pack with
 *   an LMI (it has no plan).
 * rayen_wide_fused_bwd64_workspace_bytes(pack, B): bytes of device scratch with which the call groups the rows of the batch
 *   by active constraint before it deals them to workgroups (the layout of rayen_wide_fused_bwd_workspace_bytes: int32
 *   cursors and permutation); 0 for a pack with fewer than two non-linear segments, a pack that is not served, or B == 0.
 * rayen_ray_project_wide_fused_bwd_f64: v [B, ldv], kappa [B], active [B, 2] and grad_y [B, ldg] as for
 *   rayen_ray_project_bwd_f64; grad_v [B, ldgv] receives its first n columns.  `workspace` NULL or smaller than asked for:
 *   batch order (the same bits).  `samples` as above: anything but 0, 16, 32 is RAYEN_E_BAD_ARG; a pack that is not
 *   served, or a forced 32 whose plan is beyond LDS, answers RAYEN_E_UNSUPPORTED; B == 0 is RAYEN_OK.  A row's gradient bits
 *   depend on the pack and that row's inputs alone: not on `samples`, the workspace, B or the row's place in the batch.
 *   The FIRST call on a pack uploads the kernel's images (the forward's fp64 image of W_ext is shared where
 *   rayen_ray_project_wide_fused64_f64 has built it) -- it allocates and synchronises, and while `stream` is capturing it
 *   answers RAYEN_E_NOT_PREPARED instead: make one call before the capture.  Later calls are asynchronous and allocate
 *   nothing. */
int rayen_wide_fused_bwd64_served(const RayenPack* pack);
int rayen_wide_fused_bwd64_plan(const RayenPack* pack, int32_t samples, int64_t* out);
int64_t rayen_wide_fused_bwd64_workspace_bytes(const RayenPack* pack, int64_t B);
int rayen_ray_project_wide_fused_bwd_f64(const RayenPack* pack, const double* v, int64_t B, int64_t ldv, const double* kappa,
                                         const int32_t* active, const double* grad_y, int64_t ldg, double* grad_v, int64_t ldgv,
                                         void* workspace, int64_t workspace_bytes, int32_t samples, void* stream);

#endif /* RAYEN_HIP_WIDE_FUSED_BWD64_H */
