/*
 * rayen_hip_wide_fused64.h -- C ABI v15 (additive): the fp64 forward of wide sets in one launch
 * (rayen_amd/csrc/rayen_wide_fused64.hip).  Included by rayen_hip.h (which declares RayenPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_WIDE_FUSED64_H
#define RAYEN_HIP_WIDE_FUSED64_H

/* The forward of rayen_ray_project_f64 for sets beyond the n the fp64 matrix-core kernel keeps in registers (n > 64),
 * WITHOUT the products matrix T = v W_ext' of the ABI v7 route: the fp64 twin of rayen_hip_wide_fused.h.  A workgroup owns
 * S consecutive rows of the batch (S = 32 where its LDS fits, else 16), stages them in LDS once, streams the rows of
 * W_ext = [W ; NA_E] past them in blocks of 16 on v_mfma_f64_16x16x4_f64 and reduces every block while its products are in
 * registers.  Exact fp64 arithmetic (another summation order than the GEMM's).  Selected only by calling this entry point;
 * every other entry runs what it ran before.
 *
 * rayen_wide_fused64_served(pack): 1 where the kernel serves the pack -- no LMI segment, 1 <= n <= 1024, and the S x n tile
 *   (padded) with the segments' per-sample scratch within 160 KiB - 256 B of LDS at S = 16
 *   (rayen_amd/csrc/rayen_wide_fused64_layout.h); pure host code.
 * rayen_wide_fused64_plan(pack, samples, out): the block plan for a tile of `samples` samples (0: the plan's own choice,
 *   16 or 32: forced) as thirteen integers -- n, kp, ks, samples, rows_w_pad, nb_w, rows_e_pad, nb_e, rows_pad,
 *   scratch_words (8-byte words), tile_bytes, lds_bytes, served; pure host code.  RAYEN_E_BAD_ARG for a null argument or
 *   another `samples`, RAYEN_E_UNSUPPORTED for a pack with an LMI (it has no plan).
 * rayen_ray_project_wide_fused64_f64: arguments, null-pointer rules (y, kappa, active, nan_flag optional; y == NULL
 *   computes kappa alone) and error codes of rayen_ray_project_f64, and `samples` as above: anything but 0, 16, 32 is
 *   RAYEN_E_BAD_ARG; a pack that is not served, or a forced 32 whose plan is beyond LDS, answers RAYEN_E_UNSUPPORTED.  The
 *   bits of a row do not depend on `samples`.  The FIRST call on a pack uploads the kernel's image of W_ext (rows padded
 *   to 16, fp64) -- it allocates and synchronises, and while `stream` is capturing it answers RAYEN_E_NOT_PREPARED
 *   instead: make one call before the capture.  Later calls are asynchronous and allocate nothing.  A pack that never calls
 *   this allocates nothing for it.  The image holds the set's own W: RAYEN_PREPARE_INWARD_BIAS does not enter.
 *   rayen_last_forward_kernel() answers RAYEN_KERNEL_WIDE_FUSED64 after it. */
int rayen_wide_fused64_served(const RayenPack* pack);
int rayen_wide_fused64_plan(const RayenPack* pack, int32_t samples, int64_t* out);
int rayen_ray_project_wide_fused64_f64(const RayenPack* pack, const double* v, int64_t B, int64_t ldv, double* y, int64_t ldy,
                                       double* kappa, int32_t* active, int32_t* nan_flag, int32_t samples, void* stream);

#endif /* RAYEN_HIP_WIDE_FUSED64_H */
