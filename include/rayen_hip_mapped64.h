/*
 * rayen_hip_mapped64.h -- C ABI v15 (additive): the module's mapper v = Wm x + b in front of the fp64 matrix-core forward,
 * one launch (the MAPPED instances of rayen_amd/csrc/rayen_mfma_f64.hip).  Included by rayen_hip.h (which declares RayenPack
 * and the error codes); not meant to be included alone.
 */
#ifndef RAYEN_HIP_MAPPED64_H
#define RAYEN_HIP_MAPPED64_H

/* y = project(Wm x + b) in fp64: the fp64 twin of rayen_ray_project_mapped_f32.  v = b + Wm x is formed on
 * v_mfma_f64_16x16x4_f64 into the registers the constraint walk reads its direction from, so v reaches memory only when the
 * caller asks for it (v_out, for the backward).  Exact fp64 arithmetic, in another summation order than a library GEMM's.
 *
 * rayen_mapper_fusable_f64(pack, in_dim): 1 where rayen_ray_project_mapped_f64 serves the pack behind an in_dim-wide
 *   mapper -- the packs the fp64 matrix-core forward serves (RayenPackInfo.mfma_f64: n <= 64, no LMI) and
 *   1 <= in_dim <= 512 -- else 0 (a null pack included).
 * rayen_ray_project_mapped_f64: x [B, ldx] (ldx >= in_dim), Wm [n, ldw] row-major (= Linear.weight, read in place with
 *   8-byte loads: any ldw >= in_dim, no alignment beyond a double's; nothing is cached, so weights an optimiser has stepped
 *   are simply read again), bias [n] or NULL, v_out [B, ldvo] (ldvo >= n) or NULL -- columns at or beyond n are not
 *   written.  y, kappa, active, nan_flag as for rayen_ray_project_f64 (y required); their bits are those of
 *   rayen_ray_project_f64 on the v this call forms.  RAYEN_E_BAD_ARG for a null pack / Wm / y, B < 0, in_dim <= 0,
 *   ldx < in_dim, ldw < in_dim, ldy < k, x == NULL with B > 0, or v_out with ldvo < n; RAYEN_E_UNSUPPORTED wherever
 *   rayen_mapper_fusable_f64 answers 0; B == 0 is RAYEN_OK.  Asynchronous on `stream`, allocates nothing, safe under
 *   stream capture.  rayen_last_forward_kernel() answers RAYEN_KERNEL_MFMA after it. */
int rayen_mapper_fusable_f64(const RayenPack* pack, int32_t in_dim);
int rayen_ray_project_mapped_f64(const RayenPack* pack, const double* x, int64_t B, int64_t ldx, int32_t in_dim,
                                 const double* Wm, int64_t ldw, const double* bias, double* v_out, int64_t ldvo,
                                 double* y, int64_t ldy, double* kappa, int32_t* active, int32_t* nan_flag, void* stream);

#endif /* RAYEN_HIP_MAPPED64_H */
