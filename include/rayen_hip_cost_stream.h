/*
 * rayen_hip_cost_stream.h -- C ABI v15 (additive): the soft cost of sets whose stacked rows do not fit LDS
 * (rayen_amd/csrc/rayen_cost_stream.hip).  Included by rayen_hip.h (which declares RayenCostPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_COST_STREAM_H
#define RAYEN_HIP_COST_STREAM_H

/* The outputs and the contract of rayen_soft_cost_* (rayen_hip.h), by a second route: the image of the stacked rows is cut
 * into windows (each a self-contained image in the resident layout; a quadratic or a cone is never split, a run of linear
 * or equality rows is split between tiles (fp32) or rows (fp64)) that a workgroup brings through LDS one after another,
 * two buffers, the next window's copy under the current one's walk.  The arithmetic per sample is the resident kernels',
 * in the same order: where both routes serve a set their results agree bit for bit.  Selected only by calling these entry
 * points: rayen_cost_served and rayen_soft_cost_* answer what they answered before.
 *
 * Served: k <= 64; fp32: cones of at most 64 rows; every item within one window; all windows together within 1 GiB.  A
 * set's LMI composes as in rayen_soft_cost_*: the rows' launch, then the LMI's on the same stream.
 *
 * rayen_cost_stream_set(pack, window_bytes): builds the stream images of both precisions from the arrays the pack was
 *   created from (the pack keeps them on the host when k <= 64) and uploads them to the pack's device, which must be
 *   current; not during stream capture.  window_bytes = 0: the default, 80 KiB (two buffers in the 160 KiB of LDS).  Any
 *   other value (for tests) must be a positive multiple of 16 up to the default, or RAYEN_E_BAD_ARG.  A window too small for
 *   the set's largest item leaves that precision unserved; that is not an error.  A further call with the same size
 *   returns RAYEN_OK without doing anything; with another size it replaces the images (after the launches that read them).
 * rayen_cost_stream_served(pack, f64): 1 when the streamed route serves the WHOLE set at the precision (rows and LMI);
 *   0 before rayen_cost_stream_set.
 * rayen_soft_cost_stream_f32 / _f64: arguments, results and error codes of rayen_soft_cost_f32 / _f64;
 *   RAYEN_E_UNSUPPORTED where rayen_cost_stream_served answers 0. */
int rayen_cost_stream_set(RayenCostPack* pack, int64_t window_bytes);
int rayen_cost_stream_served(const RayenCostPack* pack, int32_t f64);
int rayen_soft_cost_stream_f32(const RayenCostPack* pack, const float* y, int64_t B, int64_t ld, float* cost, float* worst,
                               int32_t* which, float* grad, int64_t ld_grad, void* stream);
int rayen_soft_cost_stream_f64(const RayenCostPack* pack, const double* y, int64_t B, int64_t ld, double* cost,
                               double* worst, int32_t* which, double* grad, int64_t ld_grad, void* stream);

#endif /* RAYEN_HIP_COST_STREAM_H */
