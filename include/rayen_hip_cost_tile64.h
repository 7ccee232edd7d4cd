/*
 * rayen_hip_cost_tile64.h -- C ABI v15 (additive): the soft cost in fp64 on the fp64 matrix cores
 * (rayen_amd/csrc/rayen_cost_tile64.hip).  Included by rayen_hip.h (which declares RayenCostPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_COST_TILE64_H
#define RAYEN_HIP_COST_TILE64_H

/* The outputs and the contract of rayen_soft_cost_f64 (rayen_hip.h), by a third route: the stacked rows in blocks of 16 on
 * v_mfma_f64_16x16x4_f64, 32 samples per wave, the image brought through LDS in windows (two buffers, the next window's copy
 * under the current one's walk; a set of one window is copied once).  Exact fp64; a row's bits depend on the set and on that
 * row's input alone -- not on B, on the other rows, on the window size or on whether grad was asked for.  Against the lane
 * kernels of rayen_soft_cost_f64 / rayen_soft_cost_stream_f64 the differences are summation order.  Selected only by calling
 * these entry points: rayen_cost_served, rayen_cost_stream_served and their calls answer what they answered before.
 *
 * Served: fp64; 1 <= k <= 64; every item (a quadratic: ceil(k / 16) blocks; a cone: ceil(rows / 16) blocks) within one
 * window; the table and all windows together within 1 GiB.  A cone of any number of rows that fits a window is served.  A
 * set's LMI composes as in rayen_soft_cost_*: the rows' launch, then the LMI's on the same stream.  There is no fp32 entry
 * point.
 *
 * rayen_cost_tile64_set(pack, window_bytes): builds the image from the arrays the pack was created from (the pack keeps
 *   them on the host when k <= 64) and uploads it to the pack's device, which must be current; not during stream capture.
 *   window_bytes = 0: the default, 80 KiB (two buffers in the 160 KiB of LDS).  Any other value (for tests) must be a
 *   positive multiple of 16 up to the default, or RAYEN_E_BAD_ARG.  A window too small for the set's largest item leaves the
 *   set unserved; that is not an error.  A further call with the same size returns RAYEN_OK without doing anything; with
 *   another size it replaces the image (after the launches that read it).
 * rayen_cost_tile64_served(pack): 1 when the route serves the WHOLE set (rows and LMI); 0 before rayen_cost_tile64_set.
 * rayen_soft_cost_tile64_f64: arguments, results and error codes of rayen_soft_cost_f64; RAYEN_E_UNSUPPORTED where
 *   rayen_cost_tile64_served answers 0. */
int rayen_cost_tile64_set(RayenCostPack* pack, int64_t window_bytes);
int rayen_cost_tile64_served(const RayenCostPack* pack);
int rayen_soft_cost_tile64_f64(const RayenCostPack* pack, const double* y, int64_t B, int64_t ld, double* cost,
                               double* worst, int32_t* which, double* grad, int64_t ld_grad, void* stream);

#endif /* RAYEN_HIP_COST_TILE64_H */
