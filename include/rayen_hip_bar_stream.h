/*
 * rayen_hip_bar_stream.h -- C ABI v15 (additive): method='Bar' for packs whose image of G does not fit LDS
 * (rayen_amd/csrc/rayen_bar_stream.hip).  Included by rayen_hip.h (which declares RayenBarPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_BAR_STREAM_H
#define RAYEN_HIP_BAR_STREAM_H

/* The outputs and the contract of rayen_bar_forward_* / rayen_bar_backward_* (rayen_hip.h), by a second route: the pack's
 * image of G stays in global memory and a workgroup brings it through two LDS buffers in windows (whole groups of four
 * generators; the next window's copy is issued before the current one's walk) while its lanes keep their rows' sums in
 * registers.  The arithmetic per row is the resident kernels', in the same order: where both routes serve a pack their y,
 * rowstat and grad_q agree bit for bit.  Selected only by calling these entry points: rayen_bar_forward_* / _backward_*
 * answer what they answered before.  No LDS proportional to the set is needed: every pack that exists (k <= 64,
 * nv + nr >= 1) is served.  Like the resident route: any B >= 0, asynchronous on the stream, no allocation, the pack is not
 * changed, graph-capturable.
 *
 * rayen_bar_resident_served(pack, f64): 1 when rayen_bar_forward_* / rayen_bar_backward_* serve the pack at the precision
 *   (its image fits the 160 KiB of LDS), else 0.
 * rayen_bar_stream_forward_f32 / _f64, rayen_bar_stream_backward_f32 / _f64: the arguments of rayen_bar_forward_* /
 *   rayen_bar_backward_* and window_bytes in front of the stream.  window_bytes = 0: the default, 20 KiB (the fastest
 *   measured; a workgroup's LDS is two windows and 512 bytes for yp, so three workgroups fit a CU).  Any other value (for
 *   tests and measurements) must be a positive multiple of 16 up to the default and hold at least one group of four
 *   generators (16 K sizeof(T) bytes, K = k rounded up to 4, 8, 16, 32 or 64), or the call returns RAYEN_E_BAD_ARG and
 *   launches nothing.  A window is rounded down to whole groups. */
int rayen_bar_resident_served(const RayenBarPack* pack, int32_t f64);
int rayen_bar_stream_forward_f32(const RayenBarPack* pack, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                                 float* rowstat, int32_t* nan_flag, int64_t window_bytes, void* stream);
int rayen_bar_stream_forward_f64(const RayenBarPack* pack, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                                 double* rowstat, int32_t* nan_flag, int64_t window_bytes, void* stream);
int rayen_bar_stream_backward_f32(const RayenBarPack* pack, const float* q, int64_t ldq, const float* rowstat,
                                  const float* grad_y, int64_t B, float* grad_q, int64_t window_bytes, void* stream);
int rayen_bar_stream_backward_f64(const RayenBarPack* pack, const double* q, int64_t ldq, const double* rowstat,
                                  const double* grad_y, int64_t B, double* grad_q, int64_t window_bytes, void* stream);

#endif /* RAYEN_HIP_BAR_STREAM_H */
