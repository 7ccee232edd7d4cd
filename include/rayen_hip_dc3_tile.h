/*
 * rayen_hip_dc3_tile.h -- C ABI v15 (additive): method='DC3' on tiles of 32 samples (rayen_amd/csrc/rayen_dc3_tile.hip).
 * Included by rayen_hip.h (which declares RayenDc3Pack and the error codes); not meant to be included alone.
 */
#ifndef RAYEN_HIP_DC3_TILE_H
#define RAYEN_HIP_DC3_TILE_H

/* The iteration, stop rule and contract of rayen_dc3_forward_* / _backward_* (rayen_hip.h)
 * for sets whose image does not fit LDS.  A workgroup owns 32 consecutive rows of the batch as the columns of fp32 MFMA
 * products; the operand images (A1e by 32-row blocks, the same blocks transposed, Pe_i and Pe_i' padded to whole blocks, C)
 * are streamed from device memory.  fp32 only; exact fp32 arithmetic (another summation order than the lane kernels').
 * Selected only by calling these entry points: rayen_dc3_forward_* / _backward_* run what they ran before.
 *
 * rayen_dc3_tile_shape_served(n, m, nq, no): 1 where the tile kernels serve a set of n <= 64 variables, m effective rows, nq
 *   quadratics and no = k - n completed variables (1 <= n <= 64, m, nq, no >= 0, the image within 1 GiB: about
 *   8 (m + nq n + no) max(n, 32) bytes); pure host code, no device needed.  fp64 and n > 64 are not served.
 * rayen_dc3_tile_pack_set(pack, ..): uploads the tile image of the arrays the pack was created from (the caller passes them
 *   again: the pack keeps no host copy) on the pack's device, which must be current; once per pack (further calls return
 *   RAYEN_OK without reading), not during stream capture.  A shape that is not served gets no image and RAYEN_OK.
 * rayen_dc3_tile_served(pack): 1 once the pack holds a tile image.  Without one the two calls answer RAYEN_E_UNSUPPORTED.
 * rayen_dc3_tile_workspace_bytes(pack, B, max_steps, backward): the scratch of a call (forward: the violations and, beyond
 *   32 steps, (p, s) of every 32-row tile twice; backward: the trajectory [max_steps][tiles][32 or 64][32]); -1 on bad
 *   arguments.
 * rayen_dc3_tile_forward_f32 / _backward_f32: arguments, results and error codes of rayen_dc3_forward_f32 /
 *   rayen_dc3_backward_f32, with ws sized by rayen_dc3_tile_workspace_bytes.  *tstar of either forward may be handed to
 *   either backward. */
int rayen_dc3_tile_shape_served(int32_t n, int32_t m, int32_t nq, int32_t no);
int rayen_dc3_tile_pack_set(RayenDc3Pack* pack, const double* A1e, const double* b1e, const double* Pe, const double* qe,
                            const double* re, const double* C, const double* c0);
int rayen_dc3_tile_served(const RayenDc3Pack* pack);
int64_t rayen_dc3_tile_workspace_bytes(const RayenDc3Pack* pack, int64_t B, int32_t max_steps, int32_t backward);
int rayen_dc3_tile_forward_f32(const RayenDc3Pack* pack, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                               double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                               int64_t ws_bytes, int32_t* nan_flag, void* stream);
int rayen_dc3_tile_backward_f32(const RayenDc3Pack* pack, const float* q, int64_t B, int64_t ldq, const float* grad_y,
                                int64_t ldg, float* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                                const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream);

#endif /* RAYEN_HIP_DC3_TILE_H */
