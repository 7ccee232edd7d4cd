/*
 * rayen_hip_dc3_tile64.h -- C ABI v15 (additive): method='DC3' in fp64 on tiles of 16 samples
 * (rayen_amd/csrc/rayen_dc3_tile64.hip).  Included by rayen_hip.h (which declares RayenDc3Pack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_DC3_TILE64_H
#define RAYEN_HIP_DC3_TILE64_H

/* The iteration, stop rule and contract of rayen_dc3_forward_f64 / rayen_dc3_backward_f64 (rayen_hip.h) for fp64 inputs on
 * sets the fp64 lane kernel does not stage (more than 32 variables, or an fp64 image beyond LDS).  A workgroup owns 16
 * consecutive rows of the batch as the columns of v_mfma_f64_16x16x4_f64 products; the operand images (A1e by 16-row blocks,
 * the same blocks transposed, Pe_i and Pe_i' padded to whole blocks, C) are streamed from device memory.  fp64 only; exact
 * fp64 arithmetic (another summation order than the lane kernel's); lr, momentum and eps are used as doubles.  A row's bits
 * depend on the set and on that row alone, never on the batch it came in.  Selected only by calling these entry points:
 * rayen_dc3_forward_* / _backward_* and rayen_dc3_tile_* (fp32 only) run what they ran before.
 *
 * rayen_dc3_tile64_shape_served(n, m, nq, no): 1 where these kernels serve a set of n variables, m effective rows, nq
 *   quadratics and no = k - n completed variables (1 <= n <= 64, m, nq, no >= 0, the image within 1 GiB: about
 *   16 (m + nq n + no) ceil16(n) bytes); pure host code, no device needed.  n > 64 is not served.
 * rayen_dc3_tile64_pack_set(pack, ..): uploads the fp64 tile image of the arrays the pack was created from (the caller
 *   passes them again: the pack keeps no host copy) on the pack's device, which must be current; once per pack (further
 *   calls return RAYEN_OK without reading), not during stream capture.  A shape that is not served gets no image and
 *   RAYEN_OK.  Independent of rayen_dc3_tile_pack_set: a pack may hold either image, both or none.
 * rayen_dc3_tile64_served(pack): 1 once the pack holds an fp64 tile image.  Without one the two calls answer
 *   RAYEN_E_UNSUPPORTED.
 * rayen_dc3_tile64_workspace_bytes(pack, B, max_steps, backward): the scratch of a call (forward: the violations, 8 bytes a
 *   step, and, beyond 32 steps, (p, s) of every 16-row tile twice; backward: the trajectory
 *   [max_steps][tiles][16 ceil(n / 16)][16] doubles); -1 on bad arguments.
 * rayen_dc3_tile64_forward_f64 / _backward_f64: arguments, results and error codes of rayen_dc3_forward_f64 /
 *   rayen_dc3_backward_f64, with ws sized by rayen_dc3_tile64_workspace_bytes.  *tstar of any fp64 forward may be handed to
 *   any fp64 backward. */
int rayen_dc3_tile64_shape_served(int32_t n, int32_t m, int32_t nq, int32_t no);
int rayen_dc3_tile64_pack_set(RayenDc3Pack* pack, const double* A1e, const double* b1e, const double* Pe, const double* qe,
                              const double* re, const double* C, const double* c0);
int rayen_dc3_tile64_served(const RayenDc3Pack* pack);
int64_t rayen_dc3_tile64_workspace_bytes(const RayenDc3Pack* pack, int64_t B, int32_t max_steps, int32_t backward);
int rayen_dc3_tile64_forward_f64(const RayenDc3Pack* pack, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                                 double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                                 int64_t ws_bytes, int32_t* nan_flag, void* stream);
int rayen_dc3_tile64_backward_f64(const RayenDc3Pack* pack, const double* q, int64_t B, int64_t ldq, const double* grad_y,
                                  int64_t ldg, double* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                                  const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream);

#endif /* RAYEN_HIP_DC3_TILE64_H */
