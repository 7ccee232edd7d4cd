/*
 * rayen_hip_tile64.h -- C ABI v15 (additive): the Euclidean projection in fp64 on tiles of 16 samples
 * (rayen_amd/csrc/rayen_proj_tile64.hip).  Included by rayen_hip.h (which declares RayenProjPack and the error codes); not
 * meant to be included alone.
 */
#ifndef RAYEN_HIP_TILE64_H
#define RAYEN_HIP_TILE64_H

/* The iteration, stop rule and contract of rayen_proj_forward_f64 / rayen_proj_backward_f64 (rayen_hip.h) for fp64 inputs
 * on programs beyond the fp64 wave kernel's envelope.  A workgroup owns 16 consecutive rows of the batch as the columns of
 * v_mfma_f64_16x16x4_f64 products; the operand images are streamed from device memory.  fp64 only; exact fp64 arithmetic
 * (another summation order than the wave kernel's); rho, sigma, alpha and eps are used as doubles.  A row's bits depend on
 * the set and on that row alone, never on the batch it came in.  Selected only by calling these entry points:
 * rayen_proj_forward_* / _backward_* and rayen_proj_tile_* (fp32 only) run and refuse what they did before.
 *
 * Envelope: 1 <= n <= 64, no PSD block, the rows -- re-laid into blocks of 16 dealt to four waves, a cone never crossing two
 * waves -- in at most 24 (n <= 32) or 20 (n > 32) blocks a wave (1 536 / 1 280 padded rows), at most 4 096 cones, and the
 * backward's LDS (the cone blocks' images twice, 128 bytes a cone row each) within 160 KiB - 256.
 *
 * rayen_proj_tile64_layout: the envelope and the re-laying alone, pure host code (no device needed).  perm_out [Mp] (may be
 *   NULL; size it 1 536): padded row -> original row, -1 for a pad (a zero orthant row); wave_first_block_out [5] (may be
 *   NULL): wave w owns blocks [w], [w + 1]) of 16 padded rows; lds_bytes_out (may be NULL): the backward's dynamic LDS.
 *   RAYEN_E_UNSUPPORTED: the kernels do not serve a program of these sizes.
 * rayen_proj_tile64_pack_set(pack, ..): uploads the fp64 tile images of the arrays the pack was created from (the caller
 *   passes them again: the pack keeps no host copy) on the pack's device, which must be current; once per pack (further
 *   calls return RAYEN_OK without reading), not during stream capture.  A program that is not served, or a pack with a
 *   PSD block, gets no image and RAYEN_OK.
 * rayen_proj_tile64_served(pack): 1 once the pack holds the images.  Without them the two calls answer
 *   RAYEN_E_UNSUPPORTED.
 * forward / backward: the argument lists, the contract and the results' layout of rayen_proj_forward_f64 /
 *   rayen_proj_backward_f64 -- vstar is [B, m] in the ORIGINAL row order, so a v* of either fp64 forward serves either
 *   fp64 backward -- with ws of at least rayen_proj_tile64_workspace_bytes(pack, B, backward) bytes. */
int rayen_proj_tile64_layout(int32_t n, int32_t m_lin, const int32_t* soc_rows, int32_t n_soc, int32_t* Mp,
                             int32_t* perm_out, int32_t* wave_first_block_out, int64_t* lds_bytes_out);
int rayen_proj_tile64_pack_set(RayenProjPack* pack, const double* G, const double* h, const double* Kinv, const double* w0,
                               const int32_t* soc_rows, int32_t n_soc);
int rayen_proj_tile64_served(const RayenProjPack* pack);
int64_t rayen_proj_tile64_workspace_bytes(const RayenProjPack* pack, int64_t B, int32_t backward);
int rayen_proj_tile64_forward_f64(const RayenProjPack* pack, const double* q, int64_t B, int64_t ldq, double* z, int64_t ldz,
                                  int32_t* iters, double* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                                  void* stream);
int rayen_proj_tile64_backward_f64(const RayenProjPack* pack, const double* g, int64_t B, int64_t ldg, const double* vstar,
                                   const int32_t* iters, double* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                                   int64_t ws_bytes, void* stream);

#endif /* RAYEN_HIP_TILE64_H */
