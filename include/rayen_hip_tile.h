/*
 * rayen_hip_tile.h -- C ABI v15: the Euclidean projection on tiles of 32 samples (rayen_amd/csrc/rayen_proj_tile.hip).
 * Included by rayen_hip.h (which declares RayenProjPack and the error codes); not meant to be included alone.
 */
#ifndef RAYEN_HIP_TILE_H
#define RAYEN_HIP_TILE_H

/* The same projection as rayen_proj_forward_* / _backward_* on tiles of 32 samples on the matrix cores (rayen_proj_tile.hip), for programs beyond the
 * wave kernel's envelope: n <= 64, no PSD block, the rows -- re-laid into blocks of 32 dealt to four waves, a cone never
 * crossing two waves -- in at most 12 (n <= 32) or 10 (n > 32) blocks a wave, the cone blocks' images in LDS.  fp32 only.
 * rayen_proj_pack_create builds the tile images next to the wave kernel's wherever that envelope holds;
 * rayen_proj_tile_served says whether it did.  The rayen_proj_forward_* / _backward_* entries above never run the tile
 * kernel: they refuse exactly what they refused before.
 *
 * rayen_proj_tile_layout: the re-laying alone, pure host code (no device needed).  perm_out [Mp] (may be NULL; size it
 *   128 * 12): padded row -> original row, -1 for a pad (a zero orthant row); wave_first_block_out [5] (may be NULL): wave w
 *   owns blocks [w], [w + 1]) of 32 padded rows.  RAYEN_E_UNSUPPORTED: no layout of at most 12 blocks a wave holds the rows.
 * forward / backward: the argument lists, the contract and the results' layout of rayen_proj_forward_f32 /
 *   rayen_proj_backward_f32 -- vstar is [B, m] in the ORIGINAL row order, so a v* of either forward serves either
 *   backward -- with ws of at least rayen_proj_tile_workspace_bytes(pack, B, backward) bytes. */
int rayen_proj_tile_layout(int32_t m_lin, const int32_t* soc_rows, int32_t n_soc, int32_t* Mp, int32_t* perm_out,
                           int32_t* wave_first_block_out);
int rayen_proj_tile_served(const RayenProjPack* pack);
int64_t rayen_proj_tile_workspace_bytes(const RayenProjPack* pack, int64_t B, int32_t backward);
int rayen_proj_tile_forward_f32(const RayenProjPack* pack, const float* q, int64_t B, int64_t ldq, float* z, int64_t ldz,
                                int32_t* iters, float* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                                void* stream);
int rayen_proj_tile_backward_f32(const RayenProjPack* pack, const float* g, int64_t B, int64_t ldg, const float* vstar,
                                 const int32_t* iters, float* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                                 int64_t ws_bytes, void* stream);

#endif /* RAYEN_HIP_TILE_H */
