// RayenProjPack: what rayen_proj.hip (wave per sample, image in LDS) and rayen_proj_tile.hip (32 samples per workgroup
// on the matrix cores) share.  The wave kernel's fields are filled by rayen_proj_pack_create; the tile kernel's images
// hang off `tile` (null: the shape is outside tile_served(), or the set has a PSD block); the fp64 tile kernel's
// (rayen_proj_tile64.hip) off `tile64`, uploaded on request by rayen_proj_tile64_pack_set.
#pragma once

#include <cstdint>

#include "rayen_side_pack.h"

struct RayenProjTile;
struct RayenProjTile64;

namespace rayen {
constexpr int kProjMaxSoc = 32;               // cones the WAVE kernel's argument block holds
// rayen_proj_tile.hip: the tile images of a program (null: not served, or no memory), and their release
RayenProjTile* proj_tile_create(const double* G, const double* h, const double* Kinv, const double* w0, int n, int m,
                                int m_lin, const int32_t* soc_rows, int n_soc);
void proj_tile_destroy(RayenProjTile* t);
// rayen_proj_tile64.hip: the fp64 tile images of a program (null: not served, or no memory), and their release
RayenProjTile64* proj_tile64_create(const double* G, const double* h, const double* Kinv, const double* w0, int n, int m,
                                    int m_lin, const int32_t* soc_rows, int n_soc);
void proj_tile64_destroy(RayenProjTile64* t);
}  // namespace rayen

struct RayenProjPack {
  int device = -1, n = 0, m = 0, m_lin = 0, n_soc = 0;
  int16_t soc_row0[rayen::kProjMaxSoc] = {}, soc_rows[rayen::kProjMaxSoc] = {};
  int psd_row0 = 0, psd_dim = 0;                // the PSD block (svec rows psd_row0 .. m - 1); psd_dim 0: none
  int unclaimed = 0;                            // rows after the cones that rayen_proj_pack_set_psd has yet to claim
  double rho = 1.0, sigma = 1e-6, alpha = 1.6;
  float* img32 = nullptr;
  double* img64 = nullptr;
  RayenProjTile* tile = nullptr;                // the tile kernel's images (fp32 only)
  RayenProjTile64* tile64 = nullptr;            // the fp64 tile kernel's images (fp64 only; on request)
};
