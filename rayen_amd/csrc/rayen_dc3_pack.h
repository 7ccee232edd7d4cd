// RayenDc3Pack: what rayen_dc3.hip (one lane per sample, image in LDS) and rayen_dc3_tile_kernel.h (sample tiles on the
// matrix cores, fp32 and fp64) share.  The lane kernels' fields are filled by rayen_dc3_pack_create; a tile geometry's image
// is uploaded by rayen_dc3_tile_pack_set / rayen_dc3_tile64_pack_set on request (null: never asked for, or the shape is
// outside the layout's served()).
#pragma once

#include <cstdint>

#include "rayen_side_pack.h"

struct RayenDc3Pack {
  int device = -1, k = 0, n = 0, m = 0, nq = 0, no = 0, NP = 0;
  float* img32 = nullptr;
  double* img64 = nullptr;
  int32_t* perm = nullptr;      // [n] partial variables, then [no] other variables
  float* tile_img = nullptr;    // Dc3TileLayout32 of rayen_dc3_tile_image.h (fp32 only)
  double* tile_img64 = nullptr; // Dc3TileLayout64 of the same header (fp64 only)
};
