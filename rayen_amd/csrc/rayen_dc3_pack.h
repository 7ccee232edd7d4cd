// RayenDc3Pack: what rayen_dc3.hip (one lane per sample, image in LDS) and rayen_dc3_tile.hip (32 samples per workgroup
// on the matrix cores) share.  The lane kernels' fields are filled by rayen_dc3_pack_create; the tile kernels' image is
// uploaded by rayen_dc3_tile_pack_set on request (null: never asked for, or the shape is outside dc3_tile_served()).
#pragma once

#include <cstdint>

#include "rayen_side_pack.h"

struct RayenDc3Pack {
  int device = -1, k = 0, n = 0, m = 0, nq = 0, no = 0, NP = 0;
  float* img32 = nullptr;
  double* img64 = nullptr;
  int32_t* perm = nullptr;      // [n] partial variables, then [no] other variables
  float* tile_img = nullptr;    // rayen_dc3_tile_image.h (fp32 only)
  double* tile_img64 = nullptr; // rayen_dc3_tile64_image.h (fp64 only; rayen_dc3_tile64_pack_set, likewise on request)
};
