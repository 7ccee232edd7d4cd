// The soft-cost pack, shared by its translation units: rayen_cost.hip (the pack, the image builders and the resident
// kernels), rayen_cost_stream.hip (the streamed route: windows of the same image through LDS) and rayen_cost_tile64.hip (the
// fp64 tile route: an image of its own in blocks of 16 rows).  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "rayen_cost_lmi.h"
#include "rayen_side_pack.h"

namespace rayen {
struct CostStream;      // rayen_cost_stream.hip
void cost_stream_free(CostStream* s);
struct CostTile64;      // rayen_cost_tile64.hip
void cost_tile64_free(CostTile64* t);
}  // namespace rayen

struct RayenCostPack {
  int device = -1, k = 0, n_simd = 1024;
  // fp32 image (one buffer of 4-byte words): W [nt][32][64] swizzled | rowc [nt][32] | colv [nf][64] | desc [nt][8]
  int32_t* img32 = nullptr;
  int nt = 0, rowc_off = 0, colv_off = 0, desc_off = 0;
  size_t bytes32 = 0;
  bool served32 = false;
  // fp64 image (8-byte words): W [R][K] | rowc [R] | colv [nf][K] | fconst [ni] | desc [ni][8] (ints)
  double* img64 = nullptr;
  int K64 = 0, ni = 0, rowc64_off = 0, colv64_off = 0, fc64_off = 0, desc64_off = 0;
  size_t bytes64 = 0;
  bool served64 = false;
  // the set's LMI (rayen_cost_pack_set_lmi; rayen_cost_lmi.hip).  n_rows: the rows the images above hold; lmi_id: the
  // LMI's index in the stacked order; eq_shift: what the equality rows' indices move up by (1 with an LMI, 0 without)
  rayen::CostLmiImage* lmi = nullptr;
  int n_rows = 0, lmi_id = 0, eq_shift = 0;
  // the streamed route (rayen_cost_stream_set): the set's arrays as they were passed, kept on the HOST so that the stream
  // images can be built on request (k <= 64 only), and the images themselves once somebody asked
  std::vector<double> host;
  std::vector<int32_t> host_soc_rows;
  int m1 = 0, nq = 0, nsoc = 0, m2 = 0;
  rayen::CostStream* stream = nullptr;
  // the fp64 tile route (rayen_cost_tile64_set): its image of the same host arrays, once somebody asked
  rayen::CostTile64* tile64 = nullptr;
};

namespace rayen {

struct CostSetView {
  const double *A1, *b1, *P, *q, *r, *M, *s, *c, *d, *A2, *b2;
  const int32_t* soc_rows;
  int m1, nq, nsoc, m2, k;
};

// The images of a set in the layouts above, geometry into `geom` (nt, *_off, bytes32 | K64, ni, *64_off, bytes64).  False
// when the image is larger than `budget` bytes: then only the size is set (bytes32 | K64, ni, bytes64), the offsets are
// left alone and no words are written.  fp32 also answers false, with nothing set, for a cone of more than 64 rows.
bool cost_build32(const CostSetView& v, RayenCostPack* geom, std::vector<int32_t>* words, size_t budget);
bool cost_build64(const CostSetView& v, RayenCostPack* geom, std::vector<double>* words, size_t budget);

inline int cost_check_call(const RayenCostPack* p, const void* y, const int64_t B, const int64_t ld, const void* grad,
                           const int64_t ldg) {
  if (p == nullptr || B < 0) return RAYEN_E_BAD_ARG;
  if (B > 0 && (y == nullptr || ld < p->k || (grad != nullptr && ldg < p->k))) return RAYEN_E_BAD_ARG;
  return RAYEN_OK;
}

// the whole set at one precision: its rows (when it has any; `rows`: does the route serve them?) and its LMI (when it has
// one)
template <typename T>
inline bool cost_serves_set(const RayenCostPack* p, const bool rows) {
  if (p->n_rows > 0 && !rows) return false;
  if (p->lmi != nullptr) return cost_lmi_serves<T>(p->lmi);
  return p->n_rows > 0;
}

// the rows' launch (resident or streamed), then the LMI's on the same stream (accumulating when the rows came first)
template <typename T, typename Rows>
inline int cost_call(const RayenCostPack* pack, const bool rows, const T* y, int64_t B, int64_t ld, T* cost, T* worst,
                     int32_t* which, T* grad, int64_t ld_grad, void* stream, Rows&& launch_rows) {
  int rc = cost_check_call(pack, y, B, ld, grad, ld_grad);
  if (rc != RAYEN_OK) return rc;
  if (!cost_serves_set<T>(pack, rows)) return RAYEN_E_UNSUPPORTED;
  const bool both = pack->lmi != nullptr && pack->n_rows > 0;
  if (both && which != nullptr && worst == nullptr) return RAYEN_E_BAD_ARG;     // (the LMI's launch compares with the stored worst)
  rc = check_device(pack->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pack->n_rows > 0) {
    rc = launch_rows(st);
    if (rc != RAYEN_OK) return rc;
  }
  if (pack->lmi == nullptr) return RAYEN_OK;
  return cost_lmi_launch<T>(pack->lmi, y, B, ld, cost, worst, which, grad, ld_grad, both ? 1 : 0, pack->lmi_id, st);
}

}  // namespace rayen
