// method='DC3' beyond LDS in fp32: the kernels of rayen_dc3_tile_kernel.h at the geometry Dc3Geom32 -- 32-sample tiles on
// v_mfma_f32_32x32x2_f32, n in one or two blocks of 32 rows -- behind the six entry points of include/rayen_hip_dc3_tile.h.
#include "rayen_dc3_tile_kernel.h"

namespace tile = rayen::dc3_tile;
using G = tile::Dc3Geom32;

extern "C" {

int rayen_dc3_tile_shape_served(int32_t n, int32_t m, int32_t nq, int32_t no) { return tile::shape_served<G>(n, m, nq, no); }

int rayen_dc3_tile_pack_set(RayenDc3Pack* p, const double* A1e, const double* b1e, const double* Pe, const double* qe,
                            const double* re, const double* C, const double* c0) {
  return tile::pack_set<G>(p, A1e, b1e, Pe, qe, re, C, c0);
}

int rayen_dc3_tile_served(const RayenDc3Pack* pack) { return tile::served<G>(pack) ? 1 : 0; }

int64_t rayen_dc3_tile_workspace_bytes(const RayenDc3Pack* p, int64_t B, int32_t max_steps, int32_t backward) {
  return tile::workspace_bytes<G>(p, B, max_steps, backward);
}

int rayen_dc3_tile_forward_f32(const RayenDc3Pack* p, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                               double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                               int64_t ws_bytes, int32_t* nan_flag, void* stream) {
  return tile::forward<G>(p, q, B, ldq, y, ldy, lr, momentum, eps, max_steps, tstar, ws, ws_bytes, nan_flag, stream);
}

int rayen_dc3_tile_backward_f32(const RayenDc3Pack* p, const float* q, int64_t B, int64_t ldq, const float* grad_y,
                                int64_t ldg, float* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                                const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream) {
  return tile::backward<G>(p, q, B, ldq, grad_y, ldg, grad_q, ldgq, lr, momentum, max_steps, tstar, ws, ws_bytes, stream);
}

}  // extern "C"
