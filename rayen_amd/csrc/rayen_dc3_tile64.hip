// method='DC3' beyond LDS in fp64 (the reference's training dtype; header of rayen_mfma_f64.hip): the kernels of
// rayen_dc3_tile_kernel.h at the geometry Dc3Geom64 -- 16-sample tiles on v_mfma_f64_16x16x4_f64, n in one to four blocks
// of 16 rows -- behind the six entry points of include/rayen_hip_dc3_tile64.h.  What 'tile' / 'auto' run on fp64 input: sets
// the fp64 lane kernel does not stage (33 <= n <= 64, or an fp64 image over LDS).
#include "rayen_dc3_tile_kernel.h"

namespace tile = rayen::dc3_tile;
using G = tile::Dc3Geom64;

extern "C" {

int rayen_dc3_tile64_shape_served(int32_t n, int32_t m, int32_t nq, int32_t no) { return tile::shape_served<G>(n, m, nq, no); }

int rayen_dc3_tile64_pack_set(RayenDc3Pack* p, const double* A1e, const double* b1e, const double* Pe, const double* qe,
                              const double* re, const double* C, const double* c0) {
  return tile::pack_set<G>(p, A1e, b1e, Pe, qe, re, C, c0);
}

int rayen_dc3_tile64_served(const RayenDc3Pack* pack) { return tile::served<G>(pack) ? 1 : 0; }

int64_t rayen_dc3_tile64_workspace_bytes(const RayenDc3Pack* p, int64_t B, int32_t max_steps, int32_t backward) {
  return tile::workspace_bytes<G>(p, B, max_steps, backward);
}

int rayen_dc3_tile64_forward_f64(const RayenDc3Pack* p, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                                 double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                                 int64_t ws_bytes, int32_t* nan_flag, void* stream) {
  return tile::forward<G>(p, q, B, ldq, y, ldy, lr, momentum, eps, max_steps, tstar, ws, ws_bytes, nan_flag, stream);
}

int rayen_dc3_tile64_backward_f64(const RayenDc3Pack* p, const double* q, int64_t B, int64_t ldq, const double* grad_y,
                                  int64_t ldg, double* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                                  const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream) {
  return tile::backward<G>(p, q, B, ldq, grad_y, ldg, grad_q, ldgq, lr, momentum, max_steps, tstar, ws, ws_bytes, stream);
}

}  // extern "C"
