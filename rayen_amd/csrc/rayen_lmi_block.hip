// Instances of the workgroup-per-sample LMI kernels (see rayen_lmi_block.h).
#include "rayen_lmi_block.h"

namespace rayen {

#define RAYEN_LMI_BLOCK_INSTANCES(T)                                                                                     \
  template bool lmi_block_eligible_mixed<T>(const RayenPack*);                                                           \
  template bool lmi_block_eligible<T>(const RayenPack*);                                                                 \
  template bool lmi_block_serves<T>(const LmiWaveImage*);                                                                \
  template int lmi_block_prepare<T>(const LmiWaveImage*);                                                                \
  template int lmi_block_forward<T>(const RayenPack*, const LmiWaveImage*, const T*, int64_t, int64_t, T*, int64_t, T*,  \
                                    int32_t*, int32_t*, hipStream_t, const T*, int64_t, int);                            \
  template bool lmi_block_bwd_serves<T>(const LmiWaveImage*);                                                            \
  template int lmi_block_backward<T>(const RayenPack*, const LmiWaveImage*, const T*, int64_t, int64_t, const T*,        \
                                     const int32_t*, const T*, int64_t, T*, int64_t, hipStream_t, int, int);             \
  template bool lmi_block_products_serves<T>(const LmiWaveImage*);                                                       \
  template int lmi_block_forward_products<T>(const RayenPack*, const LmiWaveImage*, const T*, int64_t, const T*, int64_t, \
                                             int64_t, T*, int64_t, T*, int32_t*, int32_t*, hipStream_t);                 \
  template int lmi_block_bwd_coefficients<T>(const RayenPack*, const LmiWaveImage*, const T*, int64_t, const T*, int64_t, \
                                             int64_t, const T*, const int32_t*, const T*, int64_t, T*, int64_t, T*,      \
                                             hipStream_t);
RAYEN_LMI_BLOCK_INSTANCES(float)
RAYEN_LMI_BLOCK_INSTANCES(double)
#undef RAYEN_LMI_BLOCK_INSTANCES

}  // namespace rayen

#ifdef RAYEN_LB_PROFILE
extern "C" void rayen_debug_lb_prof(unsigned long long* out8) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(rayen::lb::g_lb_prof), 8 * sizeof(unsigned long long));
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(rayen::lb::g_lb_prof), zero, sizeof(zero));
}
#endif
