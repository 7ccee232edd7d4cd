// fp64 instances of the four-lanes-per-sample LMI kernel (see rayen_lmi_quad.h).
#include "rayen_lmi_quad.h"

namespace rayen {

template bool lmi_quad_eligible<double>(const RayenPack*);
template int lmi_quad_build<double>(const RayenPack*, LmiQuadImage**, int64_t*);
template int lmi_quad_forward<double>(const RayenPack*, const LmiQuadImage*, const double*, int64_t, int64_t, double*, int64_t,
                                      double*, int32_t*, int32_t*, hipStream_t);
template bool lmi_quad_bwd_serves<double>(const RayenPack*, const LmiQuadImage*);
template int lmi_quad_backward<double>(const RayenPack*, const LmiQuadImage*, const double*, int64_t, int64_t, const double*,
                                       const int32_t*, const double*, int64_t, double*, int64_t, hipStream_t);

}  // namespace rayen
