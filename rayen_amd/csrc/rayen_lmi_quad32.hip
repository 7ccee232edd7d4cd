// fp32 instances of the four-lanes-per-sample LMI kernel (see rayen_lmi_quad.h).
#include "rayen_lmi_quad.h"

namespace rayen {

template bool lmi_quad_eligible<float>(const RayenPack*);
template int lmi_quad_build<float>(const RayenPack*, LmiQuadImage**, int64_t*);
template int lmi_quad_forward<float>(const RayenPack*, const LmiQuadImage*, const float*, int64_t, int64_t, float*, int64_t,
                                     float*, int32_t*, int32_t*, hipStream_t);
void lmi_quad_free(LmiQuadImage* img) {
  if (img == nullptr) return;
  if (img->data) (void)hipFree(img->data);
  if (img->wrow) (void)hipFree(img->wrow);
  if (img->wm) (void)hipFree(img->wm);
  if (img->lin_id) (void)hipFree(img->lin_id);
  delete img;
}
template bool lmi_quad_bwd_serves<float>(const RayenPack*, const LmiQuadImage*);
template int lmi_quad_backward<float>(const RayenPack*, const LmiQuadImage*, const float*, int64_t, int64_t, const float*,
                                      const int32_t*, const float*, int64_t, float*, int64_t, hipStream_t);

}  // namespace rayen
