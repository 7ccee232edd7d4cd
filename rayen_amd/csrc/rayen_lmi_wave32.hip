// fp32 instances of the wave-per-sample LMI kernels (see rayen_lmi_wave.h).
#include "rayen_lmi_wave.h"

namespace rayen {

template bool lmi_wave_eligible<float>(const RayenPack*);
template int lmi_wave_build<float>(const RayenPack*, LmiWaveImage**, int64_t*);
template bool lmi_wave_serves<float>(const LmiWaveImage*);
void lmi_wave_free(LmiWaveImage* img) { lw::lmi_wave_free_image(img); }
template int lmi_wave_forward<float>(const RayenPack*, const LmiWaveImage*, const float*, int64_t, int64_t, float*, int64_t, float*,
                               int32_t*, int32_t*, hipStream_t);
template int lmi_wave_backward<float>(const RayenPack*, const LmiWaveImage*, const float*, int64_t, int64_t, const float*,
                                const int32_t*, const float*, int64_t, float*, int64_t, hipStream_t);

}  // namespace rayen
