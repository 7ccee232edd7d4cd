// fp64 instances of the wave-per-sample LMI kernels (see rayen_lmi_wave.h).
#include "rayen_lmi_wave.h"

namespace rayen {

template bool lmi_wave_eligible<double>(const RayenPack*);
template int lmi_wave_build<double>(const RayenPack*, LmiWaveImage**, int64_t*);
template bool lmi_wave_serves<double>(const LmiWaveImage*);
template int lmi_wave_forward<double>(const RayenPack*, const LmiWaveImage*, const double*, int64_t, int64_t, double*, int64_t, double*,
                                int32_t*, int32_t*, hipStream_t);
template int lmi_wave_backward<double>(const RayenPack*, const LmiWaveImage*, const double*, int64_t, int64_t, const double*,
                                 const int32_t*, const double*, int64_t, double*, int64_t, hipStream_t);

}  // namespace rayen
