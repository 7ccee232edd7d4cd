// The LMI of a soft-cost pack (rayen_cost.hip owns the pack; rayen_cost_lmi.hip the kernel and this image).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rayen {

// generators of S(y) = -(F_k + sum_a y_a F_a) in both precisions: [k + 1][Pp], packed lower triangle, transposed,
// generator-major, negated, the constant term last (the layout of LmiWaveImage::gt)
struct CostLmiImage {
  float* gt32 = nullptr;
  double* gt64 = nullptr;
  int r = 0, k = 0, P = 0, Pp = 0;
};

// F [k + 1, r, r] row-major fp64 (lower triangle read).  RAYEN_OK or RAYEN_E_ALLOC; the current device gets the image.
int cost_lmi_build(const double* F, int r, int k, CostLmiImage** out);
void cost_lmi_free(CostLmiImage* img);

// does a wave's LDS hold the r x r matrix and its vectors at this precision?
template <typename T> bool cost_lmi_serves(const CostLmiImage* img);

// One launch on `stream`.  accumulate == 0: cost / worst / which / grad are written (the LMI is the set's only constraint);
// accumulate != 0: they hold what the kernels of rayen_cost.hip left for the set's other rows and the LMI, whose index in
// the stacked order is lmi_id, is added.  Any of cost / worst / which may be null; grad null = values alone.
template <typename T>
int cost_lmi_launch(const CostLmiImage* img, const T* y, int64_t B, int64_t ld, T* cost, T* worst, int32_t* which, T* grad,
                    int64_t ldg, int accumulate, int lmi_id, hipStream_t stream);

}  // namespace rayen
