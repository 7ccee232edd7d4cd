// Soft cost and violation of the LMI  F(y) = F_k + sum_a y_a F_a >= 0  on the ORIGINAL constraints (the fourth family of
// rayen_cost.hip's stacked order; rayen_amd/soft_cost.py: g = -lambda_min(F(y)), one value per sample):
//
//     g       = lambda_max(S),  S = -(F_k + sum_a y_a F_a)
//     cost   += relu(g)^2
//     grad_a += 2 relu(g) dg/dy_a,   dg/dy_a = x' (-F_a) x   with x the unit eigenvector of lambda_max(S)
//
// One 64-lane wave per sample, on the device helpers of rayen_lmi_wave.h: S in the wave's LDS (odd leading dimension: the 64
// lanes of a column walk hit 64 banks), Householder tridiagonalisation, Sturm multisection over the lanes; only a sample
// with g > 0 that is asked for a gradient pays for the eigenvector (inverse iteration, back through the reflectors) and the
// k contractions.  The generators stay in global memory, so k is bounded only by the 3 k elements of LDS next to the matrix.
//
// accumulate == 0 (the LMI is the set's only constraint): cost, worst, which and grad are written.  accumulate != 0: the
// launch follows the kernels of rayen_cost.hip on the same stream over the same rows and adds to what they left; worst /
// which are replaced where g is larger, and on an exact tie where the stored index is an equality row's (> lmi_id).
//
// A sample whose y is not finite (or whose g comes out as a NaN) answers cost = worst = NaN, which = -1; its gradient is
// NaN when this kernel owns the row (accumulate == 0) and left as it is otherwise.
//
// Bounds: one workgroup per sample b < B; columns >= k of y / grad are never touched; every LDS offset is below
// lw::lds_elems(r, k + 1, k), which the host holds against the limit before it launches.
#include "rayen_cost_lmi.h"

#include <cmath>
#include <new>
#include <vector>

#include "rayen_lmi_wave.h"
#include "rayen_side_pack.h"

namespace rayen {

namespace {

constexpr int kMaxR = 1024;      // far beyond what the LDS holds: anything larger is refused before r * r is formed

// acc + a * b with the product rounded on its own (no fused multiply-add): an accumulating launch then adds exactly what
// the launch of the LMI alone writes, so the two can be told apart from an overwrite bit for bit
template <typename T>
__device__ __forceinline__ T add_product(const T acc, const T a, const T b) {
#pragma clang fp contract(off)
  const T m = a * b;
  return acc + m;
}

template <typename T, bool GRAD>
__global__ __launch_bounds__(64) void cost_lmi_kernel(const T* __restrict__ gt, const int r, const int k, const int P,
                                                      const int Pp, const T* __restrict__ y, const int64_t B,
                                                      const int64_t ld, T* __restrict__ cost, T* __restrict__ worst,
                                                      int32_t* __restrict__ which, T* __restrict__ grad, const int64_t ldg,
                                                      const int accumulate, const int lmi_id) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
  T* A = reinterpret_cast<T*>(cl_smem);
  const int LD = lw::ld_of(r), n = k + 1;
  T* dd = A + (size_t)r * LD;
  T* ee = dd + r;
  T* tau = ee + r;
  T* vv = tau + r;
  T* ww = vv + r;
  T* zz = ww + r;
  T* vs = zz + r;                                  // [y ; 1]
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  bool bad = false;
  for (int a = lane; a < k; a += 64) {
    const T v = y[b * ld + a];
    bad |= !(fabs(v) < (T)INFINITY);
    vs[a] = v;
  }
  if (lane == 0) vs[k] = T(1);
  bad = __ballot(bad) != 0;
  __syncthreads();

  T g = T(0);
  if (!bad) {
    lw::form_S<T>(A, LD, gt, vs, n, P, Pp, lane);
    lw::tridiagonalise<T>(A, LD, r, dd, ee, tau, vv, ww, lane);
    g = lw::lambda_max_tridiagonal<T>(dd, ee, r, lane);
    bad = !(g == g);
  }
  if (bad) {       // (wave-uniform)
    const T nan = (T)NAN;
    if (lane == 0) {
      if (cost != nullptr) cost[b] = nan;
      if (worst != nullptr) worst[b] = nan;
      if (which != nullptr) which[b] = -1;
    }
    if (GRAD && !accumulate)
      for (int a = lane; a < k; a += 64) grad[b * ldg + a] = nan;
    return;
  }

  const T p = g > T(0) ? g : T(0);
  if (lane == 0) {
    if (!accumulate) {
      if (cost != nullptr) cost[b] = add_product(T(0), p, p);
      if (worst != nullptr) worst[b] = g;
      if (which != nullptr) which[b] = lmi_id;
    } else {
      if (cost != nullptr) cost[b] = add_product(cost[b], p, p);
      if (worst != nullptr) {
        const T w = worst[b];                      // (a NaN left by the other rows' kernel stays: neither test holds)
        const bool tie_won = which != nullptr && g == w && which[b] > lmi_id;
        if (g > w || tie_won) {
          worst[b] = g;
          if (which != nullptr) which[b] = lmi_id;
        }
      }
    }
  }
  if (!GRAD) return;
  if (!(g > T(0))) {                               // inside: exactly nothing
    if (!accumulate)
      for (int a = lane; a < k; a += 64) grad[b * ldg + a] = T(0);
    return;
  }
  lw::top_eigenvector<T>(A, LD, r, dd, ee, tau, vv, ww, zz, g, lane);
  lw::outer_product_packed<T>(A, zz, P, lane);
  const T two_g = T(2) * g;
  for (int a0 = 0; a0 < k; a0 += 64) {
    const int na = k - a0 < 64 ? k - a0 : 64;
    T mine = T(0);                                 // lane j keeps generator a0 + j: one coalesced write per 64 of them
    for (int j = 0; j < na; ++j) {
      const T* col = gt + (size_t)(a0 + j) * Pp;
      T part = T(0);
      for (int idx = lane; idx < P; idx += 64) part = fma(col[idx], A[idx], part);
      part = lw::wsum(part);
      if (lane == j) mine = part;
    }
    if (lane < na) {
      T* dst = grad + b * ldg + a0 + lane;
      *dst = add_product(accumulate ? *dst : T(0), two_g, mine);
    }
  }
}

template <typename T> T* image_of(const CostLmiImage* img);
template <> float* image_of<float>(const CostLmiImage* img) { return img->gt32; }
template <> double* image_of<double>(const CostLmiImage* img) { return img->gt64; }

template <typename T>
size_t lds_bytes(const CostLmiImage* img) {
  return lw::lds_elems(img->r, img->k + 1, img->k) * sizeof(T);
}

// the images of one precision, and above 48 KiB of LDS the kernels' opt-in (pack creation is the place for it)
template <typename T>
int build_one(const double* F, CostLmiImage* img, T** dev) {
  const int r = img->r, n = img->k + 1, Pp = img->Pp;
  std::vector<T> gt((size_t)n * Pp, T(0));
  for (int a = 0; a < n; ++a)
    for (int i = 0; i < r; ++i)
      for (int j = 0; j <= i; ++j) gt[(size_t)a * Pp + i * (i + 1) / 2 + j] = (T)(-F[((size_t)a * r + i) * r + j]);
  if (!upload_image(gt, dev)) return RAYEN_E_ALLOC;
  const size_t lds = lds_bytes<T>(img);
  if (lds > kLdsNoOptIn && lds <= lw::kWaveLdsMax &&
      !(allow_lds(cost_lmi_kernel<T, true>, lw::kWaveLdsMax) && allow_lds(cost_lmi_kernel<T, false>, lw::kWaveLdsMax)))
    return RAYEN_E_LAUNCH;
  return RAYEN_OK;
}

}  // namespace

int cost_lmi_build(const double* F, const int r, const int k, CostLmiImage** out) {
  CostLmiImage* img = new (std::nothrow) CostLmiImage();
  if (img == nullptr) return RAYEN_E_ALLOC;
  img->r = r;
  img->k = k;
  img->P = r <= kMaxR ? r * (r + 1) / 2 : 0;
  img->Pp = (img->P + 63) / 64 * 64;
  int rc = RAYEN_OK;
  // (a matrix no precision holds gets no image: every call answers RAYEN_E_UNSUPPORTED before it would be read)
  if (cost_lmi_serves<float>(img)) rc = build_one<float>(F, img, &img->gt32);
  if (rc == RAYEN_OK && cost_lmi_serves<double>(img)) rc = build_one<double>(F, img, &img->gt64);
  if (rc != RAYEN_OK) {
    cost_lmi_free(img);
    return rc;
  }
  *out = img;
  return RAYEN_OK;
}

void cost_lmi_free(CostLmiImage* img) {
  if (img == nullptr) return;
  if (img->gt32) (void)hipFree(img->gt32);
  if (img->gt64) (void)hipFree(img->gt64);
  delete img;
}

template <typename T>
bool cost_lmi_serves(const CostLmiImage* img) {
  return img != nullptr && img->r >= 1 && img->r <= kMaxR && lds_bytes<T>(img) <= lw::kWaveLdsMax;
}

template <typename T>
int cost_lmi_launch(const CostLmiImage* img, const T* y, const int64_t B, const int64_t ld, T* cost, T* worst,
                    int32_t* which, T* grad, const int64_t ldg, const int accumulate, const int lmi_id, hipStream_t stream) {
  if (!cost_lmi_serves<T>(img) || image_of<T>(img) == nullptr) return RAYEN_E_UNSUPPORTED;
  if (B == 0) return RAYEN_OK;
  if (B > 0x7fffffffLL) return RAYEN_E_UNSUPPORTED;
  const size_t lds = lds_bytes<T>(img);
  auto kern = grad != nullptr ? cost_lmi_kernel<T, true> : cost_lmi_kernel<T, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds, stream, image_of<T>(img), img->r, img->k, img->P, img->Pp, y, B,
                     ld, cost, worst, which, grad, ldg, accumulate, lmi_id);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

template bool cost_lmi_serves<float>(const CostLmiImage*);
template bool cost_lmi_serves<double>(const CostLmiImage*);
template int cost_lmi_launch<float>(const CostLmiImage*, const float*, int64_t, int64_t, float*, float*, int32_t*, float*,
                                    int64_t, int, int, hipStream_t);
template int cost_lmi_launch<double>(const CostLmiImage*, const double*, int64_t, int64_t, double*, double*, int32_t*,
                                     double*, int64_t, int, int, hipStream_t);

}  // namespace rayen
