// method='Bar' (the reference's barycentric layer, rayen/constraint_module.py:479-486): forward and backward.
//
//     lambda = softmax(q[:, :nv]),  mu = |q[:, nv:nv+nr]|,  y = G [lambda; mu] + yp,  G = NA_E [V R]  (k x m, m = nv + nr)
//
// Memory-bound (2k flop per element of q read), so the layout is about the bytes:
//  * the image of G ([m4 + 1][K], m4 = m rounded up to 4: generator j's k coefficients in row gen_slot(j), zero-padded to
//    K in {4, 8, 16, 32, 64}, yp in row m4)
//    is copied into LDS once per workgroup; a workgroup then walks row groups until the batch is done;
//  * L lanes (a power of two <= 16, about a quarter of m) share a row; lane i of a group reads the row's 16-byte pieces
//    i, i + L, ... -- consecutive lanes, consecutive pieces -- so each row is read from HBM once, coalesced;
//  * per lane: an online max over its vertex columns (the K accumulators and the sum rescaled only when the max grows),
//    exp(q - max) weights and |q| weights multiplied into G from LDS (ds_read_b128 rows of K coefficients);
//  * per group: max and sum reduced across the L lanes, the vertex part scaled by exp(M_lane - M) / S lane-locally, the ray
//    part added, ONE K-wide sum across the group; lane i then stores y[i], y[i + L], ... with yp added.
// The backward recomputes e = exp(q - lse) from the forward's per-row log-sum-exp and normalises it again,
// lambda = e / sum(e): lse is stored rounded to the working precision, and exp turns that rounding (up to ulp(lse) / 2,
// which grows with the logits) into a common relative error of every e -- the quotient cancels it exactly.  It forms
// g = G' grad_y column by column (K FMAs per element of q) and writes grad_q = lambda (g - <lambda, g>) on the vertex
// columns and sign(q) g on the ray columns, in the same 16-byte pieces.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "rayen_bar_pack.h"      // the pack, the image's layout, load4 / store4, the group reductions: shared with rayen_bar_stream.hip

namespace {

using namespace rayen::bar;
using rayen::kLdsBudget;                      // the kernels stage nothing but the image

template <typename T>
__device__ __forceinline__ void stage_image(T* lds, const T* __restrict__ img, int m, int K) {
  const int n16 = (int)(((size_t)(((m + 3) & ~3) + 1) * K * sizeof(T)) / 16);
  uint4* dst = reinterpret_cast<uint4*>(lds);
  const uint4* src = reinterpret_cast<const uint4*>(img);
  for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

template <typename T, int K>
__global__ __launch_bounds__(kThreads) void bar_forward_kernel(const T* __restrict__ img, int nv, int m, int lgL,
                                                               const T* __restrict__ q, int64_t B, int64_t ldq, int vec,
                                                               T* __restrict__ y, int64_t ldy, int k,
                                                               T* __restrict__ rowstat, int32_t* __restrict__ nan_flag) {
  extern __shared__ __align__(16) unsigned char bar_smem[];
  T* G = reinterpret_cast<T*>(bar_smem);
  stage_image(G, img, m, K);
  const int L = 1 << lgL;
  const int li = threadIdx.x & (L - 1);
  const int rows_per_iter = kThreads >> lgL;
  const int npieces = (m + 3) >> 2;
  const int pv = (nv + 3) >> 2;          // pieces that hold vertex columns
  const int pr = nv >> 2;                // first piece that holds a ray column
  const T ninf = -static_cast<T>(INFINITY);
  for (int64_t row = (int64_t)blockIdx.x * rows_per_iter + (threadIdx.x >> lgL); row < B;
       row += (int64_t)gridDim.x * rows_per_iter) {
    const T* __restrict__ qr = q + row * ldq;
    T acc[K];
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] = T(0);
    T lse = T(0);
    if (nv > 0) {
      T M = ninf, s = T(0);
      for (int p = li; p < pv; p += L) {
        T v[4];
        load4(qr + 4 * p, vec != 0, m - 4 * p, v);
        T pm = ninf;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * p + c < nv) pm = fmax(pm, v[c]);
        if (pm > M) {                    // online max: rescale only when it grows
          const T f = exp_(M - pm);
          s *= f;
#pragma unroll
          for (int i = 0; i < K; ++i) acc[i] *= f;
          M = pm;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = 4 * p + c;
          if (j < nv) {
            // (a -inf logit weighs 0, as in torch's softmax, also while this lane's max is still -inf)
            const T w = v[c] == ninf ? T(0) : exp_(v[c] - M);
            s += w;
            const T* __restrict__ g = G + (size_t)gen_slot(j) * K;
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i] = fma(g[i], w, acc[i]);
          }
        }
      }
      const T Mg = group_max(M, L);
      const T f = M == ninf ? T(0) : exp_(M - Mg);
      const T S = group_sum(s * f, L);
      const T scale = f / S;
#pragma unroll
      for (int i = 0; i < K; ++i) acc[i] *= scale;
      lse = Mg + log_(S);
    }
    for (int p = pr + li; p < npieces; p += L) {
      T v[4];
      load4(qr + 4 * p, vec != 0, m - 4 * p, v);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = 4 * p + c;
        if (j >= nv && j < m) {
          const T w = fabs(v[c]);
          const T* __restrict__ g = G + (size_t)gen_slot(j) * K;
#pragma unroll
          for (int i = 0; i < K; ++i) acc[i] = fma(g[i], w, acc[i]);
        }
      }
    }
    if (L > 1) {
#pragma unroll
      for (int i = 0; i < K; ++i) acc[i] = group_sum(acc[i], L);
    }
    T* __restrict__ yr = y + row * ldy;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (i < k && (i & (L - 1)) == li) {
        const T out = acc[i] + G[(size_t)((m + 3) & ~3) * K + i];
        yr[i] = out;
        bad |= out != out;
      }
    }
    if (rowstat != nullptr && li == 0) rowstat[row] = lse;
    if (bad && nan_flag != nullptr) atomicOr(nan_flag, 1);
  }
}

template <typename T, int K>
__global__ __launch_bounds__(kThreads) void bar_backward_kernel(const T* __restrict__ img, int nv, int m, int lgL,
                                                                const T* __restrict__ q, int64_t B, int64_t ldq, int vec_in,
                                                                int vec_out, const T* __restrict__ rowstat,
                                                                const T* __restrict__ grad_y, int k,
                                                                T* __restrict__ grad_q) {
  extern __shared__ __align__(16) unsigned char bar_smem[];
  T* G = reinterpret_cast<T*>(bar_smem);
  stage_image(G, img, m, K);
  const int L = 1 << lgL;
  const int li = threadIdx.x & (L - 1);
  const int rows_per_iter = kThreads >> lgL;
  const int npieces = (m + 3) >> 2;
  const int pv = (nv + 3) >> 2;
  for (int64_t row = (int64_t)blockIdx.x * rows_per_iter + (threadIdx.x >> lgL); row < B;
       row += (int64_t)gridDim.x * rows_per_iter) {
    const T* __restrict__ qr = q + row * ldq;
    T gy[K];
#pragma unroll
    for (int i = 0; i < K; ++i) gy[i] = i < k ? grad_y[row * k + i] : T(0);
    const T lse = nv > 0 ? rowstat[row] : T(0);
    T dot = T(0), inv = T(0);            // <lambda, g> and 1 / sum_j exp(q_j - lse)
    if (nv > 0) {
      T s = T(0);
      for (int p = li; p < pv; p += L) {
        T v[4];
        load4(qr + 4 * p, vec_in != 0, m - 4 * p, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = 4 * p + c;
          if (j < nv) {
            const T* __restrict__ g = G + (size_t)gen_slot(j) * K;
            T gj = T(0);
#pragma unroll
            for (int i = 0; i < K; ++i) gj = fma(g[i], gy[i], gj);
            const T e = exp_(v[c] - lse);
            s += e;
            dot = fma(e, gj, dot);
          }
        }
      }
      inv = T(1) / group_sum(s, L);
      dot = group_sum(dot, L) * inv;
    }
    T* __restrict__ gr = grad_q + row * ldq;
    for (int p = li; p < npieces; p += L) {
      T v[4], o[4];
      load4(qr + 4 * p, vec_in != 0, m - 4 * p, v);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = 4 * p + c;
        T gj = T(0);
        if (j < m) {
          const T* __restrict__ g = G + (size_t)gen_slot(j) * K;
#pragma unroll
          for (int i = 0; i < K; ++i) gj = fma(g[i], gy[i], gj);
        }
        const T sgn = v[c] > T(0) ? T(1) : (v[c] < T(0) ? T(-1) : T(0));
        o[c] = j < nv ? exp_(v[c] - lse) * inv * (gj - dot) : sgn * gj;
      }
      store4(gr + 4 * p, vec_out != 0, m - 4 * p, o);
    }
  }
}

// workgroups: enough to cover the batch, at most as many as fit on the chip at once (LDS and waves per CU)
unsigned grid_for(const RayenBarPack* p, int64_t B, int lgL, size_t lds) {
  const int64_t rows_per_iter = kThreads >> lgL;
  const int64_t need = (B + rows_per_iter - 1) / rows_per_iter;
  int64_t per_cu = (int64_t)(kLdsBudget / lds);
  if (per_cu > 4) per_cu = 4;
  if (per_cu < 1) per_cu = 1;
  const int64_t cap = (int64_t)p->cus * per_cu;
  return (unsigned)(need < cap ? need : cap);
}

template <typename T, int K>
int launch_forward(const RayenBarPack* p, const T* q, int64_t B, int64_t ldq, T* y, int64_t ldy, T* rowstat,
                   int32_t* nan_flag, hipStream_t stream) {
  const size_t lds = lds_bytes<T>(p);
  auto kern = bar_forward_kernel<T, K>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const int m = p->nv + p->nr, lgL = group_log2(m);
  const int vec = rayen::rows_aligned16(q, ld_words<T>(ldq));
  const int64_t chunk = rows_per_launch(ldq > ldy ? ldq : ldy, sizeof(T));
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t b = B - r0 < chunk ? B - r0 : chunk;
    hipLaunchKernelGGL(kern, dim3(grid_for(p, b, lgL, lds)), dim3(kThreads), lds, stream, image<T>(p), p->nv, m, lgL,
                       q + r0 * ldq, b, ldq, vec, y + r0 * ldy, ldy, p->k, rowstat ? rowstat + r0 : nullptr, nan_flag);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename T, int K>
int launch_backward(const RayenBarPack* p, const T* q, int64_t ldq, const T* rowstat, const T* grad_y, int64_t B,
                    T* grad_q, hipStream_t stream) {
  const size_t lds = lds_bytes<T>(p);
  auto kern = bar_backward_kernel<T, K>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const int m = p->nv + p->nr, lgL = group_log2(m);
  const int vec_in = rayen::rows_aligned16(q, ld_words<T>(ldq));
  const int vec_out = rayen::rows_aligned16(grad_q, ld_words<T>(ldq));
  const int64_t chunk = rows_per_launch(ldq > p->k ? ldq : p->k, sizeof(T));
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t b = B - r0 < chunk ? B - r0 : chunk;
    hipLaunchKernelGGL(kern, dim3(grid_for(p, b, lgL, lds)), dim3(kThreads), lds, stream, image<T>(p), p->nv, m, lgL,
                       q + r0 * ldq, b, ldq, vec_in, vec_out, rowstat ? rowstat + r0 : nullptr, grad_y + r0 * p->k, p->k,
                       grad_q + r0 * ldq);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename T>
int bar_forward(const RayenBarPack* p, const T* q, int64_t B, int64_t ldq, T* y, int64_t ldy, T* rowstat,
                int32_t* nan_flag, void* stream) {
  if (p == nullptr || B < 0) return RAYEN_E_BAD_ARG;
  const int m = p->nv + p->nr;
  if (B > 0 && (q == nullptr || y == nullptr || ldq < m || ldy < p->k)) return RAYEN_E_BAD_ARG;
  if (image<T>(p) == nullptr || lds_bytes<T>(p) > kLdsBudget) return RAYEN_E_UNSUPPORTED;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rayen::dispatch_width<kMinK, kMaxK>(p->K, [&](auto K) {
    return launch_forward<T, K()>(p, q, B, ldq, y, ldy, rowstat, nan_flag, s);
  });
}

template <typename T>
int bar_backward(const RayenBarPack* p, const T* q, int64_t ldq, const T* rowstat, const T* grad_y, int64_t B,
                 T* grad_q, void* stream) {
  if (p == nullptr || B < 0) return RAYEN_E_BAD_ARG;
  const int m = p->nv + p->nr;
  if (B > 0 && (q == nullptr || grad_y == nullptr || grad_q == nullptr || ldq < m || (p->nv > 0 && rowstat == nullptr)))
    return RAYEN_E_BAD_ARG;
  if (image<T>(p) == nullptr || lds_bytes<T>(p) > kLdsBudget) return RAYEN_E_UNSUPPORTED;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rayen::dispatch_width<kMinK, kMaxK>(p->K, [&](auto K) {
    return launch_backward<T, K()>(p, q, ldq, rowstat, grad_y, B, grad_q, s);
  });
}

template <typename T>
bool upload(const double* G, const double* yp, int k, int m, int K, T** out) {
  const int mp = (m + 3) & ~3;      // generators padded to whole groups of four (zero rows), yp behind them
  std::vector<T> h((size_t)(mp + 1) * K, T(0));
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < k; ++i) h[(size_t)gen_slot(j) * K + i] = static_cast<T>(G[(size_t)i * m + j]);
  for (int i = 0; i < k; ++i) h[(size_t)mp * K + i] = static_cast<T>(yp[i]);
  return rayen::upload_image(h, out);
}

}  // namespace

extern "C" {

int rayen_bar_pack_create(const double* G, const double* yp, int32_t k, int32_t nv, int32_t nr, RayenBarPack** out) {
  if (out == nullptr) return RAYEN_E_BAD_ARG;
  *out = nullptr;
  if (G == nullptr || yp == nullptr || k <= 0 || nv < 0 || nr < 0 || nv + nr <= 0) return RAYEN_E_BAD_ARG;
  if (k > kMaxK) return RAYEN_E_UNSUPPORTED;
  int dev = -1, cus = 0;
  if (rayen::side_pack_device(&dev, &cus, 256) != RAYEN_OK) return RAYEN_E_NO_DEVICE;
  RayenBarPack* p = new (std::nothrow) RayenBarPack();
  if (p == nullptr) return RAYEN_E_ALLOC;
  p->device = dev;
  p->k = k;
  p->nv = nv;
  p->nr = nr;
  p->K = rayen::padded_width<kMinK, kMaxK>(k);
  p->cus = cus;
  const int m = nv + nr;
  if (!upload<float>(G, yp, k, m, p->K, &p->img32) || !upload<double>(G, yp, k, m, p->K, &p->img64)) {
    rayen_bar_pack_destroy(p);
    return RAYEN_E_ALLOC;
  }
  *out = p;
  return RAYEN_OK;
}

void rayen_bar_pack_destroy(RayenBarPack* p) {
  if (p == nullptr) return;
  {
    rayen::DeviceScope on_device(p->device);
    if (p->img32) (void)hipFree(p->img32);
    if (p->img64) (void)hipFree(p->img64);
  }
  delete p;
}

int rayen_bar_forward_f32(const RayenBarPack* pack, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                          float* rowstat, int32_t* nan_flag, void* stream) {
  return bar_forward<float>(pack, q, B, ldq, y, ldy, rowstat, nan_flag, stream);
}

int rayen_bar_forward_f64(const RayenBarPack* pack, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                          double* rowstat, int32_t* nan_flag, void* stream) {
  return bar_forward<double>(pack, q, B, ldq, y, ldy, rowstat, nan_flag, stream);
}

int rayen_bar_backward_f32(const RayenBarPack* pack, const float* q, int64_t ldq, const float* rowstat,
                           const float* grad_y, int64_t B, float* grad_q, void* stream) {
  return bar_backward<float>(pack, q, ldq, rowstat, grad_y, B, grad_q, stream);
}

int rayen_bar_backward_f64(const RayenBarPack* pack, const double* q, int64_t ldq, const double* rowstat,
                           const double* grad_y, int64_t B, double* grad_q, void* stream) {
  return bar_backward<double>(pack, q, ldq, rowstat, grad_y, B, grad_q, stream);
}

}  // extern "C"
