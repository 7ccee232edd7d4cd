// method='DC3' (the reference's completion + gradient-correction baseline, rayen/constraint_module.py:265-336): forward and
// backward in exact fp32 / fp64.
//
// The reference iterates on the full y, but y[other] stays the affine function c0 + C p of p = y[partial] throughout, so the
// iteration lives in R^n (n = k - number of independent equalities):
//
//     r = relu(A1e p - b1e),  g_i = 0.5 p'Pe_i p + qe_i'p + re_i,  u_i = Pe_i p + qe_i
//     grad = 2 A1e' r + sum_i 2 u_i relu(g_i),   s <- lr grad + momentum s,   p <- p - s
//
// and after the last step y[partial] = p, y[other] = c0 + C p.  The stop is the reference's and BATCH-GLOBAL: after every
// step the maximum over the whole batch of the relu'd residuals is compared with eps; every row takes the same number of
// steps.  No host sync and no grid barrier:
//  * the steps run in chunks of kChunk per launch; (p, s) ping-pongs between two state buffers (none with one chunk);
//  * each step's batch maximum lands in viol[t] (the violation AFTER step t) by an atomic max on the bits of a
//    non-negative float (NaN is sent as the canonical quiet NaN, which orders above +inf: `NaN < eps` is false, as in torch);
//  * a chunk launch first scans viol[1..t0]: if an earlier step already met the stop rule it exits without writing, so the
//    start state of the stopping chunk survives;
//  * every chunk writes y from its end state; one finishing launch finds the stop step t*, and if t* is not its chunk's end
//    replays t* - t0 steps from the surviving start state and overwrites y.  It writes t* for the caller.
// Layout: one lane per row, p / s / grad in registers (n padded to NP in {4, 8, 16, 32, 64}; fp64 up to 32), the constants
// in LDS (copied once per workgroup) and read as wave-uniform 16-byte pieces (a broadcast, no bank conflict).  Vector FMAs
// throughout: this layout gives the matrix cores no tile; from NP = 16 up it also takes every VGPR.
// The backward differentiates the unrolled T = t* steps like autograd does on the reference (the stop decision carries no
// gradient, relu'(0) = 0): it recomputes p_0..p_{T-1} into a caller-provided workspace [T][n][B], then sweeps back
//     sbar_t = -pbar_{t+1} + momentum sbar_{t+1},   pbar_t = pbar_{t+1} + lr J(p_t)' sbar_t
//     J' x = 2 A1e' diag[r > 0] A1e x + sum_i 2 (relu(g_i) Pe_i' x + [g_i > 0] (u_i . x) grad g_i),
//     grad g_i = 0.5 (Pe_i + Pe_i') p + qe_i      (the reference's Pe_i is not symmetric when the set has equalities)
// from pbar_T = grad_y[partial] + C' grad_y[other]; grad_q = pbar_0.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "rayen_dc3_pack.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;                    // steps per launch
constexpr int kMinNP = 4, kMaxNP = 64;        // the kernels' NP: n padded to a power of two between these (fp64: up to 32)
using rayen::kLdsBudget;                      // 256 bytes of it are left to the kernels' static variables: sh_t today;
                                              // -Rpass-analysis=kernel-resource-usage prints the figure

struct Dims {
  int n, k, m, nq, no;
  int off_b, off_q, qstride, off_C, off_c0, total;      // in elements of T
};

inline int round4(int x) { return (x + 3) & ~3; }

Dims dims_of(const RayenDc3Pack* p) {
  Dims d;
  d.n = p->n; d.k = p->k; d.m = p->m; d.nq = p->nq; d.no = p->no;
  const int NP = p->NP;
  d.off_b = p->m * NP;
  d.off_q = d.off_b + round4(p->m);
  d.qstride = NP * NP + NP + 4;
  d.off_C = d.off_q + p->nq * d.qstride;
  d.off_c0 = d.off_C + p->no * NP;
  d.total = d.off_c0 + round4(p->no) + 4;
  return d;
}

template <typename T> struct BitsOf;
template <> struct BitsOf<float> {
  using type = unsigned int;
  static constexpr type kNan = 0x7fc00000u;
  static __device__ __forceinline__ type to(float v) { return __float_as_uint(v); }
  static __device__ __forceinline__ float from(type b) { return __uint_as_float(b); }
};
template <> struct BitsOf<double> {
  using type = unsigned long long;
  static constexpr type kNan = 0x7ff8000000000000ull;
  static __device__ __forceinline__ type to(double v) { return (type)__double_as_longlong(v); }
  static __device__ __forceinline__ double from(type b) { return __longlong_as_double((long long)b); }
};

// max that keeps a NaN once it has seen one (torch.max over a batch with a NaN is NaN)
template <typename T>
__device__ __forceinline__ T max_nan(T acc, T x) { return (x > acc || x != x) ? x : acc; }

template <typename T>
__device__ __forceinline__ T wave_max_nan(T v) {
  for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
  return v;
}

template <typename T>
__device__ __forceinline__ void record_violation(typename BitsOf<T>::type* slot, T v, bool active) {
  using Bt = BitsOf<T>;
  if (!active) v = T(0);
  v = wave_max_nan(v);
  if ((threadIdx.x & 63) == 0) {
    const typename Bt::type bits = v != v ? Bt::kNan : Bt::to(v);
    if (bits != 0) atomicMax(slot, bits);
  }
}

template <typename T>
__device__ __forceinline__ void stage_image(T* lds, const T* __restrict__ img, int total) {
  const int n16 = (int)(((size_t)total * sizeof(T)) / 16);
  uint4* dst = reinterpret_cast<uint4*>(lds);
  const uint4* src = reinterpret_cast<const uint4*>(img);
  for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// Residuals at p: returns max(0, every linear residual, every g_i) (NaN kept); with GRAD also the correction direction.
template <typename T, int NP, bool GRAD>
__device__ __forceinline__ T eval_point(const T* __restrict__ L, const Dims& d, const T (&p)[NP], T (&grad)[NP]) {
  T viol = T(0);
  if constexpr (GRAD) {
#pragma unroll
    for (int j = 0; j < NP; ++j) grad[j] = T(0);
  }
  const T* __restrict__ bb = L + d.off_b;
  for (int i = 0; i < d.m; ++i) {
    const T* __restrict__ a = L + (size_t)i * NP;
    T row[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) row[j] = a[j];
    T r = -bb[i];
#pragma unroll
    for (int j = 0; j < NP; ++j) r = fma(row[j], p[j], r);
    viol = max_nan(viol, r);
    if constexpr (GRAD) {
      const T rr = r > T(0) ? r + r : (r != r ? r : T(0));
#pragma unroll
      for (int j = 0; j < NP; ++j) grad[j] = fma(row[j], rr, grad[j]);
    }
  }
  for (int c = 0; c < d.nq; ++c) {
    const T* __restrict__ P = L + d.off_q + (size_t)c * d.qstride;
    const T* __restrict__ qv = P + NP * NP;
    T u[NP];
    T g2 = T(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      T acc = qv[j];
#pragma unroll
      for (int l = 0; l < NP; ++l) acc = fma(P[j * NP + l], p[l], acc);
      u[j] = acc;
      g2 = fma(p[j], acc + qv[j], g2);
    }
    const T g = fma(T(0.5), g2, qv[NP]);
    viol = max_nan(viol, g);
    if constexpr (GRAD) {
      const T gg = g > T(0) ? g + g : (g != g ? g : T(0));
#pragma unroll
      for (int j = 0; j < NP; ++j) grad[j] = fma(u[j], gg, grad[j]);
    }
  }
  return viol;
}

// pbar += lr J(p)' x   (J of the correction direction at p; see the header comment)
template <typename T, int NP>
__device__ __forceinline__ void jacobian_transpose(const T* __restrict__ L, const Dims& d, const T (&p)[NP],
                                                   const T (&x)[NP], T lr, T (&pbar)[NP]) {
  const T* __restrict__ bb = L + d.off_b;
  const T lr2 = lr + lr;
  for (int i = 0; i < d.m; ++i) {
    const T* __restrict__ a = L + (size_t)i * NP;
    T row[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) row[j] = a[j];
    T r = -bb[i], dx = T(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      r = fma(row[j], p[j], r);
      dx = fma(row[j], x[j], dx);
    }
    const T coef = r > T(0) ? lr2 * dx : T(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) pbar[j] = fma(row[j], coef, pbar[j]);
  }
  for (int c = 0; c < d.nq; ++c) {
    const T* __restrict__ P = L + d.off_q + (size_t)c * d.qstride;
    const T* __restrict__ qv = P + NP * NP;
    T u[NP];
    T g2 = T(0), w = T(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      T acc = qv[j];
#pragma unroll
      for (int l = 0; l < NP; ++l) acc = fma(P[j * NP + l], p[l], acc);
      u[j] = acc;
      g2 = fma(p[j], acc + qv[j], g2);
      w = fma(acc, x[j], w);
    }
    const T g = fma(T(0.5), g2, qv[NP]);
    if (__any(g > T(0))) {
      // 2 (relu(g) Pe' x + [g > 0] w (0.5 (Pe + Pe') p + qe)) = Pe' (2 relu(g) x + [g > 0] w p) + [g > 0] w (u + qe)
      const T cg = g > T(0) ? lr2 * g : T(0);
      const T cw = g > T(0) ? lr * w : T(0);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const T xj = fma(cg, x[j], cw * p[j]);
#pragma unroll
        for (int l = 0; l < NP; ++l) pbar[l] = fma(P[j * NP + l], xj, pbar[l]);
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) pbar[j] = fma(cw, u[j] + qv[j], pbar[j]);
    }
  }
}

template <typename T>
struct FwdArgs {
  const T* img;
  Dims d;
  const int32_t* perm;
  const T* q;
  int64_t B, ldq;
  T* y;
  int64_t ldy;
  T lr, momentum, eps;
  int max_steps;
  int chunk;                 // >= 0: run chunk `chunk`; -1: the finishing launch
  typename BitsOf<T>::type* viol;     // [max_steps + 1]
  T* state0;                 // [2 n][B] each: p then s (nullptr with a single chunk)
  T* state1;
  int32_t* tstar;
  int32_t* nan_flag;
};

template <typename T, int NP>
__global__ __launch_bounds__(kThreads) void dc3_forward_kernel(const FwdArgs<T> a) {
  extern __shared__ __align__(16) unsigned char dc3_smem[];
  __shared__ int sh_t;
  using Bt = BitsOf<T>;
  T* L = reinterpret_cast<T*>(dc3_smem);
  const Dims d = a.d;
  int chunk = a.chunk, nsteps;
  const bool record = chunk >= 0;
  if (record) {
    const int t0 = chunk * kChunk;
    // (a vote through sh_t, not __syncthreads_or: that one brings 256 bytes of static LDS of its own, which with sh_t is
    // more than kLdsBudget leaves beside the largest image)
    if (threadIdx.x == 0) sh_t = 0;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t <= t0; t += kThreads)
      if (Bt::from(a.viol[t]) < a.eps) sh_t = 1;
    __syncthreads();
    if (sh_t) return;                             // an earlier step already met the stop rule: write nothing
    nsteps = a.max_steps - t0 < kChunk ? a.max_steps - t0 : kChunk;
  } else {
    if (threadIdx.x == 0) sh_t = a.max_steps;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t < a.max_steps; t += kThreads)
      if (Bt::from(a.viol[t]) < a.eps) atomicMin(&sh_t, t);
    __syncthreads();
    const int ts = sh_t;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.tstar = ts;
    chunk = (ts - 1) / kChunk;
    const int t0 = chunk * kChunk;
    const int end = a.max_steps - t0 < kChunk ? a.max_steps : t0 + kChunk;
    if (ts == end) return;                        // that chunk's own y is the answer
    nsteps = ts - t0;
  }
  stage_image(L, a.img, d.total);
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool active = row < a.B;
  T p[NP], s[NP], grad[NP];
  const T* src = chunk == 0 ? nullptr : ((chunk & 1) ? a.state1 : a.state0);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    p[j] = T(0);
    s[j] = T(0);
    if (active && j < d.n) {
      if (src == nullptr) {
        p[j] = a.q[row * a.ldq + j];
      } else {
        p[j] = src[(int64_t)j * a.B + row];
        s[j] = src[(int64_t)(d.n + j) * a.B + row];
      }
    }
  }
  const int t0 = chunk * kChunk;
  for (int step = 0; step < nsteps; ++step) {
    const T v = eval_point<T, NP, true>(L, d, p, grad);
    if (record && step >= 1) record_violation<T>(a.viol + t0 + step, v, active);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      s[j] = a.lr * grad[j] + a.momentum * s[j];
      p[j] -= s[j];
    }
  }
  if (record) {
    const T v = eval_point<T, NP, false>(L, d, p, grad);
    record_violation<T>(a.viol + t0 + nsteps, v, active);
  }
  if (!active) return;
  if (record && t0 + nsteps < a.max_steps) {
    T* dst = (chunk & 1) ? a.state0 : a.state1;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (j < d.n) {
        dst[(int64_t)j * a.B + row] = p[j];
        dst[(int64_t)(d.n + j) * a.B + row] = s[j];
      }
    }
  }
  T* __restrict__ yr = a.y + row * a.ldy;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (j < d.n) {
      yr[a.perm[j]] = p[j];
      bad |= p[j] != p[j];
    }
  }
  for (int o = 0; o < d.no; ++o) {
    const T* __restrict__ crow = L + d.off_C + (size_t)o * NP;
    T acc = L[d.off_c0 + o];
#pragma unroll
    for (int j = 0; j < NP; ++j) acc = fma(crow[j], p[j], acc);
    yr[a.perm[d.n + o]] = acc;
    bad |= acc != acc;
  }
  if (bad && a.nan_flag != nullptr) atomicOr(a.nan_flag, 1);
}

template <typename T>
struct BwdArgs {
  const T* img;
  Dims d;
  const int32_t* perm;
  const T* q;
  int64_t B, ldq;
  const T* grad_y;
  int64_t ldg;
  T* grad_q;
  int64_t ldgq;
  T lr, momentum;
  int max_steps;
  const int32_t* tstar;
  T* traj;                   // [max_steps][n][B]
};

template <typename T, int NP>
__global__ __launch_bounds__(kThreads) void dc3_backward_kernel(const BwdArgs<T> a) {
  extern __shared__ __align__(16) unsigned char dc3_smem[];
  T* L = reinterpret_cast<T*>(dc3_smem);
  const Dims d = a.d;
  stage_image(L, a.img, d.total);
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= a.B) return;             // (no cross-lane traffic below apart from the wave-uniform vote)
  int T_steps = *a.tstar;
  if (T_steps > a.max_steps) T_steps = a.max_steps;
  T p[NP], s[NP], w[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    p[j] = j < d.n ? a.q[row * a.ldq + j] : T(0);
    s[j] = T(0);
  }
  for (int t = 0; t < T_steps; ++t) {
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (j < d.n) a.traj[((int64_t)t * d.n + j) * a.B + row] = p[j];
    if (t + 1 < T_steps) {
      (void)eval_point<T, NP, true>(L, d, p, w);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        s[j] = a.lr * w[j] + a.momentum * s[j];
        p[j] -= s[j];
      }
    }
  }
  // pbar_T = grad_y[partial] + C' grad_y[other]; s now holds sbar (zero beyond the last step)
  const T* __restrict__ gy = a.grad_y + row * a.ldg;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    w[j] = j < d.n ? gy[a.perm[j]] : T(0);
    s[j] = T(0);
  }
  for (int o = 0; o < d.no; ++o) {
    const T* __restrict__ crow = L + d.off_C + (size_t)o * NP;
    const T go = gy[a.perm[d.n + o]];
#pragma unroll
    for (int j = 0; j < NP; ++j) w[j] = fma(crow[j], go, w[j]);
  }
  // lr J(p_t)' sbar_t is summed on its own and added to pbar once per step: its m + nq n terms are small beside pbar, and
  // adding them to pbar one by one costs each of them pbar's rounding (fp32, n = 64: 1e-5 of grad_q after 45 steps)
  T dj[NP];
  for (int t = T_steps - 1; t >= 0; --t) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      s[j] = a.momentum * s[j] - w[j];
      p[j] = j < d.n ? a.traj[((int64_t)t * d.n + j) * a.B + row] : T(0);
      dj[j] = T(0);
    }
    jacobian_transpose<T, NP>(L, d, p, s, a.lr, dj);
#pragma unroll
    for (int j = 0; j < NP; ++j) w[j] += dj[j];
  }
  T* __restrict__ gq = a.grad_q + row * a.ldgq;
#pragma unroll
  for (int j = 0; j < NP; ++j)
    if (j < d.n) gq[j] = w[j];
}

template <typename T> const T* image(const RayenDc3Pack* p);
template <> const float* image<float>(const RayenDc3Pack* p) { return p->img32; }
template <> const double* image<double>(const RayenDc3Pack* p) { return p->img64; }

template <typename T>
bool served(const RayenDc3Pack* p) {
  const int max_np = sizeof(T) == 4 ? 64 : 32;      // what the kernels keep in registers
  return image<T>(p) != nullptr && p->NP <= max_np && (size_t)dims_of(p).total * sizeof(T) <= kLdsBudget - 256;
}

int n_chunks(int max_steps) { return (max_steps + kChunk - 1) / kChunk; }

// the scratch buffers (rayen_side_layout.h): what rayen_dc3_workspace_bytes reports and what the launches are handed
template <typename T>
rayen::WsLayout<3> forward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  return rayen::dc3_forward_ws(p->n, B, max_steps, n_chunks(max_steps), sizeof(T));
}

template <typename T>
rayen::WsLayout<1> backward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  return rayen::dc3_backward_ws(p->n, B, max_steps, sizeof(T));
}

template <typename T, int NP>
int launch_forward(const RayenDc3Pack* p, FwdArgs<T> a, hipStream_t stream) {
  const size_t lds = (size_t)a.d.total * sizeof(T);
  auto kern = dc3_forward_kernel<T, NP>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const unsigned grid = (unsigned)((a.B + kThreads - 1) / kThreads);
  const int chunks = n_chunks(a.max_steps);
  for (int c = 0; c <= chunks; ++c) {
    a.chunk = c < chunks ? c : -1;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, a);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename T, int NP>
int launch_backward(const RayenDc3Pack* p, const BwdArgs<T>& a, hipStream_t stream) {
  const size_t lds = (size_t)a.d.total * sizeof(T);
  auto kern = dc3_backward_kernel<T, NP>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const unsigned grid = (unsigned)((a.B + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, a);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

template <typename T>
int dc3_forward(const RayenDc3Pack* p, const T* q, int64_t B, int64_t ldq, T* y, int64_t ldy, double lr, double momentum,
                double eps, int32_t max_steps, int32_t* tstar, void* ws, int64_t ws_bytes, int32_t* nan_flag,
                void* stream) {
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || y == nullptr || ldq < p->n || ldy < p->k)) return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served<T>(p)) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<3> w = forward_ws<T>(p, B, max_steps);
  if (ws == nullptr || ws_bytes < (int64_t)w.total) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(ws, 0, w.bytes[rayen::kDc3Viol], s) != hipSuccess) return RAYEN_E_LAUNCH;
  if (B == 0) {
    // an empty batch takes no step (the reference's maximum over nothing raises)
    return hipMemsetAsync(tstar, 0, sizeof(int32_t), s) == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
  }
  FwdArgs<T> a;
  a.img = image<T>(p);
  a.d = dims_of(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.y = y; a.ldy = ldy;
  a.lr = (T)lr; a.momentum = (T)momentum; a.eps = (T)eps;
  a.max_steps = max_steps;
  a.chunk = 0;
  a.viol = w.at<typename BitsOf<T>::type>(ws, rayen::kDc3Viol);
  a.state0 = w.at<T>(ws, rayen::kDc3State0);      // (null with a single chunk)
  a.state1 = w.at<T>(ws, rayen::kDc3State1);
  a.tstar = tstar;
  a.nan_flag = nan_flag;
  return rayen::dispatch_width<kMinNP, kMaxNP>(p->NP, [&](auto NP) {
    if constexpr (sizeof(T) == 4 || NP() <= 32) return launch_forward<T, NP()>(p, a, s);
    else return (int)RAYEN_E_UNSUPPORTED;
  });
}

template <typename T>
int dc3_backward(const RayenDc3Pack* p, const T* q, int64_t B, int64_t ldq, const T* grad_y, int64_t ldg, T* grad_q,
                 int64_t ldgq, double lr, double momentum, int32_t max_steps, const int32_t* tstar, void* ws,
                 int64_t ws_bytes, void* stream) {
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || grad_y == nullptr || grad_q == nullptr || ldq < p->n || ldg < p->k || ldgq < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served<T>(p)) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<1> w = backward_ws<T>(p, B, max_steps);
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  BwdArgs<T> a;
  a.img = image<T>(p);
  a.d = dims_of(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.grad_y = grad_y; a.ldg = ldg; a.grad_q = grad_q; a.ldgq = ldgq;
  a.lr = (T)lr; a.momentum = (T)momentum;
  a.max_steps = max_steps;
  a.tstar = tstar;
  a.traj = w.at<T>(ws, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rayen::dispatch_width<kMinNP, kMaxNP>(p->NP, [&](auto NP) {
    if constexpr (sizeof(T) == 4 || NP() <= 32) return launch_backward<T, NP()>(p, a, s);
    else return (int)RAYEN_E_UNSUPPORTED;
  });
}

template <typename T>
bool upload(const RayenDc3Pack* p, const double* A1e, const double* b1e, const double* Pe, const double* qe,
            const double* re, const double* C, const double* c0, T** out) {
  const Dims d = dims_of(p);
  const int NP = p->NP, n = p->n;
  std::vector<T> h((size_t)d.total, T(0));
  for (int i = 0; i < p->m; ++i) {
    for (int j = 0; j < n; ++j) h[(size_t)i * NP + j] = static_cast<T>(A1e[(size_t)i * n + j]);
    h[(size_t)d.off_b + i] = static_cast<T>(b1e[i]);
  }
  for (int c = 0; c < p->nq; ++c) {
    T* P = h.data() + d.off_q + (size_t)c * d.qstride;
    for (int j = 0; j < n; ++j) {
      for (int l = 0; l < n; ++l) P[(size_t)j * NP + l] = static_cast<T>(Pe[((size_t)c * n + j) * n + l]);
      P[(size_t)NP * NP + j] = static_cast<T>(qe[(size_t)c * n + j]);
    }
    P[(size_t)NP * NP + NP] = static_cast<T>(re[c]);
  }
  for (int o = 0; o < p->no; ++o) {
    for (int j = 0; j < n; ++j) h[(size_t)d.off_C + (size_t)o * NP + j] = static_cast<T>(C[(size_t)o * n + j]);
    h[(size_t)d.off_c0 + o] = static_cast<T>(c0[o]);
  }
  return rayen::upload_image(h, out);
}

}  // namespace

extern "C" {

int rayen_dc3_pack_create(const double* A1e, const double* b1e, int32_t m, const double* Pe, const double* qe,
                          const double* re, int32_t nq, const double* C, const double* c0, const int32_t* partial,
                          const int32_t* other, int32_t n, int32_t k, RayenDc3Pack** out) {
  if (out == nullptr) return RAYEN_E_BAD_ARG;
  *out = nullptr;
  if (n < 1 || k < n || m < 0 || nq < 0 || partial == nullptr || (m > 0 && (A1e == nullptr || b1e == nullptr)) ||
      (nq > 0 && (Pe == nullptr || qe == nullptr || re == nullptr)) ||
      (k > n && (C == nullptr || c0 == nullptr || other == nullptr)))
    return RAYEN_E_BAD_ARG;
  for (int j = 0; j < n; ++j)
    if (partial[j] < 0 || partial[j] >= k) return RAYEN_E_BAD_ARG;
  for (int o = 0; o < k - n; ++o)
    if (other[o] < 0 || other[o] >= k) return RAYEN_E_BAD_ARG;
  int dev = -1;
  if (rayen::side_pack_device(&dev) != RAYEN_OK) return RAYEN_E_NO_DEVICE;
  RayenDc3Pack* p = new (std::nothrow) RayenDc3Pack();
  if (p == nullptr) return RAYEN_E_ALLOC;
  p->device = dev;
  p->k = k; p->n = n; p->m = m; p->nq = nq; p->no = k - n;
  p->NP = rayen::padded_width<kMinNP, kMaxNP>(n);
  *out = p;
  if (p->NP == 0) return RAYEN_OK;        // beyond what the kernels stage: every call answers RAYEN_E_UNSUPPORTED
  const Dims d = dims_of(p);
  std::vector<int32_t> perm((size_t)k);
  for (int j = 0; j < n; ++j) perm[j] = partial[j];
  for (int o = 0; o < k - n; ++o) perm[n + o] = other[o];
  bool ok = rayen::upload_image(perm, &p->perm);
  // an image that cannot fit LDS is not uploaded (the calls answer RAYEN_E_UNSUPPORTED)
  if (ok && (size_t)d.total * sizeof(float) <= kLdsBudget - 256) ok = upload<float>(p, A1e, b1e, Pe, qe, re, C, c0, &p->img32);
  if (ok && (size_t)d.total * sizeof(double) <= kLdsBudget - 256 && p->NP <= 32)
    ok = upload<double>(p, A1e, b1e, Pe, qe, re, C, c0, &p->img64);
  if (!ok) {
    rayen_dc3_pack_destroy(p);
    *out = nullptr;
    return RAYEN_E_ALLOC;
  }
  return RAYEN_OK;
}

void rayen_dc3_pack_destroy(RayenDc3Pack* p) {
  if (p == nullptr) return;
  {
    rayen::DeviceScope on_device(p->device);
    if (p->img32) (void)hipFree(p->img32);
    if (p->img64) (void)hipFree(p->img64);
    if (p->perm) (void)hipFree(p->perm);
    if (p->tile_img) (void)hipFree(p->tile_img);
    if (p->tile_img64) (void)hipFree(p->tile_img64);
  }
  delete p;
}

int64_t rayen_dc3_workspace_bytes(const RayenDc3Pack* p, int64_t B, int32_t max_steps, int32_t f64, int32_t backward) {
  if (p == nullptr || B < 0 || max_steps < 1) return -1;
  const size_t elem = f64 ? sizeof(double) : sizeof(float);
  if (backward) return (int64_t)rayen::dc3_backward_ws(p->n, B, max_steps, elem).total;
  return (int64_t)rayen::dc3_forward_ws(p->n, B, max_steps, n_chunks(max_steps), elem).total;
}

int rayen_dc3_forward_f32(const RayenDc3Pack* pack, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                          double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                          int64_t ws_bytes, int32_t* nan_flag, void* stream) {
  return dc3_forward<float>(pack, q, B, ldq, y, ldy, lr, momentum, eps, max_steps, tstar, ws, ws_bytes, nan_flag, stream);
}

int rayen_dc3_forward_f64(const RayenDc3Pack* pack, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                          double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                          int64_t ws_bytes, int32_t* nan_flag, void* stream) {
  return dc3_forward<double>(pack, q, B, ldq, y, ldy, lr, momentum, eps, max_steps, tstar, ws, ws_bytes, nan_flag, stream);
}

int rayen_dc3_backward_f32(const RayenDc3Pack* pack, const float* q, int64_t B, int64_t ldq, const float* grad_y,
                           int64_t ldg, float* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                           const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream) {
  return dc3_backward<float>(pack, q, B, ldq, grad_y, ldg, grad_q, ldgq, lr, momentum, max_steps, tstar, ws, ws_bytes,
                             stream);
}

int rayen_dc3_backward_f64(const RayenDc3Pack* pack, const double* q, int64_t B, int64_t ldq, const double* grad_y,
                           int64_t ldg, double* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                           const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream) {
  return dc3_backward<double>(pack, q, B, ldq, grad_y, ldg, grad_q, ldgq, lr, momentum, max_steps, tstar, ws, ws_bytes,
                              stream);
}

}  // extern "C"
