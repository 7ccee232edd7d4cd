// Batched Euclidean projection onto the constraint set (the core of the reference's PP / UP baselines,
// rayen/constraint_module.py:76-96 and :488-504): forward and implicit backward in exact fp32 / fp64.
//
// The program min ||z - q||^2 s.t. G z + h in K (orthant rows first, then second-order cones, t stored last) is the same
// for the whole batch; rayen_amd/projection.py assembles and equilibrates the rows, picks rho and forms
// Kinv = ((2 + sigma) I + rho G'G)^-1 once per set, in fp64 on the host.  A sample's state is (x [n], v [m]); one iteration:
//
//     p  = Pi_K(v)
//     xt = Kinv (sigma x + 2 q + w0 + rho G'(2 p - v)),      w0 = -rho G'h
//     r  = G xt + h - p
//     stop, answer xt:   max|r| <= eps (1 + max|p|)  and  max|xt - x| <= eps (1 + max|xt|)
//     x <- x + alpha (xt - x),     v <- v + alpha r
//
// starting from x = q, v = Pi_K(G q + h).  The stop is PER ROW: a row with G q + h in K answers q after 0 iterations; a row
// that reaches max_iters answers its last xt and reports iters == max_iters.  The backward runs the LINEARISED iteration
// (Pi_K replaced by its derivative at the forward's v*, h and w0 dropped, 2 g / max|g| in place of 2 q) to the same rule:
// the Jacobian of a Euclidean projection is symmetric, so its fixed point is grad_q / max|g|.
//
// Layout: one wave per sample, four samples per workgroup, workgroups stride over the batch.  G' (n x mpad, mpad odd),
// Kinv, h and w0 live in LDS, copied once per workgroup.  Lane j holds x_j (n <= 64); lane l holds rows l, l + 64, ... of
// v (R <= 9 registers).  G xt: every lane walks its rows over j, reading G'[j][row] (consecutive lanes, consecutive banks)
// and xt_j as a broadcast from the wave's LDS scratch.  G'u: lane j walks i over the m rows, reading G'[j][i] (lane stride
// mpad: odd, so conflict-free) and u_i as a broadcast.  Vector FMAs throughout; what bounds it is in DESIGN.md.
// The iterations run in launches of kChunk; between launches (x, v) of the rows still running rest in the caller's
// workspace, finished rows are skipped, a workgroup whose rows have all finished leaves before it stages the image.  No
// host sync, no grid barrier, no atomics.
//
// A set with an LMI (rayen_proj_pack_set_psd) has ONE PSD block, the last r (r + 1) / 2 rows of v, stored as svec: one row
// per (i, j) with i <= j, row-major ((0,0), (0,1), .., (0,r-1), (1,1), ..), the off-diagonal rows scaled by sqrt(2), so
// that the norm of the block is the Frobenius norm of the matrix and Pi_K on it is V max(lambda, 0) V'.  "Has a PSD block"
// is a template parameter: a set without one runs the instantiations it ran before.  The block adds per-wave LDS scratch:
// an eigenvector matrix V, a working matrix A and a second working matrix (the backward's products), each r x (r | 1),
// r eigenvalues and the (c, s) of a round's rotations.  1 <= r <= 32.
//
// Eigen-decomposition: parallel cyclic Jacobi by the wave, in LDS.  Round-robin over r' = r rounded up to even: r' - 1
// rounds per sweep, r' / 2 disjoint pairs per round (a pair with the padding index is skipped).  Per round the pair owners
// (lanes 0 .. r'/2 - 1) compute (c, s) with t = sign(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) / (2 a_pq); the
// whole wave applies the row rotations to A, then the column rotations to A and V; wave_sync() between the steps.  The
// sweep loop stops when the off-diagonal norm is <= tol ||A||_F (reduced over the wave: wave-uniform) or at kSweepCap, so
// every loop has a bounded, wave-uniform trip count whatever the data; a NaN block never meets the test, runs to the cap
// and answers NaN in its own row.  Cap and tol come from a HOST run of the same sweep (numpy, same ordering, same formulas,
// same precision) on the PSD blocks of the seeded test cases (tests/proj_lmi_reference.py: G q + h and the mirror's v* of
// every row, r = 1 .. 32): fp32, tol 1e-6 (the sweep's floor there is 2.4e-7): worst 7 sweeps -> cap 9; fp64, tol 1e-13
// (floor 4.6e-16): worst 8 sweeps -> cap 10.  The off-diagonal norm bounds the error of the rebuilt projection.
// Forward: the decomposition starts cold each iteration; a block whose eigenvalues are all >= 0 is copied (p == v bit for
// bit: the 0-iteration contract of an interior row), otherwise each lane rebuilds its own rows of V max(lambda, 0) V' as
// v - V min(lambda, 0) V' (r FMAs per row, sqrt(2) on the off-diagonals).
// Backward: v*'s block is decomposed once per launch, V and lambda stay in the scratch, and each iteration computes
// V (B o (V'HV)) V' with B_ij = 1 (both > 0), 0 (both <= 0), lambda_+ / (lambda_+ - lambda_-) (mixed; 0 counts as <= 0).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_proj_pack.h"

namespace {
constexpr int kMaxSoc = rayen::kProjMaxSoc;
constexpr int kMaxPsd = 32;                   // largest PSD block served (r x r)
}

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 32;                    // iterations per launch
constexpr int kMaxR = 9;                      // rows of v per lane
constexpr int kMaxRows = 64 * kMaxR;
constexpr int kMaxN = 64;
using rayen::kLdsBudget;                      // 256 bytes of it are left to static variables (sh_any)

struct Dims {
  int n, m, m_lin, n_soc, mpad;
  int off_K, off_h, off_w0, total, scratch;   // in elements of T; scratch: per wave
  int psd_row0, psd_dim, psd_pad, psd_mat;    // the PSD block: its first row, r, r | 1, elements of one r x (r | 1) matrix
};

inline int round4(int x) { return (x + 3) & ~3; }

Dims dims_of(const RayenProjPack* p) {
  Dims d;
  d.n = p->n; d.m = p->m; d.m_lin = p->m_lin; d.n_soc = p->n_soc;
  d.mpad = p->m | 1;
  d.off_K = round4(p->n * d.mpad);
  d.off_h = d.off_K + round4(p->n * p->n);
  d.off_w0 = d.off_h + round4(p->m);
  d.total = d.off_w0 + round4(p->n);
  d.scratch = 128 + round4(p->m);             // xt / rhs [64], cone statistics [64], u [m]
  d.psd_row0 = p->psd_row0; d.psd_dim = p->psd_dim; d.psd_pad = p->psd_dim | 1;
  d.psd_mat = round4(p->psd_dim * d.psd_pad);
  if (p->psd_dim > 0) d.scratch += 96 + 3 * d.psd_mat;      // rotations [64], lambda [32], V, A and the second work matrix
  return d;
}

size_t lds_bytes(const Dims& d, size_t elem) { return ((size_t)d.total + (size_t)kWaves * d.scratch) * elem; }

// served(): the one rule.  n in lanes, m in kMaxR registers per lane, the cones in the argument block, the PSD block at
// most kMaxPsd x kMaxPsd (its 528 svec rows count in m), the image and the waves' scratch in LDS.
bool shape_served(const RayenProjPack* p, size_t elem) {
  return p->n >= 1 && p->n <= kMaxN && p->m >= 1 && p->m <= kMaxRows && p->n_soc <= kMaxSoc && p->unclaimed == 0 &&
         p->psd_dim >= 0 && p->psd_dim <= kMaxPsd && lds_bytes(dims_of(p), elem) <= kLdsBudget - 256;
}

template <typename T> const T* image(const RayenProjPack* p);
template <> const float* image<float>(const RayenProjPack* p) { return p->img32; }
template <> const double* image<double>(const RayenProjPack* p) { return p->img64; }

template <typename T>
bool served(const RayenProjPack* p) { return image<T>(p) != nullptr && shape_served(p, sizeof(T)); }

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// LDS traffic between the lanes of ONE wave: order it for the compiler and the hardware, no workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <typename T>
struct ProjArgs {
  const T* img;
  Dims d;
  int16_t soc_row0[kMaxSoc], soc_rows[kMaxSoc];
  const T* in;               // q (forward) or g (backward), [B][ld_in]
  int64_t B, ld_in;
  T* out;                    // z or grad_q, [B][ld_out]
  int64_t ld_out;
  int32_t* iters;            // [B]: written by the forward, read by the backward
  T* vstar;                  // [B][m]: the forward's v (state between launches, v* at the end); read by the backward
  T* xs;                     // [B][n]: x between launches
  T* dvs;                    // [B][m]: the backward's v between launches
  int32_t* status;           // [B]: 1 once a row has finished
  T rho, sigma, alpha, eps;
  int max_iters, chunk;
};

// (s, t) of cone c of the vector whose rows this lane holds in v[] and whose copy is in su[]
template <typename T, int R>
__device__ __forceinline__ void cone_stats(const ProjArgs<T>& a, int c, int lane, const T (&v)[R], const T* su, T& s, T& t) {
  const int row0 = a.soc_row0[c], last = row0 + a.soc_rows[c] - 1;
  T s2 = T(0);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    s2 += (i >= row0 && i < last) ? v[r] * v[r] : T(0);
  }
  s = sqrt(wave_sum(s2));
  t = su[last];
}

// ---- the PSD block -------------------------------------------------------------------------------------------------
template <typename T> struct Jacobi;
template <> struct Jacobi<float> { static constexpr int kSweepCap = 9; static constexpr float kTol2 = 1e-12f; };
template <> struct Jacobi<double> { static constexpr int kSweepCap = 10; static constexpr double kTol2 = 1e-26; };

// idx / r for 0 <= idx < 1024, 1 <= r <= 32 (exact: (idx + 1/2) / r is at least 1 / 64 away from an integer)
__device__ __forceinline__ int div_small(int idx, float rinv) { return (int)(((float)idx + 0.5f) * rinv); }

// pair k of round s of the round-robin over nm1 + 1 players: (p, q), p < q
__device__ __forceinline__ void pair_of(int k, int s, int nm1, int& p, int& q) {
  int x = k == 0 ? nm1 : (s + k) % nm1;
  int y = k == 0 ? s : (s + nm1 - k) % nm1;
  p = x < y ? x : y;
  q = x < y ? y : x;
}

// A [r x rp] symmetric in LDS -> eigenvalues in lam[0..r), eigenvectors in the columns of V (A is destroyed).  fro2 is
// ||A||_F^2.  Called by the whole wave; ends with a wave_sync().
template <typename T>
__device__ __forceinline__ void jacobi_eig(T* __restrict__ A, T* __restrict__ V, T* __restrict__ lam, T* __restrict__ rot,
                                            int r, int rp, int lane, T fro2) {
  const float rinv = 1.0f / (float)r;
  const int rr = r * r;
  for (int idx = lane; idx < rr; idx += 64) {
    const int i = div_small(idx, rinv), j = idx - i * r;
    V[i * rp + j] = i == j ? T(1) : T(0);
  }
  wave_sync();
  const int r2 = (r + 1) & ~1, np = r2 >> 1, nm1 = r2 - 1;
  for (int sweep = 0; sweep < Jacobi<T>::kSweepCap; ++sweep) {
    T off2 = T(0);
    for (int idx = lane; idx < rr; idx += 64) {
      const int i = div_small(idx, rinv), j = idx - i * r;
      const T x = A[i * rp + j];
      off2 += i == j ? T(0) : x * x;
    }
    off2 = wave_sum(off2);
    if (off2 <= Jacobi<T>::kTol2 * fro2) break;          // (wave-uniform; false on a NaN)
    for (int s = 0; s < nm1; ++s) {
      if (lane < np) {
        int p, q;
        pair_of(lane, s, nm1, p, q);
        T c = T(1), sn = T(0);
        if (q < r) {
          const T apq = A[p * rp + q];
          if (apq != T(0)) {
            const T tau = (A[q * rp + q] - A[p * rp + p]) / (apq + apq);
            const T t = (tau >= T(0) ? T(1) : T(-1)) / (fabs(tau) + sqrt(T(1) + tau * tau));
            c = T(1) / sqrt(T(1) + t * t);
            sn = t * c;
          }
        }
        rot[2 * lane] = c;
        rot[2 * lane + 1] = sn;
      }
      wave_sync();
      // rows p and q of A <- J'A, one (pair, column) per item
      for (int idx = lane; idx < np * r; idx += 64) {
        const int k = div_small(idx, rinv), j = idx - k * r;
        int p, q;
        pair_of(k, s, nm1, p, q);
        if (q < r) {
          const T c = rot[2 * k], sn = rot[2 * k + 1];
          const T ap = A[p * rp + j], aq = A[q * rp + j];
          A[p * rp + j] = c * ap - sn * aq;
          A[q * rp + j] = sn * ap + c * aq;
        }
      }
      wave_sync();
      // columns p and q of A <- A J and of V <- V J, one (pair, row) per item
      for (int idx = lane; idx < np * r; idx += 64) {
        const int k = div_small(idx, rinv), i = idx - k * r;
        int p, q;
        pair_of(k, s, nm1, p, q);
        if (q < r) {
          const T c = rot[2 * k], sn = rot[2 * k + 1];
          const T ap = A[i * rp + p], aq = A[i * rp + q];
          A[i * rp + p] = c * ap - sn * aq;
          A[i * rp + q] = sn * ap + c * aq;
          const T vp = V[i * rp + p], vq = V[i * rp + q];
          V[i * rp + p] = c * vp - sn * vq;
          V[i * rp + q] = sn * vp + c * vq;
        }
      }
      wave_sync();
    }
  }
  if (lane < r) lam[lane] = A[lane * rp + lane];
  wave_sync();
}

template <typename T, int R, bool BWD, bool PSD>
__global__ __launch_bounds__(kThreads) void proj_kernel(const ProjArgs<T> a) {
  extern __shared__ __align__(16) unsigned char proj_smem[];
  __shared__ int sh_any;
  T* L = reinterpret_cast<T*>(proj_smem);
  const Dims d = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t groups = (a.B + kWaves - 1) / kWaves;
  if (a.chunk > 0) {
    // leave before staging anything when every row of this workgroup has finished
    if (threadIdx.x == 0) sh_any = 0;
    __syncthreads();
    for (int64_t idx = threadIdx.x;; idx += kThreads) {
      const int64_t group = blockIdx.x + (idx / kWaves) * (int64_t)gridDim.x;
      if (group >= groups) break;
      const int64_t row = group * kWaves + (idx % kWaves);
      if (row < a.B && a.status[row] == 0) sh_any = 1;
    }
    __syncthreads();
    if (sh_any == 0) return;
  }
  {
    const int n16 = (int)(((size_t)d.total * sizeof(T)) / 16);
    uint4* dst = reinterpret_cast<uint4*>(L);
    const uint4* src = reinterpret_cast<const uint4*>(a.img);
    for (int i = threadIdx.x; i < n16; i += kThreads) dst[i] = src[i];
    __syncthreads();
  }
  const T* __restrict__ Gt = L;
  const T* __restrict__ Kinv = L + d.off_K;
  const T* __restrict__ hh = L + d.off_h;
  T* sx = L + d.total + (size_t)wave * d.scratch;      // [64]
  T* sc = sx + 64;                                     // [64]: (s, t) of v* per cone (backward)
  T* su = sc + 64;                                     // [round4(m)]
  T* rot = su + ((d.m + 3) & ~3);                          // [64]: (c, s) of a round's rotations          (PSD only)
  T* lam = rot + 64;                                   // [32]: eigenvalues
  T* Vm = lam + 32;                                    // [r x rp]: eigenvectors (the backward: of v*, kept)
  T* Am = Vm + d.psd_mat;                              // [r x rp]: working matrix
  T* Tm = Am + d.psd_mat;                              // [r x rp]: second working matrix (the backward's products)
  const int pr = d.psd_dim, prp = d.psd_pad;
  const int n = d.n, m = d.m, mpad = d.mpad;
  const bool own = lane < n;
  const T w0j = (!BWD && own) ? L[d.off_w0 + lane] : T(0);
  int off[R];
  bool valid[R];
  T hr[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    valid[r] = i < m;
    off[r] = valid[r] ? i : m - 1;
    hr[r] = BWD ? T(0) : hh[off[r]];
  }
  // (i, j) of the svec rows this lane holds: i | j << 8, or -1 for a row outside the block
  int pij[PSD ? R : 1];
  if constexpr (PSD) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int rem = lane + 64 * r - d.psd_row0, i = 0;
      const bool in = rem >= 0 && valid[r];
      for (int k = 0; k < pr; ++k)
        if (rem >= pr - i) { rem -= pr - i; ++i; }
      pij[r] = in ? (i | ((i + rem) << 8)) : -1;
    }
  }
  const T kSqrt2 = T(1.4142135623730951), kRsqrt2 = T(0.7071067811865476);
  // Am = smat of the block of the vector in w[]; returns ||block||^2 (= ||Am||_F^2)
  auto psd_smat = [&](const T (&w)[R]) -> T {
    T part = T(0);
    if constexpr (PSD) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (pij[r] >= 0) {
          const int i = pij[r] & 255, j = pij[r] >> 8;
          const T x = i == j ? w[r] : w[r] * kRsqrt2;
          Am[i * prp + j] = x;
          Am[j * prp + i] = x;
          part += w[r] * w[r];
        }
      part = wave_sum(part);
    }
    return part;
  };
  const int t0 = a.chunk * kChunk;
  const int t_end = a.max_iters - t0 < kChunk ? a.max_iters : t0 + kChunk;

  for (int64_t group = blockIdx.x; group < groups; group += gridDim.x) {
    const int64_t row = group * kWaves + wave;
    if (row >= a.B) break;                             // (wave-uniform; no workgroup barrier below)
    if (a.chunk > 0 && a.status[row] != 0) continue;
    const T inj = own ? a.in[row * a.ld_in + lane] : T(0);
    T x, rhs2, scale = T(1);
    T v[R], vs[R], p[R], acc[R];
    if constexpr (BWD) {
      scale = wave_max(fabs(inj));
      if (a.chunk == 0 && (a.iters[row] == 0 || !(scale > T(0)))) {
        // the row was inside (J = I), or its gradient is zero (or NaN: handed on)
        if (own) a.out[row * a.ld_out + lane] = inj;
        if (lane == 0) a.status[row] = 1;
        continue;
      }
      rhs2 = (inj / scale) * T(2);
#pragma unroll
      for (int r = 0; r < R; ++r) vs[r] = valid[r] ? a.vstar[row * m + off[r]] : T(0);
      // (s, t) of v* per cone: the same in every iteration
      wave_sync();
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (valid[r]) su[off[r]] = vs[r];
      wave_sync();
      for (int c = 0; c < d.n_soc; ++c) {
        T s, t;
        cone_stats<T, R>(a, c, lane, vs, su, s, t);
        if (lane == 0) { sc[2 * c] = s; sc[2 * c + 1] = t; }
      }
      wave_sync();
      if constexpr (PSD) {
        // V and lambda of v*'s block: kept for every iteration of this launch
        const T fro2 = psd_smat(vs);
        wave_sync();
        jacobi_eig<T>(Am, Vm, lam, rot, pr, prp, lane, fro2);
      }
    } else {
      rhs2 = inj * T(2);
    }

    // p = Pi_K(v) (forward) or D Pi_K(v*) v (backward) of the vector in v[]; su is overwritten
    auto cone_op = [&]() {
      wave_sync();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (valid[r]) su[off[r]] = v[r];
        if constexpr (BWD) p[r] = vs[r] > T(0) ? v[r] : T(0);
        else p[r] = fmax(v[r], T(0));
      }
      wave_sync();
      for (int c = 0; c < d.n_soc; ++c) {
        const int row0 = a.soc_row0[c], last = row0 + a.soc_rows[c] - 1;
        if constexpr (!BWD) {
          T s, t;
          cone_stats<T, R>(a, c, lane, v, su, s, t);
          const bool inside = s <= t, zero = s <= -t;
          const T half = T(0.5) * (s + t);
          const T coef = inside ? T(1) : (zero ? T(0) : half / s);
          const T tout = inside ? t : (zero ? T(0) : half);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i >= row0 && i < last) p[r] = coef * v[r];
            if (i == last) p[r] = tout;
          }
        } else {
          const T s = sc[2 * c], t = sc[2 * c + 1];
          const bool inside = s <= t, zero = s <= -t;
          const T inv = s > T(0) ? T(1) / s : T(0);
          T part = T(0);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            part += (i >= row0 && i < last) ? vs[r] * v[r] : T(0);
          }
          const T xd = wave_sum(part) * inv;           // xhat . dx
          const T dt = su[last];
          const T da = T(0.5) * (xd + dt);
          const T ratio = T(0.5) * (s + t) * inv;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            const T xh = vs[r] * inv;
            const T mid = da * xh + ratio * (v[r] - xh * xd);
            if (i >= row0 && i < last) p[r] = inside ? v[r] : (zero ? T(0) : mid);
            if (i == last) p[r] = inside ? dt : (zero ? T(0) : da);
          }
        }
      }
      if constexpr (PSD) {
        const T fro2 = psd_smat(v);
        wave_sync();
        if constexpr (!BWD) {
          jacobi_eig<T>(Am, Vm, lam, rot, pr, prp, lane, fro2);
          const bool bad = lane < pr && !(lam[lane] >= T(0));
          if (__any(bad)) {
            // this lane's rows of V max(lambda, 0) V', taken as v - V min(lambda, 0) V': the same matrix, but what the
            // sweep's rounding (V'V - I is 3e-6 at r = 20 in fp32) multiplies is the negative part alone, not ||A||; with
            // the sum over the positive part the fp32 iteration at r >= 20 jitters above its stop rule and never ends
#pragma unroll
            for (int r = 0; r < R; ++r)
              if (pij[r] >= 0) {
                const int i = pij[r] & 255, j = pij[r] >> 8;
                T sum = T(0);
                for (int k = 0; k < pr; ++k) sum = fma(Vm[i * prp + k] * fmax(-lam[k], T(0)), Vm[j * prp + k], sum);
                p[r] = v[r] + (i == j ? sum : sum * kSqrt2);
              }
          } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
              if (pij[r] >= 0) p[r] = v[r];
          }
        } else {
          // V (B o (V'HV)) V' with H = Am: Tm = V'H, Am = B o (Tm V), Tm = V Am, rows of Tm V'
          const float rinv = 1.0f / (float)pr;
          const int rr = pr * pr;
          for (int idx = lane; idx < rr; idx += 64) {
            const int i = div_small(idx, rinv), j = idx - i * pr;
            T sum = T(0);
            for (int k = 0; k < pr; ++k) sum = fma(Vm[k * prp + i], Am[k * prp + j], sum);
            Tm[i * prp + j] = sum;
          }
          wave_sync();
          for (int idx = lane; idx < rr; idx += 64) {
            const int i = div_small(idx, rinv), j = idx - i * pr;
            T sum = T(0);
            for (int k = 0; k < pr; ++k) sum = fma(Tm[i * prp + k], Vm[k * prp + j], sum);
            const T li = lam[i], lj = lam[j];
            const bool pi = li > T(0), pj = lj > T(0);
            const T hi = fmax(li, lj), lo = fmin(li, lj);
            const T b = (pi && pj) ? T(1) : ((pi != pj) ? hi / (hi - lo) : T(0));
            Am[i * prp + j] = (li == li && lj == lj) ? b * sum : li + lj;          // (a NaN eigenvalue is handed on)
          }
          wave_sync();
          for (int idx = lane; idx < rr; idx += 64) {
            const int i = div_small(idx, rinv), j = idx - i * pr;
            T sum = T(0);
            for (int k = 0; k < pr; ++k) sum = fma(Vm[i * prp + k], Am[k * prp + j], sum);
            Tm[i * prp + j] = sum;
          }
          wave_sync();
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (pij[r] >= 0) {
              const int i = pij[r] & 255, j = pij[r] >> 8;
              T sum = T(0);
              for (int k = 0; k < pr; ++k) sum = fma(Tm[i * prp + k], Vm[j * prp + k], sum);
              p[r] = i == j ? sum : sum * kSqrt2;
            }
        }
      }
    };

    // acc[r] = (G s)[row r] for the vector s in sx[0..n)
    auto times_G = [&]() {
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = T(0);
      for (int j = 0; j < n; ++j) {
        const T sj = sx[j];
        const T* __restrict__ g = Gt + (size_t)j * mpad;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma(g[off[r]], sj, acc[r]);
      }
    };

    if (a.chunk == 0) {
      x = BWD ? inj / scale : inj;
      wave_sync();
      sx[lane] = x;
      wave_sync();
      times_G();
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = valid[r] ? acc[r] + hr[r] : T(0);
      cone_op();
      if constexpr (!BWD) {
        bool same = true;
#pragma unroll
        for (int r = 0; r < R; ++r) same = same && (!valid[r] || p[r] == v[r]);
        if (__all(same)) {
          // G q + h in K: the row is inside and answers q
          if (own) a.out[row * a.ld_out + lane] = inj;
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (valid[r]) a.vstar[row * m + off[r]] = v[r];
          if (lane == 0) { a.iters[row] = 0; a.status[row] = 1; }
          continue;
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = p[r];
    } else {
      x = own ? a.xs[row * n + lane] : T(0);
      const T* __restrict__ vsrc = BWD ? a.dvs : a.vstar;
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = valid[r] ? vsrc[row * m + off[r]] : T(0);
    }

    bool finished = false;
    for (int t = t0 + 1; t <= t_end; ++t) {
      cone_op();
      wave_sync();
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (valid[r]) su[off[r]] = (p[r] + p[r]) - v[r];
      wave_sync();
      // w = (G'u)_lane
      T w = T(0);
      if (own) {
        const T* __restrict__ g = Gt + (size_t)lane * mpad;
        T w1 = T(0), w2 = T(0), w3 = T(0);
        int i = 0;
        for (; i + 4 <= m; i += 4) {
          w = fma(g[i], su[i], w);
          w1 = fma(g[i + 1], su[i + 1], w1);
          w2 = fma(g[i + 2], su[i + 2], w2);
          w3 = fma(g[i + 3], su[i + 3], w3);
        }
        for (; i < m; ++i) w = fma(g[i], su[i], w);
        w = (w + w1) + (w2 + w3);
      }
      sx[lane] = own ? fma(a.rho, w, fma(a.sigma, x, rhs2 + w0j)) : T(0);
      wave_sync();
      T xt = T(0);
      if (own) {
        T x1 = T(0);
        int l = 0;
        for (; l + 2 <= n; l += 2) {
          xt = fma(Kinv[l * n + lane], sx[l], xt);
          x1 = fma(Kinv[(l + 1) * n + lane], sx[l + 1], x1);
        }
        if (l < n) xt = fma(Kinv[l * n + lane], sx[l], xt);
        xt += x1;
      }
      wave_sync();
      sx[lane] = xt;
      wave_sync();
      times_G();
      T r1 = T(0), pm = T(0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r] = valid[r] ? (acc[r] + hr[r]) - p[r] : T(0);
        r1 = fmax(r1, fabs(acc[r]));
        pm = fmax(pm, valid[r] ? fabs(p[r]) : T(0));
      }
      const T dx = xt - x;
      r1 = wave_max(r1);
      pm = wave_max(pm);
      const T r2 = wave_max(fabs(dx)), xm = wave_max(fabs(xt));
      const bool conv = r1 <= a.eps * (T(1) + pm) && r2 <= a.eps * (T(1) + xm);
      if (conv || t == a.max_iters) {
        if (own) a.out[row * a.ld_out + lane] = BWD ? xt * scale : xt;
        if constexpr (!BWD) {
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (valid[r]) a.vstar[row * m + off[r]] = v[r];
          if (lane == 0) a.iters[row] = t;
        }
        if (lane == 0) a.status[row] = 1;
        finished = true;
        break;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = fma(a.alpha, acc[r], v[r]);
      x = fma(a.alpha, dx, x);
    }
    if (!finished) {
      if (own) a.xs[row * n + lane] = x;
      T* __restrict__ vdst = BWD ? a.dvs : a.vstar;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (valid[r]) vdst[row * m + off[r]] = v[r];
      if (a.chunk == 0 && lane == 0) a.status[row] = 0;
    }
  }
}

template <typename T, int R, bool BWD, bool PSD>
int launch_as(const RayenProjPack* p, ProjArgs<T> a, hipStream_t stream) {
  const size_t lds = lds_bytes(a.d, sizeof(T));
  auto kern = proj_kernel<T, R, BWD, PSD>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const int64_t groups = (a.B + kWaves - 1) / kWaves;
  int64_t per_cu = (int64_t)(kLdsBudget / (lds + 256));
  per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
  const unsigned grid = (unsigned)(groups < 256 * per_cu ? groups : 256 * per_cu);
  const int chunks = (a.max_iters + kChunk - 1) / kChunk;
  for (int c = 0; c < chunks; ++c) {
    a.chunk = c;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, a);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename T, int R, bool BWD>
int launch(const RayenProjPack* p, ProjArgs<T> a, hipStream_t stream) {
  return p->psd_dim > 0 ? launch_as<T, R, BWD, true>(p, a, stream) : launch_as<T, R, BWD, false>(p, a, stream);
}

template <typename T, bool BWD>
int run(const RayenProjPack* p, const T* in, int64_t B, int64_t ld_in, T* out, int64_t ld_out, int32_t* iters, T* vstar,
        double eps, int32_t max_iters, void* ws, int64_t ws_bytes, void* stream) {
  if (p == nullptr || B < 0 || max_iters < 1 || !(eps >= 0.0)) return RAYEN_E_BAD_ARG;
  if (B > 0 && (in == nullptr || out == nullptr || iters == nullptr || vstar == nullptr || ld_in < p->n || ld_out < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) / kMaxRows) return RAYEN_E_BAD_ARG;
  if (!served<T>(p)) return RAYEN_E_UNSUPPORTED;
  // the scratch buffer (rayen_side_layout.h): what rayen_proj_workspace_bytes reports and what the launches are handed
  const rayen::WsLayout<3> w = rayen::proj_ws(p->n, p->m, B, BWD, sizeof(T));
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  ProjArgs<T> a;
  a.img = image<T>(p);
  a.d = dims_of(p);
  std::memcpy(a.soc_row0, p->soc_row0, sizeof(a.soc_row0));
  std::memcpy(a.soc_rows, p->soc_rows, sizeof(a.soc_rows));
  a.in = in; a.B = B; a.ld_in = ld_in; a.out = out; a.ld_out = ld_out; a.iters = iters; a.vstar = vstar;
  a.xs = w.at<T>(ws, rayen::kProjXs);
  a.status = w.at<int32_t>(ws, rayen::kProjStatus);
  a.dvs = w.at<T>(ws, rayen::kProjDvs);              // (null in the forward)
  a.rho = (T)p->rho; a.sigma = (T)p->sigma; a.alpha = (T)p->alpha; a.eps = (T)eps;
  a.max_iters = max_iters;
  a.chunk = 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->m <= 64) return launch<T, 1, BWD>(p, a, s);
  if (p->m <= 192) return launch<T, 3, BWD>(p, a, s);
  return launch<T, kMaxR, BWD>(p, a, s);
}

template <typename T>
bool upload(const RayenProjPack* p, const double* G, const double* h, const double* Kinv, const double* w0, T** out) {
  const Dims d = dims_of(p);
  std::vector<T> img((size_t)d.total, T(0));
  for (int i = 0; i < p->m; ++i) {
    for (int j = 0; j < p->n; ++j) img[(size_t)j * d.mpad + i] = static_cast<T>(G[(size_t)i * p->n + j]);
    img[(size_t)d.off_h + i] = static_cast<T>(h[i]);
  }
  for (int j = 0; j < p->n; ++j) {
    for (int l = 0; l < p->n; ++l) img[(size_t)d.off_K + (size_t)j * p->n + l] = static_cast<T>(Kinv[(size_t)j * p->n + l]);
    img[(size_t)d.off_w0 + j] = static_cast<T>(w0[j]);
  }
  return rayen::upload_image(img, out);
}

}  // namespace

extern "C" {

int rayen_proj_pack_create(const double* G, const double* h, const double* Kinv, const double* w0, int32_t n, int32_t m,
                           int32_t m_lin, const int32_t* soc_rows, int32_t n_soc, double rho, double sigma, double alpha,
                           RayenProjPack** out) {
  if (out == nullptr) return RAYEN_E_BAD_ARG;
  *out = nullptr;
  if (n < 1 || m < 1 || m_lin < 0 || m_lin > m || n_soc < 0 || G == nullptr || h == nullptr || Kinv == nullptr ||
      w0 == nullptr || (n_soc > 0 && soc_rows == nullptr) || !(rho > 0.0) || !(sigma >= 0.0) || !(alpha > 0.0 && alpha < 2.0))
    return RAYEN_E_BAD_ARG;
  int64_t rows = m_lin;
  for (int c = 0; c < n_soc; ++c) {
    if (soc_rows[c] < 1) return RAYEN_E_BAD_ARG;
    rows += soc_rows[c];
  }
  if (rows > m) return RAYEN_E_BAD_ARG;        // rows < m: the rest is a PSD block that rayen_proj_pack_set_psd claims
  int dev = -1;
  if (rayen::side_pack_device(&dev) != RAYEN_OK) return RAYEN_E_NO_DEVICE;
  RayenProjPack* p = new (std::nothrow) RayenProjPack();
  if (p == nullptr) return RAYEN_E_ALLOC;
  p->device = dev;
  p->n = n; p->m = m; p->m_lin = m_lin; p->n_soc = n_soc;
  p->rho = rho; p->sigma = sigma; p->alpha = alpha;
  p->psd_row0 = m;
  *out = p;
  // the tile kernel's images (rayen_proj_tile.hip): where its envelope holds and no row is left for a PSD block
  if (rows == m) p->tile = rayen::proj_tile_create(G, h, Kinv, w0, n, m, m_lin, soc_rows, n_soc);
  if (n > kMaxN || m > kMaxRows || n_soc > kMaxSoc) {                     // not staged: every call answers RAYEN_E_UNSUPPORTED
    p->unclaimed = (int)(m - rows);
    return RAYEN_OK;
  }
  int at = m_lin;
  for (int c = 0; c < n_soc; ++c) {
    p->soc_row0[c] = (int16_t)at;
    p->soc_rows[c] = (int16_t)soc_rows[c];
    at += soc_rows[c];
  }
  bool ok = true;
  if (shape_served(p, sizeof(float))) ok = upload<float>(p, G, h, Kinv, w0, &p->img32);
  if (ok && shape_served(p, sizeof(double))) ok = upload<double>(p, G, h, Kinv, w0, &p->img64);
  if (!ok) {
    rayen_proj_pack_destroy(p);
    *out = nullptr;
    return RAYEN_E_ALLOC;
  }
  p->unclaimed = (int)(m - rows);                // (> 0: not served until rayen_proj_pack_set_psd claims the block)
  return RAYEN_OK;
}

int rayen_proj_pack_set_psd(RayenProjPack* p, int32_t row0, int32_t r) {
  if (p == nullptr || r < 1 || r > 32767 || p->psd_dim != 0 || p->unclaimed == 0 || row0 != p->m - p->unclaimed ||
      (int64_t)r * (r + 1) / 2 != p->unclaimed)
    return RAYEN_E_BAD_ARG;
  p->psd_row0 = row0;
  p->psd_dim = r;
  p->unclaimed = 0;
  // the block's scratch counts against the LDS budget: an image that no longer fits is dropped (RAYEN_E_UNSUPPORTED)
  rayen::DeviceScope on_device(p->device);
  if (p->img32 && !shape_served(p, sizeof(float))) { (void)hipFree(p->img32); p->img32 = nullptr; }
  if (p->img64 && !shape_served(p, sizeof(double))) { (void)hipFree(p->img64); p->img64 = nullptr; }
  return RAYEN_OK;
}

void rayen_proj_pack_destroy(RayenProjPack* p) {
  if (p == nullptr) return;
  {
    rayen::DeviceScope on_device(p->device);
    if (p->img32) (void)hipFree(p->img32);
    if (p->img64) (void)hipFree(p->img64);
    rayen::proj_tile_destroy(p->tile);
    rayen::proj_tile64_destroy(p->tile64);
  }
  delete p;
}

int64_t rayen_proj_workspace_bytes(const RayenProjPack* p, int64_t B, int32_t f64, int32_t backward) {
  if (p == nullptr || B < 0) return -1;
  return (int64_t)rayen::proj_ws(p->n, p->m, B, backward != 0, f64 ? sizeof(double) : sizeof(float)).total;
}

int rayen_proj_forward_f32(const RayenProjPack* pack, const float* q, int64_t B, int64_t ldq, float* z, int64_t ldz,
                           int32_t* iters, float* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                           void* stream) {
  return run<float, false>(pack, q, B, ldq, z, ldz, iters, vstar, eps, max_iters, ws, ws_bytes, stream);
}

int rayen_proj_forward_f64(const RayenProjPack* pack, const double* q, int64_t B, int64_t ldq, double* z, int64_t ldz,
                           int32_t* iters, double* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                           void* stream) {
  return run<double, false>(pack, q, B, ldq, z, ldz, iters, vstar, eps, max_iters, ws, ws_bytes, stream);
}

int rayen_proj_backward_f32(const RayenProjPack* pack, const float* g, int64_t B, int64_t ldg, const float* vstar,
                            const int32_t* iters, float* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                            int64_t ws_bytes, void* stream) {
  return run<float, true>(pack, g, B, ldg, grad_q, ldgq, const_cast<int32_t*>(iters), const_cast<float*>(vstar), eps,
                          max_iters, ws, ws_bytes, stream);
}

int rayen_proj_backward_f64(const RayenProjPack* pack, const double* g, int64_t B, int64_t ldg, const double* vstar,
                            const int32_t* iters, double* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                            int64_t ws_bytes, void* stream) {
  return run<double, true>(pack, g, B, ldg, grad_q, ldgq, const_cast<int32_t*>(iters), const_cast<double*>(vstar), eps,
                           max_iters, ws, ws_bytes, stream);
}

}  // extern "C"
