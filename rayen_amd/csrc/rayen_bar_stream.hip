// method='Bar' for packs whose image of G = NA_E [V R] does NOT fit LDS (rayen_bar.hip serves the ones that do), and,
// on request, for those that do: the image stays in global memory, where the pack has it, and a workgroup brings it through
// two LDS buffers in WINDOWS (rayen_bar_stream_layout.h: whole groups of four generators, a contiguous slice of the image)
// while its lanes keep their rows' state in registers -- the forward the online max M, the sum s and acc[K], the backward s
// and <lambda, g>.  Geometry and arithmetic are the resident kernels': L lanes share a row, lane li owns the row's pieces
// li, li + L, ... (of the forward's ray pieces pr + li, pr + li + L, ..., as the resident ray loop deals them), and of the
// window in LDS it processes those of its pieces that fall inside, in ascending order.  Every
// lane therefore sees the same operations on the same operands in the same order as in bar_forward_kernel /
// bar_backward_kernel, and y, rowstat and grad_q are the resident kernels' bit for bit wherever both serve a pack.
//
// Sequence.  One pass over a workgroup's rows is a sequence of STEPS, each one window (rayen_bar_stream_layout.h):
//     forward:  the windows of the vertex pieces | the group's max and sum, the vertex part scaled | the windows of the ray pieces
//     backward: the windows of the vertex pieces | the group's sum and <lambda, g> | every window from 0, grad_q written
// A step whose window is the previous step's (the mixed vertex / ray piece's window, a set of one window) copies nothing.
//
// Buffers.  Two, of the largest window's size (one when the set is a single window, which then stays).  Per step:
//     s_waitcnt vmcnt(0); barrier      -- this step's window has landed (every thread waited for its own part of the copy),
//                                         and every wave is done with the previous step
//     copy of the next step's window -> the other buffer, which nobody reads any more
//     walk of this step's window
// The copy is LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes land at consecutive LDS addresses), the protocol of
// rayen_cost_stream.hip.  q arrives through ordinary loads, and the compiler waits vmcnt(0) at the first use of such a load:
// the part of the next window's copy issued in front of it is waited for there, not hidden under the walk.
//
// Rows.  A lane group carries R rows at once (R sets of accumulators, R rows of q in flight), so a workgroup reads the image
// once per (512 / L) R rows: bar_stream_rows_per_pass.  R per K and precision: bar_stream_rows.
//
// Uniformity.  The loops over passes and over steps have workgroup-uniform trip counts: every wave takes every barrier and
// issues its share of every copy.  A lane group whose rows are all >= B loads and stores nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "rayen_bar_pack.h"
#include "rayen_bar_stream_layout.h"

namespace {

using namespace rayen::bar;
using rayen::BarStreamSeq;
using rayen::kBarStreamYpBytes;

static_assert(rayen::kBarStreamLds == (int64_t)rayen::kLdsBudget, "rayen_bar_stream_layout.h restates the LDS budget");
static_assert(rayen::kBarStreamThreads == kThreads, "rayen_bar_stream_layout.h restates the workgroup size");
static_assert(kMaxK * 8 <= kBarStreamYpBytes, "yp's slot holds K doubles");

// this wave's share of a window's copy: chunks of 1 KiB (64 lanes x 16 bytes), dealt over the waves; the lanes past the
// window's end fetch nothing (and nothing lands at their LDS addresses)
__device__ __forceinline__ void stream_copy(const uint4* __restrict__ src, const int n16, unsigned char* dst, const int wave,
                                            const int lane) {
  const int n_chunks = (n16 + 63) >> 6;
  for (int c = wave; c < n_chunks; c += kThreads / 64) {
    const int p = c * 64 + lane;
    if (p < n16)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + p),
                                       (__attribute__((address_space(3))) void*)(dst + (size_t)c * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ void stream_landed() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// what a kernel knows of the windows: g groups of four generators each, `n16` 16-byte pieces a group
struct Windows {
  const uint4* img;
  int g, npieces, group16;
  __device__ __forceinline__ const uint4* src(const int w) const { return img + (size_t)w * g * group16; }
  __device__ __forceinline__ int n16(const int w) const {
    const int left = npieces - w * g;
    return (left < g ? left : g) * group16;
  }
};

// The copy protocol of a workgroup, stated once for both kernels.  `start` issues the first step's copy; `begin(step, w,
// again)` opens a step: its window w has landed and every wave is done with the previous step; the next step's window
// (the next pass's first where this is the pass's last and `again` says there is a next pass) goes into the other buffer
// unless it is the one at hand.  Returns where the window at hand starts, in 16-byte pieces of the workgroup's LDS.
struct Steps {
  Windows win;
  BarStreamSeq seq;
  unsigned char* bufs;
  int nsteps, buf_bytes, wave, lane;
  int cur;      // the buffer of the step at hand
  __device__ __forceinline__ void start() {
    cur = 0;
    const int w0 = rayen::bar_stream_seq_window(seq, 0);
    stream_copy(win.src(w0), win.n16(w0), bufs, wave, lane);
  }
  __device__ __forceinline__ int begin(const int step, const int w, const bool again) {
    const int wn = rayen::bar_stream_seq_window(seq, step + 1 < nsteps ? step + 1 : 0);
    stream_landed();
    const int at = (int)(kBarStreamYpBytes >> 4) + cur * (buf_bytes >> 4);
    if ((step + 1 < nsteps || again) && wn != w) {
      cur ^= 1;
      stream_copy(win.src(wn), win.n16(wn), bufs + (size_t)cur * buf_bytes, wave, lane);
    }
    return at;
  }
};

// a window in LDS, `at16` 16-byte pieces into the workgroup's LDS: yp's slot and every window are whole 16-byte pieces, and
// the offset is formed so that the compiler sees it (it then reads a generator's coefficients 16 bytes at a time,
// ds_read_b128, as the resident kernels do; from a byte offset it cannot see through it reads 4 or 8 at a time)
template <typename T>
__device__ __forceinline__ const T* window_base(const unsigned char* smem, const int at16) {
  return reinterpret_cast<const T*>(smem + ((size_t)at16 << 4));
}

// the lane's first piece >= lo (its pieces are li, li + L, ...)
__device__ __forceinline__ int first_piece(const int lo, const int li, const int L) { return lo + ((li - lo) & (L - 1)); }

template <typename T, int K, int R>
__global__ __launch_bounds__(kThreads) void bar_stream_forward_kernel(const T* __restrict__ img, const int nv, const int m,
                                                                      const int lgL, const int g, const int buf_bytes,
                                                                      const T* __restrict__ q, const int64_t B,
                                                                      const int64_t ldq, const int vec, T* __restrict__ y,
                                                                      const int64_t ldy, const int k, T* __restrict__ rowstat,
                                                                      int32_t* __restrict__ nan_flag) {
  extern __shared__ __align__(16) unsigned char bar_stream_smem[];
  const T* yp = reinterpret_cast<const T*>(bar_stream_smem);
  unsigned char* bufs = bar_stream_smem + kBarStreamYpBytes;
  const int L = 1 << lgL;
  const int li = threadIdx.x & (L - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_iter = kThreads >> lgL;
  const int npieces = (m + 3) >> 2;
  const int pv = (nv + 3) >> 2;          // pieces that hold vertex columns
  const int pr = nv >> 2;                // first piece that holds a ray column
  const T ninf = -static_cast<T>(INFINITY);
  const BarStreamSeq seq = rayen::bar_stream_forward_seq(nv, m, g);
  const int nsteps = rayen::bar_stream_seq_steps(seq);
  const Windows win{reinterpret_cast<const uint4*>(img), g, npieces, (int)(4 * K * sizeof(T) / 16)};
  const int64_t rows_per_pass = (int64_t)rows_per_iter * R;
  const int64_t n_pass = (B + rows_per_pass - 1) / rows_per_pass;

  if ((int64_t)blockIdx.x >= n_pass) return;      // (workgroup-uniform: no barrier is left behind)
  if (threadIdx.x < K) reinterpret_cast<T*>(bar_stream_smem)[threadIdx.x] = img[(size_t)((m + 3) & ~3) * K + threadIdx.x];
  Steps steps{win, seq, bufs, nsteps, buf_bytes, wave, lane, 0};
  steps.start();
  for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
    const int64_t row0 = pass * rows_per_pass + (threadIdx.x >> lgL);
    const bool again = pass + gridDim.x < n_pass;
    bool live[R];
    const T* __restrict__ qr[R];
    T acc[R][K], M[R], s[R], lse[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + (int64_t)r * rows_per_iter;
      live[r] = row < B;
      qr[r] = q + (live[r] ? row : 0) * ldq;
#pragma unroll
      for (int i = 0; i < K; ++i) acc[r][i] = T(0);
      M[r] = ninf;
      s[r] = T(0);
      lse[r] = T(0);
    }
    int step = 0;
    for (; step < seq.first_end; ++step) {      // the windows of the vertex pieces
      const int w = rayen::bar_stream_seq_window(seq, step);
      const T* __restrict__ G = window_base<T>(bar_stream_smem, steps.begin(step, w, again));
      const int slot0 = 4 * w * g;      // the window's generators: image rows [4 w g, ...) at G
      const int w_hi = (w + 1) * g < pv ? (w + 1) * g : pv;
      for (int p = first_piece(w * g, li, L); p < w_hi; p += L) {
        T v[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (live[r]) load4(qr[r] + 4 * p, vec != 0, m - 4 * p, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!live[r]) continue;
          T pm = ninf;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * p + c < nv) pm = fmax(pm, v[r][c]);
          if (pm > M[r]) {                    // online max: rescale only when it grows
            const T f = exp_(M[r] - pm);
            s[r] *= f;
#pragma unroll
            for (int i = 0; i < K; ++i) acc[r][i] *= f;
            M[r] = pm;
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = 4 * p + c;
            if (j < nv) {
              // (a -inf logit weighs 0, as in torch's softmax, also while this lane's max is still -inf)
              const T wgt = v[r][c] == ninf ? T(0) : exp_(v[r][c] - M[r]);
              s[r] += wgt;
              const T* __restrict__ gj = G + (size_t)(gen_slot(j) - slot0) * K;
#pragma unroll
              for (int i = 0; i < K; ++i) acc[r][i] = fma(gj[i], wgt, acc[r][i]);
            }
          }
        }
      }
    }
    if (nv > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!live[r]) continue;
        const T Mg = group_max(M[r], L);
        const T f = M[r] == ninf ? T(0) : exp_(M[r] - Mg);
        const T S = group_sum(s[r] * f, L);
        const T scale = f / S;
#pragma unroll
        for (int i = 0; i < K; ++i) acc[r][i] *= scale;
        lse[r] = Mg + log_(S);
      }
    }
    for (; step < nsteps; ++step) {      // the windows of the ray pieces
      const int w = rayen::bar_stream_seq_window(seq, step);
      const T* __restrict__ G = window_base<T>(bar_stream_smem, steps.begin(step, w, again));
      const int slot0 = 4 * w * g;
      const int w_lo = w * g > pr ? w * g : pr, w_hi = (w + 1) * g < npieces ? (w + 1) * g : npieces;
      // (the resident kernel's ray loop starts at piece pr + li: of the ray pieces lane li owns pr + li, pr + li + L, ...)
      for (int p = first_piece(w_lo, (pr + li) & (L - 1), L); p < w_hi; p += L) {
        T v[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (live[r]) load4(qr[r] + 4 * p, vec != 0, m - 4 * p, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!live[r]) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = 4 * p + c;
            if (j >= nv && j < m) {
              const T wgt = fabs(v[r][c]);
              const T* __restrict__ gj = G + (size_t)(gen_slot(j) - slot0) * K;
#pragma unroll
              for (int i = 0; i < K; ++i) acc[r][i] = fma(gj[i], wgt, acc[r][i]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
      if (L > 1) {
#pragma unroll
        for (int i = 0; i < K; ++i) acc[r][i] = group_sum(acc[r][i], L);
      }
      const int64_t row = row0 + (int64_t)r * rows_per_iter;
      T* __restrict__ yr = y + row * ldy;
      bool bad = false;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        if (i < k && (i & (L - 1)) == li) {
          const T out = acc[r][i] + yp[i];
          yr[i] = out;
          bad |= out != out;
        }
      }
      if (rowstat != nullptr && li == 0) rowstat[row] = lse[r];
      if (bad && nan_flag != nullptr) atomicOr(nan_flag, 1);
    }
  }
}

template <typename T, int K, int R>
__global__ __launch_bounds__(kThreads) void bar_stream_backward_kernel(const T* __restrict__ img, const int nv, const int m,
                                                                       const int lgL, const int g, const int buf_bytes,
                                                                       const T* __restrict__ q, const int64_t B,
                                                                       const int64_t ldq, const int vec_in, const int vec_out,
                                                                       const T* __restrict__ rowstat,
                                                                       const T* __restrict__ grad_y, const int k,
                                                                       T* __restrict__ grad_q) {
  extern __shared__ __align__(16) unsigned char bar_stream_smem[];
  unsigned char* bufs = bar_stream_smem + kBarStreamYpBytes;      // (yp's slot stays unused: one LDS layout for both kernels)
  const int L = 1 << lgL;
  const int li = threadIdx.x & (L - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_iter = kThreads >> lgL;
  const int npieces = (m + 3) >> 2;
  const int pv = (nv + 3) >> 2;
  const BarStreamSeq seq = rayen::bar_stream_backward_seq(nv, m, g);
  const int nsteps = rayen::bar_stream_seq_steps(seq);
  const Windows win{reinterpret_cast<const uint4*>(img), g, npieces, (int)(4 * K * sizeof(T) / 16)};
  const int64_t rows_per_pass = (int64_t)rows_per_iter * R;
  const int64_t n_pass = (B + rows_per_pass - 1) / rows_per_pass;

  if ((int64_t)blockIdx.x >= n_pass) return;      // (workgroup-uniform)
  Steps steps{win, seq, bufs, nsteps, buf_bytes, wave, lane, 0};
  steps.start();
  for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
    const int64_t row0 = pass * rows_per_pass + (threadIdx.x >> lgL);
    const bool again = pass + gridDim.x < n_pass;
    bool live[R];
    const T* __restrict__ qr[R];
    T* __restrict__ gr[R];
    T gy[R][K], lse[R], dot[R], inv[R], s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + (int64_t)r * rows_per_iter;
      live[r] = row < B;
      const int64_t at = live[r] ? row : 0;
      qr[r] = q + at * ldq;
      gr[r] = grad_q + at * ldq;
#pragma unroll
      for (int i = 0; i < K; ++i) gy[r][i] = (live[r] && i < k) ? grad_y[at * k + i] : T(0);
      lse[r] = (live[r] && nv > 0) ? rowstat[at] : T(0);
      dot[r] = T(0);            // <lambda, g> and 1 / sum_j exp(q_j - lse)
      inv[r] = T(0);
      s[r] = T(0);
    }
    int step = 0;
    for (; step < seq.first_end; ++step) {      // the windows of the vertex pieces: sum and <lambda, g>
      const int w = rayen::bar_stream_seq_window(seq, step);
      const T* __restrict__ G = window_base<T>(bar_stream_smem, steps.begin(step, w, again));
      const int slot0 = 4 * w * g;
      const int w_hi = (w + 1) * g < pv ? (w + 1) * g : pv;
      for (int p = first_piece(w * g, li, L); p < w_hi; p += L) {
        T v[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (live[r]) load4(qr[r] + 4 * p, vec_in != 0, m - 4 * p, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!live[r]) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = 4 * p + c;
            if (j < nv) {
              const T* __restrict__ gen = G + (size_t)(gen_slot(j) - slot0) * K;
              T gj = T(0);
#pragma unroll
              for (int i = 0; i < K; ++i) gj = fma(gen[i], gy[r][i], gj);
              const T e = exp_(v[r][c] - lse[r]);
              s[r] += e;
              dot[r] = fma(e, gj, dot[r]);
            }
          }
        }
      }
    }
    if (nv > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!live[r]) continue;
        inv[r] = T(1) / group_sum(s[r], L);
        dot[r] = group_sum(dot[r], L) * inv[r];
      }
    }
    for (; step < nsteps; ++step) {      // every window from 0: grad_q
      const int w = rayen::bar_stream_seq_window(seq, step);
      const T* __restrict__ G = window_base<T>(bar_stream_smem, steps.begin(step, w, again));
      const int slot0 = 4 * w * g;
      const int w_hi = (w + 1) * g < npieces ? (w + 1) * g : npieces;
      for (int p = first_piece(w * g, li, L); p < w_hi; p += L) {
        T v[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (live[r]) load4(qr[r] + 4 * p, vec_in != 0, m - 4 * p, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!live[r]) continue;
          T o[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = 4 * p + c;
            T gj = T(0);
            if (j < m) {
              const T* __restrict__ gen = G + (size_t)(gen_slot(j) - slot0) * K;
#pragma unroll
              for (int i = 0; i < K; ++i) gj = fma(gen[i], gy[r][i], gj);
            }
            const T sgn = v[r][c] > T(0) ? T(1) : (v[r][c] < T(0) ? T(-1) : T(0));
            o[c] = j < nv ? exp_(v[r][c] - lse[r]) * inv[r] * (gj - dot[r]) : sgn * gj;
          }
          store4(gr[r] + 4 * p, vec_out != 0, m - 4 * p, o);
        }
      }
    }
  }
}

// R a call runs with: the layout header's table.  For measurements (scripts/bench_bar_stream.py) RAYEN_BAR_STREAM_ROWS = 1,
// 2 or 4 in the environment of the process, read once at its first streamed call, replaces the table; never more than the
// largest whose kernels keep their rows' state in registers (profiles/bench/bar_stream.txt has the resource lines; the
// instances beyond are not compiled).  Results do not depend on R.
int rows_from_environment() {
  static const int rows = [] {
    const char* e = std::getenv("RAYEN_BAR_STREAM_ROWS");
    const int r = e != nullptr ? std::atoi(e) : 0;
    return (r == 1 || r == 2 || r == 4) ? r : 0;
  }();
  return rows;
}

template <typename T, int K>
constexpr int max_rows() {
  if (sizeof(T) == 8) return K <= 8 ? 4 : K <= 32 ? 2 : 1;
  return K <= 32 ? 4 : 2;
}

template <int K>
constexpr bool table_fits() {
  return rayen::bar_stream_rows(K, 0) <= max_rows<float, K>() && rayen::bar_stream_rows(K, 1) <= max_rows<double, K>();
}
static_assert(table_fits<4>() && table_fits<8>() && table_fits<16>() && table_fits<32>() && table_fits<64>(),
              "bar_stream_rows (rayen_bar_stream_layout.h) asks for no more rows than are instantiated");

template <typename T, int K>
int rows_of_call() {
  int r = rows_from_environment();
  if (r == 0) r = rayen::bar_stream_rows(K, sizeof(T) == 8);
  const int cap = max_rows<T, K>();
  return r < cap ? r : cap;
}

struct Geometry {
  int m, lgL, g, buf_bytes;
  size_t lds;
  int64_t per_cu;
};

template <typename T>
Geometry geometry(const RayenBarPack* p, const int64_t window_bytes) {
  Geometry ge;
  ge.m = p->nv + p->nr;
  ge.lgL = group_log2(ge.m);
  ge.g = (int)rayen::bar_stream_groups(window_bytes, p->K, sizeof(T));
  ge.buf_bytes = (int)rayen::bar_stream_buffer_bytes(ge.m, ge.g, p->K, sizeof(T));
  ge.lds = (size_t)rayen::bar_stream_lds_bytes(ge.m, ge.g, p->K, sizeof(T));
  ge.per_cu = rayen::bar_stream_wg_per_cu((int64_t)ge.lds);
  return ge;
}

// workgroups: enough to cover the batch, at most as many as fit on the chip at once (LDS and waves per CU)
unsigned grid_for(const RayenBarPack* p, const Geometry& ge, const int64_t B, const int R) {
  const int64_t rows_per_pass = (int64_t)(kThreads >> ge.lgL) * R;
  const int64_t need = (B + rows_per_pass - 1) / rows_per_pass;
  const int64_t cap = (int64_t)p->cus * ge.per_cu;
  return (unsigned)(need < cap ? need : cap);
}

template <typename T, int K, int R>
int launch_forward(const RayenBarPack* p, const Geometry& ge, const T* q, int64_t B, int64_t ldq, T* y, int64_t ldy,
                   T* rowstat, int32_t* nan_flag, hipStream_t stream) {
  auto kern = bar_stream_forward_kernel<T, K, R>;
  if (!rayen::allow_lds(kern, ge.lds)) return RAYEN_E_LAUNCH;
  const int vec = rayen::rows_aligned16(q, ld_words<T>(ldq));
  const int64_t chunk = rows_per_launch(ldq > ldy ? ldq : ldy, sizeof(T));
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t b = B - r0 < chunk ? B - r0 : chunk;
    hipLaunchKernelGGL(kern, dim3(grid_for(p, ge, b, R)), dim3(kThreads), ge.lds, stream, image<T>(p), p->nv, ge.m, ge.lgL,
                       ge.g, ge.buf_bytes, q + r0 * ldq, b, ldq, vec, y + r0 * ldy, ldy, p->k,
                       rowstat ? rowstat + r0 : nullptr, nan_flag);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename T, int K, int R>
int launch_backward(const RayenBarPack* p, const Geometry& ge, const T* q, int64_t ldq, const T* rowstat, const T* grad_y,
                    int64_t B, T* grad_q, hipStream_t stream) {
  auto kern = bar_stream_backward_kernel<T, K, R>;
  if (!rayen::allow_lds(kern, ge.lds)) return RAYEN_E_LAUNCH;
  const int vec_in = rayen::rows_aligned16(q, ld_words<T>(ldq));
  const int vec_out = rayen::rows_aligned16(grad_q, ld_words<T>(ldq));
  const int64_t chunk = rows_per_launch(ldq > p->k ? ldq : p->k, sizeof(T));
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t b = B - r0 < chunk ? B - r0 : chunk;
    hipLaunchKernelGGL(kern, dim3(grid_for(p, ge, b, R)), dim3(kThreads), ge.lds, stream, image<T>(p), p->nv, ge.m, ge.lgL,
                       ge.g, ge.buf_bytes, q + r0 * ldq, b, ldq, vec_in, vec_out, rowstat ? rowstat + r0 : nullptr,
                       grad_y + r0 * p->k, p->k, grad_q + r0 * ldq);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

// f(std::integral_constant<int, R>) for the R of this call
template <typename T, int K, typename F>
int dispatch_rows(F&& f) {
  const int R = rows_of_call<T, K>();
  if constexpr (max_rows<T, K>() >= 4)
    if (R == 4) return f(std::integral_constant<int, 4>());
  if constexpr (max_rows<T, K>() >= 2)
    if (R >= 2) return f(std::integral_constant<int, 2>());
  return f(std::integral_constant<int, 1>());
}

// For measurements (scripts/bench_bar_stream.py: the default window is chosen among 20, 40 and 80 KiB) a process whose
// environment has RAYEN_BAR_STREAM_MEASURE=1, read once at its first streamed call, may pass windows up to the largest two
// buffers and yp's slot leave room for instead of up to the default.
bool measuring() {
  static const bool on = [] {
    const char* e = std::getenv("RAYEN_BAR_STREAM_MEASURE");
    return e != nullptr && e[0] == '1' && e[1] == 0;
  }();
  return on;
}

// the window of a call: RAYEN_E_BAD_ARG for a size the layout refuses or one that does not hold a group of four generators
template <typename T>
int check_window(const RayenBarPack* p, const int64_t window_bytes) {
  const bool ok = rayen::bar_stream_window_ok(window_bytes) ||
                  (measuring() && window_bytes > 0 && window_bytes % 16 == 0 && window_bytes <= rayen::kBarStreamMaxWindow);
  if (!ok || rayen::bar_stream_groups(window_bytes, p->K, sizeof(T)) < 1) return RAYEN_E_BAD_ARG;
  return RAYEN_OK;
}

template <typename T>
int bar_stream_forward(const RayenBarPack* p, const T* q, int64_t B, int64_t ldq, T* y, int64_t ldy, T* rowstat,
                       int32_t* nan_flag, int64_t window_bytes, void* stream) {
  if (p == nullptr || B < 0) return RAYEN_E_BAD_ARG;
  const int m = p->nv + p->nr;
  if (B > 0 && (q == nullptr || y == nullptr || ldq < m || ldy < p->k)) return RAYEN_E_BAD_ARG;
  if (image<T>(p) == nullptr) return RAYEN_E_UNSUPPORTED;
  int rc = check_window<T>(p, window_bytes);
  if (rc != RAYEN_OK) return rc;
  rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Geometry ge = geometry<T>(p, window_bytes);
  return rayen::dispatch_width<kMinK, kMaxK>(p->K, [&](auto K) {
    return dispatch_rows<T, K()>([&](auto R) {
      return launch_forward<T, K(), R()>(p, ge, q, B, ldq, y, ldy, rowstat, nan_flag, s);
    });
  });
}

template <typename T>
int bar_stream_backward(const RayenBarPack* p, const T* q, int64_t ldq, const T* rowstat, const T* grad_y, int64_t B,
                        T* grad_q, int64_t window_bytes, void* stream) {
  if (p == nullptr || B < 0) return RAYEN_E_BAD_ARG;
  const int m = p->nv + p->nr;
  if (B > 0 && (q == nullptr || grad_y == nullptr || grad_q == nullptr || ldq < m || (p->nv > 0 && rowstat == nullptr)))
    return RAYEN_E_BAD_ARG;
  if (image<T>(p) == nullptr) return RAYEN_E_UNSUPPORTED;
  int rc = check_window<T>(p, window_bytes);
  if (rc != RAYEN_OK) return rc;
  rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Geometry ge = geometry<T>(p, window_bytes);
  return rayen::dispatch_width<kMinK, kMaxK>(p->K, [&](auto K) {
    return dispatch_rows<T, K()>([&](auto R) {
      return launch_backward<T, K(), R()>(p, ge, q, ldq, rowstat, grad_y, B, grad_q, s);
    });
  });
}

}  // namespace

extern "C" {

int rayen_bar_resident_served(const RayenBarPack* pack, int32_t f64) {
  if (pack == nullptr) return 0;
  if (f64) return pack->img64 != nullptr && lds_bytes<double>(pack) <= rayen::kLdsBudget;
  return pack->img32 != nullptr && lds_bytes<float>(pack) <= rayen::kLdsBudget;
}

int rayen_bar_stream_forward_f32(const RayenBarPack* pack, const float* q, int64_t B, int64_t ldq, float* y, int64_t ldy,
                                 float* rowstat, int32_t* nan_flag, int64_t window_bytes, void* stream) {
  return bar_stream_forward<float>(pack, q, B, ldq, y, ldy, rowstat, nan_flag, window_bytes, stream);
}

int rayen_bar_stream_forward_f64(const RayenBarPack* pack, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                                 double* rowstat, int32_t* nan_flag, int64_t window_bytes, void* stream) {
  return bar_stream_forward<double>(pack, q, B, ldq, y, ldy, rowstat, nan_flag, window_bytes, stream);
}

int rayen_bar_stream_backward_f32(const RayenBarPack* pack, const float* q, int64_t ldq, const float* rowstat,
                                  const float* grad_y, int64_t B, float* grad_q, int64_t window_bytes, void* stream) {
  return bar_stream_backward<float>(pack, q, ldq, rowstat, grad_y, B, grad_q, window_bytes, stream);
}

int rayen_bar_stream_backward_f64(const RayenBarPack* pack, const double* q, int64_t ldq, const double* rowstat,
                                  const double* grad_y, int64_t B, double* grad_q, int64_t window_bytes, void* stream) {
  return bar_stream_backward<double>(pack, q, ldq, rowstat, grad_y, B, grad_q, window_bytes, stream);
}

}  // extern "C"
