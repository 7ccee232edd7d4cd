// Soft cost and violation of a batch for sets whose image of stacked rows does NOT fit LDS (rayen_cost.hip serves the ones
// that do): the image is cut on the host into WINDOWS, each a self-contained image in the resident layout
// (rayen_cost_stream_layout.h), and a workgroup brings the windows through LDS one after another while its waves keep
// their samples' accumulators (cost_half, cost_full, wv, wi, gacc | cs, wv, wi, gv) in registers.  Every window is walked
// by the resident kernels' own functions (rayen_cost_walk.h: walk32 on v_mfma_f32_32x32x2_f32, walk64 a lane per sample),
// so a sample sees the same operations in the same order as in the resident kernel and the two routes agree bit for bit
// wherever both serve a set.
//
// Buffers.  Two, of the largest window's size (one when the set is a single window, which then stays).  Window number q of
// a workgroup's sequence (windows 0 .. nw-1 for its first sample groups, again for its next ones, ...) lives in buffer
// q & 1.  Per window:
//     s_waitcnt vmcnt(0); barrier      -- window q has landed (every thread waited for its own part of the copy), and every
//                                         wave is done with window q - 1
//     copy of window q + 1 -> buffer (q + 1) & 1 = the buffer of window q - 1, which nobody reads any more
//     walk of window q in buffer q & 1
// The copy is LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes land at consecutive LDS addresses, nothing returns
// through the vector registers), so it runs under the walk: by scripts/ubench/mfma_coissue.hip such loads run beside the
// matrix pipe, loads through the registers do not.
//
// Uniformity.  The loops over sample groups and over windows have workgroup-uniform trip counts: all four waves take every
// barrier and issue their share of every copy.  A wave whose 32 samples are all >= B (fp32), or a lane whose sample is
// (fp64), skips the walk and the stores: it reads and writes nothing.
//
// Offsets.  Every LDS offset of a window comes from that window's entry of the table the host built with it (8 ints:
// offset and size in 16-byte pieces, tiles | items, rowc, colv, fconst, desc offsets in words).  Only the ids the descriptors
// carry (id0, which) are the set's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_cost_pack.h"
#include "rayen_cost_stream_layout.h"
#include "rayen_cost_walk.h"

namespace rayen {

// one precision's stream image on the device: table [nw][8] ints | the windows (each starts on a 16-byte boundary)
struct CostStreamSide {
  int32_t* dev = nullptr;
  int nw = 0;
  int64_t buf_bytes = 0;      // the largest window
  bool served = false;
};

struct CostStream {
  int64_t window_bytes = 0;
  CostStreamSide s32, s64;
};

void cost_stream_free(CostStream* s) {
  if (s == nullptr) return;
  if (s->s32.dev) (void)hipFree(s->s32.dev);
  if (s->s64.dev) (void)hipFree(s->s64.dev);
  delete s;
}

}  // namespace rayen

namespace {

using namespace rayen::cost;
using rayen::CostStreamItem;
using rayen::CostStreamPiece;
using rayen::CostStreamSide;
using rayen::CostStreamWindow;

static_assert(rayen::kCostStreamLds == (int64_t)rayen::kLdsBudget, "rayen_cost_stream_layout.h restates the LDS budget");
constexpr int kTableWords = 8;
enum { TW_OFF16 = 0, TW_N16 = 1, TW_COUNT = 2, TW_ROWC = 3, TW_COLV = 4, TW_FC = 5, TW_DESC = 6 };

// this wave's share of a window's copy: chunks of 1 KiB (64 lanes x 16 bytes), dealt over the four waves; the lanes past
// the window's end fetch nothing (and nothing lands at their LDS addresses)
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

__device__ __forceinline__ int table_word(const int32_t* __restrict__ table, const int w, const int which) {
  return __builtin_amdgcn_readfirstlane(table[w * kTableWords + which]);
}

template <bool GRAD>
__global__ __launch_bounds__(kThreads) void cost_stream_mfma_kernel(const int32_t* __restrict__ table, const int nw,
                                                                    const int buf_bytes, const float* __restrict__ y,
                                                                    const int64_t B, const int64_t ld, const int k,
                                                                    const int vec_in, float* __restrict__ cost,
                                                                    float* __restrict__ worst, int32_t* __restrict__ which,
                                                                    float* __restrict__ grad, const int64_t ldg,
                                                                    const int vec_out, const int eq_shift) {
  extern __shared__ __align__(16) unsigned char stream_smem[];
  const uint4* __restrict__ img = reinterpret_cast<const uint4*>(table);
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
  const int64_t n_groups = (B + 31) / 32;
  const int64_t stride = (int64_t)gridDim.x * (kThreads / 64);
  const float ninf = -INFINITY;
  const bool two = nw > 1;

  if ((int64_t)blockIdx.x * (kThreads / 64) >= n_groups) return;      // (workgroup-uniform: no barrier is left behind)
  stream_copy(img + table_word(table, 0, TW_OFF16), table_word(table, 0, TW_N16), stream_smem, wave, lane);
  unsigned q = 0;      // windows this workgroup has taken so far
  for (int64_t g0 = (int64_t)blockIdx.x * (kThreads / 64); g0 < n_groups; g0 += stride) {
    const int64_t grp = g0 + wave;
    const bool active = grp < n_groups;      // (wave-uniform)
    const int64_t s = grp * 32 + i;
    const bool live = active && s < B;
    float yr[32];
    load_y32(y, s, live, ld, k, vec_in, h, yr);
    f32x16 gacc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[0][r] = gacc[1][r] = 0.0f;
    float cost_half = 0.0f, cost_full = 0.0f, wv = ninf;
    int wi = -1;
    const bool again = g0 + stride < n_groups;
    for (int w = 0; w < nw; ++w, ++q) {
      // (the table is read in front of the wait: a load behind the copy's issue would have to wait for the copy)
      const int nx = w + 1 < nw ? w + 1 : 0;
      const int nx_off16 = table_word(table, nx, TW_OFF16), nx_n16 = table_word(table, nx, TW_N16);
      const int nt = table_word(table, w, TW_COUNT), rowc_off = table_word(table, w, TW_ROWC);
      const int colv_off = table_word(table, w, TW_COLV), desc_off = table_word(table, w, TW_DESC);
      stream_landed();
      if (two && (w + 1 < nw || again))
        stream_copy(img + nx_off16, nx_n16, stream_smem + (size_t)((q + 1) & 1) * buf_bytes, wave, lane);
      if (active) {
        const float* __restrict__ W = reinterpret_cast<const float*>(stream_smem + (size_t)(two ? (q & 1) : 0) * buf_bytes);
        walk32<GRAD>(W, W + rowc_off, W + colv_off, reinterpret_cast<const int*>(W) + desc_off, nt, yr, i, h, eq_shift, gacc,
                     cost_half, cost_full, wv, wi);
      }
    }
    if (active) store32<GRAD>(cost_half, cost_full, wv, wi, gacc, s, live, h, k, cost, worst, which, grad, ldg, vec_out);
  }
}

template <int K, bool GRAD>
__global__ __launch_bounds__(kThreads) void cost_stream_lane64_kernel(const int32_t* __restrict__ table, const int nw,
                                                                      const int buf_bytes, const double* __restrict__ y,
                                                                      const int64_t B, const int64_t ld, const int k,
                                                                      double* __restrict__ cost, double* __restrict__ worst,
                                                                      int32_t* __restrict__ which, double* __restrict__ grad,
                                                                      const int64_t ldg, const int eq_shift) {
  extern __shared__ __align__(16) unsigned char stream_smem[];
  const uint4* __restrict__ img = reinterpret_cast<const uint4*>(table);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const bool two = nw > 1;

  if ((int64_t)blockIdx.x * kThreads >= B) return;      // (workgroup-uniform)
  stream_copy(img + table_word(table, 0, TW_OFF16), table_word(table, 0, TW_N16), stream_smem, wave, lane);
  unsigned q = 0;
  for (int64_t s0 = (int64_t)blockIdx.x * kThreads; s0 < B; s0 += stride) {
    const int64_t s = s0 + threadIdx.x;
    const bool live = s < B;
    const double* __restrict__ ys = y + (live ? s : 0) * ld;
    double yv[K], gv[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      yv[c] = (live && c < k) ? ys[c] : 0.0;
      gv[c] = 0.0;
    }
    double cs = 0.0, wv = -INFINITY;
    int wi = -1;
    const bool again = s0 + stride < B;
    for (int w = 0; w < nw; ++w, ++q) {
      const int nx = w + 1 < nw ? w + 1 : 0;
      const int nx_off16 = table_word(table, nx, TW_OFF16), nx_n16 = table_word(table, nx, TW_N16);
      const int ni = table_word(table, w, TW_COUNT), rowc_off = table_word(table, w, TW_ROWC);
      const int colv_off = table_word(table, w, TW_COLV), fc_off = table_word(table, w, TW_FC);
      const int desc_off = table_word(table, w, TW_DESC);
      stream_landed();
      if (two && (w + 1 < nw || again))
        stream_copy(img + nx_off16, nx_n16, stream_smem + (size_t)((q + 1) & 1) * buf_bytes, wave, lane);
      if (live) {      // (a quadratic reads its sample's y from memory: that load returns behind the copy)
        const double* __restrict__ W = reinterpret_cast<const double*>(stream_smem + (size_t)(two ? (q & 1) : 0) * buf_bytes);
        walk64<K, GRAD>(W, W + rowc_off, W + colv_off, W + fc_off, reinterpret_cast<const int*>(W + desc_off), ni, ys, k, yv,
                        eq_shift, gv, cs, wv, wi);
      }
    }
    if (live) {
      if (cs != cs) { wv = cs; wi = -1; }
      if (cost != nullptr) cost[s] = cs;
      if (worst != nullptr) worst[s] = wv;
      if (which != nullptr) which[s] = wi;
      if (GRAD) {
        double* __restrict__ gs = grad + s * ldg;
#pragma unroll
        for (int c = 0; c < K; ++c)
          if (c < k) gs[c] = gv[c];
      }
    }
  }
}

// ---- host: the windows

rayen::CostSetView stream_view(const RayenCostPack* p) {      // (the order rayen_cost_pack_create stored the arrays in)
  const size_t k = (size_t)p->k;
  size_t msoc = 0;
  for (int j = 0; j < p->nsoc; ++j) msoc += (size_t)p->host_soc_rows[j];
  const size_t len[11] = {p->m1 * k, (size_t)p->m1, p->nq * k * k, p->nq * k, (size_t)p->nq, msoc * k, msoc, p->nsoc * k,
                          (size_t)p->nsoc, p->m2 * k, (size_t)p->m2};
  const double* at[11];
  size_t off = 0;
  for (int a = 0; a < 11; ++a) {
    at[a] = p->host.data() + off;
    off += len[a];
  }
  return rayen::CostSetView{at[0], at[1], at[2], at[3], at[4], at[5], at[6], at[7], at[8], at[9], at[10],
                            p->host_soc_rows.data(), p->m1, p->nq, p->nsoc, p->m2, p->k};
}

struct Cut {
  std::vector<CostStreamWindow> windows;
  std::vector<CostStreamPiece> pieces;
  int64_t total = 0;
};

bool cut(const std::vector<CostStreamItem>& items, const int f64, const int K, const int64_t window_bytes, Cut* c) {
  int64_t np = 0;
  const int64_t nw = rayen::cost_stream_partition(items.data(), (int64_t)items.size(), f64, K, window_bytes, nullptr, 0,
                                                  nullptr, 0, &np, &c->total);
  if (nw <= 0) return false;
  c->windows.resize((size_t)nw);
  c->pieces.resize((size_t)np);
  return rayen::cost_stream_partition(items.data(), (int64_t)items.size(), f64, K, window_bytes, c->windows.data(), nw,
                                      c->pieces.data(), np, nullptr, nullptr) == nw;
}

// stream image: table [nw][8] | windows; false when the set is not served at this window size (an item larger than the
// window, a cone of more than 64 rows, an image beyond kCostStreamMaxImage)
bool build_stream32(const rayen::CostSetView& v, const int64_t window_bytes, std::vector<int32_t>* out, CostStreamSide* side) {
  RayenCostPack g;
  std::vector<int32_t> full;
  if (!rayen::cost_build32(v, &g, &full, (size_t)rayen::kCostStreamMaxImage)) return false;
  const int32_t* fdesc = full.data() + g.desc_off;
  // items: a run of linear (or equality) tiles is one splittable item; a quadratic / a cone its one or two tiles
  std::vector<CostStreamItem> items;
  std::vector<int> tile0;
  for (int t = 0; t < g.nt;) {
    const int type = fdesc[t * kDescWords];
    if (type == CT_LIN || type == CT_EQ) {
      int n = 1;
      while (t + n < g.nt && fdesc[(t + n) * kDescWords] == type) ++n;
      items.push_back({n, 0, 1});
      tile0.push_back(t);
      t += n;
    } else {
      const int n = fdesc[t * kDescWords + 5];
      items.push_back({n, 1, 0});
      tile0.push_back(t);
      t += n;
    }
  }
  Cut c;
  if (!cut(items, 0, 0, window_bytes, &c)) return false;
  const size_t nw = c.windows.size(), table_words = nw * kTableWords;
  if ((int64_t)(table_words * 4) + c.total > rayen::kCostStreamMaxImage) return false;
  out->assign(table_words + (size_t)(c.total / 4), 0);
  size_t at = table_words;      // words
  int64_t largest = 0;
  for (size_t w = 0; w < nw; ++w) {
    const CostStreamWindow& win = c.windows[w];
    const int nt = win.units, nf = win.forms;
    const int rowc_off = nt * 2048, colv_off = rowc_off + nt * 32, desc_off = colv_off + nf * 64;
    int32_t* tw = out->data() + w * kTableWords;
    tw[TW_OFF16] = (int32_t)(at / 4);
    tw[TW_N16] = (int32_t)(win.bytes / 16);
    tw[TW_COUNT] = nt;
    tw[TW_ROWC] = rowc_off;
    tw[TW_COLV] = colv_off;
    tw[TW_DESC] = desc_off;
    int32_t* dst = out->data() + at;
    int lt = 0, lf = 0;
    for (int pc = 0; pc < win.pieces; ++pc) {
      const CostStreamPiece& piece = c.pieces[(size_t)win.piece0 + pc];
      const bool formed = items[piece.item].forms != 0;
      for (int u = 0; u < piece.units; ++u, ++lt) {
        const int T = tile0[piece.item] + piece.unit0 + u;
        std::memcpy(dst + (size_t)lt * 2048, full.data() + (size_t)T * 2048, 2048 * 4);
        std::memcpy(dst + rowc_off + lt * 32, full.data() + g.rowc_off + (size_t)T * 32, 32 * 4);
        int32_t* d = dst + desc_off + lt * kDescWords;
        std::memcpy(d, fdesc + (size_t)T * kDescWords, kDescWords * 4);
        if (formed) {
          if (u == 0) std::memcpy(dst + colv_off + lf * 64, full.data() + g.colv_off + (size_t)d[3] * 64, 64 * 4);
          d[3] = lf;
        }
      }
      if (formed) ++lf;
    }
    if (lt != nt || lf != nf) return false;
    at += (size_t)(win.bytes / 4);
    if (win.bytes > largest) largest = win.bytes;
  }
  side->nw = (int)nw;
  side->buf_bytes = largest;
  return true;
}

bool build_stream64(const rayen::CostSetView& v, const int64_t window_bytes, std::vector<int32_t>* out, CostStreamSide* side) {
  RayenCostPack g;
  std::vector<double> full;
  if (!rayen::cost_build64(v, &g, &full, (size_t)rayen::kCostStreamMaxImage)) return false;
  const int K = g.K64;
  const int32_t* fdesc = reinterpret_cast<const int32_t*>(full.data() + g.desc64_off);
  std::vector<CostStreamItem> items;
  for (int it = 0; it < g.ni; ++it) {
    const int type = fdesc[it * kDescWords];
    const bool run = type == CT_LIN || type == CT_EQ;
    items.push_back({fdesc[it * kDescWords + 5], run ? 0 : 1, run ? 1 : 0});
  }
  Cut c;
  if (!cut(items, 1, K, window_bytes, &c)) return false;
  const size_t nw = c.windows.size(), table_words = nw * kTableWords;
  if ((int64_t)(table_words * 4) + c.total > rayen::kCostStreamMaxImage) return false;
  out->assign(table_words + (size_t)(c.total / 4), 0);
  size_t at = table_words;      // 4-byte words (windows start on 16-byte boundaries: the table is 32 bytes a window)
  int64_t largest = 0;
  for (size_t w = 0; w < nw; ++w) {
    const CostStreamWindow& win = c.windows[w];
    const int R = win.units, nf = win.forms, ni = win.pieces;
    const int rowc_off = R * K, colv_off = rowc_off + R, fc_off = colv_off + nf * K, desc_off = fc_off + ni;
    int32_t* tw = out->data() + w * kTableWords;
    tw[TW_OFF16] = (int32_t)(at / 4);
    tw[TW_N16] = (int32_t)(win.bytes / 16);
    tw[TW_COUNT] = ni;
    tw[TW_ROWC] = rowc_off;
    tw[TW_COLV] = colv_off;
    tw[TW_FC] = fc_off;
    tw[TW_DESC] = desc_off;
    unsigned char* dst = reinterpret_cast<unsigned char*>(out->data() + at);
    auto put = [&](const size_t word, const double* src, const size_t n) { std::memcpy(dst + word * 8, src, n * 8); };
    int lr = 0, lf = 0;
    for (int pc = 0; pc < ni; ++pc) {
      const CostStreamPiece& piece = c.pieces[(size_t)win.piece0 + pc];
      const int32_t* fd = fdesc + (size_t)piece.item * kDescWords;
      const bool formed = items[piece.item].forms != 0;
      const int row0 = fd[1] + piece.unit0;
      put((size_t)lr * K, full.data() + (size_t)row0 * K, (size_t)piece.units * K);
      put((size_t)rowc_off + lr, full.data() + g.rowc64_off + row0, (size_t)piece.units);
      put((size_t)fc_off + pc, full.data() + g.fc64_off + piece.item, 1);
      if (formed) put((size_t)colv_off + (size_t)lf * K, full.data() + g.colv64_off + (size_t)fd[3] * K, (size_t)K);
      int32_t d[kDescWords] = {fd[0], lr, fd[2] + (formed ? 0 : piece.unit0), formed ? lf : 0, 0, piece.units, 0, 0};
      std::memcpy(dst + (size_t)desc_off * 8 + (size_t)pc * kDescWords * 4, d, sizeof(d));
      lr += piece.units;
      if (formed) ++lf;
    }
    if (lr != R || lf != nf) return false;
    at += (size_t)(win.bytes / 4);
    if (win.bytes > largest) largest = win.bytes;
  }
  side->nw = (int)nw;
  side->buf_bytes = largest;
  return true;
}

size_t stream_lds(const CostStreamSide& s) { return (size_t)(s.nw > 1 ? 2 * s.buf_bytes : s.buf_bytes); }

template <bool GRAD>
int launch32(const RayenCostPack* p, const float* y, int64_t B, int64_t ld, float* cost, float* worst, int32_t* which,
             float* grad, int64_t ldg, hipStream_t stream) {
  const CostStreamSide& s = p->stream->s32;
  auto kern = cost_stream_mfma_kernel<GRAD>;
  if (!rayen::allow_lds(kern, stream_lds(s))) return RAYEN_E_LAUNCH;
  const int64_t grid = rayen::persistent_grid(B, 32, rayen::launch_simds(p->n_simd), kThreads / 64);
  const int vec_in = (p->k % 4 == 0) && rayen::rows_aligned16(y, ld);
  const int vec_out = GRAD && (p->k % 4 == 0) && rayen::rows_aligned16(grad, ldg);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), stream_lds(s), stream, s.dev, s.nw, (int)s.buf_bytes, y, B, ld,
                     p->k, vec_in, cost, worst, which, grad, ldg, vec_out, p->eq_shift);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

template <int K, bool GRAD>
int launch64(const RayenCostPack* p, const double* y, int64_t B, int64_t ld, double* cost, double* worst, int32_t* which,
             double* grad, int64_t ldg, hipStream_t stream) {
  const CostStreamSide& s = p->stream->s64;
  auto kern = cost_stream_lane64_kernel<K, GRAD>;
  if (!rayen::allow_lds(kern, stream_lds(s))) return RAYEN_E_LAUNCH;
  const int64_t grid = rayen::persistent_grid(B, kThreads, rayen::launch_simds(p->n_simd) / 4, 1);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), stream_lds(s), stream, s.dev, s.nw, (int)s.buf_bytes, y, B, ld,
                     p->k, cost, worst, which, grad, ldg, p->eq_shift);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

bool rows_streamed(const RayenCostPack* p, const bool f64) {
  return p != nullptr && p->stream != nullptr && (f64 ? p->stream->s64.served : p->stream->s32.served);
}

}  // namespace

extern "C" {

int rayen_cost_stream_set(RayenCostPack* pack, int64_t window_bytes) {
  if (pack == nullptr || !rayen::cost_stream_window_ok(window_bytes)) return RAYEN_E_BAD_ARG;
  const int64_t window = window_bytes == 0 ? rayen::kCostStreamWindow : window_bytes;
  if (pack->stream != nullptr && pack->stream->window_bytes == window) return RAYEN_OK;
  int rc = rayen::check_device(pack->device);
  if (rc != RAYEN_OK) return rc;
  rayen::CostStream* st = new (std::nothrow) rayen::CostStream();
  if (st == nullptr) return RAYEN_E_ALLOC;
  st->window_bytes = window;
  if (pack->k <= 64 && pack->n_rows > 0) {
    try {
      const rayen::CostSetView v = stream_view(pack);
      std::vector<int32_t> w32, w64;
      st->s32.served = build_stream32(v, window, &w32, &st->s32);
      st->s64.served = build_stream64(v, window, &w64, &st->s64);
      if ((st->s32.served && !rayen::upload_image(w32, &st->s32.dev)) ||
          (st->s64.served && !rayen::upload_image(w64, &st->s64.dev))) {
        rayen::cost_stream_free(st);
        return RAYEN_E_ALLOC;
      }
    } catch (const std::bad_alloc&) {
      rayen::cost_stream_free(st);
      return RAYEN_E_ALLOC;
    }
  }
  rayen::cost_stream_free(pack->stream);      // (another window size: hipFree waits for the launches that read the old images)
  pack->stream = st;
  return RAYEN_OK;
}

int rayen_cost_stream_served(const RayenCostPack* pack, int32_t f64) {
  if (pack == nullptr || pack->stream == nullptr) return 0;
  const bool rows = rows_streamed(pack, f64 != 0);
  return (f64 ? rayen::cost_serves_set<double>(pack, rows) : rayen::cost_serves_set<float>(pack, rows)) ? 1 : 0;
}

int rayen_soft_cost_stream_f32(const RayenCostPack* pack, const float* y, int64_t B, int64_t ld, float* cost, float* worst,
                               int32_t* which, float* grad, int64_t ld_grad, void* stream) {
  return rayen::cost_call<float>(pack, rows_streamed(pack, false), y, B, ld, cost, worst, which, grad, ld_grad, stream,
                                 [&](hipStream_t st) {
                                   return grad != nullptr ? launch32<true>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st)
                                                          : launch32<false>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st);
                                 });
}

int rayen_soft_cost_stream_f64(const RayenCostPack* pack, const double* y, int64_t B, int64_t ld, double* cost, double* worst,
                               int32_t* which, double* grad, int64_t ld_grad, void* stream) {
  return rayen::cost_call<double>(pack, rows_streamed(pack, true), y, B, ld, cost, worst, which, grad, ld_grad, stream,
                                  [&](hipStream_t st) {
                                    const int K = rayen::padded_width<kMinK64, kMaxK64>(pack->k);
                                    return rayen::dispatch_width<kMinK64, kMaxK64>(K, [&](auto Kc) {
                                      return grad != nullptr
                                                 ? launch64<Kc(), true>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st)
                                                 : launch64<Kc(), false>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st);
                                    });
                                  });
}

}  // extern "C"
