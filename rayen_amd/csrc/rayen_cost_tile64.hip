// Soft cost and violation of a batch in fp64 on v_mfma_f64_16x16x4_f64 (kernel='tile64'): the outputs and the contract of
// rayen_soft_cost_f64, by a third route next to the resident lane kernel (rayen_cost.hip) and the streamed one
// (rayen_cost_stream.hip).  Layout, slot function, windows and envelope: rayen_cost_tile64_layout.h.
//
// Sample on the matrix column.  A wave holds NS column blocks of 16 samples.  Lane (n = lane & 15, g = lane >> 4) holds, of
// sample n of every column block,
//     yv[j]       = y[4 j + g]                       j < K / 4      (the B operand of step j of the first product)
//     gacc[cb][i] = grad[16 cb + 4 i + g]            = grad[4 (4 cb + i) + g]: the same columns as yv[4 cb + i]
// First product, per block of 16 stacked rows: T = W_block Y', K / 4 MFMAs per column block; step j takes W[m][4 j + g] from
// lane (m, g).  The C/D map of the instruction (row = 4 i + g in register i of lane group g) puts rows
// rho(i, g) = 4 i + g of the block in the four registers of a lane.  Second product, grad' += W_block' C': step i sums over
// the rows 4 i + 0 .. 3 and takes row 4 i + g from lane group g -- the row register i of that lane holds.  So the
// coefficients (2 relu(g), 2 relu(g) u / ||u||, 2 e) are written over T in place and feed the second product as they lie; and
// a quadratic's P y (block b, register i: row 16 b + 4 i + g) lines up with yv[4 b + i] and with gacc[b][i]: plain FMAs.
// Every per-sample reduction is a sum over a lane's registers and two exchanges between the four lane groups.
//
// Arithmetic.  Exact fp64, every term by an explicit fma; the order in which a sample's terms are added depends on the set
// alone (blocks are cut from the start of a run or an item, windows are cut between blocks), never on B, on the other
// samples of the wave, on the window size or on whether grad was asked for.  The second product of a block is skipped when
// no sample of the wave has a coefficient other than 0 (one ballot): the skipped terms are +-0 added to accumulators that
// are never -0.  A cone of one block keeps its products in registers; a larger one computes them again, block by block,
// for the gradient (the same operations: the same bits).
//
// Windows.  The protocol of rayen_cost_stream.hip: two LDS buffers of the largest window's size (one when the set is a single
// window, which is copied once and stays), LDS-DMA copies (global_load_lds_dwordx4) of window q + 1 under the walk of window
// q, the table words read in front of the wait, workgroup-uniform trip counts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_cost_pack.h"
#include "rayen_cost_tile64_layout.h"

namespace rayen {

struct CostTile64 {
  int64_t window_bytes = 0;
  int32_t* dev = nullptr;      // table [nw][8] ints | the windows (each starts on a 16-byte boundary)
  int nw = 0, K = 0;
  int64_t buf_bytes = 0;       // the largest window
  bool served = false;
};

void cost_tile64_free(CostTile64* t) {
  if (t == nullptr) return;
  if (t->dev) (void)hipFree(t->dev);
  delete t;
}

}  // namespace rayen

namespace {

using rayen::cost_tile64_slot;
using rayen::CostTile64;
using rayen::CostTile64Item;
using rayen::CostTile64Piece;
using rayen::CostTile64Window;

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { CT_LIN = 0, CT_EQ = 1, CT_QUAD = 2, CT_SOC = 3 };      // (the types of rayen_cost_walk.h)
constexpr int kThreads = 256;                                 // four waves: one per SIMD
constexpr int kWaves = kThreads / 64;
constexpr int kDescWords = 8;      // per block: type, nvalid (rows of the block | of the whole cone), id0, form, blocks of the item
constexpr int kTableWords = rayen::kCostTile64TableWords;
enum { TW_OFF16 = 0, TW_N16 = 1, TW_COUNT = 2, TW_ROWC = 3, TW_COLV = 4, TW_FC = 5, TW_DESC = 6 };

static_assert(rayen::kCostTile64Lds == (int64_t)rayen::kLdsBudget, "rayen_cost_tile64_layout.h restates the LDS budget");

template <typename T>
__device__ __forceinline__ T relu_(const T g) { return g < T(0) ? T(0) : g; }      // (keeps a NaN)

// the sum over the four lane groups, the same bits in all four
__device__ __forceinline__ double groups_sum(const double v) {
  const double a = v + __shfl_xor(v, 16, 64);
  return a + __shfl_xor(a, 32, 64);
}

__device__ __forceinline__ void tile_copy(const uint4* __restrict__ src, const int n16, unsigned char* dst, const int wave,
                                          const int lane) {
  const int n_chunks = (n16 + 63) >> 6;
  for (int c = wave; c < n_chunks; c += kWaves) {
    const int p = c * 64 + lane;
    if (p < n16)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + p),
                                       (__attribute__((address_space(3))) void*)(dst + (size_t)c * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ void tile_landed() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__device__ __forceinline__ int table_word(const int32_t* __restrict__ table, const int w, const int which) {
  return __builtin_amdgcn_readfirstlane(table[w * kTableWords + which]);
}

// T[cb] register i = row 4 i + g of the block, for this lane's sample of column block cb
template <int K, int NS, int NY>
__device__ __forceinline__ void first_product(const double* __restrict__ Wb, const double (&yv)[NS][NY], const int n, const int g,
                                              f64x4 (&T)[NS]) {
#pragma unroll
  for (int cb = 0; cb < NS; ++cb) T[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < K / 4; ++j) {
    const double a = Wb[cost_tile64_slot(n, 4 * j + g)];
#pragma unroll
    for (int cb = 0; cb < NS; ++cb) T[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yv[cb][j], T[cb], 0, 0, 0);
  }
}

// gacc[cb][kb] register i' (column 16 kb + 4 i' + g of grad) += sum over the block's rows of C[sample][row] W[row][column]
template <int K, int NS, int NCB>
__device__ __forceinline__ void second_product(const double* __restrict__ Wb, const f64x4 (&C)[NS], f64x4 (&gacc)[NS][NCB],
                                               const int n, const int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int kb = 0; kb < NCB; ++kb) {
      double a = 0.0;
      if (K >= 16 || n < K) a = Wb[cost_tile64_slot(4 * i + g, 16 * kb + n)];      // (K = 8: columns 8 .. 15 do not exist)
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) gacc[cb][kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, C[cb][i], gacc[cb][kb], 0, 0, 0);
    }
  }
}

template <int NS>
struct Sums {
  double part[NS], full[NS], wv[NS];      // cost of this lane's rows | of whole-sample terms (the same in all four groups)
  int wi[NS];
};

// the `nb` blocks of a window (W | rowc | colv | fc | desc, all in LDS) against the wave's NS x 16 samples
template <int K, int NS, bool GRAD>
__device__ __forceinline__ void walk(const double* __restrict__ W, const double* __restrict__ rowc,
                                     const double* __restrict__ colv, const double* __restrict__ fc, const int* __restrict__ desc,
                                     const int nb, const double (&yv)[NS][(K < 16 ? 16 : K) / 4], const int n, const int g,
                                     const int eq_shift, f64x4 (&gacc)[NS][(K < 16 ? 16 : K) / 16], Sums<NS>& s) {
  constexpr int KF = K < 16 ? 16 : K, NY = KF / 4, NCB = KF / 16, BLK = 16 * K;
  int t = 0;
  while (t < nb) {
    const int* d = desc + t * kDescWords;
    const int type = __builtin_amdgcn_readfirstlane(d[0]);
    const int nvalid = __builtin_amdgcn_readfirstlane(d[1]);
    const int id0 = __builtin_amdgcn_readfirstlane(d[2]);
    const int form = __builtin_amdgcn_readfirstlane(d[3]);
    const int nblk = __builtin_amdgcn_readfirstlane(d[4]);
    const double* __restrict__ Wb = W + (size_t)t * BLK;
    if (type == CT_LIN || type == CT_EQ) {
      f64x4 T[NS];
      first_product<K, NS, NY>(Wb, yv, n, g, T);
      const int idr = type == CT_EQ ? id0 + eq_shift : id0;      // (an LMI sits between the inequalities and these)
      bool any = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int R = 4 * i + g;
        const bool valid = R < nvalid;
        const double rc = rowc[t * 16 + R];
#pragma unroll
        for (int cb = 0; cb < NS; ++cb) {
          const double gv = T[cb][i] - rc;
          const double p = type == CT_EQ ? gv : relu_(gv);
          const double val = type == CT_EQ ? fabs(gv) : gv;
          if (valid) {
            s.part[cb] = fma(p, p, s.part[cb]);
            if (val > s.wv[cb]) { s.wv[cb] = val; s.wi[cb] = idr + R; }
          }
          const double cf = valid ? 2.0 * p : 0.0;
          T[cb][i] = cf;
          any |= !(cf == 0.0);
        }
      }
      if (GRAD && __builtin_amdgcn_ballot_w64(any) != 0) second_product<K, NS, NCB>(Wb, T, gacc, n, g);
      t += 1;
    } else if (type == CT_QUAD) {      // blocks of the symmetrised P: T = P y, row 16 b + 4 i + g beside yv[4 b + i]
      const double* __restrict__ q = colv + (size_t)form * KF;
      const double fconst = fc[t];
      f64x4 Tq[NCB][NS];
      double part[NS];
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) part[cb] = 0.0;
#pragma unroll
      for (int b = 0; b < NCB; ++b) {
        if (b < nblk) {
          first_product<K, NS, NY>(Wb + (size_t)b * BLK, yv, n, g, Tq[b]);
        } else {
#pragma unroll
          for (int cb = 0; cb < NS; ++cb) Tq[b][cb] = f64x4{0.0, 0.0, 0.0, 0.0};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double qv = q[16 * b + 4 * i + g];
#pragma unroll
          for (int cb = 0; cb < NS; ++cb) part[cb] = fma(yv[cb][4 * b + i], fma(0.5, Tq[b][cb][i], qv), part[cb]);
        }
      }
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        const double gv = groups_sum(part[cb]) + fconst;
        const double p = relu_(gv);
        s.full[cb] = fma(p, p, s.full[cb]);
        if (gv > s.wv[cb]) { s.wv[cb] = gv; s.wi[cb] = id0; }
        if (GRAD && !(p == 0.0)) {
          const double c2 = 2.0 * p;
#pragma unroll
          for (int b = 0; b < NCB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) gacc[cb][b][i] = fma(c2, Tq[b][cb][i] + q[16 * b + 4 * i + g], gacc[cb][b][i]);
        }
      }
      t += nblk;
    } else {      // CT_SOC: nblk blocks of M rows, nvalid rows in all
      const double* __restrict__ cv = colv + (size_t)form * KF;
      const double fconst = fc[t];
      double n2[NS], cy[NS];
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        n2[cb] = 0.0;
        cy[cb] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < NY; ++j) {
        const double c = cv[4 * j + g];
#pragma unroll
        for (int cb = 0; cb < NS; ++cb) cy[cb] = fma(yv[cb][j], c, cy[cb]);
      }
      f64x4 U[NS];
      // u = M y + s of block b, 0 in the rows past the cone's end
      auto cone_block = [&](const int b) {
        first_product<K, NS, NY>(Wb + (size_t)b * BLK, yv, n, g, U);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int R = 4 * i + g;
          const bool valid = 16 * b + R < nvalid;
          const double rc = rowc[(t + b) * 16 + R];
#pragma unroll
          for (int cb = 0; cb < NS; ++cb) U[cb][i] = valid ? U[cb][i] + rc : 0.0;
        }
      };
      for (int b = 0; b < nblk; ++b) {
        cone_block(b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int cb = 0; cb < NS; ++cb) n2[cb] = fma(U[cb][i], U[cb][i], n2[cb]);
      }
      double c2[NS], sc[NS];
      bool any = false;
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        const double nrm = sqrt(groups_sum(n2[cb]));
        const double gv = nrm - groups_sum(cy[cb]) - fconst;
        const double p = relu_(gv);
        s.full[cb] = fma(p, p, s.full[cb]);
        if (gv > s.wv[cb]) { s.wv[cb] = gv; s.wi[cb] = id0; }
        c2[cb] = 2.0 * p;
        sc[cb] = nrm > 0.0 ? c2[cb] / nrm : (nrm == 0.0 ? 0.0 : nrm);      // (a NaN norm stays a NaN)
        any |= !(p == 0.0);
      }
      if (GRAD && __builtin_amdgcn_ballot_w64(any) != 0) {
#pragma unroll
        for (int cb = 0; cb < NS; ++cb) {
          if (!(c2[cb] == 0.0)) {
#pragma unroll
            for (int j = 0; j < NY; ++j) gacc[cb][j >> 2][j & 3] = fma(-c2[cb], cv[4 * j + g], gacc[cb][j >> 2][j & 3]);
          }
        }
        for (int b = 0; b < nblk; ++b) {
          if (nblk > 1) cone_block(b);      // (one block: U is still that block's)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cb = 0; cb < NS; ++cb) U[cb][i] = !(c2[cb] == 0.0) ? sc[cb] * U[cb][i] : 0.0;
          second_product<K, NS, NCB>(Wb + (size_t)b * BLK, U, gacc, n, g);
        }
      }
      t += nblk;
    }
  }
}

template <int K, int NS, bool GRAD>
__global__ __launch_bounds__(kThreads) void cost_tile64_kernel(const int32_t* __restrict__ table, const int nw,
                                                               const int buf_bytes, const double* __restrict__ y,
                                                               const int64_t B, const int64_t ld, const int k,
                                                               double* __restrict__ cost, double* __restrict__ worst,
                                                               int32_t* __restrict__ which, double* __restrict__ grad,
                                                               const int64_t ldg, const int eq_shift) {
  constexpr int KF = K < 16 ? 16 : K, NY = KF / 4, NCB = KF / 16, PER_WAVE = 16 * NS;
  extern __shared__ __align__(16) unsigned char tile_smem[];
  const uint4* __restrict__ img = reinterpret_cast<const uint4*>(table);
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
  const int64_t n_groups = (B + PER_WAVE - 1) / PER_WAVE;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  const bool two = nw > 1;

  if ((int64_t)blockIdx.x * kWaves >= n_groups) return;      // (workgroup-uniform: no barrier is left behind)
  tile_copy(img + table_word(table, 0, TW_OFF16), table_word(table, 0, TW_N16), tile_smem, wave, lane);
  unsigned q = 0;      // windows this workgroup has taken so far
  for (int64_t g0 = (int64_t)blockIdx.x * kWaves; g0 < n_groups; g0 += stride) {
    const int64_t grp = g0 + wave;
    const bool active = grp < n_groups;      // (wave-uniform)
    int64_t smp[NS];
    bool live[NS];
    double yv[NS][NY];
    f64x4 gacc[NS][NCB];
    Sums<NS> s;
#pragma unroll
    for (int cb = 0; cb < NS; ++cb) {
      smp[cb] = grp * PER_WAVE + 16 * cb + n;
      live[cb] = active && smp[cb] < B;
      const double* __restrict__ ys = y + (live[cb] ? smp[cb] : 0) * ld;
#pragma unroll
      for (int j = 0; j < NY; ++j) yv[cb][j] = (live[cb] && 4 * j + g < k) ? ys[4 * j + g] : 0.0;
#pragma unroll
      for (int kb = 0; kb < NCB; ++kb) gacc[cb][kb] = f64x4{0.0, 0.0, 0.0, 0.0};
      s.part[cb] = 0.0;
      s.full[cb] = 0.0;
      s.wv[cb] = -INFINITY;
      s.wi[cb] = -1;
    }
    const bool again = g0 + stride < n_groups;
    for (int w = 0; w < nw; ++w, ++q) {
      // (the table is read in front of the wait: a load behind the copy's issue would have to wait for the copy)
      const int nx = w + 1 < nw ? w + 1 : 0;
      const int nx_off16 = table_word(table, nx, TW_OFF16), nx_n16 = table_word(table, nx, TW_N16);
      const int nb = table_word(table, w, TW_COUNT), rowc_off = table_word(table, w, TW_ROWC);
      const int colv_off = table_word(table, w, TW_COLV), fc_off = table_word(table, w, TW_FC);
      const int desc_off = table_word(table, w, TW_DESC);
      tile_landed();
      if (two && (w + 1 < nw || again))
        tile_copy(img + nx_off16, nx_n16, tile_smem + (size_t)((q + 1) & 1) * buf_bytes, wave, lane);
      if (active) {
        const double* __restrict__ W = reinterpret_cast<const double*>(tile_smem + (size_t)(two ? (q & 1) : 0) * buf_bytes);
        walk<K, NS, GRAD>(W, W + rowc_off, W + colv_off, W + fc_off, reinterpret_cast<const int*>(W + desc_off), nb, yv, n, g,
                          eq_shift, gacc, s);
      }
    }
    if (active) {
#pragma unroll
      for (int cb = 0; cb < NS; ++cb) {
        double c = groups_sum(s.part[cb]) + s.full[cb];
        double wv = s.wv[cb];
        int wi = s.wi[cb];
#pragma unroll
        for (int m = 16; m <= 32; m *= 2) {      // the four groups' largest values meet: ties go to the lowest index
          const double ov = __shfl_xor(wv, m, 64);
          const int oi = __shfl_xor(wi, m, 64);
          if (ov > wv || (ov == wv && oi >= 0 && (wi < 0 || oi < wi))) { wv = ov; wi = oi; }
        }
        if (c != c) { wv = c; wi = -1; }
        if (live[cb] && g == 0) {
          if (cost != nullptr) cost[smp[cb]] = c;
          if (worst != nullptr) worst[smp[cb]] = wv;
          if (which != nullptr) which[smp[cb]] = wi;
        }
        if (GRAD && live[cb]) {
          double* __restrict__ gs = grad + smp[cb] * ldg;
#pragma unroll
          for (int j = 0; j < NY; ++j)
            if (4 * j + g < k) gs[4 * j + g] = gacc[cb][j >> 2][j & 3];
        }
      }
    }
  }
}

// ---- host: blocks, windows, image

struct ItemSource {      // an item of the set: `rows` rows of `k` columns at A (quadratic: P, symmetrised on the way)
  int type, rows, id0;
  const double *A, *rowc, *form;
  double fconst;
};

rayen::CostSetView tile_view(const RayenCostPack* p) {      // (the order rayen_cost_pack_create stored the arrays in)
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

bool build_tile64(const rayen::CostSetView& v, const int64_t window_bytes, std::vector<int32_t>* out, CostTile64* side) {
  const int k = v.k, K = rayen::cost_tile64_width(k);
  if (K == 0) return false;
  const int KF = rayen::cost_tile64_form_width(K), BLK = 16 * K;
  std::vector<ItemSource> src;
  if (v.m1 > 0) src.push_back({CT_LIN, v.m1, 0, v.A1, v.b1, nullptr, 0.0});
  for (int iq = 0; iq < v.nq; ++iq)
    src.push_back({CT_QUAD, k, v.m1 + iq, v.P + (size_t)iq * k * k, nullptr, v.q + (size_t)iq * k, v.r[iq]});
  size_t mrow = 0;
  for (int j = 0; j < v.nsoc; ++j) {
    src.push_back({CT_SOC, v.soc_rows[j], v.m1 + v.nq + j, v.M + mrow * k, v.s + mrow, v.c + (size_t)j * k, v.d[j]});
    mrow += (size_t)v.soc_rows[j];
  }
  if (v.m2 > 0) src.push_back({CT_EQ, v.m2, v.m1 + v.nq + v.nsoc, v.A2, v.b2, nullptr, 0.0});
  std::vector<CostTile64Item> items;
  for (const ItemSource& it : src) {
    const bool run = it.type == CT_LIN || it.type == CT_EQ;
    items.push_back({rayen::cost_tile64_blocks(it.rows), run ? 0 : 1, run ? 1 : 0});
  }
  if (!rayen::cost_tile64_served(k, items.data(), (int64_t)items.size(), window_bytes)) return false;
  int64_t np = 0, total = 0;
  const int64_t nw = rayen::cost_tile64_partition(items.data(), (int64_t)items.size(), K, window_bytes, nullptr, 0, nullptr, 0,
                                                  &np, &total);
  std::vector<CostTile64Window> windows((size_t)nw);
  std::vector<CostTile64Piece> pieces((size_t)np);
  if (rayen::cost_tile64_partition(items.data(), (int64_t)items.size(), K, window_bytes, windows.data(), nw, pieces.data(), np,
                                   nullptr, nullptr) != nw)
    return false;
  const size_t table_words = (size_t)nw * kTableWords;
  out->assign(table_words + (size_t)(total / 4), 0);
  size_t at = table_words;      // 4-byte words (windows start on 16-byte boundaries: the table is 32 bytes a window)
  int64_t largest = 0;
  for (int64_t w = 0; w < nw; ++w) {
    const CostTile64Window& win = windows[(size_t)w];
    const int nb = win.blocks, nf = win.forms;
    const int rowc_off = nb * BLK, colv_off = rowc_off + nb * 16, fc_off = colv_off + nf * KF, desc_off = fc_off + nb;
    int32_t* tw = out->data() + w * kTableWords;
    tw[TW_OFF16] = (int32_t)(at / 4);
    tw[TW_N16] = (int32_t)(win.bytes / 16);
    tw[TW_COUNT] = nb;
    tw[TW_ROWC] = rowc_off;
    tw[TW_COLV] = colv_off;
    tw[TW_FC] = fc_off;
    tw[TW_DESC] = desc_off;
    // (the vector's storage and `at`, a multiple of 4 words, keep the doubles on 8-byte boundaries)
    double* dst = reinterpret_cast<double*>(out->data() + at);
    int32_t* desc = reinterpret_cast<int32_t*>(dst + desc_off);
    int lb = 0, lf = 0;
    for (int pc = 0; pc < win.pieces; ++pc) {
      const CostTile64Piece& piece = pieces[(size_t)win.piece0 + pc];
      const ItemSource& it = src[(size_t)piece.item];
      const bool run = it.type == CT_LIN || it.type == CT_EQ;
      for (int u = 0; u < piece.blocks; ++u, ++lb) {
        const int b = piece.block0 + u, row0 = 16 * b;
        const int rows = it.rows - row0 < 16 ? it.rows - row0 : 16;
        double* Wb = dst + (size_t)lb * BLK;
        for (int m = 0; m < rows; ++m) {
          const int r = row0 + m;
          for (int c = 0; c < k; ++c)
            Wb[cost_tile64_slot(m, c)] = it.type == CT_QUAD ? 0.5 * (it.A[(size_t)r * k + c] + it.A[(size_t)c * k + r])
                                                            : it.A[(size_t)r * k + c];
          if (it.rowc != nullptr) dst[rowc_off + lb * 16 + m] = it.rowc[r];
        }
        dst[fc_off + lb] = it.fconst;
        int32_t* d = desc + lb * kDescWords;
        d[0] = it.type;
        d[1] = run ? rows : it.rows;
        d[2] = run ? it.id0 + row0 : it.id0;
        d[3] = run ? 0 : lf;
        d[4] = run ? 1 : items[(size_t)piece.item].blocks;
      }
      if (!run) {
        for (int c = 0; c < k; ++c) dst[colv_off + lf * KF + c] = it.form[c];
        ++lf;
      }
    }
    if (lb != nb || lf != nf) return false;
    at += (size_t)(win.bytes / 4);
    if (win.bytes > largest) largest = win.bytes;
  }
  side->nw = (int)nw;
  side->K = K;
  side->buf_bytes = largest;
  return true;
}

size_t tile_lds(const CostTile64& s) { return (size_t)(s.nw > 1 ? 2 * s.buf_bytes : s.buf_bytes); }

template <int K, int NS, bool GRAD>
int launch(const RayenCostPack* p, const double* y, int64_t B, int64_t ld, double* cost, double* worst, int32_t* which,
           double* grad, int64_t ldg, hipStream_t stream) {
  const CostTile64& s = *p->tile64;
  auto kern = cost_tile64_kernel<K, NS, GRAD>;
  if (!rayen::allow_lds(kern, tile_lds(s))) return RAYEN_E_LAUNCH;
  const int64_t grid = rayen::persistent_grid(B, 16 * NS, rayen::launch_simds(p->n_simd), kWaves);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), tile_lds(s), stream, s.dev, s.nw, (int)s.buf_bytes, y, B, ld,
                     p->k, cost, worst, which, grad, ldg, p->eq_shift);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

bool rows_tiled(const RayenCostPack* p) { return p != nullptr && p->tile64 != nullptr && p->tile64->served; }

}  // namespace

extern "C" {

int rayen_cost_tile64_set(RayenCostPack* pack, int64_t window_bytes) {
  if (pack == nullptr || !rayen::cost_tile64_window_ok(window_bytes)) return RAYEN_E_BAD_ARG;
  const int64_t window = window_bytes == 0 ? rayen::kCostTile64Window : window_bytes;
  if (pack->tile64 != nullptr && pack->tile64->window_bytes == window) return RAYEN_OK;
  int rc = rayen::check_device(pack->device);
  if (rc != RAYEN_OK) return rc;
  CostTile64* t = new (std::nothrow) CostTile64();
  if (t == nullptr) return RAYEN_E_ALLOC;
  t->window_bytes = window;
  if (pack->k <= rayen::kCostTile64MaxK && pack->n_rows > 0) {
    try {
      std::vector<int32_t> words;
      t->served = build_tile64(tile_view(pack), window, &words, t);
      if (t->served && !rayen::upload_image(words, &t->dev)) {
        rayen::cost_tile64_free(t);
        return RAYEN_E_ALLOC;
      }
    } catch (const std::bad_alloc&) {
      rayen::cost_tile64_free(t);
      return RAYEN_E_ALLOC;
    }
  }
  rayen::cost_tile64_free(pack->tile64);      // (another window size: hipFree waits for the launches that read the old image)
  pack->tile64 = t;
  return RAYEN_OK;
}

int rayen_cost_tile64_served(const RayenCostPack* pack) {
  if (pack == nullptr || pack->tile64 == nullptr) return 0;
  return rayen::cost_serves_set<double>(pack, rows_tiled(pack)) ? 1 : 0;
}

int rayen_soft_cost_tile64_f64(const RayenCostPack* pack, const double* y, int64_t B, int64_t ld, double* cost, double* worst,
                               int32_t* which, double* grad, int64_t ld_grad, void* stream) {
  return rayen::cost_call<double>(pack, rows_tiled(pack), y, B, ld, cost, worst, which, grad, ld_grad, stream,
                                  [&](hipStream_t st) {
                                    return rayen::dispatch_width<8, 64>(pack->tile64->K, [&](auto Kc) {
                                      constexpr int K = decltype(Kc)::value;
                                      return grad != nullptr
                                                 ? launch<K, 2, true>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st)
                                                 : launch<K, 2, false>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st);
                                    });
                                  });
}

}  // extern "C"
