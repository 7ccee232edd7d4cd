// Wide sets in fp64 (n > 64), fused: kappa, active and y in ONE launch from v and W_ext = [W ; NA_E]; the products matrix
// T = v W_ext' of the products route (rayen_wide.hip behind a library GEMM) never reaches memory.  The fp64 twin of
// rayen_wide_fused.hip at the geometry of v_mfma_f64_16x16x4_f64; exact fp64 (the instruction is an fma chain: the
// differences from the products route are summation order).
//
// A workgroup of four waves owns a tile of S consecutive samples (S = 32 where the plan's LDS fits, else 16:
// rayen_wide_fused64_layout.h), which it stages in LDS once ([S][ks], columns of a tail tile beyond B zero); a sample is a
// COLUMN of every product.  The rows of W_ext are cut into blocks of 16; the waves split the blocks in contiguous runs.
// For a block a wave accumulates the 16 rows x S samples product over K = n, one accumulator per COLUMN BLOCK of 16
// samples: lane l holds column l & 15 of each, register i is row (l >> 4) + 4 i.  Operands come in 16-byte pieces: lane
// group g = l >> 4 of a group of eight k reads k0 + 2 g and k0 + 2 g + 1 of its row of W (global memory / L2) and of its
// sample (LDS), so the two MFMAs of the group take .x and .y on BOTH operands -- a permutation of k, which the sum does
// not see.  With S = 32 every piece of W feeds both column blocks: the image, twice the bytes of the fp32 one, is read
// once per 32 samples.
//
// The K loop of a column block runs TWO accumulator chains, the even and the odd groups of eight k, added at the end (the
// f64 MFMA is long: one chain leaves the pipe idle between dependent issues).  Both tile sizes run the same two chains, so
// the bits of a sample do not depend on S, on its column or on its tile-mates.
//
// Reductions, masks, scratch, the final pass and the treatment of y are those of rayen_wide_fused.hip on doubles: see
// there.  Rows outside a segment are masked arithmetically with 64-bit words.
// (the image, the MFMA macro and block_product<NC>: rayen_wide_fused64_common.h, shared with rayen_wide_fused_bwd64.hip)
#include "rayen_wide_fused64_common.h"

namespace rayen {

namespace {

constexpr int kThreads = 256;
constexpr int kMinWaves = 2;       // waves a SIMD the instances are compiled for at least
// workgroups a CU holds at most, by the registers of the instances of S (<= 102 VGPRs at S = 16,
// <= 142 at S = 32, of 512 a SIMD)
constexpr int per_cu_max(const int S) { return S == 16 ? 4 : 3; }

struct Args {
  const double* W;
  const double* y0;
  const F64Seg* segs;
  const int32_t* item_start;
  const FItem* items;
  int n_seg, n, k, kp, ks, nb_w, nb_e, rows_w_pad, scratch_words;
  const double* v;
  int64_t B, ldv;
  double* y;
  int64_t ldy;
  double* kappa;
  int32_t* active;
  int32_t* nan_flag;
};

__device__ __forceinline__ int block_start(int nb, int w) { return (int)((int64_t)nb * w / kWideFusedWaves); }

__device__ __forceinline__ long long bits_of(double x) { return __double_as_longlong(x); }
__device__ __forceinline__ double from_bits(long long x) { return __longlong_as_double(x); }
// all ones where 0 <= j < nrows
__device__ __forceinline__ long long inside(int j, int nrows) { return (long long)((~j & (j - nrows)) >> 31); }

// (m, at) <- the larger of (m, at) and (bm, bat): NaN wins, ties (and two NaNs) go to the lower row
__device__ __forceinline__ void lin_merge(double& m, int& at, const double bm, const int bat) {
  const bool lower = bat >= 0 && (at < 0 || bat < at);
  const bool take = (bm != bm) ? (!(m != m) || lower) : (bm > m || (bm == m && lower));
  if (take) { m = bm; at = bat; }
}

// WANT_Y: a.y != nullptr; IDENTITY: NA_E = I; S: samples of a tile (instances, so that none is a predicate the loops carry)
template <bool WANT_Y, bool IDENTITY, int S>
__global__ __launch_bounds__(kThreads, kMinWaves) void wide_fused64_kernel(const Args a) {
  constexpr int NC = S / 16, PER_WAVE = S / 4;
  extern __shared__ __align__(16) double wf64_smem[];
  double* vt = wf64_smem;                         // [S][ks]
  double* scr = vt + S * a.ks;                    // the segments' partials
  double* step = scr + a.scratch_words;           // [2][S]: 1 / max(1, kappa), NaN carry
  const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int groups = a.kp >> 3;
  const int64_t n_tiles = (a.B + S - 1) / S;
  const int wb0 = block_start(a.nb_w, wave), wb1 = block_start(a.nb_w, wave + 1);
  const int eb0 = block_start(a.nb_e, wave), eb1 = block_start(a.nb_e, wave + 1);
  const double* brow = vt + col * a.ks + 2 * grp;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // the tile of v: S / 4 samples a wave, rows read along k
#pragma unroll 1
    for (int r = 0; r < PER_WAVE; ++r) {
      const int s = wave * PER_WAVE + r;
      const int64_t smp = tile * S + s;
      const bool in = smp < a.B;
      const double* __restrict__ vr = a.v + (in ? smp : 0) * a.ldv;
      for (int j = lane; j < a.kp; j += 64) vt[s * a.ks + j] = (in && j < a.n) ? vr[j] : 0.0;
    }
    __syncthreads();
    // this wave's blocks of W, then (sets with equality constraints, y wanted) its blocks of NA_E: one walk
    const int n_w = wb1 - wb0, n_e = (WANT_Y && !IDENTITY) ? eb1 - eb0 : 0;
#pragma unroll 1
    for (int t = 0; t < n_w + n_e; ++t) {
      const bool of_e = t >= n_w;
      const int b = of_e ? eb0 + (t - n_w) : wb0 + t;
      const size_t row0 = (size_t)b * 16 + (of_e ? a.rows_w_pad : 0);
      f64x4 acc[NC];
      block_product<NC>(a.W + (row0 + col) * a.kp + 2 * grp, brow, a.ks, groups, acc);
      if (of_e) {
        // NA_E v, unscaled, into y
        const int left = a.k - 16 * b;              // rows of this block that exist
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int64_t sample = tile * S + 16 * c + col;
          if (sample < a.B) {
            double* yr = a.y + sample * a.ldy + 16 * b;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (grp + 4 * i < left) yr[grp + 4 * i] = acc[c][i];
          }
        }
        continue;
      }
      const int it1 = a.item_start[b + 1];
#pragma unroll 1
      for (int it = a.item_start[b]; it < it1; ++it) {
        const FItem item = a.items[it];
        const F64Seg& sg = a.segs[item.seg];
        if (item.kind != 0) {
          // an aux row of the segment, as it is: one lane of the column holds it
          const int rr = sg.aux_row + (item.kind - 1) - 16 * b;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            long long bits = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int x = (grp + 4 * i) ^ rr;
              bits |= bits_of(acc[c][i]) & ~(long long)((x | -x) >> 31);          // (all ones where the row is rr)
            }
            if ((rr & 3) == grp) scr[sg.aux_off + (item.kind - 1) * S + 16 * c + col] = from_bits(bits);
          }
          continue;
        }
        const int lo = sg.row0 - 16 * b;          // the segment's first row, in rows of this block
        const bool first = b == (sg.first_block > wb0 ? sg.first_block : wb0);      // this wave's first block of the segment
        if (sg.type == RAYEN_SEG_LIN) {
          double* p = scr + sg.part_off + (wave - sg.wave_first) * 2 * S;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            double m = 0.0;
            int at = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              // (rows rise with i inside a lane: the first NaN and the first of equal values stay)
              const int j = grp + 4 * i - lo;
              const long long msk = inside(j, sg.nrows);
              const double t = from_bits((bits_of(acc[c][i]) & msk) | (0xfff0000000000000ll & ~msk));
              const bool take = (t != t) ? !(m != m) : t > m;
              m = take ? t : m;
              at = take ? j : at;
            }
            lin_merge(m, at, __shfl_xor(m, 16, 64), __shfl_xor(at, 16, 64));
            lin_merge(m, at, __shfl_xor(m, 32, 64), __shfl_xor(at, 32, 64));
            if (grp == 0) {
              const int s = 16 * c + col;
              if (!first) lin_merge(m, at, p[s], (int)p[S + s]);
              p[s] = m;
              p[S + s] = (double)at;
            }
          }
        } else {
          double* p = scr + sg.part_off + (wave - sg.wave_first) * S;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            double sum = 0.0;
            if (sg.type == RAYEN_SEG_QUAD_SYM) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int j = grp + 4 * i - lo;
                const long long msk = inside(j, sg.nrows);
                const double vj = from_bits(bits_of(vt[(16 * c + col) * a.ks + (j & (int)msk)]) & msk);
                sum = fma(from_bits(bits_of(acc[c][i]) & msk), vj, sum);
              }
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int j = grp + 4 * i - lo;
                const double t = from_bits(bits_of(acc[c][i]) & inside(j, sg.nrows));
                sum = fma(t, t, sum);
              }
            }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            if (grp == 0) {
              const int s = 16 * c + col;
              p[s] = first ? sum : p[s] + sum;
            }
          }
        }
      }
    }
    if (WANT_Y && !IDENTITY) __threadfence();       // the stores above are read back below by other waves of this workgroup
    __syncthreads();
    if (threadIdx.x < S) {
      // the formulas of wide_epilogue_kernel<double> (rayen_wide.hip) on the folded partials of sample `s`
      const int s = threadIdx.x;
      const int64_t sample = tile * S + s;
      double kap = 0.0;
      int aseg = -1, arow = 0;
      for (int g = 0; g < a.n_seg; ++g) {
        const F64Seg& sg = a.segs[g];
        if (sg.type == RAYEN_SEG_LIN) {
          double m = 0.0;
          int at = -1;
          for (int w = sg.wave_first; w <= sg.wave_last; ++w) {
            if (block_start(a.nb_w, w) == block_start(a.nb_w, w + 1)) continue;       // a wave without a block
            const double* p = scr + sg.part_off + (w - sg.wave_first) * 2 * S;
            lin_merge(m, at, p[s], (int)p[S + s]);
          }
          if (m > kap || (m != m)) { kap = m; aseg = g; arow = sg.row0 + at; }
        } else if (sg.type == RAYEN_SEG_QUAD_SYM || sg.type == RAYEN_SEG_QUAD_FAC || sg.type == RAYEN_SEG_SOC) {
          double acc = 0.0;
          for (int w = sg.wave_first; w <= sg.wave_last; ++w) {
            if (block_start(a.nb_w, w) == block_start(a.nb_w, w + 1)) continue;
            acc += scr[sg.part_off + (w - sg.wave_first) * S + s];
          }
          double cand;
          if (sg.type != RAYEN_SEG_SOC) {
            cand = scr[sg.aux_off + s] + sqrt(fmax(acc, 0.0));
          } else {
            // a' x^2 + b' x + c' = 0 with a' = f1 < 0, tau = f0; a ray that never meets the cone contributes 0
            const double cr = scr[sg.aux_off + s], br = scr[sg.aux_off + S + s];
            const double cp = acc - cr * cr;
            const double bp = 2.0 * br - 2.0 * cr * sg.f0;
            const double disc = bp * bp - 4.0 * sg.f1 * cp;
            cand = 0.0;
            if (disc >= 0.0) {
              const double root = sqrt(disc), inv2a = 0.5 / sg.f1;
              cand = fmax((-bp - root) * inv2a, (-bp + root) * inv2a);
            } else if (disc != disc) {
              cand = disc;
            }
          }
          if (cand > kap || (cand != cand)) { kap = cand; aseg = g; arow = 0; }
        }
      }
      step[s] = 1.0 / fmax(1.0, kap);      // (fmax drops a NaN kappa; the outputs carry it through `kap` itself)
      step[S + s] = (kap != kap) ? kap : 0.0;
      if (sample < a.B) {
        // (the two null tests are made here, from pointers the optimiser cannot see through: hoisted out of the tile loop
        // they are scalars the register allocator has to park in a VGPR's lanes)
        double* kappa_out = a.kappa;
        int32_t* active_out = a.active;
        asm volatile("" : "+s"(kappa_out), "+s"(active_out));
        if (kappa_out) kappa_out[sample] = kap;
        if (active_out) { active_out[2 * sample] = aseg; active_out[2 * sample + 1] = arow; }
      }
    }
    __syncthreads();
    if (WANT_Y) {
#pragma unroll 1
      for (int r = 0; r < PER_WAVE; ++r) {
        const int s = wave * PER_WAVE + r;
        const int64_t smp = tile * S + s;
        if (smp >= a.B) break;
        double* yr = a.y + smp * a.ldy;
        const double scale = step[s], carry = step[S + s];
        for (int i = lane; i < a.k; i += 64) {
          const double src = IDENTITY ? vt[s * a.ks + i] : yr[i];
          const double o = fma(src, scale, a.y0[i]) + carry;
          bad |= (o != o);
          yr[i] = o;
        }
      }
    }
    __syncthreads();         // the tile and the scratch are rewritten by the next round
  }
  if (a.nan_flag && bad) atomicOr(a.nan_flag, 1);
}

void seg_inputs(const RayenPack* p, std::vector<WideFusedSegIn>* in) {
  for (const RayenSegment& g : p->segs) {
    const int naux = (g.type == RAYEN_SEG_QUAD_SYM || g.type == RAYEN_SEG_QUAD_FAC) ? 1 : (g.type == RAYEN_SEG_SOC ? 2 : 0);
    in->push_back(WideFusedSegIn{g.row0, g.nrows, g.type == RAYEN_SEG_LIN ? 2 : 1, naux});
  }
}

// the plan of a pack for a tile of `samples` samples (0: the plan's own choice); false where it is not served
bool shape_plan(const RayenPack* p, const int samples, WideFused64Plan* plan, std::vector<WideFusedSegPlan>* seg_plans) {
  if (p == nullptr || p->wide == nullptr) return false;            // (no tables: the set has an LMI)
  std::vector<WideFusedSegIn> in;
  seg_inputs(p, &in);
  std::vector<WideFusedSegPlan> sp(in.size());
  const WideFused64Plan pl =
      wide_fused64_plan(p->n, p->k, p->n_rows, p->out_identity, in.data(), (int32_t)in.size(), sp.data(), samples);
  if (plan) *plan = pl;
  if (seg_plans) seg_plans->swap(sp);
  return pl.served != 0;
}

void image_free(WideFused64Image* img) {
  if (img == nullptr) return;
  if (img->W) (void)hipFree(img->W);
  if (img->y0) (void)hipFree(img->y0);
  for (F64Seg* s : img->segs)
    if (s) (void)hipFree(s);
  if (img->item_start) (void)hipFree(img->item_start);
  if (img->items) (void)hipFree(img->items);
  delete img;
}

template <typename F>
void for_each_instance(F&& f) {
  f(wide_fused64_kernel<false, false, 16>); f(wide_fused64_kernel<false, true, 16>);
  f(wide_fused64_kernel<true, false, 16>); f(wide_fused64_kernel<true, true, 16>);
  f(wide_fused64_kernel<false, false, 32>); f(wide_fused64_kernel<false, true, 32>);
  f(wide_fused64_kernel<true, false, 32>); f(wide_fused64_kernel<true, true, 32>);
}

int image_build(const RayenPack* p, WideFused64Image** out) {
  *out = nullptr;
  WideFused64Plan plan16;
  std::vector<WideFusedSegPlan> sp[2];
  if (!shape_plan(p, 16, &plan16, &sp[0])) return RAYEN_E_UNSUPPORTED;       // (what fits 32 samples fits 16)
  WideFused64Image* img = new WideFused64Image();
  img->plan[0] = plan16;
  (void)shape_plan(p, 32, &img->plan[1], &sp[1]);
  img->n_seg = (int)p->segs.size();
  img->n_simd = device_simds(p->device, 1024);
  const std::vector<double> W = wide_fused64_rows_image(p, plan16.rows_w_pad, plan16.rows_pad, plan16.kp);
  std::vector<F64Seg> segs[2];
  std::vector<std::vector<FItem>> per_block((size_t)plan16.nb_w);
  for (size_t i = 0; i < p->segs.size(); ++i) {
    const RayenSegment& g = p->segs[i];
    for (int h = 0; h < 2; ++h) {
      const WideFusedSegPlan& s = sp[h][i];
      segs[h].push_back(F64Seg{g.type, g.row0, g.nrows, g.aux_row, s.first_block, s.last_block, s.wave_first, s.wave_last,
                               s.part_off, s.aux_off, g.f0, g.f1});
    }
    const WideFusedSegPlan& s = sp[0][i];
    for (int b = s.first_block; b <= s.last_block; ++b) per_block[(size_t)b].push_back(FItem{(int32_t)i, 0});
    const int naux = (g.type == RAYEN_SEG_QUAD_SYM || g.type == RAYEN_SEG_QUAD_FAC) ? 1 : (g.type == RAYEN_SEG_SOC ? 2 : 0);
    for (int x = 0; x < naux; ++x)
      per_block[(size_t)((g.aux_row + x) / kWideFused64Block)].push_back(FItem{(int32_t)i, 1 + x});
  }
  std::vector<int32_t> item_start;
  std::vector<FItem> items;
  for (const auto& blk : per_block) {
    item_start.push_back((int32_t)items.size());
    items.insert(items.end(), blk.begin(), blk.end());
  }
  item_start.push_back((int32_t)items.size());
  if (items.empty()) items.push_back(FItem{0, 0});       // (no allocation of zero bytes)
  for (auto& s : segs)
    if (s.empty()) s.push_back(F64Seg{});
  const bool ok = upload_to_device(W, &img->W, &img->bytes) && upload_to_device(p->y0, &img->y0, &img->bytes) &&
                  upload_to_device(segs[0], &img->segs[0], &img->bytes) && upload_to_device(segs[1], &img->segs[1], &img->bytes) &&
                  upload_to_device(item_start, &img->item_start, &img->bytes) && upload_to_device(items, &img->items, &img->bytes);
  if (!ok) { image_free(img); return RAYEN_E_ALLOC; }
  bool attr = true;
  for_each_instance([&](auto kern) {
    attr = attr && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kWideFused64Lds) == hipSuccess;
  });
  if (!attr) {
    image_free(img);
    return RAYEN_E_LAUNCH;
  }
  *out = img;
  return RAYEN_OK;
}

}  // namespace

bool wide_fused64_served(const RayenPack* p) { return shape_plan(p, 0, nullptr, nullptr); }

bool wide_fused64_plan_of(const RayenPack* p, const int samples, WideFused64Plan* plan) {
  WideFused64Plan pl;
  (void)shape_plan(p, samples, &pl, nullptr);
  if (p == nullptr || p->wide == nullptr) return false;
  *plan = pl;
  return true;
}

void wide_fused64_free(WideFused64Image* img) { image_free(img); }

int wide_fused64_forward(const RayenPack* p, const double* v, int64_t B, int64_t ldv, double* y, int64_t ldy, double* kappa,
                         int32_t* active, int32_t* nan_flag, int samples, hipStream_t stream) {
  const WideFused64Image* img = nullptr;
  {
    std::lock_guard<std::mutex> lock(wide_fused_mutex());
    if (p->wf64_state == 0) {
      if (!shape_plan(p, 0, nullptr, nullptr)) {
        p->wf64_state = 2;
      } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
          return RAYEN_E_NOT_PREPARED;            // the image's uploads do not belong in a capture: ask once before it
        WideFused64Image* built = nullptr;
        const int rc = image_build(p, &built);
        if (rc != RAYEN_OK) return rc;
        p->wf64 = built;
        p->wf64_state = 1;
      }
    }
    if (p->wf64_state != 1) return RAYEN_E_UNSUPPORTED;
    img = p->wf64;
  }
  // the tile: the caller's, or 32 samples where the plan serves them
  const int h = samples == 0 ? (img->plan[1].served ? 1 : 0) : (samples == 32 ? 1 : 0);
  const WideFused64Plan& pl = img->plan[h];
  if (!pl.served) return RAYEN_E_UNSUPPORTED;      // (a forced 32 beyond its LDS)
  if (B == 0) return RAYEN_OK;
  Args a;
  a.W = img->W; a.y0 = img->y0; a.segs = img->segs[h]; a.item_start = img->item_start; a.items = img->items;
  a.n_seg = img->n_seg; a.n = p->n; a.k = p->k; a.kp = pl.kp; a.ks = pl.ks; a.nb_w = pl.nb_w; a.nb_e = pl.nb_e;
  a.rows_w_pad = pl.rows_w_pad; a.scratch_words = pl.scratch_words;
  a.v = v; a.B = B; a.ldv = ldv; a.y = y; a.ldy = ldy; a.kappa = kappa; a.active = active; a.nan_flag = nan_flag;
  // workgroups a CU holds: LDS, and what the registers allow
  int64_t per_cu = (160 * 1024) / pl.lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > per_cu_max(pl.samples) ? per_cu_max(pl.samples) : per_cu);
  const int64_t slots = (int64_t)(launch_simds(img->n_simd) / 4) * per_cu;
  const unsigned grid = (unsigned)persistent_grid(B, pl.samples, slots, 1);
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), (size_t)pl.lds_bytes, stream, a); };
  const bool ident = p->out_identity != 0;
  if (h == 0) {
    if (y == nullptr) { if (ident) launch(wide_fused64_kernel<false, true, 16>); else launch(wide_fused64_kernel<false, false, 16>); }
    else { if (ident) launch(wide_fused64_kernel<true, true, 16>); else launch(wide_fused64_kernel<true, false, 16>); }
  } else {
    if (y == nullptr) { if (ident) launch(wide_fused64_kernel<false, true, 32>); else launch(wide_fused64_kernel<false, false, 32>); }
    else { if (ident) launch(wide_fused64_kernel<true, true, 32>); else launch(wide_fused64_kernel<true, false, 32>); }
  }
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace rayen
