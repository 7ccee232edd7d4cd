// Wide sets (n > 128), fused: kappa, active and y in ONE launch from v and W_ext = [W ; NA_E]; the products matrix
// T = v W_ext' of the products route (rayen_wide.hip behind a library GEMM) never reaches memory.  Exact fp32
// (v_mfma_f32_32x32x2_f32 is an fmaf chain: the differences from the products route are summation order).
//
// A workgroup of four waves owns a tile of 32 consecutive samples, which it stages in LDS once ([32][ks], columns of a
// tail tile beyond B zero); a sample is a COLUMN of every product.  The rows of W_ext are cut into blocks of 32
// (rayen_wide_fused_layout.h); the waves split the blocks in contiguous runs.  For a block a wave accumulates the
// 32 rows x 32 samples product over K = n: lane l holds column l & 31; register i of the accumulator is row
// 8 (i >> 2) + 4 (l >> 5) + (i & 3).  Operands come in 16-byte pieces: half-wave h of a group of eight k reads
// k0 + 4 h .. k0 + 4 h + 3 of its row of W (global memory / L2) and of its sample (LDS), so MFMA j of the group pairs
// k0 + j with k0 + 4 + j on BOTH operands -- a permutation of k, which the sum does not see.
//
// While a block's accumulators are live the wave applies the reductions of wide_epilogue_kernel (rayen_wide.hip) to the
// segments that have rows in it -- LIN: max and arg-max (NaN wins, ties to the lower row), QUAD_SYM: sum T_j v_j,
// QUAD_FAC / SOC: sum T_j^2, and the aux rows as they are -- into its own slot of the per-sample scratch in LDS (folded
// over its blocks in rising order).  After a barrier lane s of wave 0 folds the waves' slots in rising order and applies
// that kernel's formulas: the arithmetic of a sample depends on the set alone, not on its tile-mates or on timing.
//
// y: with NA_E = I from the LDS tile.  Otherwise the blocks of NA_E follow those of W and their products are stored
// UNSCALED into y as they are produced (y is its own scratch); once kappa is known the same workgroup rescales them in
// place -- behind a device-scope fence and the workgroup barrier, which make its own stores visible to it.
// y == nullptr (computeKappa) skips those blocks.
//
// Rows outside a segment are masked ARITHMETICALLY (an all-ones / zero word from the row index) and the kernel comes in four
// instances (y wanted or not, NA_E = I or not): written with compares and run-time flags, the sixteen-row reductions left
// the compiler over 70 wave masks to keep, more than the scalar registers hold.
//
// The image is built the first time the route is asked for (never during stream capture: the call then answers
// RAYEN_E_NOT_PREPARED) from the pack's host copy of W and NA_E; a pack that never asks allocates nothing.
#include "rayen_wide_fused_common.h"

namespace rayen {

namespace {

constexpr int kThreads = 256;

struct Args {
  const float* W;
  const float* y0;
  const FSeg* segs;
  const int32_t* item_start;
  const FItem* items;
  int n_seg, n, k, kp, ks, nb_w, nb_e, rows_w_pad, scratch_words;
  const float* v;
  int64_t B, ldv;
  float* y;
  int64_t ldy;
  float* kappa;
  int32_t* active;
  int32_t* nan_flag;
};

__device__ __forceinline__ int block_start(int nb, int w) { return (int)((int64_t)nb * w / kWideFusedWaves); }

// (m, at) <- the larger of (m, at) and (bm, bat): NaN wins, ties (and two NaNs) go to the lower row
__device__ __forceinline__ void lin_merge(float& m, int& at, const float bm, const int bat) {
  const bool lower = bat >= 0 && (at < 0 || bat < at);
  const bool take = (bm != bm) ? (!(m != m) || lower) : (bm > m || (bm == m && lower));
  if (take) { m = bm; at = bat; }
}

// WANT_Y: a.y != nullptr; IDENTITY: NA_E = I (instances, so that neither is a predicate the loops carry)
template <bool WANT_Y, bool IDENTITY>
__global__ __launch_bounds__(kThreads, 4) void wide_fused_kernel(const Args a) {
  extern __shared__ __align__(16) float wf_smem[];
  float* vt = wf_smem;                           // [32][ks]
  float* scr = vt + 32 * a.ks;                   // the segments' partials
  float* step = scr + a.scratch_words;           // [2][32]: 1 / max(1, kappa), NaN carry
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int groups = a.kp >> 3;
  const int64_t n_tiles = (a.B + 31) / 32;
  const int wb0 = block_start(a.nb_w, wave), wb1 = block_start(a.nb_w, wave + 1);
  const int eb0 = block_start(a.nb_e, wave), eb1 = block_start(a.nb_e, wave + 1);
  const float* brow = vt + col * a.ks + 4 * half;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // the tile of v: eight samples a wave, rows read along k
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int s = wave * 8 + r;
      const int64_t smp = tile * 32 + s;
      const bool in = smp < a.B;
      const float* __restrict__ vr = a.v + (in ? smp : 0) * a.ldv;
      for (int j = lane; j < a.kp; j += 64) vt[s * a.ks + j] = (in && j < a.n) ? vr[j] : 0.0f;
    }
    __syncthreads();
    const int64_t sample = tile * 32 + col;
    const bool live = sample < a.B;
    // this wave's blocks of W, then (sets with equality constraints, y wanted) its blocks of NA_E: one walk
    const int n_w = wb1 - wb0, n_e = (WANT_Y && !IDENTITY) ? eb1 - eb0 : 0;
    float* yr = a.y + (live ? sample : 0) * a.ldy;
#pragma unroll 1
    for (int t = 0; t < n_w + n_e; ++t) {
      const bool of_e = t >= n_w;
      const int b = of_e ? eb0 + (t - n_w) : wb0 + t;
      const size_t row0 = (size_t)b * 32 + (of_e ? a.rows_w_pad : 0);
      const f32x16 acc = block_product(a.W + (row0 + col) * a.kp + 4 * half, brow, groups);
      if (of_e) {
        // NA_E v, unscaled, into y
        if (live) {
          const int left = a.k - 32 * b;              // rows of this block that exist
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (row_of(i, half) < left) yr[32 * b + row_of(i, half)] = acc[i];
        }
        continue;
      }
      const int it1 = a.item_start[b + 1];
#pragma unroll 1
      for (int it = a.item_start[b]; it < it1; ++it) {
        const FItem item = a.items[it];
        const FSeg& sg = a.segs[item.seg];
        if (item.kind != 0) {
          // an aux row of the segment, as it is: one lane of the column holds it
          const int rr = sg.aux_row + (item.kind - 1) - 32 * b;
          int bits = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int x = row_of(i, half) ^ rr;
            bits |= __float_as_int(acc[i]) & ~((x | -x) >> 31);          // (all ones where the row is rr)
          }
          if (((rr >> 2) & 1) == half) scr[sg.aux_off + (item.kind - 1) * 32 + col] = __int_as_float(bits);
          continue;
        }
        const int lo = sg.row0 - 32 * b;          // the segment's first row, in rows of this block
        const bool first = b == (sg.first_block > wb0 ? sg.first_block : wb0);      // this wave's first block of the segment
        if (sg.type == RAYEN_SEG_LIN) {
          float m = 0.0f;
          int at = -1;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            // (rows rise with i inside a lane: the first NaN and the first of equal values stay)
            const int j = row_of(i, half) - lo;
            const int msk = (~j & (j - sg.nrows)) >> 31;            // all ones inside the segment
            const float t = __int_as_float((__float_as_int(acc[i]) & msk) | (0xff800000 & ~msk));
            const bool take = (t != t) ? !(m != m) : t > m;
            m = take ? t : m;
            at = take ? j : at;
          }
          lin_merge(m, at, __shfl_xor(m, 32, 64), __shfl_xor(at, 32, 64));
          if (half == 0) {
            float* p = scr + sg.part_off + (wave - sg.wave_first) * 64;
            if (!first) {
              const float pm = p[col];
              const int pat = __float_as_int(p[32 + col]);
              lin_merge(m, at, pm, pat);
            }
            p[col] = m;
            p[32 + col] = __int_as_float(at);
          }
        } else {
          float sum = 0.0f;
          if (sg.type == RAYEN_SEG_QUAD_SYM) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int j = row_of(i, half) - lo;
              const int msk = (~j & (j - sg.nrows)) >> 31;
              const float vj = __int_as_float(__float_as_int(vt[col * a.ks + (j & msk)]) & msk);
              sum = fmaf(__int_as_float(__float_as_int(acc[i]) & msk), vj, sum);
            }
          } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int j = row_of(i, half) - lo;
              const float t = __int_as_float(__float_as_int(acc[i]) & ((~j & (j - sg.nrows)) >> 31));
              sum = fmaf(t, t, sum);
            }
          }
          sum += __shfl_xor(sum, 32, 64);
          if (half == 0) {
            float* p = scr + sg.part_off + (wave - sg.wave_first) * 32;
            p[col] = first ? sum : p[col] + sum;
          }
        }
      }
    }
    if (WANT_Y && !IDENTITY) __threadfence();       // the stores above are read back below by other waves of this workgroup
    __syncthreads();
    if (threadIdx.x < 32) {
      // the formulas of wide_epilogue_kernel (rayen_wide.hip) on the folded partials of sample `col`
      float kap = 0.0f;
      int aseg = -1, arow = 0;
      for (int g = 0; g < a.n_seg; ++g) {
        const FSeg& sg = a.segs[g];
        if (sg.type == RAYEN_SEG_LIN) {
          float m = 0.0f;
          int at = -1;
          for (int w = sg.wave_first; w <= sg.wave_last; ++w) {
            if (block_start(a.nb_w, w) == block_start(a.nb_w, w + 1)) continue;       // a wave without a block
            const float* p = scr + sg.part_off + (w - sg.wave_first) * 64;
            lin_merge(m, at, p[col], __float_as_int(p[32 + col]));
          }
          if (m > kap || (m != m)) { kap = m; aseg = g; arow = sg.row0 + at; }
        } else if (sg.type == RAYEN_SEG_QUAD_SYM || sg.type == RAYEN_SEG_QUAD_FAC || sg.type == RAYEN_SEG_SOC) {
          float acc = 0.0f;
          for (int w = sg.wave_first; w <= sg.wave_last; ++w) {
            if (block_start(a.nb_w, w) == block_start(a.nb_w, w + 1)) continue;
            acc += scr[sg.part_off + (w - sg.wave_first) * 32 + col];
          }
          float cand;
          if (sg.type != RAYEN_SEG_SOC) {
            cand = scr[sg.aux_off + col] + sqrtf(fmaxf(acc, 0.0f));
          } else {
            // a' x^2 + b' x + c' = 0 with a' = f1 < 0, tau = f0; a ray that never meets the cone contributes 0
            const float cr = scr[sg.aux_off + col], br = scr[sg.aux_off + 32 + col];
            const float cp = acc - cr * cr;
            const float bp = 2.0f * br - 2.0f * cr * sg.f0;
            const float disc = bp * bp - 4.0f * sg.f1 * cp;
            cand = 0.0f;
            if (disc >= 0.0f) {
              const float root = sqrtf(disc), inv2a = 0.5f / sg.f1;
              cand = fmaxf((-bp - root) * inv2a, (-bp + root) * inv2a);
            } else if (disc != disc) {
              cand = disc;
            }
          }
          if (cand > kap || (cand != cand)) { kap = cand; aseg = g; arow = 0; }
        }
      }
      step[col] = 1.0f / fmaxf(1.0f, kap);      // (fmax drops a NaN kappa; the outputs carry it through `kap` itself)
      step[32 + col] = (kap != kap) ? kap : 0.0f;
      if (live) {
        // (the two null tests are made here, from pointers the optimiser cannot see through: hoisted out of the tile loop
        // they were the last scalars the register allocator had to park in a VGPR's lanes)
        float* kappa_out = a.kappa;
        int32_t* active_out = a.active;
        asm volatile("" : "+s"(kappa_out), "+s"(active_out));
        if (kappa_out) kappa_out[sample] = kap;
        if (active_out) { active_out[2 * sample] = aseg; active_out[2 * sample + 1] = arow; }
      }
    }
    __syncthreads();
    if (WANT_Y) {
#pragma unroll 1
      for (int r = 0; r < 8; ++r) {
        const int s = wave * 8 + r;
        const int64_t smp = tile * 32 + s;
        if (smp >= a.B) break;
        float* yr = a.y + smp * a.ldy;
        const float scale = step[s], carry = step[32 + s];
        for (int i = lane; i < a.k; i += 64) {
          const float src = IDENTITY ? vt[s * a.ks + i] : yr[i];
          const float o = fmaf(src, scale, a.y0[i]) + carry;
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

bool shape_served(const RayenPack* p, WideFusedPlan* plan, std::vector<WideFusedSegPlan>* seg_plans) {
  if (p == nullptr || p->wide == nullptr) return false;            // (no tables: the set has an LMI)
  std::vector<WideFusedSegIn> in;
  seg_inputs(p, &in);
  std::vector<WideFusedSegPlan> sp(in.size());
  const WideFusedPlan pl = wide_fused_plan(p->n, p->k, p->n_rows, p->out_identity, in.data(), (int32_t)in.size(), sp.data());
  if (plan) *plan = pl;
  if (seg_plans) seg_plans->swap(sp);
  return pl.served != 0;
}

void image_free(WideFusedImage* img) {
  if (img == nullptr) return;
  if (img->W) (void)hipFree(img->W);
  if (img->y0) (void)hipFree(img->y0);
  if (img->segs) (void)hipFree(img->segs);
  if (img->item_start) (void)hipFree(img->item_start);
  if (img->items) (void)hipFree(img->items);
  delete img;
}

int image_build(const RayenPack* p, WideFusedImage** out) {
  *out = nullptr;
  WideFusedPlan plan;
  std::vector<WideFusedSegPlan> sp;
  if (!shape_served(p, &plan, &sp)) return RAYEN_E_UNSUPPORTED;
  WideFusedImage* img = new WideFusedImage();
  img->plan = plan;
  img->n_seg = (int)p->segs.size();
  img->n_simd = device_simds(p->device, 1024);
  const std::vector<float> W = wide_fused_rows_image(p, plan);
  std::vector<float> y0(p->y0.begin(), p->y0.end());
  std::vector<FSeg> segs;
  std::vector<std::vector<FItem>> per_block((size_t)plan.nb_w);
  for (size_t i = 0; i < p->segs.size(); ++i) {
    const RayenSegment& g = p->segs[i];
    const WideFusedSegPlan& s = sp[i];
    segs.push_back(FSeg{g.type, g.row0, g.nrows, g.aux_row, s.first_block, s.last_block, s.wave_first, s.wave_last, s.part_off,
                        s.aux_off, (float)g.f0, (float)g.f1});
    for (int b = s.first_block; b <= s.last_block; ++b) per_block[(size_t)b].push_back(FItem{(int32_t)i, 0});
    const int naux = (g.type == RAYEN_SEG_QUAD_SYM || g.type == RAYEN_SEG_QUAD_FAC) ? 1 : (g.type == RAYEN_SEG_SOC ? 2 : 0);
    for (int x = 0; x < naux; ++x) per_block[(size_t)((g.aux_row + x) / 32)].push_back(FItem{(int32_t)i, 1 + x});
  }
  std::vector<int32_t> item_start;
  std::vector<FItem> items;
  for (const auto& blk : per_block) {
    item_start.push_back((int32_t)items.size());
    items.insert(items.end(), blk.begin(), blk.end());
  }
  item_start.push_back((int32_t)items.size());
  if (items.empty()) items.push_back(FItem{0, 0});       // (no allocation of zero bytes)
  if (segs.empty()) segs.push_back(FSeg{});
  const bool ok = upload_to_device(W, &img->W, &img->bytes) && upload_to_device(y0, &img->y0, &img->bytes) &&
                  upload_to_device(segs, &img->segs, &img->bytes) && upload_to_device(item_start, &img->item_start, &img->bytes) &&
                  upload_to_device(items, &img->items, &img->bytes);
  if (!ok) { image_free(img); return RAYEN_E_ALLOC; }
  bool attr = true;
  auto want = [&](auto kern) {
    attr = attr && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kWideFusedLds) == hipSuccess;
  };
  want(wide_fused_kernel<false, false>); want(wide_fused_kernel<false, true>);
  want(wide_fused_kernel<true, false>); want(wide_fused_kernel<true, true>);
  if (!attr) {
    image_free(img);
    return RAYEN_E_LAUNCH;
  }
  *out = img;
  return RAYEN_OK;
}

}  // namespace

std::mutex& wide_fused_mutex() {
  static std::mutex m;
  return m;
}

bool wide_fused_served(const RayenPack* p) { return shape_served(p, nullptr, nullptr); }

void wide_fused_free(WideFusedImage* img) { image_free(img); }

int wide_fused_forward(const RayenPack* p, const float* v, int64_t B, int64_t ldv, float* y, int64_t ldy, float* kappa,
                       int32_t* active, int32_t* nan_flag, hipStream_t stream) {
  const WideFusedImage* img = nullptr;
  {
    std::lock_guard<std::mutex> lock(wide_fused_mutex());
    if (p->wf32_state == 0) {
      if (!shape_served(p, nullptr, nullptr)) {
        p->wf32_state = 2;
      } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
          return RAYEN_E_NOT_PREPARED;            // the image's uploads do not belong in a capture: ask once before it
        WideFusedImage* built = nullptr;
        const int rc = image_build(p, &built);
        if (rc != RAYEN_OK) return rc;
        p->wf32 = built;
        p->wf32_state = 1;
      }
    }
    if (p->wf32_state != 1) return RAYEN_E_UNSUPPORTED;
    img = p->wf32;
  }
  if (B == 0) return RAYEN_OK;
  const WideFusedPlan& pl = img->plan;
  Args a;
  a.W = img->W; a.y0 = img->y0; a.segs = img->segs; a.item_start = img->item_start; a.items = img->items;
  a.n_seg = img->n_seg; a.n = p->n; a.k = p->k; a.kp = pl.kp; a.ks = pl.ks; a.nb_w = pl.nb_w; a.nb_e = pl.nb_e;
  a.rows_w_pad = pl.rows_w_pad; a.scratch_words = pl.scratch_words;
  a.v = v; a.B = B; a.ldv = ldv; a.y = y; a.ldy = ldy; a.kappa = kappa; a.active = active; a.nan_flag = nan_flag;
  // workgroups a CU holds: LDS, and at most four waves a SIMD (the registers allow four)
  int64_t per_cu = (160 * 1024) / pl.lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  const int64_t slots = (int64_t)(launch_simds(img->n_simd) / 4) * per_cu;
  const unsigned grid = (unsigned)persistent_grid(B, kWideFusedTile, slots, 1);
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), (size_t)pl.lds_bytes, stream, a); };
  if (y == nullptr) {
    if (p->out_identity) launch(wide_fused_kernel<false, true>); else launch(wide_fused_kernel<false, false>);
  } else {
    if (p->out_identity) launch(wide_fused_kernel<true, true>); else launch(wide_fused_kernel<true, false>);
  }
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace rayen
