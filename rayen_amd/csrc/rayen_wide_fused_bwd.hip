// Wide sets (n > 128), fused backward: grad_v from (v, kappa, active, grad_y) in ONE launch; neither the products matrix
// T = v W_ext' nor the coefficient matrix C of the products route (rayen_wide.hip::wide_bwd_coeff_kernel behind two library
// GEMMs) reaches memory, and only the rows of each sample's ACTIVE constraint are touched.  The arithmetic is that kernel's:
//   s = 1 / max(1, kappa), u = NA_E' g, tv = u . v, coef = kappa > 1 ? -s^2 tv : 0,
//   grad_v = s u + [kappa > 1] (the active segment's combination of rows of W)
// in exact fp32 on v_mfma_f32_32x32x2_f32 (an fmaf chain; against the products route the differences are summation order).
//
// The forward's skeleton (rayen_wide_fused.hip, rayen_wide_fused_common.h): a workgroup of four waves owns 32 samples, a
// sample is a COLUMN of every product, operands come in 16-byte pieces, no branch inside a K chunk.  Per tile:
//   1. u (sets with equality constraints): the tile's rows of grad_y in LDS, the image of NA_E' ([np][ke]) streamed past
//      them, u stored UNSCALED into grad_v (its own scratch; a device-scope fence and the barrier before the re-read).
//   2. a wave stages eight samples' v in LDS, folds tv = u . v over the row (lane partials, then the wave's tree: the
//      sample's own data alone), and writes s u -- plus coef W[row] for a sample that a linear row clipped -- over u.
//   3. the distinct NON-LINEAR active segments of the tile's clipped samples, in rising order (a wave-wide minimum over
//      the records in LDS): T = W_seg v in blocks of 32 rows dealt round-robin to the waves, folded per sample in registers
//      (sum T_j v_j | sum T_j^2, cr and br of a cone) and through four per-wave partials in LDS in fixed order; the closer
//      per sample; then sum_j c_j W[row0 + j] (n outputs x 32 samples, K = the segment's rows) against the segment's
//      TRANSPOSED image, the same loop.  c = v for QUAD_SYM (the v tile is the coefficient tile), c = T for QUAD_FAC and
//      SOC (an LDS tile [32][ts]); the factor (coef / rad | -2 q) scales the OUTPUT column, and columns of samples that do
//      not belong to the segment are computed and not stored -- a column depends on its own sample alone.
//   A row of grad_v is final when the workgroup leaves the tile; each of its words is read-modified-written at most once.
// The gradient bits of a sample depend on the set and that sample's inputs alone: not on its tile-mates, B, or `perm`.
//
// Grouping by active constraint: `perm` (tile t serves samples perm[32 t ..]) comes from three small launches -- count,
// scan, scatter over the keys of rayen_wide_fused_bwd_layout.h, in rayen_wide_fused_bwd_group.h (one source with the fp64
// backward) -- into the caller's workspace; no allocation, no host synchronisation, any number of segments.  Order inside a
// bucket is whatever the atomics give (no bit depends on it).
//
// Guards: an `active` record outside the segment table, a linear row outside its segment, !(kappa > 1) (NaN included) give
// s u alone; every row index of an image is clamped to the image.
#include "rayen_wide_fused_common.h"
#include "rayen_wide_fused_bwd_layout.h"
#include "rayen_wide_fused_bwd_group.h"

namespace rayen {

struct BSeg {   // 48 bytes
  int32_t type, row0, nrows, aux_row;
  int32_t rp, key;         // K of the transposed image (0: linear rows); 0 | 1 + d
  int64_t toff;            // the transposed image's first word in Wt
  float f0, f1;
  int32_t pad0, pad1;
};

struct WideFusedBwdImage {
  const float* W = nullptr;      // [rows_pad][kp]: the forward's image where it existed, else W_own
  float* W_own = nullptr;
  float* Wt = nullptr;           // the non-linear segments, transposed: segment d at toff, [np][rp_d]
  float* Et = nullptr;           // NA_E': [np][ke] (null with NA_E = I)
  BSeg* segs = nullptr;          // [n_seg]
  int n_seg = 0, n_nl = 0;
  int rows_pad = 0;
  int n_simd = 1024;
  WideFusedBwdPlan plan;
  int64_t bytes = 0;
};

namespace {

constexpr int kThreads = 256;
constexpr int kNoSeg = 0x7fffffff;

struct BArgs {
  const float* W;
  const float* Wt;
  const float* Et;
  const BSeg* segs;
  int n_seg, n, k, kp, ks, ke, gs, ts, np, rows_pad, region_words;
  const float* v;
  int64_t B, ldv;
  const float* kappa;
  const int32_t* active;
  const float* gy;
  int64_t ldg;
  float* gv;
  int64_t ldgv;
  const int32_t* perm;
};

__device__ __forceinline__ bool nonlinear(const int type) {
  return type == RAYEN_SEG_QUAD_SYM || type == RAYEN_SEG_QUAD_FAC || type == RAYEN_SEG_SOC;
}

// the row of the batch at place `idx` of the tiles' order, -1: none (beyond B, or a word of `perm` that names no row)
__device__ __forceinline__ int64_t sample_of(const BArgs& a, const int64_t idx) {
  if (idx >= a.B) return -1;
  const int64_t smp = a.perm ? (int64_t)a.perm[idx] : idx;
  return (smp >= 0 && smp < a.B) ? smp : -1;
}

// IDENTITY: NA_E = I (u = g, no step 1)
template <bool IDENTITY>
__global__ __launch_bounds__(kThreads, 3) void wide_fused_bwd_kernel(const BArgs a) {
  extern __shared__ __align__(16) float wb_smem[];
  float* vt = wb_smem;                            // [32][ks] (before it, in the same words: the g tile [32][gs])
  float* tt = vt + 32 * a.ks;                     // [32][ts]
  float* part = wb_smem + a.region_words;         // [4][32]
  float* crs = part + 128;
  float* brs = part + 160;
  int* asg = reinterpret_cast<int*>(part + 192);  // the sample's active non-linear segment, -1: none
  float* coefs = part + 224;
  float* kaps = part + 256;
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_tiles = (a.B + 31) / 32;
  const int nbo = a.np >> 5;
  const float* vb = vt + col * a.ks + 4 * half;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t idx = tile * 32 + col;
    const int64_t smp = sample_of(a, idx);
    const bool live = smp >= 0;
    float* out = a.gv + (live ? smp : 0) * a.ldgv;
    if (!IDENTITY) {
      // 1. u = NA_E' g, unscaled, into grad_v
      float* gt = wb_smem;
#pragma unroll 1
      for (int r = 0; r < 8; ++r) {
        const int s = wave * 8 + r;
        const int64_t sp = sample_of(a, tile * 32 + s);
        const bool in = sp >= 0;
        const int64_t sm = in ? sp : 0;
        const float* gr = a.gy + sm * a.ldg;
        for (int j = lane; j < a.ke; j += 64) gt[s * a.gs + j] = (in && j < a.k) ? gr[j] : 0.0f;
      }
      __syncthreads();
      const float* gb = gt + col * a.gs + 4 * half;
#pragma unroll 1
      for (int ob = wave; ob < nbo; ob += 4) {
        const f32x16 acc = block_product(a.Et + (size_t)(32 * ob + col) * a.ke + 4 * half, gb, a.ke >> 3);
        if (live) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int j = 32 * ob + row_of(i, half);
            if (j < a.n) out[j] = acc[i];
          }
        }
      }
      __threadfence();          // the stores above are read back below by other waves of this workgroup
      __syncthreads();
      __threadfence();
    }
    // 2. the tile of v; tv, the step and the records of eight samples a wave; s u (+ the one row of a linear constraint)
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int s = wave * 8 + r;
      const int64_t sp = sample_of(a, tile * 32 + s);
      const bool in = sp >= 0;
      const int64_t sm = in ? sp : 0;
      const float* vr = a.v + sm * a.ldv;
      float* gr_out = a.gv + sm * a.ldgv;
      const float* ur = IDENTITY ? a.gy + sm * a.ldg : gr_out;
      float tv = 0.0f;
      for (int j = lane; j < a.kp; j += 64) {
        const bool ok = in && j < a.n;
        const float vj = ok ? vr[j] : 0.0f;
        vt[s * a.ks + j] = vj;
        tv = fmaf(ok ? ur[j] : 0.0f, vj, tv);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) tv += __shfl_xor(tv, o, 64);
      const float kap = in ? a.kappa[sm] : 0.0f;
      const float sc = 1.0f / fmaxf(1.0f, kap);
      const bool clipped = kap > 1.0f;
      const float coef = clipped ? -sc * sc * tv : 0.0f;
      const int ag = in ? a.active[2 * sm] : -1;
      int nl = -1, linrow = -1;
      if (clipped && ag >= 0 && ag < a.n_seg) {
        const BSeg& sg = a.segs[ag];
        if (sg.type == RAYEN_SEG_LIN) {
          const int row = a.active[2 * sm + 1];
          if (row >= sg.row0 && row < sg.row0 + sg.nrows) linrow = row;
        } else if (nonlinear(sg.type)) {
          nl = ag;
        }
      }
      if (lane == 0) { asg[s] = nl; coefs[s] = coef; kaps[s] = kap; }
      if (in) {
        const float* wr = a.W + (size_t)(linrow >= 0 ? linrow : 0) * a.kp;
        for (int j = lane; j < a.n; j += 64) {
          const float su = sc * ur[j];
          gr_out[j] = linrow >= 0 ? fmaf(coef, wr[j], su) : su;
        }
      }
    }
    __threadfence();            // (step 3 adds to rows other waves wrote)
    __syncthreads();
    __threadfence();
    // 3. the distinct non-linear active segments of the tile, rising
    int cur = -1;
    for (;;) {
      int c = asg[col];
      c = c > cur ? c : kNoSeg;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const int oc = __shfl_xor(c, o, 64);
        c = oc < c ? oc : c;
      }
      c = __builtin_amdgcn_readfirstlane(c);
      if (c == kNoSeg) break;
      cur = c;
      const BSeg sg = a.segs[cur];
      const bool sym = sg.type == RAYEN_SEG_QUAD_SYM, soc = sg.type == RAYEN_SEG_SOC;
      const int nb1 = (sg.nrows + 31) >> 5;
      float sum = 0.0f;
#pragma unroll 1
      for (int bb = wave; bb < nb1 + (soc ? 1 : 0); bb += 4) {
        const bool aux = bb == nb1;                 // a cone's two aux rows: one more block, rows 0 and 1 of it
        int row = aux ? sg.aux_row + col : sg.row0 + 32 * bb + col;
        row = row < a.rows_pad - 1 ? row : a.rows_pad - 1;        // (rows beyond the segment are masked below)
        const f32x16 acc = block_product(a.W + (size_t)row * a.kp + 4 * half, vb, a.kp >> 3);
        if (aux) {
          if (half == 0) { crs[col] = acc[0]; brs[col] = acc[1]; }
          continue;
        }
        if (sym) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int j = 32 * bb + row_of(i, half);
            const bool in = j < sg.nrows;
            sum = fmaf(in ? acc[i] : 0.0f, vt[col * a.ks + (in ? j : 0)], sum);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int j = 32 * bb + row_of(i, half);
            const float t = j < sg.nrows ? acc[i] : 0.0f;
            sum = fmaf(t, t, sum);
            if (j < sg.rp) tt[col * a.ts + j] = t;
          }
        }
      }
      sum += __shfl_xor(sum, 32, 64);
      if (half == 0) part[wave * 32 + col] = sum;
      __syncthreads();
      const float acc2 = ((part[col] + part[32 + col]) + part[64 + col]) + part[96 + col];
      const bool member = live && asg[col] == cur;
      const float coef = coefs[col], kap = kaps[col];
      float so, a0, a1 = 0.0f;
      if (!soc) {
        const float rad = sqrtf(fmaxf(acc2, 0.0f));
        so = rad > 0.0f ? coef / rad : 0.0f;
        a0 = coef;
      } else {
        const float cr = crs[col], br = brs[col];
        const float bp = 2.0f * br - 2.0f * cr * sg.f0;
        const float den = 2.0f * sg.f1 * kap + bp;
        const float q = den != 0.0f ? coef / den : 0.0f;
        so = -2.0f * q;
        a0 = q * (2.0f * sg.f0 * kap + 2.0f * cr);
        a1 = -2.0f * q * kap;
      }
      const int aux1 = sg.aux_row + 1 < a.rows_pad ? sg.aux_row + 1 : a.rows_pad - 1;
      const float* w0 = a.W + (size_t)sg.aux_row * a.kp;
      const float* w1 = a.W + (size_t)aux1 * a.kp;
      const float* cb = sym ? vb : tt + col * a.ts + 4 * half;
      const float* timg = a.Wt + sg.toff;
#pragma unroll 1
      for (int ob = wave; ob < nbo; ob += 4) {
        const f32x16 acc = block_product(timg + (size_t)(32 * ob + col) * sg.rp + 4 * half, cb, sg.rp >> 3);
        if (member) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int j = 32 * ob + row_of(i, half);
            if (j < a.n) {
              float x = fmaf(a0, w0[j], out[j]);
              if (soc) x = fmaf(a1, w1[j], x);
              out[j] = fmaf(so, acc[i], x);
            }
          }
        }
      }
      __syncthreads();          // the T tile, the partials and the aux values are rewritten by the next segment
    }
    __syncthreads();            // the tile and the records are rewritten by the next round
  }
}

bool shape_served(const RayenPack* p, WideFusedBwdPlan* plan) {
  if (p == nullptr || p->wide == nullptr) return false;            // (no tables: the set has an LMI)
  int widest = 0;
  for (const RayenSegment& g : p->segs) {
    if (g.nrows < 0 || g.row0 < 0 || g.row0 + g.nrows > p->n_rows) return false;
    if (g.type == RAYEN_SEG_LIN) continue;
    if (g.type == RAYEN_SEG_QUAD_SYM) {
      if (g.nrows > p->n) return false;                            // (its coefficient tile is the v tile)
    } else if (g.type == RAYEN_SEG_QUAD_FAC || g.type == RAYEN_SEG_SOC) {
      widest = g.nrows > widest ? g.nrows : widest;
    } else {
      return false;
    }
    if (g.aux_row < 0 || g.aux_row + (g.type == RAYEN_SEG_SOC ? 1 : 0) >= p->n_rows) return false;
  }
  const WideFusedBwdPlan pl = wide_fused_bwd_plan(p->n, p->k, p->out_identity, widest);
  if (plan) *plan = pl;
  return pl.served != 0;
}

int count_nonlinear(const RayenPack* p) {
  int n = 0;
  for (const RayenSegment& g : p->segs) n += (g.type != RAYEN_SEG_LIN) ? 1 : 0;
  return n;
}

void image_free(WideFusedBwdImage* img) {
  if (img == nullptr) return;
  if (img->W_own) (void)hipFree(img->W_own);
  if (img->Wt) (void)hipFree(img->Wt);
  if (img->Et) (void)hipFree(img->Et);
  if (img->segs) (void)hipFree(img->segs);
  delete img;
}

// (under wide_fused_mutex) `fwd`: the forward's image where the pack has built one
int image_build(const RayenPack* p, const WideFusedImage* fwd, WideFusedBwdImage** out) {
  *out = nullptr;
  WideFusedBwdPlan plan;
  if (!shape_served(p, &plan)) return RAYEN_E_UNSUPPORTED;
  WideFusedBwdImage* img = new WideFusedBwdImage();
  img->plan = plan;
  img->n_seg = (int)p->segs.size();
  img->n_simd = device_simds(p->device, 1024);
  const int n = p->n, np = plan.np;
  bool ok = true;
  if (fwd != nullptr) {
    img->W = fwd->W;
    img->rows_pad = fwd->plan.rows_pad;
  } else {
    const WideFusedPlan rows = wide_fused_plan(n, p->k, p->n_rows, p->out_identity, nullptr, 0, nullptr);
    ok = upload_to_device(wide_fused_rows_image(p, rows), &img->W_own, &img->bytes);
    img->W = img->W_own;
    img->rows_pad = rows.rows_pad;
  }
  std::vector<BSeg> segs;
  std::vector<float> Wt;
  for (const RayenSegment& g : p->segs) {
    BSeg s{g.type, g.row0, g.nrows, g.aux_row, 0, 0, 0, (float)g.f0, (float)g.f1, 0, 0};
    if (g.type != RAYEN_SEG_LIN) {
      s.rp = wide_fused_bwd_pad8(g.nrows);
      s.key = 1 + img->n_nl++;
      s.toff = (int64_t)Wt.size();
      Wt.resize(Wt.size() + (size_t)np * s.rp, 0.0f);
      float* t = Wt.data() + s.toff;
      for (int r = 0; r < g.nrows; ++r)
        for (int j = 0; j < n; ++j) t[(size_t)j * s.rp + r] = (float)p->W[(size_t)(g.row0 + r) * n + j];
    }
    segs.push_back(s);
  }
  if (segs.empty()) segs.push_back(BSeg{});
  if (Wt.empty()) Wt.assign(8, 0.0f);                  // (no allocation of zero bytes)
  ok = ok && upload_to_device(segs, &img->segs, &img->bytes) && upload_to_device(Wt, &img->Wt, &img->bytes);
  if (ok && !p->out_identity) {
    std::vector<float> Et((size_t)np * plan.ke, 0.0f);
    for (int i = 0; i < p->k; ++i)
      for (int j = 0; j < n; ++j) Et[(size_t)j * plan.ke + i] = (float)p->NA_E[(size_t)i * n + j];
    ok = upload_to_device(Et, &img->Et, &img->bytes);
  }
  if (!ok) { image_free(img); return RAYEN_E_ALLOC; }
  bool attr = true;
  auto want = [&](auto kern) {
    attr = attr && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kWideFusedBwdLds) == hipSuccess;
  };
  want(wide_fused_bwd_kernel<false>); want(wide_fused_bwd_kernel<true>);
  if (!attr) {
    image_free(img);
    return RAYEN_E_LAUNCH;
  }
  *out = img;
  return RAYEN_OK;
}

}  // namespace

bool wide_fused_bwd_served(const RayenPack* p) { return shape_served(p, nullptr); }

int64_t wide_fused_bwd_workspace_bytes(const RayenPack* p, int64_t B) {
  if (!shape_served(p, nullptr)) return 0;
  return wide_fused_bwd_workspace(count_nonlinear(p), B);
}

void wide_fused_bwd_free(WideFusedBwdImage* img) { image_free(img); }

int wide_fused_backward(const RayenPack* p, const float* v, int64_t B, int64_t ldv, const float* kappa, const int32_t* active,
                        const float* grad_y, int64_t ldg, float* grad_v, int64_t ldgv, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream) {
  const WideFusedBwdImage* img = nullptr;
  {
    std::lock_guard<std::mutex> lock(wide_fused_mutex());
    if (p->wfb32_state == 0) {
      if (!shape_served(p, nullptr)) {
        p->wfb32_state = 2;
      } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
          return RAYEN_E_NOT_PREPARED;            // the images' uploads do not belong in a capture: ask once before it
        WideFusedBwdImage* built = nullptr;
        const int rc = image_build(p, p->wf32_state == 1 ? p->wf32 : nullptr, &built);
        if (rc != RAYEN_OK) return rc;
        p->wfb32 = built;
        p->wfb32_state = 1;
      }
    }
    if (p->wfb32_state != 1) return RAYEN_E_UNSUPPORTED;
    img = p->wfb32;
  }
  if (B == 0) return RAYEN_OK;
  const WideFusedBwdPlan& pl = img->plan;
  // the permutation, where the caller brought room for it (rayen_wide_fused_bwd_group.h)
  const int32_t* perm = nullptr;
  if (!bwd_group<float, BSeg>(img->segs, img->n_seg, img->n_nl, img->n_simd, kappa, active, B, workspace, workspace_bytes,
                              stream, &perm))
    return RAYEN_E_LAUNCH;
  BArgs a;
  a.W = img->W; a.Wt = img->Wt; a.Et = img->Et; a.segs = img->segs;
  a.n_seg = img->n_seg; a.n = p->n; a.k = p->k; a.kp = pl.kp; a.ks = pl.ks; a.ke = pl.ke; a.gs = pl.gs; a.ts = pl.ts;
  a.np = pl.np; a.rows_pad = img->rows_pad; a.region_words = pl.region_words;
  a.v = v; a.B = B; a.ldv = ldv; a.kappa = kappa; a.active = active; a.gy = grad_y; a.ldg = ldg; a.gv = grad_v; a.ldgv = ldgv;
  a.perm = perm;
  // workgroups a CU holds: LDS, and at most three waves a SIMD (the registers allow three)
  int64_t per_cu = (160 * 1024) / pl.lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > 3 ? 3 : per_cu);
  const int64_t slots = (int64_t)(launch_simds(img->n_simd) / 4) * per_cu;
  const unsigned grid = (unsigned)persistent_grid(B, 32, slots, 1);
  if (p->out_identity)
    hipLaunchKernelGGL(wide_fused_bwd_kernel<true>, dim3(grid), dim3(kThreads), (size_t)pl.lds_bytes, stream, a);
  else
    hipLaunchKernelGGL(wide_fused_bwd_kernel<false>, dim3(grid), dim3(kThreads), (size_t)pl.lds_bytes, stream, a);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace rayen
