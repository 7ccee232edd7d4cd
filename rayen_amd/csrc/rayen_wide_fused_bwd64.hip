// Wide sets in fp64 (n > 64), fused backward: grad_v from (v, kappa, active, grad_y) in ONE launch; neither the products
// matrix T = v W_ext' nor the coefficient matrix C of the products route (rayen_wide.hip::wide_bwd_coeff_kernel behind two
// library GEMMs) reaches memory, and only the rows of each sample's ACTIVE constraint are touched.  The fp64 twin of
// rayen_wide_fused_bwd.hip -- its algorithm step for step, its arithmetic, guards and closers the same formulas on doubles:
//   s = 1 / max(1, kappa), u = NA_E' g, tv = u . v, coef = kappa > 1 ? -s^2 tv : 0,
//   grad_v = s u + [kappa > 1] (the active segment's combination of rows of W)
// -- at the geometry of the fp64 fused forward (rayen_wide_fused64.hip, rayen_wide_fused64_common.h): exact fp64 on
// v_mfma_f64_16x16x4_f64 (an fma chain; against the products route the differences are summation order).
//
// A workgroup of four waves owns S samples (32 where the plan's LDS fits, else 16: rayen_wide_fused_bwd64_layout.h); rows and
// outputs go in blocks of 16, a sample is a COLUMN: lane l holds column l & 15 of each of the S / 16 column blocks, register
// i is row (l >> 4) + 4 i.  Operands come in 16-byte pieces, and every column block sums K in TWO accumulator chains, the
// even and the odd groups of eight k.  At S = 32 a wave keeps two column blocks: each piece of an image it reads feeds both.
// Per tile:
//   1. u (sets with equality constraints): the tile's rows of grad_y in LDS, the image of NA_E' ([np][ke]) streamed past
//      them, u stored UNSCALED into grad_v (its own scratch; a device-scope fence and the barrier before the re-read).
//   2. a wave stages S / 4 samples' v in LDS, folds tv = u . v over the row (lane partials, then the wave's tree: the
//      sample's own data alone), and writes s u -- plus coef W[row] for a sample that a linear row clipped -- over u.
//   3. the distinct NON-LINEAR active segments of the tile's clipped samples, in rising order (a wave-wide minimum over
//      the records in LDS): T = W_seg v in blocks of 16 rows dealt round-robin to the waves, folded per sample in registers
//      (sum T_j v_j | sum T_j^2, cr and br of a cone) and through four per-wave partials in LDS in fixed order; the closer
//      per sample; then sum_j c_j W[row0 + j] (n outputs x S samples, K = the segment's rows) against the segment's
//      TRANSPOSED image, the same loop.  c = v for QUAD_SYM (the v tile is the coefficient tile), c = T for QUAD_FAC and
//      SOC (an LDS tile [S][ts]); the factor (coef / rad | -2 q) scales the OUTPUT column, and columns of samples that do
//      not belong to the segment are computed and not stored -- a column depends on its own sample alone.
//   A row of grad_v is final when the workgroup leaves the tile; each of its words is read-modified-written at most once.
// Both tile sizes run the same two chains, the same deal of blocks to waves and the same folds: the gradient bits of a sample
// depend on the set and that sample's inputs alone -- not on S, its column, its tile-mates, B, or `perm`.
//
// Grouping by active constraint (`perm`): rayen_wide_fused_bwd_group.h, one source with the fp32 backward.
//
// Guards: an `active` record outside the segment table, a linear row outside its segment, !(kappa > 1) (NaN included) give
// s u alone; every row index of an image is clamped to the image.
#include "rayen_wide_fused64_common.h"
#include "rayen_wide_fused_bwd64_layout.h"
#include "rayen_wide_fused_bwd_group.h"

namespace rayen {

struct B64Seg {   // 48 bytes
  int32_t type, row0, nrows, aux_row;
  int32_t rp, key;         // K of the transposed image (0: linear rows); 0 | 1 + d
  int64_t toff;            // the transposed image's first word in Wt
  double f0, f1;
};

struct WideFusedBwd64Image {
  const double* W = nullptr;     // [rows_pad][kp]: the fp64 forward's image where it existed, else W_own
  double* W_own = nullptr;
  double* Wt = nullptr;          // the non-linear segments, transposed: segment d at toff, [np][rp_d]
  double* Et = nullptr;          // NA_E': [np][ke] (null with NA_E = I)
  B64Seg* segs = nullptr;        // [n_seg]
  int n_seg = 0, n_nl = 0;
  int rows_pad = 0;
  int n_simd = 1024;
  WideFusedBwd64Plan plan[2];    // S = 16 | 32
  int64_t bytes = 0;
};

namespace {

constexpr int kThreads = 256;
constexpr int kMinWaves = 2;       // waves a SIMD the instances are compiled for at least
constexpr int kNoSeg = 0x7fffffff;
// workgroups a CU holds at most, by the registers of the instances of S (<= 131 VGPRs at S = 16,
// <= 189 at S = 32, of 512 a SIMD)
constexpr int per_cu_max(const int S) { return S == 16 ? 3 : 2; }

struct BArgs {
  const double* W;
  const double* Wt;
  const double* Et;
  const B64Seg* segs;
  int n_seg, n, k, kp, ks, ke, gs, ts, np, rows_pad, region_words;
  const double* v;
  int64_t B, ldv;
  const double* kappa;
  const int32_t* active;
  const double* gy;
  int64_t ldg;
  double* gv;
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

// IDENTITY: NA_E = I (u = g, no step 1); S: samples of a tile
template <bool IDENTITY, int S>
__global__ __launch_bounds__(kThreads, kMinWaves) void wide_fused_bwd64_kernel(const BArgs a) {
  constexpr int NC = S / 16, PER_WAVE = S / 4;
  extern __shared__ __align__(16) double wb64_smem[];
  double* vt = wb64_smem;                           // [S][ks] (before it, in the same words: the g tile [S][gs])
  double* tt = vt + S * a.ks;                       // [S][ts]
  double* part = wb64_smem + a.region_words;        // [4][S]
  double* crs = part + 4 * S;
  double* brs = part + 5 * S;
  int* asg = reinterpret_cast<int*>(part + 6 * S);  // the sample's active non-linear segment, -1: none
  double* coefs = part + 7 * S;
  double* kaps = part + 8 * S;
  const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_tiles = (a.B + S - 1) / S;
  const int nbo = a.np >> 4;
  const double* vb = vt + col * a.ks + 2 * grp;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    bool live[NC];
    double* out[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int64_t smp = sample_of(a, tile * S + 16 * c + col);
      live[c] = smp >= 0;
      out[c] = a.gv + (live[c] ? smp : 0) * a.ldgv;
    }
    if (!IDENTITY) {
      // 1. u = NA_E' g, unscaled, into grad_v
      double* gt = wb64_smem;
#pragma unroll 1
      for (int r = 0; r < PER_WAVE; ++r) {
        const int s = wave * PER_WAVE + r;
        const int64_t sp = sample_of(a, tile * S + s);
        const bool in = sp >= 0;
        const int64_t sm = in ? sp : 0;
        const double* gr = a.gy + sm * a.ldg;
        for (int j = lane; j < a.ke; j += 64) gt[s * a.gs + j] = (in && j < a.k) ? gr[j] : 0.0;
      }
      __syncthreads();
      const double* gb = gt + col * a.gs + 2 * grp;
#pragma unroll 1
      for (int ob = wave; ob < nbo; ob += 4) {
        f64x4 acc[NC];
        block_product<NC>(a.Et + (size_t)(16 * ob + col) * a.ke + 2 * grp, gb, a.gs, a.ke >> 3, acc);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (live[c]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * ob + grp + 4 * i;
              if (j < a.n) out[c][j] = acc[c][i];
            }
          }
        }
      }
      __threadfence();          // the stores above are read back below by other waves of this workgroup
      __syncthreads();
      __threadfence();
    }
    // 2. the tile of v; tv, the step and the records of S / 4 samples a wave; s u (+ the one row of a linear constraint)
#pragma unroll 1
    for (int r = 0; r < PER_WAVE; ++r) {
      const int s = wave * PER_WAVE + r;
      const int64_t sp = sample_of(a, tile * S + s);
      const bool in = sp >= 0;
      const int64_t sm = in ? sp : 0;
      const double* vr = a.v + sm * a.ldv;
      double* gr_out = a.gv + sm * a.ldgv;
      const double* ur = IDENTITY ? a.gy + sm * a.ldg : gr_out;
      double tv = 0.0;
      for (int j = lane; j < a.kp; j += 64) {
        const bool ok = in && j < a.n;
        const double vj = ok ? vr[j] : 0.0;
        vt[s * a.ks + j] = vj;
        tv = fma(ok ? ur[j] : 0.0, vj, tv);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) tv += __shfl_xor(tv, o, 64);
      const double kap = in ? a.kappa[sm] : 0.0;
      const double sc = 1.0 / fmax(1.0, kap);
      const bool clipped = kap > 1.0;
      const double coef = clipped ? -sc * sc * tv : 0.0;
      const int ag = in ? a.active[2 * sm] : -1;
      int nl = -1, linrow = -1;
      if (clipped && ag >= 0 && ag < a.n_seg) {
        const B64Seg& sg = a.segs[ag];
        if (sg.type == RAYEN_SEG_LIN) {
          const int row = a.active[2 * sm + 1];
          if (row >= sg.row0 && row < sg.row0 + sg.nrows) linrow = row;
        } else if (nonlinear(sg.type)) {
          nl = ag;
        }
      }
      if (lane == 0) { asg[s] = nl; coefs[s] = coef; kaps[s] = kap; }
      if (in) {
        const double* wr = a.W + (size_t)(linrow >= 0 ? linrow : 0) * a.kp;
        for (int j = lane; j < a.n; j += 64) {
          const double su = sc * ur[j];
          gr_out[j] = linrow >= 0 ? fma(coef, wr[j], su) : su;
        }
      }
    }
    __threadfence();            // (step 3 adds to rows other waves wrote)
    __syncthreads();
    __threadfence();
    // 3. the distinct non-linear active segments of the tile, rising
    int cur = -1;
    for (;;) {
      int cm = asg[lane & (S - 1)];
      cm = cm > cur ? cm : kNoSeg;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(cm, o, 64);
        cm = oc < cm ? oc : cm;
      }
      cm = __builtin_amdgcn_readfirstlane(cm);
      if (cm == kNoSeg) break;
      cur = cm;
      const B64Seg sg = a.segs[cur];
      const bool sym = sg.type == RAYEN_SEG_QUAD_SYM, soc = sg.type == RAYEN_SEG_SOC;
      const int nb1 = (sg.nrows + 15) >> 4;
      double sum[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) sum[c] = 0.0;
#pragma unroll 1
      for (int bb = wave; bb < nb1 + (soc ? 1 : 0); bb += 4) {
        const bool aux = bb == nb1;                 // a cone's two aux rows: one more block, rows 0 and 1 of it
        int row = aux ? sg.aux_row + col : sg.row0 + 16 * bb + col;
        row = row < a.rows_pad - 1 ? row : a.rows_pad - 1;        // (rows beyond the segment are masked below)
        f64x4 acc[NC];
        block_product<NC>(a.W + (size_t)row * a.kp + 2 * grp, vb, a.ks, a.kp >> 3, acc);
        if (aux) {
          // (row 0 of the block is register 0 of lane group 0, row 1 register 0 of lane group 1)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (grp == 0) crs[16 * c + col] = acc[c][0];
            if (grp == 1) brs[16 * c + col] = acc[c][0];
          }
          continue;
        }
        if (sym) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * bb + grp + 4 * i;
              const bool in = j < sg.nrows;
              sum[c] = fma(in ? acc[c][i] : 0.0, vt[(16 * c + col) * a.ks + (in ? j : 0)], sum[c]);
            }
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * bb + grp + 4 * i;
              const double t = j < sg.nrows ? acc[c][i] : 0.0;
              sum[c] = fma(t, t, sum[c]);
              if (j < sg.rp) tt[(16 * c + col) * a.ts + j] = t;
            }
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        sum[c] += __shfl_xor(sum[c], 16, 64);
        sum[c] += __shfl_xor(sum[c], 32, 64);
        if (grp == 0) part[wave * S + 16 * c + col] = sum[c];
      }
      __syncthreads();
      const int aux1 = sg.aux_row + 1 < a.rows_pad ? sg.aux_row + 1 : a.rows_pad - 1;
      const double* w0 = a.W + (size_t)sg.aux_row * a.kp;
      const double* w1 = a.W + (size_t)aux1 * a.kp;
      bool member[NC];
      double so[NC], a0[NC], a1[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int s = 16 * c + col;
        const double acc2 = ((part[s] + part[S + s]) + part[2 * S + s]) + part[3 * S + s];
        member[c] = live[c] && asg[s] == cur;
        const double coef = coefs[s], kap = kaps[s];
        a1[c] = 0.0;
        if (!soc) {
          const double rad = sqrt(fmax(acc2, 0.0));
          so[c] = rad > 0.0 ? coef / rad : 0.0;
          a0[c] = coef;
        } else {
          const double cr = crs[s], br = brs[s];
          const double bp = 2.0 * br - 2.0 * cr * sg.f0;
          const double den = 2.0 * sg.f1 * kap + bp;
          const double q = den != 0.0 ? coef / den : 0.0;
          so[c] = -2.0 * q;
          a0[c] = q * (2.0 * sg.f0 * kap + 2.0 * cr);
          a1[c] = -2.0 * q * kap;
        }
      }
      const double* cb = sym ? vb : tt + col * a.ts + 2 * grp;
      const int cs = sym ? a.ks : a.ts;
      const double* timg = a.Wt + sg.toff;
#pragma unroll 1
      for (int ob = wave; ob < nbo; ob += 4) {
        f64x4 acc[NC];
        block_product<NC>(timg + (size_t)(16 * ob + col) * sg.rp + 2 * grp, cb, cs, sg.rp >> 3, acc);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (member[c]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * ob + grp + 4 * i;
              if (j < a.n) {
                double x = fma(a0[c], w0[j], out[c][j]);
                if (soc) x = fma(a1[c], w1[j], x);
                out[c][j] = fma(so[c], acc[c][i], x);
              }
            }
          }
        }
      }
      __syncthreads();          // the T tile, the partials and the aux values are rewritten by the next segment
    }
    __syncthreads();            // the tile and the records are rewritten by the next round
  }
}

// the shape conditions of rayen_wide_fused_bwd.hip::shape_served, then the plan for a tile of `samples` samples
// (`plan` receives the pack's own plan -- its widest QUAD_FAC / SOC segment included -- whether a shape condition holds or
// not; where one fails it is marked not served)
bool shape_plan(const RayenPack* p, const int samples, WideFusedBwd64Plan* plan) {
  if (p == nullptr || p->wide == nullptr) return false;            // (no tables: the set has an LMI)
  int widest = 0;
  bool shape = true;
  for (const RayenSegment& g : p->segs) {
    if (g.nrows < 0 || g.row0 < 0 || g.row0 + g.nrows > p->n_rows) { shape = false; continue; }
    if (g.type == RAYEN_SEG_LIN) continue;
    if (g.type == RAYEN_SEG_QUAD_SYM) {
      if (g.nrows > p->n) shape = false;                           // (its coefficient tile is the v tile)
    } else if (g.type == RAYEN_SEG_QUAD_FAC || g.type == RAYEN_SEG_SOC) {
      widest = g.nrows > widest ? g.nrows : widest;
    } else {
      shape = false;
    }
    if (g.aux_row < 0 || g.aux_row + (g.type == RAYEN_SEG_SOC ? 1 : 0) >= p->n_rows) shape = false;
  }
  WideFusedBwd64Plan pl = wide_fused_bwd64_plan(p->n, p->k, p->out_identity, widest, samples);
  if (!shape) { pl.served = 0; pl.region_words = 0; }
  if (plan) *plan = pl;
  return pl.served != 0;
}

int count_nonlinear(const RayenPack* p) {
  int n = 0;
  for (const RayenSegment& g : p->segs) n += (g.type != RAYEN_SEG_LIN) ? 1 : 0;
  return n;
}

void image_free(WideFusedBwd64Image* img) {
  if (img == nullptr) return;
  if (img->W_own) (void)hipFree(img->W_own);
  if (img->Wt) (void)hipFree(img->Wt);
  if (img->Et) (void)hipFree(img->Et);
  if (img->segs) (void)hipFree(img->segs);
  delete img;
}

template <typename F>
void for_each_instance(F&& f) {
  f(wide_fused_bwd64_kernel<false, 16>); f(wide_fused_bwd64_kernel<true, 16>);
  f(wide_fused_bwd64_kernel<false, 32>); f(wide_fused_bwd64_kernel<true, 32>);
}

// (under wide_fused_mutex) `fwd`: the fp64 forward's image where the pack has built one
int image_build(const RayenPack* p, const WideFused64Image* fwd, WideFusedBwd64Image** out) {
  *out = nullptr;
  WideFusedBwd64Plan plan16;
  if (!shape_plan(p, 16, &plan16)) return RAYEN_E_UNSUPPORTED;       // (what fits 32 samples fits 16)
  WideFusedBwd64Image* img = new WideFusedBwd64Image();
  img->plan[0] = plan16;
  (void)shape_plan(p, 32, &img->plan[1]);
  img->n_seg = (int)p->segs.size();
  img->n_simd = device_simds(p->device, 1024);
  const int n = p->n, np = plan16.np;
  bool ok = true;
  if (fwd != nullptr) {
    img->W = fwd->W;
    img->rows_pad = fwd->plan[0].rows_pad;
  } else {
    const int rows_w_pad = wide_fused64_pad16(p->n_rows);
    const int rows_pad = rows_w_pad + (p->out_identity ? 0 : wide_fused64_pad16(p->k));
    ok = upload_to_device(wide_fused64_rows_image(p, rows_w_pad, rows_pad, plan16.kp), &img->W_own, &img->bytes);
    img->W = img->W_own;
    img->rows_pad = rows_pad;
  }
  std::vector<B64Seg> segs;
  std::vector<double> Wt;
  for (const RayenSegment& g : p->segs) {
    B64Seg s{g.type, g.row0, g.nrows, g.aux_row, 0, 0, 0, g.f0, g.f1};
    if (g.type != RAYEN_SEG_LIN) {
      s.rp = wide_fused_bwd_pad8(g.nrows);
      s.key = 1 + img->n_nl++;
      s.toff = (int64_t)Wt.size();
      Wt.resize(Wt.size() + (size_t)np * s.rp, 0.0);
      double* t = Wt.data() + s.toff;
      for (int r = 0; r < g.nrows; ++r)
        for (int j = 0; j < n; ++j) t[(size_t)j * s.rp + r] = p->W[(size_t)(g.row0 + r) * n + j];
    }
    segs.push_back(s);
  }
  if (segs.empty()) segs.push_back(B64Seg{});
  if (Wt.empty()) Wt.assign(8, 0.0);                   // (no allocation of zero bytes)
  ok = ok && upload_to_device(segs, &img->segs, &img->bytes) && upload_to_device(Wt, &img->Wt, &img->bytes);
  if (ok && !p->out_identity) {
    std::vector<double> Et((size_t)np * plan16.ke, 0.0);
    for (int i = 0; i < p->k; ++i)
      for (int j = 0; j < n; ++j) Et[(size_t)j * plan16.ke + i] = p->NA_E[(size_t)i * n + j];
    ok = upload_to_device(Et, &img->Et, &img->bytes);
  }
  if (!ok) { image_free(img); return RAYEN_E_ALLOC; }
  bool attr = true;
  for_each_instance([&](auto kern) {
    attr = attr && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kWideFusedBwd64Lds) == hipSuccess;
  });
  if (!attr) {
    image_free(img);
    return RAYEN_E_LAUNCH;
  }
  *out = img;
  return RAYEN_OK;
}

}  // namespace

bool wide_fused_bwd64_served(const RayenPack* p) { return shape_plan(p, 0, nullptr); }

bool wide_fused_bwd64_plan_of(const RayenPack* p, const int samples, WideFusedBwd64Plan* plan) {
  if (p == nullptr || p->wide == nullptr) return false;
  (void)shape_plan(p, samples, plan);
  return true;
}

int64_t wide_fused_bwd64_workspace_bytes(const RayenPack* p, int64_t B) {
  if (!shape_plan(p, 0, nullptr)) return 0;
  return wide_fused_bwd_workspace(count_nonlinear(p), B);
}

void wide_fused_bwd64_free(WideFusedBwd64Image* img) { image_free(img); }

int wide_fused_bwd64_backward(const RayenPack* p, const double* v, int64_t B, int64_t ldv, const double* kappa,
                              const int32_t* active, const double* grad_y, int64_t ldg, double* grad_v, int64_t ldgv,
                              void* workspace, int64_t workspace_bytes, int samples, hipStream_t stream) {
  const WideFusedBwd64Image* img = nullptr;
  {
    std::lock_guard<std::mutex> lock(wide_fused_mutex());
    if (p->wfb64_state == 0) {
      if (!shape_plan(p, 0, nullptr)) {
        p->wfb64_state = 2;
      } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
          return RAYEN_E_NOT_PREPARED;            // the images' uploads do not belong in a capture: ask once before it
        WideFusedBwd64Image* built = nullptr;
        const int rc = image_build(p, p->wf64_state == 1 ? p->wf64 : nullptr, &built);
        if (rc != RAYEN_OK) return rc;
        p->wfb64 = built;
        p->wfb64_state = 1;
      }
    }
    if (p->wfb64_state != 1) return RAYEN_E_UNSUPPORTED;
    img = p->wfb64;
  }
  // the tile: the caller's, or 32 samples where the plan serves them
  const int h = samples == 0 ? (img->plan[1].served ? 1 : 0) : (samples == 32 ? 1 : 0);
  const WideFusedBwd64Plan& pl = img->plan[h];
  if (!pl.served) return RAYEN_E_UNSUPPORTED;      // (a forced 32 beyond its LDS)
  if (B == 0) return RAYEN_OK;
  // the permutation, where the caller brought room for it (rayen_wide_fused_bwd_group.h)
  const int32_t* perm = nullptr;
  if (!bwd_group<double, B64Seg>(img->segs, img->n_seg, img->n_nl, img->n_simd, kappa, active, B, workspace, workspace_bytes,
                                 stream, &perm))
    return RAYEN_E_LAUNCH;
  BArgs a;
  a.W = img->W; a.Wt = img->Wt; a.Et = img->Et; a.segs = img->segs;
  a.n_seg = img->n_seg; a.n = p->n; a.k = p->k; a.kp = pl.kp; a.ks = pl.ks; a.ke = pl.ke; a.gs = pl.gs; a.ts = pl.ts;
  a.np = pl.np; a.rows_pad = img->rows_pad; a.region_words = pl.region_words;
  a.v = v; a.B = B; a.ldv = ldv; a.kappa = kappa; a.active = active; a.gy = grad_y; a.ldg = ldg; a.gv = grad_v; a.ldgv = ldgv;
  a.perm = perm;
  // workgroups a CU holds: LDS, and what the registers allow
  int64_t per_cu = (160 * 1024) / pl.lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > per_cu_max(pl.samples) ? per_cu_max(pl.samples) : per_cu);
  const int64_t slots = (int64_t)(launch_simds(img->n_simd) / 4) * per_cu;
  const unsigned grid = (unsigned)persistent_grid(B, pl.samples, slots, 1);
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), (size_t)pl.lds_bytes, stream, a); };
  const bool ident = p->out_identity != 0;
  if (h == 0) { if (ident) launch(wide_fused_bwd64_kernel<true, 16>); else launch(wide_fused_bwd64_kernel<false, 16>); }
  else { if (ident) launch(wide_fused_bwd64_kernel<true, 32>); else launch(wide_fused_bwd64_kernel<false, 32>); }
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace rayen
