// The image of the f16-pair forward and the choice of the schedule that serves a call: host code only, no kernel.
//
// ONE image (two f16 pieces of every entry of gW W in MFMA fragment order, the item list, the packs, y0) is read by four
// schedules of the same arithmetic, which agree bit for bit: rayen_mfma_pair.hip (plain), rayen_mfma_pair_io.hip (rows
// trickled through LDS), rayen_mfma_pair_ws8.hip (W stationary), rayen_mfma_pair_wl.hip (W in LDS).  The arithmetic and the
// scaling are described at the top of rayen_mfma_pair.hip.
#include "rayen_pair_image.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rayen {

void mfma_pair_free(PairImage* img) {
  if (img == nullptr) return;
  if (img->Wh) (void)hipFree(img->Wh);
  if (img->items) (void)hipFree(img->items);
  if (img->packs) (void)hipFree(img->packs);
  if (img->y0) (void)hipFree(img->y0);
  if (img->wl_screen) (void)hipFree(img->wl_screen);
  if (img->wl_items) (void)hipFree(img->wl_items);
  delete img;
}

// Screening constants (rayen_mfma_pair_wl.hip, "Screening").  A segment qualifies when its items are contiguous from MF_FIRST
// to MF_LAST, own their tiles (MI_QFAC / MI_SOC; a cone only with a' < 0: its closer is monotone in the sum of squares then),
// its index fits the counter and its rows are finite.  The rows are the tile's as the MFMAs see them: a half of a shared tile
// contributes its own 32 columns only.
std::vector<WlScreen> pair_screen_table(const TileLayout& b, const double w_scale) {
  const int n_items = (int)b.items.size(), np = b.n_pad;
  std::vector<WlScreen> tab((size_t)n_items + 1);
  std::memset(tab.data(), 0, tab.size() * sizeof(WlScreen));
  for (WlScreen& s : tab) s.ts_after = -1;
  bool any = false;
  for (int i = 0; i < n_items; ++i) {
    const MItem& first = b.items[i];
    if ((first.type != MI_QFAC && first.type != MI_SOC) || !(first.flags & MF_FIRST)) continue;
    int j = i;
    while (!(b.items[j].flags & MF_LAST) && j + 1 < n_items && b.items[j + 1].type == first.type && b.items[j + 1].seg == first.seg &&
           !(b.items[j + 1].flags & MF_FIRST))
      ++j;
    if (!(b.items[j].flags & MF_LAST)) continue;
    if (first.seg < 0 || first.seg >= 64 || first.aux < 0 || !(first.seg_inv > 0.f)) continue;
    if (first.type == MI_SOC && !(first.f1 < 0.f && std::isfinite(first.f0) && std::isfinite(first.f1))) continue;
    std::vector<std::vector<double>> own;
    bool finite = true;
    for (int it = i; it <= j; ++it) {
      const MItem& m = b.items[it];
      const int c0 = m.shape() == MS_HALF_B ? 32 : 0, c1 = m.shape() == MS_HALF_A ? 32 : np;
      for (int r = 0; r < 32; ++r) {
        std::vector<double> row(np, 0.0);
        for (int c = c0; c < c1; ++c) {
          row[c] = b.raw[((size_t)m.tile() * 32 + r) * np + c];
          finite = finite && std::isfinite(row[c]);
        }
        own.push_back(std::move(row));
      }
    }
    if (!finite) continue;
    std::vector<const double*> rows;
    for (const auto& r : own) rows.push_back(r.data());
    const double lam = spectral_bound_rows(rows, np) * w_scale * w_scale * (1.0 + std::ldexp(1.0, -10));
    float c = (float)lam;
    if ((double)c < lam) c = std::nextafter(c, INFINITY);
    if (!(c > 0.f) || !std::isfinite(c)) continue;
    WlScreen& s = tab[i];
    s.cnst = c;
    s.span = (j - i + 1) | (first.type == MI_SOC ? 1 << 16 : 0);
    s.aux = first.aux;
    s.seg = first.seg;
    s.f0 = first.f0;
    s.f1 = first.f1;
    s.seg_inv = first.seg_inv;
    s.ts_after = j + 1 < n_items ? b.items[j + 1].tile_shape : -1;
    // the probe constant (round 8, "Probe" in rayen_mfma_pair_wl.hip): the same rows, entrywise absolute
    const double ca = pair_probe_constant(rows, np, w_scale);
    float cf = (float)ca;
    if ((double)cf < ca) cf = std::nextafter(cf, INFINITY);
    s.cabs = (cf > 0.f && std::isfinite(cf)) ? cf : 0.f;
    any = true;
    i = j;
  }
  if (!any) tab.clear();
  return tab;
}

bool pair_wl_reorder(std::vector<MItem>& items, std::vector<WlScreen>& screen, const std::vector<uint64_t>& hits) {
  const int n_items = (int)items.size();
  if ((int)screen.size() != n_items + 1) return false;
  struct Block { int first, count; uint64_t hits; };
  // blocks of the list: a whole segment (FIRST .. LAST, one type, one index) or a single item of anything else
  std::vector<Block> blocks;
  std::vector<char> is_seg;
  for (int i = 0; i < n_items;) {
    const MItem& f = items[i];
    int j = i;
    bool seg = (f.type == MI_QFAC || f.type == MI_SOC) && (f.flags & MF_FIRST);
    if (seg) {
      while (!(items[j].flags & MF_LAST) && j + 1 < n_items && items[j + 1].type == f.type && items[j + 1].seg == f.seg &&
             !(items[j + 1].flags & MF_FIRST))
        ++j;
      if (!(items[j].flags & MF_LAST)) return false;
    } else if (f.type == MI_QFAC || f.type == MI_SOC) {
      return false;
    }
    const uint64_t h = seg && f.seg >= 0 && (size_t)f.seg < hits.size() ? hits[f.seg] : 0;
    blocks.push_back({i, j - i + 1, h});
    is_seg.push_back(seg ? 1 : 0);
    i = j + 1;
  }
  bool moved = false;
  std::vector<Block> order = blocks;
  for (size_t a = 0; a < order.size();) {
    size_t e = a;
    while (e < order.size() && is_seg[e]) ++e;
    if (e > a + 1) {
      std::stable_sort(order.begin() + a, order.begin() + e, [](const Block& x, const Block& y) { return x.hits > y.hits; });
      for (size_t k = a; k < e; ++k) moved = moved || order[k].first != blocks[k].first;
    }
    a = e > a ? e : a + 1;
  }
  if (!moved) return false;
  std::vector<MItem> out_items;
  std::vector<WlScreen> out_screen;
  for (const Block& bl : order)
    for (int k = 0; k < bl.count; ++k) {
      out_items.push_back(items[bl.first + k]);
      out_screen.push_back(screen[bl.first + k]);
    }
  out_screen.push_back(screen[n_items]);
  for (int i = 0; i < n_items; ++i) out_items[i].qbegin = out_items[i + 1 < n_items ? i + 1 : i].tile_shape;
  for (int i = 0; i < n_items; ++i) {
    WlScreen& s = out_screen[i];
    if (!(s.cnst > 0.f) && !(s.cabs > 0.f)) continue;
    const int behind = i + (s.span & 0xFFFF);
    s.ts_after = behind < n_items ? out_items[behind].tile_shape : -1;
  }
  items.swap(out_items);
  screen.swap(out_screen);
  return true;
}

std::atomic<int>& pair_screen_cell() {
  static std::atomic<int> mode([] {
    const char* e = std::getenv("RAYEN_PAIR_SCREEN");
    return (e != nullptr && e[0] == '0') ? 0 : ((e != nullptr && e[0] == '2') ? 2 : 1);
  }());
  return mode;
}
std::atomic<unsigned*>& pair_screen_counters_cell() {
  static std::atomic<unsigned*> buf(nullptr);
  return buf;
}

std::atomic<int>& pair_drain_cell() {
  static std::atomic<int> mode([] {
    const char* e = std::getenv("RAYEN_PAIR_DRAIN");
    return (e != nullptr && e[0] == '1') ? 1 : 0;
  }());
  return mode;
}
}  // namespace rayen
extern "C" int rayen_pair_drain(int mode) {
  if (mode == 0 || mode == 1) return rayen::pair_drain_cell().exchange(mode, std::memory_order_relaxed);
  return rayen::pair_drain_cell().load(std::memory_order_relaxed);
}
namespace rayen {

static int pair_build(const RayenPack* p, PairImage** out, int64_t* bytes, bool tri);
int mfma_pair_build(const RayenPack* p, PairImage** out, int64_t* bytes) {
  // (RAYEN_PAIR_TRI=0: dense factors, two tiles each -- the image of rounds 3 and 4, for A/B measurements)
  const char* tri_env = std::getenv("RAYEN_PAIR_TRI");
  return pair_build(p, out, bytes, !(tri_env != nullptr && tri_env[0] == '0'));
}
bool mfma_pair_has_halves(const PairImage* img) { return img != nullptr && img->has_halves; }
// the image of the instances behind the fused mapper: every item a full tile
int mfma_pair_build_dense(const RayenPack* p, PairImage** out, int64_t* bytes) { return pair_build(p, out, bytes, false); }

static int pair_build(const RayenPack* p, PairImage** out, int64_t* bytes, const bool tri) {
  TileLayout b(p->n);
  const int rc = layout_tiles(p, b, /*allow_pack=*/true, /*allow_sym=*/false, tri);
  if (rc != RAYEN_OK) return rc;
  if (b.packs.empty()) { MPack none; std::memset(&none, 0, sizeof(none)); b.packs.push_back(none); }
  // an item also carries the NEXT item's tile and shape (in `qbegin`, which only symmetric-form layouts use): the walks
  // need them in front of an item's burst, and a scalar load issued there would be waited for there
  for (size_t i = 0; i < b.items.size(); ++i) b.items[i].qbegin = b.items[i + 1 < b.items.size() ? i + 1 : i].tile_shape;
  // ---- one power of two per quadratic / cone on top of the image's gW (round 3).  f16 has five exponent bits: with ONE
  // scale for the whole image, a constraint whose rows are 2^-15 of the image's largest entry keeps only its leading
  // pieces (config 5's jerk limits next to its corridor rows: 3e-5 -- the creation-time measurement sent the set to the
  // bf16 triples).  A candidate phi.v + ||U v|| is homogeneous in ITS OWN rows (aux rows and factor rows together), so
  // every such segment's rows are boosted by f_s = 2^e_s into the band the image's largest entry sits in, and its
  // candidate is multiplied by 1 / f_s (exact) before it meets the running maximum (MItem::seg_inv, MPack::inv).
  // Linear rows keep the image's scale (their maximum runs over rows of different segments' worth of scale).
  std::vector<float> seg_inv(p->segs.size(), 1.f);
  {
    // who owns an entry of the image: [tile row][column half] (a shared tile's rows belong to one segment in columns
    // 0..31 and to another in columns 32..63, rayen_tiles.h)
    const int n_tiles0 = b.n_tiles();
    const int half_w = b.n_pad >= 64 ? 32 : b.n_pad;
    std::vector<int> cell_seg((size_t)n_tiles0 * 32 * 2, -1);
    auto own_row = [&](int tile, int r, int shape, int seg) {
      if (shape != MS_HALF_B) cell_seg[((size_t)tile * 32 + r) * 2 + 0] = seg;
      if (shape != MS_HALF_A) cell_seg[((size_t)tile * 32 + r) * 2 + 1] = seg;
    };
    int cur_aux = -1;
    for (size_t idx = 0; idx < b.items.size(); ++idx) {
      const MItem& it = b.items[idx];
      if (it.type == MI_AUX) cur_aux = it.tile();
      if (it.type == MI_QFAC || it.type == MI_SOC) {
        for (int r = 0; r < 32; ++r) own_row(it.tile(), r, it.shape(), it.seg);
        if (cur_aux >= 0) {
          own_row(cur_aux, it.aux, MS_FULL, it.seg);
          if (it.type == MI_SOC) own_row(cur_aux, it.aux + 1, MS_FULL, it.seg);
        }
      }
      if (it.type == MI_PACK) {
        const MPack& pk = b.packs[it.aux];
        for (int a = 0; a < 4; ++a)
          for (int h = 0; h < 2; ++h) {
            if (pk.seg[a][h] < 0) continue;
            for (int c = 0; c < 4; ++c) own_row(it.tile(), 8 * a + 4 * h + c, MS_FULL, pk.seg[a][h]);
            if (cur_aux >= 0) own_row(cur_aux, pk.aux[a][h], MS_FULL, pk.seg[a][h]);
          }
      }
    }
    auto cell_of = [&](size_t r, int c) { return cell_seg[r * 2 + (c >= half_w ? 1 : 0)]; };
    double image_big = 0.0;
    std::vector<double> seg_big(p->segs.size(), 0.0);
    for (size_t r = 0; r < (size_t)n_tiles0 * 32; ++r)
      for (int c = 0; c < b.n_pad; ++c) {
        const double x = std::fabs(b.raw[r * b.n_pad + c]);
        if (!std::isfinite(x)) continue;
        image_big = x > image_big ? x : image_big;
        const int sg = cell_of(r, c);
        if (sg >= 0 && x > seg_big[sg]) seg_big[sg] = x;
      }
    std::vector<double> boost(p->segs.size(), 1.0);
    for (size_t s = 0; s < p->segs.size(); ++s) {
      if (!(seg_big[s] > 0.0) || !(image_big > 0.0)) continue;
      int ex_seg = 0, ex_img = 0;
      (void)std::frexp(seg_big[s], &ex_seg);
      (void)std::frexp(image_big, &ex_img);
      int e = ex_img - ex_seg;                    // the segment's largest entry into the binade of the image's
      e = e < 0 ? 0 : (e > 60 ? 60 : e);
      boost[s] = std::ldexp(1.0, e);
      seg_inv[s] = (float)std::ldexp(1.0, -e);
    }
    for (size_t r = 0; r < (size_t)n_tiles0 * 32; ++r)
      for (int c = 0; c < b.n_pad; ++c) {
        const int sg = cell_of(r, c);
        if (sg >= 0 && boost[sg] != 1.0) b.raw[r * b.n_pad + c] *= boost[sg];
      }
    for (MItem& it : b.items)
      if (it.type == MI_QFAC || it.type == MI_SOC) it.seg_inv = seg_inv[it.seg];
    for (MPack& pk : b.packs)
      for (int a = 0; a < 4; ++a)
        for (int h = 0; h < 2; ++h) pk.inv[a][h] = pk.seg[a][h] >= 0 ? seg_inv[pk.seg[a][h]] : 1.f;
  }
  const std::vector<float> frag = b.fragments_f32();

  PairImage* img = new PairImage();
  img->nkk = b.n_pad / 32;
  img->identity = p->out_identity;
  img->n_items = (int)b.items.size();
  img->host_items = b.items;
  for (const MItem& it : b.items) img->has_halves = img->has_halves || it.shape() != MS_FULL;
  for (const RayenSegment& g : p->segs) img->aux_rows += aux_rows_of(g);
  img->first_out = img->n_items;
  for (int i = img->n_items - 1; i >= 0; --i)
    if (b.items[i].type == MI_OUT) img->first_out = i;
  img->n_simd = device_simds(p->device, img->n_simd);
  // gW: the largest entry of the image into [2^13, 2^14)
  float big = 0.f;
  for (const float x : frag)
    if (std::isfinite(x)) big = std::fmax(big, std::fabs(x));
  int ex = 0;
  if (big > 0.f) (void)std::frexp(big, &ex);   // big = f 2^ex, f in [0.5, 1)
  int shift = big > 0.f ? 14 - ex : 0;
  shift = shift > 100 ? 100 : (shift < -100 ? -100 : shift);   // (beyond: f16 overflow -> the self-check rejects the pack)
  img->w_scale = std::ldexp(1.0f, shift);
  img->w_inv = std::ldexp(1.0f, -shift);
  // two f16 pieces of every scaled entry, in the fragment order of v_mfma_f32_32x32x16_f16 (the bf16 instruction's):
  // chunk (tile, k-step s, piece) = 64 lanes x 8 elements, element i of lane l = column
  // 16 s + 8 (i >> 2) + 4 (l >> 5) + (i & 3) of row l & 31 = entry [2 s + (i >> 2)][l][i & 3] of the fp32 image
  const int n_tiles = b.n_tiles(), ns = b.nq() / 2;
  img->n_tiles = n_tiles;
  std::vector<_Float16> wh((size_t)n_tiles * ns * 2 * 64 * 8);
  for (int t = 0; t < n_tiles; ++t)
    for (int sp = 0; sp < ns; ++sp)
      for (int l = 0; l < 64; ++l)
        for (int i = 0; i < 8; ++i) {
          const float x = frag[(((size_t)t * b.nq() + 2 * sp + (i >> 2)) * 64 + l) * 4 + (i & 3)] * img->w_scale;
          const _Float16 h1 = (_Float16)x;                    // round to nearest even
          const _Float16 h2 = (_Float16)(x - (float)h1);      // (exact difference)
          const size_t base = (((size_t)t * ns + sp) * 2) * 64 * 8 + (size_t)l * 8 + i;
          wh[base] = h1;
          wh[base + 64 * 8] = h2;
        }
  if (!upload_walk_image(p, b, wh, &img->Wh, &img->y0, &img->items, &img->packs, &img->bytes)) {
    mfma_pair_free(img);
    return RAYEN_E_ALLOC;
  }
  img->host_screen = pair_screen_table(b, (double)img->w_scale);
  if (!img->host_screen.empty() && !upload_to_device(img->host_screen, &img->wl_screen, &img->bytes)) {
    mfma_pair_free(img);
    return RAYEN_E_ALLOC;
  }
  *bytes = img->bytes;
  *out = img;
  return RAYEN_OK;
}

// Schedules of the f16-pair forward (same arithmetic): 3 (default, round 6) = the image of W resident in LDS
// (rayen_mfma_pair_wl.hip) where the pack and the call allow it, else as 1 | 1 (the default of rounds 3-5) = rows of v and y
// trickled through LDS under the tile walk (rayen_mfma_pair_io.hip) where the call's shape allows it, the W-stationary
// kernel for mid-size batches | 0 = rayen_mfma_pair.hip always | 2 = W-stationary (rayen_mfma_pair_ws8.hip) where the pack
// and the call allow it, else as 1.  All bit-identical.  RAYEN_PAIR_IO / rayen_pair_schedule select (A/B runs).
std::atomic<int>& pair_schedule_cell() {
  static std::atomic<int> mode([] {
    const char* e = std::getenv("RAYEN_PAIR_IO");
    return (e != nullptr && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : 3;
  }());
  return mode;
}
int pair_schedule() { return pair_schedule_cell().load(std::memory_order_relaxed); }

int mfma_pair_family_forward(const RayenPack* p, const float* v, int64_t B, int64_t ldv, float* y, int64_t ldy, float* kappa,
                             int32_t* active, int32_t* nan_flag, hipStream_t stream, int* served) {
  const PairImage* img = p->pr32;
  const int mode = pair_schedule();
  const auto ws8_serves = [&] { return mfma_pair_ws8_serves(p, img, p->ws8_32, v, B, ldv, y, ldy); };
  const auto ws8_forward = [&] {
    *served = RAYEN_KERNEL_PAIR_WS;
    return mfma_pair_ws8_forward(p, img, p->ws8_32, v, B, ldv, y, ldy, kappa, active, nan_flag, stream);
  };
  if (mode == 3 && mfma_pair_wl_serves(p, img, v, B, ldv, y, ldy)) {
    *served = RAYEN_KERNEL_PAIR_WL;
    return mfma_pair_wl_forward(p, img, v, B, ldv, y, ldy, kappa, active, nan_flag, stream);
  }
  if (mode == 2 && ws8_serves()) return ws8_forward();
  if (mode >= 1 && mfma_pair_io_serves(p, img, v, B, ldv, y, ldy)) {
    *served = RAYEN_KERNEL_PAIR_IO;
    return mfma_pair_io_forward(p, img, v, B, ldv, y, ldy, kappa, active, nan_flag, stream);
  }
  // Batches between two groups per CU and one group per resident wave (32 768 <= B < 131 072 on this chip): too small
  // for the trickled rows to have interior rounds, and the plain kernel leaves SIMDs with one wave or none -- there the
  // W-stationary kernel is the fastest of the three bit-identical schedules (12.7 against 18.2 us at B = 32 768,
  // 20.5 / 22.6 at 65 536, 27.2 / 28.4 at 98 304: profiles/bench/r04_midbatch_schedules.txt).
  if (mode == 1 && ws8_serves()) return ws8_forward();
  *served = RAYEN_KERNEL_PAIR;
  return mfma_pair_forward(p, img, v, B, ldv, y, ldy, kappa, active, nan_flag, stream);
}

// the instances behind the module's mapper v = Wm x + b (rayen_ray_project_mapped_image_f32)
int mfma_pair_family_forward_mapped(const RayenPack* p, const float* x, int64_t B, int64_t ldx, int in_dim, const void* image,
                                    float* v_out, int64_t ldvo, float* y, int64_t ldy, float* kappa, int32_t* active,
                                    int32_t* nan_flag, hipStream_t stream, int* served) {
  // (round 6: the W-in-LDS schedule with the mapper's image next to W's -- on the pack's own image, shared tiles included)
  if (pair_schedule() == 3 && mfma_pair_wl_serves_mapped(p, p->pr32, x, B, ldx, in_dim, v_out, ldvo, y, ldy)) {
    *served = RAYEN_KERNEL_PAIR_WL;
    return mfma_pair_wl_forward_mapped(p, p->pr32, x, B, ldx, in_dim, image, v_out, ldvo, y, ldy, kappa, active, nan_flag, stream);
  }
  return mfma_pair_forward_mapped(p, p->pr32m != nullptr ? p->pr32m : p->pr32, x, B, ldx, in_dim, image, v_out, ldvo, y, ldy,
                                  kappa, active, nan_flag, stream);
}

}  // namespace rayen
