// The device image every schedule of the f16-pair forward reads (rayen_mfma_pair.hip, rayen_mfma_pair_io.hip,
// rayen_mfma_pair_ws8.hip, rayen_mfma_pair_wl.hip), its host functions and the choice of the schedule that serves a call
// (rayen_pair_image.hip).  Host code only: no kernel, no vector type.
#pragma once

#include <atomic>

#include "rayen_tiles.h"

namespace rayen {

// Side table of the W-in-LDS schedule (rayen_mfma_pair_wl.hip, round 7), one record per item and a blank one behind the last:
// where an item is the FIRST of a quadratic / cone segment that owns its tiles, what the walk needs to decide in front of it
// whether the whole segment can be skipped for a 32-sample group -- see "Screening" in rayen_mfma_pair_wl.hip.  MItem is not
// touched: three inline-asm kernels read it.
struct WlScreen {
  float cnst;        // 0: no spectral test here (nothing to decide when cabs is 0 too) | an upper bound of lambda_max(R'R) of
                     // the segment's rows AS LAID OUT, in the walk's scaled domain ((gW f_s)^2 folded in), rounded up by 2^-10:
                     // sum of squares <= cnst ||sv v||^2
  int32_t span;      // items the segment spans | 1 << 16: the closer is the cone's (else the quadratic's)
  int32_t aux;       // the closer's fields, as in the segment's MItem
  int32_t seg;       // caller's segment index: the counter's slot (below 64)
  float f0, f1, seg_inv;
  int32_t ts_after;  // tile | shape of the item behind the segment (what the walk fetches when it skips), -1: the list ends
  // round 8 (appended): 0: no probe | the probe constant (rayen_tiles.h::pair_probe_constant, rounded up): the sum of squares the
  // walk would reach is at most (sqrt(sum of squares of the leading products) + sqrt(cabs ||sv v||^2))^2
  float cabs;
  int32_t reserved[3];
};

// two f16 pieces of every entry of gW W (gW a power of two), in the fragment order of v_mfma_f32_32x32x16_f16
struct PairImage {
  void* Wh = nullptr;      // [n_tiles][NS][2][64] x 8 f16
  MItem* items = nullptr;
  MPack* packs = nullptr;
  float* y0 = nullptr;
  int n_items = 0;
  int nkk = 0;
  int identity = 0;
  int n_simd = 1024;
  float w_scale = 1.f, w_inv = 1.f;
  int aux_rows = 0;        // aux rows (phi | c, M'beta) of the whole set
  int first_out = 0;       // index of the first NA_E tile in the item list (n_items when NA_E = I)
  bool has_halves = false; // some items read half of a shared tile (rayen_tiles.h): not for the mapped instances
  int n_tiles = 0;         // tiles of the image (rayen_mfma_pair_wl.hip copies all of them into LDS)
  bool wl_ready = false;          // the W-in-LDS kernels were promised their dynamic LDS at pack creation
  bool wl_mapped_ready = false;   // ... and their mapped instances (room for the widest mapper next to the image)
  int64_t bytes = 0;
  std::vector<MItem> host_items;   // the item list as uploaded (rayen_mfma_pair_ws8.hip deals it out to eight waves)
  WlScreen* wl_screen = nullptr;   // [n_items + 1] on the device; null: no segment of this image can be screened
  std::vector<WlScreen> host_screen;
  // round 8: the W-in-LDS schedule's OWN item list -- the shared one with its quadratic / cone segments in the order of how often
  // each sets kappa (pair_wl_reorder; wl_screen / host_screen then follow this order).  null: the shared list.
  MItem* wl_items = nullptr;
  std::vector<MItem> wl_host_items;
};

// the side table of an item list whose tiles are b.raw (boosts applied), for the image scale gW = w_scale: empty when no
// segment qualifies (the constant is spectral_bound_rows of rayen_tiles.h: tests/test_pair_screen_bound.py)
std::vector<WlScreen> pair_screen_table(const TileLayout& b, double w_scale);

// `items` / `screen` (record i belongs to item i, a blank one behind the last) with the quadratic / cone segments of every run of
// adjacent segments sorted by `hits[segment]` descending -- ties, and with them the segments that never hit, keep their order --
// each segment's items adjacent as before, tiles and shapes untouched, the next-tile links (MItem::qbegin) and ts_after
// rebuilt.  false (nothing changed): no run of two segments, a list that is not FIRST .. LAST shaped, or the order stays.
bool pair_wl_reorder(std::vector<MItem>& items, std::vector<WlScreen>& screen, const std::vector<uint64_t>& hits);

// screening of the W-in-LDS schedule: 1 on (default: the spectral test and the probe), 2 the spectral test only (round 7), 0 off
// (RAYEN_PAIR_SCREEN at start-up, rayen_pair_screen afterwards)
std::atomic<int>& pair_screen_cell();
// the armed counter buffer (64 x uint32 on the device, slot = segment index) or null
std::atomic<unsigned*>& pair_screen_counters_cell();

// progress-ordered issue priority in the W-in-LDS schedule (round 9, "Drain" in rayen_mfma_pair_wl.hip): 0 off, 1 on
// (RAYEN_PAIR_DRAIN at start-up, rayen_pair_drain afterwards)
std::atomic<int>& pair_drain_cell();

// eligibility is mfma_split_eligible's
int mfma_pair_build(const RayenPack* p, PairImage** out, int64_t* bytes);
int mfma_pair_build_dense(const RayenPack* p, PairImage** out, int64_t* bytes);   // without shared tiles (fused mapper)
bool mfma_pair_has_halves(const PairImage* img);
void mfma_pair_free(PairImage* img);

// the schedule in force (RAYEN_PAIR_IO at start-up, rayen_pair_schedule afterwards); modes: rayen_pair_image.hip
std::atomic<int>& pair_schedule_cell();
int pair_schedule();

// One forward call on a pack the f16-pair kernels serve (p->pr32_state == 1), by the schedule in force.  *served: the
// RAYEN_KERNEL_* family that took it (the mapped twin leaves it alone where the plain kernel serves the call).
int mfma_pair_family_forward(const RayenPack* p, const float* v, int64_t B, int64_t ldv, float* y, int64_t ldy, float* kappa,
                             int32_t* active, int32_t* nan_flag, hipStream_t stream, int* served);
int mfma_pair_family_forward_mapped(const RayenPack* p, const float* x, int64_t B, int64_t ldx, int in_dim, const void* image,
                                    float* v_out, int64_t ldvo, float* y, int64_t ldy, float* kappa, int32_t* active,
                                    int32_t* nan_flag, hipStream_t stream, int* served);

}  // namespace rayen
