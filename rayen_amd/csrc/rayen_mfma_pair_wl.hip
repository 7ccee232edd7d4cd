// Paired-half forward with the IMAGE OF W RESIDENT IN LDS (round 6; rayen/constraint_module.py:468-474, 351-458 in one
// launch; the arithmetic is rayen_mfma_pair.hip's, bit for bit).
//
// Why: in rayen_mfma_pair.hip / rayen_mfma_pair_io.hip every wave pulls the whole image through the CU's vector-memory
// path once per 64 samples -- eight 1-KiB global_load_dwordx4 per tile and wave, sixteen cycles of that path each
// (scripts/ubench/mfma_coissue.hip: 64 B per clock and CU), ten with the two row operations: eight waves keep it busy
// 1 280 of the ~2 400 cycles a tile takes, and a wave that cannot hand over its re-load cannot issue its next MFMA either
// (HISTORY.md, "the same ablations on config 3's walk": no A re-loads -18 %, neither re-loads nor row operations -29 %).
// Here the image is copied into LDS ONCE per workgroup (one workgroup per CU; config 3: 14 tiles = 112 KiB) and an A
// operand is a ds_read_b128: 4 LDS cycles instead of 16 vector-memory cycles, on a path nothing else uses.  What that
// buys besides:
//   * no row buffers in LDS (there is no room for them and no need): a lane reads ITS sample's row straight from memory as
//     eight 16-byte pieces (fragment shape: lanes (col, hi) of a row cover 32 contiguous bytes, four consecutive
//     instructions complete a 128-byte line) -- the wait is left to the other waves of the SIMD; requested at the top of the
//     group in rounds 6-9 and in the mapped instances; since round 10 (RAYEN_WL_HEAD bit 2) the first group's in the head --
//     two waves of the workgroup behind the image's chunks in front of the barrier, the others right behind it -- and every
//     further group's behind the last store of y of the group before --
//     through a buffer descriptor whose extent is the batch (one add per group; rows beyond the batch and pieces beyond
//     a ragged width are out of range: loads return 0, stores are dropped), and writes its row of y through 2 KiB of LDS
//     as whole lines;
//   * vmcnt counts nothing but those rows and the stores of y: one counted wait, in the head of the early waves (the image has
//     landed, the first rows are in flight), no stand-in operations;
//   * groups of 32 samples (one sample tile per wave): ~120 instead of 160+ live registers, so FOUR waves per SIMD
//     (sixteen per workgroup, dealt groups on demand from a counter in LDS) take turns on the matrix pipe -- by the same
//     microbenchmark a partner's plain VALU / SALU / LDS instructions issue while a wave's MFMAs execute; measured
//     monotone in the wave count (16: 46.4 us, 12: 49.5, 8: 54.7) -- and the first rows a wave waits for are 8 KiB, not 16;
//   * the image itself arrives by LDS-DMA (global_load_lds_dwordx4: nothing through the registers);
//   * every batch size (one workgroup per CU as soon as there is a group for it), n = k below the padded width, the
//     module's mapper in front (NKX > 0: its image next to W's).
// The item list, the image, the epilogues and the order of the products inside a tile are the other schedules': same bits.
//
// Screening (round 7; SCREEN instances, rayen_pair_screen): kappa is a maximum over segments, so a quadratic / cone whose
// candidate is below the running maximum for all 32 samples of a group changes neither kappa nor y nor the arg-max record,
// and its tiles (config 3: 18 MFMAs and 16 A-operand reads per cone) need not be multiplied.  In front of the first item of
// such a segment (side table WlScreen, rayen_pair_image.h: one record per item, loaded with the previous item's record) the
// wave forms   ub = closer(aux rows, cnst * ||sv v||^2)   with the segment's OWN closer and skips the segment's items iff
// ub < max(kap, other half's kap) on every live lane (dead lanes of a ragged group have no say; a NaN or an infinite row
// makes every comparison false and skips nothing).  The segments behind it are decided at the same point until one stays;
// then the A operands of the item that does run are fetched over the ones prefetched for the skipped item.
//   Why ub dominates the candidate the walk would have computed.  The accumulators of the segment's items are
// acc = (gW f_s R)(sv v) with R the rows as laid out, so their sum of squares is ||gW f_s R sv v||^2 <= lambda_max((gW f_s)^2
// R'R) ||sv v||^2 in exact arithmetic; cnst is that eigenvalue (fp64 Jacobi, certified by a Cholesky of c I - R'R:
// spectral_bound_rows) times 1 + 2^-10.  The margin pays for: the f16 pairs of W and of sv v (each 2^-22 of its row's
// largest entry, the dropped p2 p2 products 2^-22 again), the fp32 accumulation of 64 products per accumulator and of the 64
// squares (errors relative to ||R||_F ||v|| <= 8 sqrt(lambda_max) ||v||: below 2^-15 of the bound together), and the fp32
// sum ||sv v||^2 computed here (2^-19): three orders of magnitude inside 2^-10.  Both closers are monotone in the sum of
// squares operation by operation -- sqrt, products by positive constants and sums round monotonically; in
// pair_soc_candidate (a' < 0, checked at image creation) cp, disc and root grow with it and the root taken,
// (-bp - root) / 2a', grows with root and is the larger of the two -- and a candidate of 0 (negative discriminant, NaN)
// never beats the running maximum.  So ub >= the candidate, and a skipped candidate would have lost every comparison:
// same bits (tests/test_gpu_pair_wl_screen.py, and every bit-for-bit test of the four schedules).
//
// Probe (round 8; same instances, mode 1 of rayen_pair_screen): the spectral bound is lambda_max ||v||^2, and a quadratic's
// true sum of squares sits near a quarter of it (config 3), so that test fires only when the running maximum is twice the
// candidate -- for the cones, never for the quadratics.  A tight test is cheap: the walk rebuilds every fp32 product from three
// f16 products a2 b1, a1 b2, a1 b1, and the LEADING one alone gives the accumulator to 2^-10.  Where the spectral test leaves a
// segment standing and its record carries a probe constant (WlScreen::cabs), the wave reads only the leading pieces a1 of the
// segment's items from LDS, runs  p = sum_sp a1 vb[0][0][sp]  per item from zero (a third of the MFMAs; acc and part are dead
// between two segments), sums the squares across the items exactly as the epilogue does, and forms
//   ub_total = (sqrt(total_probe) + sqrt(cabs nv2))^2 (1 + 2^-12),   ub = closer(aux rows, ub_total)
// with the segment's OWN closer; the segment is skipped iff ub < max(kap, other half's kap) on every live lane, nv2 < inf, and
// the row is one the margin is proved for (below).  Skipped: the segments behind it are decided at the same point.  Not skipped:
// the segment is walked as always -- both pieces fetched, the products in their order, nothing of the probe reused.
//   Why ub_total dominates the sum of squares the walk would have computed.  Write a = the scaled fp32 entry of the image,
// a1 = f16(a), a2 = f16(a - a1), x = sv v, b1 = f16(x), b2 = f16(x - b1) (round to nearest: the image and pair_split_*).  In exact
// arithmetic the walk's accumulator is F_i = sum_k (a2 b1 + a1 b2 + a1 b1), the probe's P_i = sum_k a1 b1.  |a2| <= 2^-11 (1 +
// 2^-10) |a| + 2^-24 and |a1| <= (1 + 2^-11) |a| + 2^-25 (the absolute terms: pieces below 2^-14 are f16 subnormals), the same
// for b2, b1 against x, so  |F_i - P_i| <= 2^-10 (1 + 2^-9) sum_k |a_ik| |x_k| + 2^-23 (||a_i||_1 + ||x||_1) + 2^-42.  For a row
// whose largest scaled entry reached 2^13 -- pow2_scale puts it into [2^13, 2^14) unless max |v| < 2^-113, where the scale is
// clamped; the kernel tests nv2 >= 2^26 and takes the zero row, whose products all vanish, as well -- ||a_i||_1 <= 8 ||a_i||_2
// <= 2^-10 ||a_i||_2 ||x||, so the 2-norm over the segment's m rows is
//   ||F - P|| <= (2^-10 (1 + 2^-9 + 2^-20) || |R| ||_2 + 2^-20 sqrt(m)) ||x||,
// |R| the rows as laid out, entrywise absolute, in the scaled domain.  The fp32 accumulation of the 192 products of F and the
// 64 of P adds at most 2^-16 sum_k |a| |x| per row.  cabs = (2^-10 (1 + 2^-4) sqrt(lambda_max(|R|'|R|)) gW f_s + 2^-19 sqrt(m))^2,
// rounded up (rayen_tiles.h::pair_probe_constant: spectral_bound_rows of the absolute rows, Cholesky certificate included;
// tests/test_pair_probe_bound.py: no direction uses more than 0.13 of it), covers both with room.  The two sums of squares are
// fp32 sums of at most 64 non-negative terms per lane and a pair of adds (relative error 2^-18 each, either direction), nv2
// carries 2^-19, the two v_sqrt_f32 one ulp each, the product, the sum and the square a rounding each: below 2^-15 of ub_total
// together, paid by the factor 1 + 2^-12.  So ub_total >= the walk's fp32 total, the closers are monotone in it (above), and
// a skipped candidate would have lost every comparison: same bits (tests/test_gpu_pair_wl_probe.py).
//   Order (round 8): the probe pays only against a high running maximum, so this schedule walks its own copy of the item list
// in which the quadratics / cones of a run of adjacent segments come in the order of how often each sets kappa on the
// pack-creation directions (wl_screen_gate, pair_wl_reorder).  A candidate's bits do not depend on its place and kappa is a
// maximum; the other schedules keep the shared list, so their bit-for-bit tests against this one cover the permutation.
//
// Served: NA_E = I, n = k in (32 (NKK - 1), 32 NKK] and a multiple of 4, rows 16-byte aligned, the image + the aux patches within 160 KiB of LDS, at most
// sixteen aux rows at NKK = 2 (eight behind a mapper).  Everything else stays on the other schedules.
#include "rayen_split_image.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>

namespace rayen {

namespace {
#ifndef RAYEN_WL_WAVES
#define RAYEN_WL_WAVES 16
#endif
#ifndef RAYEN_WL_NT
#define RAYEN_WL_NT 1
#endif
// 1: a group's rows are requested one group ahead (64 registers at two sample tiles) | 0: at the top of the group, the wait
// left to the other waves of the SIMD
#ifndef RAYEN_WL_AHEAD
#define RAYEN_WL_AHEAD 0
#endif
constexpr int kWlWaves = RAYEN_WL_WAVES;      // waves per workgroup = per CU
constexpr int kWlNT = RAYEN_WL_NT;            // sample tiles (of 32) per wave and group
// developer ablation builds (scripts/ubench/tu_variant.sh rayen_mfma_pair_wl <name> -DRAYEN_WL_ABL=<bits>; WRONG RESULTS):
// 1 rows requested once per wave | 2 no rows of y stored | 8 plain stores | 16 no epilogues | 32 no MFMAs | 64 the walk stops four
// items early (config 3: both cones -- the ceiling of what screening them can give)
#ifndef RAYEN_WL_ABL
#define RAYEN_WL_ABL 0
#endif
// bit 0: the image is copied by LDS-DMA (0: through registers) | bit 1: a wave's first rows are pulled towards L2 meanwhile
// (config 3, B = 262 144, gpurun_out/r06zza: 0 -> 46.1-46.6 us, 1 -> 45.3-45.9, 2 -> 47.4-49.4: the extra requests cost more than the
// round trip they hide) | bit 2 (round 10; the instances without a mapper, RAYEN_WL_AHEAD = 0): the first rows of the workgroup's
// first RAYEN_WL_EARLY waves are REQUESTED behind the image's chunks and in front of the barrier -- into their registers, once; the
// wait in front of the barrier is for the image alone (vmcnt retires in order: the rows stay in flight) -- those of the other
// waves right behind the barrier, and a further group's rows at the bottom of the group in front of it, behind its last store of
// y.  -DRAYEN_WL_HEAD=1 (scripts/ubench/tu_variant.sh) rebuilds the head of rounds 6-9 for a same-box A/B.
#ifndef RAYEN_WL_HEAD
#define RAYEN_WL_HEAD 5
#endif
// (RAYEN_WL_HEAD bit 2) how many waves of a workgroup request their first rows in front of the barrier.  The image and the rows
// come through the same vector-memory path of the CU, so rows requested early do not arrive sooner in all, they only arrive
// before the barrier opens: with all sixteen early the four waves of a SIMD left the barrier into their splits together and
// the launch was SLOWER at every batch size (config 3, five interleaved runs each, against the head of rounds 6-9: B = 262 144
// 0.03927-0.03963 against 0.03875-0.03899 ms, 32 768 +1.5 %, 1 048 576 +0.5 %; entry to first MFMA 6.4-6.8 against 5.7-5.8 us).
// With two early those two multiply while the others' rows arrive and are split: 0.04000-0.04033 against 0.04021-0.04092
// (parent 0.04060-0.04088), 32 768 0.01318-0.01328 against 0.01333-0.01348; four: no gain at 262 144, a loss at 32 768 (all of
// its busy waves early); eight: the parent's time (profiles/bench/r10_wl_head_probe.txt).
#ifndef RAYEN_WL_EARLY
#define RAYEN_WL_EARLY 2
#endif
// 1: the running maximum over both halves is formed once per decision point (round 10) | 0: once per test, as in rounds 7-9
#ifndef RAYEN_WL_KMAX_ONCE
#define RAYEN_WL_KMAX_ONCE 1
#endif
// aux rows a wave keeps per sample tile: 32 at NKK = 1; at NKK = 2 sixteen (2 KiB: what the staging of y needs anyway), eight in the
// mapped instances (1 KiB: the mapper's image takes the room)
#ifndef RAYEN_WL_AUXR2
#define RAYEN_WL_AUXR2 16
#endif
template <int NKK, bool MAPPED = false> struct WlGeom { static constexpr int AUXR = NKK == 2 ? (MAPPED ? 8 : RAYEN_WL_AUXR2) : 32; };
// a wave's own LDS: the aux patch during the walk ([sample tile][aux row][sample]), then the 4 KiB through which its rows of
// y leave as whole 128-byte lines (32 rows x one line)
// (one sample tile per wave: 16 rows at a time through 2 KiB, so that three or four waves per SIMD fit next to the image)
#ifndef RAYEN_WL_SR
#define RAYEN_WL_SR 0
#endif
constexpr int wl_stage_rows(int nt) { return RAYEN_WL_SR ? RAYEN_WL_SR : (nt == 1 ? 16 : 32); }
constexpr int wl_region_bytes(int nkk, int nt) {
  return nt * (nkk == 2 ? WlGeom<2>::AUXR : WlGeom<1>::AUXR) * 128 > wl_stage_rows(nt) * 128 ? nt * (nkk == 2 ? WlGeom<2>::AUXR : WlGeom<1>::AUXR) * 128
                                                                                             : wl_stage_rows(nt) * 128;
}
// one LDS-DMA: every lane fetches 16 bytes from gbase + voff; lane L lands at LDS byte lds + 16 L.  Nothing returns through the
// vector registers -- by scripts/ubench/mfma_coissue.hip such loads run beside a partner wave's MFMAs, register loads do not.
// (M0 = the LDS base; written in the statement that reads it, restored behind it)
__device__ __forceinline__ void wl_dma16(const char* gbase, const unsigned voff, const unsigned lds) {
  unsigned keep;
  uint64_t asm_base;
  asm volatile(RAYEN_ASM_BASE_COPY "s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[lds]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[off], " RAYEN_ASM_BASE "\n\ts_mov_b32 m0, %[k]"
               : [k] "=&s"(keep), [b] "=&s"(asm_base)
               : [off] "v"(voff), [base] "s"(gbase), [lds] "s"(lds)
               : "memory");
}
// x + (the other half's x) and max(x, the other half's x) without LDS (round 9, the instances without a mapper): one
// v_permlane32_swap on two copies of x leaves [low half's x | low half's x] and [high half's x | high half's x]; their sum /
// maximum is the same value in both halves and, both operations being commutative, the bits of x + xhalf(x) / fmaxf(x, xhalf(x)).
// The ds_bpermute_b32 of xhalf forces an s_waitcnt lgkmcnt(0), which also drains the next item's A-operand reads and its record.
// developer builds: -DRAYEN_WL_SWAP=0 keeps xhalf
#ifndef RAYEN_WL_SWAP
#define RAYEN_WL_SWAP 1
#endif
template <bool SWAP> __device__ __forceinline__ float wl_half_sum(const float x) {
  if constexpr (SWAP && RAYEN_WL_SWAP) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
  } else {
    return x + xhalf(x);
  }
}
template <bool SWAP> __device__ __forceinline__ float wl_half_max(const float x) {
  if constexpr (SWAP && RAYEN_WL_SWAP) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
  } else {
    return fmaxf(x, xhalf(x));
  }
}
// (SCREEN instances) the NaN / Inf flag of a row from its ||sv v||^2, which the screening decisions need anyway: the scaled entries
// are below 2^14 and there are 64 squares, so a finite row cannot overflow, and an infinite or NaN component propagates through
// its product and the sums -- nan_row = !(nv2 < inf) replaces the sixteen pair_nan_fold of the split and the two compares
// (tests/test_pair_nv2_flag_host.py).  developer builds: -DRAYEN_WL_NANNV2=0 keeps pair_nan_fold
#ifndef RAYEN_WL_NANNV2
#define RAYEN_WL_NANNV2 1
#endif
// Drain (round 9; rayen_pair_drain, the instances without a mapper): the issue arbiter of a SIMD serves priority first, then age,
// so under equal priorities the four waves of a SIMD finish their last groups one after the other and the last one walks the
// tail alone, issuing for a third of its clocks.  With the switch on, a wave's priority follows its PROGRESS: 3 in its first
// group, one less with every further group it claims, and inside the last group it will walk one less again a third and two
// thirds of the way down the item list -- the wave that is behind outranks the wave that is ahead.  One s_setprio per step (the
// priority is an immediate: a uniform branch picks it); no wave ever waits for another.
//   Measured (profiles/bench/r09_wl_drain.txt; config 3): the waves of a SIMD do finish together -- 8.2 -> 4.5 us with three, two
// and one of them alive at B = 262 144 -- and the launch is 1.4 % SLOWER there (1.7 % at B = 32 768): held back together, all four
// reach their epilogues and stores at once, where the staggered finish overlaps one wave's closing vector work with the others'
// MFMAs.  Faster only at eight groups per wave (B = 1 048 576: -2.0 % in one session).  Off by default.
__device__ __forceinline__ void wl_set_level(const int level) {
  if (level <= 0) __builtin_amdgcn_s_setprio(3);
  else if (level == 1) __builtin_amdgcn_s_setprio(2);
  else if (level == 2) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
// the mapped instances carry the mapper's image (up to 16 KiB) next to W's: eight rows at a time through 1 KiB
constexpr int kWlStageRowsMapped = 8;
constexpr int wl_region_bytes_mapped(int nkk, int nt) {
  return nt * (nkk == 2 ? WlGeom<2, true>::AUXR : WlGeom<1, true>::AUXR) * 128 > kWlStageRowsMapped * 128
             ? nt * (nkk == 2 ? WlGeom<2, true>::AUXR : WlGeom<1, true>::AUXR) * 128
             : kWlStageRowsMapped * 128;
}
}  // namespace

// developer build (scripts/ubench/tu_variant.sh rayen_mfma_pair_wl clock -DRAYEN_WL_CLOCK; scripts/ubench/wl_clock.py): s_memtime
// (shader clocks) and s_memrealtime (100 MHz) at entry and exit of wave 0 of every 16th workgroup -- the shader clock the
// kernel actually ran at (the chip lowers it under matrix load).  Nothing in the library build.
// developer build (-DRAYEN_WL_STAMPS; scripts/ubench/wl_stamps.py): s_memtime per item of the SECOND group of waves 0 and 4 of
// workgroup 0 -- [item top | burst and the next item's reads issued | epilogue done].  Nothing in the library build.
#ifdef RAYEN_WL_STAMPS
#ifndef RAYEN_WL_STAMP_ROUND
#define RAYEN_WL_STAMP_ROUND 1
#endif
__device__ unsigned long long wl_stamp_buf[2 * 40 * 4];
extern "C" int rayen_debug_wl_stamps(void* dst, size_t bytes) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(wl_stamp_buf), bytes < sizeof(wl_stamp_buf) ? bytes : sizeof(wl_stamp_buf)) == hipSuccess ? 0 : -1;
}
#define RAYEN_WL_STAMP(item, slot)                                                                              \
  do {                                                                                                          \
    if (stamp_on && lane == 0 && (item) < 40) wl_stamp_buf[((wave >> 2) * 40 + (item)) * 4 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define RAYEN_WL_STAMP(item, slot) do { } while (0)
#endif
// Round 9: the probe covers all sixteen waves of every 16th workgroup -- [workgroup / 16][wave][entry | first MFMA | end of the
// first group | exit] x [s_memtime, s_memrealtime], then the wave's HW_ID (its SIMD) and the groups it walked
// (scripts/ubench/wl_drain.py: how long a SIMD runs with 4, 3, 2, 1 and 0 of its waves alive).
#ifdef RAYEN_WL_CLOCK
constexpr int kWlClockSlots = 10;
__device__ unsigned long long wl_clock_buf[16 * 16 * kWlClockSlots];
extern "C" int rayen_debug_wl_clock(void* dst, size_t bytes) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(wl_clock_buf), bytes < sizeof(wl_clock_buf) ? bytes : sizeof(wl_clock_buf)) == hipSuccess ? 0 : -1;
}
#define RAYEN_WL_CLOCK_AT(slot)                                               \
  do {                                                                        \
    if (probe) {                                                              \
      clock_at[2 * (slot) + 0] = __builtin_amdgcn_s_memtime();                \
      clock_at[2 * (slot) + 1] = __builtin_amdgcn_s_memrealtime();            \
    }                                                                         \
  } while (0)
#else
#define RAYEN_WL_CLOCK_AT(slot) do { } while (0)
#endif

// NKX > 0: the module's mapper v = Wm x + b in front of the walk (rayen/constraint_module.py:259-263, 525; the arithmetic of
// rayen_mfma_pair.hip's mapped instances, bit for bit): `v` / `ldv` / `n_in` are then x, its leading dimension and its width, the
// mapper's f16-pair image (NKK x 2 NKX K-steps x 2 pieces of 1 KiB, then bias, gM, 1 / gM: pair_mapper_image_kernel) is copied into
// LDS behind the image of W, and v reaches memory only when v_out != null (training).
// DRAIN: the instances rayen_pair_drain(1) selects ("Drain" above).  Instances of their own, not a kernel argument: with the
// switch as an argument the walk that does NOT use it ran 1 % slower (eleven more scalar registers spilled at the group's top, a
// compare and a branch per item; profiles/bench/r09_wl_drain.txt).
template <int NKK, bool TRACK, int NT, int NW, int NKX = 0, bool SCREEN = false, bool DRAIN = false>
__global__ __launch_bounds__(NW * 64, 1) void mfma_pair_wl_kernel(
    const f16x8* __restrict__ Wh, const MItem* __restrict__ items, int n_items,
    const MPack* __restrict__ packs, const float* __restrict__ y0, int n_tiles, int n,
    const float* __restrict__ v, int64_t B, int64_t ldv, float* __restrict__ y, int64_t ldy,
    float* __restrict__ kappa_out, int32_t* __restrict__ active_out,
    int32_t* __restrict__ nan_flag, const float w_scale, const float w_inv,
    const f16x8* __restrict__ mimg, int n_in, float* __restrict__ v_out, int64_t ldvo,
    const WlScreen* __restrict__ scr, unsigned* __restrict__ scr_count, const int probe_on) {
  static_assert(!SCREEN || (NT == 1 && NKX == 0), "screening: one sample tile per wave, no mapper in front");
  static_assert(!DRAIN || NKX == 0, "progress-ordered priority: the instances without a mapper");
  constexpr int NS = NKK * 2, NCH = NS * 2, NQ = NKK * 4, AUXR = WlGeom<NKK, (NKX > 0)>::AUXR;
  constexpr int NSX = NKX * 2, NQX = NKX * 4, MCH = NKK * NSX * 2;   // the mapper's K-steps, row pieces, 1-KiB chunks
  constexpr bool SWAP = NKX == 0;      // (the mapped instances keep xhalf)
  constexpr bool NANNV2 = SCREEN && RAYEN_WL_NANNV2 != 0;
  // (RAYEN_WL_HEAD bit 2) the first rows requested in the head, the next ones at the bottom of a group.  The mapped instances keep
  // the request at the top of the group: they sit at 128 registers with spills already, and their rows feed the mapper first
  constexpr bool ROWS_FIRST = (RAYEN_WL_HEAD & 4) != 0 && (RAYEN_WL_HEAD & 2) == 0 && NKX == 0 && RAYEN_WL_AHEAD == 0;
  extern __shared__ __attribute__((aligned(1024))) char wl_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hi = lane >> 5;
  char* const wimg = wl_smem;                                                   // [n_tiles][NS][2][64] x 16 bytes
  constexpr int REGION = NKX > 0 ? wl_region_bytes_mapped(NKK, NT) : wl_region_bytes(NKK, NT);
  constexpr int SR = NKX > 0 ? kWlStageRowsMapped : wl_stage_rows(NT);
  char* const mlds = wl_smem + (size_t)n_tiles * (NCH * 1024);                  // (mapped) [NKK][NSX][2][64] x 16 bytes
  char* const stage = mlds + MCH * 1024 + wave * REGION;
  float (*const aux_lds)[AUXR][32] = reinterpret_cast<float (*)[AUXR][32]>(stage);   // [sample tile][row][sample]
  float* const y0_lds = reinterpret_cast<float*>(mlds + MCH * 1024 + NW * REGION);
  float* const bias_lds = y0_lds + NKK * 32;                                    // (mapped) gM b, zero-padded
  unsigned* const take_lds = reinterpret_cast<unsigned*>(bias_lds + (NKX > 0 ? NKK * 32 : 0));   // the workgroup's next unclaimed group
  // Groups are dealt to WORKGROUPS statically (group b + j gridDim.x is the j-th of workgroup b) and to the waves of a
  // workgroup on demand, j from a counter in LDS: the issue arbiter prefers the older wave of a SIMD, so with equal shares
  // the first waves of a workgroup finish early and their partners walk alone at the end (s_memtime / s_memrealtime probes,
  // B = 1 048 576: wave 0 lives 156 us of a 191 us launch)
  const int64_t n_groups = (B + NT * 32 - 1) / (NT * 32);
  const int64_t grp_stride = (int64_t)gridDim.x;
  int64_t grp = (int64_t)blockIdx.x + (int64_t)wave * grp_stride;
  bool bad = false;
  bool first_walk = true;
  unsigned skipped = 0;      // (SCREEN) lane s: segment-groups of segment s this wave skipped
#ifdef RAYEN_WL_STAMPS
  int stamp_round = 0;
  bool stamp_on = false;
#endif
#ifdef RAYEN_WL_CLOCK
  const bool probe = (blockIdx.x & 15) == 0 && (blockIdx.x >> 4) < 16;      // (uniform: every wave of the workgroup stamps)
  unsigned long long clock_at[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int clock_groups = 0;
  RAYEN_WL_CLOCK_AT(0);
#endif
  // (DRAIN) the wave's progress level -- groups claimed so far, plus the steps inside its last group -- and the item at which
  // the next step falls (never, outside a last group)
  [[maybe_unused]] int drain_level = 0, drain_at = 0x7FFFFFFF;

  // ---- the image, once: chunk c (1 KiB) by wave c mod NW, by LDS-DMA (RAYEN_WL_HEAD; nothing passes through the registers).  See
  // below the request lambda for the rest of the head: the early waves' first rows behind the chunks, a wait for the chunks alone.
  for (int i = threadIdx.x; i < NKK * 32; i += NW * 64) y0_lds[i] = y0[i];
  if (threadIdx.x == 0) *take_lds = NW;     // (the first NW are the waves' first groups)
  float gm_inv = 1.f;
  int gm_exp = 0;
  if constexpr (NKX > 0) {
    const float* tail = reinterpret_cast<const float*>(mimg + (size_t)MCH * 64);
    const float gm = tail[NKK * 32];
    gm_inv = tail[NKK * 32 + 1];
    gm_exp = (int)((__builtin_bit_cast(unsigned, gm) >> 23) & 255u) - 127;
    for (int i = threadIdx.x; i < NKK * 32; i += NW * 64) bias_lds[i] = tail[i] * gm;
  }
#if !(RAYEN_WL_HEAD & 1)
  {
    const int n_chunks = n_tiles * NCH;
    const char* src = reinterpret_cast<const char*>(Wh) + lane * 16;
#pragma unroll 4
    for (int c = wave; c < n_chunks; c += NW)
      *reinterpret_cast<u32x4*>(wimg + c * 1024 + lane * 16) = *reinterpret_cast<const u32x4*>(src + (size_t)c * 1024);
  }
#endif

  // this lane's rows of group g (one per sample tile): pieces 2 q + hi (columns 8 q + 4 hi .. + 3), zero beyond the batch.
  // Buffer addressing (round 6, from the ISA: the 64-bit `row * ldv` products, the predicates and the zeroing of the flat form
  // were ~70 vector instructions per group, the multiplies at a quarter rate; the stores of y ~80): the descriptor's extent is
  // B rows, the lane's byte offset inside a group is a constant, a group adds one uniform term -- and rows beyond the batch are
  // out of range: their loads return 0, their stores are dropped by the hardware.  (Offsets are 32-bit: mfma_pair_wl_serves.)
  const __amdgpu_buffer_rsrc_t v_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(v), 0, (int)(unsigned)((uint64_t)B * (uint64_t)ldv * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t y_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(y, 0, (int)(unsigned)((uint64_t)B * (uint64_t)ldy * 4u), 0x00020000);
  const unsigned v_lane_off = (unsigned)col * (unsigned)ldv * 4u + 16u * (unsigned)hi;
  const unsigned y_lane_off = (unsigned)(lane >> 3) * (unsigned)ldy * 4u + 16u * (unsigned)((lane & 7) ^ ((lane >> 3) & 7));
  f32x4 vraw[NT][NQ];
  f32x4 xraw[NT][NKX > 0 ? NQX : 1];     // (mapped) the rows of x; vraw then holds gM sx v out of the mapper's accumulators
  // n = k below the padded width (a multiple of 4: whole pieces): the pieces beyond a row's n columns would be the next row's --
  // their offset is sent out of range instead (loads return 0, stores are dropped), one select per piece
  const bool ragged_n = n < NKK * 32;
  const bool ragged_in = NKX > 0 && n_in < NKX * 32;
  constexpr unsigned kNowhere = 0xFFFFFFF0u;
  // (`one_copy`: the head's request, once per wave -- a select per piece instead of the two copies, so that exactly NT * NQ loads
  // stand between the image's chunks and the counted wait)
  auto request = [&](const int64_t g, auto one_copy) {
    constexpr bool ONE = decltype(one_copy)::value;
    const unsigned goff = v_lane_off + (unsigned)g * (unsigned)(NT * 32) * (unsigned)ldv * 4u;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if constexpr (NKX > 0) {
        if (__builtin_expect(ragged_in, 0)) {
          asm volatile("; ragged width" ::: "memory");
#pragma unroll
          for (int q = 0; q < NQX; ++q) {
            unsigned off = goff + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q;
            off = (8 * q + 4 * hi < n_in) ? off : kNowhere;
            xraw[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, off, 0, 0));
          }
        } else {
#pragma unroll
          for (int q = 0; q < NQX; ++q)
            xraw[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                v_rsrc, goff + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q, 0, 0));
        }
      } else {
        // (two copies behind a wave-uniform branch, the empty statement keeps hipcc from folding them back into one with a select
        // per piece: at the padded width -- the headline -- the selects were 3 % of the kernel's vector instructions)
        if constexpr (ONE) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            unsigned off = goff + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q;
            off = (8 * q + 4 * hi < n) ? off : kNowhere;
            vraw[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, off, 0, 0));
          }
        } else if (__builtin_expect(ragged_n, 0)) {
          asm volatile("; ragged width" ::: "memory");
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            unsigned off = goff + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q;
            off = (8 * q + 4 * hi < n) ? off : kNowhere;
            vraw[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, off, 0, 0));
          }
        } else {
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            vraw[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                v_rsrc, goff + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q, 0, 0));
        }
      }
    }
  };
  // largest |component| of the requested rows (this lane's half of each): the FIRST use of the rows' registers.  It sits in
  // front of the previous group's stores of y -- vmcnt retires in order and counts stores, so a wait for these loads that
  // came behind the stores would wait for the stores' HBM round trip as well
  float m_half[NT];
  auto half_max = [&]() {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float m = 0.f;
      if constexpr (NKX > 0) {
#pragma unroll
        for (int q = 0; q < NQX; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) m = fmaxf(m, __builtin_fabsf(xraw[t][q][c]));
      } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) m = fmaxf(m, __builtin_fabsf(vraw[t][q][c]));
      }
      m_half[t] = m;
      asm volatile("" : "+v"(m_half[t]));   // (pinned here: hipcc otherwise sinks the maxima -- and their wait -- behind the stores)
    }
  };
#pragma unroll
  for (int t = 0; t < NT; ++t) m_half[t] = 0.f;
  // One 128-byte line (h) of each of a sample tile's 32 rows out of the registers that hold pieces 2 qq + hi of the lane's OWN row:
  // through the wave's LDS (slot = piece ^ (row & 7): the eight lanes of a write or read group hit eight different 16-byte bank
  // groups), SR rows at a time, and out as whole lines -- lane L stores slot L & 7 of row 8 i + (L >> 3).  `goff` = the lane's
  // constant offset + the group's rows, `ld4` = the leading dimension in bytes; pieces beyond `width` columns and rows beyond
  // the batch are out of the descriptor's range.
  auto put_lines = [&](const f32x4 (&o)[4], const int h, const int t, const __amdgpu_buffer_rsrc_t rsrc, const unsigned goff,
                       const unsigned ld4, const int width, const bool ragged) {
#pragma unroll
    for (int part = 0; part < 32 / SR; ++part) {      // rows [SR part, SR part + SR) of the tile
      if (SR == 32 || (col / SR) == part) {
        char* slot = stage + (col % SR) * 128;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) *reinterpret_cast<f32x4*>(slot + (((2 * qq + hi) ^ (col & 7)) * 16)) = o[qq];
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < SR / 8; ++i) {
        const int r = 8 * i + (lane >> 3);
        const f32x4 x = *reinterpret_cast<const f32x4*>(stage + r * 128 + (lane & 7) * 16);
        // row (lane >> 3) of the eight, slot (lane & 7) ^ (row & 7): the lane's constant; rows beyond the batch are dropped
        unsigned off = goff + (unsigned)(t * 32 + part * SR + 8 * i) * ld4 + 128u * h;
        if (__builtin_expect(ragged, 0)) {
          asm volatile("; ragged width" ::: "memory");     // (a branch, not a select per store: see request)
          off = (32 * h + 4 * ((lane & 7) ^ ((lane >> 3) & 7)) < width) ? off : kNowhere;
        }
        if constexpr (RAYEN_WL_ABL & 2) { if (x[0] == 123.456f) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), rsrc, off, 0, 0); }
        else if constexpr (RAYEN_WL_ABL & 8) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), rsrc, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), rsrc, off, 0, 2);   // (2: non-temporal)
      }
      __builtin_amdgcn_wave_barrier();
    }
  };
#if RAYEN_WL_HEAD
  {
    // the image's chunks, then -- behind them, loads retire in order -- the wave's first rows.  Bit 2 (ROWS_FIRST): the group's real
    // request, into the row registers; the HBM round trip runs while the other waves' chunks land and the barrier opens.  Bit 1
    // (rounds 6-9, off): pulled towards L2 into the wave's own (still unused) kilobyte and thrown away, whole groups only (that
    // path has no bounds), the real request at the top of the walk.  Only the image is waited for.
    const int n_chunks = n_tiles * NCH;
    const unsigned img_at = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(wimg));
    const unsigned lane16 = lane * 16;
    if (RAYEN_WL_HEAD & 1)
      for (int c = wave; c < n_chunks; c += NW)
        wl_dma16(reinterpret_cast<const char*>(Wh) + (size_t)c * 1024, lane16, img_at + c * 1024);
    if constexpr (NKX > 0)
      for (int c = wave; c < MCH; c += NW)
        wl_dma16(reinterpret_cast<const char*>(mimg) + (size_t)c * 1024, lane16, img_at + (n_chunks + c) * 1024);
    if ((RAYEN_WL_HEAD & 2) && (grp + 1) * (NT * 32) <= B) {
      const char* gb = reinterpret_cast<const char*>(v + grp * (NT * 32) * ldv);
      const unsigned lds_at = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(stage));
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < NQ; ++q) wl_dma16(gb, v_lane_off + (unsigned)t * 32u * (unsigned)ldv * 4u + 32u * q, lds_at);
      asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NT * NQ) : "memory");
    } else if (ROWS_FIRST && wave < RAYEN_WL_EARLY && grp < n_groups) {
      // (bit 2) the first rows of the workgroup's first RAYEN_WL_EARLY waves behind the image's chunks: NT * NQ loads --
      // everything older has landed once that many are outstanding.  Every other wave waits for everything.
      request(grp, std::true_type{});
      asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NT * NQ) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
#endif
  if (RAYEN_WL_AHEAD && grp < n_groups) {
    request(grp, std::false_type{});
    half_max();
  }
  __syncthreads();  // the only workgroup barrier: the image is in LDS
  // (bit 2) the later waves' first rows, behind the barrier as in rounds 6-9: they arrive while the early waves split and multiply
  if constexpr (ROWS_FIRST) {
    if (wave >= RAYEN_WL_EARLY && grp < n_groups) request(grp, std::true_type{});
  }

  while (grp < n_groups) {
    const int64_t s_base = grp * (NT * 32);
    int taken = 0;
    if (lane == 0) taken = (int)atomicAdd(take_lds, 1u);
    const int64_t next = (int64_t)blockIdx.x + (int64_t)__builtin_amdgcn_readfirstlane(taken) * grp_stride;
    bool live[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) live[t] = (s_base + t * 32 + col) < B;
    if constexpr (DRAIN) {
      wl_set_level(drain_level);
      drain_level = drain_level < 3 ? drain_level + 1 : 3;      // (the next group's level, or the first step inside this one)
      drain_at = next >= n_groups ? n_items / 3 : 0x7FFFFFFF;
    }
    if constexpr (!RAYEN_WL_AHEAD) {
      // (ROWS_FIRST: the rows were requested in the head or at the bottom of the previous group; only their first use is here)
      if constexpr (!ROWS_FIRST) request(grp, std::false_type{});
      half_max();
    }

#ifdef RAYEN_WL_STAMPS
    stamp_on = blockIdx.x == 0 && (wave == 0 || wave == 4) && stamp_round == RAYEN_WL_STAMP_ROUND;
    ++stamp_round;
    RAYEN_WL_STAMP(38, 0);
#endif
    // ---- rows -> scaled f16 pairs.  sv = 2^(13 - floor(log2 max|v|)): exponent arithmetic only (rayen_mfma_pair.hip);
    // vb[t][piece][k-step] = 8 f16 = the B operand of one MFMA; element i = column 16 sp + 8 (i >> 2) + 4 hi + (i & 3)
    f16x8 vb[NT][2][NS];
    float v_scl[NT], v_inv[NT];
    bool nan_row[NT];
    int sx_exp[NT];
    if constexpr (NKX > 0) {
      // ---- the mapper: x scaled per sample (sx, a power of two) and split like v; the accumulators start at gM sx b; per K-step
      // of x and row tile of v the three products in the order of rayen_mfma_pair.hip (a2 x1, a1 x2, a1 x1); A operands from LDS.
      // The fp32 results ARE in B-operand order: register 4 a + c of row tile tp is direction element 32 tp + 8 a + 4 hi + c.
      static_assert(NT == 1, "the mapped instances walk one sample tile per wave");
      static_assert((RAYEN_WL_HEAD & 1) != 0, "the mapper's image is copied by the LDS-DMA head");
      const unsigned vo_goff = (unsigned)(lane >> 3) * (unsigned)ldvo * 4u + 16u * (unsigned)((lane & 7) ^ ((lane >> 3) & 7)) +
                               (unsigned)s_base * (unsigned)ldvo * 4u;
      const __amdgpu_buffer_rsrc_t vo_rsrc =
          __builtin_amdgcn_make_buffer_rsrc(v_out, 0, (int)(unsigned)((uint64_t)B * (uint64_t)ldvo * 4u), 0x00020000);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float mx = fmaxf(m_half[t], xhalf(m_half[t]));
        float sx, sx_inv;
        pow2_scale(mx, sx, sx_inv, sx_exp[t]);
        f32x16 macc[NKK];
#pragma unroll
        for (int tp = 0; tp < NKK; ++tp)
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(&bias_lds[32 * tp + 8 * a4 + 4 * hi]);
#pragma unroll
            for (int c = 0; c < 4; ++c) macc[tp][4 * a4 + c] = b4[c] * sx;
          }
#pragma unroll
        for (int sxs = 0; sxs < NSX; ++sxs) {
          u32x4 w1, w2;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = 2 * sxs + (j >> 1), c = 2 * (j & 1);
            unsigned a, b;
            pair_split_lo(a, b, xraw[t][q][c], sx);
            pair_split_hi(a, b, xraw[t][q][c + 1], sx);
            w1[j] = a;
            w2[j] = b;
          }
          const f16x8 xb0 = __builtin_bit_cast(f16x8, w1), xb1 = __builtin_bit_cast(f16x8, w2);
#pragma unroll
          for (int tp = 0; tp < NKK; ++tp) {
            const char* ch = mlds + (size_t)((tp * NSX + sxs) * 2) * 1024 + lane * 16;
            const f16x8 a1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(ch));
            const f16x8 a2 = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(ch + 1024));
            macc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, xb0, macc[tp], 0, 0, 0);
            macc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, xb1, macc[tp], 0, 0, 0);
            macc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, xb0, macc[tp], 0, 0, 0);
          }
        }
        // macc = gM sx v.  v itself leaves only for the backward (training): the same lines as y
        if (v_out != nullptr) {
#pragma unroll
          for (int h = 0; h < NKK; ++h) {
            f32x4 o[4];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
              for (int c = 0; c < 4; ++c) o[qq][c] = fmaf(macc[h][4 * qq + c] * gm_inv, sx_inv, 0.f);
            put_lines(o, h, t, vo_rsrc, vo_goff, (unsigned)ldvo * 4u, n, ragged_n);
          }
        }
        float m = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            vraw[t][q][c] = macc[q >> 2][4 * (q & 3) + c];
            m = fmaxf(m, __builtin_fabsf(vraw[t][q][c]));
          }
        m_half[t] = m;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float m = wl_half_max<SWAP>(m_half[t]);
      float sv;
      int sv_exp;
      pow2_scale(m, sv, v_inv[t], sv_exp);
      v_scl[t] = sv;
      if constexpr (NKX > 0) {
        // the pieces are split from f x (gM sx v), f = the power of two above; sv = f gM sx as a power of two (the exponents are
        // added: the product of the floats could overflow on the way)
        int e = sv_exp + gm_exp + sx_exp[t];
        e = e > 126 ? 126 : (e < -126 ? -126 : e);
        v_scl[t] = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
        v_inv[t] = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
      }
      f16x2 z = {(_Float16)0.f, (_Float16)0.f};
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        u32x4 w1, w2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {           // register j of the K-step: columns q = 2 sp + (j >> 1), c = 2 (j & 1) + {0, 1}
          const int q = 2 * sp + (j >> 1), c = 2 * (j & 1);
          unsigned a, b;
          pair_split_lo(a, b, vraw[t][q][c], sv);
          pair_split_hi(a, b, vraw[t][q][c + 1], sv);
          w1[j] = a;
          w2[j] = b;
          if constexpr (!NANNV2) pair_nan_fold(z, a);
        }
        vb[t][0][sp] = __builtin_bit_cast(f16x8, w1);
        vb[t][1][sp] = __builtin_bit_cast(f16x8, w2);
      }
      if constexpr (!NANNV2) nan_row[t] = pair_nan_seen(z);
    }
    // (SCREEN) ||sv v||^2 of the lane's row, from the SCALED values (a row of 1e-25 does not underflow to a bound of 0): two
    // chains over the lane's half, the halves added
    float nv2 = 0.f;
    if constexpr (SCREEN) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < 4; c += 2) {
          const float x0 = vraw[0][q][c] * v_scl[0], x1 = vraw[0][q][c + 1] * v_scl[0];
          s0 = fmaf(x0, x0, s0);
          s1 = fmaf(x1, x1, s1);
        }
      nv2 = wl_half_sum<SWAP>(s0 + s1);
      if constexpr (NANNV2) nan_row[0] = !(nv2 < __builtin_inff());
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- the next group's rows: in flight for the whole walk
    if (RAYEN_WL_AHEAD && next < n_groups && !(RAYEN_WL_ABL & 1)) request(next, std::false_type{});
    __builtin_amdgcn_sched_barrier(0);

    // kap, part, the aux patch and the accumulators live in the SCALED domain (gW sv times the natural value)
    float kap[NT], part[NT];
    int acode[NT];   // arg-max bookkeeping in one register: (segment << 20) | row, -1 = none
#pragma unroll
    for (int t = 0; t < NT; ++t) { kap[t] = 0.f; part[t] = 0.f; acode[t] = -1; }
    {
      f32x16 acc[NT];
      const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // The A operands of an item are read from LDS one item AHEAD, right behind the previous item's MFMAs: their latency
      // runs under that item's epilogue (the chunk registers are dead once its MFMAs have read them).  The last item of a
      // group fetches the first item's chunks for the next group.
      const int ts_first = items[0].tile_shape;
      int ts_next = ts_first;
      u32x4 abuf[NCH];   // [2 sp + 0] leading piece, [2 sp + 1] second piece of K-step sp
      auto fetch = [&](const int ts_of) {
        const char* tb = wimg + (size_t)(ts_of & 0xFFFFFF) * (NCH * 1024) + lane * 16;
        if constexpr (NS == 4) {
          const int shape = __builtin_amdgcn_readfirstlane((ts_of >> 24) & 3);
          if (shape != MS_HALF_B) {
#pragma unroll
            for (int c = 0; c < 4; ++c) abuf[c] = *reinterpret_cast<const u32x4*>(tb + c * 1024);
          }
          if (shape != MS_HALF_A) {
#pragma unroll
            for (int c = 4; c < 8; ++c) abuf[c] = *reinterpret_cast<const u32x4*>(tb + c * 1024);
          }
        } else {
#pragma unroll
          for (int c = 0; c < NCH; ++c) abuf[c] = *reinterpret_cast<const u32x4*>(tb + c * 1024);
        }
      };
      if (first_walk) {
        fetch(ts_first);
        first_walk = false;
      }
      const int n_walk = n_items - ((RAYEN_WL_ABL & 64) ? 4 : 0);
      for (int it = 0; it < n_walk; ++it) {
        RAYEN_WL_STAMP(it, 0);
        if constexpr (DRAIN) {
          if (it >= drain_at) {      // (a further step down inside the wave's last group)
            wl_set_level(drain_level);
            drain_level = drain_level < 3 ? drain_level + 1 : 3;
            drain_at = drain_at < 2 * (n_items / 3) ? 2 * (n_items / 3) : 0x7FFFFFFF;
          }
        }
#ifdef RAYEN_WL_CLOCK
        if (it == 0 && clock_groups == 0) RAYEN_WL_CLOCK_AT(1);
#endif
        const int ts = ts_next;      // (known since the previous item: nothing in front of the burst waits for a scalar load)
        // Two passes over the item's K-steps, by product size: the 2^-11 cross products first, the leading products last
        // (rayen_mfma_pair.hip).  A full tile multiplies all K-steps; the halves of a shared tile (rayen_tiles.h) K-steps
        // 0,1 or 2,3, the accumulator starting afresh at the first of them.
        auto burst = [&](auto S0, auto S1) {
          constexpr int s0 = decltype(S0)::value, s1 = decltype(S1)::value;
#pragma unroll
          for (int sp = s0; sp < s1; ++sp) {
            const f16x8 a1 = __builtin_bit_cast(f16x8, abuf[2 * sp + 0]), a2 = __builtin_bit_cast(f16x8, abuf[2 * sp + 1]);
#pragma unroll
            for (int t = 0; t < NT; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, vb[t][0][sp], sp == s0 ? zero : acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, vb[t][1][sp], acc[t], 0, 0, 0);
          }
#pragma unroll
          for (int sp = s0; sp < s1; ++sp) {
            const f16x8 a1 = __builtin_bit_cast(f16x8, abuf[2 * sp + 0]);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, vb[t][0][sp], acc[t], 0, 0, 0);
          }
        };
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RAYEN_WL_ABL & 32) {
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[t][g] = __builtin_bit_cast(float, __builtin_bit_cast(u32x4, vb[t][0][g & 3])[g >> 2]);
        } else if constexpr (NS == 4) {
          const int shape = __builtin_amdgcn_readfirstlane((ts >> 24) & 3);
          if (shape == MS_FULL) burst(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
          else if (shape == MS_HALF_A) burst(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
          else burst(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
        } else {
          burst(std::integral_constant<int, 0>{}, std::integral_constant<int, NS>{});
        }
        __builtin_amdgcn_sched_barrier(0);
        // (the item's record is requested BEHIND its MFMAs: LDS and scalar loads share a counter that hipcc can only wait
        // out in full, so a request in front of the burst would hold the MFMAs back for the scalar cache's latency)
        const MItem item = items[it];
        WlScreen sc_next;
        if constexpr (SCREEN) sc_next = scr[it + 1];      // (a blank record behind the last item)
        ts_next = (it + 1 < n_walk) ? item.qbegin : ts_first;      // (qbegin: the NEXT item's tile and shape, mfma_pair_build)
        if constexpr (!(RAYEN_WL_ABL & 32)) fetch(ts_next);
        RAYEN_WL_STAMP(it, 1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RAYEN_WL_ABL & 16) {
#pragma unroll
          for (int t = 0; t < NT; ++t) kap[t] = fmaxf(kap[t], acc[t][0]);
          continue;
        }

        if (item.type == MI_LIN) {
          const int lin_code = (item.seg << 20) + item.row0 + 4 * hi;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if (TRACK) {
#pragma unroll
              for (int g = 0; g < 16; ++g)
                if (acc[t][g] > kap[t]) {
                  kap[t] = acc[t][g];
                  acode[t] = lin_code + ((g & 3) + 8 * (g >> 2));
                }
            } else {
#pragma unroll
              for (int g = 0; g < 16; ++g) kap[t] = fmaxf(kap[t], acc[t][g]);
            }
          }
        } else if (item.type == MI_QFAC || item.type == MI_SOC) {
          // a running sum of squares over the segment's tiles, closed on its last tile (two chains of plain FMAs: the values
          // of the other schedules' packed FMA, in instructions that issue under a partner's MFMAs)
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            float s0 = (item.flags & MF_FIRST) ? 0.f : part[t], s1 = 0.f;
#pragma unroll
            for (int g = 0; g < 16; g += 2) {
              s0 = fmaf(acc[t][g], acc[t][g], s0);
              s1 = fmaf(acc[t][g + 1], acc[t][g + 1], s1);
            }
            part[t] = s0 + s1;
          }
          if (item.flags & MF_LAST) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const float total = wl_half_sum<SWAP>(part[t]);
              const float a0 = aux_lds[t][item.aux][col];
              float kc;
              if (item.type != MI_SOC) {
                kc = (a0 + __builtin_amdgcn_sqrtf(fmaxf(total, 0.f))) * item.seg_inv;   // (the segment's own power of two undone)
              } else {
                kc = pair_soc_candidate(a0, aux_lds[t][item.aux + 1][col], total, w_inv * item.seg_inv, v_inv[t], item.f0,
                                        item.f1, v_scl[t], w_scale);
              }
              if (kc > kap[t]) { kap[t] = kc; acode[t] = item.seg << 20; }
            }
          }
        } else if (item.type == MI_AUX) {
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < AUXR / 2; ++g) aux_lds[t][(g & 3) + 8 * (g >> 2) + 4 * hi][col] = acc[t][g];   // (rows 0 .. AUXR - 1 of the tile)
          __builtin_amdgcn_wave_barrier();
        } else if (item.type == MI_PACK) {
          const MPack pk = packs[item.aux];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const int slot = hi ? pk.aux[a][1] : pk.aux[a][0];
            const int sid = hi ? pk.seg[a][1] : pk.seg[a][0];
            const bool pair = (item.row0 >> a) & 1;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              float qs = acc[t][4 * a] * acc[t][4 * a];
#pragma unroll
              for (int c = 1; c < 4; ++c) qs = fmaf(acc[t][4 * a + c], acc[t][4 * a + c], qs);
              if (pair) qs = wl_half_sum<SWAP>(qs);
              const float kc = (aux_lds[t][slot & (AUXR - 1)][col] + __builtin_amdgcn_sqrtf(qs)) * (hi ? pk.inv[a][1] : pk.inv[a][0]);
              if (sid >= 0 && kc > kap[t]) { kap[t] = kc; acode[t] = sid << 20; }
            }
          }
        }
        RAYEN_WL_STAMP(it, 2);
        if constexpr (SCREEN) {
          // ---- Screening (header): the next item opens a segment whose candidate may be provably below the running maximum
          // of every live lane -- then its items are not walked.  The segments behind it are decided here too, until one stays.
          if (sc_next.cnst > 0.f || sc_next.cabs > 0.f) {
            WlScreen s = sc_next;
            int nx = it + 1, ts_to = ts_next;
            const int ts_held = ts_next;      // the item whose operands abuf holds (the probe reads operands of its own)
            // (kap does not change between here and the end of the decisions: the probe writes acc and part only)
            [[maybe_unused]] const float kmax_held = wl_half_max<SWAP>(kap[0]);
            auto kmax_now = [&] { return RAYEN_WL_KMAX_ONCE ? kmax_held : wl_half_max<SWAP>(kap[0]); };
            // (a NaN or an infinite row decides nothing: every comparison with it is false)
            const bool nv_ok = nv2 < __builtin_inff();
            // (the probe's margin is proved for a row whose largest scaled entry reached 2^13 -- every row but one below 2^-113,
            // where the scale is clamped -- and for the zero row, whose products are all zero)
            const bool probe_row = (nv2 >= 67108864.f) || (nv2 == 0.f);
            for (;;) {
              bool skip = false;
              if (s.cnst > 0.f) {
                const float tb = s.cnst * nv2;
                const float a0 = aux_lds[0][s.aux][col];
                float ub;
                if (!(s.span >> 16)) {
                  ub = (a0 + __builtin_amdgcn_sqrtf(fmaxf(tb, 0.f))) * s.seg_inv;
                } else {
                  ub = pair_soc_candidate(a0, aux_lds[0][s.aux + 1][col], tb, w_inv * s.seg_inv, v_inv[0], s.f0, s.f1, v_scl[0], w_scale);
                }
                const bool below = (ub < kmax_now()) && nv_ok;
                skip = __ballot(live[0] && !below) == 0;
              }
              if (!skip && probe_on != 0 && s.cabs > 0.f) {
                // ---- Probe (header): the segment's sum of squares from the LEADING products a1 b1 alone, a third of the MFMAs,
                // into acc / part (dead between two segments); only the leading pieces of its items are read from LDS
                const int span = s.span & 0xFFFF;
                int ts_j = ts_to;
                for (int j = 0; j < span; ++j) {
                  const char* tb = wimg + (size_t)(ts_j & 0xFFFFFF) * (NCH * 1024) + lane * 16;
                  const int shape = NS == 4 ? __builtin_amdgcn_readfirstlane((ts_j >> 24) & 3) : MS_FULL;
                  // (operands of the probe's own, always from LDS -- the first item's leading pieces a second time: a conditional
                  // overwrite of abuf cost ~30 register copies per probed segment, and a probe that fails finds abuf intact)
                  auto lead = [&](auto S0, auto S1) {
                    constexpr int s0 = decltype(S0)::value, s1 = decltype(S1)::value;
                    u32x4 pa[NS];
#pragma unroll
                    for (int sp = s0; sp < s1; ++sp) pa[sp] = *reinterpret_cast<const u32x4*>(tb + (2 * sp) * 1024);
#pragma unroll
                    for (int sp = s0; sp < s1; ++sp)
                      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, pa[sp]), vb[0][0][sp],
                                                                      sp == s0 ? zero : acc[0], 0, 0, 0);
                  };
                  if constexpr (NS == 4) {
                    if (shape == MS_FULL) lead(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
                    else if (shape == MS_HALF_A) lead(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
                    else lead(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
                  } else {
                    lead(std::integral_constant<int, 0>{}, std::integral_constant<int, NS>{});
                  }
                  if (j + 1 < span) ts_j = items[nx + j].qbegin;
                  float s0 = j == 0 ? 0.f : part[0], s1 = 0.f;
#pragma unroll
                  for (int g = 0; g < 16; g += 2) {
                    s0 = fmaf(acc[0][g], acc[0][g], s0);
                    s1 = fmaf(acc[0][g + 1], acc[0][g + 1], s1);
                  }
                  part[0] = s0 + s1;
                }
                const float total = wl_half_sum<SWAP>(part[0]);
                const float r = __builtin_amdgcn_sqrtf(fmaxf(total, 0.f)) + __builtin_amdgcn_sqrtf(s.cabs * nv2);
                const float tb = (r * r) * 1.000244140625f;      // (1 + 2^-12: the fp32 roundings of both sums and of this line)
                const float a0 = aux_lds[0][s.aux][col];
                float ub;
                if (!(s.span >> 16)) {
                  ub = (a0 + __builtin_amdgcn_sqrtf(fmaxf(tb, 0.f))) * s.seg_inv;
                } else {
                  ub = pair_soc_candidate(a0, aux_lds[0][s.aux + 1][col], tb, w_inv * s.seg_inv, v_inv[0], s.f0, s.f1, v_scl[0], w_scale);
                }
                const bool below = (ub < kmax_now()) && nv_ok && probe_row;
                skip = __ballot(live[0] && !below) == 0;
              }
              if (!skip) break;
              nx += s.span & 0xFFFF;
              ts_to = s.ts_after;
              skipped += (lane == s.seg) ? 1u : 0u;
              if (ts_to < 0) break;
              s = scr[nx];
              if (!(s.cnst > 0.f) && !(s.cabs > 0.f)) break;
            }
            if (nx != it + 1) {
              // the A operands already fetched belong to a skipped item: those of the item that does run are fetched below (none
              // left: the first item's, for the next group)
              ts_next = ts_to < 0 ? ts_first : ts_to;
              it = nx - 1;
            }
            // (nothing skipped: abuf still holds the next item's operands, whatever the probes read)
            if (ts_held != ts_next) fetch(ts_next);
          }
        }
      }
    }
    RAYEN_WL_STAMP(38, 1);

    // ---- kappa is final
    float knat[NT], scale[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (TRACK || !SWAP) {      // (the arg-max exchange needs the other half's value itself)
        const float other = xhalf(kap[t]);
        if (TRACK) {
          const int ocode = __shfl_xor(acode[t], 32);
          if (other > kap[t] || (other == kap[t] && hi == 1)) acode[t] = ocode;
        }
        kap[t] = fmaxf(kap[t], other);
      } else {
        kap[t] = wl_half_max<SWAP>(kap[t]);
      }
      knat[t] = (kap[t] * w_inv) * v_inv[t];
      scale[t] = v_inv[t] * (1.0f / fmaxf(1.0f, knat[t]));   // (the rebuilt direction carries sv only)
    }
    if (hi == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (!live[t]) continue;
        const int64_t s = s_base + t * 32 + col;
        if (kappa_out) kappa_out[s] = knat[t];
        if (TRACK) { active_out[2 * s] = acode[t] >> 20; active_out[2 * s + 1] = acode[t] < 0 ? 0 : (acode[t] & 0xFFFFF); }
      }
    }

    // the next rows have had the walk to arrive: first use (see half_max; unconditional -- on every path into the next group
    // the loads have been waited for)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (RAYEN_WL_AHEAD) half_max();
    __builtin_amdgcn_sched_barrier(0);

    // ---- y = y0 + v / max(1, kappa): v rebuilt from its pieces (22 bits of it; scaled by sv, undone by `scale`).  A lane
    // holds pieces 2 q + hi of ITS row: written to memory as they are, every store instruction would touch 32 lines with 32
    // bytes each (measured: non-temporal 331 us, plain 197 us at B = 1 048 576 against 157 without the stores, and the plain
    // ones leave the L2 dirty for the end of the kernel).  So one 128-byte line of each of the tile's 32 rows at a time goes
    // through the wave's 4 KiB of LDS (slot = piece ^ (row & 7): the eight lanes of a write or read group hit eight different
    // 16-byte bank groups) and leaves as whole lines: lane L stores slot L & 7 of row 8 i + (L >> 3).
    const unsigned y_goff = y_lane_off + (unsigned)s_base * (unsigned)ldy * 4u;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float one = 1.0f;
      asm volatile("" : "+v"(one));
#pragma unroll
      for (int h = 0; h < NKK; ++h) {          // line h of the tile's rows
        f32x4 o[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int q = 4 * h + qq;
          const f32x4 o4 = *reinterpret_cast<const f32x4*>(&y0_lds[8 * q + 4 * hi]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = (q & 1) * 4 + c;
            const unsigned w1 = __builtin_bit_cast(u32x4, vb[t][0][q >> 1])[i >> 1], w2 = __builtin_bit_cast(u32x4, vb[t][1][q >> 1])[i >> 1];
            const float val = (i & 1) ? pair_rebuild_hi(w1, w2, one) : pair_rebuild_lo(w1, w2, one);     // fl32(p1 + p2)
            o[qq][c] = fmaf(val, scale[t], o4[c]);
          }
        }
        put_lines(o, h, t, y_rsrc, y_goff, (unsigned)ldy * 4u, n, ragged_n);
      }
      bad |= live[t] && nan_row[t];      // (the row's own components: y is NaN exactly when one of them is NaN or Inf)
    }
    RAYEN_WL_STAMP(38, 2);
#ifdef RAYEN_WL_CLOCK
    if (clock_groups == 0) RAYEN_WL_CLOCK_AT(2);
    ++clock_groups;
#endif
    // (ROWS_FIRST) the next group's rows, right behind the last store of y: the row registers are dead from the split to here, and
    // the guard is the loop's own condition.  The wait at the top covers these stores either way (vmcnt retires in order).
    if constexpr (ROWS_FIRST) {
      __builtin_amdgcn_sched_barrier(0);
      if (next < n_groups) request(next, std::false_type{});
    }
    grp = next;
  }  // persistent loop over sample groups
  if (nan_flag && bad) atomicOr(nan_flag, 1);
  if constexpr (SCREEN) {
    if (scr_count != nullptr && skipped != 0) atomicAdd(scr_count + lane, skipped);      // one atomic instruction per wave
  }
#ifdef RAYEN_WL_CLOCK
  RAYEN_WL_CLOCK_AT(3);
  if (probe && lane == 0) {
    unsigned long long* const rec = wl_clock_buf + ((blockIdx.x >> 4) * 16 + (wave & 15)) * kWlClockSlots;
#pragma unroll
    for (int i = 0; i < 8; ++i) rec[i] = clock_at[i];
    rec[8] = __builtin_amdgcn_s_getreg(63492);      // (HW_REG_HW_ID, all 32 bits: the SIMD is bits 5:4)
    rec[9] = (unsigned long long)clock_groups;
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static int pair_wl_lds_bytes_mapped(const PairImage* img, int nkx) {
  return img->n_tiles * (img->nkk * 4 * 1024) + img->nkk * (nkx * 2) * 2 * 1024 + kWlWaves * wl_region_bytes_mapped(img->nkk, 1) +
         2 * img->nkk * 128 + 16;
}
static int pair_wl_lds_bytes(const PairImage* img) {
  return img->n_tiles * (img->nkk * 4 * 1024) + kWlWaves * wl_region_bytes(img->nkk, kWlNT) + img->nkk * 128 + 16;
}

bool mfma_pair_wl_serves(const RayenPack* p, const PairImage* img, const float* v, int64_t B, int64_t ldv,
                         const float* y, int64_t ldy) {
  if (img == nullptr || img->nkk < 1 || img->nkk > 2 || img->n_tiles <= 0 || !img->wl_ready) return false;
  // (n = k: the padded width or, round 6, anything down to the next narrower instance in whole 16-byte pieces -- config 2's 16)
  if (!img->identity || p->k != p->n || p->n > img->nkk * 32 || p->n <= (img->nkk - 1) * 32 || (p->n % 4) != 0) return false;
  if (ldv < p->n || ldy < p->n) return false;
  if ((ldv % 4) != 0 || (ldy % 4) != 0) return false;
  // (buffer addressing with 32-bit byte offsets: mfma_pair_wl_forward cuts a batch beyond 4 GiB of rows into several launches)
  if (ldv > (1 << 22) || ldy > (1 << 22)) return false;
  if (!base_aligned16(v) || !base_aligned16(y)) return false;
  if (img->nkk == 2 && img->aux_rows > WlGeom<2>::AUXR) return false;
  if (pair_wl_lds_bytes(img) > 160 * 1024) return false;
  // Every batch size (round 6, gpurun_out/r06zzd, r06zze; config 3, us per call): the grid is one workgroup per CU as soon as there is
  // a group for it, so a small batch leaves most waves of a workgroup idle and its busy waves alone on their SIMDs --
  //   B = 32: 10.7 (plain 15.6) | 4 096: 11.3 (18.6) | 32 768: 13.6 (19.3) | 65 536: 15.9 (20.9, W-stationary) | 98 304: 20.5 (24.9) | 131 072: 25.5 (29.7)
  // (the other schedules pull the 112 KiB image through every wave's vector-memory path from L2; here one copy per CU, then LDS).
  // Until the grid covered every CU (it was n_groups / 16 workgroups) this schedule lost below 98 304 rows.
  const int64_t n_groups = (B + kWlNT * 32 - 1) / (kWlNT * 32);
  static const int64_t min_groups_env = [] { const char* e = getenv("RAYEN_WL_MIN_GROUPS"); return e ? atoll(e) : 1ll; }();   // developer sweeps
  return n_groups >= min_groups_env;
}

// (pack creation, this thread: the gate's launches choose their own mode, whatever the switch says, and count into their own buffer)
static thread_local unsigned* wl_gate_counters = nullptr;
static thread_local int wl_gate_mode = 1;      // 0: the instances of round 6 (the ordering launch) | 2: spectral test only | 1: both

// Which segments are worth a decision, and in which order this schedule walks them.  A decision costs vector instructions in
// a kernel whose vector time adds to its matrix time: a set whose quadratics take turns at the maximum never skips them and ran
// 6-7 % SLOWER with every segment decided (profiles/bench/r07_wl_screen.txt).  So, once per pack: 4 096 directions uniform in
// [-1, 1]^n (fixed seed; kappa and the bounds are homogeneous in v, only the direction matters) go through
//   1. the tracking instance of round 6: how often each segment sets kappa.  The quadratics / cones of a run of adjacent segments
//      are walked in that order, most frequent first (pair_wl_reorder: the probe pays only against a high running maximum; a
//      candidate's bits do not depend on its place and kappa is a maximum) -- this schedule's own copy of the list;
//   2. (unless RAYEN_PAIR_SCREEN_GATE=0) the screening instance twice with the counters armed, spectral test alone and with the
//      probe.  A segment the spectral test skipped for less than a quarter of the 32-sample groups loses its constant; a segment
//      whose probe, in the groups the spectral test left to it, skipped less than kMinProbeShare loses its probe.  By MFMA count
//      a probe breaks even at 1/3 (a skip saves two thirds of the segment, a failed probe costs one third more), the failed
//      probe's second epilogue and re-fetch move that up: 1/2 (profiles/bench/r08_wl_probe.txt).
// A pack left without a segment to decide runs the instances of round 6 on the shared list.  Anything that goes wrong here turns
// screening off for the pack; the results never depend on it.
static void wl_screen_gate(const RayenPack* p, PairImage* img, const bool gate) {
  constexpr int kProbe = 4096;
  constexpr double kMinShare = 0.25;
  constexpr double kMinProbeShare = 0.5;
  const int n = p->n;
  auto drop = [&] {
    (void)hipFree(img->wl_screen);
    img->wl_screen = nullptr;
    img->host_screen.clear();
    if (img->wl_items) (void)hipFree(img->wl_items);
    img->wl_items = nullptr;
    img->wl_host_items.clear();
  };
  std::vector<float> dirs((size_t)kProbe * n);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  for (float& x : dirs) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    x = (float)((double)(state >> 11) / (double)(1ull << 53) * 2.0 - 1.0);
  }
  float *dv = nullptr, *dy = nullptr;
  unsigned* dc = nullptr;
  int32_t* da = nullptr;
  unsigned counts_s[64] = {0}, counts_b[64] = {0};
  std::vector<int32_t> act((size_t)2 * kProbe, -1);
  auto launch = [&](const int mode, int32_t* active) {
    wl_gate_counters = dc;
    wl_gate_mode = mode;
    const bool fine = mfma_pair_wl_forward(p, img, dv, kProbe, n, dy, n, nullptr, active, nullptr, nullptr) == RAYEN_OK;
    wl_gate_counters = nullptr;
    wl_gate_mode = 1;
    return fine && hipStreamSynchronize(nullptr) == hipSuccess;
  };
  bool ok = hipMalloc(&dv, dirs.size() * sizeof(float)) == hipSuccess && hipMalloc(&dy, dirs.size() * sizeof(float)) == hipSuccess &&
            hipMalloc(&dc, sizeof(counts_s)) == hipSuccess && hipMalloc(&da, act.size() * sizeof(int32_t)) == hipSuccess &&
            hipMemcpy(dv, dirs.data(), dirs.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemset(dc, 0, sizeof(counts_s)) == hipSuccess;
  // ---- 1. the order
  ok = ok && launch(0, da) && hipMemcpy(act.data(), da, act.size() * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
  if (ok) {
    std::vector<uint64_t> hits(p->segs.size(), 0);
    for (int r = 0; r < kProbe; ++r) {
      const int32_t sg = act[(size_t)2 * r];
      if (sg >= 0 && (size_t)sg < hits.size()) ++hits[sg];
    }
    std::vector<MItem> own = img->host_items;
    std::vector<WlScreen> tab = img->host_screen;
    if (pair_wl_reorder(own, tab, hits)) {
      ok = upload_to_device(own, &img->wl_items, &img->bytes) &&
           hipMemcpy(img->wl_screen, tab.data(), tab.size() * sizeof(WlScreen), hipMemcpyHostToDevice) == hipSuccess;
      if (ok) {
        img->wl_host_items.swap(own);
        img->host_screen.swap(tab);
      }
    }
  }
  // ---- 2. the gate
  if (ok && gate) {
    ok = launch(2, nullptr) && hipMemcpy(counts_s, dc, sizeof(counts_s), hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemset(dc, 0, sizeof(counts_s)) == hipSuccess && launch(1, nullptr) &&
         hipMemcpy(counts_b, dc, sizeof(counts_b), hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (dv) (void)hipFree(dv);
  if (dy) (void)hipFree(dy);
  if (dc) (void)hipFree(dc);
  if (da) (void)hipFree(da);
  if (!ok) { drop(); return; }
  if (!gate) return;
  bool any = false, changed = false;
  const double groups = kProbe / 32;
  for (WlScreen& s : img->host_screen) {
    if (!(s.cnst > 0.f) && !(s.cabs > 0.f)) continue;
    const double by_bound = counts_s[s.seg], by_both = counts_b[s.seg] > counts_s[s.seg] ? counts_b[s.seg] : counts_s[s.seg];
    const bool keep_bound = s.cnst > 0.f && by_bound >= kMinShare * groups;
    const double left = keep_bound ? groups - by_bound : groups, by_probe = keep_bound ? by_both - by_bound : by_both;
    const bool keep_probe = s.cabs > 0.f && left > 0.0 && by_probe >= kMinProbeShare * left;
    if (!keep_bound && s.cnst > 0.f) { s.cnst = 0.f; changed = true; }
    if (!keep_probe && s.cabs > 0.f) { s.cabs = 0.f; changed = true; }
    any = any || keep_bound || keep_probe;
  }
  if (!any) { drop(); return; }
  if (changed && hipMemcpy(img->wl_screen, img->host_screen.data(), img->host_screen.size() * sizeof(WlScreen), hipMemcpyHostToDevice) != hipSuccess)
    drop();
}

// called by rayen_pack_create (the only place that may touch function attributes)
int mfma_pair_wl_prepare(const RayenPack* p, PairImage* img) {
  if (img == nullptr || img->nkk < 1 || img->nkk > 2 || img->n_tiles <= 0 || !img->identity) return RAYEN_OK;
  const int lds = pair_wl_lds_bytes(img);
  if (lds > 160 * 1024) return RAYEN_OK;
  static std::mutex mu;
  static int promised = 0;      // (the attribute belongs to the kernel instance: every pack asks for the running maximum)
  std::lock_guard<std::mutex> hold(mu);
  promised = std::max(promised, lds);
  const int ask = promised;
  bool ok = true;
  auto want = [&](auto kern) {
    ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess;
  };
  want(mfma_pair_wl_kernel<1, false, kWlNT, kWlWaves>); want(mfma_pair_wl_kernel<1, true, kWlNT, kWlWaves>);
  want(mfma_pair_wl_kernel<2, false, kWlNT, kWlWaves>); want(mfma_pair_wl_kernel<2, true, kWlNT, kWlWaves>);
  if constexpr (kWlNT == 1) {      // the screening instances (same LDS)
    want(mfma_pair_wl_kernel<1, false, 1, kWlWaves, 0, true>); want(mfma_pair_wl_kernel<1, true, 1, kWlWaves, 0, true>);
    want(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 0, true>); want(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 0, true>);
  }
  // the instances of rayen_pair_drain(1)
  want(mfma_pair_wl_kernel<1, false, kWlNT, kWlWaves, 0, false, true>); want(mfma_pair_wl_kernel<1, true, kWlNT, kWlWaves, 0, false, true>);
  want(mfma_pair_wl_kernel<2, false, kWlNT, kWlWaves, 0, false, true>); want(mfma_pair_wl_kernel<2, true, kWlNT, kWlWaves, 0, false, true>);
  if constexpr (kWlNT == 1) {
    want(mfma_pair_wl_kernel<1, false, 1, kWlWaves, 0, true, true>); want(mfma_pair_wl_kernel<1, true, 1, kWlWaves, 0, true, true>);
    want(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 0, true, true>); want(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 0, true, true>);
  }
  if (!ok) return RAYEN_E_LAUNCH;
  img->wl_ready = true;
  // (RAYEN_PAIR_SCREEN_GATE=0 at pack creation: every qualifying segment stays decided -- tests and A/B runs)
  const char* gate_env = getenv("RAYEN_PAIR_SCREEN_GATE");
  if (kWlNT == 1 && img->wl_screen != nullptr) wl_screen_gate(p, img, !(gate_env != nullptr && gate_env[0] == '0'));
  // the mapped instances, for the widest mapper this pack can be given (in_dim = the padded width): attributes are set HERE, never
  // on a launch path; a pack whose image leaves no room for it keeps its mapped calls on rayen_mfma_pair.hip
  const int lds_m = pair_wl_lds_bytes_mapped(img, img->nkk);
  if (kWlNT == 1 && lds_m <= 160 * 1024) {
    static int promised_m = 0;
    promised_m = std::max(promised_m, lds_m);
    const int ask_m = promised_m;
    auto want_m = [&](auto kern) {
      ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, ask_m) == hipSuccess;
    };
    want_m(mfma_pair_wl_kernel<1, false, 1, kWlWaves, 1>); want_m(mfma_pair_wl_kernel<1, true, 1, kWlWaves, 1>);
    want_m(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 1>); want_m(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 1>);
    want_m(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 2>); want_m(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 2>);
    if (!ok) return RAYEN_E_LAUNCH;
    img->wl_mapped_ready = true;
  }
  return RAYEN_OK;
}

// ---- the module's mapper in front (rayen_ray_project_mapped_image_f32): x [B, in_dim] -> v = Wm x + b -> y, one launch
bool mfma_pair_wl_serves_mapped(const RayenPack* p, const PairImage* img, const float* x, int64_t B, int64_t ldx, int in_dim,
                                const float* v_out, int64_t ldvo, const float* y, int64_t ldy) {
  if (kWlNT != 1 || img == nullptr || img->nkk < 1 || img->nkk > 2 || img->n_tiles <= 0 || !img->wl_mapped_ready) return false;
  if (!img->identity || p->k != p->n || p->n > img->nkk * 32 || p->n <= (img->nkk - 1) * 32 || (p->n % 4) != 0) return false;
  if (in_dim < 4 || in_dim > img->nkk * 32 || (in_dim % 4) != 0 || ldx < in_dim || ldy < p->n) return false;
  if ((ldx % 4) != 0 || (ldy % 4) != 0 || ldx > (1 << 22) || ldy > (1 << 22)) return false;
  if (!base_aligned16(x) || !base_aligned16(y)) return false;
  if (v_out != nullptr && ((ldvo % 4) != 0 || ldvo < p->n || ldvo > (1 << 22) || !base_aligned16(v_out))) return false;
  if (img->nkk == 2 && img->aux_rows > WlGeom<2, true>::AUXR) return false;
  if (pair_wl_lds_bytes_mapped(img, (in_dim + 31) / 32) > 160 * 1024) return false;
  static const int64_t min_groups_env = [] { const char* e = getenv("RAYEN_WL_MIN_GROUPS"); return e ? atoll(e) : 1ll; }();   // developer sweeps
  return B >= 1 && (B + 31) / 32 >= min_groups_env;
}

int mfma_pair_wl_forward_mapped(const RayenPack* p, const PairImage* img, const float* x, int64_t B, int64_t ldx, int in_dim,
                                const void* image, float* v_out, int64_t ldvo, float* y, int64_t ldy, float* kappa,
                                int32_t* active, int32_t* nan_flag, hipStream_t stream) {
  if (B == 0) return RAYEN_OK;
  if (image == nullptr || !mfma_pair_wl_serves_mapped(p, img, x, B, ldx, in_dim, v_out, ldvo, y, ldy)) return RAYEN_E_UNSUPPORTED;
  const int nkx = (in_dim + 31) / 32;
  const int64_t cus = launch_simds(img->n_simd) / 4;
  const int lds = pair_wl_lds_bytes_mapped(img, nkx);
  const int64_t ld_max = std::max<int64_t>(std::max(std::max(ldx, ldy), v_out ? ldvo : 1), 1);
  const int64_t rows_max = (((int64_t)0xFFFFFFFFll / (ld_max * 4)) - 64) / 32 * 32;
  for (int64_t r0 = 0; r0 < B; r0 += rows_max) {
    const int64_t Bc = std::min(B - r0, rows_max);
    const int64_t n_groups = (Bc + 31) / 32;
    const unsigned grid = (unsigned)std::min<int64_t>(cus, n_groups);
    const float* xc = x + r0 * ldx;
    float* yc = y + r0 * ldy;
    float* voc = v_out ? v_out + r0 * ldvo : nullptr;
    float* kc = kappa ? kappa + r0 : nullptr;
    int32_t* ac = active ? active + 2 * r0 : nullptr;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(kWlWaves * 64), lds, stream, static_cast<const f16x8*>(img->Wh), img->items,
                         img->n_items, img->packs, img->y0, img->n_tiles, p->n, xc, Bc, ldx, yc, ldy, kc, ac, nan_flag,
                         img->w_scale, img->w_inv, static_cast<const f16x8*>(image), in_dim, voc, ldvo,
                         static_cast<const WlScreen*>(nullptr), static_cast<unsigned*>(nullptr), 0);
    };
    if (img->nkk == 1) {
      if (active != nullptr) go(mfma_pair_wl_kernel<1, true, 1, kWlWaves, 1>);
      else go(mfma_pair_wl_kernel<1, false, 1, kWlWaves, 1>);
    } else if (nkx == 1) {
      if (active != nullptr) go(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 1>);
      else go(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 1>);
    } else {
      if (active != nullptr) go(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 2>);
      else go(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 2>);
    }
  }
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

int mfma_pair_wl_forward(const RayenPack* p, const PairImage* img, const float* v, int64_t B, int64_t ldv,
                         float* y, int64_t ldy, float* kappa, int32_t* active, int32_t* nan_flag,
                         hipStream_t stream) {
  if (B == 0) return RAYEN_OK;
  if (!mfma_pair_wl_serves(p, img, v, B, ldv, y, ldy)) return RAYEN_E_UNSUPPORTED;
  const int64_t cus = launch_simds(img->n_simd) / 4;
  const int lds = pair_wl_lds_bytes(img);
  // The descriptors address 32-bit byte offsets, and the rows of a ragged last group beyond the batch must not wrap: a
  // batch whose rows span more than that goes out as several launches over whole groups (same groups, same bits).
  const int64_t ld_max = std::max<int64_t>(std::max(ldv, ldy), 1);
  const int64_t rows_max = (((int64_t)0xFFFFFFFFll / (ld_max * 4)) - 64) / (kWlNT * 32) * (kWlNT * 32);
  // screening (header): only where the image has a segment to screen; off by rayen_pair_screen(0) -- the instances of round 6
  // (mode 2: the spectral test alone, round 7's behaviour; the gate's launches choose for themselves)
  const int mode = wl_gate_counters != nullptr ? wl_gate_mode : pair_screen_cell().load(std::memory_order_relaxed);
  const bool screen = kWlNT == 1 && img->wl_screen != nullptr && mode != 0;
  const int probe_on = mode == 1 ? 1 : 0;
  unsigned* const counters = wl_gate_counters != nullptr ? wl_gate_counters : pair_screen_counters_cell().load(std::memory_order_relaxed);
  // (round 9: progress-ordered issue priority, rayen_pair_drain; the gate's launches run without it)
  const bool drain_on = wl_gate_counters == nullptr && pair_drain_cell().load(std::memory_order_relaxed) != 0;
  // (round 8: this schedule's own order of the list, where pack creation found one)
  const MItem* const items = img->wl_items != nullptr ? img->wl_items : img->items;
  for (int64_t r0 = 0; r0 < B; r0 += rows_max) {
    const int64_t Bc = std::min(B - r0, rows_max);
    const int64_t n_groups = (Bc + kWlNT * 32 - 1) / (kWlNT * 32);
    // one workgroup per CU; every CU takes part as soon as there is a group for it (a workgroup whose waves have no group of their own
    // to start with just leaves them idle: two busy waves on a SIMD run twice as fast as four)
    const unsigned grid = (unsigned)std::min<int64_t>(cus, n_groups);
    const float* vc = v + r0 * ldv;
    float* yc = y + r0 * ldy;
    float* kc = kappa ? kappa + r0 : nullptr;
    int32_t* ac = active ? active + 2 * r0 : nullptr;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(kWlWaves * 64), lds, stream, static_cast<const f16x8*>(img->Wh), items,
                         img->n_items, img->packs, img->y0, img->n_tiles, p->n, vc, Bc, ldv, yc, ldy, kc, ac, nan_flag,
                         img->w_scale, img->w_inv, static_cast<const f16x8*>(nullptr), 0, static_cast<float*>(nullptr), (int64_t)0,
                         screen ? img->wl_screen : nullptr, screen ? counters : nullptr, probe_on);
    };
    auto pick = [&](auto drain) {      // (the same eight instances with and without progress-ordered priority)
      constexpr bool D = decltype(drain)::value;
      if constexpr (kWlNT == 1) {
        if (screen) {
          if (img->nkk == 1) {
            if (active != nullptr) go(mfma_pair_wl_kernel<1, true, 1, kWlWaves, 0, true, D>);
            else go(mfma_pair_wl_kernel<1, false, 1, kWlWaves, 0, true, D>);
          } else {
            if (active != nullptr) go(mfma_pair_wl_kernel<2, true, 1, kWlWaves, 0, true, D>);
            else go(mfma_pair_wl_kernel<2, false, 1, kWlWaves, 0, true, D>);
          }
          return;
        }
      }
      if (img->nkk == 1) {
        if (active != nullptr) go(mfma_pair_wl_kernel<1, true, kWlNT, kWlWaves, 0, false, D>);
        else go(mfma_pair_wl_kernel<1, false, kWlNT, kWlWaves, 0, false, D>);
      } else {
        if (active != nullptr) go(mfma_pair_wl_kernel<2, true, kWlNT, kWlWaves, 0, false, D>);
        else go(mfma_pair_wl_kernel<2, false, kWlNT, kWlWaves, 0, false, D>);
      }
    };
    if (drain_on) pick(std::true_type{});
    else pick(std::false_type{});
  }
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace rayen
