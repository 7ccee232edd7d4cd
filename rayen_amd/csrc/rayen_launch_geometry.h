// Launch geometry of the persistent kernels, stated once.  Plain integers and pointers, no HIP type: any C++ compiler
// takes this header alone (tests/test_launch_geometry_host.py does).  The SIMD count callers pass comes from
// launch_simds() (rayen_internal.h), through which the reserved CUs enter.
#pragma once

#include <stdint.h>

namespace rayen {

// n_groups groups dealt over `slots` resident waves in equal rounds, `block_waves` waves per workgroup: the grid size.
// (slots = launch_simds(n_simd) * waves per SIMD; the W-stationary kernel: slots = CUs, one "wave" = one workgroup)
inline int64_t grid_for_groups(const int64_t n_groups, const int64_t slots, const int block_waves) {
  const int64_t rounds = (n_groups + slots - 1) / slots;
  const int64_t waves = (n_groups + rounds - 1) / rounds;
  return (waves + block_waves - 1) / block_waves;
}
// the same for a batch of B > 0 rows in groups of `per_wave`
inline int64_t persistent_grid(const int64_t B, const int per_wave, const int64_t slots, const int block_waves) {
  return grid_for_groups((B + per_wave - 1) / per_wave, slots, block_waves);
}
inline bool base_aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }
// rows of `ld` 4-byte words behind `ptr` all start on 16-byte boundaries (the kernels' vec_in / vec_out: 16-byte pieces of
// a row).  `ld` counts floats; rows of doubles pass twice their leading dimension (rayen_bar.hip::ld_words).
inline bool rows_aligned16(const void* ptr, const int64_t ld) { return (ld % 4 == 0) && base_aligned16(ptr); }

}  // namespace rayen
