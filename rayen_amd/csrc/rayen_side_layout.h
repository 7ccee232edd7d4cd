// What the side layers (Bar, DC3, Euclidean projection, soft cost) share that needs no HIP type, stated once: the LDS
// budget, the run-time width -> kernel-instance dispatch, and the layout of their scratch buffers.  Plain integers and
// pointers: any C++ compiler takes this header alone (tests/test_side_layout_host.py does).  The HIP half -- device checks,
// the dynamic-LDS opt-in -- is rayen_side_pack.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "rayen_hip.h"

namespace rayen {

constexpr size_t kLdsBudget = 160 * 1024;      // gfx950 LDS per CU: the most a workgroup's image may take
constexpr size_t kLdsNoOptIn = 48 * 1024;      // dynamic LDS a kernel may ask for without allow_lds() (rayen_side_pack.h)

inline size_t align256(const size_t x) { return (x + 255) & ~(size_t)255; }

// the power of two in [LO, HI] a width of `w` >= 1 columns is padded to (what a kernel instance keeps in registers);
// 0 beyond HI
template <int LO, int HI>
inline int padded_width(const int w) {
  for (int K = LO; K <= HI; K *= 2)
    if (w <= K) return K;
  return 0;
}

// run-time padded width -> the kernel instance: f(std::integral_constant<int, K>) for the power of two K in [LO, HI],
// whose answer is handed on; any other width answers RAYEN_E_UNSUPPORTED.  Every K in the range is instantiated: a callee
// that has no instance at some K says so itself (if constexpr), as rayen_dc3.hip does for fp64 at 64.
template <int LO, int HI, typename F>
inline int dispatch_width(const int K, F&& f) {
  static_assert(LO > 0 && (LO & (LO - 1)) == 0 && (HI & (HI - 1)) == 0, "powers of two");
  if constexpr (LO > HI) {
    return RAYEN_E_UNSUPPORTED;
  } else {
    if (K == LO) return f(std::integral_constant<int, LO>());
    return dispatch_width<2 * LO, HI>(K, f);
  }
}

// A scratch buffer cut into N regions, each `elem` x `count` bytes rounded up to whole 256-byte lines.  The size a layer
// reports (`total`) and the pointers it hands its kernels (`at`) come from the same list, so they cannot drift apart.
struct WsRegion {
  size_t elem, count;
};

template <int N>
struct WsLayout {
  size_t offset[N], bytes[N], total;
  // region i of the buffer at `ws`; null for a region the call does not use (count 0)
  template <typename T>
  T* at(void* ws, const int i) const {
    return bytes[i] ? reinterpret_cast<T*>(static_cast<unsigned char*>(ws) + offset[i]) : nullptr;
  }
};

template <int N>
inline WsLayout<N> ws_layout(const WsRegion (&regions)[N]) {
  WsLayout<N> l;
  l.total = 0;
  for (int i = 0; i < N; ++i) {
    l.offset[i] = l.total;
    l.bytes[i] = align256(regions[i].elem * regions[i].count);
    l.total += l.bytes[i];
  }
  return l;
}

// ---- the layers' scratch buffers (B rows of `elem`-byte numbers)

// DC3 forward: viol [max_steps + 1] slots wide enough for the bits of a double | with more than one launch of steps
// (`chunks`), (p, s) [2 n][B] twice: the launches ping-pong between them
enum { kDc3Viol = 0, kDc3State0 = 1, kDc3State1 = 2 };
inline WsLayout<3> dc3_forward_ws(const int n, const int64_t B, const int max_steps, const int chunks, const size_t elem) {
  const size_t state = chunks > 1 ? (size_t)2 * n * (size_t)B : 0;
  return ws_layout<3>({{8, (size_t)(max_steps + 1)}, {elem, state}, {elem, state}});
}

// DC3 backward: the recomputed trajectory [max_steps][n][B]
inline WsLayout<1> dc3_backward_ws(const int n, const int64_t B, const int max_steps, const size_t elem) {
  return ws_layout<1>({{elem, (size_t)max_steps * n * (size_t)B}});
}

// projection: x [B][n] and status [B] between launches | the backward's own v [B][m]
enum { kProjXs = 0, kProjStatus = 1, kProjDvs = 2 };
inline WsLayout<3> proj_ws(const int n, const int m, const int64_t B, const bool backward, const size_t elem) {
  return ws_layout<3>({{elem, (size_t)B * n}, {sizeof(int32_t), (size_t)B}, {elem, backward ? (size_t)B * m : 0}});
}

}  // namespace rayen
