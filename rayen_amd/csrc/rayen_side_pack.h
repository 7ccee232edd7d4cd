// Host code the side layers' packs share (RayenBarPack, RayenDc3Pack, RayenProjPack, RayenCostPack: an fp32 and an fp64
// LDS image on one device behind typed entry points).  Plain functions and one scope guard; the packs stay plain structs
// of their own.  What needs no HIP type is in rayen_side_layout.h; DESIGN.md ("host code shared by the side layers") has
// the steps to add a layer with both.
#pragma once

#include <cstring>

#include "rayen_internal.h"
#include "rayen_side_layout.h"

namespace rayen {

// pack creation: the current device and, for the layers whose grids depend on it, its CU count (`fallback_cus` where the
// runtime reports none).  RAYEN_E_NO_DEVICE without a device or on anything but gfx950.
inline int side_pack_device(int* device, int* cus = nullptr, const int fallback_cus = 0) {
  hipDeviceProp_t prop;
  if (hipGetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, *device) != hipSuccess ||
      std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return RAYEN_E_NO_DEVICE;
  if (cus != nullptr) *cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : fallback_cus;
  return RAYEN_OK;
}

// a call: the pack's device must be the current one
inline int check_device(const int device) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return RAYEN_E_NO_DEVICE;
  return dev == device ? RAYEN_OK : RAYEN_E_DEVICE_MISMATCH;
}

// *_pack_destroy: the pack's device is current inside the scope (hipFree of its images), the caller's again after it
class DeviceScope {
 public:
  explicit DeviceScope(const int device) {
    switched_ = hipGetDevice(&prev_) == hipSuccess && prev_ != device && hipSetDevice(device) == hipSuccess;
  }
  ~DeviceScope() {
    if (switched_) (void)hipSetDevice(prev_);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;

 private:
  int prev_ = -1;
  bool switched_ = false;
};

// may `kern` be launched with `lds` bytes of dynamic LDS?  Beyond kLdsNoOptIn the kernel has to opt in; where that fails
// the runtime's sticky error is cleared (or the runtime's next caller finds this error waiting for it).
template <typename Kern>
inline bool allow_lds(Kern kern, const size_t lds) {
  if (lds <= kLdsNoOptIn) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==
      hipSuccess)
    return true;
  (void)hipGetLastError();
  return false;
}

// an image: host vector -> fresh device allocation (upload_to_device without the byte count)
template <typename T>
inline bool upload_image(const std::vector<T>& host, T** dev) {
  int64_t bytes = 0;
  return upload_to_device(host, dev, &bytes);
}

}  // namespace rayen
