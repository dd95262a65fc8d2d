// Helpers of the image stage (nuclei.hip, label.hip, edt.hip, geodesic.hip, reconstruct.hip, watershed.hip, and through
// image_window.hpp window.hip, morph.hip, rank.hip): the argument rules these
// files share, the one reader of "is this pixel zero", and the carver that lays out their workspaces.  Each stage has ONE layout function that uses up a Carver and fills the stage's pointer struct;
// its *_ws_bytes entry point runs that function on a counting carver (layout_bytes) and its launchers run it on the caller's buffer,
// so a size and the offsets behind it cannot drift apart.
#pragma once
#include <stdint.h>

#include <utility>

constexpr int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }      // b >= 0; every workspace piece starts on such a boundary
static inline bool bad_image_dims(int H, int W) { return H < 0 || W < 0 || (int64_t)H * W >= ((int64_t)1 << 31); }      // raster indices fit int32
static inline bool bad_elem_bytes(int bytes) { return bytes != 1 && bytes != 2 && bytes != 4 && bytes != 8; }      // images are read as integers
// The step costs of geodesic.hip and watershed.hip: 1 <= a <= b <= 2a or b == 0, and no path cost overflows int32.
static inline bool bad_step_costs(int H, int W, int a, int b) {
  if (a < 1 || (b != 0 && (b < a || (int64_t)b > 2 * (int64_t)a))) return true;
  return (int64_t)(b != 0 ? b : a) * H * W >= ((int64_t)1 << 31);
}
static inline bool bad_connectivity(int connectivity) { return connectivity != 1 && connectivity != 2; }
// A batch of launches first .. first + count - 1 (tile_relax.hpp): at least one, and first + count + 1 fits int32 (a round stamps r + 1).
static inline bool bad_launch_range(int first, int count) { return first < 0 || count < 1 || first > 0x7fffffff - count - 1; }

__device__ __forceinline__ bool image_nonzero(const void* img, int bytes, int64_t i) {     // `bytes` is uniform
  switch (bytes) {
    case 1: return static_cast<const uint8_t*>(img)[i] != 0;
    case 2: return static_cast<const uint16_t*>(img)[i] != 0;
    case 4: return static_cast<const uint32_t*>(img)[i] != 0;
    default: return static_cast<const uint64_t*>(img)[i] != 0;
  }
}

// Bump allocation over one buffer.  Without a base it only counts: take() returns null and `used` ends as the bytes the layout needs.
struct Carver {
  char* base;
  int64_t used = 0;
  explicit Carver(void* ws = nullptr) : base(static_cast<char*>(ws)) {}
  template <typename T>
  T* take(int64_t count) {
    T* piece = base != nullptr ? reinterpret_cast<T*>(base + used) : nullptr;
    used += align256(count * (int64_t)sizeof(T));
    return piece;
  }
};

template <typename Ws, typename... A>
int64_t layout_bytes(Ws (*layout)(Carver&&, A...), A... a) {
  Carver c;
  layout(std::move(c), a...);      // a layout only calls c.take(): c still holds the count
  return c.used;
}
