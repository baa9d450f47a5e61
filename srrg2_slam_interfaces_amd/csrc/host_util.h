// host_util.h -- small host-side helpers shared by the drivers (error slot, HIP error check, device buffer)
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/srrg2_slam_amd.h"

namespace srrg2amd {

extern thread_local std::string g_err;
int fail(int code, const std::string& msg);

// hipFree under a name of this library's: device memory is freed here and nowhere else
inline hipError_t device_free(void* p) { return hipFree(p); }

// Device memory that frees itself.  A handle's buffers are members of this type and nothing else: the handle's destructor
// quiesces its streams in its body, the members free themselves after it.  Move-only; never at namespace or static scope
// (nothing may be freed after the HIP runtime has shut down).
template <typename T>
struct DevBuf {
  T* p          = nullptr;
  size_t cap    = 0;      // elements
  bool borrowed = false;  // p belongs to another DevBuf (a slice that shares the clouds of another slice)
  DevBuf() = default;
  DevBuf(const DevBuf&)            = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.forget(); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap, borrowed = o.borrowed;
      o.forget();
    }
    return *this;
  }
  ~DevBuf() { release(); }
  // view of another buffer: no ownership; the lender must outlive the use (re-borrowed at every compute())
  void borrow(const DevBuf<T>& o) {
    release();
    p        = o.p;
    cap      = o.cap;
    borrowed = o.p != nullptr;
  }
  int reserve(size_t n) {
    if (borrowed) forget();
    if (n <= cap) return 0;
    release();
    size_t want = n + n / 8 + 16;
    hipError_t e = hipMalloc((void**) &p, want * sizeof(T));
    if (e != hipSuccess) return fail(SRRG2_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    cap = want;
    return 0;
  }
  // reserve(want) that keeps the first `keep` elements: a new block, the copy queued on `stream` and waited for, then the old
  // block is freed and the new one adopted.  An error leaves the buffer as it was (the new block frees itself).
  int grow(size_t want, size_t keep, hipStream_t stream) {
    if (want <= cap) return 0;
    DevBuf<T> nb;
    int rc;
    if ((rc = nb.reserve(want))) return rc;
    if (keep > 0 && p) {
      hipError_t e = hipMemcpyAsync(nb.p, p, sizeof(T) * keep, hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return fail(SRRG2_E_HIP, std::string("grow: ") + hipGetErrorString(e));
    }
    *this = std::move(nb);
    return 0;
  }
  void release() {
    if (p && !borrowed) (void) device_free(p);
    forget();
  }

 private:
  void forget() {
    p        = nullptr;
    cap      = 0;
    borrowed = false;
  }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value, "a DevBuf has one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value, "handles move their buffers");

// Pinned host memory that frees itself: the host mirror of a DevBuf.  reserve(n, slack) gives room for n elements, n + slack
// when it has to allocate (the content is dropped).  Move-only, never at namespace or static scope.
template <typename T>
struct PinnedBuf {
  T* p       = nullptr;
  size_t cap = 0;  // elements
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&)            = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  int reserve(size_t n, size_t slack = 0) {
    if (n <= cap) return 0;
    release();
    hipError_t e = hipHostMalloc((void**) &p, (n + slack) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return fail(SRRG2_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    cap = n + slack;
    return 0;
  }
  void release() {
    if (p) (void) hipHostFree(p);
    p   = nullptr;
    cap = 0;
  }
};
static_assert(!std::is_copy_constructible<PinnedBuf<int>>::value, "a PinnedBuf has one owner");
static_assert(std::is_nothrow_move_constructible<PinnedBuf<int>>::value, "handles move their buffers");

// what scene.hip needs to see of an aligner slice after compute() (device pointers into the aligner's buffers)
struct AlignerSliceView {
  const float4* moving_sorted;  // .w = caller's index (= index in the cloud given to set_moving)
  const int* corr_fixed;        // per sorted moving point: matched fixed index or -1
  const float* corr_resp;
  const unsigned char* corr_stat;
  int nm, nf;
  bool prune;  // keep_only_inlier_correspondences && Success: only inlier correspondences count
  int device;
  void* ready_event;  // hipEvent_t recorded on the aligner's stream behind the kernels that wrote the arrays: wait for it on the
                      // consuming stream (hipStreamWaitEvent) before reading them
};
int aligner_slice_view(srrg2_aligner_s* a, int slice_idx, AlignerSliceView* v);

// what descriptors.hip needs to see of a scene: the points (validity), the descriptors (null: the scene has none), its stream
struct SceneFeatureView {
  const float4* pts;
  const uint4* desc;  // two per point
  int n, dim, device;
  hipStream_t stream;
};
int scene_feature_view(srrg2_scene* s, SceneFeatureView* v);

}  // namespace srrg2amd

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      return srrg2amd::fail(SRRG2_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    }                                                                                              \
  } while (0)
