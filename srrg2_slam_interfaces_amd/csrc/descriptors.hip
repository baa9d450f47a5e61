// descriptors.hip -- device-resident database of 256-bit binary descriptors with exact matching: the matching half of
// MultiLoopDetectorHBST_ (S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp), behind the
// srrg2_descriptor_db_* entry points of include/srrg2_slam_amd.h.
//
// The reference matches through srrg_hbst::BinaryTree256 (multi_loop_detector_hbst.h:40-44).  Here the tree has one
// leaf: every query descriptor is compared with every database descriptor of every map that passes the age gate.
//   addPreviousQuery                    :41-70   srrg2_descriptor_db_add: valid descriptors appended as one map
//   computeCorrespondences              :72-161  srrg2_descriptor_db_match: k_desc_match + k_desc_map_stats
//   _computeCorrespondencesFromMatches  :163-197 k_desc_emit (per reference descriptor the best query)
// Three kernels per match():
//   k_desc_match      one thread per DPT database descriptors held in VGPRs; the valid query descriptors are staged in
//                     LDS in tiles of TILE and read as broadcasts.  Per pair: 8 xor + 8 bcnt, one compare + increment
//                     of the thread's pair count, one min of the key (distance << 23 | query slot).  The minimum key is
//                     the deduplication rule of :176-182 (smallest distance, then the first query in point order: the
//                     slots ascend with the point index).  No atomics: each descriptor's key and count are written once.
//   k_desc_map_stats  one workgroup per searched map: the sum of its descriptors' counts (int64; the reference's
//                     number_of_matches before deduplication) and the number of descriptors whose best query matches.
//   k_desc_emit       one workgroup per candidate map: a stable compaction of its matched descriptors into the
//                     correspondences, ascending in the reference point index.
// The host reads the per-map statistics once, picks the candidates (count gate, :152-154) and reads the
// correspondences once.
// A scene that carries descriptors (srrg2_scene_set_features) is added / matched without its descriptors leaving the
// device (the reference reads them from the local map's cloud: :84-85, :131-136): k_scene_flag marks the Valid points,
// an exclusive scan numbers them, k_scene_stage scatters descriptors and point indices -- ascending point index, the
// order stage() produces on the host -- into the database tail (add) or the query buffers (match); one count crosses to
// the host.  The three kernels above then run unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_types.h"
#include "host_util.h"
#include "kernels.h"

using srrg2amd::DevBuf;
using srrg2amd::fail;

namespace {

constexpr int THREADS     = 256;
constexpr int DPT         = 4;     // database descriptors per thread (amortise each LDS read of a query over DPT pairs)
constexpr int TILE        = 1024;  // query descriptors per LDS tile: 32 KiB
constexpr int SLOT_BITS   = 23;    // key = distance (0 .. 256: 9 bits) << 23 | query slot
constexpr uint32_t SLOT_MASK = (1u << SLOT_BITS) - 1;
constexpr int MAX_QUERY   = 1 << SLOT_BITS;

struct MapStat {
  long long count;  // matching pairs before deduplication
  long long kept;   // descriptors whose best query matches (= correspondences after deduplication)
};

struct Candidate {
  long long begin, end;  // descriptor range of the map in the database
  long long out;         // offset of its first correspondence
};

// v_bcnt_u32_b32 d, x, acc = popcount(x) + acc.  Written as asm so that the compiler keeps the accumulating form: from
// __builtin_popcount(x) + acc it builds a tree of bcnt-with-0 and v_add3_u32 (3 extra VALU per pair).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

__device__ __forceinline__ uint32_t hamming(const uint32_t (&a)[8], const uint4 x, const uint4 y) {
  uint32_t d = __builtin_popcount(a[0] ^ x.x);
  d          = bcnt_acc(a[1] ^ x.y, d);
  d          = bcnt_acc(a[2] ^ x.z, d);
  d          = bcnt_acc(a[3] ^ x.w, d);
  d          = bcnt_acc(a[4] ^ y.x, d);
  d          = bcnt_acc(a[5] ^ y.y, d);
  d          = bcnt_acc(a[6] ^ y.z, d);
  d          = bcnt_acc(a[7] ^ y.w, d);
  return d;
}

// Database descriptors [0, lo) and [lo + skip, ...) are searched (the maps between fail the age gate): nactive of them.
// db / query: two uint4 per descriptor.  L: a distance d matches iff d < L.
__global__ void __launch_bounds__(THREADS) k_desc_match(const uint4* __restrict__ db, long long lo, long long skip,
                                                        long long nactive, const uint4* __restrict__ query, int nq,
                                                        uint32_t L, uint32_t* __restrict__ best,
                                                        uint32_t* __restrict__ count) {
  __shared__ uint4 tile[2 * TILE];
  uint32_t a[DPT][8];
  long long j[DPT];
  uint32_t key[DPT], cnt[DPT];
  const long long base = (long long) blockIdx.x * (THREADS * DPT) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < DPT; ++k) {
    const long long g = base + (long long) k * THREADS;
    j[k]              = g < lo ? g : g + skip;
    uint4 x = make_uint4(0, 0, 0, 0), y = x;
    if (g < nactive) {
      x = db[2 * j[k]];
      y = db[2 * j[k] + 1];
    }
    a[k][0] = x.x; a[k][1] = x.y; a[k][2] = x.z; a[k][3] = x.w;
    a[k][4] = y.x; a[k][5] = y.y; a[k][6] = y.z; a[k][7] = y.w;
    key[k] = 0xffffffffu;
    cnt[k] = 0;
  }
  for (int t0 = 0; t0 < nq; t0 += TILE) {
    const int nt = min(TILE, nq - t0);
    __syncthreads();  // (the previous tile is no longer read)
    for (int i = threadIdx.x; i < 2 * nt; i += THREADS) tile[i] = query[2 * (long long) t0 + i];
    __syncthreads();
    for (int qi = 0; qi < nt; ++qi) {
      const uint4 x = tile[2 * qi], y = tile[2 * qi + 1];  // same address in every lane: broadcast
      const uint32_t slot = (uint32_t) (t0 + qi);
#pragma unroll
      for (int k = 0; k < DPT; ++k) {
        const uint32_t d = hamming(a[k], x, y);
        cnt[k] += d < L ? 1u : 0u;
        key[k] = min(key[k], (d << SLOT_BITS) | slot);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DPT; ++k) {
    if (base + (long long) k * THREADS < nactive) {
      best[j[k]]  = key[k];
      count[j[k]] = cnt[k];
    }
  }
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();  // (red is reused by the next call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Workgroup b -> map b (b < map_lo) or b + map_skip; map r holds descriptors [starts[r], starts[r + 1]).
__global__ void __launch_bounds__(THREADS) k_desc_map_stats(const long long* __restrict__ starts, int map_lo, int map_skip,
                                                            const uint32_t* __restrict__ best,
                                                            const uint32_t* __restrict__ count, uint32_t L,
                                                            MapStat* __restrict__ stats) {
  __shared__ long long red_c[THREADS / 64];
  __shared__ long long red_k[THREADS / 64];
  const int r = (int) blockIdx.x < map_lo ? (int) blockIdx.x : (int) blockIdx.x + map_skip;
  const long long b = starts[r], e = starts[r + 1];
  long long c = 0, kept = 0;
  for (long long i = b + threadIdx.x; i < e; i += THREADS) {
    c += count[i];
    kept += (best[i] >> SLOT_BITS) < L ? 1 : 0;
  }
  c    = block_sum(c, red_c);
  kept = block_sum(kept, red_k);
  if (threadIdx.x == 0) stats[r] = MapStat{c, kept};
}

// Workgroup k compacts candidate k: its matched descriptors in database order (= reference point order).
__global__ void __launch_bounds__(THREADS) k_desc_emit(const Candidate* __restrict__ cands,
                                                       const uint32_t* __restrict__ best,
                                                       const int32_t* __restrict__ ref_idx,
                                                       const int32_t* __restrict__ query_idx, uint32_t L,
                                                       srrg2_correspondence* __restrict__ out) {
  __shared__ int wave_n[THREADS / 64];
  const Candidate c = cands[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long o = c.out;
  for (long long b = c.begin; b < c.end; b += THREADS) {
    const long long i = b + threadIdx.x;
    uint32_t k        = 0xffffffffu;
    if (i < c.end) k = best[i];
    const bool keep         = (k >> SLOT_BITS) < L;
    const unsigned long long m = __ballot(keep);
    const int before        = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();  // (wave_n of the previous chunk has been read)
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wave_n[w];
    if (keep) {
      srrg2_correspondence r;
      r.fixed_idx      = query_idx[k & SLOT_MASK];
      r.moving_idx     = ref_idx[i];
      r.response       = (float) (k >> SLOT_BITS);
      out[o + wbase + before] = r;
    }
    o += (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
  }
}

// ---- staging from a scene ---------------------------------------------------------------------------------------------
// Valid <=> finite coordinates (scene.hip's valid_point)
__global__ void k_scene_flag(int dim, const float4* __restrict__ pts, int n, int* __restrict__ flags) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    flags[i]       = (isfinite(p.x) && isfinite(p.y) && (dim == 2 || isfinite(p.z))) ? 1 : 0;
  }
}

// offset: the exclusive scan of the flags (offset[n] is not read: a point is valid iff its coordinates are, tested again)
__global__ void k_scene_stage(int dim, const float4* __restrict__ pts, const uint4* __restrict__ desc, int n,
                              const int* __restrict__ offset, int cap, uint4* __restrict__ out_desc,
                              int32_t* __restrict__ out_idx) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && (dim == 2 || isfinite(p.z)))) continue;
    const int k = offset[i];
    if (k >= cap) continue;  // (cannot happen: cap is the scan's total; a guard against writing past the buffers)
    const uint4 a = desc[2 * (size_t) i], b = desc[2 * (size_t) i + 1];
    out_desc[2 * (size_t) k]     = a;
    out_desc[2 * (size_t) k + 1] = b;
    out_idx[k]                   = i;
  }
}

// a device buffer that keeps its first `used` elements when it grows: the capacity doubles, from 1024 on
template <typename T>
int grow_keep(DevBuf<T>& buf, size_t need, size_t used, hipStream_t s) {
  if (need <= buf.cap) return 0;
  return buf.grow(std::max<size_t>(buf.cap * 2, std::max<size_t>(need, 1024)), used, s);
}

// pinned host staging that grows by half, from 4096 bytes on
int host_reserve(srrg2amd::PinnedBuf<char>& buf, size_t bytes) {
  return buf.reserve(bytes, std::max<size_t>(bytes + bytes / 2, 4096) - bytes);
}

// d < t for an integer distance d in 0 .. 256  <=>  d < L
uint32_t distance_limit(float t) {
  if (!(t > 0.f)) return 0;
  if (t > 256.f) return 257;
  return (uint32_t) std::ceil(t);
}

}  // namespace

struct srrg2_descriptor_db {
  int device         = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // database: descriptors (two uint4 each), the point index of each in its map, per-map descriptor ranges
  DevBuf<uint4> desc;
  DevBuf<int32_t> ref_idx;
  DevBuf<long long> starts;             // device copy of h_starts
  std::vector<long long> h_starts{0};  // h_starts[r] .. h_starts[r + 1]: map r
  // per-match scratch
  DevBuf<uint32_t> best, count;
  DevBuf<uint4> query;
  DevBuf<int32_t> query_idx;
  DevBuf<MapStat> stats;
  DevBuf<Candidate> cands;
  DevBuf<srrg2_correspondence> corr;
  srrg2amd::PinnedBuf<char> staging;
  // staging from a scene: flags -> offsets, the scan's block sums, the event that orders this stream behind the scene's
  DevBuf<int> sflags, sscan;
  hipEvent_t ev_scene = nullptr;
  // last match()
  std::vector<MapStat> h_stats;
  std::vector<int64_t> map_counts;
  std::vector<int32_t> cand_ref;
  std::vector<int64_t> cand_count, cand_off{0};
  std::vector<srrg2_correspondence> h_corr;
  double last_ms = 0.0;
  // The ordering is what this destructor is for: the stream retires before any buffer above is freed (the members free
  // themselves after this body).
  ~srrg2_descriptor_db() {
    (void) hipSetDevice(device);
    if (stream) (void) hipStreamSynchronize(stream);
    for (hipEvent_t ev : {ev_scene, ev0, ev1})
      if (ev) (void) hipEventDestroy(ev);
    if (stream) (void) hipStreamDestroy(stream);
  }
};

namespace {

int db_device(srrg2_descriptor_db* h) {
  HIP_TRY(hipSetDevice(h->device));
  return 0;
}

// valid descriptors -> staging: nv rows of 32 bytes, then nv int32 point indices (at a 16-byte aligned offset)
int stage(srrg2_descriptor_db* h, const uint8_t* d, const uint8_t* valid, int n, int* nv_out, size_t* idx_off) {
  int nv = 0;
  for (int i = 0; i < n; ++i) nv += (!valid || valid[i]) ? 1 : 0;
  const size_t off = ((size_t) nv * SRRG2_DESCRIPTOR_BYTES + 15) / 16 * 16;
  int rc;
  if ((rc = host_reserve(h->staging, off + (size_t) nv * 4 + 16))) return rc;
  uint8_t* rows  = (uint8_t*) h->staging.p;
  int32_t* idx   = (int32_t*) (rows + off);
  int k          = 0;
  for (int i = 0; i < n; ++i) {
    if (valid && !valid[i]) continue;
    std::memcpy(rows + (size_t) k * SRRG2_DESCRIPTOR_BYTES, d + (size_t) i * SRRG2_DESCRIPTOR_BYTES, SRRG2_DESCRIPTOR_BYTES);
    idx[k++] = i;
  }
  *nv_out  = nv;
  *idx_off = off;
  return 0;
}

int scene_blocks(int n) {
  int b = (n + THREADS - 1) / THREADS;
  return b < 1 ? 1 : (b > 2048 ? 2048 : b);
}

// the checks shared by add_scene / match_scene
int scene_view(srrg2_descriptor_db* h, srrg2_scene_h scene, const char* who, srrg2amd::SceneFeatureView* v) {
  if (!h || !scene) return fail(SRRG2_E_INVALID, std::string(who) + ": NULL handle");
  int rc;
  if ((rc = srrg2amd::scene_feature_view(scene, v))) return rc;
  if (v->device != h->device) return fail(SRRG2_E_INVALID, std::string(who) + ": the scene lives on another device");
  if (!v->desc) return fail(SRRG2_E_STATE, std::string(who) + ": the scene carries no descriptors (srrg2_scene_set_features)");
  if (v->n > MAX_QUERY) return fail(SRRG2_E_INVALID, std::string(who) + ": a scene holds at most 2^23 points here");
  return 0;
}

// number the Valid points of the scene: h->sflags = exclusive scan of the flags, *nv_out = their count (one pinned int).
// The database's stream first waits for what is queued on the scene's.
int scene_count(srrg2_descriptor_db* h, const srrg2amd::SceneFeatureView& v, int* nv_out) {
  *nv_out = 0;
  if (v.n == 0) return 0;
  int rc;
  if (!h->ev_scene) HIP_TRY(hipEventCreateWithFlags(&h->ev_scene, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->ev_scene, v.stream));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_scene, 0));
  if ((rc = h->sflags.reserve((size_t) v.n + 1))) return rc;
  if ((rc = h->sscan.reserve((size_t) srrg2amd::scan_num_blocks(v.n) + 2))) return rc;
  if ((rc = host_reserve(h->staging, 64))) return rc;
  hipLaunchKernelGGL(k_scene_flag, dim3(scene_blocks(v.n)), dim3(THREADS), 0, h->stream, v.dim, v.pts, v.n, h->sflags.p);
  int* dtotal = h->sscan.p + h->sscan.cap - 1;
  srrg2amd::launch_exclusive_scan(h->sflags.p, v.n, h->sscan.p, dtotal, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->staging.p, dtotal, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *nv_out = *(const int*) h->staging.p;
  return 0;
}

void scene_scatter(srrg2_descriptor_db* h, const srrg2amd::SceneFeatureView& v, int nv, uint4* out_desc, int32_t* out_idx) {
  hipLaunchKernelGGL(k_scene_stage, dim3(scene_blocks(v.n)), dim3(THREADS), 0, h->stream, v.dim, v.pts, v.desc, v.n,
                     h->sflags.p, nv, out_desc, out_idx);
}

}  // namespace

int srrg2_descriptor_db_create(int device, srrg2_descriptor_db_h* out) {
  if (!out) return fail(SRRG2_E_INVALID, "descriptor_db_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "descriptor_db_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "descriptor_db_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<srrg2_descriptor_db> h(new srrg2_descriptor_db());  // (a failure below deletes it)
  h->device = device;
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&h->ev0));
  HIP_TRY(hipEventCreate(&h->ev1));
  int rc;
  if ((rc = grow_keep(h->starts, 1024, 0, h->stream))) return rc;
  HIP_TRY(hipMemsetAsync(h->starts.p, 0, sizeof(long long), h->stream));
  *out = h.release();
  return 0;
}

int srrg2_descriptor_db_destroy(srrg2_descriptor_db_h h) {
  delete h;  // (null: nothing to do)
  return 0;
}

namespace {

// add() behind the argument checks.  sv: the descriptors come from a scene on the device, else from d / valid on the host
int add_impl(srrg2_descriptor_db* h, const uint8_t* d, const uint8_t* valid, int n, const srrg2amd::SceneFeatureView* sv,
             int* index_out) {
  int rc;
  if ((rc = db_device(h))) return rc;
  if (index_out) *index_out = -1;
  int nv       = 0;
  size_t off   = 0;
  if (sv) {
    if ((rc = scene_count(h, *sv, &nv))) return rc;
  } else if ((rc = stage(h, d, valid, n, &nv, &off))) {
    return rc;
  }
  if (nv == 0) return 0;  // addPreviousQuery skips an empty request (:46-49)
  const int maps      = (int) h->h_starts.size() - 1;
  const long long old = h->h_starts.back(), now = old + nv;
  if ((rc = grow_keep(h->desc, (size_t) now * 2, (size_t) old * 2, h->stream))) return rc;
  if ((rc = grow_keep(h->ref_idx, (size_t) now, (size_t) old, h->stream))) return rc;
  if ((rc = grow_keep(h->starts, (size_t) maps + 2, (size_t) maps + 1, h->stream))) return rc;
  h->h_starts.push_back(now);
  if (sv) {
    scene_scatter(h, *sv, nv, h->desc.p + 2 * old, h->ref_idx.p + old);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(h->desc.p + 2 * old, h->staging.p, (size_t) nv * SRRG2_DESCRIPTOR_BYTES, hipMemcpyHostToDevice,
                           h->stream));
    HIP_TRY(hipMemcpyAsync(h->ref_idx.p + old, (uint8_t*) h->staging.p + off, (size_t) nv * 4, hipMemcpyHostToDevice,
                           h->stream));
  }
  HIP_TRY(hipMemcpyAsync(h->starts.p + maps + 1, &h->h_starts.back(), sizeof(long long), hipMemcpyHostToDevice,
                         h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (the staging buffer is reused by the next call; a scene is no longer read)
  if (index_out) *index_out = maps;
  return 0;
}

}  // namespace

int srrg2_descriptor_db_add(srrg2_descriptor_db_h h, const uint8_t* d, const uint8_t* valid, int n, int* index_out) {
  if (!h || n < 0 || (n > 0 && !d)) return fail(SRRG2_E_INVALID, "descriptor_db_add: bad arguments");
  return add_impl(h, d, valid, n, nullptr, index_out);
}

int srrg2_descriptor_db_add_scene(srrg2_descriptor_db_h h, srrg2_scene_h scene, int* index_out) {
  srrg2amd::SceneFeatureView v;
  int rc;
  if ((rc = scene_view(h, scene, "descriptor_db_add_scene", &v))) return rc;
  return add_impl(h, nullptr, nullptr, v.n, &v, index_out);
}

int srrg2_descriptor_db_size(srrg2_descriptor_db_h h, int* maps, int64_t* descriptors) {
  if (!h) return fail(SRRG2_E_INVALID, "descriptor_db_size: NULL handle");
  if (maps) *maps = (int) h->h_starts.size() - 1;
  if (descriptors) *descriptors = h->h_starts.back();
  return 0;
}

namespace {

// match() behind the argument checks; sv as in add_impl
int match_impl(srrg2_descriptor_db* h, const uint8_t* d, const uint8_t* valid, int n, const srrg2amd::SceneFeatureView* sv,
               int64_t query_index, float max_distance, uint32_t min_age, int64_t min_matches, int* K_out) {
  int rc;
  if ((rc = db_device(h))) return rc;
  h->cand_ref.clear();
  h->cand_count.clear();
  h->cand_off.assign(1, 0);
  h->h_corr.clear();
  h->last_ms = 0.0;
  if (K_out) *K_out = 0;
  const int maps        = (int) h->h_starts.size() - 1;
  const uint32_t L      = distance_limit(max_distance);
  // age gate (:150-151) with the reference's unsigned arithmetic: map r fails iff q - min_age <= r <= q
  const long long q     = query_index;
  const int map_lo      = (int) std::min<long long>(maps, std::max<long long>(0, q - (long long) min_age));
  const int map_hi      = (int) std::min<long long>(maps, q + 1);
  const int map_skip    = std::max(0, map_hi - map_lo);
  const int searched    = maps - map_skip;
  const long long lo    = h->h_starts[map_lo], skip = h->h_starts[map_lo + map_skip] - lo;
  const long long nactive = h->h_starts.back() - skip;
  h->map_counts.assign(maps, 0);
  for (int r = map_lo; r < map_lo + map_skip; ++r) h->map_counts[r] = -1;
  int nv     = 0;
  size_t off = 0;
  if (sv) {
    if ((rc = scene_count(h, *sv, &nv))) return rc;
  } else if ((rc = stage(h, d, valid, n, &nv, &off))) {
    return rc;
  }
  if (nv == 0 || nactive == 0 || searched == 0) return 0;  // no pair: every searched map counts 0
  if ((rc = grow_keep(h->query, (size_t) nv * 2, 0, h->stream))) return rc;
  if ((rc = grow_keep(h->query_idx, (size_t) nv, 0, h->stream))) return rc;
  if ((rc = grow_keep(h->best, (size_t) h->h_starts.back(), 0, h->stream))) return rc;
  if ((rc = grow_keep(h->count, (size_t) h->h_starts.back(), 0, h->stream))) return rc;
  if ((rc = grow_keep(h->stats, (size_t) maps, 0, h->stream))) return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  if (sv) {
    scene_scatter(h, *sv, nv, h->query.p, h->query_idx.p);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(h->query.p, h->staging.p, (size_t) nv * SRRG2_DESCRIPTOR_BYTES, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->query_idx.p, (uint8_t*) h->staging.p + off, (size_t) nv * 4, hipMemcpyHostToDevice, h->stream));
  }
  const long long blocks = (nactive + THREADS * DPT - 1) / (THREADS * DPT);
  hipLaunchKernelGGL(k_desc_match, dim3((unsigned) blocks), dim3(THREADS), 0, h->stream, h->desc.p, lo, skip, nactive,
                     h->query.p, nv, L, h->best.p, h->count.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_desc_map_stats, dim3(searched), dim3(THREADS), 0, h->stream, h->starts.p, map_lo, map_skip,
                     h->best.p, h->count.p, L, h->stats.p);
  HIP_TRY(hipGetLastError());
  h->h_stats.resize(maps);
  HIP_TRY(hipMemcpyAsync(h->h_stats.data(), h->stats.p, (size_t) maps * sizeof(MapStat), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // count gate (:152-154): number_of_matches > relocalize_min_inliers; candidates ascend in r
  std::vector<Candidate> cands;
  for (int r = 0; r < maps; ++r) {
    if (r >= map_lo && r < map_lo + map_skip) continue;
    const MapStat s = h->h_stats[r];
    h->map_counts[r] = s.count;
    if (s.count > 0 && s.count > min_matches) {
      cands.push_back(Candidate{h->h_starts[r], h->h_starts[r + 1], h->cand_off.back()});
      h->cand_ref.push_back(r);
      h->cand_count.push_back(s.count);
      h->cand_off.push_back(h->cand_off.back() + s.kept);
    }
  }
  const int K            = (int) cands.size();
  const long long total  = h->cand_off.back();
  if (K > 0 && total > 0) {
    if ((rc = grow_keep(h->cands, (size_t) K, 0, h->stream))) return rc;
    if ((rc = grow_keep(h->corr, (size_t) total, 0, h->stream))) return rc;
    if ((rc = host_reserve(h->staging, (size_t) K * sizeof(Candidate)))) return rc;
    std::memcpy(h->staging.p, cands.data(), (size_t) K * sizeof(Candidate));
    HIP_TRY(hipMemcpyAsync(h->cands.p, h->staging.p, (size_t) K * sizeof(Candidate), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_desc_emit, dim3(K), dim3(THREADS), 0, h->stream, h->cands.p, h->best.p, h->ref_idx.p,
                       h->query_idx.p, L, h->corr.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  h->h_corr.resize((size_t) total);
  if (total > 0)
    HIP_TRY(hipMemcpyAsync(h->h_corr.data(), h->corr.p, (size_t) total * sizeof(srrg2_correspondence),
                           hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms;
  if (K_out) *K_out = K;
  return 0;
}

}  // namespace

int srrg2_descriptor_db_match(srrg2_descriptor_db_h h, const uint8_t* d, const uint8_t* valid, int n,
                              int64_t query_index, float max_distance, uint32_t min_age, int64_t min_matches,
                              int* K_out) {
  if (!h || n < 0 || (n > 0 && !d) || std::isnan(max_distance) || query_index < 0 || min_matches < 0)
    return fail(SRRG2_E_INVALID, "descriptor_db_match: bad arguments");
  if (n > MAX_QUERY) return fail(SRRG2_E_INVALID, "descriptor_db_match: a query holds at most 2^23 descriptors");
  return match_impl(h, d, valid, n, nullptr, query_index, max_distance, min_age, min_matches, K_out);
}

int srrg2_descriptor_db_match_scene(srrg2_descriptor_db_h h, srrg2_scene_h scene, int64_t query_index, float max_distance,
                                    uint32_t min_age, int64_t min_matches, int* K_out) {
  if (std::isnan(max_distance) || query_index < 0 || min_matches < 0)
    return fail(SRRG2_E_INVALID, "descriptor_db_match_scene: bad arguments");
  srrg2amd::SceneFeatureView v;
  int rc;
  if ((rc = scene_view(h, scene, "descriptor_db_match_scene", &v))) return rc;
  return match_impl(h, nullptr, nullptr, v.n, &v, query_index, max_distance, min_age, min_matches, K_out);
}

int srrg2_descriptor_db_get_candidates(srrg2_descriptor_db_h h, int32_t* reference, int64_t* num_matches,
                                       int64_t* corr_offsets, int* n_inout) {
  if (!h || !n_inout) return fail(SRRG2_E_INVALID, "descriptor_db_get_candidates: bad arguments");
  const int K = (int) h->cand_ref.size();
  if (reference || num_matches || corr_offsets) {
    if (*n_inout < K) return fail(SRRG2_E_INVALID, "descriptor_db_get_candidates: buffer too small");
    if (reference) std::memcpy(reference, h->cand_ref.data(), (size_t) K * sizeof(int32_t));
    if (num_matches) std::memcpy(num_matches, h->cand_count.data(), (size_t) K * sizeof(int64_t));
    if (corr_offsets) std::memcpy(corr_offsets, h->cand_off.data(), (size_t) (K + 1) * sizeof(int64_t));
  }
  *n_inout = K;
  return 0;
}

int srrg2_descriptor_db_get_correspondences(srrg2_descriptor_db_h h, srrg2_correspondence* buf, int64_t* n_inout) {
  if (!h || !n_inout) return fail(SRRG2_E_INVALID, "descriptor_db_get_correspondences: bad arguments");
  const int64_t n = (int64_t) h->h_corr.size();
  if (buf) {
    if (*n_inout < n) return fail(SRRG2_E_INVALID, "descriptor_db_get_correspondences: buffer too small");
    std::memcpy(buf, h->h_corr.data(), (size_t) n * sizeof(srrg2_correspondence));
  }
  *n_inout = n;
  return 0;
}

int srrg2_descriptor_db_get_map_counts(srrg2_descriptor_db_h h, int64_t* counts, int* n_inout) {
  if (!h || !n_inout) return fail(SRRG2_E_INVALID, "descriptor_db_get_map_counts: bad arguments");
  const int n = (int) h->map_counts.size();
  if (counts) {
    if (*n_inout < n) return fail(SRRG2_E_INVALID, "descriptor_db_get_map_counts: buffer too small");
    std::memcpy(counts, h->map_counts.data(), (size_t) n * sizeof(int64_t));
  }
  *n_inout = n;
  return 0;
}

int srrg2_descriptor_db_last_match_ms(srrg2_descriptor_db_h h, double* ms) {
  if (!h || !ms) return fail(SRRG2_E_INVALID, "descriptor_db_last_match_ms: bad arguments");
  *ms = h->last_ms;
  return 0;
}
