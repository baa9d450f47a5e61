// rectify.hip -- srrg2_rectifier_*, srrg2_rectify_image / _pair, srrg2_stereo_rectify: lens undistortion and stereo
// rectification of raw images on the device, the stage in front of the image adaptors.  No reference counterpart; DESIGN.md
// section 4 "Rectification" is the contract and tests/rectify_restatement.py its executable form.  The map is float64 with the
// operation order of the contract (the library is built without FP contraction), everything behind it is integer: the result
// is a function of the parameters and the pixels alone, bit for bit.
//   k_rect_map          one thread per destination pixel: the camera model -> (U, V) in 1/256 source pixel, or INT32_MIN twice;
//                        the valid count and the rows / columns that hold a valid entry are reduced per workgroup in LDS.  Rows
//                        of the map lie at a pitch that is a multiple of 4 entries, so a row's groups of four start 32-byte
//                        aligned.  Runs once per camera.
//   k_rect_remap<TYPE>  a workgroup owns a 64 x 16 destination tile, a thread 4 adjacent pixels of a row: two 16-byte loads
//                        of the map, 16 byte gathers (U8, bilinear) or 4 element gathers (U16 / F32, nearest), one 32-bit store
//                        where the four bytes exist and lie aligned, single stores otherwise.  A wave covers 4 rows x 64 columns,
//                        so its gathers touch a compact source patch.  blockIdx.y picks the image of a pair.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "host_util.h"
#include "scene_state.h"

using srrg2amd::fail;

struct srrg2_rectifier_s {
  int device = 0;
  hipStream_t stream = nullptr;
  // recorded behind every piece of work that reads the map or the staging blocks; `last` is the stream it was recorded on
  // (nullptr: nothing outstanding): work on another stream, a new map and the destructor wait for it
  hipEvent_t done  = nullptr;
  hipStream_t last = nullptr;
  bool is_set = false, identity = false;
  srrg2_rectifier_params p;
  int pitch = 0;  // entries per row of the map
  srrg2amd::DevBuf<int> map, info;
  srrg2amd::PinnedBuf<int> info_host;
  srrg2amd::DevBuf<unsigned char> src_stage, dst_stage;
  ~srrg2_rectifier_s() {
    (void) hipSetDevice(device);
    if (done && last) (void) hipEventSynchronize(done);
    if (stream) (void) hipStreamSynchronize(stream);
    if (done) (void) hipEventDestroy(done);
    if (stream) (void) hipStreamDestroy(stream);
  }
};

namespace {

enum { TILE_W = 64, TILE_H = 16, MAX_SIDE = 1 << 22, INFO_WORDS = 8 };
enum { I_VALID = 0, I_ROW_MIN, I_ROW_MAX, I_COL_MIN, I_COL_MAX };

struct RectModel {
  double fx, fy, cx, cy;      // source
  double k1, k2, p1, p2, k3, k4, k5, k6;
  double R[9];
  double nfx, nfy, ncx, ncy;  // target
  double u_max, v_max;        // 256 (src_cols - 1), 256 (src_rows - 1)
  int rows, cols, pitch;
};

// map: rows x pitch entries (U, V); the pad columns get the invalid entry
__global__ __launch_bounds__(256) void k_rect_map(RectModel M, int* __restrict__ map, int* __restrict__ info) {
  __shared__ int s[5];
  if (threadIdx.x == 0) s[I_VALID] = 0, s[I_ROW_MIN] = INT_MAX, s[I_ROW_MAX] = -1, s[I_COL_MIN] = INT_MAX, s[I_COL_MAX] = -1;
  __syncthreads();
  const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
  if (i < (long long) M.rows * M.pitch) {
    const int r = (int) (i / M.pitch), c = (int) (i - (long long) r * M.pitch);
    int U = INT_MIN, V = INT_MIN;
    if (c < M.cols) {
      const double x  = ((double) c - M.ncx) / M.nfx, y = ((double) r - M.ncy) / M.nfy;
      const double X  = (M.R[0] * x + M.R[3] * y) + M.R[6];
      const double Y  = (M.R[1] * x + M.R[4] * y) + M.R[7];
      const double W  = (M.R[2] * x + M.R[5] * y) + M.R[8];
      const double xn = X / W, yn = Y / W;
      const double r2  = xn * xn + yn * yn;
      const double num = 1.0 + r2 * (M.k1 + r2 * (M.k2 + r2 * M.k3));
      const double den = 1.0 + r2 * (M.k4 + r2 * (M.k5 + r2 * M.k6));
      const double rad = num / den;
      const double xy  = xn * yn;
      const double xd  = xn * rad + ((2.0 * M.p1) * xy + M.p2 * (r2 + 2.0 * (xn * xn)));
      const double yd  = yn * rad + (M.p1 * (r2 + 2.0 * (yn * yn)) + (2.0 * M.p2) * xy);
      const double u = M.fx * xd + M.cx, v = M.fy * yd + M.cy;
      const double Ud = floor(u * 256.0 + 0.5), Vd = floor(v * 256.0 + 0.5);
      // decided on the doubles: nothing out of range is ever converted (a NaN fails every comparison)
      if (W > 0.0 && den > 0.0 && isfinite(u) && isfinite(v) && Ud >= 0.0 && Ud <= M.u_max && Vd >= 0.0 && Vd <= M.v_max) {
        U = (int) Ud, V = (int) Vd;
        atomicAdd(&s[I_VALID], 1);
        atomicMin(&s[I_ROW_MIN], r), atomicMax(&s[I_ROW_MAX], r);
        atomicMin(&s[I_COL_MIN], c), atomicMax(&s[I_COL_MAX], c);
      }
    }
    *reinterpret_cast<int2*>(map + 2 * i) = make_int2(U, V);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s[I_VALID] > 0) {
    atomicAdd(&info[I_VALID], s[I_VALID]);
    atomicMin(&info[I_ROW_MIN], s[I_ROW_MIN]), atomicMax(&info[I_ROW_MAX], s[I_ROW_MAX]);
    atomicMin(&info[I_COL_MIN], s[I_COL_MIN]), atomicMax(&info[I_COL_MAX], s[I_COL_MAX]);
  }
}

// one image of a call: its map (rows x pitch entries), source and destination with their row strides in bytes
struct RemapJob {
  const int* map;
  const unsigned char* src;
  unsigned char* dst;
  long long src_stride, dst_stride;
  int src_rows, src_cols;
};
struct RemapJobs {
  RemapJob j[2];
};

template <int TYPE>
struct Pixel;
template <>
struct Pixel<SRRG2_IMAGE_U16> {
  typedef unsigned short T;
  static __device__ __forceinline__ T none() { return 0; }
};
template <>
struct Pixel<SRRG2_IMAGE_F32> {
  typedef unsigned T;  // (the bits: a NaN's payload survives)
  static __device__ __forceinline__ T none() { return 0x7fc00000u; }
};

__device__ __forceinline__ unsigned bilinear_u8(const RemapJob& j, int U, int V, unsigned border) {
  if (U == INT_MIN) return border;
  const int x0 = U >> 8, y0 = V >> 8;  // (0 <= U <= 256 (src_cols - 1), rows likewise: x0, y0 lie inside)
  const int x1 = min(x0 + 1, j.src_cols - 1), y1 = min(y0 + 1, j.src_rows - 1);
  const unsigned fx = U & 255, fy = V & 255;
  const unsigned char *a = j.src + (long long) y0 * j.src_stride, *b = j.src + (long long) y1 * j.src_stride;
  return ((unsigned) a[x0] * (256 - fx) * (256 - fy) + (unsigned) a[x1] * fx * (256 - fy) + (unsigned) b[x0] * (256 - fx) * fy +
          (unsigned) b[x1] * fx * fy + 32768u) >> 16;
}

// tiles: tiles_x * tiles_y workgroups along x (a row count beyond the y limit of a grid stays possible), the image along y
template <int TYPE>
__global__ __launch_bounds__(256) void k_rect_remap(RemapJobs J, int rows, int cols, int pitch, int tiles_x, unsigned border) {
  const RemapJob& j = J.j[blockIdx.y];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int r = ty * TILE_H + (threadIdx.x >> 4), c = tx * TILE_W + (threadIdx.x & 15) * 4;  // the thread's pixels: (r, c .. c + 3)
  if (r >= rows || c >= cols) return;
  const int4* m = reinterpret_cast<const int4*>(j.map + 2 * ((long long) r * pitch + c));  // (pitch and c: multiples of 4)
  const int4 m0 = m[0], m1 = m[1];
  const int U[4] = {m0.x, m0.z, m1.x, m1.z}, V[4] = {m0.y, m0.w, m1.y, m1.w};
  const int left = min(4, cols - c);
  if constexpr (TYPE == SRRG2_IMAGE_U8) {
    unsigned v[4], word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = q < left ? bilinear_u8(j, U[q], V[q], border) : 0u;
      word |= v[q] << (8 * q);
    }
    unsigned char* out = j.dst + (long long) r * j.dst_stride + c;
    if (left == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
      *reinterpret_cast<unsigned*>(out) = word;
    } else {  // the row's tail, or a row that does not start on a word
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < left) out[q] = (unsigned char) v[q];
    }
  } else {
    typedef typename Pixel<TYPE>::T T;
    T* out = reinterpret_cast<T*>(j.dst + (long long) r * j.dst_stride) + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= left) break;
      T v = Pixel<TYPE>::none();
      if (U[q] != INT_MIN)
        v = reinterpret_cast<const T*>(j.src + (long long) ((V[q] + 128) >> 8) * j.src_stride)[(U[q] + 128) >> 8];
      out[q] = v;
    }
  }
}

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

int element_size(int type) { return type == SRRG2_IMAGE_U8 ? 1 : type == SRRG2_IMAGE_U16 ? 2 : type == SRRG2_IMAGE_F32 ? 4 : 0; }

// what srrg2_rectifier_set refuses for the parameters alone
int check_params(const std::string& who, const srrg2_rectifier_params* p) {
  if (!p) return fail(SRRG2_E_INVALID, who + "null params");
  if (p->src_rows < 0 || p->src_cols < 0 || p->dst_rows < 0 || p->dst_cols < 0)
    return fail(SRRG2_E_INVALID, who + "rows and cols must be >= 0");
  if ((long long) p->src_rows * p->src_cols > 0x7fffffffLL || (long long) p->dst_rows * p->dst_cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, who + "rows*cols beyond int32");
  if (!finite_all(p->camera_matrix, 9) || !finite_all(p->distortion, 8) || !finite_all(p->rotation, 9) ||
      !finite_all(p->new_camera_matrix, 9))
    return fail(SRRG2_E_INVALID, who + "a parameter that is not finite");
  if (p->camera_matrix[0] == 0.0 || p->camera_matrix[4] == 0.0 || p->new_camera_matrix[0] == 0.0 || p->new_camera_matrix[4] == 0.0)
    return fail(SRRG2_E_INVALID, who + "fx and fy of both camera matrices must be non-zero");
  if (p->camera_matrix[1] != 0.0 || p->new_camera_matrix[1] != 0.0)
    return fail(SRRG2_E_UNSUPPORTED, who + "a camera matrix with skew (K[0][1] != 0)");
  if (p->src_rows > MAX_SIDE || p->src_cols > MAX_SIDE) return fail(SRRG2_E_UNSUPPORTED, who + "a source side above 4194304");
  return 0;
}

// one image of a call as the caller describes it
struct ImageArg {
  const void* src;
  int src_stride;
  void* dst;
  int dst_stride;
};

int check_image(const std::string& who, const srrg2_rectifier_s* h, int esize, const ImageArg& a) {
  const long long src_n = (long long) h->p.src_rows * h->p.src_cols, dst_n = (long long) h->p.dst_rows * h->p.dst_cols;
  if (dst_n == 0) return 0;
  if (!a.dst || (src_n > 0 && !a.src)) return fail(SRRG2_E_INVALID, who + "null image");
  if (src_n > 0 && ((long long) a.src_stride < (long long) h->p.src_cols * esize || a.src_stride % esize != 0 ||
                    reinterpret_cast<uintptr_t>(a.src) % esize != 0))
    return fail(SRRG2_E_INVALID, who + "source row stride smaller than a row or misaligned");
  if ((long long) a.dst_stride < (long long) h->p.dst_cols * esize || a.dst_stride % esize != 0 ||
      reinterpret_cast<uintptr_t>(a.dst) % esize != 0)
    return fail(SRRG2_E_INVALID, who + "destination row stride smaller than a row or misaligned");
  return 0;
}

// n images (1 or 2) of one type through their handles' maps, the targets of one shape: staging, ONE launch, the copy back
int run(const std::string& who, srrg2_rectifier_s* const* hs, int n, srrg2_scene* order_on, int type, int src_mem, int dst_mem, int border,
        const ImageArg* img) {
  srrg2_rectifier_s* const h = hs[0];  // (its stream and staging blocks serve the call)
  const int esize = element_size(type);
  const int rows = h->p.dst_rows, cols = h->p.dst_cols;
  if ((long long) rows * cols == 0) return 0;
  HIP_TRY(hipSetDevice(h->device));
  const bool queued = order_on && dst_mem == SRRG2_MEM_DEVICE;
  hipStream_t st = queued ? order_on->stream : h->stream;
  for (int k = 0; k < n; ++k)  // work of an earlier call on another stream still reads the map and the staging blocks
    if (hs[k]->last && hs[k]->last != st) HIP_TRY(hipStreamWaitEvent(st, hs[k]->done, 0));
  int rc;
  RemapJobs J;
  std::memset(&J, 0, sizeof(J));
  size_t src_off[2] = {0, 0}, src_bytes[2] = {0, 0}, dst_off[2] = {0, 0}, need_src = 0, need_dst = 0;
  const size_t dst_row = ((size_t) cols * esize + 3) / 4 * 4;  // rows of a staged destination: packed up to a word
  for (int k = 0; k < n; ++k) {
    const srrg2_rectifier_params& p = hs[k]->p;
    if (src_mem == SRRG2_MEM_HOST && (long long) p.src_rows * p.src_cols > 0) {  // rows up to the last pixel, as they lie
      src_off[k]   = need_src;
      src_bytes[k] = (size_t) (p.src_rows - 1) * (size_t) img[k].src_stride + (size_t) p.src_cols * esize;
      need_src     = (need_src + src_bytes[k] + 63) / 64 * 64;
    }
    if (dst_mem == SRRG2_MEM_HOST) {
      dst_off[k] = need_dst;
      need_dst   = (need_dst + dst_row * (size_t) rows + 63) / 64 * 64;
    }
  }
  if ((need_src && (rc = h->src_stage.reserve(need_src))) || (need_dst && (rc = h->dst_stage.reserve(need_dst)))) return rc;
  for (int k = 0; k < n; ++k) {
    const srrg2_rectifier_params& p = hs[k]->p;
    RemapJob& j = J.j[k];
    j.map        = hs[k]->map.p;
    j.src_rows   = p.src_rows, j.src_cols = p.src_cols;
    j.src        = static_cast<const unsigned char*>(img[k].src);
    j.src_stride = img[k].src_stride;
    if (src_bytes[k]) {
      HIP_TRY(hipMemcpyAsync(h->src_stage.p + src_off[k], img[k].src, src_bytes[k], hipMemcpyHostToDevice, st));
      j.src = h->src_stage.p + src_off[k];
    }
    j.dst        = static_cast<unsigned char*>(img[k].dst);
    j.dst_stride = img[k].dst_stride;
    if (dst_mem == SRRG2_MEM_HOST) j.dst = h->dst_stage.p + dst_off[k], j.dst_stride = (long long) dst_row;
  }
  const int tiles_x = (cols + TILE_W - 1) / TILE_W, tiles_y = (rows + TILE_H - 1) / TILE_H;
  if ((long long) tiles_x * tiles_y > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "more than 2^31 - 1 tiles");
  const dim3 grid((unsigned) (tiles_x * tiles_y), (unsigned) n), block(256);
  if (type == SRRG2_IMAGE_U8)
    hipLaunchKernelGGL(k_rect_remap<SRRG2_IMAGE_U8>, grid, block, 0, st, J, rows, cols, h->pitch, tiles_x, (unsigned) border);
  else if (type == SRRG2_IMAGE_U16)
    hipLaunchKernelGGL(k_rect_remap<SRRG2_IMAGE_U16>, grid, block, 0, st, J, rows, cols, h->pitch, tiles_x, 0u);
  else
    hipLaunchKernelGGL(k_rect_remap<SRRG2_IMAGE_F32>, grid, block, 0, st, J, rows, cols, h->pitch, tiles_x, 0u);
  HIP_TRY(hipGetLastError());
  if (dst_mem == SRRG2_MEM_HOST)
    for (int k = 0; k < n; ++k)
      HIP_TRY(hipMemcpy2DAsync(img[k].dst, (size_t) img[k].dst_stride, J.j[k].dst, dst_row, (size_t) cols * esize, (size_t) rows,
                               hipMemcpyDeviceToHost, st));
  for (int k = 0; k < n; ++k) {
    HIP_TRY(hipEventRecord(hs[k]->done, st));
    hs[k]->last = st;
  }
  if (!queued) {
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n; ++k) hs[k]->last = nullptr;
  }
  return 0;
}

double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace

extern "C" int srrg2_rectifier_create(int device, srrg2_rectifier_h* out) {
  if (!out) return fail(SRRG2_E_INVALID, "rectifier_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "rectifier_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "rectifier_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<srrg2_rectifier_s> h(new srrg2_rectifier_s());  // (a failure below deletes it)
  h->device = device;
  srrg2_rectifier_default_params(&h->p);
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return 0;
}

extern "C" int srrg2_rectifier_destroy(srrg2_rectifier_h h) {
  delete h;  // (null: nothing to do)
  return 0;
}

extern "C" void srrg2_rectifier_default_params(srrg2_rectifier_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->rotation[0] = p->rotation[4] = p->rotation[8] = 1.0;
}

extern "C" int srrg2_rectifier_set(srrg2_rectifier_h h, const srrg2_rectifier_params* p, srrg2_rectifier_info* info_out) {
  const std::string who = "rectifier_set: ";
  int rc;
  if ((rc = check_params(who, p))) return rc;  // (the parameters first: what they are refused for needs no handle)
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  if (h->last && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));  // a queued call still reads the old map
  const int pitch = (p->dst_cols + 3) / 4 * 4;
  const long long entries = (long long) p->dst_rows * pitch;
  h->is_set = false;
  if ((rc = h->map.reserve(2 * (size_t) entries + 8)) || (rc = h->info.reserve(INFO_WORDS)) || (rc = h->info_host.reserve(2 * INFO_WORDS)))
    return rc;
  int* const init = h->info_host.p + INFO_WORDS;
  init[I_VALID] = 0, init[I_ROW_MIN] = INT_MAX, init[I_ROW_MAX] = -1, init[I_COL_MIN] = INT_MAX, init[I_COL_MAX] = -1;
  std::memset(h->info_host.p, 0, INFO_WORDS * sizeof(int));
  if (entries > 0) {
    RectModel M;
    M.fx = p->camera_matrix[0], M.fy = p->camera_matrix[4], M.cx = p->camera_matrix[2], M.cy = p->camera_matrix[5];
    M.k1 = p->distortion[0], M.k2 = p->distortion[1], M.p1 = p->distortion[2], M.p2 = p->distortion[3];
    M.k3 = p->distortion[4], M.k4 = p->distortion[5], M.k5 = p->distortion[6], M.k6 = p->distortion[7];
    for (int i = 0; i < 9; ++i) M.R[i] = p->rotation[i];
    M.nfx = p->new_camera_matrix[0], M.nfy = p->new_camera_matrix[4], M.ncx = p->new_camera_matrix[2], M.ncy = p->new_camera_matrix[5];
    M.u_max = 256.0 * (double) (p->src_cols - 1), M.v_max = 256.0 * (double) (p->src_rows - 1);
    M.rows = p->dst_rows, M.cols = p->dst_cols, M.pitch = pitch;
    const long long blocks = (entries + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "a map of more than 2^39 entries");
    HIP_TRY(hipMemcpyAsync(h->info.p, init, 5 * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rect_map, dim3((unsigned) blocks), dim3(256), 0, st, M, h->map.p, h->info.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->info_host.p, h->info.p, 5 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));  // the one wait
  h->last = nullptr;
  h->p = *p, h->pitch = pitch;
  const double* R = p->rotation;
  h->identity = R[0] == 1.0 && R[4] == 1.0 && R[8] == 1.0 && R[1] == 0.0 && R[2] == 0.0 && R[3] == 0.0 && R[5] == 0.0 && R[6] == 0.0 &&
                R[7] == 0.0;
  h->is_set = true;
  if (info_out) {
    const int* c = h->info_host.p;
    const bool any = c[I_VALID] > 0;
    info_out->num_pixels = (int32_t) ((long long) p->dst_rows * p->dst_cols);
    info_out->num_valid  = c[I_VALID];
    info_out->first_row = any ? c[I_ROW_MIN] : -1, info_out->last_row = any ? c[I_ROW_MAX] : -1;
    info_out->first_col = any ? c[I_COL_MIN] : -1, info_out->last_col = any ? c[I_COL_MAX] : -1;
  }
  return 0;
}

extern "C" int srrg2_rectifier_get_map(srrg2_rectifier_h h, int32_t* uv_out, int64_t capacity) {
  const std::string who = "rectifier_get_map: ";
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  if (!h->is_set) return fail(SRRG2_E_INVALID, who + "no camera set (srrg2_rectifier_set)");
  const long long n = (long long) h->p.dst_rows * h->p.dst_cols;
  if (capacity < 2 * n) return fail(SRRG2_E_INVALID, who + "capacity below 2 * dst_rows * dst_cols words");
  if (n == 0) return 0;
  if (!uv_out) return fail(SRRG2_E_INVALID, who + "null uv_out");
  HIP_TRY(hipSetDevice(h->device));
  const size_t row = 8 * (size_t) h->p.dst_cols;
  HIP_TRY(hipMemcpy2DAsync(uv_out, row, h->map.p, 8 * (size_t) h->pitch, row, (size_t) h->p.dst_rows, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int srrg2_rectifier_camera(srrg2_rectifier_h h, srrg2_depth_adaptor_params* cam) {
  const std::string who = "rectifier_camera: ";
  if (!h || !cam) return fail(SRRG2_E_INVALID, who + "null handle or params");
  if (!h->is_set) return fail(SRRG2_E_INVALID, who + "no camera set (srrg2_rectifier_set)");
  const double* K = h->p.new_camera_matrix;
  const float k[9] = {(float) K[0], 0.f, (float) K[2], 0.f, (float) K[4], (float) K[5], 0.f, 0.f, 1.f};
  std::memcpy(cam->camera_matrix, k, sizeof(k));
  cam->rows = h->p.dst_rows, cam->cols = h->p.dst_cols;
  return 0;
}

extern "C" int srrg2_rectify_image(srrg2_rectifier_h h, srrg2_scene_h order_on, const void* src, int type, int src_stride, int src_mem,
                                   void* dst, int dst_stride, int dst_mem, int border) {
  const std::string who = "rectify_image: ";
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  if (!h->is_set) return fail(SRRG2_E_INVALID, who + "no camera set (srrg2_rectifier_set)");
  if ((src_mem != SRRG2_MEM_HOST && src_mem != SRRG2_MEM_DEVICE) || (dst_mem != SRRG2_MEM_HOST && dst_mem != SRRG2_MEM_DEVICE))
    return fail(SRRG2_E_INVALID, who + "bad mem");
  const int esize = element_size(type);
  if (!esize) return fail(SRRG2_E_INVALID, who + "bad image type");
  if (border < 0 || border > 255) return fail(SRRG2_E_INVALID, who + "border 0 .. 255");
  if (order_on && order_on->device != h->device) return fail(SRRG2_E_INVALID, who + "order_on lives on another device");
  const ImageArg img{src, src_stride, dst, dst_stride};
  int rc;
  if ((rc = check_image(who, h, esize, img))) return rc;
  if (type != SRRG2_IMAGE_U8 && !h->identity)
    return fail(SRRG2_E_UNSUPPORTED, who + "a depth image under a rotation (z along the optical axis would change)");
  return run(who, &h, 1, order_on, type, src_mem, dst_mem, border, &img);
}

extern "C" int srrg2_rectify_pair(srrg2_rectifier_h left_h, srrg2_rectifier_h right_h, srrg2_scene_h order_on, const void* left,
                                  int left_stride, const void* right, int right_stride, int mem, void* dst_left, int dst_left_stride,
                                  void* dst_right, int dst_right_stride, int dst_mem, int border) {
  const std::string who = "rectify_pair: ";
  if (!left_h || !right_h) return fail(SRRG2_E_INVALID, who + "null handle");
  if (!left_h->is_set || !right_h->is_set) return fail(SRRG2_E_INVALID, who + "no camera set (srrg2_rectifier_set)");
  if (left_h == right_h) return fail(SRRG2_E_INVALID, who + "one handle for both images");
  if (left_h->device != right_h->device) return fail(SRRG2_E_INVALID, who + "the handles live on different devices");
  if ((mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) || (dst_mem != SRRG2_MEM_HOST && dst_mem != SRRG2_MEM_DEVICE))
    return fail(SRRG2_E_INVALID, who + "bad mem");
  if (border < 0 || border > 255) return fail(SRRG2_E_INVALID, who + "border 0 .. 255");
  if (order_on && order_on->device != left_h->device) return fail(SRRG2_E_INVALID, who + "order_on lives on another device");
  if (left_h->p.dst_rows != right_h->p.dst_rows || left_h->p.dst_cols != right_h->p.dst_cols)
    return fail(SRRG2_E_INVALID, who + "targets of different shape");
  const ImageArg img[2] = {{left, left_stride, dst_left, dst_left_stride}, {right, right_stride, dst_right, dst_right_stride}};
  srrg2_rectifier_s* const hs[2] = {left_h, right_h};
  int rc;
  for (int k = 0; k < 2; ++k)
    if ((rc = check_image(who, hs[k], 1, img[k]))) return rc;
  return run(who, hs, 2, order_on, SRRG2_IMAGE_U8, mem, dst_mem, border, img);
}

// host only, float64, + - * / sqrt in the order of the contract
extern "C" int srrg2_stereo_rectify(const double* KL, const double* KR, const double* R, const double* t, double* R1_out, double* R2_out,
                                    double* Knew_out, double* baseline_out) {
  const std::string who = "stereo_rectify: ";
  if (!KL || !KR || !R || !t) return fail(SRRG2_E_INVALID, who + "null input");
  if (!finite_all(KL, 9) || !finite_all(KR, 9) || !finite_all(R, 9) || !finite_all(t, 3))
    return fail(SRRG2_E_INVALID, who + "an input that is not finite");
  double c[3], e1[3], e2[3], e3[3], zm[3], z[3];
  for (int i = 0; i < 3; ++i) c[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);  // -R^T t
  const double b = std::sqrt(dot3(c, c));
  if (!(b > 0.0) || !std::isfinite(b)) return fail(SRRG2_E_INVALID, who + "the two cameras share their centre");
  for (int i = 0; i < 3; ++i) e1[i] = c[i] / b;
  zm[0] = (0.0 + R[6]) / 2.0, zm[1] = (0.0 + R[7]) / 2.0, zm[2] = (1.0 + R[8]) / 2.0;
  cross3(zm, e1, z);
  const double zn = std::sqrt(dot3(z, z));
  if (!(zn > 0.0) || !std::isfinite(zn)) return fail(SRRG2_E_INVALID, who + "the baseline runs along the mean optical axis");
  for (int i = 0; i < 3; ++i) e2[i] = z[i] / zn;
  cross3(e1, e2, e3);
  double R1[9];
  for (int i = 0; i < 3; ++i) R1[i] = e1[i], R1[3 + i] = e2[i], R1[6 + i] = e3[i];
  if (R1_out) std::memcpy(R1_out, R1, sizeof(R1));
  if (R2_out)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R2_out[3 * i + j] = dot3(R1 + 3 * i, R + 3 * j);  // R1 R^T
  if (Knew_out) {
    const double f = (KL[4] + KR[4]) / 2.0;
    const double K[9] = {f, 0.0, (KL[2] + KR[2]) / 2.0, 0.0, f, (KL[5] + KR[5]) / 2.0, 0.0, 0.0, 1.0};
    std::memcpy(Knew_out, K, sizeof(K));
  }
  if (baseline_out) *baseline_out = b;
  return 0;
}
