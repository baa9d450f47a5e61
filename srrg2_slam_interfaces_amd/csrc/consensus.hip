// consensus.hip -- srrg2_consensus_compute: a consensus pose (RANSAC with a fixed hypothesis count) from the descriptor matches of
// K candidates, on the device.  The reference has no such step (its HBST detector hands raw matches to the locked solve,
// S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:257-377); DESIGN.md section 4 "Consensus pose" is the contract
// and tests/consensus_restatement.py its executable form.  The sampler and the minimal solvers are consensus_math.h (float64,
// + - * / sqrt); the score is float32 in the written order; counts and costs are integers: the result is a function of the
// clouds, the records and the parameters alone, bit for bit, whatever the scheduling.
//   k_cns_gather   one thread per pair: both points packed as float4 (f.w = valid, m.w = the candidate), so that no later pass
//                  reads a cloud
//   k_cns_hyp      one thread per (candidate, hypothesis): sample, solve, length check; the scored ones are compacted per
//                  candidate with ONE atomic per wave (ballot + popcount), the three counters likewise
//   k_cns_score    one workgroup per (candidate, tile of SCORE_TILE pairs, chunk of SCORE_CHUNK survivors): each lane keeps its
//                  SCORE_PPT pairs in registers, the pose is uniform (scalar loads); count by ballot + popcount, cost by a wave
//                  shuffle sum, the four waves meet in LDS and ONE 32-bit and ONE 64-bit atomic per (hypothesis, workgroup)
//                  leave.  The grid is the worst case (every hypothesis scored); a workgroup reads the survivor count from
//                  device memory and leaves when its chunk is empty
//   k_cns_select   one wave per candidate: largest count, smallest cost, smallest h; the valid pairs; the result record
//   k_cns_flags    one thread per pair: inlier of its candidate's best pose (FOUND candidates only)
//   (exclusive scan of the flags: srrg2amd::launch_exclusive_scan)
//   k_cns_scatter  flagged pair -> its slot of the capacity-bounded output; the K + 1 offsets
// The number of launches does not depend on K, H or N, and there is ONE host wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "consensus_math.h"
#include "det_math.h"
#include "host_util.h"
#include "kernels.h"

using srrg2amd::DevBuf;
using srrg2amd::fail;

namespace {

constexpr int SCORE_THREADS = 256;                        // four waves
constexpr int SCORE_PPT     = 4;                          // pairs per lane
constexpr int SCORE_TILE    = SCORE_THREADS * SCORE_PPT;  // pairs per workgroup
constexpr int SCORE_CHUNK   = 16;                         // survivors per workgroup
constexpr int HYP_THREADS   = 256;

struct CandMeta {
  int corr_begin, n;      // the candidate's pairs: [corr_begin, corr_begin + n) of the packed arrays
  int mov_begin, mov_n;   // its cloud: points [mov_begin, mov_begin + mov_n) of the moving array
  double scale;           // 2^cost_exponent
  int cost_exponent, pad;
};
static_assert(sizeof(CandMeta) == 32, "CandMeta");

struct CnsParams {
  int dim, H, K, length_check, min_inliers;
  unsigned seed;
  float tau32;
  double tau, msd2;
};

__device__ __forceinline__ bool finite_f(float x) { return (x - x) == 0.f; }

// the packed arrays and the kernel-side pose are those of dim 3: a dim-2 pair has z = 0 and a dim-2 pose a zero third row and
// column, which adds +-0 to the sums of the contract's dim-2 expressions and leaves e as it is
__global__ __launch_bounds__(256) void k_cns_gather(int P, int K, int dim, const CandMeta* __restrict__ cand,
                                                    const srrg2_correspondence* __restrict__ corr, const char* __restrict__ fixed,
                                                    int fstride, int nf, const char* __restrict__ moving, int mstride,
                                                    float4* __restrict__ pf, float4* __restrict__ pm) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int lo = 0, hi = K - 1;  // the last candidate whose pairs begin at or before p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cand[mid].corr_begin <= p) lo = mid;
    else hi = mid - 1;
  }
  const CandMeta c             = cand[lo];
  const srrg2_correspondence r = corr[p];
  float4 f = make_float4(0.f, 0.f, 0.f, 0.f), m = make_float4(0.f, 0.f, 0.f, __int_as_float(lo));
  if (r.fixed_idx >= 0 && r.fixed_idx < nf && r.moving_idx >= 0 && r.moving_idx < c.mov_n) {
    const float* a = reinterpret_cast<const float*>(fixed + (size_t) r.fixed_idx * (size_t) fstride);
    const float* b = reinterpret_cast<const float*>(moving + ((size_t) c.mov_begin + (size_t) r.moving_idx) * (size_t) mstride);
    const float ax = a[0], ay = a[1], az = dim == 3 ? a[2] : 0.f;
    const float bx = b[0], by = b[1], bz = dim == 3 ? b[2] : 0.f;
    if (finite_f(ax) && finite_f(ay) && finite_f(az) && finite_f(bx) && finite_f(by) && finite_f(bz)) {
      f = make_float4(ax, ay, az, 1.f);
      m.x = bx, m.y = by, m.z = bz;
    }
  }
  pf[p] = f;
  pm[p] = m;
}

// grid (ceil(H / HYP_THREADS), K).  pose: 12 floats per (candidate, slot), hyp_id the slot's hypothesis; ctr: 3 words per
// candidate (degenerate, rejected, scored)
template <int DIM>
__global__ __launch_bounds__(HYP_THREADS) void k_cns_hyp(CnsParams P, const CandMeta* __restrict__ cand, const float4* __restrict__ pf,
                                                         const float4* __restrict__ pm, int* __restrict__ nsurv, int* __restrict__ ctr,
                                                         float* __restrict__ pose, int* __restrict__ hyp_id) {
  constexpr int S = DIM == 3 ? 3 : 2;
  const int k = blockIdx.y, h = blockIdx.x * HYP_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const CandMeta c = cand[k];
  int status = -1;
  double X[12];
  if (h < P.H) {
    int idx[S];
    status = cm::HYP_DEGENERATE;
    if (cm::sample<S>(P.seed, (uint32_t) h, c.n, idx)) {
      float f[S][3], m[S][3];
      bool valid = true;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const float4 a = pf[c.corr_begin + idx[j]], b = pm[c.corr_begin + idx[j]];
        valid = valid && a.w != 0.f;
        f[j][0] = a.x, f[j][1] = a.y, f[j][2] = a.z;
        m[j][0] = b.x, m[j][1] = b.y, m[j][2] = b.z;
      }
      if (valid) {
        if constexpr (DIM == 3) status = cm::solve3(m[0], m[1], m[S - 1], f[0], f[1], f[S - 1], P.msd2, P.tau, P.length_check, X);
        else status = cm::solve2(m[0], m[1], f[0], f[1], P.msd2, P.tau, P.length_check, X);
      }
    }
  }
  const unsigned long long scored = __ballot(status == cm::HYP_SCORED);
  const unsigned long long degen  = __ballot(status == cm::HYP_DEGENERATE);
  const unsigned long long reject = __ballot(status == cm::HYP_REJECTED);
  int base = 0;
  if (lane == 0) {  // one atomic per wave and counter
    if (degen) atomicAdd(&ctr[3 * k + 0], __popcll(degen));
    if (reject) atomicAdd(&ctr[3 * k + 1], __popcll(reject));
    if (scored) {
      atomicAdd(&ctr[3 * k + 2], __popcll(scored));
      base = atomicAdd(&nsurv[k], __popcll(scored));
    }
  }
  base = __shfl(base, 0);
  if (status != cm::HYP_SCORED) return;
  const int slot    = base + __popcll(scored & ((1ull << lane) - 1ull));
  const size_t at   = (size_t) k * (size_t) P.H + (size_t) slot;
  float* const out  = pose + at * 12;
  hyp_id[at]        = h;
  if (DIM == 3) {
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = (float) X[i];  // this cast is the pose that is scored and returned
  } else {
    out[0] = (float) X[0], out[1] = (float) X[1], out[2] = 0.f, out[3] = (float) X[2];
    out[4] = (float) X[3], out[5] = (float) X[4], out[6] = 0.f, out[7] = (float) X[5];
    out[8] = 0.f, out[9] = 0.f, out[10] = 0.f, out[11] = 0.f;
  }
}

__device__ __forceinline__ float pair_error(const float* X, const float4& m, const float4& f) {
  const float r0 = (((X[0] * m.x + X[1] * m.y) + X[2] * m.z) + X[3]) - f.x;
  const float r1 = (((X[4] * m.x + X[5] * m.y) + X[6] * m.z) + X[7]) - f.y;
  const float r2 = (((X[8] * m.x + X[9] * m.y) + X[10] * m.z) + X[11]) - f.z;
  return (r0 * r0 + r1 * r1) + r2 * r2;
}

// grid (tiles * chunks, K): chunk = blockIdx.x % chunks, tile = blockIdx.x / chunks
__global__ __launch_bounds__(SCORE_THREADS) void k_cns_score(int H, int chunks, float tau32, const CandMeta* __restrict__ cand,
                                                             const float4* __restrict__ pf, const float4* __restrict__ pm,
                                                             const int* __restrict__ nsurv, const float* __restrict__ pose,
                                                             int* __restrict__ count, long long* __restrict__ cost) {
  __shared__ int s_cnt[SCORE_THREADS / 64][SCORE_CHUNK];
  __shared__ long long s_cost[SCORE_THREADS / 64][SCORE_CHUNK];
  const int k = blockIdx.y, chunk = blockIdx.x % chunks, tile = blockIdx.x / chunks;
  const CandMeta c = cand[k];
  const int ns = nsurv[k], s0 = chunk * SCORE_CHUNK;
  if (s0 >= ns || (long long) tile * SCORE_TILE >= c.n) return;  // (the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 f[SCORE_PPT], m[SCORE_PPT];
  bool ok[SCORE_PPT];
#pragma unroll
  for (int j = 0; j < SCORE_PPT; ++j) {
    const int i = tile * SCORE_TILE + j * SCORE_THREADS + (int) threadIdx.x;
    ok[j]       = false;
    f[j] = m[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < c.n) {
      f[j]  = pf[c.corr_begin + i];
      m[j]  = pm[c.corr_begin + i];
      ok[j] = f[j].w != 0.f;
    }
  }
  const float t2 = tau32 * tau32;
  const int nq   = min(SCORE_CHUNK, ns - s0);
  for (int q = 0; q < nq; ++q) {
    const float* __restrict__ Xp = pose + ((size_t) k * (size_t) H + (size_t) (s0 + q)) * 12;
    float X[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) X[i] = Xp[i];  // (uniform: the same address in every lane)
    int cnt       = 0;
    long long sum = 0;
#pragma unroll
    for (int j = 0; j < SCORE_PPT; ++j) {
      const float e   = pair_error(X, m[j], f[j]);
      const bool in   = ok[j] && e <= t2;
      cnt += __popcll(__ballot(in));
      if (in) sum += (long long) ((double) e * c.scale);  // trunc: the term is >= 0
    }
    if (cnt) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    }
    if (lane == 0) {
      s_cnt[wave][q]  = cnt;
      s_cost[wave][q] = sum;
    }
  }
  __syncthreads();
  if ((int) threadIdx.x < nq) {  // ONE 32-bit and ONE 64-bit atomic per (hypothesis, workgroup)
    const int q = threadIdx.x;
    int cnt = 0;
    long long sum = 0;
#pragma unroll
    for (int w = 0; w < SCORE_THREADS / 64; ++w) cnt += s_cnt[w][q], sum += s_cost[w][q];
    if (cnt) {
      const size_t at = (size_t) k * (size_t) H + (size_t) (s0 + q);
      atomicAdd(&count[at], cnt);
      atomicAdd(reinterpret_cast<unsigned long long*>(&cost[at]), (unsigned long long) sum);
    }
  }
}

// (count, cost, h) of a survivor: a beats b iff more inliers, then less cost, then the lower hypothesis
__device__ __forceinline__ bool better(int ca, long long sa, int ha, int cb, long long sb, int hb) {
  if (ca != cb) return ca > cb;
  if (sa != sb) return sa < sb;
  return ha < hb;
}

// one wave per candidate (blockDim = 64).  best: 16 floats per candidate -- the kernel-side pose and, in [12], FOUND as 1.f
__global__ __launch_bounds__(64) void k_cns_select(CnsParams P, const CandMeta* __restrict__ cand, const float4* __restrict__ pf,
                                                   const int* __restrict__ nsurv, const int* __restrict__ ctr,
                                                   const float* __restrict__ pose, const int* __restrict__ hyp_id,
                                                   const int* __restrict__ count, const long long* __restrict__ cost,
                                                   srrg2_consensus_result* __restrict__ results, float* __restrict__ best) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const CandMeta c  = cand[k];
  const int ns      = nsurv[k];
  const size_t row  = (size_t) k * (size_t) P.H;
  int bc = -1, bh = 0x7fffffff, bs = -1;
  long long bcost = 0;
  for (int s = lane; s < ns; s += 64) {
    const int cc = count[row + s], hh = hyp_id[row + s];
    const long long ss = cost[row + s];
    if (bs < 0 || better(cc, ss, hh, bc, bcost, bh)) bc = cc, bcost = ss, bh = hh, bs = s;
  }
  int nvalid = 0;
  for (int i = lane; i < c.n; i += 64) nvalid += pf[c.corr_begin + i].w != 0.f ? 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int oc = __shfl_xor(bc, off), oh = __shfl_xor(bh, off), os = __shfl_xor(bs, off);
    const long long ocost = __shfl_xor(bcost, off);
    nvalid += __shfl_xor(nvalid, off);
    if (os >= 0 && (bs < 0 || better(oc, ocost, oh, bc, bcost, bh))) bc = oc, bcost = ocost, bh = oh, bs = os;
  }
  if (lane != 0) return;
  const int s = P.dim == 3 ? 3 : 2;
  srrg2_consensus_result r;
  for (int i = 0; i < 12; ++i) r.moving_in_fixed[i] = 0.f;
  r.status = SRRG2_CONSENSUS_NO_HYPOTHESIS, r.best_hypothesis = -1, r.num_inliers = 0, r.cost = 0;
  r.num_pairs = c.n, r.num_valid_pairs = nvalid;
  r.num_degenerate = ctr[3 * k + 0], r.num_rejected = ctr[3 * k + 1], r.num_scored = ctr[3 * k + 2];
  r.cost_exponent = c.cost_exponent, r.reserved = 0;
  float* const b = best + 16 * (size_t) k;
  for (int i = 0; i < 16; ++i) b[i] = 0.f;
  if (bs >= 0) {
    const float* X = pose + (row + (size_t) bs) * 12;
    for (int i = 0; i < 12; ++i) b[i] = X[i];
    if (P.dim == 3) {
      for (int i = 0; i < 12; ++i) r.moving_in_fixed[i] = X[i];
    } else {
      r.moving_in_fixed[0] = X[0], r.moving_in_fixed[1] = X[1], r.moving_in_fixed[2] = X[3];
      r.moving_in_fixed[3] = X[4], r.moving_in_fixed[4] = X[5], r.moving_in_fixed[5] = X[7];
      r.moving_in_fixed[8] = 1.f;
    }
    const int need = P.min_inliers > s ? P.min_inliers : s;
    r.status = bc < need ? SRRG2_CONSENSUS_TOO_FEW_INLIERS : SRRG2_CONSENSUS_FOUND;
    r.best_hypothesis = bh, r.num_inliers = bc, r.cost = bcost;
    b[12] = r.status == SRRG2_CONSENSUS_FOUND ? 1.f : 0.f;
  }
  results[k] = r;
}

__global__ __launch_bounds__(256) void k_cns_flags(int P, float tau32, const float4* __restrict__ pf, const float4* __restrict__ pm,
                                                   const float* __restrict__ best, int* __restrict__ flags) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float4 f = pf[p], m = pm[p];
  const float* b = best + 16 * (size_t) __float_as_int(m.w);
  int flag = 0;
  if (b[12] != 0.f && f.w != 0.f) {
    float X[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) X[i] = b[i];
    flag = pair_error(X, m, f) <= tau32 * tau32 ? 1 : 0;
  }
  flags[p] = flag;
}

// offset: the exclusive scan of the flags (P + 1 words).  Threads [0, K] also write the offsets.
__global__ __launch_bounds__(256) void k_cns_scatter(int P, int K, const CandMeta* __restrict__ cand, const int* __restrict__ offset,
                                                     const srrg2_correspondence* __restrict__ corr, srrg2_correspondence* __restrict__ out,
                                                     long long cap, long long* __restrict__ offsets_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= K) offsets_out[p] = (long long) offset[p < K ? cand[p].corr_begin : P];
  if (p >= P) return;
  const int at = offset[p];
  if (offset[p + 1] == at || at < 0 || (long long) at >= cap) return;
  out[at] = corr[p];
}

size_t align16(size_t x) { return (x + 15) & ~(size_t) 15; }

}  // namespace

struct srrg2_consensus_s {
  int dim = 3, device = 0;
  hipStream_t stream = nullptr;
  DevBuf<char> in, out;        // the call's one upload and one download
  DevBuf<float4> pf, pm;       // packed pairs
  DevBuf<float> pose, best;    // 12 floats per (candidate, slot); 16 per candidate
  DevBuf<int> hyp_id, flags, scan_sums;
  DevBuf<long long> acc;       // zeroed per call: cost (K H words), count (K H ints), nsurv (K), ctr (3 K)
  srrg2amd::PinnedBuf<char> host_in, host_out;  // their pinned mirrors
  // The ordering is what this destructor is for: the stream retires before any buffer above is freed (the members free
  // themselves after this body).
  ~srrg2_consensus_s() {
    (void) hipSetDevice(device);
    if (stream) (void) hipStreamSynchronize(stream);
    if (stream) (void) hipStreamDestroy(stream);
  }
};

extern "C" void srrg2_consensus_default_params(srrg2_consensus_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->num_hypotheses      = 256;    // untuned
  p->inlier_distance     = 0.05f;  // untuned
  p->min_sample_distance = 0.1f;   // untuned
  p->length_check        = 1;
}

extern "C" int srrg2_consensus_create(int dim, int device, srrg2_consensus_h* out) {
  if (!out) return fail(SRRG2_E_INVALID, "consensus_create: out is NULL");
  if (dim != 2 && dim != 3) return fail(SRRG2_E_INVALID, "consensus_create: dim must be 2 or 3");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "consensus_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "consensus_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<srrg2_consensus_s> h(new srrg2_consensus_s());  // (a failure below deletes it)
  h->dim = dim, h->device = device;
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  *out = h.release();
  return 0;
}

extern "C" int srrg2_consensus_destroy(srrg2_consensus_h h) {
  delete h;  // (null: nothing to do)
  return 0;
}

extern "C" int srrg2_consensus_compute(srrg2_consensus_h h, const float* fixed, int fixed_stride_bytes, int num_fixed, int K,
                                       const float* moving, int moving_stride_bytes, const int32_t* moving_offsets, int mem,
                                       const srrg2_correspondence* correspondences, const int32_t* corr_offsets,
                                       const srrg2_consensus_params* p, srrg2_consensus_result* results,
                                       srrg2_correspondence* inliers_out, int64_t inlier_capacity, int64_t* inlier_offsets_out) {
  const std::string who = "consensus_compute: ";
  if (!h || !p) return fail(SRRG2_E_INVALID, who + "null handle or params");
  if (K < 0) return fail(SRRG2_E_INVALID, who + "K >= 0");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "mem must be HOST or DEVICE");
  if (p->num_hypotheses < 1 || p->num_hypotheses > 65536) return fail(SRRG2_E_INVALID, who + "num_hypotheses 1 .. 65536");
  if (!std::isfinite(p->inlier_distance) || !(p->inlier_distance > 0.f)) return fail(SRRG2_E_INVALID, who + "inlier_distance > 0 and finite");
  if (!std::isfinite(p->min_sample_distance) || !(p->min_sample_distance >= 0.f))
    return fail(SRRG2_E_INVALID, who + "min_sample_distance >= 0 and finite");
  if (p->min_inliers < 0) return fail(SRRG2_E_INVALID, who + "min_inliers >= 0");
  if (p->length_check != 0 && p->length_check != 1) return fail(SRRG2_E_INVALID, who + "length_check must be 0 or 1");
  if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  if (inlier_capacity < 0) return fail(SRRG2_E_INVALID, who + "inlier_capacity >= 0");
  if (num_fixed < 0) return fail(SRRG2_E_INVALID, who + "num_fixed >= 0");
  if (K == 0) {
    if (inlier_offsets_out) inlier_offsets_out[0] = 0;
    return 0;
  }
  if (!results || !moving_offsets || !corr_offsets) return fail(SRRG2_E_INVALID, who + "null results or offsets");
  if (K > 65535) return fail(SRRG2_E_UNSUPPORTED, who + "more than 65535 candidates in one call");
  const int dim = h->dim;
  if (moving_offsets[0] < 0 || corr_offsets[0] < 0) return fail(SRRG2_E_INVALID, who + "negative offsets");
  for (int k = 0; k < K; ++k)
    if (moving_offsets[k + 1] < moving_offsets[k] || corr_offsets[k + 1] < corr_offsets[k])
      return fail(SRRG2_E_INVALID, who + "decreasing offsets");
  const int m0 = moving_offsets[0], nm_all = moving_offsets[K] - m0;
  const int c0 = corr_offsets[0], P = corr_offsets[K] - c0;
  if ((num_fixed > 0 && !fixed) || (nm_all > 0 && !moving) || (P > 0 && !correspondences))
    return fail(SRRG2_E_INVALID, who + "null clouds or records where points or records exist");
  auto bad_stride = [&](int st, int n) { return n > 0 && (st % 4 != 0 || st < dim * 4); };
  if (bad_stride(fixed_stride_bytes, num_fixed) || bad_stride(moving_stride_bytes, nm_all))
    return fail(SRRG2_E_INVALID, who + "stride must be a multiple of 4 and >= dim*4");
  int n_max = 0;
  for (int k = 0; k < K; ++k) n_max = std::max(n_max, corr_offsets[k + 1] - corr_offsets[k]);
  const int H         = p->num_hypotheses;
  const int chunks    = (H + SCORE_CHUNK - 1) / SCORE_CHUNK;
  const long long tiles = ((long long) n_max + SCORE_TILE - 1) / SCORE_TILE;
  if (tiles * chunks > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "too many pairs times hypotheses for one launch");
  HIP_TRY(hipSetDevice(h->device));

  // ---- the one upload: candidates | records | (host clouds) ----
  const size_t fixed_bytes  = num_fixed > 0 ? (size_t) (num_fixed - 1) * (size_t) fixed_stride_bytes + (size_t) dim * 4 : 0;
  const size_t moving_bytes = nm_all > 0 ? (size_t) (nm_all - 1) * (size_t) moving_stride_bytes + (size_t) dim * 4 : 0;
  const size_t off_cand = 0, off_corr = align16(sizeof(CandMeta) * (size_t) K);
  const size_t off_fixed  = off_corr + align16(sizeof(srrg2_correspondence) * (size_t) P);
  const size_t off_moving = off_fixed + (mem == SRRG2_MEM_HOST ? align16(fixed_bytes) : 0);
  const size_t in_bytes   = off_moving + (mem == SRRG2_MEM_HOST ? align16(moving_bytes) : 0);
  const long long cap     = inliers_out ? std::min<long long>(inlier_capacity, P) : 0;
  const size_t out_res = 0, out_off = align16(sizeof(srrg2_consensus_result) * (size_t) K);
  const size_t out_rec   = out_off + align16(sizeof(long long) * ((size_t) K + 1));
  const size_t out_bytes = out_rec + sizeof(srrg2_correspondence) * (size_t) cap;
  const size_t KH        = (size_t) K * (size_t) H;
  const size_t acc_words = KH + (KH + 1) / 2 + ((size_t) 4 * K + 1) / 2;
  int rc;
  if ((rc = h->host_in.reserve(in_bytes, in_bytes / 8 + 256)) || (rc = h->host_out.reserve(out_bytes, out_bytes / 8 + 256)) ||
      (rc = h->in.reserve(in_bytes)) || (rc = h->out.reserve(out_bytes)) || (rc = h->pf.reserve((size_t) P + 1)) ||
      (rc = h->pm.reserve((size_t) P + 1)) || (rc = h->pose.reserve(KH * 12)) || (rc = h->best.reserve((size_t) K * 16)) ||
      (rc = h->hyp_id.reserve(KH)) || (rc = h->flags.reserve((size_t) P + 1)) ||
      (rc = h->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(P) + 2)) || (rc = h->acc.reserve(acc_words)))
    return rc;
  const double tau = (double) p->inlier_distance, msd = (double) p->min_sample_distance;
  CandMeta* const hc = reinterpret_cast<CandMeta*>(h->host_in.p + off_cand);
  for (int k = 0; k < K; ++k) {
    CandMeta& c = hc[k];
    c.corr_begin = corr_offsets[k] - c0, c.n = corr_offsets[k + 1] - corr_offsets[k];
    c.mov_begin = moving_offsets[k] - m0, c.mov_n = moving_offsets[k + 1] - moving_offsets[k];
    c.cost_exponent = dm::fixed_point_exponent(c.n, tau * tau);
    c.scale         = dm::pow2(c.cost_exponent);
    c.pad           = 0;
  }
  if (P > 0) std::memcpy(h->host_in.p + off_corr, correspondences + c0, sizeof(srrg2_correspondence) * (size_t) P);
  const char* const moving0 = reinterpret_cast<const char*>(moving) + (size_t) m0 * (size_t) moving_stride_bytes;
  const char *d_fixed = reinterpret_cast<const char*>(fixed), *d_moving = moving0;
  if (mem == SRRG2_MEM_HOST) {
    if (fixed_bytes) std::memcpy(h->host_in.p + off_fixed, fixed, fixed_bytes);
    if (moving_bytes) std::memcpy(h->host_in.p + off_moving, moving0, moving_bytes);
    d_fixed = h->in.p + off_fixed, d_moving = h->in.p + off_moving;
  }
  hipStream_t st = h->stream;
  HIP_TRY(hipMemcpyAsync(h->in.p, h->host_in.p, in_bytes, hipMemcpyHostToDevice, st));
  const CandMeta* const d_cand             = reinterpret_cast<const CandMeta*>(h->in.p + off_cand);
  const srrg2_correspondence* const d_corr = reinterpret_cast<const srrg2_correspondence*>(h->in.p + off_corr);
  long long* const d_cost = h->acc.p;
  int* const d_count      = reinterpret_cast<int*>(h->acc.p + KH);
  int* const d_nsurv      = reinterpret_cast<int*>(h->acc.p + KH + (KH + 1) / 2);
  int* const d_ctr        = d_nsurv + K;
  srrg2_consensus_result* const d_res = reinterpret_cast<srrg2_consensus_result*>(h->out.p + out_res);
  long long* const d_offsets          = reinterpret_cast<long long*>(h->out.p + out_off);
  srrg2_correspondence* const d_recs  = reinterpret_cast<srrg2_correspondence*>(h->out.p + out_rec);
  CnsParams C;
  C.dim = dim, C.H = H, C.K = K, C.length_check = p->length_check, C.min_inliers = p->min_inliers, C.seed = p->seed, C.tau32 = p->inlier_distance;
  C.tau = tau, C.msd2 = msd * msd;

  HIP_TRY(hipMemsetAsync(h->acc.p, 0, acc_words * sizeof(long long), st));
  if (P > 0)
    hipLaunchKernelGGL(k_cns_gather, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, st, P, K, dim, d_cand, d_corr, d_fixed,
                       fixed_stride_bytes, num_fixed, d_moving, moving_stride_bytes, h->pf.p, h->pm.p);
  const dim3 hyp_grid((unsigned) ((H + HYP_THREADS - 1) / HYP_THREADS), (unsigned) K);
  if (dim == 3)
    hipLaunchKernelGGL(k_cns_hyp<3>, hyp_grid, dim3(HYP_THREADS), 0, st, C, d_cand, h->pf.p, h->pm.p, d_nsurv, d_ctr, h->pose.p, h->hyp_id.p);
  else
    hipLaunchKernelGGL(k_cns_hyp<2>, hyp_grid, dim3(HYP_THREADS), 0, st, C, d_cand, h->pf.p, h->pm.p, d_nsurv, d_ctr, h->pose.p, h->hyp_id.p);
  if (tiles > 0)
    hipLaunchKernelGGL(k_cns_score, dim3((unsigned) (tiles * chunks), (unsigned) K), dim3(SCORE_THREADS), 0, st, H, chunks, C.tau32, d_cand,
                       h->pf.p, h->pm.p, d_nsurv, h->pose.p, d_count, d_cost);
  hipLaunchKernelGGL(k_cns_select, dim3((unsigned) K), dim3(64), 0, st, C, d_cand, h->pf.p, d_nsurv, d_ctr, h->pose.p, h->hyp_id.p, d_count,
                     d_cost, d_res, h->best.p);
  if (P > 0) {
    hipLaunchKernelGGL(k_cns_flags, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, st, P, C.tau32, h->pf.p, h->pm.p, h->best.p, h->flags.p);
    srrg2amd::launch_exclusive_scan(h->flags.p, P, h->scan_sums.p, h->scan_sums.p + srrg2amd::scan_num_blocks(P) + 1, st);
  } else {
    HIP_TRY(hipMemsetAsync(h->flags.p, 0, sizeof(int), st));
  }
  const int scatter_threads = std::max(P, K + 1);
  hipLaunchKernelGGL(k_cns_scatter, dim3((unsigned) ((scatter_threads + 255) / 256)), dim3(256), 0, st, P, K, d_cand, h->flags.p, d_corr, d_recs,
                     cap, d_offsets);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->host_out.p, h->out.p, out_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the call's one host wait: results, offsets and records together

  const long long* const offs = reinterpret_cast<const long long*>(h->host_out.p + out_off);
  const long long total       = offs[K];
  if (total < 0 || total > P) return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
  std::memcpy(results, h->host_out.p + out_res, sizeof(srrg2_consensus_result) * (size_t) K);
  if (inlier_offsets_out) std::memcpy(inlier_offsets_out, offs, sizeof(long long) * ((size_t) K + 1));
  const long long give = std::min(total, cap);
  if (give > 0) std::memcpy(inliers_out, h->host_out.p + out_rec, sizeof(srrg2_correspondence) * (size_t) give);
  return 0;
}
