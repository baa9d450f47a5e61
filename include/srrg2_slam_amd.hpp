// srrg2_slam_amd.hpp -- header-only C++17 mirror of the reference's aligner interface over the C ABI.
//
// The reference is C++ (S/registration/aligners/*.h); this header gives its callers the same vocabulary --
// class and method names, argument meaning, exceptions for misuse, AlignerBase::Status for outcomes -- without
// srrg2_core / Eigen, so it compiles in this repository.  INTEGRATION.md shows how the same calls sit inside real
// srrg2_core types.  Everything forwards to include/srrg2_slam_amd.h; no arithmetic of the hot path lives here.
//
//   MultiAligner                    MultiAlignerBase_<Variable>            multi_aligner.h:19-150, multi_aligner_impl.cpp
//   AlignerTerminationCriteria      AlignerTerminationCriteriaStandard_    aligner_termination_criteria.h:33-71
//   MotionModelConstantVelocity     MotionModelConstantVelocity<Estimate>  motion_models/motion_model_constant_velocity.hpp
//   AlignerSliceMotionModel         AlignerSliceMotionModel_               aligner_slice_motion_model.hpp:13-92
//   AlignerSliceOdomPrior           AlignerSliceOdom{2,3}DPrior            aligner_slice_odometry_prior.{h,cpp}
//   Scene / SceneClipperBall / MergerCorrespondenceHomo                    mapping/scene_clipper.h, merger_correspondence_homo.h
//   DescriptorDatabase              srrg_hbst::BinaryTree256 in MultiLoopDetectorHBST_  multi_loop_detector_hbst_impl.cpp:41-197
//   (loop-closure drivers and the pose graph: srrg2_slam_amd_loop_closure.hpp)
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "srrg2_slam_amd.h"

namespace srrg2_slam_amd {

// ---- transforms: row-major 3x4 (SE3) / 3x3 (SE2) float, like Isometry3f / Isometry2f ---------------------------
template <int DIM>
struct Isometry {
  static constexpr int N = DIM == 2 ? 9 : 12;
  std::array<float, N> m{};
  static Isometry Identity() {
    Isometry T;
    if (DIM == 2) {
      T.m = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    } else {
      const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      std::memcpy(T.m.data(), I, sizeof(I));
    }
    return T;
  }
  const float* data() const { return m.data(); }
  float* data() { return m.data(); }
  Isometry inverse() const {
    Isometry R;
    if (DIM == 2) {
      R.m = {m[0], m[3], -(m[0] * m[2] + m[3] * m[5]), m[1], m[4], -(m[1] * m[2] + m[4] * m[5]), 0, 0, 1};
    } else {
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R.m[i * 4 + j] = m[j * 4 + i];
        R.m[i * 4 + 3] = -(m[0 * 4 + i] * m[3] + m[1 * 4 + i] * m[7] + m[2 * 4 + i] * m[11]);
      }
    }
    return R;
  }
  Isometry operator*(const Isometry& B) const {
    Isometry C;
    if (DIM == 2) {
      for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 2; ++j) C.m[i * 3 + j] = m[i * 3] * B.m[j] + m[i * 3 + 1] * B.m[3 + j];
        C.m[i * 3 + 2] = m[i * 3] * B.m[2] + m[i * 3 + 1] * B.m[5] + m[i * 3 + 2];
      }
      C.m[6] = 0; C.m[7] = 0; C.m[8] = 1;
    } else {
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
          C.m[i * 4 + j] = m[i * 4] * B.m[j] + m[i * 4 + 1] * B.m[4 + j] + m[i * 4 + 2] * B.m[8 + j];
        C.m[i * 4 + 3] = m[i * 4] * B.m[3] + m[i * 4 + 1] * B.m[7] + m[i * 4 + 2] * B.m[11] + m[i * 4 + 3];
      }
    }
    return C;
  }
};
using Isometry2f = Isometry<2>;
using Isometry3f = Isometry<3>;

struct AlignerBase {
  enum Status { Success = 0, NotEnoughCorrespondences = 1, NotEnoughInliers = 2, Fail = 3 };  // aligner.h:23-28
};

inline void check(int rc) {
  if (rc != 0) throw std::runtime_error(srrg2_amd_last_error());  // the reference throws std::runtime_error too
}

using Correspondence       = srrg2_correspondence;
using CorrespondenceVector = std::vector<Correspondence>;
using IterationStats       = srrg2_iteration_stats;
using IterationStatsVector = std::vector<IterationStats>;

// ---- MultiAlignerBase_<Variable> -------------------------------------------------------------------------------
template <int VARIABLE_KIND>
class MultiAligner_ : public AlignerBase {
public:
  static constexpr int Dim = VARIABLE_KIND == SRRG2_SE2_RIGHT ? 2 : 3;
  using EstimateType       = Isometry<Dim>;

  // PARAMs (aligner.h:30; multi_aligner.h:45-57)
  int param_max_iterations                    = 10;
  int param_min_num_inliers                   = 10;
  bool param_enable_inlier_only_runs          = false;
  bool param_keep_only_inlier_correspondences = false;

  explicit MultiAligner_(int device = 0) { check(srrg2_aligner_create(VARIABLE_KIND, device, &_h)); }
  ~MultiAligner_() { srrg2_aligner_destroy(_h); }
  MultiAligner_(const MultiAligner_&)            = delete;
  MultiAligner_& operator=(const MultiAligner_&) = delete;

  // param_slice_processors.pushBack(slice)
  int addSlice(const srrg2_slice_config& c) {
    int idx = -1;
    check(srrg2_aligner_add_slice(_h, &c, &idx));
    _nslices = idx + 1;
    return idx;
  }
  int numSlices() const { return _nslices; }
  static srrg2_slice_config defaultSliceConfig() {
    srrg2_slice_config c;
    srrg2_slice_default_config(&c, VARIABLE_KIND);
    return c;
  }
  // param_termination_criteria.setValue(...) / nullptr
  void setTerminationCriteria(const srrg2_termination_params* p) { check(srrg2_aligner_set_termination(_h, p)); }

  // slice->setFixed / setMoving of the named cloud (multi_aligner_impl.cpp:8-24): raw strided arrays
  void setFixed(int slice, const float* coords, int stride_bytes, const float* normals, int normal_stride_bytes, int n,
                int mem = SRRG2_MEM_HOST) {
    check(srrg2_aligner_set_fixed(_h, slice, coords, stride_bytes, normals, normal_stride_bytes, n, mem));
  }
  void setMoving(int slice, const float* coords, int stride_bytes, const float* normals, int normal_stride_bytes, int n,
                 int mem = SRRG2_MEM_HOST) {
    check(srrg2_aligner_set_moving(_h, slice, coords, stride_bytes, normals, normal_stride_bytes, n, mem));
  }
  // factor->setCorrespondences(corrs) of a SRRG2_FINDER_CORRESPONDENCES slice: locked during compute()
  // (MultiLoopDetectorHBST_::_computeAlignments, multi_loop_detector_hbst_impl.cpp:330,343)
  void setCorrespondences(int slice, const std::vector<srrg2_correspondence>& c) {
    check(srrg2_aligner_set_correspondences(_h, slice, c.data(), (int) c.size()));
  }
  // slice->setSensorInRobot(); the reference re-reads the platform TF on every setMovingInFixed
  // (aligner_slice_processor_impl.cpp:20-36): call it whenever the sensor pose changed
  void setSensorInRobot(int slice, const EstimateType& T) { check(srrg2_aligner_set_sensor_in_robot(_h, slice, T.data())); }
  void setPriorMeasurement(int slice, const EstimateType& Z) { check(srrg2_aligner_set_prior_measurement(_h, slice, Z.data())); }
  // ONE alignment over the ranks of a communicator, sharded by moving points (srrg2_aligner_set_point_shard):
  // `reduce` adds / maximises the device buffer in place over all ranks on the given stream (e.g. ncclAllReduce);
  // total_moving_points counts the moving points of all ranks.  reduce == nullptr switches the mode off.
  void setPointShard(srrg2_reduce_fn reduce, void* user, int64_t total_moving_points) {
    check(srrg2_aligner_set_point_shard(_h, reduce, user, total_moving_points));
  }

  void setMovingInFixed(const EstimateType& X) { check(srrg2_aligner_set_moving_in_fixed(_h, X.data())); }
  const EstimateType& movingInFixed() const {
    check(srrg2_aligner_get_moving_in_fixed(_h, _X.data()));
    return _X;
  }

  void compute() {  // multi_aligner_impl.cpp:47-95, blocking
    srrg2_aligner_params p{param_max_iterations, param_min_num_inliers, param_enable_inlier_only_runs ? 1 : 0,
                           param_keep_only_inlier_correspondences ? 1 : 0};
    check(srrg2_aligner_set_params(_h, &p));
    int st = Fail;
    check(srrg2_aligner_compute(_h, &st));
    _status = static_cast<Status>(st);
    int n   = 0;
    check(srrg2_aligner_get_iteration_stats(_h, nullptr, &n));
    _iteration_stats.resize((size_t) n);
    if (n) check(srrg2_aligner_get_iteration_stats(_h, _iteration_stats.data(), &n));
  }
  // K independent alignments against the fixed scene already set: the loop body of
  // MultiLoopDetectorBruteForce_::compute (multi_loop_detector_brute_force_impl.cpp:64-91) for all candidates at once.
  // clouds: K pointers to packed Dim-float records with their sizes; normals may be empty (none) or K pointers.
  std::vector<srrg2_batch_result> computeBatch(const std::vector<const float*>& clouds, const std::vector<int>& sizes,
                                               const std::vector<const float*>& normals,
                                               const std::vector<EstimateType>& guesses) {
    const int K = (int) clouds.size();
    if ((int) sizes.size() != K || (int) guesses.size() != K || (!normals.empty() && (int) normals.size() != K))
      throw std::runtime_error("MultiAligner_::computeBatch|inconsistent argument sizes");
    std::vector<int32_t> offsets((size_t) K + 1, 0);
    for (int k = 0; k < K; ++k) offsets[(size_t) k + 1] = offsets[(size_t) k] + sizes[(size_t) k];
    std::vector<float> coords((size_t) offsets[(size_t) K] * Dim), nrm;
    if (!normals.empty()) nrm.resize(coords.size());
    std::vector<float> g((size_t) K * EstimateType::N);
    for (int k = 0; k < K; ++k) {
      std::memcpy(coords.data() + (size_t) offsets[(size_t) k] * Dim, clouds[(size_t) k], sizeof(float) * (size_t) sizes[(size_t) k] * Dim);
      if (!normals.empty())
        std::memcpy(nrm.data() + (size_t) offsets[(size_t) k] * Dim, normals[(size_t) k], sizeof(float) * (size_t) sizes[(size_t) k] * Dim);
      std::memcpy(g.data() + (size_t) k * EstimateType::N, guesses[(size_t) k].data(), sizeof(float) * EstimateType::N);
    }
    srrg2_aligner_params p{param_max_iterations, param_min_num_inliers, param_enable_inlier_only_runs ? 1 : 0,
                           param_keep_only_inlier_correspondences ? 1 : 0};
    check(srrg2_aligner_set_params(_h, &p));
    std::vector<srrg2_batch_result> results((size_t) K);
    if (K)
      check(srrg2_aligner_compute_batch(_h, K, coords.data(), Dim * 4, normals.empty() ? nullptr : nrm.data(), Dim * 4,
                                        offsets.data(), SRRG2_MEM_HOST, g.data(), results.data()));
    return results;
  }
  // K independent alignments, pair k = fixed cloud k against moving cloud k (srrg2_align_pairs): what K x { setFixed;
  // setMoving; setMovingInFixed; compute() } returns, in one call, the slice's own fixed cloud untouched.
  // fixed / moving: K pointers to packed Dim-float records with their sizes; normals may be empty (none) or K pointers.
  std::vector<srrg2_batch_result> computeBatchPairs(const std::vector<const float*>& fixed, const std::vector<int>& fixed_sizes,
                                                    const std::vector<const float*>& fixed_normals,
                                                    const std::vector<const float*>& moving, const std::vector<int>& moving_sizes,
                                                    const std::vector<const float*>& moving_normals,
                                                    const std::vector<EstimateType>& guesses) {
    const int K = (int) fixed.size();
    if ((int) fixed_sizes.size() != K || (int) moving.size() != K || (int) moving_sizes.size() != K || (int) guesses.size() != K ||
        (!fixed_normals.empty() && (int) fixed_normals.size() != K) || (!moving_normals.empty() && (int) moving_normals.size() != K))
      throw std::runtime_error("MultiAligner_::computeBatchPairs|inconsistent argument sizes");
    auto pack = [K](const std::vector<const float*>& clouds, const std::vector<const float*>& normals, const std::vector<int>& sizes,
                    std::vector<int32_t>& offsets, std::vector<float>& coords, std::vector<float>& nrm) {
      offsets.assign((size_t) K + 1, 0);
      for (int k = 0; k < K; ++k) offsets[(size_t) k + 1] = offsets[(size_t) k] + sizes[(size_t) k];
      coords.resize((size_t) offsets[(size_t) K] * Dim);
      if (!normals.empty()) nrm.resize(coords.size());
      for (int k = 0; k < K; ++k) {
        const size_t off = (size_t) offsets[(size_t) k] * Dim, bytes = sizeof(float) * (size_t) sizes[(size_t) k] * Dim;
        if (bytes) std::memcpy(coords.data() + off, clouds[(size_t) k], bytes);
        if (bytes && !normals.empty()) std::memcpy(nrm.data() + off, normals[(size_t) k], bytes);
      }
    };
    std::vector<int32_t> foff, moff;
    std::vector<float> fc, fn, mc, mn;
    pack(fixed, fixed_normals, fixed_sizes, foff, fc, fn);
    pack(moving, moving_normals, moving_sizes, moff, mc, mn);
    std::vector<float> g((size_t) K * EstimateType::N);
    for (int k = 0; k < K; ++k) std::memcpy(g.data() + (size_t) k * EstimateType::N, guesses[(size_t) k].data(), sizeof(float) * EstimateType::N);
    srrg2_aligner_params p{param_max_iterations, param_min_num_inliers, param_enable_inlier_only_runs ? 1 : 0,
                           param_keep_only_inlier_correspondences ? 1 : 0};
    check(srrg2_aligner_set_params(_h, &p));
    std::vector<srrg2_batch_result> results((size_t) K);
    if (K)
      check(srrg2_align_pairs(_h, K, fc.data(), Dim * 4, fixed_normals.empty() ? nullptr : fn.data(), Dim * 4, foff.data(), mc.data(),
                              Dim * 4, moving_normals.empty() ? nullptr : mn.data(), Dim * 4, moff.data(), SRRG2_MEM_HOST, g.data(),
                              results.data()));
    return results;
  }
  // one cue slice's K moving clouds in a computeBatchSlices call: K pointers to packed Dim-float records with their sizes,
  // normals empty (none) or K pointers
  struct SliceClouds {
    int slice = 0;
    std::vector<const float*> clouds;
    std::vector<int> sizes;
    std::vector<const float*> normals;
  };
  // K independent alignments against the bound fixed clouds, every cue slice with a moving cloud of its own per alignment
  // (srrg2_align_batch_slices): what K x { setMoving per slice; setMovingInFixed; compute() } returns, in one call.  `slices`:
  // the cue slices that own their clouds (a slice bound by shareClouds takes its source's; prior slices have no entry).
  std::vector<srrg2_batch_result> computeBatchSlices(const std::vector<SliceClouds>& slices, const std::vector<EstimateType>& guesses) {
    const int K = (int) guesses.size();
    std::vector<srrg2_batch_slice_clouds> entries((size_t) std::max(_nslices, 1));
    std::memset(entries.data(), 0, sizeof(srrg2_batch_slice_clouds) * entries.size());
    std::vector<std::vector<int32_t>> offsets(slices.size());
    std::vector<std::vector<float>> coords(slices.size()), nrm(slices.size());
    for (size_t i = 0; i < slices.size(); ++i) {
      const SliceClouds& sc = slices[i];
      if (sc.slice < 0 || sc.slice >= _nslices) throw std::runtime_error("MultiAligner_::computeBatchSlices|bad slice index");
      if ((int) sc.clouds.size() != K || (int) sc.sizes.size() != K || (!sc.normals.empty() && (int) sc.normals.size() != K))
        throw std::runtime_error("MultiAligner_::computeBatchSlices|inconsistent argument sizes");
      offsets[i].assign((size_t) K + 1, 0);
      for (int k = 0; k < K; ++k) offsets[i][(size_t) k + 1] = offsets[i][(size_t) k] + sc.sizes[(size_t) k];
      coords[i].resize((size_t) offsets[i][(size_t) K] * Dim);
      if (!sc.normals.empty()) nrm[i].resize(coords[i].size());
      for (int k = 0; k < K; ++k) {
        const size_t off = (size_t) offsets[i][(size_t) k] * Dim, bytes = sizeof(float) * (size_t) sc.sizes[(size_t) k] * Dim;
        if (bytes) std::memcpy(coords[i].data() + off, sc.clouds[(size_t) k], bytes);
        if (bytes && !sc.normals.empty()) std::memcpy(nrm[i].data() + off, sc.normals[(size_t) k], bytes);
      }
      srrg2_batch_slice_clouds& e = entries[(size_t) sc.slice];
      e.coords              = coords[i].data();
      e.coord_stride_bytes  = Dim * 4;
      e.normals             = sc.normals.empty() ? nullptr : nrm[i].data();
      e.normal_stride_bytes = Dim * 4;
      e.offsets             = offsets[i].data();
    }
    std::vector<float> g((size_t) K * EstimateType::N);
    for (int k = 0; k < K; ++k) std::memcpy(g.data() + (size_t) k * EstimateType::N, guesses[(size_t) k].data(), sizeof(float) * EstimateType::N);
    srrg2_aligner_params p{param_max_iterations, param_min_num_inliers, param_enable_inlier_only_runs ? 1 : 0,
                           param_keep_only_inlier_correspondences ? 1 : 0};
    check(srrg2_aligner_set_params(_h, &p));
    std::vector<srrg2_batch_result> results((size_t) K);
    if (K) check(srrg2_align_batch_slices(_h, K, _nslices, entries.data(), SRRG2_MEM_HOST, g.data(), results.data()));
    return results;
  }
  // slice `slice` reads the clouds of slice `source` (two slices with the same fixed_slice_name / moving_slice_name bind to
  // the same clouds of the scene: aligner_slice_processor_base_impl.cpp:27-50); -1: clouds of its own again
  void shareClouds(int slice, int source) { check(srrg2_aligner_share_clouds(_h, slice, source)); }
  Status status() const { return _status; }
  const IterationStatsVector& iterationStats() const { return _iteration_stats; }
  // H = sum w J^T J of the last Gauss-Newton iteration of the last compute() (the solver's system after
  // multi_aligner_impl.cpp:112-116), D x D row-major, D = 3 (SE2) or 6 (SE3)
  std::vector<float> information() {
    std::vector<float> H(36, 0.f);
    check(srrg2_aligner_get_information(_h, H.data()));
    return H;
  }
  int numCorrespondences() {
    int n = 0;
    check(srrg2_aligner_num_correspondences(_h, &n));
    return n;
  }
  // SRRG2_PATH_* bits of the launch path the last compute() took (strategy only: results never depend on it)
  int lastComputePath() {
    int32_t f = 0;
    check(srrg2_aligner_last_compute_path(_h, &f));
    return (int) f;
  }
  CorrespondenceVector correspondences(int slice) {
    int n = 0;
    check(srrg2_aligner_get_correspondences(_h, slice, nullptr, &n));
    CorrespondenceVector v((size_t) n);
    if (n) check(srrg2_aligner_get_correspondences(_h, slice, v.data(), &n));
    return v;
  }
  srrg2_aligner_h handle() { return _h; }

private:
  srrg2_aligner_h _h = nullptr;
  int _nslices       = 0;
  Status _status     = Fail;  // aligner.h:56
  mutable EstimateType _X = EstimateType::Identity();
  IterationStatsVector _iteration_stats;
};
using MultiAligner2D   = MultiAligner_<SRRG2_SE2_RIGHT>;        // multi_aligner.h:152-158
using MultiAligner3D   = MultiAligner_<SRRG2_SE3_EULER_RIGHT>;
using MultiAligner3DQR = MultiAligner_<SRRG2_SE3_QUAT_RIGHT>;

// ---- MotionModelConstantVelocity (motion_model_constant_velocity.hpp:17-46) -----------------------------------------
template <int DIM>
class MotionModelConstantVelocity {
public:
  using EstimateType = Isometry<DIM>;
  const EstimateType& estimate() const { return _motion; }
  void compute() { _motion = _robot_in_local_map_previous.inverse() * _robot_in_local_map; }
  void setRobotInLocalMap(const EstimateType& T) {
    _robot_in_local_map_previous = _robot_in_local_map;
    _robot_in_local_map          = T;
  }
  void shiftTrackerEstimate(const EstimateType& estimate) {
    _robot_in_local_map_previous = estimate * (_robot_in_local_map_previous.inverse() * _robot_in_local_map);
    _robot_in_local_map          = estimate;
  }
  void setRobotInLocalMapPrevious(const EstimateType& T) { _robot_in_local_map_previous = T; }
  void clear() {
    _motion = _robot_in_local_map = _robot_in_local_map_previous = EstimateType::Identity();
  }

private:
  EstimateType _motion                      = EstimateType::Identity();
  EstimateType _robot_in_local_map          = EstimateType::Identity();
  EstimateType _robot_in_local_map_previous = EstimateType::Identity();
};
using MotionModelConstantVelocity2D = MotionModelConstantVelocity<2>;
using MotionModelConstantVelocity3D = MotionModelConstantVelocity<3>;

// ---- AlignerSliceMotionModel_ (aligner_slice_motion_model.hpp:44-79) -----------------------------------------------------
template <typename AlignerType>
class AlignerSliceMotionModel {
public:
  using EstimateType = typename AlignerType::EstimateType;
  using PoseBuffer   = std::deque<EstimateType>;  // StdDequeEigenIsometry3f
  MotionModelConstantVelocity<AlignerType::Dim>* param_motion_model = nullptr;

  explicit AlignerSliceMotionModel(AlignerType& aligner) : _aligner(aligner) {
    srrg2_slice_config c       = AlignerType::defaultSliceConfig();
    c.kind                     = SRRG2_SLICE_PRIOR;
    c.finder                   = SRRG2_FINDER_NONE;
    c.prior_sets_initial_guess = 1;  // init() calls aligner->setMovingInFixed(_motion_inverse), :69-70
    _slice                     = aligner.addSlice(c);
  }
  void setFixed(const PoseBuffer* fixed_slice) { _fixed_slice = fixed_slice; }
  void init() {
    if (!param_motion_model) throw std::runtime_error("AlignerSliceMotionModel_::init|ERROR: no motion model is set");
    if (!_fixed_slice) throw std::runtime_error("AlignerSliceMotionModel_::init|ERROR: no fixed pose set");
    if (!_fixed_slice->empty()) {
      param_motion_model->setRobotInLocalMap(_fixed_slice->back());
      if (_fixed_slice->size() > 1) param_motion_model->setRobotInLocalMapPrevious(*(_fixed_slice->end() - 2));
      param_motion_model->compute();
    }
    _motion_inverse = param_motion_model->estimate().inverse();
    _aligner.setPriorMeasurement(_slice, _motion_inverse);
  }

private:
  AlignerType& _aligner;
  int _slice                     = -1;
  const PoseBuffer* _fixed_slice = nullptr;
  EstimateType _motion_inverse   = EstimateType::Identity();
};

// ---- AlignerSliceOdom{2,3}DPrior (aligner_slice_odometry_prior.cpp:6-37) ------------------------------------------------
template <typename AlignerType>
class AlignerSliceOdomPrior {
public:
  using EstimateType = typename AlignerType::EstimateType;
  explicit AlignerSliceOdomPrior(AlignerType& aligner) : _aligner(aligner) {
    srrg2_slice_config c = AlignerType::defaultSliceConfig();
    c.kind               = SRRG2_SLICE_PRIOR;
    c.finder             = SRRG2_FINDER_NONE;
    _slice               = aligner.addSlice(c);
  }
  void setFixed(const EstimateType* T) { _fixed_slice = T; }
  void setMoving(const EstimateType* T) { _moving_slice = T; }
  void init() {
    if (!_fixed_slice) throw std::runtime_error("AlignerSliceProcessor_::factor| no fixed");
    if (!_moving_slice) throw std::runtime_error("AlignerSliceProcessor_::factor| no moving");
    EstimateType delta = EstimateType::Identity();
    if (_count > 1) delta = _fixed_slice->inverse() * (*_moving_slice);
    _aligner.setPriorMeasurement(_slice, delta);
    ++_count;
  }

private:
  AlignerType& _aligner;
  int _slice                        = -1;
  int _count                        = 0;
  const EstimateType* _fixed_slice  = nullptr;
  const EstimateType* _moving_slice = nullptr;
};

// ---- scene slices in device memory: SceneClipper_ / MergerCorrespondenceHomo_ ------
//   Scene                       a PointNormal{2,3}f cloud living in HBM (LocalMap scene slice / measurement); with setFeatures
//                               a PointIntensityDescriptor{2,3}f one: descriptor + intensity travel through clip and merge
//   SceneClipperBall            SceneClipper_<Estimate, Scene>              S/mapping/scene_clipper.h:17-122
//   SceneClipperProjective      the same interface, projective policy (3-D): what a pinhole camera sees of the scene
//   SceneClipperScan            the same interface, scan policy (2-D): what a planar laser scanner sees of the scene
//   SceneClipperSpherical       the same interface, spherical policy (3-D): what a spinning lidar sees of the scene
//   MergerCorrespondenceHomo    MergerCorrespondenceHomo_<Estimate, Scene>  S/mapping/merger_correspondence_homo.h
template <int DIM>
class Scene {
public:
  explicit Scene(int device = 0) { check(srrg2_scene_create(DIM, device, &_h)); }
  ~Scene() { srrg2_scene_destroy(_h); }
  Scene(const Scene&)            = delete;
  Scene& operator=(const Scene&) = delete;
  void set(const float* coords, int stride_bytes, const float* normals, int normal_stride_bytes, int n,
           int mem = SRRG2_MEM_HOST) {
    check(srrg2_scene_set(_h, coords, stride_bytes, normals, normal_stride_bytes, n, mem));
  }
  int size() const {
    int n = 0;
    check(srrg2_scene_size(_h, &n));
    return n;
  }
  // packed DIM-float records
  void get(std::vector<float>& coords, std::vector<float>& normals) const {
    int n = size();
    coords.assign((size_t) n * DIM, 0.f);
    normals.assign((size_t) n * DIM, 0.f);
    check(srrg2_scene_get(_h, coords.data(), normals.data(), n, &n));
  }
  // device float4 arrays (stride 16 bytes), e.g. for MultiAligner_::setMoving(..., SRRG2_MEM_DEVICE)
  void deviceArrays(const float*& coords, const float*& normals, int& n) const {
    check(srrg2_scene_device_arrays(_h, &coords, &normals, &n));
  }
  // per-point features: rows of SRRG2_DESCRIPTOR_BYTES bytes and / or floats, nullptr = that field is absent (both: dropped);
  // n must be size().  Strides in bytes.
  void setFeatures(const uint8_t* descriptors, int descriptor_stride_bytes, const float* intensity, int intensity_stride_bytes,
                   int n, int mem = SRRG2_MEM_HOST) {
    check(srrg2_scene_set_features(_h, descriptors, descriptor_stride_bytes, intensity, intensity_stride_bytes, n, mem));
  }
  bool hasDescriptors() const {
    int d = 0;
    check(srrg2_scene_has_features(_h, &d, nullptr));
    return d != 0;
  }
  bool hasIntensity() const {
    int i = 0;
    check(srrg2_scene_has_features(_h, nullptr, &i));
    return i != 0;
  }
  // packed rows of 32 bytes / floats; a field the scene does not carry comes back empty
  void getFeatures(std::vector<uint8_t>& descriptors, std::vector<float>& intensity) const {
    int n = size();
    descriptors.assign(hasDescriptors() ? (size_t) n * SRRG2_DESCRIPTOR_BYTES : 0, 0);
    intensity.assign(hasIntensity() ? (size_t) n : 0, 0.f);
    check(srrg2_scene_get_features(_h, descriptors.empty() ? nullptr : descriptors.data(),
                                   intensity.empty() ? nullptr : intensity.data(), n, &n));
  }
  // device arrays (nullptr for an absent field), valid until the scene is next modified
  void deviceFeatures(const uint8_t*& descriptors, const float*& intensity, int& n) const {
    check(srrg2_scene_device_features(_h, &descriptors, &intensity, &n));
  }
  // normals from the PCA of every point's radius neighbourhood (srrg2_scene_estimate_normals; defaults:
  // srrg2_normals_default_params(&p, DIM)).  curvature: per point as indexed BEFORE the call, NaN where none was formed.
  srrg2_normals_result estimateNormals(const srrg2_normals_params& p, std::vector<float>* curvature = nullptr) {
    srrg2_normals_result r;
    if (curvature) curvature->assign((size_t) size(), 0.f);
    check(srrg2_scene_estimate_normals(_h, &p, curvature && !curvature->empty() ? curvature->data() : nullptr, &r));
    return r;
  }
  // voxel-grid decimation into `dst` (srrg2_scene_voxelize; defaults: srrg2_voxel_default_params(&p)): this scene stays as it is,
  // dst.globalIndices() names every emitted point's representative here.  counts: points per emitted cell.
  srrg2_voxel_result voxelize(const srrg2_voxel_params& p, Scene<DIM>& dst, std::vector<int32_t>* counts = nullptr) {
    srrg2_voxel_result r;
    if (counts) counts->assign((size_t) size(), 0);
    check(srrg2_scene_voxelize(_h, &p, dst._h, counts && !counts->empty() ? counts->data() : nullptr, &r));
    if (counts) counts->resize((size_t) r.num_voxels);
    return r;
  }
  // local -> global indices of the last clip / decimation INTO this scene
  std::vector<int> globalIndices() const {
    int n = 0;
    check(srrg2_scene_global_indices(_h, nullptr, &n));
    std::vector<int> g((size_t) n);
    if (n > 0) check(srrg2_scene_global_indices(_h, g.data(), &n));
    return g;
  }
  srrg2_scene_h handle() const { return _h; }

private:
  srrg2_scene_h _h = nullptr;
};

// ---- scene clippers: SceneClipper_ (S/mapping/scene_clipper.h:17-122) with the ball policy and the three sensor views ----------
// what the four share: the full scene, the clipped scene, the pose, status() and globalIndices()
template <int DIM>
class SceneClipperBase_ {
public:
  enum Status { Error = 0, Successful = 1, Ready = 2 };  // scene_clipper.h:24-28
  using EstimateType = Isometry<DIM>;
  using SceneType    = Scene<DIM>;
  void setFullScene(SceneType* s) { _full = s; }
  void setClippedSceneInRobot(SceneType* s) { _clipped = s; }
  void setRobotInLocalMap(const EstimateType& T) { _robot_in_local_map = T; }
  Status status() const { return _status; }
  std::vector<int> globalIndices() const {  // :98-101
    int n = 0;
    check(srrg2_scene_global_indices(_clipped->handle(), nullptr, &n));
    std::vector<int> v((size_t) n);
    if (n) check(srrg2_scene_global_indices(_clipped->handle(), v.data(), &n));
    return v;
  }

protected:
  void ready(const char* who) const {
    if (!_full || !_clipped) throw std::runtime_error(std::string(who) + "::compute|scene not set");
  }
  SceneType* _full    = nullptr;
  SceneType* _clipped = nullptr;
  EstimateType _robot_in_local_map = EstimateType::Identity();
  Status _status = Error;
};

template <int DIM>
class SceneClipperBall : public SceneClipperBase_<DIM> {
public:
  using Status      = typename SceneClipperBase_<DIM>::Status;
  float param_range = 10.f;
  void compute() {
    this->ready("SceneClipperBall");
    int st = Status::Error;
    check(srrg2_scene_clip_ball(this->_full->handle(), this->_robot_in_local_map.data(), param_range, this->_clipped->handle(), &st));
    this->_status = static_cast<Status>(st);
  }
};

// the clippers with a sensor: `param` (the PARAMs, sensor_in_robot among them), last() -- the counts of the last compute() --
// and the frame of compute(): clip(who, call), where call(full, robot_in_local_map, clipped, &result) makes the C call
template <int DIM, typename Params>
class SceneViewClipperBase_ : public SceneClipperBase_<DIM> {
public:
  Params param;
  void setSensorInRobot(const Isometry<DIM>& T) { std::memcpy(param.sensor_in_robot, T.data(), sizeof(param.sensor_in_robot)); }  // :86-89
  const srrg2_clip_result& last() const { return _last; }

protected:
  template <typename Call>
  void clip(const char* who, Call call) {
    this->ready(who);
    this->_status = SceneClipperBase_<DIM>::Error;
    check(call(this->_full->handle(), this->_robot_in_local_map.data(), this->_clipped->handle(), &_last));
    this->_status = static_cast<typename SceneClipperBase_<DIM>::Status>(_last.status);
  }
  srrg2_clip_result _last{};
};

// the points of a 3-D scene that a pinhole camera at sensor_in_robot sees (srrg2_scene_clip_projective): param.camera_matrix,
// image_rows / image_cols, depth range and occlusion_margin are the PARAMs
class SceneClipperProjective : public SceneViewClipperBase_<3, srrg2_projective_clip_params> {
public:
  SceneClipperProjective() { srrg2_clip_default_projective_params(&param); }
  void setCameraMatrix(const float* K_row_major) { std::memcpy(param.camera_matrix, K_row_major, sizeof(param.camera_matrix)); }
  void compute() {
    clip("SceneClipperProjective", [this](srrg2_scene_h full, const float* T, srrg2_scene_h clipped, srrg2_clip_result* out) {
      return srrg2_scene_clip_projective(full, T, &param, clipped, out);
    });
  }
};

// the points of a 2-D scene that a planar laser scanner at sensor_in_robot sees (srrg2_scene_clip_scan): param.angle_min,
// angle_increment, num_beams, range interval and occlusion_margin are the PARAMs
class SceneClipperScan : public SceneViewClipperBase_<2, srrg2_scan_clip_params> {
public:
  SceneClipperScan() { srrg2_clip_default_scan_params(&param); }
  void compute() {
    clip("SceneClipperScan", [this](srrg2_scene_h full, const float* T, srrg2_scene_h clipped, srrg2_clip_result* out) {
      return srrg2_scene_clip_scan(full, T, &param, clipped, out);
    });
  }
};

// the points of a 3-D scene that a spinning lidar at sensor_in_robot sees (srrg2_scene_clip_spherical): param.model (e.g. from
// srrg2_spherical_model_full_turn) and occlusion_margin are the PARAMs
class SceneClipperSpherical : public SceneViewClipperBase_<3, srrg2_spherical_clip_params> {
public:
  SceneClipperSpherical() { srrg2_clip_default_spherical_params(&param); }
  void setModel(const srrg2_spherical_model& m) { param.model = m; }
  // one elevation (radians) per row of param.model, strictly ascending or descending, for sensors whose rings are not uniformly
  // spaced (srrg2_scene_clip_spherical_rings; the model's elevation_min / elevation_increment are then ignored); a copy is kept.
  // nullptr or rows == 0: back to the model's uniform rows
  void setRingElevations(const double* elevations, int rows) {
    _rings.assign(elevations, elevations + (elevations && rows > 0 ? rows : 0));
  }
  const std::vector<double>& ringElevations() const { return _rings; }
  void compute() {
    ready("SceneClipperSpherical");
    if (!_rings.empty() && (int) _rings.size() != param.model.rows)
      throw std::runtime_error("SceneClipperSpherical::compute|one ring elevation per row of the model expected");
    clip("SceneClipperSpherical", [this](srrg2_scene_h full, const float* T, srrg2_scene_h clipped, srrg2_clip_result* out) {
      return srrg2_scene_clip_spherical_rings(full, T, &param, _rings.empty() ? nullptr : _rings.data(), clipped, out);
    });
  }

private:
  std::vector<double> _rings;
};

template <int DIM>
class MergerCorrespondenceHomo {
public:
  enum Status { Error = 0, Initializing = 1, Success = 2 };  // merger.h:19-23
  using EstimateType = Isometry<DIM>;
  using SceneType    = Scene<DIM>;
  // PARAMs: merger_correspondence_homo.h:22-31, merger.h:126-131
  float param_maximum_response                  = 50.f;
  float param_maximum_distance_geometry_squared = 0.25f;
  unsigned param_target_number_of_merges        = 200;
  void setScene(SceneType* s) { _scene = s; }
  void setMeasurement(const SceneType* m) { _meas = m; }
  void setMeasurementInScene(const EstimateType& T) { _T = T; }
  void setCorrespondences(const CorrespondenceVector* c) { _corr = c; }  // nullptr: none set (impl.cpp:30)
  void compute() {
    ready();
    srrg2_merger_params p = params();
    check(srrg2_scene_merge(_scene->handle(), _meas->handle(), _T.data(), _corr ? _corr->data() : nullptr,
                            _corr ? (int) _corr->size() : -1, &p, &_last));
    _status = static_cast<Status>(_last.status);
  }
  // correspondences taken on the device from the aligner run that matched `clipped` (moving) against the measurement
  // (fixed): TrackerSliceProcessor_::merge(), tracker_slice_processor_impl.cpp:160-186
  template <typename AlignerType>
  void computeFromAligner(AlignerType& aligner, int slice, const SceneType& clipped) {
    ready();
    srrg2_merger_params p = params();
    check(srrg2_scene_merge_from_aligner(_scene->handle(), _meas->handle(), _T.data(), aligner.handle(), slice,
                                         clipped.handle(), &p, &_last));
    _status = static_cast<Status>(_last.status);
  }
  Status status() const { return _status; }
  const srrg2_merge_result& last() const { return _last; }

private:
  void ready() const {
    if (!_scene || !_meas) throw std::runtime_error("MergerCorrespondenceHomo::compute|scene or measurement not set");
  }
  srrg2_merger_params params() const {
    return srrg2_merger_params{param_maximum_response, param_maximum_distance_geometry_squared,
                               (int32_t) param_target_number_of_merges};
  }
  SceneType* _scene       = nullptr;
  const SceneType* _meas  = nullptr;
  const CorrespondenceVector* _corr = nullptr;
  EstimateType _T = EstimateType::Identity();
  srrg2_merge_result _last{};
  Status _status = Error;
};

// the per-frame data association of a visual tracker (srrg2_scene_track_features): which keypoint of the measurement (fixed) is
// which landmark of the clipped local map (moving), by projective window and Hamming distance -- a concrete
// CorrespondenceFinder_ (S/registration/correspondence_finder.h:56-114: setFixed / setMoving / setLocalMapInSensor / compute).
// param: camera matrix, image size, depth range, search_radius, max_distance, min_margin, cross_check.  correspondences() is
// what MultiAligner_::setCorrespondences takes; toMerger() flips and globalises it for MergerCorrespondenceHomo.
class FeatureTracker {
public:
  srrg2_track_params param;
  FeatureTracker() { srrg2_track_default_params(&param); }
  void setCameraMatrix(const float* K_row_major) { std::memcpy(param.camera_matrix, K_row_major, sizeof(param.camera_matrix)); }
  void setFixed(const Scene<3>* measurement) { _fixed = measurement; }
  void setMoving(Scene<3>* clipped_map) { _moving = clipped_map; }
  void setMovingInSensor(const Isometry3f& T) { _T = T; }
  void compute() {
    if (!_fixed || !_moving) throw std::runtime_error("FeatureTracker::compute|fixed or moving not set");
    _corr.assign((size_t) _moving->size(), Correspondence{});  // (at most one pair per landmark)
    _result = srrg2_track_result{};
    check(srrg2_scene_track_features(_moving->handle(), _fixed->handle(), _T.data(), &param, _corr.data(), (int) _corr.size(),
                                     &_result));
    _corr.resize((size_t) _result.num_correspondences);
  }
  const CorrespondenceVector& correspondences() const { return _corr; }
  const srrg2_track_result& result() const { return _result; }
  // {fixed_idx = map point, moving_idx = measurement point}: the pairs as the merger reads them
  // (TrackerSliceProcessor_::merge(), tracker_slice_processor_impl.cpp:160-186); moving_global_indices = the clipped map's
  static CorrespondenceVector toMerger(const CorrespondenceVector& corr, const std::vector<int>& moving_global_indices) {
    CorrespondenceVector out(corr.size());
    for (size_t k = 0; k < corr.size(); ++k)
      out[k] = Correspondence{moving_global_indices.at((size_t) corr[k].moving_idx), corr[k].fixed_idx, corr[k].response};
    return out;
  }

private:
  const Scene<3>* _fixed = nullptr;
  Scene<3>* _moving      = nullptr;
  Isometry3f _T          = Isometry3f::Identity();
  CorrespondenceVector _corr;
  srrg2_track_result _result{};
};

// ---- measurement adaptors: RawDataPreprocessor_ (S/raw_data_preprocessors/raw_data_preprocessor.h:13-88) -------------
//   DepthImageAdaptor   depth image (+ intensity image) -> Scene<3>, organised or compact, with normals
//   LaserScanAdaptor    ranges -> Scene<2> with normals
//   LidarSweepAdaptor   3-D lidar sweep (point list, + intensity) -> Scene<3>, organised or compact, with normals
//   ImageFeatureAdaptor 8-bit intensity image (+ depth image) -> Scene<3> of keypoints with descriptors and intensity
//   PyramidFeatureAdaptor the same on every level of a scale pyramid of the image -> ONE Scene<3>, level-major
//   StereoFeatureAdaptor rectified pair of 8-bit images -> Scene<3> of matched, triangulated keypoints with descriptors
// setRawData / setMeas / compute / status / reset; status() is Error after setRawData until compute() (:67-72).  The raw
// data is borrowed until compute() has run.  compute(false) asks for no counts: an organised adapt then only queues its work.
class AdaptorBase_ {
public:
  enum Status { Ready = 0, Initializing = 1, Error = 2 };  // raw_data_preprocessor.h:22
  Status status() const { return _status; }
  const srrg2_adapt_result& last() const { return _last; }

protected:
  void finish(int rc, bool want_result) {
    _status = Error;
    check(rc);
    _status = want_result ? static_cast<Status>(_last.status) : Ready;
  }
  srrg2_adapt_result _last{};
  Status _status = Initializing;
};

class DepthImageAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_depth_adaptor_params param;
  DepthImageAdaptor() { srrg2_adapt_default_depth_params(&param); }
  // images with a row stride in bytes; intensity may be nullptr with SRRG2_IMAGE_NONE; param.rows / cols say the size
  void setRawData(const void* depth, int depth_type, int depth_row_stride_bytes, const void* intensity = nullptr,
                  int intensity_type = SRRG2_IMAGE_NONE, int intensity_row_stride_bytes = 0, int mem = SRRG2_MEM_HOST) {
    _depth = depth, _depth_type = depth_type, _depth_stride = depth_row_stride_bytes;
    _inten = intensity, _inten_type = intensity_type, _inten_stride = intensity_row_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
  }
  void compute(bool want_result = true) {
    if (!_meas || !_has_raw) throw std::runtime_error("DepthImageAdaptor::compute|raw data or measurement not set");
    finish(srrg2_adapt_depth_image(_meas->handle(), _depth, _depth_type, _depth_stride, _inten, _inten_type, _inten_stride, _mem,
                                   &param, want_result ? &_last : nullptr),
           want_result);
  }

private:
  MeasurementType* _meas = nullptr;
  const void* _depth = nullptr;
  const void* _inten = nullptr;
  int _depth_type = SRRG2_IMAGE_NONE, _depth_stride = 0, _inten_type = SRRG2_IMAGE_NONE, _inten_stride = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
};

class LaserScanAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<2>;
  srrg2_scan_adaptor_params param;
  LaserScanAdaptor() { srrg2_adapt_default_scan_params(&param); }
  void setRawData(const float* ranges, int num_beams, int mem = SRRG2_MEM_HOST) {
    _ranges = ranges, _num_beams = num_beams, _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
  }
  void compute(bool want_result = true) {
    if (!_meas || !_has_raw) throw std::runtime_error("LaserScanAdaptor::compute|raw data or measurement not set");
    finish(srrg2_adapt_laser_scan(_meas->handle(), _ranges, _num_beams, _mem, &param, want_result ? &_last : nullptr), want_result);
  }

private:
  MeasurementType* _meas = nullptr;
  const float* _ranges   = nullptr;
  int _num_beams = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
};

class LidarSweepAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_lidar_adaptor_params param;
  LidarSweepAdaptor() {
    srrg2_adapt_default_lidar_params(&param);
    srrg2_adapt_default_lidar_sweep_extras(&_extras);
  }
  // a full-turn sensor: srrg2_spherical_model_full_turn into param.model
  void setFullTurnModel(int rows, int cols, double elevation_first, double elevation_last) {
    check(srrg2_spherical_model_full_turn(&param.model, rows, cols, elevation_first, elevation_last));
  }
  // n records of x, y, z (sensor frame) with a stride in bytes; intensity may be nullptr (points + 3 with stride 16 reads XYZI)
  void setRawData(const float* points, int point_stride_bytes, int n, const float* intensity = nullptr,
                  int intensity_stride_bytes = 0, int mem = SRRG2_MEM_HOST) {
    _points = points, _point_stride = point_stride_bytes, _n = n;
    _inten = intensity, _inten_stride = intensity_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  // srrg2_lidar_sweep_extras (srrg2_adapt_lidar_sweep_ex); with none of the three set, compute() is srrg2_adapt_lidar_sweep.
  // one elevation (radians) per row of param.model, strictly monotonic; a copy is kept.  nullptr or rows == 0: uniform rows
  void setRingElevations(const double* elevations, int rows) {
    _rings.assign(elevations, elevations + (elevations && rows > 0 ? rows : 0));
  }
  // one float per point, in the memory of the points, borrowed like them; time_begin / time_end: the times that mean the sweep's
  // start and end.  nullptr: with a motion set, the time comes from the raw azimuth
  void setTimes(const float* times, int stride_bytes, double time_begin, double time_end) {
    _extras.times = times, _extras.time_stride_bytes = stride_bytes;
    _extras.time_begin = time_begin, _extras.time_end = time_end;
  }
  // de-skew: the sensor at the sweep's end in its frame at the sweep's start (prev^-1 * curr of a constant-velocity model);
  // reference: the normalised time of the frame the scene is expressed in (1 = the end).  An identity motion gives the plain
  // adapt's values
  void setMotion(const Isometry<3>& motion, double reference = 1.0) {
    std::memcpy(_extras.motion, motion.data(), sizeof(_extras.motion));
    _extras.reference = reference;
    _extras.deskew    = 1;
  }
  const srrg2_lidar_sweep_extras& extras() const { return _extras; }
  const std::vector<double>& ringElevations() const { return _rings; }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
  }
  void compute(bool want_result = true) {
    if (!_meas || !_has_raw) throw std::runtime_error("LidarSweepAdaptor::compute|raw data or measurement not set");
    if (!_rings.empty() && (int) _rings.size() != param.model.rows)
      throw std::runtime_error("LidarSweepAdaptor::compute|one ring elevation per row of the model expected");
    srrg2_lidar_sweep_extras x = _extras;
    x.ring_elevations          = _rings.empty() ? nullptr : _rings.data();
    finish(srrg2_adapt_lidar_sweep_ex(_meas->handle(), _points, _point_stride, _inten, _inten_stride, _n, _mem, &param, &x,
                                      want_result ? &_last : nullptr),
           want_result);
  }

private:
  MeasurementType* _meas = nullptr;
  const float* _points   = nullptr;
  const float* _inten    = nullptr;
  int _point_stride = 0, _inten_stride = 0, _n = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
  srrg2_lidar_sweep_extras _extras;
  std::vector<double> _rings;
};

// 8-bit intensity image (+ optional depth image) -> Scene<3> of keypoints: point, 256-bit descriptor, intensity, no normals;
// globalIndices() = pixel indices (srrg2_adapt_image_features).  camera: camera_matrix, rows, cols and the depth scale / gates
// are read.  last() keeps status and scene_size; features() has every counter, keypoints() the records in the scene's order.
class ImageFeatureAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_feature_params param;
  srrg2_depth_adaptor_params camera;
  ImageFeatureAdaptor() {
    srrg2_adapt_default_feature_params(&param);
    srrg2_adapt_default_depth_params(&camera);
  }
  // images with a row stride in bytes; depth may be nullptr with SRRG2_IMAGE_NONE; camera.rows / cols say the size
  void setRawData(const uint8_t* intensity, int intensity_row_stride_bytes, const void* depth = nullptr,
                  int depth_type = SRRG2_IMAGE_NONE, int depth_row_stride_bytes = 0, int mem = SRRG2_MEM_HOST) {
    _inten = intensity, _inten_stride = intensity_row_stride_bytes;
    _depth = depth, _depth_type = depth_type, _depth_stride = depth_row_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
    _keypoints.clear();
  }
  void compute() {
    if (!_meas || !_has_raw) throw std::runtime_error("ImageFeatureAdaptor::compute|raw data or measurement not set");
    // every selected keypoint fits: the cap, or every admissible pixel
    const long long inner = (long long) (camera.rows > 32 ? camera.rows - 32 : 0) * (long long) (camera.cols > 32 ? camera.cols - 32 : 0);
    const long long want  = param.max_features > 0 && param.max_features < inner ? param.max_features : inner;
    _keypoints.assign((size_t) (want > 0 ? want : 0), srrg2_keypoint{});
    _features = srrg2_feature_result{};
    const int rc = srrg2_adapt_image_features(_meas->handle(), _inten, SRRG2_IMAGE_U8, _inten_stride, _depth, _depth_type,
                                              _depth_stride, _mem, &camera, &param, _keypoints.empty() ? nullptr : _keypoints.data(),
                                              (int) _keypoints.size(), &_features);
    if (rc != 0) _keypoints.clear();
    _last            = srrg2_adapt_result{};
    _last.status     = _features.status;
    _last.num_raw    = _features.num_pixels;
    _last.num_valid  = _features.scene_size;
    _last.scene_size = _features.scene_size;
    finish(rc, true);
    _keypoints.resize((size_t) _features.scene_size < _keypoints.size() ? (size_t) _features.scene_size : _keypoints.size());
  }
  const srrg2_feature_result& features() const { return _features; }
  const std::vector<srrg2_keypoint>& keypoints() const { return _keypoints; }

private:
  MeasurementType* _meas = nullptr;
  const uint8_t* _inten  = nullptr;
  const void* _depth     = nullptr;
  int _inten_stride = 0, _depth_type = SRRG2_IMAGE_NONE, _depth_stride = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
  srrg2_feature_result _features{};
  std::vector<srrg2_keypoint> _keypoints;
};

// ImageFeatureAdaptor over a scale pyramid (srrg2_adapt_image_features_pyramid): ONE Scene<3> with the keypoints of every level,
// level-major, at their level-0 positions; globalIndices() = the nearest level-0 pixel (it may repeat across levels).  pyramid:
// num_levels and the ratio scale_num / scale_den.  last() keeps status and scene_size; result() has every per-level counter,
// keypoints() the records in the scene's order.
class PyramidFeatureAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_feature_params param;
  srrg2_pyramid_params pyramid;
  srrg2_depth_adaptor_params camera;
  PyramidFeatureAdaptor() {
    srrg2_adapt_default_feature_params(&param);
    srrg2_adapt_default_pyramid_params(&pyramid);
    srrg2_adapt_default_depth_params(&camera);
  }
  // images with a row stride in bytes; depth may be nullptr with SRRG2_IMAGE_NONE; camera.rows / cols say the size
  void setRawData(const uint8_t* intensity, int intensity_row_stride_bytes, const void* depth = nullptr,
                  int depth_type = SRRG2_IMAGE_NONE, int depth_row_stride_bytes = 0, int mem = SRRG2_MEM_HOST) {
    _inten = intensity, _inten_stride = intensity_row_stride_bytes;
    _depth = depth, _depth_type = depth_type, _depth_stride = depth_row_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
    _keypoints.clear();
  }
  void compute() {
    if (!_meas || !_has_raw) throw std::runtime_error("PyramidFeatureAdaptor::compute|raw data or measurement not set");
    // every selected keypoint fits: the cap, or every admissible pixel of every level
    long long want = param.max_features > 0 ? param.max_features : 0;
    if (param.max_features <= 0 && pyramid.scale_num > 0)
      for (int l = 0, rows = camera.rows, cols = camera.cols; l < pyramid.num_levels && rows > 32 && cols > 32;
           ++l, rows = rows * pyramid.scale_den / pyramid.scale_num, cols = cols * pyramid.scale_den / pyramid.scale_num)
        want += (long long) (rows - 32) * (long long) (cols - 32);
    _keypoints.assign((size_t) want, srrg2_pyramid_keypoint{});
    _result = srrg2_pyramid_result{};
    const int rc = srrg2_adapt_image_features_pyramid(_meas->handle(), _inten, SRRG2_IMAGE_U8, _inten_stride, _depth, _depth_type,
                                                      _depth_stride, _mem, &camera, &param, &pyramid,
                                                      _keypoints.empty() ? nullptr : _keypoints.data(), (int) _keypoints.size(), &_result);
    if (rc != 0) _keypoints.clear();
    _last            = srrg2_adapt_result{};
    _last.status     = _result.status;
    _last.num_raw    = camera.rows * camera.cols;
    _last.num_valid  = _result.scene_size;
    _last.scene_size = _result.scene_size;
    finish(rc, true);
    _keypoints.resize((size_t) _result.scene_size < _keypoints.size() ? (size_t) _result.scene_size : _keypoints.size());
  }
  const srrg2_pyramid_result& result() const { return _result; }
  const std::vector<srrg2_pyramid_keypoint>& keypoints() const { return _keypoints; }

private:
  MeasurementType* _meas = nullptr;
  const uint8_t* _inten  = nullptr;
  const void* _depth     = nullptr;
  int _inten_stride = 0, _depth_type = SRRG2_IMAGE_NONE, _depth_stride = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
  srrg2_pyramid_result _result{};
  std::vector<srrg2_pyramid_keypoint> _keypoints;
};

// a rectified pair of 8-bit images -> Scene<3> of the left image's keypoints that found their partner in the right image:
// triangulated point, left descriptor, left intensity, no normals; globalIndices() = left pixel indices
// (srrg2_adapt_stereo_features).  param: the per-image extraction; stereo: baseline (set it: the default 0 is refused), disparity
// range, row tolerance, gates; camera: camera_matrix, rows, cols, depth_min, depth_max are read.  last() keeps status and
// scene_size; result() has every counter, keypoints() and matches() the records in the scene's order.
class StereoFeatureAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_feature_params param;
  srrg2_stereo_params stereo;
  srrg2_depth_adaptor_params camera;
  StereoFeatureAdaptor() {
    srrg2_adapt_default_feature_params(&param);
    srrg2_adapt_default_stereo_params(&stereo);
    srrg2_adapt_default_depth_params(&camera);
  }
  // images with a row stride in bytes, both of camera.rows x camera.cols and in the same memory
  void setRawData(const uint8_t* left, int left_row_stride_bytes, const uint8_t* right, int right_row_stride_bytes,
                  int mem = SRRG2_MEM_HOST) {
    _left = left, _left_stride = left_row_stride_bytes;
    _right = right, _right_stride = right_row_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
    _keypoints.clear();
    _matches.clear();
  }
  void compute() {
    if (!_meas || !_has_raw) throw std::runtime_error("StereoFeatureAdaptor::compute|raw data or measurement not set");
    // every left keypoint fits: the cap, or every admissible pixel
    const long long inner = (long long) (camera.rows > 32 ? camera.rows - 32 : 0) * (long long) (camera.cols > 32 ? camera.cols - 32 : 0);
    const long long want  = param.max_features > 0 && param.max_features < inner ? param.max_features : inner;
    _keypoints.assign((size_t) (want > 0 ? want : 0), srrg2_keypoint{});
    _matches.assign(_keypoints.size(), srrg2_stereo_match{});
    _result = srrg2_stereo_result{};
    const int rc = srrg2_adapt_stereo_features(_meas->handle(), _left, _left_stride, _right, _right_stride, _mem, &camera, &param,
                                               &stereo, _keypoints.empty() ? nullptr : _keypoints.data(), (int) _keypoints.size(),
                                               _matches.empty() ? nullptr : _matches.data(), (int) _matches.size(), &_result);
    if (rc != 0) _keypoints.clear(), _matches.clear();
    _last            = srrg2_adapt_result{};
    _last.status     = _result.status;
    _last.num_raw    = _result.num_pixels;
    _last.num_valid  = _result.scene_size;
    _last.scene_size = _result.scene_size;
    finish(rc, true);
    const size_t got = (size_t) _result.scene_size < _keypoints.size() ? (size_t) _result.scene_size : _keypoints.size();
    _keypoints.resize(got);
    _matches.resize(got);
  }
  const srrg2_stereo_result& result() const { return _result; }
  const std::vector<srrg2_keypoint>& keypoints() const { return _keypoints; }
  const std::vector<srrg2_stereo_match>& matches() const { return _matches; }

private:
  MeasurementType* _meas = nullptr;
  const uint8_t* _left   = nullptr;
  const uint8_t* _right  = nullptr;
  int _left_stride = 0, _right_stride = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw = false;
  srrg2_stereo_result _result{};
  std::vector<srrg2_keypoint> _keypoints;
  std::vector<srrg2_stereo_match> _matches;
};

// a rectified pair of 8-bit images -> a disparity per pixel -> depth -> the Scene<3> that DepthImageAdaptor leaves for that
// depth with the left image as its intensity (srrg2_adapt_stereo_dense).  stereo: baseline (set it: the default 0 is refused),
// disparity range, paths, penalties, uniqueness, left-right check, sub-pixel; camera: all of it, as for DepthImageAdaptor.
// setMeas(nullptr) (or never): only the disparity image is computed.  compute(want_result, want_disparity): without the result
// an organised adapt whose disparity stays on the device only queues its work; with host images want_disparity fills
// disparity() (rows x cols floats, 0 = none); device images take setDisparityOut(device pointer, stride) instead.
class StereoDenseAdaptor : public AdaptorBase_ {
public:
  using MeasurementType = Scene<3>;
  srrg2_dense_stereo_params stereo;
  srrg2_depth_adaptor_params camera;
  StereoDenseAdaptor() {
    srrg2_adapt_default_dense_stereo_params(&stereo);
    srrg2_adapt_default_depth_params(&camera);
  }
  // images with a row stride in bytes, both of camera.rows x camera.cols and in the same memory
  void setRawData(const uint8_t* left, int left_row_stride_bytes, const uint8_t* right, int right_row_stride_bytes,
                  int mem = SRRG2_MEM_HOST) {
    _left = left, _left_stride = left_row_stride_bytes;
    _right = right, _right_stride = right_row_stride_bytes;
    _mem = mem, _has_raw = true;
    _status = Error;
  }
  void setMeas(MeasurementType* meas) { _meas = meas; }
  // where compute() writes the disparity image when the images are in device memory (nullptr: nowhere)
  void setDisparityOut(float* device_pointer, int row_stride_bytes) { _dev_out = device_pointer, _dev_out_stride = row_stride_bytes; }
  void reset() {
    _has_raw = false;
    _status  = Initializing;
    _disparity.clear();
  }
  void compute(bool want_result = true, bool want_disparity = false) {
    if (!_has_raw) throw std::runtime_error("StereoDenseAdaptor::compute|raw data not set");
    float* out_ptr = nullptr;
    int out_stride = 0;
    _disparity.clear();
    if (_mem == SRRG2_MEM_DEVICE) {
      out_ptr = _dev_out, out_stride = _dev_out_stride;
    } else if (want_disparity) {
      _disparity.assign((size_t) (camera.rows > 0 ? camera.rows : 0) * (size_t) (camera.cols > 0 ? camera.cols : 0), 0.f);
      out_ptr = _disparity.empty() ? nullptr : _disparity.data(), out_stride = 4 * camera.cols;
    }
    _result = srrg2_dense_stereo_result{};
    const int rc = srrg2_adapt_stereo_dense(_meas ? _meas->handle() : nullptr, _left, _left_stride, _right, _right_stride, _mem, &camera,
                                            &stereo, out_ptr, out_stride, want_result ? &_result : nullptr);
    if (rc != 0) _disparity.clear();
    _last              = srrg2_adapt_result{};
    _last.status       = _result.status;
    _last.num_raw      = _result.num_pixels;
    _last.num_in_range = _result.num_in_range;
    _last.num_valid    = _result.num_valid;
    _last.scene_size   = _result.scene_size;
    finish(rc, want_result);
  }
  const srrg2_dense_stereo_result& result() const { return _result; }
  const std::vector<float>& disparity() const { return _disparity; }

private:
  MeasurementType* _meas = nullptr;
  const uint8_t* _left   = nullptr;
  const uint8_t* _right  = nullptr;
  int _left_stride = 0, _right_stride = 0, _mem = SRRG2_MEM_HOST;
  bool _has_raw    = false;
  float* _dev_out  = nullptr;
  int _dev_out_stride = 0;
  srrg2_dense_stereo_result _result{};
  std::vector<float> _disparity;
};

// ---- rectification: lens undistortion and stereo rectification in front of the image adaptors ----------------------------
// (srrg2_rectifier_*, srrg2_rectify_image / _pair, srrg2_stereo_rectify; no reference counterpart, semantics: srrg2_slam_amd.h)
//   ImageRectifier   one camera and one target: params (camera_matrix, distortion, rotation, new_camera_matrix, shapes) -> set()
//                    builds the map on the device; rectify() remaps an image through it.  With order_on = scene.handle() and a
//                    device destination the call only queues on that scene's stream: the adaptor that then fills the scene from
//                    the rectified device image runs behind it without a host wait.
//   StereoRectifier  two of them set from a calibration (KL, KR, R, t with X_right = R X_left + t); rectify() remaps both images
//                    in one launch.  baseline goes into srrg2_dense_stereo_params, camera() into the adaptor's camera.
class ImageRectifier {
public:
  srrg2_rectifier_params params;
  explicit ImageRectifier(int device = 0) {
    srrg2_rectifier_default_params(&params);
    check(srrg2_rectifier_create(device, &_h));
  }
  ~ImageRectifier() { srrg2_rectifier_destroy(_h); }  // (waits for work queued with this map)
  ImageRectifier(const ImageRectifier&)            = delete;
  ImageRectifier& operator=(const ImageRectifier&) = delete;
  // builds the map from `params`; the counts of the map
  const srrg2_rectifier_info& set() {
    check(srrg2_rectifier_set(_h, &params, &_info));
    return _info;
  }
  const srrg2_rectifier_info& info() const { return _info; }
  // dst_rows x dst_cols entries (U, V) in 1/256 source pixel, INT32_MIN twice = invalid
  std::vector<int32_t> map() const {
    std::vector<int32_t> uv((size_t) 2 * (size_t) params.dst_rows * (size_t) params.dst_cols);
    check(srrg2_rectifier_get_map(_h, uv.empty() ? nullptr : uv.data(), (int64_t) uv.size()));
    return uv;
  }
  // the target's camera matrix, rows and cols into an adaptor's camera params
  void camera(srrg2_depth_adaptor_params& cam) const { check(srrg2_rectifier_camera(_h, &cam)); }
  // src: src_rows x src_cols of `type` (SRRG2_IMAGE_U8 / U16 / F32); dst: dst_rows x dst_cols of the same type; strides in bytes
  void rectify(const void* src, int type, int src_row_stride_bytes, void* dst, int dst_row_stride_bytes, int src_mem = SRRG2_MEM_HOST,
               int dst_mem = SRRG2_MEM_HOST, srrg2_scene_h order_on = nullptr, int border = 0) {
    check(srrg2_rectify_image(_h, order_on, src, type, src_row_stride_bytes, src_mem, dst, dst_row_stride_bytes, dst_mem, border));
  }
  srrg2_rectifier_h handle() const { return _h; }

private:
  srrg2_rectifier_h _h = nullptr;
  srrg2_rectifier_info _info{};
};

class StereoRectifier {
public:
  ImageRectifier left, right;
  double R1[9] = {0}, R2[9] = {0}, new_camera_matrix[9] = {0}, baseline = 0.0;
  explicit StereoRectifier(int device = 0) : left(device), right(device) {}
  // the rotations and the shared target camera of a calibration alone (host only)
  static void rotations(const double* KL, const double* KR, const double* R, const double* t, double* R1_out, double* R2_out,
                        double* Knew_out, double* baseline_out) {
    check(srrg2_stereo_rectify(KL, KR, R, t, R1_out, R2_out, Knew_out, baseline_out));
  }
  // distortion: 8 coefficients per camera; both sources of one shape, both targets dst_rows x dst_cols under the shared camera
  void setCalibration(const double* KL, const double* dist_left, const double* KR, const double* dist_right, const double* R,
                      const double* t, int src_rows, int src_cols, int dst_rows, int dst_cols) {
    rotations(KL, KR, R, t, R1, R2, new_camera_matrix, &baseline);
    fill(left.params, KL, dist_left, R1, src_rows, src_cols, dst_rows, dst_cols);
    fill(right.params, KR, dist_right, R2, src_rows, src_cols, dst_rows, dst_cols);
    left.set();
    right.set();
  }
  void camera(srrg2_depth_adaptor_params& cam) const { left.camera(cam); }
  // both U8 images in one launch; sources in `mem`, destinations in `dst_mem`
  void rectify(const uint8_t* left_src, int left_row_stride_bytes, const uint8_t* right_src, int right_row_stride_bytes, uint8_t* left_dst,
               int left_dst_row_stride_bytes, uint8_t* right_dst, int right_dst_row_stride_bytes, int mem = SRRG2_MEM_HOST,
               int dst_mem = SRRG2_MEM_HOST, srrg2_scene_h order_on = nullptr, int border = 0) {
    check(srrg2_rectify_pair(left.handle(), right.handle(), order_on, left_src, left_row_stride_bytes, right_src, right_row_stride_bytes,
                             mem, left_dst, left_dst_row_stride_bytes, right_dst, right_dst_row_stride_bytes, dst_mem, border));
  }

private:
  void fill(srrg2_rectifier_params& p, const double* K, const double* dist, const double* R, int src_rows, int src_cols, int dst_rows,
            int dst_cols) const {
    for (int i = 0; i < 9; ++i) p.camera_matrix[i] = K[i], p.rotation[i] = R[i], p.new_camera_matrix[i] = new_camera_matrix[i];
    for (int i = 0; i < 8; ++i) p.distortion[i] = dist ? dist[i] : 0.0;
    p.src_rows = src_rows, p.src_cols = src_cols, p.dst_rows = dst_rows, p.dst_cols = dst_cols;
  }
};

// ---- occupancy grid: laser scans and their poses -> free / occupied / unknown cells ---------------------------------------
// (srrg2_gridmap_*; no reference counterpart, semantics: srrg2_slam_amd.h)
//   GridMap   reset() allocates the two count planes from `params`; integrate() traces a batch of scans taken with the scanner of
//             `scan` from the given poses (one scan = the per-frame update), remove() takes the same scans out again bit for bit
//             -- after a pose-graph optimisation only the scans whose pose moved are re-drawn; counts() / render() read the map;
//             toScene() exports the occupied cells as a 2-D scene an aligner takes as it is.  buildLikelihood() / matchScans():
//             correlative scan matching against the map, a pose for a scan whose guess is too far off for ICP.  buildBounds() /
//             matchScansPruned() / localize(): the same search through a pyramid of upper bounds, cheap enough for the whole map
//             -- a pose for a scan that has no guess at all.
class GridMap {
public:
  srrg2_gridmap_params params;
  srrg2_gridmap_scan_params scan;
  explicit GridMap(int device = 0) {
    srrg2_gridmap_default_params(&params);
    srrg2_gridmap_default_scan_params(&scan);
    check(srrg2_gridmap_create(device, &_h));
  }
  ~GridMap() { srrg2_gridmap_destroy(_h); }  // (waits for queued work)
  GridMap(const GridMap&)            = delete;
  GridMap& operator=(const GridMap&) = delete;
  // a new, empty map from `params`
  void reset() {
    check(srrg2_gridmap_reset(_h, &params));
    _bounds_levels = 0;
  }
  // ranges: num_scans x scan.num_beams, robot_in_world: num_scans x 9 (row-major SE(2)), both in `mem`
  const srrg2_gridmap_result& integrate(const float* ranges, int num_scans, const float* robot_in_world, int mem = SRRG2_MEM_HOST,
                                        int weight = 1) {
    check(srrg2_gridmap_integrate_scans(_h, ranges, num_scans, robot_in_world, mem, &scan, weight, &_result));
    _bounds_levels = 0;
    return _result;
  }
  const srrg2_gridmap_result& remove(const float* ranges, int num_scans, const float* robot_in_world, int mem = SRRG2_MEM_HOST) {
    return integrate(ranges, num_scans, robot_in_world, mem, -1);
  }
  // queues the work on the grid's stream and returns without waiting; no counters
  void integrateQueued(const float* ranges, int num_scans, const float* robot_in_world, int mem = SRRG2_MEM_HOST, int weight = 1) {
    check(srrg2_gridmap_integrate_scans(_h, ranges, num_scans, robot_in_world, mem, &scan, weight, nullptr));
    _bounds_levels = 0;
  }
  const srrg2_gridmap_result& result() const { return _result; }
  size_t cells() const { return (size_t) params.rows * (size_t) params.cols; }
  // rows*cols words each, plane index iy*cols + ix
  void counts(std::vector<int32_t>& hits, std::vector<int32_t>& misses) const {
    hits.assign(cells(), 0);
    misses.assign(cells(), 0);
    check(srrg2_gridmap_get_counts(_h, hits.data(), misses.data(), SRRG2_MEM_HOST));
  }
  // rows x cols bytes: 0 .. 100, 255 = unknown
  std::vector<uint8_t> render(int min_observations = 1) const {
    std::vector<uint8_t> img(cells());
    check(srrg2_gridmap_render(_h, min_observations, img.data(), params.cols, SRRG2_MEM_HOST));
    return img;
  }
  // the cells that render into [occupied_percent, 100] as points at their centres; dst.globalIndices() are the plane indices
  void toScene(Scene<2>& dst, int min_observations = 1, int occupied_percent = 50) const {
    check(srrg2_gridmap_to_scene(_h, min_observations, occupied_percent, dst.handle()));
  }
  // correlative scan matching (srrg2_slam_amd.h "Correlative scan matching"): the likelihood field of the map as it is now, from
  // the default table of `radius_cells` or from the caller's radius_cells^2 + 1 bytes; every integrate / remove / reset makes it
  // stale and a match against a stale field throws
  static std::vector<uint8_t> defaultLikelihoodLut(int radius_cells) {
    std::vector<uint8_t> lut((size_t) (radius_cells > 0 ? radius_cells * radius_cells : 0) + 1);
    check(srrg2_gridmap_default_likelihood_lut(radius_cells, lut.data()));
    return lut;
  }
  void buildLikelihood(int min_observations = 1, int occupied_percent = 50, int radius_cells = 4) {
    buildLikelihood(min_observations, occupied_percent, radius_cells, defaultLikelihoodLut(radius_cells));
  }
  void buildLikelihood(int min_observations, int occupied_percent, int radius_cells, const std::vector<uint8_t>& lut) {
    if (radius_cells >= 0 && radius_cells <= 16 && lut.size() != (size_t) radius_cells * radius_cells + 1)
      throw std::runtime_error("GridMap::buildLikelihood: radius_cells^2 + 1 bytes of lut expected");
    _bounds_levels = 0;
    check(srrg2_gridmap_build_likelihood(_h, min_observations, occupied_percent, radius_cells, lut.data()));
  }
  // rows x cols bytes
  std::vector<uint8_t> likelihood() const {
    std::vector<uint8_t> img(cells());
    check(srrg2_gridmap_get_likelihood(_h, img.data(), params.cols, SRRG2_MEM_HOST));
    return img;
  }
  // the best pose of the window around each scan's guess; ranges / guesses (num_scans x 9) in `mem`.  scores: if not null, the
  // whole volume num_scans x Ntheta x Ny x Nx in flat-index order (what a covariance or an ambiguity test is derived from)
  std::vector<srrg2_gridmap_match_result> matchScans(const float* ranges, int num_scans, const float* guess_robot_in_world,
                                                     const srrg2_gridmap_match_params& window, int mem = SRRG2_MEM_HOST,
                                                     std::vector<int32_t>* scores = nullptr) {
    std::vector<srrg2_gridmap_match_result> out((size_t) (num_scans > 0 ? num_scans : 0));
    if (scores) {
      const double n = (2.0 * window.half_window_x + 1) * (2.0 * window.half_window_y + 1) * (2.0 * window.half_steps_theta + 1) *
                       (double) out.size();
      scores->assign(n >= 0 && n <= 2147483647.0 ? (size_t) n : 0, 0);  // (beyond int32 the call refuses and writes nothing)
    }
    check(srrg2_gridmap_match_scans(_h, ranges, num_scans, guess_robot_in_world, mem, &scan, &window, out.data(),
                                    scores ? scores->data() : nullptr, SRRG2_MEM_HOST));
    return out;
  }
  // pruned scan matching (srrg2_slam_amd.h "Pruned scan matching"): the bound planes P_1 .. P_levels of the field as it is now;
  // whatever makes the field stale -- buildLikelihood too -- makes them stale
  void buildBounds(int levels = 4) {
    check(srrg2_gridmap_build_bounds(_h, levels));
    _bounds_levels = levels;
  }
  // (rows + s - 1) x (cols + s - 1) bytes, s = 2^level: row y + s - 1, column x + s - 1 hold the maximum of the field over the
  // cells [x, x + s) x [y, y + s) inside the grid
  std::vector<uint8_t> bounds(int level) const {
    const size_t s = (size_t) 1 << (level < 0 ? 0 : level > 6 ? 6 : level);
    std::vector<uint8_t> img(((size_t) params.rows + s - 1) * ((size_t) params.cols + s - 1));
    check(srrg2_gridmap_get_bounds(_h, level, img.data(), (int) ((size_t) params.cols + s - 1), SRRG2_MEM_HOST));
    return img;
  }
  // matchScans through the bound planes: the same window, bit for bit the same results, without scoring most of it.  levels = 0:
  // all that were built; max_list_entries = 0: 2^20 blocks per scan and level before a scan falls back to the exhaustive search.
  // stats: if not null, one srrg2_gridmap_prune_stats per scan
  std::vector<srrg2_gridmap_match_result> matchScansPruned(const float* ranges, int num_scans, const float* guess_robot_in_world,
                                                           const srrg2_gridmap_match_params& window, int levels = 0, int max_list_entries = 0,
                                                           int mem = SRRG2_MEM_HOST, std::vector<srrg2_gridmap_prune_stats>* stats = nullptr) {
    std::vector<srrg2_gridmap_match_result> out((size_t) (num_scans > 0 ? num_scans : 0));
    if (stats) stats->assign(out.size(), srrg2_gridmap_prune_stats{});
    srrg2_gridmap_prune_params prune;
    prune.num_levels = levels > 0 ? levels : _bounds_levels, prune.max_list_entries = max_list_entries;
    check(srrg2_gridmap_match_scans_pruned(_h, ranges, num_scans, guess_robot_in_world, mem, &scan, &window, &prune, out.data(),
                                           stats ? stats->data() : nullptr));
    return out;
  }
  // the guess of localize(): the centre of cell (cols / 2, rows / 2) at heading 0, row-major SE(2)
  void centrePose(float* robot_in_world) const {
    const float P[9] = {1.f, 0.f, (float) ((double) params.origin[0] + (params.cols / 2 + 0.5) * (double) params.resolution),
                        0.f, 1.f, (float) ((double) params.origin[1] + (params.rows / 2 + 0.5) * (double) params.resolution),
                        0.f, 0.f, 1.f};
    for (int i = 0; i < 9; ++i) robot_in_world[i] = P[i];
  }
  // scans without any guess against the whole map: the window is the grid around its centre cell and ceil(pi / theta_step) steps
  // either way.  Builds the bound planes if they are stale (levels, or 4); the field must be fresh.  ranges in host memory
  std::vector<srrg2_gridmap_match_result> localize(const float* ranges, int num_scans, double theta_step, int levels = 0,
                                                   std::vector<srrg2_gridmap_prune_stats>* stats = nullptr) {
    if (_bounds_levels < (levels > 0 ? levels : 1)) buildBounds(levels > 0 ? levels : 4);
    std::vector<float> guesses((size_t) (num_scans > 0 ? num_scans : 0) * 9);
    for (size_t k = 0; k * 9 < guesses.size(); ++k) centrePose(guesses.data() + 9 * k);
    srrg2_gridmap_match_params window;
    window.half_window_x = params.cols / 2, window.half_window_y = params.rows / 2;
    window.half_steps_theta = (int) std::ceil(3.14159265358979323846 / theta_step);
    window.reserved = 0, window.theta_step = theta_step;
    return matchScansPruned(ranges, num_scans, guesses.data(), window, levels, 0, SRRG2_MEM_HOST, stats);
  }
  srrg2_gridmap_h handle() const { return _h; }

private:
  srrg2_gridmap_h _h = nullptr;
  srrg2_gridmap_result _result{};
  int _bounds_levels = 0;  // the levels of bound planes built from the field as it is
};

// ---- TSDF volume: depth frames and their poses -> a truncated signed-distance volume -----------------------------------
// (srrg2_tsdf_*; no reference counterpart, semantics: srrg2_slam_amd.h)
//   TsdfVolume   reset() allocates the planes from `params`; integrate() fuses a batch of depth frames taken with `camera` from the
//                given poses (one frame = the per-frame update), remove() takes the same frames out again bit for bit -- after a
//                pose-graph optimisation only the frames whose pose moved are re-integrated; planes() reads the volume; raycast()
//                renders it from a pose and runs the depth adaptor on the image: the scene is set_fixed of the projective
//                point-to-plane slice (frame-to-model tracking); toScene() exports the surface as a cloud with normals.
class TsdfVolume {
public:
  srrg2_tsdf_params params;
  srrg2_tsdf_frame_params frame;
  srrg2_tsdf_raycast_params ray;
  srrg2_depth_adaptor_params camera;  // of the frames and of the raycast (which hands the adaptor's fields on)
  explicit TsdfVolume(int device = 0) {
    srrg2_tsdf_default_params(&params);
    srrg2_tsdf_default_frame_params(&frame);
    srrg2_tsdf_default_raycast_params(&ray);
    srrg2_adapt_default_depth_params(&camera);
    check(srrg2_tsdf_create(device, &_h));
  }
  ~TsdfVolume() { srrg2_tsdf_destroy(_h); }  // (waits for queued work)
  TsdfVolume(const TsdfVolume&)            = delete;
  TsdfVolume& operator=(const TsdfVolume&) = delete;
  // a new, empty volume from `params`
  void reset() { check(srrg2_tsdf_reset(_h, &params)); }
  // depth (intensity: null for a volume without the plane): num_frames images one behind the other in `mem`;
  // camera_in_world: num_frames x 12 on the host
  const srrg2_tsdf_result& integrate(const void* depth, int depth_type, int depth_stride, int num_frames, const float* camera_in_world,
                                     const void* intensity = nullptr, int intensity_type = SRRG2_IMAGE_NONE, int intensity_stride = 0,
                                     int mem = SRRG2_MEM_HOST, int weight = 1) {
    check(srrg2_tsdf_integrate_frames(_h, depth, depth_type, depth_stride, intensity, intensity_type, intensity_stride, num_frames,
                                      camera_in_world, mem, &camera, &frame, weight, &_result));
    return _result;
  }
  const srrg2_tsdf_result& remove(const void* depth, int depth_type, int depth_stride, int num_frames, const float* camera_in_world,
                                  const void* intensity = nullptr, int intensity_type = SRRG2_IMAGE_NONE, int intensity_stride = 0,
                                  int mem = SRRG2_MEM_HOST) {
    return integrate(depth, depth_type, depth_stride, num_frames, camera_in_world, intensity, intensity_type, intensity_stride, mem, -1);
  }
  // queues the work on the volume's stream and returns without waiting; no counters
  void integrateQueued(const void* depth, int depth_type, int depth_stride, int num_frames, const float* camera_in_world,
                       const void* intensity = nullptr, int intensity_type = SRRG2_IMAGE_NONE, int intensity_stride = 0,
                       int mem = SRRG2_MEM_HOST, int weight = 1) {
    check(srrg2_tsdf_integrate_frames(_h, depth, depth_type, depth_stride, intensity, intensity_type, intensity_stride, num_frames,
                                      camera_in_world, mem, &camera, &frame, weight, nullptr));
  }
  const srrg2_tsdf_result& result() const { return _result; }
  size_t voxels() const { return (size_t) params.nx * (size_t) params.ny * (size_t) params.nz; }
  // nx*ny*nz words each, plane index (z ny + y) nx + x; isum stays empty for a volume without the plane
  void planes(std::vector<int32_t>& sum, std::vector<int32_t>& weight, std::vector<int32_t>& isum) const {
    sum.assign(voxels(), 0);
    weight.assign(voxels(), 0);
    isum.assign(params.with_intensity ? voxels() : 0, 0);
    check(srrg2_tsdf_get_planes(_h, sum.data(), weight.data(), params.with_intensity ? isum.data() : nullptr, SRRG2_MEM_HOST));
  }
  // the depth image a camera at camera_in_world (12 floats) would measure; dst (may be null) receives the depth adaptor's scene
  std::vector<float> raycast(const float* camera_in_world, Scene<3>* dst = nullptr) {
    std::vector<float> depth((size_t) (camera.rows > 0 ? camera.rows : 0) * (size_t) (camera.cols > 0 ? camera.cols : 0));
    check(srrg2_tsdf_raycast(_h, camera_in_world, &camera, &ray, dst ? dst->handle() : nullptr, depth.empty() ? nullptr : depth.data(),
                             SRRG2_MEM_HOST, &_raycast));
    return depth;
  }
  const srrg2_tsdf_raycast_result& lastRaycast() const { return _raycast; }
  // the zero crossings between neighbouring voxels as points with normals; dst.globalIndices() are 3 * plane index + axis
  int toScene(Scene<3>& dst, int min_weight = 1) const {
    srrg2_tsdf_export_result out{};
    check(srrg2_tsdf_to_scene(_h, min_weight, dst.handle(), &out));
    return out.num_points;
  }
  srrg2_tsdf_h handle() const { return _h; }

private:
  srrg2_tsdf_h _h = nullptr;
  srrg2_tsdf_result _result{};
  srrg2_tsdf_raycast_result _raycast{};
};

// ---- binary descriptor database: the matching half of MultiLoopDetectorHBST_ --------------------------------------
// (S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:41-197; it stands where the reference keeps its
// srrg_hbst::BinaryTree256<uint64_t>).  Exact, exhaustive matching on the device; semantics: srrg2_slam_amd.h.
class DescriptorDatabase {
public:
  struct Candidate {
    int32_t index;        // database index of the reference local map
    int64_t num_matches;  // matching pairs before deduplication
    CorrespondenceVector correspondences;  // fixed_idx = query point, moving_idx = reference point, response = distance
  };
  explicit DescriptorDatabase(int device = 0) { check(srrg2_descriptor_db_create(device, &_h)); }
  ~DescriptorDatabase() { srrg2_descriptor_db_destroy(_h); }
  DescriptorDatabase(const DescriptorDatabase&)            = delete;
  DescriptorDatabase& operator=(const DescriptorDatabase&) = delete;
  // n rows of SRRG2_DESCRIPTOR_BYTES bytes; valid: n bytes or nullptr.  Returns the database index, -1 if not added.
  int add(const uint8_t* descriptors, const uint8_t* valid, int n) {
    int index = -1;
    check(srrg2_descriptor_db_add(_h, descriptors, valid, n, &index));
    return index;
  }
  int size() const {
    int maps = 0;
    check(srrg2_descriptor_db_size(_h, &maps, nullptr));
    return maps;
  }
  int64_t numDescriptors() const {
    int64_t n = 0;
    check(srrg2_descriptor_db_size(_h, nullptr, &n));
    return n;
  }
  // computeCorrespondences (:117-161): the candidates ascending in database index
  std::vector<Candidate> match(const uint8_t* descriptors, const uint8_t* valid, int n, int64_t query_index,
                               float maximum_descriptor_distance = 25.0f, uint32_t minimum_age_difference = 0,
                               int64_t min_matches = 0) {
    int K = 0;
    check(srrg2_descriptor_db_match(_h, descriptors, valid, n, query_index, maximum_descriptor_distance,
                                    minimum_age_difference, min_matches, &K));
    return candidates(K);
  }

private:
  std::vector<Candidate> candidates(int K) {
    std::vector<int32_t> index(K);
    std::vector<int64_t> count(K), offsets(K + 1);
    check(srrg2_descriptor_db_get_candidates(_h, index.data(), count.data(), offsets.data(), &K));
    int64_t total = offsets[K];
    CorrespondenceVector all(total);
    check(srrg2_descriptor_db_get_correspondences(_h, all.data(), &total));
    std::vector<Candidate> out(K);
    for (int k = 0; k < K; ++k) {
      out[k].index       = index[k];
      out[k].num_matches = count[k];
      out[k].correspondences.assign(all.begin() + offsets[k], all.begin() + offsets[k + 1]);
    }
    return out;
  }

public:
  // add / match with the descriptors of a scene that carries them, read on the device; valid = finite coordinates
  template <int DIM>
  int add(const Scene<DIM>& scene) {
    int index = -1;
    check(srrg2_descriptor_db_add_scene(_h, scene.handle(), &index));
    return index;
  }
  template <int DIM>
  std::vector<Candidate> match(const Scene<DIM>& scene, int64_t query_index, float maximum_descriptor_distance = 25.0f,
                               uint32_t minimum_age_difference = 0, int64_t min_matches = 0) {
    int K = 0;
    check(srrg2_descriptor_db_match_scene(_h, scene.handle(), query_index, maximum_descriptor_distance,
                                          minimum_age_difference, min_matches, &K));
    return candidates(K);
  }
  // the pair count of every map in the last match(), -1 for maps the age gate skipped
  std::vector<int64_t> mapCounts() const {
    int n = 0;
    check(srrg2_descriptor_db_get_map_counts(_h, nullptr, &n));
    std::vector<int64_t> c(n);
    check(srrg2_descriptor_db_get_map_counts(_h, c.data(), &n));
    return c;
  }
  double lastMatchMs() const {
    double ms = 0.0;
    check(srrg2_descriptor_db_last_match_ms(_h, &ms));
    return ms;
  }
  srrg2_descriptor_db_h handle() const { return _h; }

private:
  srrg2_descriptor_db_h _h = nullptr;
};

}  // namespace srrg2_slam_amd
