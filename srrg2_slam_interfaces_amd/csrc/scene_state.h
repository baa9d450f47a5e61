// scene_state.h -- what a scene handle holds (srrg2_scene_h), shared by the sources that write scenes: scene.hip (set, clip,
// merge) and adaptor.hip (measurement adaptors).  Internal to the library.
#pragma once
#include <functional>

#include "host_util.h"

struct srrg2_scene {
  int dim = 3, device = 0;
  hipStream_t stream = nullptr;
  srrg2amd::DevBuf<float4> pts, nrm;
  int n            = 0;
  bool has_normals = false;
  // per-point features (absent unless set_features / a merge or clip brought them): 2 uint4 per point, 1 float per point;
  // when present their capacity follows pts.cap
  srrg2amd::DevBuf<uint4> desc;
  srrg2amd::DevBuf<float> inten;
  bool has_desc = false, has_inten = false;
  srrg2amd::DevBuf<int> gidx;  // local -> global indices of the last clip into this scene
  int ng = 0;
  // an adaptor has queued work that writes this scene and returned without waiting (srrg2_adapt_*, organised mode without a
  // result): scene.hip's entry points wait for it before the host, or a stream other than `stream`, reads or rewrites it
  bool pending = false;
  // scratch
  srrg2amd::DevBuf<int> flags, scan_sums, counts, dup_list;
  srrg2amd::DevBuf<unsigned char> merged;
  srrg2amd::DevBuf<srrg2_correspondence> corr;
  srrg2amd::DevBuf<unsigned long long> dup_keys;  // (scene index << 32 | correspondence index) of the duplicates: unsorted, sorted
  srrg2amd::DevBuf<char> sort_tmp;
  srrg2amd::DevBuf<char> staging;
  srrg2amd::DevBuf<unsigned> zmin;  // clip_projective with occlusion: per pixel the bits of the smallest camera depth seen
  srrg2amd::DevBuf<unsigned> rmin;  // clip_scan / clip_spherical with occlusion: per beam / pixel the bits of the smallest range seen
  // adapt_lidar_sweep: per pixel of the range image (range bits << 32 | input index) of the nearest point, all ones = empty
  srrg2amd::DevBuf<unsigned long long> winner;
  // adapt_lidar_sweep_ex with de-skew: per input point its de-skewed coordinates (written for in-view points, read for winners)
  srrg2amd::DevBuf<float4> deskewed;
  srrg2amd::DevBuf<uint2> sph_stage;  // clip_spherical with occlusion: per point (pixel or -1, range bits) from the minimum pass
  // estimate_normals (normals.hip): the arrays the call writes in place of the scene's own -- swapped in once it has succeeded,
  // so a refused call leaves the scene as it was -- and its scratch: cell keys and point indices (unsorted, sorted), the points
  // in cell order, per-point normal and curvature, the bounding box / cell layout / counters block
  srrg2amd::DevBuf<float4> alt_pts, alt_nrm, nrm_sorted, nrm_tmp;
  srrg2amd::DevBuf<uint4> alt_desc;
  srrg2amd::DevBuf<float> alt_inten, nrm_curv;
  srrg2amd::DevBuf<int> alt_gidx, nrm_idx, nrm_ctr;
  srrg2amd::DevBuf<unsigned long long> nrm_keys;
  // voxelize (voxel.hip; it sorts through the normals' key / index / counters scratch above): per cell the fixed-point sums and
  // the two counts, the representative's scene index; per sorted entry the cell rank; per representative the emitted point,
  // normal and count; per emitted point the count
  srrg2amd::DevBuf<long long> vox_acc;
  srrg2amd::DevBuf<int> vox_rep, vox_rank, vox_cnt, vox_counts;
  srrg2amd::DevBuf<float4> vox_pts, vox_nrm;
  // adapt_image_features (features.hip): the U8 score and U16 box-sum images (padded to whole tiles), per pixel the maxima
  // flag and the rank among the keypoints of the cut score, the counters + score histogram block, the 32 rotated patterns
  // (uploaded once), per kept keypoint its record
  srrg2amd::DevBuf<unsigned char> feat_score, feat_max;
  srrg2amd::DevBuf<unsigned short> feat_box;
  srrg2amd::DevBuf<int> feat_tie, feat_ctr;
  srrg2amd::DevBuf<unsigned> feat_pattern;
  srrg2amd::DevBuf<srrg2_keypoint> feat_kp;
  bool feat_pattern_ready = false;
  // adapt_stereo_features (stereo.hip): the right image's copy of the pipeline scratch above (the left image uses feat_* with
  // flags / scan_sums); per image [left, right] and selected keypoint its pixel, descriptor and record, per image row + 1 the
  // first keypoint at or below it, per keypoint its best candidate (distance << 32 | candidate index, all ones = none); per left
  // keypoint its match record and depth; the counters; the compacted match records
  srrg2amd::DevBuf<unsigned char> st_score, st_max;
  srrg2amd::DevBuf<unsigned short> st_box;
  srrg2amd::DevBuf<int> st_tie, st_ctr, st_flags, st_sums;
  srrg2amd::DevBuf<int> st_pixel[2], st_rows[2], st_counts;
  srrg2amd::DevBuf<uint4> st_desc[2];
  srrg2amd::DevBuf<srrg2_keypoint> st_kp[2];
  srrg2amd::DevBuf<unsigned long long> st_best[2];
  srrg2amd::DevBuf<srrg2_stereo_match> st_match, st_match_out;
  srrg2amd::DevBuf<float> st_z;
  // adapt_stereo_dense (stereo_dense.hip): both images' census words [left, right][rows*cols]; the aggregated cost volume S,
  // [row][col][d] over the processed rectangle, 16 bits per element; per rectangle pixel its best-disparity record (index |
  // unique << 16) and its sub-pixel disparity; per row of the rectangle and right-image column the diagonal's best index; per
  // image pixel the depth Z the depth adaptor then reads, the flag byte the counters are summed from and (a host disparity_out
  // only) the disparity; the three counters
  srrg2amd::DevBuf<unsigned long long> sd_census;
  srrg2amd::DevBuf<unsigned short> sd_vol, sd_right;
  srrg2amd::DevBuf<int> sd_best, sd_counts;
  srrg2amd::DevBuf<float> sd_sub, sd_z, sd_disp;
  srrg2amd::DevBuf<unsigned char> sd_flags;
  // adapt_image_features_pyramid (pyramid.hip): levels 1 .. of the image at pitches that are multiples of 4; the pipeline scratch
  // of ALL levels, each array one block with a slice per level (score / box padded to whole tiles, maxima flags, tie ranks, keep
  // flags, scan sums, counters); per kept keypoint its level pixel and its record; the pinned mirror of the levels' counters
  srrg2amd::DevBuf<unsigned char> pyr_img, pyr_score, pyr_max;
  srrg2amd::DevBuf<unsigned short> pyr_box;
  srrg2amd::DevBuf<int> pyr_tie, pyr_flags, pyr_sums, pyr_ctr, pyr_lpix;
  srrg2amd::DevBuf<srrg2_pyramid_keypoint> pyr_kp;
  srrg2amd::PinnedBuf<int> pyr_host;
  // ... and, while the content is that call's: the number of built levels and where each level's keypoints begin (level l is
  // points pyr_offset[l] .. pyr_offset[l + 1]).  scene_make_room and every other rewrite of the content clear pyr_levels; the
  // tracker reads it to search a level-major `fixed` scene level by level
  int pyr_levels = 0;
  int pyr_offset[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // track_features (tracking.hip; on the MOVING scene, whose flags / scan_sums hold the keep flags and their scan): per landmark
  // its projected pixel (-1 = not in view), its best keypoint (distance << 32 | keypoint index, all ones = none), the smallest
  // distance among its other candidates and its record; per image row + 1 the first keypoint at or below it; per keypoint the
  // best landmark (distance << 32 | landmark index); the counters + error word with the capacity-bounded compacted records
  // behind them in ONE block, and that block's pinned host mirror
  srrg2amd::DevBuf<int> trk_pix, trk_rows;
  srrg2amd::DevBuf<unsigned> trk_second;
  srrg2amd::DevBuf<unsigned long long> trk_best, trk_best_fixed;
  // ... `fixed` a pyramid scene of several levels: per level and landmark the level's best keypoint and runner-up distance
  srrg2amd::DevBuf<unsigned long long> trk_best_level;
  srrg2amd::DevBuf<unsigned> trk_second_level;
  srrg2amd::DevBuf<srrg2_correspondence> trk_rec;
  srrg2amd::DevBuf<int> trk_out;
  srrg2amd::PinnedBuf<int> trk_host;  // words
  srrg2amd::PinnedBuf<int> scalars;   // pinned host mirror of dscalars
  // device: [1] num_merged, [2] error flag, [3] duplicates seen, [4] ncorr (merge); [0] Valid, [1] in view, [2] scan total (clip);
  // [8] in range, [9] Valid (adapt)
  // (host mirror only) [12] evaluated, [13] unique, [14] consistent (adapt_stereo_dense)
  srrg2amd::DevBuf<int> dscalars;
  // The ordering is what this destructor is for: the stream retires before any buffer above is freed (the members free
  // themselves after this body).  A new scratch buffer is one member line and nothing else.
  ~srrg2_scene() {
    (void) hipSetDevice(device);
    if (stream) (void) hipStreamSynchronize(stream);
    if (stream) (void) hipStreamDestroy(stream);
  }
};

namespace srrg2amd {

// grow the point arrays (and the feature arrays that are present) to hold n points, keeping the first `keep` (scene.hip)
int scene_make_room(srrg2_scene* s, int n, int keep);
// s->flags[0..n) -> exclusive scan in place; the total comes back on the host (one wait on the scene's stream)
int scene_scan_flags(srrg2_scene* s, int n, int* total);
// two distinct scenes of one dim on one device: what a clipper -- or the voxelizer -- reads and what it writes
bool scene_clip_pair(const srrg2_scene* full, const srrg2_scene* clipped);
// both scenes current and quiet; `clipped` takes the fields of `full` and is empty until the call has succeeded
int scene_clip_begin(srrg2_scene* full, srrg2_scene* clipped);
// The tail of every call that keeps some points of `full`, in scene order, in `clipped`: the n > 0 keep flags queued in
// full->flags (n + 1 words reserved) are scanned in place; scatter(cap) launches, on full->stream, the kernel that moves a kept
// point i to clipped's slot k = flags[i] when flags[i + 1] != k and k < cap; before_wait (may be empty) queues what else the one
// host wait shall carry.  clipped->n = ng = the total when it returns (details at compact_into, scene.hip).
int scene_compact_into(srrg2_scene* full, srrg2_scene* clipped, int n, const std::function<void(int cap)>& scatter,
                       const std::function<int()>& before_wait);

}  // namespace srrg2amd
