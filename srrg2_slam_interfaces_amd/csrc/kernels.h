// kernels.h -- launchers of the HIP kernels in kernels.hip (C++ linkage, internal to the library)
#pragma once
#include "device_types.h"

namespace srrg2amd {

void launch_ingest(const float* src, int stride_floats, int n, int dim, float4* dst, unsigned* maxabs_bits,
                   int finite_per_point, hipStream_t s);
void launch_ingest_batch(const float* src, int stride_floats, const ProblemDev* probs, int K, int max_nm, int dim,
                         float4* dst, unsigned* maxabs_bits, int finite_per_point, hipStream_t s);
void launch_bbox(const float4* pts, int n, unsigned* mn, unsigned* mx, int* nvalid, hipStream_t s);
void launch_ingest_bbox(const float* src, int stride_floats, int n, int dim, float4* dst, unsigned* maxabs_bits, unsigned* mn,
                        unsigned* mx, int* nvalid, hipStream_t s, unsigned* ticket, unsigned* host_out, unsigned seq,
                        unsigned* block_out /* [INGEST_BBOX_MAX_BLOCKS][8] */, unsigned* clear_after);
#define INGEST_BBOX_MAX_BLOCKS 512
void launch_grid_count(const GridDev& g, const float4* pts, int n, int* counts, hipStream_t s);
void launch_count_nonzero(const int* counts, int n, int* out, hipStream_t s);
int scan_num_blocks(int n);
void launch_exclusive_scan(int* data, int n, int* block_sums, int* grand_total, hipStream_t s, int* copy = nullptr);
// desc_band.hip: the best 256-bit descriptor inside a band of image rows (stereo.hip, tracking.hip).  A best word is
// (Hamming distance << 32 | index), NO_CANDIDATE when nothing was inside the gate; second: the smallest distance of any other
// candidate, NO_SECOND (= the distance field of NO_CANDIDATE) when there was none.
constexpr unsigned long long NO_CANDIDATE = ~0ull;
constexpr unsigned NO_SECOND              = 0xffffffffu;
// row_begin[rows + 1] from n ascending pixel indices.  error not null: raised on a pixel outside [0, rows * cols) or not above
// its predecessor; null: the caller vouches for the pixels.
void launch_band_rows(const int* pixel, int n, int rows, int cols, int* row_begin, int* error, hipStream_t s);
// best[q] over the candidates of rows r - radius .. r + radius with lo <= candidate column - query column <= hi; q_pixel[q] < 0
// skips the query, a set error word (may be null) all of them.  second (may be null): the runner-up's distance; reverse (may be
// null, needs second): per candidate the atomicMin of (distance << 32 | query index), set to NO_CANDIDATE by the caller.
void launch_band_search(int nq, const int* q_pixel, const uint4* q_desc, const int* c_pixel, const uint4* c_desc, const int* c_rows,
                        int rows, int cols, int radius, int lo, int hi, const int* error, unsigned long long* best, unsigned* second,
                        unsigned long long* reverse, hipStream_t s);
void launch_grid_scatter(const GridDev& g, const float4* pts, const float4* nrm, int n, int* cursor, float4* out_pts,
                         float4* out_nrm, int* pos_of, hipStream_t s);
// cell neighbour lists of the grid (GridDev::list_*): ent == null counts the entries per cell into list_start, else fills
// (box_at: [fixed points] scratch of the fill pass -- the tight box of every entry, by the position of its first point)
void launch_cnl_build(const GridDev& g, const GridLists& L, const int4* offs, int noffs, int* list_start, uint2* box_at,
                      uint4* ent, hipStream_t s);
// search pass over the cell neighbour lists (any number of alignments per launch; no deferred-search queue)
// (init_C / init_inl != null: the FIRST pass of a single alignment's compute() with the prologue inside -- no k_icp_init launch;
// K == 1, fused control steps, the slot sets left zeroed by the previous compute()'s final step: run_compute decides)
// (plan_lanes > 1, launches of up to four alignments: the tiles of a launch plan, search_plan.h, with at most that many lanes per
// point, laid out for plan_capacity workgroups resident together -- 0: what the device holds of the instantiation, asked once
// per handle and kept in `cap`; plan_whole: the automatic policy -- the most lanes every point can have in ONE round, and the
// uniform tiles of `team` when not even two fit)
struct SearchCapacity {
  int cu_count = 256;
  int blocks_per_cu[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};  // [plane][kind of pass kernel]; -1: not asked yet
};
// returns the most lanes per point of a planned launch, 0 for uniform tiles
int launch_icp_step_cnl(int dim, bool plane, const SliceDev& S, const GridLists& GL, const ProblemDev* probs,
                        ProblemState* states, int K, int max_nm, int team, hipStream_t s, const CtlParams* init_C = nullptr,
                        const InitInline* init_inl = nullptr, const InitBatch* init_bat = nullptr, int plan_lanes = 0,
                        bool plan_whole = false, long long plan_capacity = 0, SearchCapacity* cap = nullptr);
// Morton sort of K moving clouds (counts/cursor: (K << kbits) + 1 ints; bb: K*6 keys initialised to
// {0xffffffff x3, 0 x3}; counts zeroed)
// kbits = total key bits (2^kbits cells per cloud); aniso != 0: bits dealt to the axes by extent (kernels_prep.hip: KeySpec);
// segments = workgroups per cloud (0: automatic)
bool launch_msort_local(const float* src, int sf, const float* nsrc, int nsf, const ProblemDev* probs, int K, int dim, int kbits,
                        int aniso, int segments, int max_nm, float4* out_pts, float4* out_nrm, unsigned* maxabs_bits,
                        hipStream_t s);
void launch_msort(const float4* pts, const float4* nrm, const ProblemDev* probs, int K, int max_nm, int kbits, int aniso,
                  unsigned* bb, int* counts, int* cursor, int* scan_sums, int* scan_total, float4* out_pts,
                  float4* out_nrm, hipStream_t s);
void launch_icp_step(int dim, bool plane, const SliceDev& S, const ProblemDev* probs, ProblemState* states, int K,
                     int max_nm, hipStream_t s, const CtlParams* init_C = nullptr, const InitInline* init_inl = nullptr);
// search pass of a batch (no deferred-search queue) with every wave's neighbourhood of the fixed cloud staged in LDS
void launch_icp_step_tile(int dim, bool plane, const SliceDev& S, const ProblemDev* probs, ProblemState* states, int K,
                          int max_nm, int cap, hipStream_t s);
// iterations >= 1 of a compute(): the converged pass, ppt moving points per thread, + the deferred-search kernel if S.queue
void launch_icp_step_fast(int dim, bool plane, const SliceDev& S, const ProblemDev* probs, ProblemState* states, int K,
                          int max_nm, int ppt, bool gather, hipStream_t s);
// correspondence records of a nearest-neighbour slice, derived on demand from the state the last pass left behind
void launch_icp_outputs(int dim, bool plane, const SliceDev& S, const ProblemDev* probs, const ProblemState* states, int K,
                        int max_nm, hipStream_t s);
int icp_step_blocks(int max_nm);
int icp_queue_blocks(int max_nm, int K);
// projective slices: z-buffer reset + z-buffer kernel + step kernel (one ICP iteration of the slice)
void launch_proj_step_pack(const SliceDev* slices, const ProblemDev* const* probs, int nslices, ProblemState* states, int K,
                           int max_nm, hipStream_t s);
// ... sharing clouds and finder parameters: one z-buffer pass and one step launch for all of them
void launch_proj_records(const SliceDev& S0, const SliceDev& S, const ProblemDev* probs0, const ProblemDev* probs,
                         ProblemState* states, int K, int max_nm, bool rebuild, hipStream_t s);
void launch_proj_step_fused(const SliceDev* slices, const ProblemDev* const* probs, int nslices, ProblemState* states, int K,
                            int max_nm, hipStream_t s,
                            const CtlParams* init_C = nullptr, const InitInline* init_inl = nullptr, ProblemDev* probs_base = nullptr);
void launch_corr_step(int dim, bool plane, const SliceDev& S, const ProblemDev* probs, ProblemState* states, int K,
                      int max_ncorr, hipStream_t s);
void launch_proj_step(bool repro, const SliceDev& S, const ProblemDev* probs, ProblemState* states, int K, int max_nm,
                      hipStream_t s);
// (pairs: a pair batch, srrg2_align_pairs -- every problem's exponent from its own fixed normals: SliceCtl::ninf_bits[problem * PAIR_ROW_WORDS])
void launch_icp_init(const CtlParams& C, const ProblemDev* probs_host, ProblemDev* probs, ProblemState* states,
                     const float* guesses_host, int tsize, hipStream_t s, bool pairs = false);
// what k_icp_init gets of a single alignment in its arguments (guess, problem table); false: a batch (read from pinned memory)
bool make_init_inline(const CtlParams& C, const ProblemDev* probs_host, const float* guesses_host, int tsize, InitInline* inl);
void launch_icp_control(const CtlParams& C, ProblemState* states, srrg2_iteration_stats* stats, hipStream_t s);
// the last control step + post + finalize of a pack of projective slices on one wave (K == 1; the control parameters come from
// their device copy, FusedCtl::ctl)
void launch_icp_final_wave_pack(const SliceDev* slices, const ProblemDev* const* probs, int nslices, ProblemState* states,
                                srrg2_iteration_stats* stats, ProblemOut* outs_host, srrg2_iteration_stats* stats_host,
                                bool with_post, hipStream_t s);
void launch_icp_small(int dim, bool plane, const SliceDev& S, const CtlParams& C, const ProblemDev* probs, ProblemState* states,
                      srrg2_iteration_stats* stats, ProblemOut* outs_host, srrg2_iteration_stats* stats_host, hipStream_t s);
// pair batches (srrg2_align_pairs): k_icp_step / k_icp_step_fast / k_icp_small with grids[problem], the problem's own grid, in place
// of S.grid (control launches, no lists, tiles or deferred-search queue)
void launch_icp_step_pairs(int dim, bool plane, const SliceDev& S, const GridDev* grids, const ProblemDev* probs,
                           ProblemState* states, int K, int max_nm, hipStream_t s);
void launch_icp_step_fast_pairs(int dim, bool plane, const SliceDev& S, const GridDev* grids, const ProblemDev* probs,
                                ProblemState* states, int K, int max_nm, int ppt, bool gather, hipStream_t s);
void launch_icp_small_pairs(int dim, bool plane, const SliceDev& S, const GridDev* grids, const CtlParams& C, const ProblemDev* probs,
                            ProblemState* states, srrg2_iteration_stats* stats, ProblemOut* outs_host,
                            srrg2_iteration_stats* stats_host, hipStream_t s);
// pair batches, fixed side: the K concatenated clouds (fprobs: {offset, count} per pair) ingested in one launch with the per-pair rows
// (PAIR_ROW_WORDS each, zeroed by the caller); then the segmented grid build over the table of the pairs' grids (cell segments of
// ncell + 1 entries: the last counts the non-finite points, so that every segment's scan starts at its pair's offset)
void launch_pairs_ingest(const float* src, int sf, const float* nsrc, int nsf, const ProblemDev* fprobs, int K, int max_nf, int dim,
                         float4* dst, float4* dst_nrm, unsigned* rows, hipStream_t s);
void launch_pairs_grid_build(const GridDev* grids, const ProblemDev* fprobs, int K, int max_nf, int max_cells, int total_cells,
                             const float4* pts, const float4* nrm, int* cell_start, int* cursor, int* scan_sums, int* scan_total,
                             float4* out_pts, float4* out_nrm, int* pos_of, hipStream_t s);
// the last control step of a compute() with fused control steps (one nearest-neighbour cue slice): one wave per problem
void launch_icp_final_wave(const CtlParams& C, const SliceDev& S, ProblemState* states, srrg2_iteration_stats* stats,
                           ProblemOut* outs_host, srrg2_iteration_stats* stats_host, bool with_post, hipStream_t s);
void launch_icp_control_final(const CtlParams& C, ProblemState* states, srrg2_iteration_stats* stats, ProblemOut* outs_host,
                               srrg2_iteration_stats* stats_host, bool with_post, hipStream_t s);
void launch_icp_post(const CtlParams& C, ProblemState* states, const srrg2_iteration_stats* stats, hipStream_t s);
void launch_icp_finalize(const CtlParams& C, ProblemState* states, const srrg2_iteration_stats* stats,
                         ProblemOut* outs_host, srrg2_iteration_stats* stats_host, bool with_post, hipStream_t s);

}  // namespace srrg2amd
