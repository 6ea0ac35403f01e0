/*
 * include/e3d_hip.h -- C-ABI of libe3dhip.so (MI355X / gfx950 HIP implementation of the
 * ETH3D dataset-pipeline scan-alignment hot path).
 *
 * The reference has no FFI: its drop-in boundary is the C++ class surface that the tool
 * mains and gtest binaries call.  Every entry point below names the
 * reference interface it replaces (file:line relative to the reference tree).  A thin C++
 * shim with the reference's class and method names sits on top of this ABI
 * (dataset-pipeline_amd/csrc/host/icp_point_to_plane.h); INTEGRATION.md shows the binding a
 * maintainer would add to the reference.
 *
 * Conventions
 *   - all functions return int status: >= 0 success (value documented per function),
 *     E3D_ERR_* (< -1) on failure; e3d_last_error() returns a thread-local message.  Nothing
 *     aborts the process (the reference CHECK()s / throws instead).
 *   - point data is n x 3 float32, row-major ("xyz xyz ...").  Pointers may be host pointers
 *     or HIP device pointers (detected with hipPointerGetAttributes); the library copies what
 *     it needs into its own device buffers (SoA, sorted by grid cell), so callers keep
 *     ownership and may free their buffers after the call returns.
 *   - poses are row-major 3x4 float32 affine matrices (Eigen::Affine3f rows 0..2).
 *   - one host thread per handle; each handle owns one HIP stream on the device that was
 *     current when it was created.
 */
#ifndef E3D_HIP_H
#define E3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: e3d_reg_params grew by the three depth-residual fields; the ICP iteration record by the NN phase times (round 2)
 * 3: e3d_icp_iter_record grew by t_nn_sort_ms / t_nn_scan_ms / t_nn_compact_ms; e3d_comm_abort, e3d_reg_profile,
 *    e3d_icp_set_sequential_distance_sum (round 3)
 * 4: e3d_icp_set_resident_rows, e3d_comm_get_stats; iteration record: multi_cost_poses, lm_passes_skipped in the two reserved
 *    words, corr_rows_rewritten / corr_rows_walked appended (round 4)
 * 5: iteration record: nn_update_launches, nn_kernel_launches, nn_batches, nn_sort_calls appended (round 5: a batch of directed pairs
 *    per kernel launch) */
#define E3D_ABI_VERSION 5

#define E3D_ERR_INVALID   (-2)   /* bad argument / bad handle state          */
#define E3D_ERR_HIP       (-3)   /* a HIP runtime call failed                */
#define E3D_ERR_NO_DEVICE (-4)   /* no gfx950 device visible                 */
#define E3D_ERR_INDEX     (-5)   /* cloud index out of range (reference: .at() throws) */

/* ---- library ------------------------------------------------------------------------- */
int e3d_abi_version(void);
/* Select the HIP device for subsequently created handles; returns the device count. */
int e3d_init(int device);
const char* e3d_last_error(void);
/* Nearest-neighbour kernel selection for handles created afterwards: 0 = automatic (by points per grid
 * cell and grid size), 1 = one thread per query (sparse data), 2 = queries sorted by target cell + LDS-staged
 * candidate buckets found through the hash table (huge sparse grids), 3 = the same with the dense cell-start
 * directory and whole row segments per wave (default for dense scans).  All three are exact and return
 * identical results; the switch only exists for tests and profiling. */
int e3d_set_nn_mode(int mode);

/* ---- (A) icp::PointToPlaneICP  (src/icp/icp_point_to_plane.h:39-80) --------------------- */
typedef struct e3d_icp e3d_icp_t;

/* PointToPlaneICP::PointToPlaneICP()  (icp_point_to_plane.cc:107) */
e3d_icp_t* e3d_icp_create(void);
void e3d_icp_destroy(e3d_icp_t* icp);

/* int PointToPlaneICP::AddPointCloud(cloud, global_T_cloud, fixed)
 * (icp_point_to_plane.h:46-48, .cc:109-135).  Returns the cloud index (>= 0) for movable
 * clouds and -1 for fixed clouds (which are transformed once and merged into one fixed
 * cloud), exactly like the reference. */
int e3d_icp_add_cloud(e3d_icp_t* icp, const float* xyz, const float* normals, size_t n,
                      const float global_T_cloud[12], int fixed);

/* bool PointToPlaneICP::Run(max_correspondence_distance, initial_iteration,
 *   max_num_iterations, convergence_threshold_max_movement, print_progress)
 * (icp_point_to_plane.h:50-54, .cc:137-163).  Returns 1 if converged, 0 if not.  With
 * print_progress the reference's stdout lines are printed (same text; "avg. distance" is
 * accumulated in f64 on the device instead of a sequential f32 sum). */
int e3d_icp_run(e3d_icp_t* icp, float max_correspondence_distance, int initial_iteration,
                int max_num_iterations, float convergence_threshold_max_movement,
                int print_progress);

/* Eigen::Affine3f PointToPlaneICP::GetResultGlobalTCloud(int)  (icp_point_to_plane.h:56,
 * .cc:165-167). */
int e3d_icp_get_pose(e3d_icp_t* icp, int cloud_index, float global_T_cloud[12]);

/* Inner LM iteration cap of PointToPlaneICPImpl (reference constant 150,
 * icp_point_to_plane.cc:312); exposed for bounded benchmarks, default 150. */
int e3d_icp_set_max_inner_iterations(e3d_icp_t* icp, int n);
/* The "avg. distance" of the progress line and the pair records' distance_sum from the reference's own sum: f32, sequential, in
 * original source order (icp_point_to_plane.cc:226-229) -- byte-identical stdout of a single-rank run, at the price of one device -> host copy of the
 * distances and a host loop per pair and outer iteration.  Default off (environment E3D_ICP_SEQUENTIAL_DISTANCE_SUM=1 switches it
 * on for the tools): the f64 sum on the device, which does not stagnate at 2^24 times the typical term.  Ignored when sharded. */
int e3d_icp_set_sequential_distance_sum(e3d_icp_t* icp, int enable);
/* Correspondence rows of the LM passes.  1 (default; environment E3D_ICP_RESIDENT=0 flips it): every directed pair of the
 * certificate search keeps one RESIDENT row per query (48 B, source order, movable clouds in their local frame) for as long as
 * its grids live; an outer iteration rewrites only the rows whose partner changed and the LM passes apply the outer pose
 * (pcl::transformPointCloudWithNormals' operation order, icp_point_to_plane.cc:192-195) in front of the inner one -- the same
 * f32 numbers as rows written in the global frame.  0: all correspondences are gathered, transformed and compacted into fresh
 * rows every outer iteration (the reference's own data flow, icp_point_to_plane.cc:183-309; used automatically when the resident
 * rows do not fit HBM).  Same correspondences, counts and residuals either way; only the order of the f64 sums differs. */
int e3d_icp_set_resident_rows(e3d_icp_t* icp, int enable);

/* Per-pair correspondence report of every AlignMeshes call since creation -- the numbers the
 * reference only prints (icp_point_to_plane.cc:226-237).  src/tgt are the impl cloud indices
 * the reference prints; -1 stands for "fixed clouds". */
typedef struct {
  int32_t iteration;
  int32_t src, tgt;
  int64_t count;
  double  distance_sum;      /* sum of squared NN distances (f64 accumulation) */
} e3d_icp_pair_record;

typedef struct {
  int32_t iteration;
  int32_t inner_iterations;  /* LM iterations executed (<= 150)                            */
  int32_t full_passes;       /* fused H/b/cost passes over all correspondences             */
  int32_t cost_passes;       /* cost-only passes (one pose set)                            */
  int32_t multi_cost_passes; /* cost-only passes evaluating LM tries (0 or 1)..9 at once   */
  int32_t multi_cost_poses;  /* ABI 4: distinct new pose sets those passes evaluated (<= 10 each; tries whose f32 poses equal the
                                current ones or an earlier try's are not evaluated again)  */
  int64_t correspondences;   /* total over all directed pairs of this rank                 */
  int64_t queries;           /* NN queries issued by this rank                             */
  double  initial_cost, final_cost;
  double  t_transform_ms, t_nn_ms, t_lm_ms;   /* HIP-event times on the handle's stream   */
  double  t_lm_kernel_ms;    /* sum of LM pass kernel durations (HIP events)               */
  double  t_nn_query_ms;     /* sum of NN query kernel durations (HIP events)              */
  double  t_lm_full_kernel_ms; /* ... of the fused H/b/cost passes alone (k_lm_pass<1..3>)   */
  double  t_nn_certify_ms;   /* k_nn_certify launches (HIP events)                         */
  double  t_nn_bounded_ms;   /* k_nn_bounded launches                                      */
  double  t_nn_search_ms;    /* k_nn_rows / k_nn_cells / k_nn_query / k_nn_mfma launches   */
  int64_t nn_certify_queries, nn_bounded_queries, nn_search_queries;   /* queries those launches covered (nn_search_queries: the
                                  queries k_nn_rows visited -- those the key kernel settled because no target point lies in their
                                  27 cells are not among them; nn_certify_queries is 0 for a pair whose certificates were not
                                  tested in this iteration) */
  int32_t nn_certify_launches, nn_bounded_launches, nn_search_launches;
  int32_t lm_passes_skipped; /* ABI 4: LM passes not launched because every pose asked for had been evaluated already */
  /* ABI 3: the rest of the NN phase, so that the per-kernel times add up to the step (HIP events) */
  double  t_nn_sort_ms;      /* query keys (incl. settling the queries with an empty 27-cell block) + radix sort of the rest */
  double  t_nn_scan_ms;      /* match counts + scans (order-preserving compaction, first stage) */
  double  t_nn_compact_ms;   /* k_compact_corr / k_corr_update: the correspondence rows        */
  /* ABI 4 */
  int64_t corr_rows_rewritten; /* correspondence rows (48 B) written this iteration: every correspondence with compacted rows, the
                                  rows whose partner changed with resident rows                                        */
  int64_t corr_rows_walked;    /* rows one LM pass reads: the correspondences, or 64 x the active row groups of resident rows */
  /* ABI 5: launches of the NN phase (the all-pairs job's per-pair launches are what does not shrink with the number of GPUs) */
  int32_t nn_update_launches;  /* k_corr_update / k_compact_corr launches                                                */
  int32_t nn_kernel_launches;  /* all kernels the library itself launched in the NN phase (search, keys, row update, totals;
                                  the launches inside rocPRIM's radix sort are not counted: nn_sort_calls sorts)          */
  int32_t nn_batches;          /* batches of directed pairs that ran with one launch per kernel (0: pair by pair)          */
  int32_t nn_sort_calls;       /* radix sorts of query lists (k_nn_rows path)                                             */
} e3d_icp_iter_record;

size_t e3d_icp_num_pair_records(const e3d_icp_t* icp);
const e3d_icp_pair_record* e3d_icp_pair_records(const e3d_icp_t* icp);
size_t e3d_icp_num_iter_records(const e3d_icp_t* icp);
const e3d_icp_iter_record* e3d_icp_iter_records(const e3d_icp_t* icp);
void e3d_icp_clear_records(e3d_icp_t* icp);

/* Multi-GPU (one process per GPU): every rank holds all clouds and handles the slice
 * [n*rank/world, n*(rank+1)/world) of every directed pair's source cloud (in grid-cell order), so
 * any number of pairs -- including the 2 pairs of a 2-scan job -- shards evenly.  `allreduce` must sum `count` doubles in
 * place across ranks (RCCL/gloo through the host language; buffer is HOST memory) and leave
 * the identical result on every rank.  The reference has no equivalent (single process).
 * world_size == 1 with a callback is a tap: every buffer still passes through the callback (the sum over one rank is the
 * identity), which lets a caller record the reduced sums of a single-GPU run -- bench.py replays them to a handle that works as
 * rank 0 of a world of 8 on the same GPU to measure what one rank of an 8-GPU job does (its `scale_model`). */
typedef int (*e3d_allreduce_fn)(double* buffer, size_t count, void* user);
int e3d_icp_set_shard(e3d_icp_t* icp, int rank, int world_size,
                      e3d_allreduce_fn allreduce, void* user);

/* Native collectives: an RCCL communicator owned by the library (one rank per GPU, xGMI inside a node).  The per-pair
 * normal-equation blocks of every LM pass are reduced on the GPU and all-reduced in place on the handle's stream, the
 * counts once per outer iteration; no host hop and no callback.  Ranks are either processes (rank 0: e3d_comm_unique_id,
 * the 128 bytes travel through the launcher's rendezvous, every rank: e3d_comm_create) or host threads of one process
 * (e3d_comm_create_all: out[i] is the communicator of devices[i], devices == NULL means 0..n-1).  world_size = 1 is valid
 * (the collectives then run with a single rank).  e3d_icp_set_comm replaces e3d_icp_set_shard; the communicator must
 * outlive the handle and live on the handle's device. */
#define E3D_COMM_ID_BYTES 128
typedef struct e3d_comm e3d_comm_t;
int e3d_comm_unique_id(char id[E3D_COMM_ID_BYTES]);
e3d_comm_t* e3d_comm_create(const char id[E3D_COMM_ID_BYTES], int rank, int world_size, int device);
int e3d_comm_create_all(int n_devices, const int* devices, e3d_comm_t** out);
void e3d_comm_destroy(e3d_comm_t* comm);
/* Aborts the communicator (ncclCommAbort): an enqueue or a collective of THIS communicator that waits for a rank that will never
 * arrive returns with an error instead of blocking forever.  Callable from any host thread, also while the communicator's own
 * thread is inside a collective (no lock is shared with the enqueue); every later collective on `comm` fails; the object is still
 * released with e3d_comm_destroy.  Aborting one communicator does not release its peers: when a rank's step fails the tools abort
 * ALL local communicators (--gpus N, csrc/host/icp_point_to_plane.h). */
int e3d_comm_abort(e3d_comm_t* comm);
/* HIP-event time, number and payload of the all-reduces enqueued on `comm` since creation (or the last reset): what the bench
 * line reports per rank at N > 1 (ABI 4).  Waits for the collectives enqueued so far.  To be called from the host thread that
 * enqueues on `comm` (or after joining it): the counters are not synchronised against a running enqueue. */
int e3d_comm_get_stats(e3d_comm_t* comm, double* allreduce_ms, int64_t* allreduce_calls, int64_t* allreduce_bytes, int reset);
int e3d_comm_rank(const e3d_comm_t* comm);
int e3d_comm_world_size(const e3d_comm_t* comm);
int e3d_icp_set_comm(e3d_icp_t* icp, e3d_comm_t* comm);

/* ---- stand-alone kernels behind the same arithmetic (parity tests, other callers) ------ */

/* FindCorrespondencesFast(source, target, max_correspondence_distance)
 * (icp_point_to_plane.cc:42-105): for every source point the exact nearest target point with
 * squared distance < (float)(d*d), lowest target index on ties.  match_index[i] = target index
 * or -1; sq_distance[i] valid where matched.  Returns the number of correspondences. */
int64_t e3d_find_correspondences(const float* source_xyz, size_t n_source,
                                 const float* target_xyz, size_t n_target,
                                 float max_correspondence_distance,
                                 int32_t* match_index, float* sq_distance);

/* pcl::transformPointCloudWithNormals + AlignedBox extend (icp_point_to_plane.cc:189-205). */
int e3d_transform_cloud(const float* xyz, const float* normals, size_t n, const float T[12],
                        float* out_xyz, float* out_normals, float bbox_min[3], float bbox_max[3]);

/* One accumulate pass of PointToPlaneICPImpl::compute (icp_point_to_plane_impl.h:119-211) for
 * one directed pair at inner poses {q = w,x,y,z ; t}.  Outputs the 12x12 pair system over
 * [source(6), target(6)] (row-major, upper triangle filled, lower mirrored), b(12), cost. */
int e3d_icp_pair_system(const float* src_xyz, const float* src_normals,
                        const float* tgt_xyz, const float* tgt_normals,
                        const int32_t* index_query, const int32_t* index_match, int64_t n_corr,
                        const float src_q[4], const float src_t[3],
                        const float tgt_q[4], const float tgt_t[3],
                        double H[144], double b[12], double* cost);

/* ---- (A') pcl::NormalEstimationTwoPassOMP (src/geometry/two_pass_normal_3d_omp.h:53-99) - */
/* setInputCloud + setKSearch(k) + setViewPoint + compute  (call sites
 * src/exe/icp_scan_aligner.cc:323-330, src/exe/normal_estimator.cc:177-194).
 * out_normals n x 3, out_curvature n.  knn_indices (optional, n*k int32) receives each point's
 * neighbour list sorted by (squared distance, index).  Pointers may be host or device memory: a
 * cloud in device memory is read in place, and results for device out_normals / out_curvature are
 * written by the kernels directly (no staging copies; the call still returns after its stream
 * has finished).  The library works on its own stream: device inputs must be complete (the
 * caller's stream work that produces them finished) when the call is made. */
int e3d_normals_knn(const float* xyz, size_t n, int k, const float viewpoint[3],
                    float* out_normals, float* out_curvature, int32_t* knn_indices);

/* Test hook: the bit-defined elementary functions of include/e3d_libm.h evaluated by a HIP kernel (n values, host or device
 * pointers).  fn: 0 atanf(x), 1 atan2f(x, y), 2 sinf(x), 3 cosf(x), 4 tanf(x), 5 log2f(x).  The reference calls the C library
 * at these places (pcl::eigen33 for src/geometry/two_pass_normal_3d.h:92-109, src/camera/camera_base_impl_fisheye.h:66-153,
 * src/opt/visibility_estimator.cc:437); kernels, host code and oracle all use this one implementation instead. */
int e3d_libm_eval(int fn, const float* x, const float* y, size_t n, float* out);

/* e3d_normals_knn / e3d_local_outlier_removal keep their device workspace (the sort, grid and list buffers of the last call, per
 * device) for the next call instead of paying hipMalloc / hipFree every time; this frees what is parked.  Workspaces larger than
 * E3D_WORKSPACE_KEEP_GB (environment, default 32) are never kept.  No counterpart in the reference (PCL allocates per call). */
int e3d_release_workspaces(void);

/* The same estimator with setRadiusSearch(radius) instead of setKSearch: every point strictly within the radius
 * (squared distance < (float)((double)radius * radius)) takes part; fewer than 3 -> NaN.  neighbor_counts (optional, n)
 * receives the number of points found, the query itself included. */
int e3d_normals_radius(const float* xyz, size_t n, float radius, const float viewpoint[3],
                       float* out_normals, float* out_curvature, int32_t* neighbor_counts);

/* pcl::LocalStatisticalOutlierRemoval<PointT>::applyFilterIndices (src/geometry/local_statistical_outlier_removal.hpp:71-172),
 * the filter of PointCloudCleaner (src/exe/point_cloud_cleaner.cc:80-107) and of the multi-resolution pipeline's callers.
 * First pass: per point the mean distance to its mean_k nearest neighbours (exact kNN with k = mean_k + 1, entry 0 being
 * the point itself; f64 sum of the f32 roots of FLANN's squared f32 distances, stored as f32).  Second pass: a point is
 * removed if its own value exceeds distance_factor_threshold x the f64 mean of its neighbours' (positive) values
 * (`negative` inverts the test like setNegative).  inlier[i] = 1 for points the filter keeps; non-finite points are never
 * kept.  mean_distances (optional, n floats) receives the first-pass values.  Neighbours at exactly equal distance are
 * ordered by index (FLANN's order there is unpinned).  1 <= mean_k <= 1023 (the ETH3D clouds were cleaned with 270 and 20);
 * the neighbour lists take n x (mean_k + 1) x 4 bytes of device memory. */
int e3d_local_outlier_removal(const float* xyz, size_t n, int mean_k, double distance_factor_threshold, int negative,
                              uint8_t* inlier, float* mean_distances);

/* ---- SplatCreator (src/exe/splat_creator.cc:75-235) ------------------------------------------------------------
 * igl::AABB<MatrixXf,3>::squared_distance (thirdparty/igl/AABB.cpp:344-430) over a triangle mesh: per point the minimum over
 * all triangles of point_simplex_squared_distance (f32, Ericson ch. 5) if it is <= max_sq_distance, else +inf (non-finite
 * points: +inf).  closest_triangle (optional, n): the triangle of the minimum, the lowest id among equal minima, -1 with +inf.
 * vertices n_vertices x 3, triangles n_triangles x 3 vertex indices; host or device pointers; a GPU index over the triangles
 *  is built per call. */
int e3d_mesh_squared_distance(const float* points, size_t n, const float* vertices, size_t n_vertices,
                              const uint32_t* triangles, size_t n_triangles, float max_sq_distance,
                              float* sq_distance, int32_t* closest_triangle);
/* SplatCreator (src/exe/splat_creator.cc:75-235): returns the number of splats m (< 0: error).  A point with a NaN normal
 * component is skipped; the splat radius is min(sqrtf(5th smallest squared distance of a k = 5 search that includes the
 * point), max_splat_size); a splat is added if the centre or one of its corners is farther than distance_threshold from the
 * mesh.  Points with a non-finite coordinate are neither searched nor splatted; fewer than 5 finite points is an error.
 * splat_vertices: the first min(m, capacity) splats, 12 floats each (corners TR, BR, BL, TL) in ascending point order; the
 * faces of splat s are (4s+2, 4s+1, 4s) and (4s, 4s+3, 4s+2).  splat_vertices == NULL with capacity 0 only counts.
 * add_splat / splat_radius (optional, n each): per point 0/1 and the radius (NaN for skipped points).  timings_ms (optional,
 * 2 floats): index build and splat pass in ms (HIP events).  Host or device pointers. */
int64_t e3d_create_splats(const float* xyz, const float* normals, size_t n, const float* vertices, size_t n_vertices,
                          const uint32_t* triangles, size_t n_triangles, float distance_threshold, float max_splat_size,
                          float* splat_vertices, size_t capacity, uint8_t* add_splat, float* splat_radius, float* timings_ms);

/* ---- CubeMapRenderer (src/exe/cube_map_renderer.cc:161-373) ----------------------------------------------------
 * Six pinhole faces (front, left, back, right, down, up; fx = fy = cx = cy = size / 2) of a coloured scan given in the
 * scanner's frame.  Point pass (:238-258): per pixel the lowest depth, among equal depths the lowest point index; a point
 * with a non-finite coordinate lands in no face.  fill != 0 adds the fill-in of :260-319 (interior pixels: depth from the
 * median of the first 3 / 5 / 7 valid neighbours, colour from the mean of all of them; border pixels get depth +inf) and
 * the colour dilation of :321-373 (3 x 3 means of the valid pixels, repeated until every pixel has a colour).  fill == 0
 * returns the raw z-buffer.  Results equal a serial execution bit for bit.  Where the reference is undefined: border pixels
 * of a face that needs no dilation are black, and a face without any valid pixel stays black.
 * xyz n x 3 floats, rgb n x 3 bytes (R, G, B); host or device pointers.  color_out 6 * size * size * 3 bytes (R, G, B),
 * depth_out 6 * size * size floats (+inf = no depth), sweeps_out (optional) six ints: dilation sweeps per face that gave at
 * least one pixel its colour (= the reference's loop iterations).  size >= 3, n < 2^31. */
int e3d_render_cube_map(const float* xyz, const uint8_t* rgb, size_t n, int size, int fill, uint8_t* color_out,
                        float* depth_out, int32_t* sweeps_out);
/* Times of this thread's last e3d_render_cube_map (HIP events, ms): [0] point pass, [1] resolve, [2] fill-in pass 1,
 * [3] dilation including its read-backs, [4] batches of sweeps looked at, [5] sweeps launched, [6..7] reserved. */
#define E3D_CUBE_MAP_TIMINGS 8
int e3d_cube_map_timings(float* out);

/* ---- (B) ImageRegistrator: dense photometric residual / Jacobian kernels -------------------------------------
 * Device-resident mirror of the parts of opt::Problem the hot loops read (src/opt/problem.h:300-388) and the inner
 * operator surfaces of the optimizer:
 *   OcclusionGeometry::RenderDepthMap (CPU-splat path)      src/opt/occlusion_geometry.cc:404-464      -> e3d_reg_render_depth
 *   VisibilityEstimator::AppendObservationsFor...           src/opt/visibility_estimator.cc:258-295,366-532 -> e3d_reg_observe
 *   VisibilityEstimator::DetermineIfAllNeighborsAreObserved src/opt/visibility_estimator.cc:199-256    -> (inside e3d_reg_observe)
 *   IntrinsicsAndPoseOptimizer::AccumulateHAndBAndResidualsForObservations
 *                                                           src/opt/intrinsics_and_pose_optimizer.cc:624-1296 -> e3d_reg_accumulate
 *   CostCalculator::AccumulateResidualsForObservations      src/opt/cost_calculator.cc:102-271         -> e3d_reg_cost
 *   ColorOptimizer::Apply                                   src/opt/color_optimizer.cc:40-123          -> e3d_reg_color_*
 * Coverage: every camera model of the reference's factory, non-rig and rig images, colour residuals (fixed + variable descriptors),
 * image and camera masks, depth-map residuals (off by default, as in the reference; not for the dependent images of a rig, which the
 * reference aborts on). */
typedef struct e3d_reg e3d_reg_t;

typedef struct {
  int32_t point_neighbor_count;        /* K, opt::Parameters::point_neighbor_count (parameters.h:42)   */
  int32_t robust_weighting_type;       /* 0 none, 1 Huber, 2 Tukey (robust_weighting.h:40-44)           */
  float   robust_weighting_parameter;
  float   fixed_residuals_weight;
  float   variable_residuals_weight;
  float   maximum_valid_intensity;     /* 252                                                           */
  float   occlusion_depth_threshold;   /* 0.01                                                          */
  float   splat_radius;                /* 0.03                                                          */
  int32_t current_image_scale;         /* Problem::current_image_scale()                                */
  int32_t image_scale_count;           /* Problem::image_scale_count()                                  */
  /* depth-based residuals (parameters.h:53-55,165-172: "not used in ETH3D pipeline"; 0 = disabled, the reference's default) */
  float   depth_residuals_weight;
  int32_t depth_robust_weighting_type; /* 2 (Tukey)                                                     */
  float   depth_robust_weighting_parameter;   /* 0.02                                                   */
} e3d_reg_params;

/* camera models (COLMAP names, src/camera/camera_base.cc:66-77) and their parameter counts:
 * PINHOLE fx fy cx cy (camera_pinhole.h:40-86); OPENCV + k1 k2 p1 p2 (camera_polynomial_tangential.h:41-159);
 * THIN_PRISM_FISHEYE + k1 k2 p1 p2 k3 k4 sx1 sy1 (camera_benchmark.h:44-52); OPENCV_FISHEYE + k1 k2 k3 k4
 * (camera_fisheye_polynomial_4.h:42-50 over camera_polynomial_4.h:43-135); FOV + omega (camera_fisheye_fov.h:44-176);
 * SIMPLE_PINHOLE f cx cy (camera_simple_pinhole.h:41-88); SIMPLE_RADIAL f cx cy k (camera_simple_radial.h:43-110); RADIAL f cx cy k1 k2
 * (camera_radial.h:43-123); POLYNOMIAL_3 fx fy cx cy k1 k2 k3 (camera_polynomial.h:43-127); FISHEYE_POLYNOMIAL_2_TANGENTIAL_2 fx fy cx cy
 * k1 k2 p1 p2 (camera_fisheye_polynomial_tangential.h).  Parameter vectors, Jacobian columns and e3d_reg_get_intrinsics_level follow the
 * class's GetParameters order. */
#define E3D_CAMERA_PINHOLE 0             /* I = 4  */
#define E3D_CAMERA_OPENCV 1              /* I = 8  */
#define E3D_CAMERA_THIN_PRISM_FISHEYE 2  /* I = 12 */
#define E3D_CAMERA_OPENCV_FISHEYE 3      /* I = 8  */
#define E3D_CAMERA_FOV 4                 /* I = 5  */
#define E3D_CAMERA_SIMPLE_PINHOLE 5      /* I = 3: f cx cy                  (one focal length: parameter order as in COLMAP) */
#define E3D_CAMERA_SIMPLE_RADIAL 6       /* I = 4: f cx cy k                (also the name SIMPLE_RADIAL_FISHEYE, camera_base.cc:74) */
#define E3D_CAMERA_RADIAL 7              /* I = 5: f cx cy k1 k2            (also the name RADIAL_FISHEYE, camera_base.cc:73) */
#define E3D_CAMERA_POLYNOMIAL_3 8        /* I = 7: fx fy cx cy k1 k2 k3 */
#define E3D_CAMERA_FISHEYE_POLYNOMIAL_2_TANGENTIAL_2 9   /* I = 8: fx fy cx cy k1 k2 p1 p2 */
/* the three classes of src/camera that the reference's factory never creates (camera_base.cc:66-77): no camera name reaches them */
#define E3D_CAMERA_FULL_OPENCV 10        /* I = 12: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6   (camera_full_opencv.h:41-196) */
#define E3D_CAMERA_RADIAL_FISHEYE_CLASS 11         /* I = 5: f cx cy k1 k2   RadialFisheyeCamera = FisheyeBase over RadialCamera */
#define E3D_CAMERA_SIMPLE_RADIAL_FISHEYE_CLASS 12  /* I = 4: f cx cy k       SimpleRadialFisheyeCamera = FisheyeBase over SimpleRadialCamera */

e3d_reg_t* e3d_reg_create(const e3d_reg_params* params);
void e3d_reg_destroy(e3d_reg_t* reg);
int e3d_reg_set_params(e3d_reg_t* reg, const e3d_reg_params* params);

/* One point scale of the multi-resolution cloud: points()[s], point radius, neighbor_point_indices_[s] (n*K, u32),
 * fixed_descriptors()[s] (n*K or NULL).  Variable descriptors start at 0 and observation counts at 99999 when fixed
 * descriptors are given (problem.cc:549-572), else 0. */
int e3d_reg_set_point_scale(e3d_reg_t* reg, int point_scale, const float* xyz, size_t n, float point_radius,
                            const uint32_t* neighbor_indices, const float* fixed_descriptors);
int e3d_reg_set_variable_descriptors(e3d_reg_t* reg, int point_scale, const float* descriptors,
                                     const int32_t* observation_counts);
int e3d_reg_get_variable_descriptors(e3d_reg_t* reg, int point_scale, float* descriptors, int32_t* observation_counts);

/* opt::Intrinsics: the model of the best available scale + its ScaledBy(0.5) pyramid of n_levels models
 * (intrinsics.cc:46-51, camera_base_impl.h:70-89) and radius cut-offs (camera_base_impl.h:410-463). */
int e3d_reg_set_intrinsics(e3d_reg_t* reg, int intrinsics_id, int camera_type, int width, int height,
                           const float* parameters, int n_parameters, int min_image_scale, int n_levels);

/* Intrinsics::camera_mask (src/opt/intrinsics.h:104; loaded once per camera by Image::LoadImageData, src/opt/image.cc:62-72): one u8
 * mask per pyramid level of the camera (level_masks[l]: width_l x height_l bytes, host or device memory, or NULL), shared by all
 * images of these intrinsics.  An observation is dropped where the image's own mask OR the camera mask is non-zero
 * (src/opt/visibility_estimator.cc:335-345, 482-503).  level_masks == NULL removes the mask.  Call after e3d_reg_set_intrinsics;
 * parameter updates of the optimiser keep it. */
int e3d_reg_set_camera_mask(e3d_reg_t* reg, int intrinsics_id, const uint8_t* const* level_masks);

/* Depth residuals (src/opt/intrinsics_and_pose_optimizer.cc:747-757, 1150-1214; cost_calculator.cc:221-245; problem.cc:593-631):
 * residual = 1 / (depth map interpolated at the observation) - 1 / (depth of the point in the image frame), one per observation,
 * weighted by e3d_reg_params.depth_residuals_weight with its own robust weighting.  Off by default and unused by the reference's
 * tools (no tool loads depth maps; its alignment test does, test_alignment.cc:469-500).  As in the reference the non-reference
 * images of a rig are not supported with depth residuals by default (:1199-1207 aborts) -- here that is an error return.
 *   e3d_reg_set_rig_depth_residuals(enable != 0) lifts that for this handle (default 0; e3d_reg_set_params keeps it): the two Jacobian
 *     terms the reference leaves open are supplied (d z / d extrinsics = row 2 of [I | -[T]x], d z / d rig pose = row 2 of
 *     R_image_rig [I | -[G]x], T = image_T_global * point, G = rig_T_global * point), and every call below accepts such images.
 *   e3d_reg_set_depth_maps: Problem::SetFixedDepthMaps for one image, one f32 map per pyramid level of its camera (caller-built
 *     pyramid, like the test's cv::resize INTER_AREA chain); NULL removes them.  Required for every image once the weight is > 0.
 *   e3d_reg_set_depth_map_level0: the same buffers from one full-resolution map (width x height floats of the image's camera,
 *     row-major, host or device memory); the pyramid is built on the device, one level per level of the camera pyramid (level sizes
 *     as e3d_reg_get_intrinsics_level reports them: int(0.5 w + 0.5)).  Afterwards every depth call behaves as if that pyramid had
 *     been passed to e3d_reg_set_depth_maps.  Arithmetic (bit-exact, so that a restatement can be compared with ==):
 *       level 0: a pixel is valid iff it is finite and > 0; every other pixel (NaN, +-inf, negative, -0) becomes +0.0f, the
 *         "no depth" of the depth kernels (ground-truth maps hold +inf where nothing was drawn);
 *       level l + 1 from level l: with a, b, c, d the pixels (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1) of level l, coordinates
 *         clamped to the last row and column, pixel (y, x) = (float)(0.25 * ((((double)a + b) + c) + d));
 *       E3D_DEPTH_HOLES_STRICT: if any of the four (clamped) source pixels is 0 the result is +0.0f;
 *       E3D_DEPTH_HOLES_AVERAGE: the plain box mean (holes count as depth 0 and pull the mean down).
 *     Errors: null handle or pointer, unknown image, unknown hole_mode.
 *   e3d_reg_get_depth_map: one level of an image's depth maps (width_l x height_l floats) back to the host, whichever call set
 *     them; an error if the image has none or the level is out of range.
 *   e3d_reg_depth_accumulate / e3d_reg_depth_cost: the depth part of AccumulateHAndBForImage / ComputeResidualsForImage for one
 *     (image, point scale); e3d_reg_apply, e3d_reg_compute_cost and e3d_reg_run_on_current_scale include them by themselves.
 *     H is the V x V upper triangle (row-major) and b has V entries, V = the image's local unknowns as in e3d_reg_accumulate:
 *     I + 6 [intrinsics, pose], or I + 12 [intrinsics, rig extrinsics, rig pose] for a non-reference rig image. */
int e3d_reg_set_depth_maps(e3d_reg_t* reg, int image_id, const float* const* level_depths);
#define E3D_DEPTH_HOLES_AVERAGE 0   /* plain 2x2 box mean: the cv::resize INTER_AREA chain of test_alignment.cc:485-489 */
#define E3D_DEPTH_HOLES_STRICT  1   /* a 2x2 block with an invalid pixel gives an invalid pixel */
int e3d_reg_set_depth_map_level0(e3d_reg_t* reg, int image_id, const float* depth, int hole_mode);
int e3d_reg_get_depth_map(e3d_reg_t* reg, int image_id, int level, float* out);
int e3d_reg_set_rig_depth_residuals(e3d_reg_t* reg, int enable);
int e3d_reg_depth_accumulate(e3d_reg_t* reg, int image_id, int point_scale, double* H, double* b, double* sum, int64_t* count);
int e3d_reg_depth_cost(e3d_reg_t* reg, int image_id, int point_scale, double* sum, int64_t* count);
/* queries one level of the pyramid the library built: size, parameters (n_parameters floats) and the radius cut-off
 * (+inf for PINHOLE; for the fisheye models the cut-off of the inner non-fisheye model, which is the one projection tests) */
int e3d_reg_get_intrinsics_level(e3d_reg_t* reg, int intrinsics_id, int level, int* width, int* height,
                                 float* parameters, float* radius_cutoff_squared);
/* opt::Image: u8 pyramid (level l has the size of intrinsics level l) and optional masks; pose image_T_global as the
 * Sophus::SE3f state: unit quaternion {w, x, y, z} + translation (what COLMAP images.txt stores).  level_pixels == NULL (then
 * level_masks must be NULL too) sets an image without pixels: its id, intrinsics and pose serve the calls that ask about geometry
 * only (e3d_reg_render_depth, the scan visibility calls, e3d_reg_stereo_plan / _ground_truth); calls that read intensities refuse it.
 * Under e3d_reg_set_shard the images of other ranks are set this way. */
int e3d_reg_set_image(e3d_reg_t* reg, int image_id, int intrinsics_id, const uint8_t* const* level_pixels,
                      const uint8_t* const* level_masks);
int e3d_reg_set_image_pose(e3d_reg_t* reg, int image_id, const float q[4], const float t[3]);
int e3d_reg_get_image_pose(e3d_reg_t* reg, int image_id, float q[4], float t[3]);
/* Camera rigs (src/opt/rig.h:41-76, RigImages in src/opt/problem.h): image_T_rig of every camera (n_cameras x {w,x,y,z},
 * n_cameras x 3; camera 0 is the reference), and frames = one image id per camera, image_ids[0] being the reference
 * image whose pose is the rig pose.  The other images' poses are derived: image_T_rig[c] * image_T_global(reference)
 * (intrinsics_and_pose_optimizer.cc:539-548); they contribute the 6 extrinsics unknowns of their camera and the 6 pose
 * unknowns of the reference image (:140-153, Rig::Update rig.cc:9-23). */
int e3d_reg_set_rig(e3d_reg_t* reg, int rig_id, int n_cameras, const float* q, const float* t);
int e3d_reg_get_rig(e3d_reg_t* reg, int rig_id, int camera_index, float q[4], float t[3]);
int e3d_reg_add_rig_images(e3d_reg_t* reg, int rig_id, const int* image_ids, int n_cameras);
/* OcclusionGeometry::SetSplatPoints */
int e3d_reg_set_splat_points(e3d_reg_t* reg, const float* xyz, size_t n);

/* OcclusionGeometry::AddMesh / AddSplats (src/opt/occlusion_geometry.cc:64-182): occlusion geometry as triangle meshes,
 * used when no splat points are set (OcclusionGeometry::RenderDepthMap :211-271).  The reference renders them with OpenGL
 * (src/opengl/renderer.cc); here a software rasteriser with the same conventions (vertex-shader distortion per camera
 * model, depth = camera-space z, nearest fragment, 0 where there is no geometry, near / far planes min / max occlusion
 * depth) followed by MaskOutOcclusionBoundaries (:284-402) over the edges extracted when compute_edges != 0
 * (ComputeEdgeNormalsList / FilterEdgeList :488-645).  Vertices are global-frame xyz, triangles 3 x u32.  Returns the
 * number of meshes held. */
int e3d_reg_add_occlusion_mesh(e3d_reg_t* reg, const float* vertices, size_t n_vertices, const uint32_t* triangles,
                               size_t n_triangles, int compute_edges);
int e3d_reg_clear_occlusion_meshes(e3d_reg_t* reg);
int e3d_reg_set_occlusion_options(e3d_reg_t* reg, float min_depth, float max_depth, int mask_occlusion_boundaries);
int64_t e3d_reg_occlusion_edge_count(e3d_reg_t* reg, int mesh_index);

/* Measurement: HIP-event durations of the two kernels behind e3d_reg_accumulate, summed over its calls since the last reset:
 * out = {pass 1 ms (k_reg_pass1: per-observation intensity + Jacobian rows), pass 2 ms (k_reg_pass2 / k_reg_pass2_mfma: residuals and
 * normal equations), observations processed, calls}. */
int e3d_reg_kernel_times(e3d_reg_t* reg, double out[4], int reset);
/* Wall-clock split of e3d_reg_run_on_current_scale by phase (accumulate, host solve, trial states, re-projection, costs, occlusion
 * depth maps, visibility, colour update).  enable = 1 switches it on (the library then synchronises its stream at every phase
 * boundary: the run gets slower, the split adds up), 0 off; `out` (may be NULL) receives "phase=milliseconds;..." of the phases
 * recorded so far, followed (ABI 4) by one "k:group=milliseconds,launches,units;" entry per kernel group of the iteration (HIP events
 * on the handle's stream, no synchronisation of their own; units = the points, observations, pixels or triangles the launches
 * covered -- what bench.py prices a group's algorithmic bytes with).  Switching clears the record.  Measurement only -- no effect on
 * results. */
int e3d_reg_profile(e3d_reg_t* reg, int enable, char* out, size_t capacity);

/* Renders the occlusion depth map of an image at an image scale (kept on the device for e3d_reg_observe);
 * depth_out (optional) receives height x width floats. */
int e3d_reg_render_depth(e3d_reg_t* reg, int image_id, int image_scale, float* depth_out);
/* Creates the observations of a point scale in an image (indices == NULL: every point, with occlusion, mask and
 * over-saturation tests against the last rendered depth map of this image and scale; indices != NULL: the given
 * visibility list without those tests) in point order, and their all-neighbours-observed flags.  Returns the count.
 * border_size >= 0 (E3D_ERR_INVALID otherwise, here and in e3d_reg_update_observations). */
int64_t e3d_reg_observe(e3d_reg_t* reg, int image_id, int point_scale, int image_scale, int border_size,
                        const uint32_t* indices, size_t n_indices);
int e3d_reg_get_observations(e3d_reg_t* reg, int image_id, int point_scale, uint32_t* point_index, float* x, float* y,
                             float* image_scale, uint8_t* all_neighbors_observed);
int e3d_reg_set_observations(e3d_reg_t* reg, int image_id, int point_scale, size_t n, const uint32_t* point_index,
                             const float* x, const float* y, const float* image_scale);
/* ComputePointIntensityAndJacobians for every observation (n x 1, n x I, n x 6); mainly for tests. */
int e3d_reg_pass1(e3d_reg_t* reg, int image_id, int point_scale, float* intensities, float* j_intrinsics, float* j_pose);
/* H: V x V row-major, upper triangle filled; b: V.  V = I + 6 with variables [intrinsics(I), pose(6)], or V = I + 12 with
 * [intrinsics(I), rig extrinsics(6), pose of the rig frame's reference image(6)] for a non-reference rig image;
 * sums / counts: [fixed, variable] robust residual sums and residual counts. */
int e3d_reg_accumulate(e3d_reg_t* reg, int image_id, int point_scale, double* H, double* b, double sums[2],
                       int64_t counts[2]);
int e3d_reg_cost(e3d_reg_t* reg, int image_id, int point_scale, double sums[2], int64_t counts[2]);
int e3d_reg_color_begin(e3d_reg_t* reg, int point_scale);
int e3d_reg_color_accumulate(e3d_reg_t* reg, int image_id, int point_scale);
int e3d_reg_color_finish(e3d_reg_t* reg, int point_scale);

/* Whole-problem steps of opt::Optimizer::RunOnCurrentScale (src/opt/optimizer.cc:49-182) on the device-resident state.
 * Images are visited in ascending image id. */
/* VisibilityEstimator::CreateObservationsForAllImages + DetermineIfAllNeighborsAreObserved (optimizer.cc:119-128); with
 * e3d_reg_set_cache_observations(1) it is ObservationsCache::GetObservations (observations_cache.cc:52-68) instead. */
int e3d_reg_update_observations(e3d_reg_t* reg, int border_size);
/* GroundTruthCreator (src/exe/ground_truth_creator.cc): visibility of the full-resolution scan points in the registered images.
 *   e3d_reg_set_scan_points: the (global-frame) scan points whose observations are counted; counts start at 0.
 *   e3d_reg_count_scan_observations: AccumulateScanObservationsForImage (:45-86) for one image -- occlusion depth map at the
 *     highest available resolution (RenderDepthMap at intrinsics.min_image_scale), then for every scan point: z > 0, rounded
 *     pixel inside the image, occlusion_image + occlusion_depth_threshold >= z, and mask(iy, ix) != excluded_flag (pass the
 *     level-0 image mask and opt::MaskType::kEvalObs = 2; NULL = no mask) -> count += 1.
 *   e3d_reg_get/set_scan_observation_counts: the counters (one int per scan point, input order).  With image sharding every
 *     rank counts its own images; the caller adds the vectors.
 *   e3d_reg_ground_truth_depth: the depth-map part of CreateGroundTruthForImage (:104-117, :146-189): gt_depth (w x h floats,
 *     +inf where nothing was seen) = min z over the visible points with count >= min_count (the tool uses 2); occlusion_depth
 *     (optional) receives the occlusion depth map the tool writes to occlusion_depth/. */
int e3d_reg_set_scan_points(e3d_reg_t* reg, const float* xyz, size_t n);
int e3d_reg_count_scan_observations(e3d_reg_t* reg, int image_id, const uint8_t* mask, int excluded_flag);
int e3d_reg_get_scan_observation_counts(e3d_reg_t* reg, int32_t* counts);
int e3d_reg_set_scan_observation_counts(e3d_reg_t* reg, const int32_t* counts);
int e3d_reg_ground_truth_depth(e3d_reg_t* reg, int image_id, const uint8_t* mask, int excluded_flag, int min_count, float* gt_depth,
                               float* occlusion_depth);
/* CreateGroundTruthForImage, scan rendering part (src/exe/ground_truth_creator.cc:149,175-187): the reference paints a square of
 * 2 * point_radius + 1 pixels over the image for every visible scan point seen in >= min_count images, in point order.  The result
 * per pixel is the LAST point covering it: winner[y * width + x] = point index + 1 (order of e3d_reg_set_scan_points), 0 = untouched. */
int e3d_reg_scan_rendering(e3d_reg_t* reg, int image_id, const uint8_t* mask, int excluded_flag, int min_count, int point_radius,
                           uint32_t* winner);
/* Problem::DebugWriteColoredPointCloud (src/opt/problem.cc:642-704), the output of ImageRegistrator --write_debug_point_clouds
 * (src/exe/image_registrator.cc:202-215, :287-295): the scan points of e3d_reg_set_scan_points coloured by the images at their
 * current poses.
 *   e3d_reg_scan_colors_begin: zero colour sums and observation counts (problem.cc:644-649).
 *   e3d_reg_scan_colors_add_image: one image of this rank (problem.cc:655-682).  Observations without scale test
 *     (VisibilityEstimator::AppendObservationsForImageNoScale, visibility_estimator.cc:117-138, :297-364): occlusion depth map, camera
 *     level, masks and grey values at best_available_image_scale(max(min_occlusion_check_image_scale (0), current_image_scale)); z > 0,
 *     rounded pixel inside the level, occlusion + occlusion_depth_threshold >= z, image mask == 0, camera mask == 0, grey value <=
 *     maximum_valid_intensity.  Each observation samples `rgb` (width x height pixels of 3 bytes R, G, B: cv::imread(IMREAD_COLOR) of
 *     the image file at the file's own size) bilinearly (InterpolateBilinearVec3, interpolate_bilinear.h:117-146) at
 *     image_x/y_at_scale(min_image_scale) (point_observation.h:84-93); a sample with x < 0, y < 0, (int)x >= width - 1 or
 *     (int)y >= height - 1 is dropped, any other adds its f32 colour to the point's sums and 1 to its count.
 *   e3d_reg_scan_colors_get/set_sums: the accumulators (sums: 3 floats r g b per scan point, counts: one int, input order).  With
 *     image sharding every rank accumulates its own images; the caller adds the vectors (f32 sums, in rank order) and installs the
 *     totals on one rank with set_sums before finish.  f32 addition is not associative: a channel may then differ by one level from
 *     the single-GPU result, whose sums grow image by image.
 *   e3d_reg_scan_colors_finish: rgb[3 i + c] = (uint8)(sum / count + 0.5f), 0 0 0 for a point no image coloured (problem.cc:687-697).
 * Errors (negative return, e3d_last_error): null handle or pixels, unknown image, an image of another rank, width or height < 2, no
 * scan points set, add_image / get_sums / finish without begin (set_sums counts as begin).  No scan points (n = 0) is not an error. */
int e3d_reg_scan_colors_begin(e3d_reg_t* reg);
int e3d_reg_scan_colors_add_image(e3d_reg_t* reg, int image_id, const uint8_t* rgb, int width, int height);
int e3d_reg_scan_colors_get_sums(e3d_reg_t* reg, float* sums, int32_t* counts);
int e3d_reg_scan_colors_set_sums(e3d_reg_t* reg, const float* sums, const int32_t* counts);
int e3d_reg_scan_colors_finish(e3d_reg_t* reg, uint8_t* rgb);
/* DatasetInspector "Label transfer" (src/dataset_inspector/gui_main_window.cc:476-559, the work in TransferLabels, :868-1054): a mask
 * drawn in one image carried to other images through the scan points of e3d_reg_set_scan_points.  Both images are taken at their
 * highest available resolution (intrinsics.model(0), mask_[0], occlusion depth at intrinsics.min_image_scale).  A point is visible
 * in an image if z > 0, pxy = NormalizedToImage(x / z, y / z) has pxy.x + 0.5f >= 0 and pxy.y + 0.5f >= 0, the pixel
 * ((int)(pxy.x + 0.5f), (int)(pxy.y + 0.5f)) lies inside the image and occlusion(iy, ix) + occlusion_depth_threshold >= z.
 *   e3d_reg_mask_transfer_source, the source half: occlusion depth of the source image, then per scan point the label it carries:
 *     the source mask's value v at its pixel if the point is visible there, v != 0 and -- when transfer_eval_obs is 0 -- v != 2
 *     (opt::MaskType::kEvalObs), else 0 (:906-926).  source_mask: width x height bytes of the source camera's level 0, values
 *     0 / 1 / 2 only; host or device.  Returns the number of labelled points.  The labels stay on the device until the next source
 *     call or e3d_reg_set_scan_points.
 *   e3d_reg_mask_transfer_target, the target half, any number of times after one source call:
 *     point pass (:931-951) on a blank mask: every labelled point visible in the target writes its label to its target pixel in
 *       cloud order, so per pixel the labelled point with the HIGHEST index decides;
 *     fill-in (:957-1032): per pixel the numbers of kObs (1) and kEvalObs (2) pixels of the point pass in the 5 x 5 window around it,
 *       clipped at the image borders; kObs count >= 3 -> kObs, then, with transfer_eval_obs, kEvalObs count >= 3 -> kEvalObs.  (So a
 *       pixel the point pass set to kEvalObs becomes kObs when its window holds >= 3 kObs but fewer than 3 kEvalObs pixels: the
 *       reference's behaviour, kept.)  The counts are taken before any pixel is filled.
 *     merge (:1034-1047): mask_out = existing_mask with the new value written wherever it is not 0 and the existing value is not
 *       kEvalObs; without existing_mask the new mask itself.
 *     existing_mask (optional, the target's current level-0 mask) and mask_out (required) are width x height bytes of the TARGET
 *     camera's level 0; host or device.  stats (optional, 3 x int64): pixels set by the point pass, non-zero pixels after the
 *     fill-in, pixels of mask_out that differ from existing_mask (from 0 without one).  The masks the handle holds for the image
 *     (e3d_reg_set_image) are neither read nor changed.
 * Source and target may be the same image and may have different cameras.  Poses, cameras, occlusion geometry, the occlusion depth
 * threshold and the min / max occlusion depths are used as e3d_reg_count_scan_observations uses them.
 * Errors (negative return, e3d_last_error): null handle, source_mask or mask_out; no scan points set; target before source; unknown
 * image (E3D_ERR_INDEX); an image of another rank; a mask value other than 0 / 1 / 2 in either mask (a source call that fails leaves
 * no labels).  No scan points (n = 0) is not an error: 0 labels, mask_out = existing_mask or zeros. */
int64_t e3d_reg_mask_transfer_source(e3d_reg_t* reg, int source_image_id, const uint8_t* source_mask, int transfer_eval_obs);
int e3d_reg_mask_transfer_target(e3d_reg_t* reg, int target_image_id, const uint8_t* existing_mask, uint8_t* mask_out, int64_t* stats);
/* DatasetInspector pose repair, "Localize image" (src/dataset_inspector/localize_image_tool.cc): the user clicks a rendered scan point,
 * then the pixel it belongs at; from >= 6 such pairs the image's pose is refined on bearing vectors.  Four calls; the first three use
 * the image's level-0 model, its current pose and -- for visibility -- exactly the test, the occlusion geometry and the occlusion
 * depth of e3d_reg_mask_transfer_source.  Pixel coordinates: (0, 0) is the centre of the top-left pixel.
 *   e3d_reg_pick_scan_points: mousePressEvent (:96-110) over the scan points ImageWidget::UpdateScanPoints keeps
 *     (gui_image_widget.cc:521-556), for n_clicks = 1 .. E3D_LOCALIZE_MAX_CLICKS clicks (clicks_xy: x y per click) in one pass over
 *     the points of e3d_reg_set_scan_points.  Per click the visible point with the smallest d = fl(fl(dx * dx) + fl(dy * dy)),
 *     dx = pxy.x - click.x, dy = pxy.y - click.y in f32 without contraction, pxy the point's unrounded position.  The reference's
 *     comparison is a strict < from +inf: of equal distances the lowest index wins, a NaN or infinite d never wins (so a NaN click
 *     finds nothing).  index_out[c]: the index in e3d_reg_set_scan_points order or -1; pixel_out (optional, 2 floats per click): the
 *     winner's pxy, NaN NaN without one; distance_out (optional): d, +inf without a winner.  Returns the number of visible points.
 *     Fewer than 2^32 - 1 scan points.  n = 0 scan points is not an error: every index is -1.
 *   e3d_reg_image_bearings: the bearing of n pixel positions (:58-61): the model's ImageToNormalized -- through the undistortion
 *     lookup with bilinear interpolation (camera_base_impl.h:188-211; the four lattice entries around each position are computed,
 *     no table is built), except for the models with their own (PINHOLE, SIMPLE_PINHOLE: linear; FOV: closed form) -- then
 *     (nx, ny, 1) as doubles divided by their norm: 3 doubles per position, host memory.
 *   e3d_reg_project_points: for n global points (xyz packed) the unrounded pixel position (NaN NaN behind the camera) and a state:
 *     0 = behind the camera or outside the image, 1 = visible, 2 = inside the image but behind the occlusion depth.
 *   e3d_pose_from_bearings: HOST ONLY (needs no device).  With d_i = (R p_i + t) / |R p_i + t| it minimises sum |f_i - d_i|^2 over the
 *     pose image_T_global = (R, t) (conventions of e3d_reg_set_image_pose) by Levenberg-Marquardt in f64 from (q_in, t_in): update
 *     (R, t) <- (exp(w) R, exp(w) t + v), analytic Jacobians, at most 100 iterations, stops when the step (w, v) is shorter than
 *     1e-12.  points: n global points, bearings: n unit vectors in the camera frame, 3 doubles each.  q_out (unit, w >= 0) and
 *     t_out are the result rounded to f32.  stats (optional): RMS angle between f_i and d_i before, after, iterations, 1 if it
 *     stopped on the step length.  Refused: n < 6 (:138-141), a non-finite input, a normal matrix whose LDLT fails (all points on
 *     one line, for instance).
 * Errors of the first three as for the label transfer: null handle or outputs, n_clicks outside its range, unknown image
 * (E3D_ERR_INDEX), an image of another rank, no scan points set (pick only). */
#define E3D_LOCALIZE_MAX_CLICKS 32
int64_t e3d_reg_pick_scan_points(e3d_reg_t* reg, int image_id, const float* clicks_xy, int n_clicks, int64_t* index_out, float* pixel_out,
                                 float* distance_out);
int e3d_reg_image_bearings(e3d_reg_t* reg, int image_id, const float* pixels_xy, int n, double* bearings_out);
int e3d_reg_project_points(e3d_reg_t* reg, int image_id, const float* xyz, size_t n, float* pixel_out, uint8_t* state_out);
int e3d_pose_from_bearings(const double* points, const double* bearings, int n, const float q_in[4], const float t_in[3], float q_out[4],
                           float t_out[3], double stats[4]);
/* ImageUndistorter: PINHOLE copies of the images, masks and depth maps of a camera of any model.  The reference leaves this step to
 * COLMAP's undistorter (its README); both rules below are this library's own and restate neither.  They need e3d_reg_set_intrinsics
 * only: no image, no pose.  Pixel coordinates: (0, 0) is the centre of the top-left pixel, here and in the plan.
 *   e3d_reg_undistort_plan: the output camera.  The level-0 model (W x H, focal lengths fx, fy; fx = fy = f for the models with one
 *     focal length) is sampled at its border pixel centres (0, y), (W - 1, y) of every row and (x, 0), (x, H - 1) of every column;
 *     each goes through the model's ImageToNormalized in f32 on the device, exactly as e3d_reg_image_bearings evaluates it before
 *     normalising (camera_base_impl.h:188-211).  Per side the inner and the outer extent of the samples: left L_in = max, L_out = min
 *     of their nx; right R_in = min, R_out = max of nx; top and bottom likewise with ny.  In f64, b = blank_pixels in [0, 1]:
 *     nL = b * L_out + (1 - b) * L_in, likewise nR, nT, nB.  s = 1, or, if max_image_size > 0 and
 *     e + 1 + 2 b exceeds it, e = max(fx * (nR - nL), fy * (nB - nT)): s = (max_image_size - 1 - 2 b) / e.  fx' = (float)(s * fx),
 *     fy' = (float)(s * fy).  Inner bounds are rounded inwards, outer bounds outwards, and the two blended as integers:
 *     x0 = ceil(b * floor(fx' * L_out) + (1 - b) * ceil(fx' * L_in)), x1 = floor(b * ceil(fx' * R_out) + (1 - b) * floor(fx' * R_in)),
 *     width = x1 - x0 + 1, cx' = -x0; the same in y.  The principal point is integral: the output lattice is the undistorted lattice
 *     cropped to a part every pixel of which has data (b = 0) or padded to hold every source pixel centre (b = 1), and without
 *     max_image_size the focal length is kept; max(width, height) <= max_image_size.  Samples without a finite position (beyond a
 *     model's radius cut-off) are skipped at b = 0.
 *     Refused (E3D_ERR_INVALID, the message names the cause): such a sample at b > 0; a side without any finite sample; nL >= nR or
 *     nT >= nB; width or height < 2 or beyond 2^24; a max_image_size that leaves s <= 0; blank_pixels outside [0, 1]; a null
 *     handle or output; unknown intrinsics (E3D_ERR_INDEX).
 *   e3d_reg_undistort: one image through the plan.  For the output pixel (x, y): nx = (float(x) - cx') / fx', ny = (float(y) - cy')
 *     / fy', (sx, sy) = the level-0 model's NormalizedToImage(nx, ny) (camera_base_impl.h:155-164; +-inf past a cut-off), all f32
 *     without contraction.  The pixel is valid iff sx and sy are finite, 0 <= sx <= W - 1 and 0 <= sy <= H - 1 -- a closed interval,
 *     where InterpolateBilinear's test is half open (interpolate_bilinear.h:79-92): the plan's inner extents map to exactly these
 *     borders.  For a valid pixel ix = min((int)sx, W - 2), iy = min((int)sy, H - 2), ax = sx - ix, ay = sy - iy and by kind
 *       0 (u8) and 1 (u8 x 3, interleaved R G B, per channel): v = (1 - ay) * ((1 - ax) * p00 + ax * p10) + ay * ((1 - ax) * p01 +
 *         ax * p11) in f32, InterpolateBilinearNoCheck's order (interpolate_bilinear.h:37-50); the output is (uint8)(int)(v + 0.5f);
 *       2 (u8 mask): the bit-OR of the four pixels; the values are the flags kObs = 1, kEvalObs = 2 of image.h:43-47, so a masked
 *         pixel that contributes masks the result;
 *       3 (f32, nearest): the value at (min((int)(sx + 0.5f), W - 1), min((int)(sy + 0.5f), H - 1)) copied as bits: NaN, +-inf and the
 *         0 of a hole survive unchanged (depth maps hold z-depth, which is constant along a ray).
 *     An invalid pixel is 0 (kinds 0, 1, 3) or 3 (kind 2: both flags, there is no data).  src: W x H pixels of the kind, dst:
 *     width x height pixels of the kind, valid_out (optional): width x height bytes, 1 = valid; host or device memory.  One output
 *     pixel per thread and no sums: the result equals a serial loop bit for bit.
 *     Refused: null handle, plan, src or dst; a kind outside 0..3; a plan with a size < 1 or a non-finite or non-positive focal
 *     length; unknown intrinsics (E3D_ERR_INDEX).
 *   e3d_reg_undistort_kernel_ms: HIP-event time of the resampling kernel of the last e3d_reg_undistort (tools/bench_undistort.py). */
typedef struct { int32_t width, height; float fx, fy, cx, cy; } e3d_undistort_plan;   /* a PINHOLE camera, pixel-centre convention */
int e3d_reg_undistort_plan(e3d_reg_t* reg, int intrinsics_id, double blank_pixels, int max_image_size, e3d_undistort_plan* out);
int e3d_reg_undistort(e3d_reg_t* reg, int intrinsics_id, const e3d_undistort_plan* plan, int kind, const void* src, void* dst,
                      uint8_t* valid_out);
int e3d_reg_undistort_kernel_ms(e3d_reg_t* reg, float* ms);
/* StereoPairCreator: rectified two-view sets (the third ETH3D product): a rectified image pair of two cameras of a rig, the disparity
 * ground truth of the left image and the mask that tells pixels seen by both cameras from half-occluded ones.  The three rules are
 * this library's own.  Pixel coordinates: (0, 0) is the centre of the top-left pixel; lengths are in the unit of the scans.
 *   e3d_reg_stereo_plan: the common PINHOLE camera and the two poses.  Inputs: image_T_global = (q_i, t_i) of the two images as
 *     e3d_reg_get_image_pose reports them (i = 0: left, 1: right) and their level-0 models.  All f64 from the f32 state, every
 *     expression evaluated left to right as written:
 *     1. n = sqrt(w w + x x + y y + z z), q / n; R_i = the quaternion's matrix (Eigen's toRotationMatrix order: tx = 2 x, twx = tx w,
 *        ..., R00 = 1 - (tyy + tzz), R01 = txy - twz, ...).  C_i[k] = -(R_i[0][k] t0 + R_i[1][k] t1 + R_i[2][k] t2).  b = C_1 - C_0,
 *        B = sqrt(bx bx + by by + bz bz), ex = b / B.
 *     2. zs = row2(R_0) + row2(R_1).  c = zs x ex (c.x = zs.y ex.z - zs.z ex.y, ...), ey = c / |c|, ez = ex x ey.  Rr = rows ex, ey, ez.
 *     3. S_i[r][k] = R_i[r][0] Rr[k][0] + R_i[r][1] Rr[k][1] + R_i[r][2] Rr[k][2] (= R_i Rr^T), rounded to f32.
 *     4. q_rect = the quaternion of Rr (Shepperd's four branches on the trace and the largest diagonal entry, as
 *        e3d_pose_from_bearings converts its result), divided by its norm, w >= 0, rounded to f32.
 *     5. t_left[k] = -(Rr[k][0] C_0.x + Rr[k][1] C_0.y + Rr[k][2] C_0.z); t_right = t_left - (B, 0, 0); both rounded to f32, so their
 *        y and z components have equal bits.  baseline = (float)B.
 *     6. f = (float)focal_length if focal_length > 0, else (float)(((fx_0 + fy_0) + (fx_1 + fy_1)) / 4) of the level-0 models.
 *     7. Window: each camera's border samples exactly as e3d_reg_undistort_plan takes them; each (nx, ny) becomes
 *        r = (S[0] nx + S[3] ny + S[6], S[1] nx + S[4] ny + S[7], S[2] nx + S[5] ny + S[8]) with the rounded S_i, and the sample
 *        ((float)(r.x / r.z), (float)(r.y / r.z)); one that is not finite or has r.z <= 0 counts as non-finite.  Per side the samples
 *        of both cameras are united and the rule of e3d_reg_undistort_plan applies unchanged with fx = fy = f.  Both rectified
 *        images share camera.width, .height, .fx = .fy, .cx, .cy; the disparity offset (doffs) is 0.
 *     Refused (E3D_ERR_INVALID) besides what e3d_reg_undistort_plan refuses: B not finite or below 1e-9; |c| < 1e-6 |zs| (the cameras
 *     look along the baseline); ey . (row1(R_0) + row1(R_1)) <= 0 (the pair is given right-then-left and the result would be upside
 *     down: the message says to swap); ez . row2(R_i) <= 0 for either image.  Unlike the undistorter at b = 0, not every output pixel
 *     need be valid: with a rotation the inner extents only approximate the common region, the validity maps below are authoritative.
 *   e3d_reg_stereo_rectify: one image through the plan's camera (`target`) and its S.  For the output pixel (x, y), f32 without
 *     contraction: nx = (float(x) - cx') / fx', ny = (float(y) - cy') / fy'; vx = (S[0] nx + S[1] ny) + S[2], vy = (S[3] nx + S[4] ny)
 *     + S[5], vz = (S[6] nx + S[7] ny) + S[8], each product and sum rounded.  The pixel is invalid if !(vz > 0); otherwise (sx, sy) =
 *     the level-0 model's NormalizedToImage(vx / vz, vy / vz) and everything from there is e3d_reg_undistort: the closed validity
 *     interval, the kinds 0..3, the values 0 / 3 of invalid pixels, the refusals, plus a non-finite entry of S.  With S the identity
 *     the result equals e3d_reg_undistort on the same target bit for bit.
 *   e3d_reg_stereo_kernel_ms: HIP-event time of the resampling kernel of the last e3d_reg_stereo_rectify (tools/bench_stereo.py).
 *   e3d_reg_stereo_ground_truth: the caller registers the rectified cameras -- one PINHOLE intrinsics [f f cx cy] of the plan's size
 *     (min_image_scale 0, one level), two images without pixels (e3d_reg_set_image(id, intr, NULL, NULL)) with the poses (q_rect, t_left)
 *     and (q_rect, t_right) -- and sets the scan points and the occlusion geometry as for e3d_reg_ground_truth_depth.  The entry sets
 *     the scan observation counters to zero, runs the visibility test of e3d_reg_count_scan_observations for both images (a pixel of
 *     left_excluded / right_excluded that is non-zero excludes, NULL = none; width x height bytes), each image's occlusion depth
 *     rendered once, and renders D1 = the depth of the nearest point visible in the left image and D2 = that of the nearest point
 *     visible in both (e3d_reg_ground_truth_depth with min_count 1 and 2).  Per pixel of the left image:
 *       disparity = (float)((double)f * B / (double)D1) with B = (double)t_left.x - (double)t_right.x where D1 is finite, else +inf
 *         (the Middlebury convention for "unknown");
 *       nocc_mask = 255 where D1 is finite and the bits of D2 equal those of D1, 128 where D1 is finite and they differ (the nearest
 *         point is hidden from the right image: half-occluded), 0 where D1 is +inf;
 *       depth (optional) = D1.
 *     The counters are left holding the counts over these two images (e3d_reg_get_scan_observation_counts).
 *     Refused (E3D_ERR_INVALID): images that do not share one PINHOLE intrinsics with fx == fy; quaternions whose bits differ; t.y or
 *     t.z whose bits differ; B <= 0; no scan points set; a null handle, disparity or nocc_mask. */
typedef struct {
  e3d_undistort_plan camera;          /* the common PINHOLE of both rectified images, fx == fy, pixel-centre convention */
  float baseline;                     /* B > 0, scan units */
  float q_rect[4];                    /* rotation of rect_T_global, {w,x,y,z}, w >= 0, the same for both images */
  float t_left[3], t_right[3];        /* translations of the two rectified image_T_global poses */
  float S_left[9], S_right[9];        /* source_T_rect rotations, row-major: ray in the rectified frame -> ray in the source camera frame */
} e3d_stereo_plan;
int e3d_reg_stereo_plan(e3d_reg_t* reg, int left_image_id, int right_image_id, double blank_pixels, int max_image_size,
                        double focal_length /* <= 0: derive */, e3d_stereo_plan* out);
int e3d_reg_stereo_rectify(e3d_reg_t* reg, int intrinsics_id, const e3d_undistort_plan* target, const float S[9], int kind,
                           const void* src, void* dst, uint8_t* valid_out);
int e3d_reg_stereo_kernel_ms(e3d_reg_t* reg, float* ms);
int e3d_reg_stereo_ground_truth(e3d_reg_t* reg, int left_rect_image_id, int right_rect_image_id, const uint8_t* left_excluded,
                                const uint8_t* right_excluded, float* disparity, uint8_t* nocc_mask, float* depth /* optional */);
/* Observations cache (src/opt/observations_cache.{h,cc}; Optimizer::set_cache_observations, optimizer.h).  When enabled, the
 * observation update re-projects a fixed per-image list of point indices with the current state and applies only the
 * scale-fit and border tests (VisibilityEstimator::AppendObservationsForIndexedPointsVisibleInImage,
 * visibility_estimator.cc:140-168, :367-403) -- no occlusion rendering, masks or over-saturation test.
 *   e3d_reg_determine_observed_indices: ObservationsCache::DetermineAndSaveObservedPointIndices (observations_cache.cc:
 *     104-125) minus the files -- a full visibility pass at image scale 0 with the current state fills the lists (of the
 *     images this rank owns).  e3d_reg_run_on_current_scale calls it by itself when caching is on and lists are missing.
 *   e3d_reg_get_observed_indices: returns the length of the list of (image, point scale) and, if `indices` is not NULL,
 *     copies it out as the std::size_t values the `.observed_indices` files hold (observations_cache.cc:146-156).
 *   e3d_reg_set_observed_indices: installs a list read from such a file (observations_cache.cc:70-102). */
int e3d_reg_set_cache_observations(e3d_reg_t* reg, int enabled);
int e3d_reg_determine_observed_indices(e3d_reg_t* reg);
int64_t e3d_reg_get_observed_indices(e3d_reg_t* reg, int image_id, int point_scale, uint64_t* indices);
int e3d_reg_set_observed_indices(e3d_reg_t* reg, int image_id, int point_scale, const uint64_t* indices, size_t count);
/* ColorOptimizer::Apply (color_optimizer.cc:40-123) */
int e3d_reg_color_update(e3d_reg_t* reg);
/* CostCalculator::ComputeCost (cost_calculator.cc:44-100) */
int e3d_reg_compute_cost(e3d_reg_t* reg, double* cost);
/* IntrinsicsAndPoseOptimizer::Apply (intrinsics_and_pose_optimizer.cc:48-259): one LM step with <= 10 tries */
int e3d_reg_apply(e3d_reg_t* reg, int print_progress, int* applied_update, float* lambda, float* max_change);
/* bool Optimizer::RunOnCurrentScale(max_num_iterations, max_change_convergence_threshold,
 *   iterations_without_new_optimum_threshold, <observations_cache_path: host side>, print_progress, &optimum_cost); returns 1 if
 * converged, 0 if not.  The state (intrinsics, poses) is left at the optimum, like the reference. */
int e3d_reg_run_on_current_scale(e3d_reg_t* reg, int max_num_iterations, float max_change_convergence_threshold,
                                 int iterations_without_new_optimum_threshold, int print_progress, double* optimum_cost,
                                 int* iterations_done);

/* Problem::DeterminePointNeighbors (src/opt/problem.cc:706-786): neighbor_indices[p * neighbor_count + j] = the j-th of the
 * shuffled (candidate_count + 1)-nearest-neighbour candidates of point p (the point itself excluded), searched within p's
 * own scan when limit_to_same_scan != 0 (fixed scan colours).  Same libstdc++ std::shuffle / std::mt19937(0) stream as the
 * reference. */
int e3d_determine_point_neighbors(const float* xyz, size_t n, const uint8_t* scan_indices, int scan_count,
                                  int limit_to_same_scan, int neighbor_count, int candidate_count,
                                  uint32_t* neighbor_indices);

/* ComputeMinMaxPointRadius over all images (src/opt/multi_scale_point_cloud.cc:126-180,236-262): for every point the smallest
 * radius that projects to half a pixel in some image (min_radius, +inf if never observed) and the largest such radius
 * divided by the minimum scaling factor 2^-(image_scale_count - 1) (max_radius, -inf if never observed).  Uses the images,
 * intrinsics, splat points and parameters already set on the handle (current_image_scale = 0 at set-up time). */
int e3d_reg_point_radius_minmax(e3d_reg_t* reg, const float* xyz, size_t n, float* min_radius, float* max_radius);

/* MergeClosePoints (src/opt/multi_scale_point_cloud.cc:44-124): greedy merge in point order -- every point not yet absorbed
 * becomes a centre and absorbs all points strictly within merge_distance -- computed in parallel (the centres are the
 * lexicographically first maximal independent set).  Outputs (capacity n each) in centre order: mean position, mean colour of
 * the scan with most merged points, that scan's index, maximum of max_radius.  Returns the number of output points.
 * The inputs are host arrays.  Refused with E3D_ERR_INVALID before anything runs on the device: a point with a NaN or infinite
 * coordinate, and a scan index >= num_scans (the reference defines neither; 1 <= num_scans <= 16, merge_distance finite and > 0). */
int64_t e3d_merge_close_points(float merge_distance, int num_scans, const float* xyz, const float* colors,
                               const uint8_t* scan_indices, const float* max_radius, size_t n, float* out_xyz,
                               float* out_colors, uint8_t* out_scan_indices, float* out_max_radius);

/* Multi-GPU (one process per GPU): images are sharded, image `id` belongs to rank `id mod world_size`
 * (e3d_reg_image_owner).  Every rank declares every intrinsics block, point scale and image (ids and poses) so that the
 * variable layout is global, but only the owner of an image uploads its pyramid -- e3d_reg_set_image accepts
 * level_pixels == NULL for images of other ranks -- and only the owner creates observations and residuals for it.
 * Exchange steps: the dense H, b and the residual sums / counts once per Apply and 4 doubles per LM try and
 * per cost evaluation (`allreduce`, HOST f64 buffer); the variable descriptors (K*N f32) and observation counts (N i32)
 * of every point scale once per colour update (`allreduce_device`: DEVICE buffer, dtype 0 = f32, 1 = i32, in-place sum;
 * the library has synchronised its stream before the call and the callback must return with the result complete).
 * Both callbacks must leave the identical result on every rank; all ranks then take the same LM decisions. */
typedef int (*e3d_allreduce_device_fn)(void* device_buffer, size_t count, int dtype, void* user);
int e3d_reg_set_shard(e3d_reg_t* reg, int rank, int world_size, e3d_allreduce_fn allreduce,
                      e3d_allreduce_device_fn allreduce_device, void* user);
/* The same sharding with the library's own RCCL communicator (see e3d_comm_create): the block-sparse normal equations, the
 * residual sums and the variable descriptors are all-reduced on the handle's stream; call before the images are set. */
int e3d_reg_set_comm(e3d_reg_t* reg, e3d_comm_t* comm);
int e3d_reg_image_owner(e3d_reg_t* reg, int image_id);

/* ---- PointCloudEditor (src/point_cloud_editor): selections and edits of one object's points --------------------------
 * The GUI's lasso, beyond-plane selection, point picking, "delete" and "move" as batch operations.  An edit handle keeps one
 * object's coordinates and its selection on the device for the whole session; a selection call is one pass over the points
 * and one synchronisation (for the count it returns).  Colours, labels and faces stay with the caller, who compacts them with
 * the flags fetched before a delete.
 *
 * Selection.  One byte per point, 0 or 1.  The reference keeps a list of indices (Scene::selected_point_indices), but every
 * path leaves that list in ascending index order -- replace and beyond-plane push indices in point order, add sorts and
 * removes duplicates, remove keeps the order -- so flags hold the same information, and "delete" / "move" / "label" visit the
 * points in the same order.
 *
 * e3d_view: the GUI's view.  A pinhole camera (RenderWidget::SetFreeOrbitViewport makes fx = fy = height, cx = width / 2 - 0.5,
 * cy = height / 2 - 0.5), camera_T_object as the row-major 3 x 4 [R * s | t] of the reference's Sim3 camera_RsT_object, and the
 * depth range of the Near / Far sliders.  Per point, in f32 and in this order:
 *     camera_point = ((r0 * x + r1 * y) + r2 * z) + t          (per row; Eigen's order, no contraction)
 *     in range     = min_depth <= camera_point.z <= max_depth   (both ends inclusive; NaN is out of range)
 *     pixel        = (fx * (camera_point.x / camera_point.z) + cx) + 0.5f, and the same in y */
typedef struct e3d_edit e3d_edit_t;
typedef struct e3d_view {
  int32_t width, height;
  float   fx, fy, cx, cy;
  float   camera_T_object[12];
  float   min_depth, max_depth;
} e3d_view;
#define E3D_EDIT_REPLACE 0
#define E3D_EDIT_ADD     1
#define E3D_EDIT_REMOVE  2
#define E3D_EDIT_MAX_POLYGON 1024
#define E3D_EDIT_MAX_CLICKS  8

/* Uploads n points (n x 3 f32, host or device; n < 2^32, n == 0 is legal here and in every call below) with an empty
 * selection; NULL on failure. */
e3d_edit_t* e3d_edit_create(const float* xyz, size_t n);
void e3d_edit_destroy(e3d_edit_t* edit);
int64_t e3d_edit_size(e3d_edit_t* edit);                          /* the current number of points */
int e3d_edit_get_points(e3d_edit_t* edit, float* xyz);            /* their coordinates, in order */
/* The selection: n bytes out (0 / 1), n bytes in (any non-zero byte selects; returns the number selected), the number selected
 * (kept on the host: no device work). */
int e3d_edit_get_selection(e3d_edit_t* edit, uint8_t* flags);
int64_t e3d_edit_set_selection(e3d_edit_t* edit, const uint8_t* flags);
int64_t e3d_edit_selection_count(e3d_edit_t* edit);

/* LassoSelectionTool::applySelection (tool_select_lasso.cc:104-230).  polygon_xy: n_vertices x 2 doubles in pixels, not closed
 * (the library repeats the first vertex).  mode: E3D_EDIT_REPLACE / _ADD / _REMOVE.  A point in range whose pixel is inside the
 * polygon is selected (added, removed).  Inside = odd-even rule over the closed polygon's edges in f64, the f32 pixel promoted:
 * an edge with y1 == y2 is skipped; otherwise it is ordered so that y1 < y2 and counts if
 *     y >= y1 && y < y2 && x1 + ((x2 - x1) / (y2 - y1)) * (y - y1) <= x.
 * This is QPolygonF::containsPoint(..., Qt::OddEvenFill) with its qFuzzyCompare(y1, y2) replaced by exact equality.  For the
 * polygons the GUI makes the two are the same test: mouse positions are integers, so |y1 - y2| >= 1 wherever y1 != y2, and with
 * |y| < 10^12 Qt's fuzzy comparison (|y1 - y2| * 10^12 <= min(|y1|, |y2|)) is then false.
 * Fewer than 3 vertices: nothing happens (:105) and the selection stays.  More than E3D_EDIT_MAX_POLYGON: an error.
 * depth (optional; width x height f32, row-major, host or device): the visibility test of mesh vertices (:177-190).  The pixel
 * is truncated to int (saturating), then clamped to the image; a vertex is not selected if the depth there is finite and
 * < 0.99f * camera_point.z.  +-inf and NaN let it pass.
 * Returns the number of selected points after the call. */
int64_t e3d_edit_lasso(e3d_edit_t* edit, const e3d_view* view, const double* polygon_xy, int n_vertices, int mode,
                       const float* depth);

/* BeyondPlaneSelectionTool::PerformSelection (tool_select_beyond_plane.cc:43-102); always replaces the selection.  points: p0,
 * p1, p2.  The plane as Eigen::Hyperplane<float, 3>::Through makes it, in f32: n = (p2 - p0) x (p1 - p0), divided by its norm,
 * offset = -p0 . n; all four coefficients negated if the signed distance of camera_position_object is negative.  A point is
 * selected if ((n.x * x + n.y * y) + n.z * z) + offset < 0 (a point on the plane and NaN are not), and with limit_to_visible
 * only if it is also in range and 0 <= pixel.x < width, 0 <= pixel.y < height.
 * Difference: where |n| <= |p2 - p0| * |p1 - p0| * FLT_EPSILON (three points on a line) Eigen fits a plane by SVD; here that is
 * an error.  Returns the number of selected points. */
int64_t e3d_edit_beyond_plane(e3d_edit_t* edit, const e3d_view* view, const float points[9],
                              const float camera_position_object[3], int limit_to_visible);

/* BeyondPlaneSelectionTool::mousePressEvent (:108-155) for up to E3D_EDIT_MAX_CLICKS clicks in one pass: per click (x, y
 * doubles in pixels) the point in range with the smallest (float)(dx * dx + dy * dy), dx and dy in f64 (the f32 pixel promoted).
 * The comparison is the reference's strict `<` starting from +inf: of equal distances the lowest index wins and a NaN or
 * infinite distance never does.  index_out[c] = -1 (and distance_out[c] = +inf) if no point qualifies.  distance_out may be
 * NULL. */
int e3d_edit_pick(e3d_edit_t* edit, const e3d_view* view, const double* clicks_xy, int n_clicks, int64_t* index_out,
                  float* distance_out);

/* The Delete key (render_widget.cc:570-642): removes the selected points, keeping the order of the others, and clears the
 * selection; returns the new number of points.  The "move" key (:677-732) is e3d_edit_extract_selected -- the selected points'
 * coordinates in index order, capacity in points, returns their number -- followed by e3d_edit_delete_selected. */
int64_t e3d_edit_delete_selected(e3d_edit_t* edit);
int64_t e3d_edit_extract_selected(e3d_edit_t* edit, float* xyz_out, size_t capacity);
/* HIP-event time of the kernels of the last selection, pick, extract or delete call on this handle, in ms. */
int e3d_edit_kernel_ms(e3d_edit_t* edit, float* ms);

/* ---- SurfaceReconstructor: an occlusion mesh from an oriented point cloud ------------------------------------------------
 * The reference sends its user to MeshLab / PoissonRecon for this step (its README, "External Surface Reconstruction": any
 * suited method may be used; the mesh should be strongly subdivided).  This is a uniform-lattice extraction of a signed
 * field, a capability of this library alone; it restates nothing of the reference.  h = voxel size, R = support radius.
 * All arithmetic is f64: points, normals, h and R arrive as f32 and are converted first.  Sums may be formed in any order.
 *
 * Lattice.  Corner (i, j, k) (int32) lies at (h i, h j, h k): the lattice is anchored at the world origin, so the result
 * does not depend on a bounding box.  Cell (i, j, k) is the cube between corners (i, j, k) and (i + 1, j + 1, k + 1).
 * Contributing points.  A point contributes nothing if a component of its position or normal is not finite or if its normal
 * is (0, 0, 0) (NormalEstimator writes NaN normals for degenerate neighbourhoods).
 * Field.  For a corner x and a contributing point p with normal n: d2 = (dx dx + dy dy) + dz dz with (dx, dy, dz) = x - p.
 * The point counts iff d2 < R R (strict).  Its weight is w = (1 - d2 / (R R))^2, S = sum w ((nx dx + ny dy) + nz dz),
 * W = sum w.  A corner is defined iff at least one point counts; then f = S / W, and it is negative iff f < 0 (f == 0 is
 * not).  Scan normals face the scanner: negative = inside the surface.
 * Crossing edge.  The edge from corner a to b = a + e_d (d = 0, 1, 2) crosses iff both corners are defined and exactly one
 * is negative; its crossing point is a + t h e_d with t = f_a / (f_a - f_b).  An edge with an undefined corner never
 * crosses: the mesh ends where the data ends, and no sheet appears behind a wall seen from one side.
 * Vertices.  A cell is active iff one of its 12 edges crosses.  Its vertex is the mean of the crossing points of its crossing
 * edges (summed by axis d, then by the edge's offset along (d + 2) % 3, then along (d + 1) % 3), rounded to f32 at the end.
 * Vertices are in ascending (k, j, i) of their cell.
 * Triangles.  Each crossing edge (a, d) gives one quad over the four cells that contain it: with u = (d + 1) % 3 and
 * v = (d + 2) % 3 the cells a + (-1, -1), a + (0, -1), a + (0, 0), a + (-1, 0) in (u, v) are q0..q3, counter-clockwise seen
 * from +e_d.  If a is not negative the four are taken in reverse (q3, q2, q1, q0 become q0..q3), so face normals point from
 * negative to positive.  The triangles are (q0, q1, q2) and (q0, q2, q3).  Quads are in ascending (k, j, i) of a, then d.
 * Refused (NULL; E3D_ERR_INVALID's message in e3d_last_error): h or R not finite or <= 0; R / h > 8; a contributing point
 * with |coordinate| / h >= 2^20 (the 21-bit cell key of the grid); contributing points whose voxels span more than
 * 2^21 - 36 along one axis (both ends of that range at once); n >= 2^31.  n == 0 or no contributing point: an empty mesh.
 * xyz, normals: n x 3 f32, host or device.  The result is a host-side handle; the call returns after all device work. */
typedef struct e3d_surface e3d_surface_t;
e3d_surface_t* e3d_surface_reconstruct(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius);
void e3d_surface_destroy(e3d_surface_t* surface);
/* The numbers of defined corners, vertices and triangles (each pointer may be NULL). */
int e3d_surface_counts(e3d_surface_t* surface, int64_t* n_corners, int64_t* n_vertices, int64_t* n_triangles);
/* The defined corners in ascending (k, j, i): lattice coordinates ijk[3 c], f[c], W[c] and the number of points that count
 * [c], so that a field error can be told from an extraction error.  Each pointer may be NULL. */
int e3d_surface_get_corners(e3d_surface_t* surface, int32_t* ijk, double* f, double* weight, int32_t* count);
/* The mesh: vertices[3 v] f32, the vertices' cells cell_ijk[3 v] (may be NULL), triangles[3 t] as vertex indices. */
int e3d_surface_get_mesh(e3d_surface_t* surface, float* vertices, int32_t* cell_ijk, uint32_t* triangles);
/* HIP-event times of the call's kernel groups in ms and their names (static strings), at most capacity of each (either
 * array may be NULL); returns the number of groups: grid, candidates, field, corners, extract, and for a handle made with
 * n_ops > 0 a sixth, solids; for one made with fill_iterations > 0 one more, fill, last. */
int e3d_surface_kernel_ms(e3d_surface_t* surface, float* ms, const char** names, int capacity);

/* ---- SurfaceReconstructor: box union and subtraction (the reference's CSG tool, src/point_cloud_editor/tool_csg.cc) --------
 * Scanners miss glass, dark or shiny objects and what no scan position sees; the reference's editor places a subdivided box by
 * hand and unites it with or subtracts it from the surface mesh through a mesh boolean.  Here the box is an analytic signed
 * function on the lattice and is combined with the scan field BEFORE the extraction above, which stays as it is.  All
 * arithmetic is f64 with no contraction, in the stated order.  x = (h i, h j, h k) is a lattice corner.
 *
 * A solid is an oriented box with centre c[3], rotation Q[9] (row-major; the columns are the box axes in world coordinates)
 * and half extents a[3].  Its function at x:  d = x - c;  u_m = (Q[0][m] d_0 + Q[1][m] d_1) + Q[2][m] d_2;  q_m = |u_m| - a_m;
 * g = max(max(q_0, q_1), q_2).  g is negative inside, zero on the surface and 1-Lipschitz; no square root, no libm call.
 * An operation list of at most 256 entries (kind, solid) is applied in order to the scan field f = S / W (defined iff a
 * point counts):
 *   union     at a defined corner f <- min(f, g); at an undefined corner with |g| <= 2 h the corner becomes defined with
 *             f = g.  (An edge of length h that crosses g = 0 has |g| < h at both ends: the rest of the band is slack.)
 *   subtract  (A minus B) at a defined corner f <- max(f, -g).  No corner becomes defined: as in the reference, subtracting
 *             from nothing gives nothing.
 * min and max return their first argument on equality.  "Negative iff f < 0", the crossing rule, t = f_a / (f_a - f_b) and the
 * vertex, quad and ordering rules are unchanged.  For a corner defined by solids alone e3d_surface_get_corners reports
 * count = 0 and W = 0; for every other corner count and W are the scan's.
 * Known artefact.  Where a union box touches a wall seen from one side, the band of newly defined positive corners outside
 * the box meets the wall's negative back side: a strip of back sheet at most two cells wide appears behind the wall.
 * Refused (NULL; E3D_ERR_INVALID, the library stays usable): more than 256 operations or an unknown kind; a centre, rotation
 * or extent that is not finite; a half extent <= 0; max |Q^T Q - I| > 1e-9 or det Q < 0; a solid whose band (its world
 * bounding box grown by 2 h, two lattice steps of margin) reaches |coordinate| / h >= 2^20; points and solids (union and
 * subtract alike) that together span more than 2^21 - 36 lattice steps along one axis; solids whose bands cover more than
 * 2^32 - 64 bricks of 4 x 4 x 4 corners, or candidates beyond the per-call limits of e3d_surface_reconstruct.
 * n_ops == 0 is e3d_surface_reconstruct: the same launches, the same bytes, the same five kernel groups.  n == 0 or no
 * contributing point is no early end when there is a union: the result is the mesh of the boxes alone. */
#define E3D_SURFACE_UNION 0
#define E3D_SURFACE_SUBTRACT 1
typedef struct e3d_surface_solid {
  int32_t kind;           /* E3D_SURFACE_UNION or E3D_SURFACE_SUBTRACT */
  double centre[3];
  double rotation[9];
  double half_extent[3];
} e3d_surface_solid_t;
e3d_surface_t* e3d_surface_reconstruct_csg(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius,
                                           const e3d_surface_solid_t* ops, size_t n_ops);

/* ---- SurfaceReconstructor: filling holes on the lattice ----------------------------------------------------------------------
 * The scan field ends where the data ends, and every hole of the mesh lets scan points behind it shine through in the tools that
 * use it as occlusion geometry.  The reference's README asks for a method that "is able to fill in unobserved surfaces such that
 * occlusions by those surfaces are also accounted for"; this is volumetric diffusion of the signed field (Davis et al., "Filling
 * holes in complex surfaces using volumetric diffusion", 2002), restricted to where the surface ends.  N = fill_iterations Jacobi
 * iterations run between the scan field and the operation list above; the scan field, the solids and the extraction are unchanged.
 * All arithmetic is f64, IEEE, with no contraction, in the stated order.
 *
 * State per lattice corner: defined, f, source.  A source is a corner the scan field defines; sources never change.  "Neighbour"
 * means the six face neighbours, always visited in the order -x, +x, -y, +y, -z, +z.  neg(c) means f(c) < 0.
 * Iteration t = 1 .. N reads state t - 1 only:
 *   1. At a crossing.  X(y) holds iff y is defined and has a defined neighbour z with neg(z) != neg(y).
 *   2. Near a crossing.  X1(y) holds iff y is defined and X(y) or X of one of its neighbours holds.
 *   3. Growth.  An undefined corner becomes defined, with source = 0, iff one of its neighbours has X1.  Its value is
 *      s / (double)c, where s starts at +0.0 and adds f of each defined neighbour in neighbour order and c is their number.
 *   4. Smoothing.  A defined non-source corner is replaced by s / (double)c with s and c built as in step 3 and its own f then
 *      added last and counted.
 *   5. Everything else keeps its state.
 * After iteration N the operation list is applied as above, to a field in which filled corners are ordinary defined corners (so
 * an edit script keeps the last word: a subtract box re-opens what the fill closed wrongly).  Then "negative iff f < 0" and the
 * unchanged extraction.  A filled corner reports count = 0 and W = 0, like a corner defined by a solid.  filled: the corners the
 * fill defined.  A vertex is filled iff a crossing edge of its cell has a filled endpoint; a triangle iff one of its vertices is.
 * Why growth is restricted to corners near a crossing.  Plain diffusion thickens every one-sided sheet by N cells and puts a
 * false sheet wherever the back of one surface faces the front of another.  With rule 3 the band follows the zero set, the
 * surface extends tangentially by one cell per iteration, and growth stops by itself once a hole has closed: a closed surface
 * has no rim.  (Growth next to X alone leaves pinholes.)
 * Known behaviour.  At a true outer boundary of the data the sheet is extended by up to N cells.  The extension runs along
 * lattice directions: a wall tilted by a drifts N h tan a off its plane.  Two surfaces that face the same way 6 cells or fewer
 * apart get a false sheet at N = 16 (at 8 cells they do not).  Holes wider than about 2 (N + R / h) cells stay open; once a hole
 * has closed, the smoothing that goes on pulls the patch flat.
 * Refused (NULL; E3D_ERR_INVALID, the library stays usable): fill_iterations < 0 or > 32; with N > 0 the range and span limits
 * of e3d_surface_reconstruct applied to the voxels of the contributing points grown by N + 4 lattice steps on every side (a
 * point within N + 4 voxels of |coordinate| / h = 2^20; a grown box, with the solids, of more than 2^21 - 36 steps along an
 * axis); the per-call item limits applied to the enlarged brick set.  A cloud with no contributing point and N > 0 is no error.
 * fill_iterations == 0 is e3d_surface_reconstruct_csg: the same launches, the same bytes, the same kernel groups.  With N > 0
 * e3d_surface_kernel_ms reports one more group, fill, last (after solids when n_ops > 0, otherwise sixth). */
e3d_surface_t* e3d_surface_reconstruct_filled(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius,
                                              int fill_iterations, const e3d_surface_solid_t* ops, size_t n_ops);
/* Which corners (in the order of e3d_surface_get_corners) and which vertices (in the order of e3d_surface_get_mesh) the fill made:
 * one byte each, 0 or 1; all 0 for a handle made with fill_iterations == 0.  Each pointer may be NULL. */
int e3d_surface_get_fill(e3d_surface_t* surface, uint8_t* corner_filled, uint8_t* vertex_filled);

/* ---- ReconstructionEvaluator: accuracy and completeness of a reconstruction against the scans ----------------------------
 * The ETH3D evaluation scheme the reference's README describes and neither tree computes: a reconstruction point within a
 * tolerance of the scans is accurate, one in the free space between a scanner and what it measured is wrong, everything else
 * is unobserved and not judged.  The rules are this library's; they restate nothing of the reference.
 *
 * Inputs: reconstruction points r (n_rec x 3 f32); S >= 1 scans, scan s with points q (f32, global frame; the scans are
 * concatenated, scan s is rows [scan_offsets[s], scan_offsets[s + 1]) with scan_offsets[0] == 0) and scanner origin o_s
 * (3 f32); T tolerances t_0 < ... < t_{T-1}, 1 <= T <= 8, finite and > 0 (f32); voxel size h > 0; cube-map size N, even,
 * 2 <= N <= 8192.  All arithmetic is f32 with the stated order and no contraction, except where f64 is named.
 *
 * 1. Ignored points.  A point with a non-finite coordinate is ignored: it is neighbour of nothing, lands in no pixel and no
 *    voxel, and its classes are 255.
 * 2. Near class (both directions).  d2(a, b) = ((dx dx) + dy dy) + dz dz with dx = a.x - b.x ... .  thr_i = (float)((double)
 *    t_i t_i).  near(a | B) is the smallest i with min_{b in B} d2(a, b) <= thr_i (inclusive), or T if there is none.
 *    near_scan[q] = near(q | reconstruction), near_rec[r] = near(r | all scans together).  Only the class is public, not the
 *    distance or the partner.
 * 3. Range image of scan s.  For d = p - o_s (componentwise f32): m = max(|dx|, |dy|, |dz|); there is no pixel if m == 0 or
 *    d is not finite.  Axis is the first of x, y, z with |d_axis| == m, face = 2 axis + (d_axis < 0), (a, b) are the other
 *    two components in cyclic order: x -> (y, z), y -> (z, x), z -> (x, y).  col = min(N - 1, (int)floorf((a / m + 1.0f) *
 *    (float)(N / 2))), row the same from b.  range(p) = sqrtf(d2(p, o_s)).  rmin_s[face, row, col] is the minimum of range(q)
 *    over the scan's non-ignored points in that pixel; the pixel is empty without one.
 * 4. Free class.  free_s[r] is the number of i with range(r) + t_i < rmin_s[pixel_s(r)] (f32 addition), 0 if r has no pixel
 *    or the pixel is empty.  The addition is monotone in t, so these i are a prefix of the tolerances.  free[r] = max_s
 *    free_s[r].  Using the pixel's minimum never calls anything behind the nearest return of a pixel free space.
 * 5. Verdict at tolerance i.  r is accurate iff near_rec[r] <= i, otherwise inaccurate iff i < free[r], otherwise unobserved.
 *    q is complete iff near_scan[q] <= i.
 * 6. Voxels.  v = (int)floorf(c / h) per coordinate (f32 division).  Scan voxels are over all scans' non-ignored points
 *    together, reconstruction voxels over the non-ignored r.  A non-ignored point with fabsf(c) / h >= 2^20 is refused, as
 *    in e3d_surface_reconstruct; v + 2^20 is then the 21-bit key field of its axis, so no accepted cloud spans too many
 *    voxels for the key.  Voxels are listed in ascending (k, j, i).
 * 7. Scores, f64.  completeness_i is the mean over the scan voxels of (# complete at i) / (# points); accuracy_i is the mean,
 *    over the reconstruction voxels with acc + inacc > 0 at i (the evaluated voxels), of acc / (acc + inacc); f1_i =
 *    ((2 a) c) / (a + c).  Each of the three is 0 where its denominator is 0.  Per-voxel ratios are single f64 divisions of
 *    integers; the sums are formed on the GPU in a fixed order, so two calls return identical bytes.
 *
 * Refused (NULL; E3D_ERR_INVALID's message in e3d_last_error): S < 1; scan_offsets not starting at 0 or descending; T
 * outside 1 .. 8; a tolerance not finite, <= 0 or not above its predecessor; h not finite or <= 0; N odd or outside
 * 2 .. 8192; a point of rule 6; n_rec or the number of scan points >= 2^31.
 * rec_xyz, scan_xyz: host or device; scan_offsets (S + 1), scan_origins (S x 3), tolerances (T): host.  The result is a
 * host-side handle; the call returns after all device work, and no device memory is kept. */
typedef struct e3d_eval e3d_eval_t;
e3d_eval_t* e3d_evaluate_reconstruction(const float* rec_xyz, size_t n_rec, const float* scan_xyz, const int64_t* scan_offsets,
                                        const float* scan_origins, int n_scans, const float* tolerances, int n_tolerances,
                                        float voxel_size, int cube_map_size);
void e3d_eval_destroy(e3d_eval_t* eval);
/* The numbers of scan voxels and reconstruction voxels and, per tolerance, of evaluated reconstruction voxels
 * (evaluated_voxels[T]).  Each pointer may be NULL. */
int e3d_eval_counts(e3d_eval_t* eval, int64_t* n_scan_voxels, int64_t* n_rec_voxels, int64_t* evaluated_voxels);
/* scores[3 T]: completeness[T], accuracy[T], f1[T]. */
int e3d_eval_get_scores(e3d_eval_t* eval, double* scores);
/* near_rec[n_rec], free[n_rec], near_scan[number of scan points].  Each pointer may be NULL. */
int e3d_eval_get_classes(e3d_eval_t* eval, uint8_t* near_rec, uint8_t* free_class, uint8_t* near_scan);
/* The voxels of one kind (0: scan, 1: reconstruction) in ascending (k, j, i): ijk[3 v], the number of points n_points[v],
 * and per tolerance count_a[T v + i] = # complete (scan) or # accurate (reconstruction) and count_b[T v + i] = # inaccurate
 * (reconstruction; zeros for the scan voxels).  Each pointer may be NULL. */
int e3d_eval_get_voxels(e3d_eval_t* eval, int kind, int32_t* ijk, int32_t* n_points, int32_t* count_a, int32_t* count_b);
/* HIP-event times of the call's kernel groups in ms and their names (static strings), at most capacity of each (either
 * array may be NULL); returns the number of groups: grid, search, range, voxels. */
int e3d_eval_kernel_ms(e3d_eval_t* eval, float* ms, const char** names, int capacity);

/* ---- StereoEvaluator: disparity maps of a stereo method against the two-view ground truth ----------------------------------
 * The counterpart of e3d_evaluate_reconstruction for the two-view sets StereoPairCreator writes (disp0GT.pfm, mask0nocc.png).
 * The rules are this library's; they restate nothing of the reference, which has no such code.
 *
 * Inputs: gt, W x H f32, row-major, top row first (+inf, any non-finite value: unknown); mask, W x H u8, or NULL; n_est >= 1
 * estimates of the same size, contiguous (estimate e is elements [e W H, (e + 1) W H)), f32; T thresholds, 1 <= T <= 8, f32,
 * finite, >= 0, strictly ascending; P percentiles, 0 <= P <= 8, int32, each in 1 .. 100.
 *
 * 1. Regions.  A pixel is known iff gt is finite.  Region 0 ("all") is the known pixels with mask != 0, region 1 ("nocc") the
 *    known pixels with mask == 255; with mask == NULL both are the known pixels.  Any mask value is accepted, only != 0 and
 *    == 255 are read.  Region 1 is a subset of region 0.
 * 2. Valid estimate.  A pixel's estimate e is valid iff it is finite (NaN and +-inf are invalid, following Middlebury's inf);
 *    any finite value is valid, negative ones included.
 * 3. Error.  err = fabsf(e - gt): one f32 subtraction, no contraction; +inf if the subtraction overflows, never NaN.
 * 4. Counts (int64), per estimate and region: n_region, the pixels of the region; n_valid, those with a valid estimate;
 *    n_bad[t], the valid ones with err > thr_t (strict).
 * 5. Sums (f64), per estimate and region, over the region's valid pixels: sum1 of (double)err, sum2 of (double)err *
 *    (double)err (each product exact).  They are formed on the GPU in an order that depends on W, H and n_est alone, so two
 *    calls return identical bytes.
 * 6. Quantiles (f32), per estimate, region and percentile p: with n = n_valid >= 1 and k = (p n + 99) / 100 - 1 in 64-bit
 *    integers (ceil(p n / 100) - 1), element k of the region's valid errors sorted ascending.  Nothing is interpolated: the
 *    result has the bits of one pixel's err.  n == 0 gives NaN.
 * 7. Derived scores (the callers', f64, from the numbers above alone): coverage = n_valid / n_region, bad_t = n_bad[t] /
 *    n_valid, bad_or_missing_t = (n_bad[t] + n_region - n_valid) / n_region, avgerr = sum1 / n_valid, rms = sqrt(sum2 /
 *    n_valid); each is 0 where its denominator is 0.
 * 8. Error map (optional, u8 x 3 per pixel and estimate, R G B).  Outside region 0: (0, 0, 0).  Invalid estimate:
 *    (255, 0, 255).  Otherwise, with c the number of thresholds with err > thr_t, palette[(c * 8) / T] of the nine entries
 *    (49,54,149) (69,117,180) (116,173,209) (171,217,233) (254,224,144) (253,174,97) (244,109,67) (215,48,39) (165,0,38).
 *    A pixel of region 0 outside region 1 (half-occluded) gets each channel >> 1, the invalid colour included.
 *
 * Refused (NULL; E3D_ERR_INVALID's message in e3d_last_error; the library stays usable): W or H < 1; W H >= 2^31; n_est < 1;
 * T outside 1 .. 8, P outside 0 .. 8; a threshold that is not finite, is negative or is not above its predecessor; a
 * percentile outside 1 .. 100; a null gt, estimates or thresholds (or percentiles with P > 0).
 * gt, mask, estimates: host or device; thresholds, percentiles: host; error_maps: host, n_est H W 3 bytes, or NULL.  The
 * ground truth and the mask are read from one copy on the device by all estimates.  The result is a host-side handle; the call
 * returns after all device work (one synchronisation, no read-back between the passes), and no device memory is kept. */
typedef struct e3d_disp_eval e3d_disp_eval_t;
e3d_disp_eval_t* e3d_evaluate_disparity(const float* gt, const uint8_t* mask, int width, int height, const float* estimates,
                                        int n_estimates, const float* thresholds, int n_thresholds, const int32_t* percentiles,
                                        int n_percentiles, uint8_t* error_maps);
void e3d_disp_eval_destroy(e3d_disp_eval_t* eval);
/* counts[n_est][2][2 + T]: per estimate and region n_region, n_valid, n_bad[T]. */
int e3d_disp_eval_get_counts(e3d_disp_eval_t* eval, int64_t* counts);
/* sums[n_est][2][2]: per estimate and region sum1, sum2. */
int e3d_disp_eval_get_sums(e3d_disp_eval_t* eval, double* sums);
/* quantiles[n_est][2][P]. */
int e3d_disp_eval_get_quantiles(e3d_disp_eval_t* eval, float* quantiles);
/* HIP-event times of the call's kernel groups in ms and their names (static strings), at most capacity of each (either
 * array may be NULL); returns the number of groups: classify, select, sums. */
int e3d_disp_eval_kernel_ms(e3d_disp_eval_t* eval, float* ms, const char** names, int capacity);

#ifdef __cplusplus
}
#endif
#endif  /* E3D_HIP_H */
