/*
 * suma_hip.h -- C-ABI of the MI355X (gfx950) projective-ICP + surfel-fusion core.
 *
 * This is the drop-in boundary for the hot path of SuMa++ (PRBonn/semantic_suma).  Every entry
 * point below replaces one method of the reference's C++ classes in src/core (Preprocessing,
 * Frame2Model/Objective + LieGaussNewton, SurfelMap, and the per-scan sequencing of
 * SurfelMapping); the reference-side adapter that keeps those class signatures and calls these
 * functions is shown in INTEGRATION.md and include/suma_adapter.hpp.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no exceptions cross the boundary.
 *  - return value: 0 = SUMA_OK, negative = error (suma_last_error() gives the text).
 *  - one suma_ctx = one HIP device + one HIP stream; calls on a ctx are serialised by the caller
 *    (as in the reference, whose methods all run on the thread that owns the GL context);
 *    different ctxs may be driven from different threads / processes (one per GPU).  suma_ctx_create makes its
 *    device the calling thread's current HIP device; a thread that drives ctxs on DIFFERENT devices must make the
 *    ctx's device current (hipSetDevice) before calling into it -- the entry points do not switch devices.
 *  - matrices are column-major 4x4 (Eigen::Matrix4f / Matrix4d default storage).
 *  - host pointers unless the name says _device.
 *  - there is NO CPU fallback: without a gfx950 device suma_ctx_create fails.
 */
#ifndef SUMA_HIP_H_
#define SUMA_HIP_H_

#include <stdint.h>

#include "suma_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SUMA_OK = 0,
  SUMA_ERR_INVALID = -1,  /* bad argument */
  SUMA_ERR_HIP = -2,      /* HIP runtime error (no device, launch failure, ...) */
  SUMA_ERR_CAPACITY = -3, /* surfel / pose / cache capacity exceeded (reference: silent TF truncation,
                             SurfelMap.cpp:726-727) */
  SUMA_ERR_NOMEM = -4
};

typedef struct suma_ctx suma_ctx;
typedef struct suma_frame suma_frame;       /* reference: class Frame, src/core/Frame.h:21-79 */
typedef struct suma_pipeline suma_pipeline; /* reference: class SurfelMapping, src/core/SurfelMapping.h */

const char* suma_version(void);
/* last error text of this ctx (or of the failed create when ctx == NULL) */
const char* suma_last_error(const suma_ctx* ctx);

/* ---- context: constructors / setParameters of Preprocessing, Frame2Model, LieGaussNewton,
 *      SurfelMap (Preprocessing.cpp:16-118, Frame2Model.cpp:14-110, LieGaussNewton.cpp:81-91,
 *      SurfelMap.cpp:8-457).  Image sizes and capacities are fixed at creation (textures and
 *      buffers are sized in the reference's constructors); all other keys may be re-sent. */
int suma_ctx_create(const suma_params* params, int hip_device, suma_ctx** out);
void suma_ctx_destroy(suma_ctx* ctx);
int suma_set_params(suma_ctx* ctx, const suma_params* params);
int suma_synchronize(suma_ctx* ctx);
/* the hipStream_t the work of this ctx is enqueued on (for event timing by the caller).  One exception: a scan
 * pipeline runs the preprocessing K1-K3 of a scan on a side stream of its own (it overlaps the surfel passes of the
 * previous scan) and joins it to this stream before the first reader.  Consequence for suma_pipeline_*_device: the scan
 * buffers must be COMPLETE when the call is made -- work the caller has enqueued on this stream to produce them is not
 * waited for by the side stream (synchronise it first, or stage through suma_pipeline_prefetch_scan, whose upload the
 * preprocessing does wait for).  SUMA_NO_SIDE_STREAM=1 in the environment keeps everything on this one stream. */
void* suma_ctx_stream(suma_ctx* ctx);

/* ---- frames: Frame::Frame / Frame::copy (Frame.h:26-61); which = SUMA_MAP_* */
int suma_frame_create(suma_ctx* ctx, uint32_t width, uint32_t height, suma_frame** out);
void suma_frame_destroy(suma_frame* f);
int suma_frame_copy(suma_ctx* ctx, suma_frame* dst, const suma_frame* src);
int suma_frame_download(suma_ctx* ctx, const suma_frame* f, int which, suma_float4* host);
int suma_frame_upload(suma_ctx* ctx, suma_frame* f, int which, const suma_float4* host);
/* a frame whose maps were written through an exported device pointer (suma_frame_device_ptr / suma_frame_export) by
 * work the library did not enqueue: tells the render de-duplication and the fused K8 products that the contents
 * changed (every writing call of this API does so by itself) */
int suma_frame_touch(suma_ctx* ctx, suma_frame* f);
uint32_t suma_frame_width(const suma_frame* f);
uint32_t suma_frame_height(const suma_frame* f);
/* device address of one map (HIP->GL interop / zero-copy consumers) */
void* suma_frame_device_ptr(const suma_frame* f, int which);
/* exchange the contents of two frames of equal size (the shared_ptr swaps of SurfelMapping::initialize,
 * SurfelMapping.cpp:323-331): O(1), no copy */
int suma_frame_swap(suma_ctx* ctx, suma_frame* a, suma_frame* b);
/* viewer feed (ViewportWidget.cpp:404-434 binds Frame::vertex_map / normal_map / semantic_map as textures): the
 * device buffer of one map with its layout -- row-major, row 0 = lowest beam, RGBA32F texels, row_bytes = 16 * width.
 * The pointer stays valid for the life of the frame; contents change with the next call that writes the frame.
 * INTEGRATION.md shows the hipGraphicsGLRegisterImage / hipMemcpy2DToArrayAsync recipe. */
int suma_frame_export(suma_ctx* ctx, const suma_frame* f, int which, void** d_ptr, uint32_t* width, uint32_t* height,
                      uint32_t* row_bytes);

/* ---- Preprocessing::process (Preprocessing.h:55-56, Preprocessing.cpp:120-339): K1 z-buffered
 *      spherical scatter, K2 cross-stencil normals + label erosion, K3 label flood fill.
 *      points: n x (x,y,z,1) as rv::Point3f; labels / probs: n floats (may be NULL). */
int suma_preprocess(suma_ctx* ctx, const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                    uint32_t timestamp, suma_frame* out);
/* same with the scan already resident in HBM */
int suma_preprocess_device(suma_ctx* ctx, const suma_float4* d_points, const float* d_labels, const float* d_probs,
                           uint32_t n, uint32_t timestamp, suma_frame* out);

/* ---- Objective::setData (Objective.h:58, Frame2Model.cpp:117-123) */
int suma_icp_set_data(suma_ctx* ctx, const suma_frame* current, const suma_frame* model);
/* ---- the parameters a Frame2Model OBJECT owns (Frame2Model::updateParameters / setParameter, Frame2Model.cpp:65-115).
 *      The reference builds two objectives with different gates -- objective_ and recovery_ = Frame2Model(fallback
 *      parameters), SurfelMapping.cpp:87-94 -- while one suma_ctx carries one parameter block.  An adapter object
 *      sends its own values before each launch; NULL returns to the ctx parameters (suma_params). */
typedef struct suma_icp_objective {
  float icp_max_distance; /* "icp-max-distance" */
  float icp_max_angle;    /* "icp-max-angle", degrees */
  int32_t weight_function; /* SUMA_WEIGHT_* ("weighting") */
  float factor;
  int32_t bilinear_sampling;
} suma_icp_objective;
int suma_icp_set_objective(suma_ctx* ctx, const suma_icp_objective* objective);
/* ---- Frame2Model::jacobianProducts (Frame2Model.h:50, Frame2Model.cpp:136-261): K6 at the given
 *      pose.  JtJ 6x6 column-major, Jtr 6; acc (optional) = the raw 2^-28 fixed-point sums,
 *      SUMA_ACC_WORDS int64.  Returns F in stats->error.
 *      Domain of the sums (the same for every entry point that runs K6: suma_icp_minimize, _minimize_batch, the scan
 *      pipeline, loop-closure verification, the localiser):
 *        - every fp32 term that enters a fixed-point word -- (w J_i) J_j, (w r) J_i, (w r) r -- must satisfy
 *          |term| < 2^23: below that bound the device's conversion is round(term * 2^28) to nearest even, exactly as
 *          the oracle's llrint.  With lidar ranges <= 120 m the largest term is about 1.5e4 (|v x n|^2).  A term at or
 *          beyond the bound leaves ONLY the word it belongs to unspecified; every other word and the three counters
 *          are still exact.  Nothing saturates.
 *        - every texel of a frame handed to K6, valid or not, must hold finite values (no NaN, no inf).
 *        - a pixel that does not contribute -- no pair, or an outlier -- never changes JtJ, Jtr or the inlier sum
 *          (words 0..26 and 28), whatever finite values it holds, including ones whose products overflow.  Word 27
 *          (F over ALL pairs) takes an outlier's w r^2 as the reference does, under the bound above. */
int suma_icp_jacobian_products(suma_ctx* ctx, const double pose[16], uint32_t iteration, double JtJ[36], double Jtr[6],
                               int64_t* acc, suma_icp_stats* stats);
/* ---- LieGaussNewton::minimize (LieGaussNewton.h:32, LieGaussNewton.cpp:13-79) with
 *      Objective::increment / SE3::exp (Objective.h:45-48, lie_algebra.cpp:4-34): the whole
 *      Gauss-Newton loop runs on the device (no per-iteration readback).
 *      history (optional): history_cap x 16 doubles receive LieGaussNewton::history(); *n_hist = entries pushed. */
int suma_icp_minimize(suma_ctx* ctx, const double T0[16], double T_out[16], double* history, uint32_t history_cap,
                      uint32_t* n_hist, suma_icp_stats* stats);
/* Frame2Model::iteration_ the NEXT suma_icp_minimize starts with (one shot; suma_icp_set_data resets it to 0 like
 * Frame2Model::setData, Frame2Model.cpp:117-123).  The reference resets the counter in setData ONLY: a caller that
 * minimises several times on one setData -- the loop over the initial guesses in checkLoopClosure,
 * SurfelMapping.cpp:693-700 -- starts its later minimisations with iteration_ > 0, which the Tukey weight reads
 * (Frame2Model_jacobians.geom:129).  An adapter object passes its own counter here before every minimisation. */
int suma_icp_set_iteration(suma_ctx* ctx, uint32_t iteration);
/* LieGaussNewton::history() (LieGaussNewton.h:44) of the last suma_icp_minimize, fetched on demand: the device always
 * records it, the copy is only paid by callers that look at it (the reference's caller keeps it for drawing,
 * SurfelMapping.cpp:391).  *n_hist = entries the minimisation pushed; min(that, history_cap) x 16 doubles are copied. */
int suma_icp_history(suma_ctx* ctx, double* history, uint32_t history_cap, uint32_t* n_hist);
/* The history lives in ONE device buffer per context; every minimisation that records one (suma_icp_minimize, also inside
 * suma_loop_closure_verify_serial / suma_loop_closure_track; NOT the batched suma_loop_closure_verify nor the scan
 * pipeline's own minimisations, which record none) overwrites it and advances this counter.  The reference keeps history_ per optimizer
 * object (LieGaussNewton.h:72): an adapter object notes the counter after ITS minimisation and refuses to hand out
 * another chain's poses when it has moved (include/suma_adapter.hpp, LieGaussNewton::history). */
uint64_t suma_icp_history_sequence(const suma_ctx* ctx);
/* LieGaussNewton::information() (LieGaussNewton.h:50, LieGaussNewton.cpp:75,103-105): J^T W J of the last step of the
 * last suma_icp_minimize (or of the last suma_icp_jacobian_products), 6x6 column-major */
int suma_icp_information(suma_ctx* ctx, double information[36]);
/* n_hyp independent minimisations of the same frame pair from different T0 (the reference's
 * loop-closure verification pattern, SurfelMapping.cpp:662-779; BASELINE config 3) in one batch. */
int suma_icp_minimize_batch(suma_ctx* ctx, const double* T0s, uint32_t n_hyp, double* T_out, suma_icp_stats* stats);

/* ---- SurfelMap (SurfelMap.h:36-78) */
int suma_map_reset(suma_ctx* ctx);                                                  /* SurfelMap.cpp:473-482 */
int suma_map_update(suma_ctx* ctx, const float pose[16], const suma_frame* frame); /* SurfelMap.cpp:492-584 */
/* render(pose_old, pose_new, frame, ct), SurfelMap.cpp:847-1021; also fills the OLD / NEW frames */
int suma_map_render(suma_ctx* ctx, const float pose_old[16], const float pose_new[16], float conf_threshold,
                    suma_frame* out);
int suma_map_render_active(suma_ctx* ctx, const float pose[16], float conf_threshold);   /* SurfelMap.cpp:1023-1069 */
int suma_map_render_inactive(suma_ctx* ctx, const float pose[16], float conf_threshold); /* SurfelMap.cpp:1071-1114 */
int suma_map_render_composed(suma_ctx* ctx, const float pose_old[16], const float pose_new[16],
                             float conf_threshold);                                      /* SurfelMap.cpp:1116-1165 */
/* oldMapFrame() / newMapFrame() / composedFrame(), SurfelMap.h:59-61; which = SUMA_FRAME_* */
suma_frame* suma_map_frame(suma_ctx* ctx, int which);
int suma_map_update_poses(suma_ctx* ctx, const float* poses16, uint32_t n); /* SurfelMap.cpp:485-490 */
int suma_map_size(suma_ctx* ctx, uint32_t* n);                              /* SurfelMap::size() */
int suma_map_timestamp(suma_ctx* ctx, uint32_t* t);
/* getAllSurfels(), SurfelMap.cpp:1232-1237: copies min(size, cap) surfels; *n = size */
int suma_map_download(suma_ctx* ctx, suma_surfel* host, uint32_t cap, uint32_t* n);
/* viewer feed / getModelSurfels() / getDataSurfels() (SurfelMap.h:64-67; SurfelMap::draw reads the surfel VBO,
 * SurfelMap.cpp:1167-1230): the device buffer of the active map, *n records of 64 bytes in the layout of
 * suma_surfel (= the reference's Surfel / its VAO layout, SurfelMap.cpp:46-55).  The map is double buffered: the
 * pointer is valid (and its contents stable) until the next suma_map_update / suma_map_upload / suma_map_reset or
 * pipeline scan.  The data surfels of the last update are the tail [*first, *first + *n_data) of the same buffer:
 * the new surfels that survived the active-area copy (the reference's data_surfels_ also holds the ones K11
 * dropped).  INTEGRATION.md shows the hipGraphicsGLRegisterBuffer recipe. */
int suma_map_export_surfels(suma_ctx* ctx, void** d_ptr, uint32_t* n);
int suma_map_export_data_surfels(suma_ctx* ctx, void** d_ptr, uint32_t* first, uint32_t* n_data);
/* replace the active map alone (tests, map surgery); a whole session is saved and resumed with
 * suma_pipeline_checkpoint_save / _load below.  At most max_surfels records are taken.
 * DOMAIN: every record's `count` (its creation stamp) must be an integer in [0, max_poses).  The update, render and
 * extraction kernels index the pose table by it unchecked, as the reference's shaders fetch poseBuffer; a record outside
 * that range makes them read out of bounds.  Position, normal, radius, confidence, weight and the semantic payload may
 * hold any float (NaN, inf and zero included: tests/test_update_crafted_host.py "bad-records"). */
int suma_map_upload(suma_ctx* ctx, const suma_surfel* host, uint32_t n, uint32_t timestamp);
/* intermediates of the last update, for stage-by-stage parity tests */
int suma_map_download_index_map(suma_ctx* ctx, uint32_t* host);      /* P, surfel id + 1 (uint32, not float) */
int suma_map_download_radius_conf(suma_ctx* ctx, suma_float4* host); /* P */
int suma_map_download_integrated(suma_ctx* ctx, uint8_t* host);      /* P */
int suma_map_counts(suma_ctx* ctx, uint32_t* n_updated, uint32_t* n_new, uint32_t* n_cached, int32_t origin_ij[2]);
/* SurfelMap::poses_ (SurfelMap.h:205-208): the pose table, entries 0 .. timestamp - 1 (16 floats each, column-major; after
 * suma_map_update_poses the optimised ones).  *n = entries in the table; min(*n, capacity) are copied. */
int suma_map_download_poses(suma_ctx* ctx, float* host, uint32_t capacity, uint32_t* n);
/* the submap cache in HBM (the reference pages tiles to host vectors, SurfelMap.h:186, SurfelMap.cpp:733-734): surfels
 * allocated from the arena (live tiles + the blocks that re-extracted tiles left behind), its capacity
 * (suma_params.cache_surfels), and how often it has been compacted -- when it runs full the live tiles are copied into
 * a fresh arena; SUMA_ERR_CAPACITY only if the live tiles alone do not fit */
int suma_map_cache_stats(suma_ctx* ctx, uint32_t* used, uint32_t* capacity, uint32_t* compactions);
/* one parked tile, as the reference keeps it in submapCache_(i, j).surfels (SurfelMap.h:186, filled by extractSurfels,
 * SurfelMap.cpp:733-734): *n = its surfels (0 for a tile that was never extracted); the first min(*n, capacity)
 * records are copied to `host` (may be NULL with capacity 0 to ask for the size) */
int suma_map_download_cached_tile(suma_ctx* ctx, int32_t i, int32_t j, suma_surfel* host, uint32_t capacity, uint32_t* n);

/* ---- SurfelMapping::processScan (SurfelMapping.h:47, SurfelMapping.cpp:175-210) without the
 *      loop-closure / pose-graph part: initialize, preprocess, updatePose
 *      (incl. the frame-to-frame fallback, :434-449), updateMap.
 *      fixed_iterations > 0 runs exactly that many GN iterations (bench mode). */
int suma_pipeline_create(const suma_params* params, int hip_device, suma_pipeline** out);
void suma_pipeline_destroy(suma_pipeline* s);
/* SurfelMapping::reset (SurfelMapping.cpp:131-169): empty map, identity poses, timestamp 0 */
int suma_pipeline_reset(suma_pipeline* s);
suma_ctx* suma_pipeline_ctx(suma_pipeline* s);
int suma_pipeline_process_scan(suma_pipeline* s, const suma_float4* points, const float* labels, const float* probs,
                               uint32_t n, int32_t fixed_iterations);
int suma_pipeline_process_scan_device(suma_pipeline* s, const suma_float4* d_points, const float* d_labels,
                                      const float* d_probs, uint32_t n, int32_t fixed_iterations);
/* ---- device-side scan ingest (KITTIReader::read hands over host vectors, KITTIReader.cpp:136-203 ->
 *      SurfelMapping::processScan(const rv::Laserscan&), SurfelMapping.cpp:175): three pinned staging slots, a copy
 *      stream and an ingest thread.  prefetch stages the scan (host copy into pinned memory + async H2D, both off
 *      the caller's thread) and returns at once; process_prefetched runs the oldest staged scan, its first kernel
 *      waiting on the upload's event.  Calling prefetch(scan k+1) before process_prefetched(scan k) overlaps the
 *      upload of k+1 with the kernels of k.  At most two scans may be staged; the host arrays must stay valid
 *      until the matching process call returns.  suma_pipeline_process_scan_async = prefetch (unless that very
 *      scan is already staged) + process_prefetched. */
int suma_pipeline_prefetch_scan(suma_pipeline* s, const suma_float4* points, const float* labels, const float* probs,
                                uint32_t n);
int suma_pipeline_process_prefetched(suma_pipeline* s, int32_t fixed_iterations);
int suma_pipeline_process_scan_async(suma_pipeline* s, const suma_float4* points, const float* labels,
                                     const float* probs, uint32_t n, int32_t fixed_iterations);
/* ---- the phases of SurfelMapping::processScan as calls of their own (SurfelMapping.cpp:175-204), for hosts that run
 *      loop closures between them -- config/default.xml:71 ships close-loops = true, and then processScan is
 *        integrateLoopClosures (:179) -> initialize + preprocess (:181-187) -> updatePose (:192) ->
 *        checkLoopClosure (:196) -> updateMap (:201) -> timestamp_ += 1 (:209).
 *      begin_scan = initialize + preprocess (K1-K3 on the side stream, the pre-ICP render(pose_old, pose_new));
 *      update_pose = updatePose (no-op while timestamp == 0, as :190); update_map = updateMap + timestamp_ += 1.
 *      suma_pipeline_process_scan* IS these three back to back: same launches, same side stream, fused K7 / K8, lazy
 *      statistics and render de-duplication -- a host with loop closures on loses none of them.
 *      Between update_pose and update_map the host may call suma_pipeline_verify_loop_closure /
 *      suma_pipeline_track_loop_closure (the device sides of checkLoopClosure) and suma_pipeline_set_pose_old;
 *      before begin_scan, suma_pipeline_integrate_loop_closures.  Or it enables the pipeline's own loop closing
 *      (suma_pipeline_enable_loop_closing) and calls suma_pipeline_check_loop_closure there. */
int suma_pipeline_begin_scan(suma_pipeline* s, const suma_float4* points, const float* labels, const float* probs,
                             uint32_t n);
int suma_pipeline_begin_scan_device(suma_pipeline* s, const suma_float4* d_points, const float* d_labels,
                                    const float* d_probs, uint32_t n);
/* the oldest scan staged with suma_pipeline_prefetch_scan */
int suma_pipeline_begin_prefetched(suma_pipeline* s);
int suma_pipeline_update_pose(suma_pipeline* s, int32_t fixed_iterations);
int suma_pipeline_update_map(suma_pipeline* s);
/* integrateLoopClosures (SurfelMapping.cpp:211-250) once the pose graph has been optimised: map_->updatePoses(poses)
 * (:236), currentPose_ = difference * currentPose_ (:239), currentPose_new_ = currentPose_old_ = currentPose_ (:243).
 * poses16: n x 16 floats (casted_poses); difference: poses_opt[beforeID_] * beforeOptimizationPose_^-1 (:229). */
int suma_pipeline_integrate_loop_closures(suma_pipeline* s, const float* poses16, uint32_t n, const double difference[16]);
/* currentPose_old_ = ... (SurfelMapping.cpp:582 after a tracked closure, :744 after a verified candidate): the pose the
 * NEXT scan's render() uses for the inactive ("old") part of the map */
int suma_pipeline_set_pose_old(suma_pipeline* s, const double pose_old[16]);
/* which: 0 currentPose_, 1 currentPose_old_, 2 currentPose_new_, 3 lastPose_old_ (:456), 4 lastPose_ */
int suma_pipeline_get_pose(const suma_pipeline* s, int which, double pose[16]);
/* result_new_ of updatePose (:417-423): the statistics pass of the current scan (resolves the lazy read-back) --
 * what checkLoopClosure compares candidates against (:538-539, :582, :727-729) */
int suma_pipeline_result_new(suma_pipeline* s, suma_icp_stats* st);

/* ---- several pose hypotheses per scan (BASELINE config 3; the reference runs several minimisations of one frame pair
 *      from different starts in its loop-closure verification, SurfelMapping.cpp:662-779): between begin_scan and
 *      update_map, INSTEAD of update_pose.  minimize_hypotheses runs n_hyp (<= 64) device-resident Gauss-Newton chains
 *      as one batch against the rendered model (map_->newMapFrame(), as updatePose does, :384); apply_increment does
 *      updatePose's pose bookkeeping (:453-474) for the increment the caller chose.  T0s / T_out: n_hyp x 16 doubles. */
int suma_pipeline_minimize_hypotheses(suma_pipeline* s, const double* T0s, uint32_t n_hyp, int32_t fixed_iterations,
                                      double* T_out, suma_icp_stats* stats);
int suma_pipeline_apply_increment(suma_pipeline* s, const double increment[16]);

int suma_pipeline_pose(const suma_pipeline* s, double pose[16]);
int suma_pipeline_last_increment(const suma_pipeline* s, double inc[16]);
int suma_pipeline_last_stats(const suma_pipeline* s, suma_icp_stats* st);
/* the frame-to-model minimisation of the last suma_pipeline_update_pose as gn_ left it (iterations = gn_->iterationCount(),
 * SurfelMapping.cpp:394; converged; the objective's counters after the last step) -- known when update_pose returns,
 * unlike the statistics pass behind it (suma_pipeline_last_stats), which is read back lazily */
int suma_pipeline_minimize_stats(const suma_pipeline* s, suma_icp_stats* st);
uint32_t suma_pipeline_timestamp(const suma_pipeline* s);
/* number of scans on which the frame-to-frame fallback minimisation ran (trackLoss_, SurfelMapping.cpp:441) */
uint32_t suma_pipeline_track_loss(const suma_pipeline* s);
/* which: 0 current data frame, 1 last model frame, 2 current model frame */
suma_frame* suma_pipeline_frame(suma_pipeline* s, int which);

/* ---- loop-closure verification, the device side of SurfelMapping::checkLoopClosure
 *      (SurfelMapping.cpp:662-757): render the inactive map from a candidate pose, run the
 *      frame-to-model minimisation from each initial guess, and -- for guesses that pass the
 *      valid / outlier gates -- render the composed (old + new) view and evaluate the objective at
 *      identity against it.  Faithful to the reference's sequencing, including its quirk that after
 *      a passing guess the objective keeps pointing at the composed frame for the remaining guesses
 *      (setData is called once before the loop, :693, and again inside the branch, :719).
 *      The candidate search, thresholds on the returned ratios and the pose-graph edges are the caller's here;
 *      suma_pipeline_enable_loop_closing (below) is the pipeline doing all of it itself. */
typedef struct suma_loop_result {
  double gn_pose[16];            /* LieGaussNewton::pose() of this guess (relative to pose_prior) */
  suma_icp_stats after_minimize; /* jacobianProducts at that pose (:705): valid / outlier ratios */
  int32_t passed;                /* valid_ratio > min_valid_ratio && outlier_ratio < max_outlier_ratio (:713) */
  float pose_old[16];            /* (pose_prior * gn_pose).cast<float>() (:714) */
  suma_icp_stats composed;       /* jacobianProducts at identity against composedFrame (:723); zero if !passed */
  double JtJ[36];                /* information matrix of that evaluation (result_old_.information, :744) */
} suma_loop_result;
int suma_loop_closure_verify(suma_ctx* ctx, const suma_frame* current, const double pose_prior[16],
                             const double* initializations, uint32_t n_init, const float pose_new[16],
                             float conf_threshold, float min_valid_ratio, float max_outlier_ratio,
                             suma_loop_result* out);
/* suma_loop_closure_verify minimises the initial guesses as ONE batched Gauss-Newton chain (grid.y = guess) with the
 * per-guess evaluation (:705) riding on the same chain states: one chain of launches and one synchronisation when no
 * guess (or only the last) passes; after a guess that passes, the later guesses -- which the reference minimises
 * against composedFrame() (:718-719) -- are redone as a batch against that frame.  This entry is the reference's
 * sequencing literally (one minimisation, one evaluation, two host round trips per guess): identical results, kept as
 * the cross-check of the batched form and for the A/B timing in bench.py. */
int suma_loop_closure_verify_serial(suma_ctx* ctx, const suma_frame* current, const double pose_prior[16],
                                    const double* initializations, uint32_t n_init, const float pose_new[16],
                                    float conf_threshold, float min_valid_ratio, float max_outlier_ratio,
                                    suma_loop_result* out);

/* the same on a pipeline's own state between suma_pipeline_update_pose and suma_pipeline_update_map: current frame,
 * currentPose_new_ and getConfidenceThreshold() are the pipeline's (SurfelMapping.cpp:679-719) */
int suma_pipeline_verify_loop_closure(suma_pipeline* s, const double pose_prior[16], const double* initializations,
                                      uint32_t n_init, float min_valid_ratio, float max_outlier_ratio,
                                      suma_loop_result* out);

/* ---- the other device part of checkLoopClosure: re-verifying a closure that is being tracked, on the scans that
 *      follow its detection (SurfelMapping.cpp:546-574): render the inactive map from lastPose_old_, minimise from
 *      lastIncrement_, gate on the valid / outlier ratios of the objective as the minimisation left it (:557-558) and on
 *      |log(lastIncrement_) - log(increment_old)| (:561-563; SE3::log, lie_algebra.cpp:36-71), then render the composed
 *      view at lastPose_old_ * increment_old and evaluate the objective at identity against it (:566-572).  The
 *      reference's gates are the literals 0.2 / 0.85 / 0.1. */
typedef struct suma_loop_track {
  double increment_old[16];      /* gn_->pose() (:560) */
  suma_icp_stats after_minimize; /* objective_->valid() / outlier() / inlier() / invalid() after minimize (:557-558) */
  float increment_difference;    /* (:561) */
  int32_t passed;                /* (:563) */
  double pose_old[16];           /* lastPose_old_ * increment_old (:564, :581): what currentPose_old_ becomes */
  suma_icp_stats composed;       /* jacobianProducts at identity against composedFrame (:570-572); zero if !passed */
  double JtJ[36];
} suma_loop_track;
int suma_loop_closure_track(suma_ctx* ctx, const suma_frame* current, const double last_pose_old[16],
                            const double last_increment[16], const float pose_new[16], float conf_threshold,
                            double min_valid_ratio, double max_outlier_ratio, double max_increment_difference,
                            suma_loop_track* out);
/* on a pipeline's own state (lastPose_old_, lastIncrement_, currentPose_new_, current frame); the reference's
 * gates are 0.2, 0.85, 0.1 */
int suma_pipeline_track_loop_closure(suma_pipeline* s, double min_valid_ratio, double max_outlier_ratio,
                                     double max_increment_difference, suma_loop_track* out);
/* SE3::log (lie_algebra.cpp:36-71), host side: x = (v, omega) */
void suma_se3_log(const double T[16], double x[6]);

/* Semantic front end (suma_semantic_project / suma_semantic_unproject, include/suma_hip.h): the range image a
 * RangeNet++-style segmentation network consumes, and the map from its class scores back to per-point labels.  It
 * stands in for RangenetAPI::infer + the argmax of the reference's KITTIReader::read (src/io/KITTIReader.cpp:172-200);
 * the network itself is the caller's.  The image has its own geometry (RangeNet++ is trained on 64 x 2048, fov 3 / -25):
 * it is NOT the data image of suma_params.  (Kept here, not in suma_types.h: that header is part of the arithmetic
 * specification the CPU checker's recorded traces are tied to.) */
#define SUMA_SEM_MAX_CLASSES 32 /* compile-time maximum of n_classes (the reference's network has 20) */
#define SUMA_SEM_CHANNELS 5     /* input planes: range, x, y, z, remission */
typedef struct suma_semantic_params {
  uint32_t width, height;            /* W x H of the network's range image */
  float fov_up, fov_down;            /* degrees; only |fov_up| and |fov_down| are used */
  float means[SUMA_SEM_CHANNELS];    /* per-channel normalisation (v - mean) / std, from the model's config */
  float stds[SUMA_SEM_CHANNELS];
  uint32_t n_classes;                /* C: score planes, 1 .. SUMA_SEM_MAX_CLASSES */
  int32_t label_map[SUMA_SEM_MAX_CLASSES]; /* class index -> reported label id (learning_map_inv) */
} suma_semantic_params;

/* ---- semantic front end (suma_semantic_params above): the device side of the reference's
 *      RangenetAPI::infer + argmax (KITTIReader.cpp:172-200) around a segmentation network the caller runs.
 *      Both entries run on the ctx stream and take caller-owned device buffers (k_semantic.hip states the arithmetic).
 *
 * suma_semantic_project: d_points n x (x, y, z, remission) as in a KITTI .bin -> d_input, a planar [5, H, W] fp32
 *   tensor of the channels (range, x, y, z, remission), each (v - mean_c) / std_c, 0 in every channel of an empty pixel.
 *   RangeNet++'s convention: depth = |p|, yaw = -atan2(y, x), pitch = asin(z / depth),
 *   u = 0.5 (yaw / pi + 1) W, v = (1 - (pitch + |fov_down|) / fov) H, fov = |fov_up| + |fov_down|; floor, then CLAMP
 *   to [0, W-1] x [0, H-1].  Row 0 is the TOP of the image (highest pitch) -- the opposite of the frames' vertex maps.
 *   A point with a non-finite coordinate, zero range or a range that overflows is not projected.  The nearest point
 *   wins its pixel, equal ranges go to the lower point index.
 *   d_pixel (optional): n int32, the pixel y * W + x of every point, -1 = not projected.
 *   d_proj_idx (optional): H * W int32, the winning point of every pixel, -1 = empty. */
int suma_semantic_project(suma_ctx* ctx, const suma_semantic_params* sp, const suma_float4* d_points, uint32_t n,
                          float* d_input, int32_t* d_pixel, int32_t* d_proj_idx);
/* suma_semantic_unproject: d_scores a planar [C, H, W] fp32 tensor (C = n_classes), d_pixel as written by
 *   suma_semantic_project -> d_labels / d_probs (n floats each).  Every projected point reads its own pixel's scores,
 *   also a point hidden behind a nearer one (suma_semantic_unproject_knn below votes instead).  scores_are_logits != 0: a softmax over C first.  Then the reference's
 *   rule literally (KITTIReader.cpp:189-200): label = 0, prob = 0; for j = 0 .. C-1: if (prob <= s_j) label =
 *   label_map[j], prob = s_j -- the last maximum wins, all-negative scores give (0, 0), a NaN never wins.  Points that
 *   were not projected (pixel < 0 or >= H * W) get (0, 0). */
int suma_semantic_unproject(suma_ctx* ctx, const suma_semantic_params* sp, const float* d_scores, int scores_are_logits,
                            const int32_t* d_pixel, uint32_t n, float* d_labels, float* d_probs);
/* ---- a scan whose labels come from network scores still on the device: begin_scan_device / process_scan_device with
 *      the back-projection in front.  The pipeline's preprocessing stream waits for producer_event (a hipEvent_t recorded
 *      behind the work that writes d_points / d_scores / d_pixel; NULL = those buffers are complete at call time), runs
 *      suma_semantic_unproject into labels / probs the ctx owns, then K1-K3 exactly as begin_scan_device does -- no host
 *      synchronisation.  Unlike the *_device entries, the scan buffers need not be complete when the call is made.
 *      They are read until the ctx stream (suma_ctx_stream) has passed the suma_pipeline_update_map of this scan
 *      (process_scan_scores includes it): the ctx stream waits for the preprocessing before its first reader of the
 *      frame, so work enqueued on the ctx stream after the call, or behind an event recorded there, may reuse them. */
int suma_pipeline_begin_scan_scores(suma_pipeline* s, const suma_semantic_params* sp, const suma_float4* d_points,
                                    const float* d_scores, int scores_are_logits, const int32_t* d_pixel, uint32_t n,
                                    void* producer_event);
int suma_pipeline_process_scan_scores(suma_pipeline* s, const suma_semantic_params* sp, const suma_float4* d_points,
                                      const float* d_scores, int scores_are_logits, const int32_t* d_pixel, uint32_t n,
                                      void* producer_event, int32_t fixed_iterations);

/* ---- RangeNet++'s KNN post-processing (Milioto et al., IROS 2019, section III-D), opt-in: the back-projection above
 *      with a vote among the points nearest in range around each point's pixel, so that a point hidden behind a nearer
 *      one does not take that one's class (k_semantic_knn.hip states the arithmetic).  The published defaults are
 *      search 5, k 5, sigma 1, cutoff 1. */
typedef struct suma_semantic_knn {
  uint32_t search; /* S: an S x S window around the pixel, odd, 1 .. 9 */
  uint32_t k;      /* K candidates vote, 1 .. S * S; the point itself is always the first */
  float sigma;     /* Gaussian of the window's distance weights, finite, > 0 */
  float cutoff;    /* a candidate farther than cutoff (weighted range difference, m) does not vote; <= 0: no cutoff */
} suma_semantic_knn;
/* suma_semantic_unproject_knn: as suma_semantic_unproject, with d_points and d_proj_idx as suma_semantic_project took /
 *   wrote them.  Each point's candidates are its pixel (its own range, the pixel's class) and the S x S - 1 pixels
 *   around it (the range of their winner, +inf when empty; outside the image 0 and no class: the columns do not wrap),
 *   ranked by |range - the point's range| * (1 - the normalised Gaussian weight of the offset), ties to the lower
 *   window index.  The first K vote for their pixel's class (the reference's argmax rule, on the index) unless it is
 *   none, index 0 or (cutoff > 0) farther than cutoff; the most votes win, equal counts go to the lowest index.
 *   label = label_map[winner], prob = the largest pixel prob among its voters; no vote gives (0, 0), and so does a
 *   point that suma_semantic_project would not have projected (d_pixel outside [0, H * W), or -- with a d_pixel that was
 *   not made from these points -- a zero, non-finite or overflowing range of its own).  search = 1 or
 *   k = 1 gives the plain back-projection for every point whose pixel class is >= 1.  Runs on the ctx stream; its
 *   scratch (12 bytes a pixel, kept by the ctx) is used only there.  Invalid parameters return SUMA_ERR_INVALID. */
int suma_semantic_unproject_knn(suma_ctx* ctx, const suma_semantic_params* sp, const suma_semantic_knn* knn,
                                const suma_float4* d_points, const float* d_scores, int scores_are_logits,
                                const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n, float* d_labels,
                                float* d_probs);
/* the *_scores pipeline entries with suma_semantic_unproject_knn in front: on the preprocessing stream, behind
 *   producer_event, with the same buffer lifetime rule (d_proj_idx is a scan buffer too).  The pipeline keeps scratch of
 *   its own for this, used only on that stream. */
int suma_pipeline_begin_scan_scores_knn(suma_pipeline* s, const suma_semantic_params* sp, const suma_semantic_knn* knn,
                                        const suma_float4* d_points, const float* d_scores, int scores_are_logits,
                                        const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n,
                                        void* producer_event);
int suma_pipeline_process_scan_scores_knn(suma_pipeline* s, const suma_semantic_params* sp, const suma_semantic_knn* knn,
                                          const suma_float4* d_points, const float* d_scores, int scores_are_logits,
                                          const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n,
                                          void* producer_event, int32_t fixed_iterations);

/* ---- SurfelMap::draw (SurfelMap.cpp:1167-1230): the viewer's picture of the active map, without a graphics pipeline.
 *      The reference's draw_surfels.{vert,geom,frag} program run by a compute rasteriser (k_draw.hip states the
 *      arithmetic).  (Kept here, not in suma_types.h, for the reason given at suma_semantic_params.) */
#define SUMA_DRAW_MAX_LIGHTS 10  /* draw_surfels.geom: uniform Light lights[10] */
#define SUMA_DRAW_MAX_SIZE 8192u /* width and height: 1 .. SUMA_DRAW_MAX_SIZE */
#define SUMA_DRAW_COLORS 260     /* texels of the semantic colour map (SurfelMap::setColorMap, SurfelMap.cpp:1238-1256) */
typedef struct suma_draw_light {
  float position[4]; /* w < 0.0001: a directional light from -position.xyz */
  float ambient[3], diffuse[3], specular[3];
} suma_draw_light;
typedef struct suma_draw_params {
  float mvp[16];          /* column-major: projection * view * conversion (ViewportWidget.cpp:913) */
  float view_pos[3];      /* camera position in the map frame (ViewportWidget.cpp:567, 909-911) */
  uint32_t width, height; /* 1 .. SUMA_DRAW_MAX_SIZE each */
  int32_t color_mode;     /* 0 .. 5, SurfelMapVisualOptions::colorMode (SurfelMap.h:23-33), default 5:
                             0 Phong, 1 normal shading, 2 abs(normal), 3 viridis(confidence), 4 surfel colour, 5 semantic */
  float conf_threshold;   /* default 10 */
  int32_t backface_culling; /* default 0 */
  int32_t use_stability;    /* default 0: SurfelMap never sets it on its draw program (SurfelMap.cpp:187-229) */
  float clear_color[4];     /* RGBA in [0, 1], default white (ViewportWidget.cpp:472) */
  uint32_t num_lights;      /* 0 .. SUMA_DRAW_MAX_LIGHTS, default 1 */
  suma_draw_light lights[SUMA_DRAW_MAX_LIGHTS];
  float mat_ambient[3], mat_diffuse[3], mat_specular[3], mat_emission[3], mat_shininess, mat_alpha;
  uint8_t color_map[SUMA_DRAW_COLORS][3]; /* label id -> RGB (setColorMap has already swapped the BGR of the config) */
} suma_draw_params;

/* The state SurfelMap's constructor leaves on draw_surfels_ (SurfelMap.cpp:195-229: the last value of every uniform it
 * sets twice, num_lights = 1; lights 1-4 hold its "evenly distributed sun light") and SurfelMapVisualOptions' defaults
 * (color_mode 5, conf_threshold 10, no back-face culling), white clear colour; mvp, view_pos, width, height and color_map
 * are the caller's (zeroed here). */
void suma_draw_params_default(suma_draw_params* dp);

/* suma_map_draw: the active map (the buffer SurfelMap::draw reads, suma_map_export_surfels) drawn on the ctx stream,
 *   behind the last update / upload / update_poses, with a 24-bit GL_LESS depth test and no blending.
 *   d_rgba8: width * height RGBA8 pixels (4 bytes each, R first) in glReadPixels order -- row 0 is the BOTTOM row.
 *   d_ids (optional): width * height int32, the index of the surfel that won each pixel, -1 where nothing was drawn.
 *   Returns without synchronising; both buffers are complete once the ctx stream has passed the call.  The z-buffer
 *   (8 bytes a pixel, grown to the largest image drawn) and a queue of max_surfels entries are the ctx's; nothing else of
 *   the ctx changes (map, poses, counters, render de-duplication).  Invalid parameters return SUMA_ERR_INVALID with a
 *   message and launch nothing. */
int suma_map_draw(suma_ctx* ctx, const suma_draw_params* dp, void* d_rgba8, int32_t* d_ids);

/* ---- the whole surfel map in the world frame: the active map and every parked submap tile, filtered, optionally fused
 *      to one record per voxel with a label vote (k_world.hip states the specification; tests/world_shim.c restates it
 *      on the host, and the export equals it byte for byte). */
typedef struct suma_world_surfel {   /* 48 bytes */
  float x, y, z, radius;             /* world frame */
  float nx, ny, nz, confidence;
  uint32_t label;                    /* 0 .. 259 */
  float prob;
  uint32_t timestamp;                /* last update (voxel mode: the latest of the members) */
  uint32_t support;                  /* source surfels behind this record; 1 without voxel fusion */
} suma_world_surfel;

typedef struct suma_world_params {
  float voxel_size;                  /* 0: one record per surfel; > 0: one record per occupied voxel (metres) */
  float min_confidence;              /* keep iff confidence > min_confidence; default -INFINITY (a NaN confidence never passes) */
  uint8_t keep_label[SUMA_DRAW_COLORS]; /* keep iff keep_label[label] != 0; default all 1 */
} suma_world_params;

typedef struct suma_world_stats {
  uint32_t n_active, n_tiles, n_parked;   /* sources: active surfels, non-empty parked tiles, their surfels */
  uint32_t n_passed;                      /* after the confidence and label filters */
  uint32_t n_dropped;                     /* passed, but world position non-finite or (voxel mode) outside the grid */
  uint32_t n_out;                         /* records the export has in total (may exceed capacity) */
} suma_world_stats;

void suma_world_params_default(suma_world_params* wp);
/* the (i, j) of every parked tile that holds records, ascending by (i, then j), as pairs ij[2 k], ij[2 k + 1]; *n = how
 * many exist (the first min(*n, capacity) are written; ij may be NULL when capacity is 0) */
int suma_map_cached_tiles(suma_ctx* ctx, int32_t* ij, uint32_t capacity, uint32_t* n);
/* suma_map_export_world: the source sequence (the active map in buffer order, then every non-empty parked tile ascending
 *   by (i, j), each in its stored order) taken to the world frame through the pose table, on the ctx stream, behind the
 *   last update / upload / update_poses.  Writes the first min(n_out, capacity) records to the DEVICE buffer d_out (may be
 *   NULL when capacity is 0: a size query) and fills *stats; SUMA_OK even when n_out > capacity (suma_map_download's
 *   convention).  Blocking, twice: it reads the map's counters and the tiles' slots to size its launches (the sorts take
 *   their size on the host), and waits for the result to fill *stats.
 *   Like suma_map_draw it leaves the map, the pose table, the cache arena, every counter and the render de-duplication
 *   untouched.  Scratch, kept by the ctx and grown by its one rule: 8 bytes per source surfel with voxel_size == 0,
 *   48 bytes with voxel_size > 0 (a 16-byte vote record and the double buffers of the two sorts: keys 2 x 8, labels
 *   2 x 4, indices 2 x 4), plus the sorts' histograms (they sort in place in those double buffers and take no copy of
 *   their input) and 16 bytes per parked tile.  Two calls on the same state give the same bytes.  A map that an
 *   overflow of max_surfels or of the cache arena has truncated is exported, and SUMA_ERR_CAPACITY returned, as the
 *   downloads do.
 *   A NULL wp or stats, a negative / NaN / infinite voxel_size, a NaN min_confidence and a NULL d_out with capacity > 0
 *   return SUMA_ERR_INVALID with a message and launch nothing. */
int suma_map_export_world(suma_ctx* ctx, const suma_world_params* wp, suma_world_surfel* d_out, uint32_t capacity,
                          suma_world_stats* stats);

/* ---- a 2.5-D semantic traversability grid of world-frame records, for a planner: per cell of an x / y raster the ground
 *      height, what stands on it within the robot's height, the voted class and a state (k_grid.hip states the
 *      specification; tests/grid_shim.c restates it on the host, and the grid equals it byte for byte).
 *      The world frame has z UP: it is the first scan's sensor frame (x forward, y left, z up), so "height" is z and the
 *      raster spans x (columns) and y (rows). */
typedef struct suma_grid_params {
  float cell_size;            /* metres; finite, > 0; default 0.2 */
  float origin_x, origin_y;   /* world coordinates of the lower corner of cell (0, 0); finite */
  uint32_t width, height;     /* cells along x / y; >= 1; width * height <= 2^26 */
  uint8_t ground_label[SUMA_DRAW_COLORS]; /* a label counts as ground iff != 0; default: 40 road, 44 parking, 48 sidewalk,
                                             49 other-ground, 60 lane-marking, 72 terrain */
  float min_normal_z;         /* default 0.7: a ground member needs |nz| >= this (a NaN never does) */
  float step_height;          /* default 0.2 m: a member more than this above the ground is an obstacle; finite */
  float clearance;            /* default 2.0 m: a member more than this above the ground is an overhang; finite, > step_height */
  uint32_t fill_radius;       /* default 2 cells; 0 .. 8: how far a cell without ground looks for a neighbour's */
} suma_grid_params;

enum { SUMA_GRID_UNKNOWN = 0, SUMA_GRID_FREE = 1, SUMA_GRID_OBSTACLE = 2, SUMA_GRID_NO_GROUND = 3 };

typedef struct suma_grid_cell {   /* 48 bytes */
  float ground_z, ground_rough, z_min, z_max;   /* NaN where undefined */
  float obstacle_z, prob;         /* the highest obstacle member's z (NaN: none); the voted label's share of the vote */
  uint32_t label, support;        /* the voted label; the records binned into the cell */
  uint32_t n_ground, n_obstacle, n_overhang;
  uint8_t state;          /* 0 UNKNOWN, 1 FREE, 2 OBSTACLE, 3 NO_GROUND */
  uint8_t ground_source;  /* 0 none, 1 own, 2 filled from a neighbour */
  uint8_t pad[2];         /* 0 */
} suma_grid_cell;

typedef struct suma_grid_stats {
  uint32_t n_records, n_dropped, n_outside, n_binned; /* n_records = n_dropped + n_outside + n_binned */
  uint32_t n_occupied;                                /* cells with support > 0 = n_free + n_obstacle + n_no_ground */
  uint32_t n_free, n_obstacle, n_no_ground;           /* cells by state */
  uint32_t n_filled;                                  /* cells with ground_source 2 */
} suma_grid_stats;

/* the defaults above; origin 0, 0 and width = height = 0: to be set, or fitted by suma_world_grid_fit */
void suma_grid_params_default(suma_grid_params* gp);
/* Both entries take a DEVICE array of n records, 16-byte aligned (what suma_map_export_world writes, or a caller's records
 *   after suma_device_upload), run on the ctx stream and block once, for their result.  They write only scratch of the ctx
 *   and the caller's d_cells: the records, the map and every counter of the ctx stay as they are.
 *   SUMA_ERR_INVALID with a message, and nothing launched: a NULL ctx / gp / stats / d_cells, a NULL d_records with n > 0,
 *   a misaligned d_records / d_cells, n >= 2^31, and any parameter outside the ranges stated at suma_grid_params.
 * suma_world_grid_fit: sets gp's origin, width and height (cell_size is read) to the raster that holds every record whose
 *   x, y and z are finite, with margin_cells (<= 2^20) empty cells around it:
 *   origin_a = (floorf(min_a / cell_size) - margin_cells) * cell_size,
 *   width = (uint)(floorf(max_x / cell_size) - floorf(min_x / cell_size)) + 1 + 2 * margin_cells, height likewise.
 *   (A record within an ulp of a cell edge may fall into the neighbouring cell when the grid divides (x - origin_x): a
 *   margin of one cell keeps every record inside.)  SUMA_ERR_CAPACITY, gp untouched, when width, height or
 *   width * height would exceed 2^26; SUMA_ERR_INVALID when no record is finite.
 * suma_world_grid: d_cells = width * height cells, row-major, row = y (cell (ix, iy) at iy * width + ix); every cell is
 *   written.  Two calls on the same input give the same bytes.
 *   Scratch, kept by the ctx and grown by its one rule: 48 bytes per record (a 16-byte member record and the double
 *   buffers of the two sorts: keys 2 x 8, labels 2 x 4, indices 2 x 4; it is the block suma_map_export_world's voxel mode
 *   uses, as are the sorts' histograms) and 16 bytes per cell (the cell's run in the sorted records, its ground count
 *   and ground height). */
int suma_world_grid_fit(suma_ctx* ctx, const suma_world_surfel* d_records, uint32_t n, uint32_t margin_cells,
                        suma_grid_params* gp);
int suma_world_grid(suma_ctx* ctx, const suma_grid_params* gp, const suma_world_surfel* d_records, uint32_t n,
                    suma_grid_cell* d_cells, suma_grid_stats* stats);

/* ---- planning on the traversability grid: per cell the clearance to the nearest blocked cell, whether a robot of a given
 *      radius may stand there, the cost-to-go to a set of goal cells and the direction of the cheapest way, and paths read
 *      off that field (k_plan.hip states the specification; tests/plan_shim.c restates it on the host, and the field and the
 *      paths equal it byte for byte).  Every quantity is an integer or one fp32 comparison. */
#define SUMA_PLAN_MAX_CLEAR_CELLS 64u
#define SUMA_PLAN_MAX_GOALS 4096u
#define SUMA_PLAN_MAX_STARTS 4096u
#define SUMA_PLAN_UNREACHED 0xffffffffu /* the cost of a cell no goal is reached from */

typedef struct suma_plan_params {
  float robot_radius;       /* metres; default 0.4; finite, 0 <= robot_radius <= max_clear_cells * cell_size */
  float max_step;           /* default 0.15: a move needs |ground_z(c) - ground_z(n)| <= max_step; not NaN */
  float max_rough;          /* default NaN = off: a cell with ground_rough > max_rough is blocked */
  uint32_t unknown_blocked; /* default 1; 0 or 1: an UNKNOWN cell is blocked */
  uint32_t max_clear_cells; /* R, default 16; 1 .. 64: the clearance is exact below (R + 1)^2 and capped there */
  uint32_t soft_cells;      /* default 3; 0 .. R + 1: cells nearer than this to a blocked cell cost more */
  uint32_t soft_weight;     /* default 2; 0 .. 255: by this much per cell of missing distance */
  uint8_t label_cost[SUMA_DRAW_COLORS]; /* default all 1: the cost of standing on a label; 0 = forbidden (blocked) */
} suma_plan_params;

/* direction k of a move, as (dx, dy); the row index grows with y:
 *   0 E (1, 0), 1 NE (1, 1), 2 N (0, 1), 3 NW (-1, 1), 4 W (-1, 0), 5 SW (-1, -1), 6 S (0, -1), 7 SE (1, -1) */
enum { SUMA_PLAN_E = 0, SUMA_PLAN_NE, SUMA_PLAN_N, SUMA_PLAN_NW, SUMA_PLAN_W, SUMA_PLAN_SW, SUMA_PLAN_S, SUMA_PLAN_SE,
       SUMA_PLAN_AT_GOAL = 8, SUMA_PLAN_NO_DIRECTION = 255 };
enum { SUMA_PLAN_BLOCKED = 1, SUMA_PLAN_TRAVERSABLE = 2, SUMA_PLAN_REACHED = 4 }; /* bits of suma_plan_cell.flags */

typedef struct suma_plan_cell { /* 8 bytes */
  uint32_t cost;   /* cost-to-go to the nearest goal; SUMA_PLAN_UNREACHED */
  uint16_t clear2; /* squared distance in cells to the nearest blocked cell, capped at (R + 1)^2; 0 on a blocked cell */
  uint8_t flags;   /* SUMA_PLAN_BLOCKED | SUMA_PLAN_TRAVERSABLE | SUMA_PLAN_REACHED */
  uint8_t next;    /* the direction of the cheapest move; 8 at a goal, 255 where unreached */
} suma_plan_cell;

typedef struct suma_plan_stats {
  uint32_t n_blocked, n_traversable, n_reached;
  uint32_t n_goals, n_goals_ignored; /* goal entries given / of these not traversable (a cell given twice counts twice) */
  uint32_t max_cost;                 /* the largest finite cost; 0 when nothing is reached */
  uint32_t n_rounds;                 /* diagnostic: relaxation rounds launched until one changed nothing */
} suma_plan_stats;

enum { SUMA_PATH_OK = 0, SUMA_PATH_UNREACHED = 1, SUMA_PATH_START_OUTSIDE = 2, SUMA_PATH_TRUNCATED = 3, SUMA_PATH_BAD_FIELD = 4 };

typedef struct suma_plan_path { /* 16 bytes: the result for one start */
  uint32_t length; /* cells on the path, the start and the goal included (the full length, also when TRUNCATED);
                      0 for UNREACHED / START_OUTSIDE; for BAD_FIELD the cells visited before the bad step */
  uint32_t status; /* SUMA_PATH_* */
  uint32_t cost;   /* the field's cost at the start; SUMA_PLAN_UNREACHED for START_OUTSIDE */
  uint32_t pad;    /* 0 */
} suma_plan_path;

/* the defaults above */
void suma_plan_params_default(suma_plan_params* pp);
/* Host only: the cell of a world position in the grid's own fp32 expression, iy * width + ix with
 *   ix = floorf((x - origin_x) / cell_size), iy likewise; -1 outside the raster, for a non-finite x or y, and for a NULL gp.
 *   How a goal or a start given in world coordinates becomes a cell. */
int64_t suma_grid_cell_index(const suma_grid_params* gp, float x, float y);
/* Both entries run on the ctx stream, use scratch of the ctx grown by its one rule, and write only that scratch and the
 *   caller's output: the grid cells, the map and every counter of the ctx stay as they are.  Of gp only width, height and
 *   cell_size are read (the ranges of suma_world_grid).  SUMA_ERR_INVALID with a message, and nothing launched or written:
 *   a NULL argument, a misaligned device pointer (d_cells 16 bytes, d_field 8), a count of 0 or above 4096, and any
 *   parameter outside the ranges stated at suma_plan_params.
 * suma_grid_plan_field: d_cells = the width * height cells suma_world_grid wrote (device); goals = n_goals cell indices on
 *   the host, each 0 <= g < width * height (SUMA_ERR_INVALID otherwise); a goal that is not traversable is ignored and
 *   counted.  d_field = width * height suma_plan_cell (device), row-major like the grid; every cell is written.
 *   SUMA_ERR_CAPACITY when width * height * 28 * (255 + soft_weight * soft_cells) >= 2^32: a cost could wrap.
 *   Blocks once per batch of relaxation rounds, for one word.  Scratch: 21 bytes a cell.
 * suma_grid_plan_paths: d_field = a field (device; the walk does not trust it); starts = n_starts cell indices on the
 *   host (a negative one, or one beyond the raster: START_OUTSIDE); path_capacity = 1 .. 2^20 cells per path, n_starts *
 *   path_capacity <= 2^26.  path_cells (host) = n_starts rows of path_capacity cell indices, the start first; entries
 *   behind min(length, path_capacity) are 0xffffffff.  results (host) = n_starts records.  The paths are made in scratch
 *   of the ctx and come back with one blocking read. */
int suma_grid_plan_field(suma_ctx* ctx, const suma_grid_params* gp, const suma_plan_params* pp, const suma_grid_cell* d_cells,
                         const int64_t* goals, uint32_t n_goals, suma_plan_cell* d_field, suma_plan_stats* stats);
int suma_grid_plan_paths(suma_ctx* ctx, const suma_grid_params* gp, const suma_plan_cell* d_field, const int64_t* starts,
                         uint32_t n_starts, uint32_t path_capacity, uint32_t* path_cells, suma_plan_path* results);

/* ---- device scratch for callers that keep scans resident in HBM (bench, replay) */
int suma_device_alloc(suma_ctx* ctx, uint64_t bytes, void** d_ptr);
int suma_device_free(suma_ctx* ctx, void* d_ptr);
int suma_device_upload(suma_ctx* ctx, void* d_dst, const void* host_src, uint64_t bytes);
int suma_device_download(suma_ctx* ctx, void* host_dst, const void* d_src, uint64_t bytes);

/* ---- pose graph (Posegraph, src/core/Posegraph.cpp): the optimiser between addEdge and integrateLoopClosures ----
 * A PriorFactor on the first node (identity, information 1e6 I) plus BetweenFactor<Pose3> edges with Gaussian
 * information, optimised by Levenberg-Marquardt in fp64 on the device (k_posegraph.hip; the mathematics is DESIGN.md
 * "Pose graph").  A graph is its own handle with its own HIP stream on `hip_device` (not a suma_ctx), so one host
 * thread may optimise it while another drives a pipeline on the same device (SurfelMapping.cpp:658 runs it under
 * std::async).  Calls on one graph are serialised by the caller; the entries that launch make the graph's device the
 * calling thread's current device.  Errors: the library's codes, text in suma_posegraph_last_error(graph) (NULL: the
 * last failed create).  Matrices are column-major: poses double[16], information double[36] in gtsam's tangent order
 * [omega, v] (rotation first).  Only the top 3 x 4 of a pose is read.  Non-finite input is SUMA_ERR_INVALID. */
typedef struct suma_posegraph suma_posegraph;

/* gtsam's LevenbergMarquardtParams defaults (suma_posegraph_default_params) and the inner CG solver's settings */
typedef struct suma_posegraph_params {
  double lambda_initial;     /* 1e-5 */
  double lambda_factor;      /* 10: lambda * factor on a rejected step, / factor on an accepted one */
  double lambda_upper_bound; /* 1e5: give up once lambda reaches it */
  double lambda_lower_bound; /* 0 */
  double min_model_fidelity; /* 1e-3: accept when (actual decrease) / (linearised decrease) exceeds it */
  double relative_error_tol; /* 1e-5 */
  double absolute_error_tol; /* 1e-5 */
  double error_tol;          /* 0 */
  double cg_tolerance;       /* 1e-10: stop CG when sqrt(r'M^-1 r / r0'M^-1 r0) <= this */
  uint32_t cg_max_iterations; /* 1000 per damped solve */
  uint32_t reserved;
} suma_posegraph_params;

enum {
  SUMA_PG_MAX_ITERATIONS = 0, /* max_iterations reached (also: max_iterations == 0) */
  SUMA_PG_CONVERGED = 1,      /* relative or absolute error decrease at or below its tolerance */
  SUMA_PG_LAMBDA_BOUND = 2,   /* no acceptable step below lambda_upper_bound */
  SUMA_PG_ERROR_TOL = 3       /* error at or below error_tol */
};

typedef struct suma_posegraph_stats {
  uint32_t iterations;    /* LM iterations (linearisations) */
  uint32_t termination;   /* SUMA_PG_* */
  uint32_t cg_iterations; /* CG iterations summed over all damped solves */
  uint32_t linear_solves; /* damped solves (accepted + rejected steps) */
  double lambda;          /* final lambda */
  double initial_error, final_error;
} suma_posegraph_stats;

void suma_posegraph_default_params(suma_posegraph_params* p);
const char* suma_posegraph_last_error(const suma_posegraph* g);
int suma_posegraph_create(int hip_device, uint32_t node_capacity, uint32_t edge_capacity, suma_posegraph** out);
void suma_posegraph_destroy(suma_posegraph* g);
int suma_posegraph_clear(suma_posegraph* g);                               /* Posegraph::clear */
int suma_posegraph_clone(const suma_posegraph* g, suma_posegraph** out);   /* Posegraph::clone (:20-22) */
/* Posegraph::setInitial (:25-46): sets the initial estimate AND the current result of node id; the first node also
 * gets the prior.  Ids are dense: id == size appends (SUMA_ERR_CAPACITY beyond node_capacity), id < size updates. */
int suma_posegraph_set_initial(suma_posegraph* g, int32_t id, const double T[16]);
/* Posegraph::addEdge (:48-59): measurement Z of Xfrom^-1 Xto; from != to, both < size; either direction.  The
 * information matrix is symmetrised, (I + I^T) / 2.  SUMA_ERR_CAPACITY beyond edge_capacity. */
int suma_posegraph_add_edge(suma_posegraph* g, int32_t from, int32_t to, const double Z[16], const double information[36]);
int suma_posegraph_pose(const suma_posegraph* g, int32_t id, double T[16]);  /* Posegraph::pose */
/* Posegraph::poses: *n = size; SUMA_ERR_CAPACITY (nothing written) when capacity < size */
int suma_posegraph_poses(const suma_posegraph* g, double* poses16, uint32_t capacity, uint32_t* n);
int32_t suma_posegraph_size(const suma_posegraph* g);                        /* Posegraph::size */
uint32_t suma_posegraph_edge_count(const suma_posegraph* g);
int suma_posegraph_error(suma_posegraph* g, double* error);                  /* Posegraph::error: 0.5 sum e' I e */
int suma_posegraph_reinitialize(suma_posegraph* g);                          /* Posegraph::reinitialize */
/* Posegraph::optimize (:92-104): blocking; params NULL = the defaults.  The result replaces the current poses. */
int suma_posegraph_optimize(suma_posegraph* g, uint32_t max_iterations, const suma_posegraph_params* params,
                            suma_posegraph_stats* stats);
/* the linear system at the current poses, as the optimiser builds it (for tests): factor_errors 6 per factor (factor 0
 * the prior, then the edges in insertion order), gradient 6 per node, diag_blocks 36 per node, band_blocks 36 per
 * node i < size - 1 (block (i, i+1)), off_blocks / off_pairs the blocks (a, b), a < b, b > a + 1, in order of the
 * first edge between a and b.  Any output may be NULL. */
int suma_posegraph_linearize(suma_posegraph* g, double* factor_errors, double* gradient, double* diag_blocks,
                             double* band_blocks, double* off_blocks, int32_t* off_pairs, uint32_t off_capacity,
                             uint32_t* n_off);

/* a graph's capacities raised to at least these (they never shrink).  Capacities are limits on the host record only: the
 * device blocks are sized by the graph itself and double when it outgrows them. */
int suma_posegraph_reserve(suma_posegraph* g, uint32_t node_capacity, uint32_t edge_capacity);
/* edge `index` in insertion order (Posegraph::save walks them): any output may be NULL; information as it is stored,
 * symmetrised */
int suma_posegraph_edge(const suma_posegraph* g, uint32_t index, int32_t* from, int32_t* to, double Z[16],
                        double information[36]);

/* ---- loop closing inside the scan pipeline: SurfelMapping::checkLoopClosure and the pose-graph bookkeeping around it
 *      (SurfelMapping.cpp:42-60, :212-253, :461-471, :478-518, :527-795, :819-826), opt-in.  Once enabled, the pipeline
 *      owns a suma_posegraph: every scan appends its node and odometry edge (updatePose, :461-471), begin_scan* first
 *      integrates a finished optimisation (integrateLoopClosures, :179), and the whole-scan entries run
 *      checkLoopClosure between updatePose and updateMap (:196).  Hosts on the phase calls place
 *      suma_pipeline_check_loop_closure there themselves.  The state machine is the reference's statement for
 *      statement (DESIGN.md 9 lists the quirks that are kept); its host-side 4x4 products and rigid inverses use the
 *      library's one fixed operation order.  (Kept here, not in suma_types.h, for the reason given at
 *      suma_semantic_params.) */
typedef struct suma_loop_params {
  float residual_threshold;      /* loop-residual-threshold, 1.05 (SurfelMapping.h:225) */
  float outlier_threshold;       /* loop-outlier-threshold, 1.1 */
  float valid_threshold;         /* loop-valid-threshold, 0.9 */
  float search_distance;         /* loop-search-distance, 20 */
  float min_trajectory_distance; /* loop-min-trajectory-distance, 200 */
  int32_t min_verifications;     /* loop-min-verifications, 3 */
  int32_t delta_timestamp;       /* loopDetlaTimestamp_, 100 */
  int32_t optimize_wait;         /* 1: an optimisation started in scan k is waited for and integrated at the start of scan
                                    k + 1 + integrate_lag (deterministic); 0: the reference's polling -- integrated at the
                                    first scan start that finds it finished, no wait, integrate_lag ignored */
  /* the gates the reference writes as literals (:567, :713): 0.2, 0.85, 0.1 */
  double min_valid_ratio, max_outlier_ratio, max_increment_difference;
  double information[36];        /* info_ of every edge (:49-59), column-major, gtsam order [omega, v]; identity */
  uint32_t optimize_iterations;  /* Posegraph::optimize(100), :825 */
  uint32_t integrate_lag;        /* 0 */
  uint32_t node_capacity;        /* initial capacity of the pipeline's graph (it grows by doubling), 1024 */
  uint32_t reserved;
} suma_loop_params;

/* what one scan's loop closing did; the persistent members are the values after the scan's last loop-closing step */
typedef struct suma_loop_status {
  int32_t found_candidate;  /* foundLoopClosureCandidate_ */
  int32_t use_candidate;    /* useLoopClosureCandidate_ */
  int32_t candidate_to;     /* `to` of the candidate this scan queued, -1: none */
  uint32_t n_unverified;    /* unverifiedLoopClosures_.size() */
  int32_t already_verified; /* alreadyVerifiedLoopClosure_ */
  int32_t loop_count;       /* loopCount_ */
  uint32_t time_without_loop_closure;
  int32_t currently_optimizing;
  int32_t started_optimization; /* this scan cloned the graph and started the optimiser (:655-660) */
  int32_t integrated;           /* this scan's start integrated an optimised graph (:212-253) */
  uint32_t edges_added;         /* loop edges added by this scan (:649) */
  float result_old_outlier_ratio;
  suma_icp_stats result_old;    /* result_old_: error, inlier_residual (already divided by inlier, :583 / :747), counters;
                                   iterations / converged unused */
  double result_old_residual;
  float loop_valid_ratio, loop_outlier_ratio, loop_relative_error_all; /* :784-786 */
  float reserved;
  double posegraph_error;       /* posegraph_->error(), :793 */
} suma_loop_status;

void suma_loop_params_default(suma_loop_params* p);
/* NULL switches loop closing off (and frees the graph).  Only between scans; a running optimisation is joined first.
 * Enabling (again) starts from the constructor's state: node 0 at identity (:43), no candidates; the graph's
 * later nodes are numbered by the pipeline's timestamp, so enable it before the first scan or after a reset. */
int suma_pipeline_enable_loop_closing(suma_pipeline* s, const suma_loop_params* params);
/* checkLoopClosure (:527-795): between suma_pipeline_update_pose and suma_pipeline_update_map, once per scan; does
 * nothing at timestamp 0 (:190) */
int suma_pipeline_check_loop_closure(suma_pipeline* s);
int suma_pipeline_loop_status(const suma_pipeline* s, suma_loop_status* out);
/* the pipeline's graph, borrowed (NULL when loop closing is off): read it with suma_posegraph_pose / _poses / _edge
 * between scans; getOptimizedPoses() = suma_posegraph_poses */
suma_posegraph* suma_pipeline_posegraph(suma_pipeline* s);
/* trajectory_distances_ (:461-471, :242-250): *n = entries, min(*n, capacity) copied */
int suma_pipeline_trajectory_distances(const suma_pipeline* s, float* out, uint32_t capacity, uint32_t* n);
/* getCandidateIndexes / getClosestIndex (:478-518) as a pure host function: j runs down from timestamp -
 * delta_timestamp, distance = float(|t(current_pose) - t(poses16[j])|), strict <, and trajectory_distances[timestamp] -
 * trajectory_distances[j] > min_trajectory_distance.  poses16: column-major 4x4 doubles, only the translation is read.
 * Returns the index or -1. */
int32_t suma_loop_find_candidate(const double* poses16, const float* trajectory_distances, uint32_t timestamp,
                                 const double current_pose[16], float radius, float min_trajectory_distance,
                                 int32_t delta_timestamp);

/* ---- checkpoint / resume of a whole pipeline: one canonical byte image of the logical state between two scans -- map,
 *      parked tiles, pose table, the pipeline's poses and last frame, loop-closing state, pose graph, an optimisation in
 *      flight -- such that a pipeline that loads it continues as the uninterrupted run does, to the bit (DESIGN.md 11;
 *      csrc/k_checkpoint.hip states the image, csrc/checkpoint_format.h the container).  The reference has nothing like
 *      it: Posegraph::save / load are empty stubs (Posegraph.cpp) and its tile cache lives in host RAM only.
 *      The surfel sections are packed and digested on the device (kc_pack), verified there before a load writes
 *      anything (kc_verify), and unpacked into a compact arena (kc_unpack).  All entries are blocking and run on the ctx
 *      stream; none is on the scan path.  The staged image (a device block as large as the largest image saved or
 *      loaded so far) stays allocated for the next save and is given back only when the ctx is destroyed
 *      (suma_pipeline_destroy); suma_pipeline_reset keeps it.  A process that saves once and needs the memory back
 *      has no entry for that.
 *      (Kept here, not in suma_types.h, for the reason given at suma_semantic_params.) */
#define SUMA_CHECKPOINT_VERSION 1u
#define SUMA_CHECKPOINT_MAX_SECTIONS 16
enum { /* section ids, in image order */
  SUMA_CKPT_PARAMS = 1, SUMA_CKPT_PIPELINE, SUMA_CKPT_MAP_STATE, SUMA_CKPT_POSES, SUMA_CKPT_ACTIVE, SUMA_CKPT_FRAME,
  SUMA_CKPT_TILE_DIR, SUMA_CKPT_TILES, SUMA_CKPT_LOOP, SUMA_CKPT_GRAPH, SUMA_CKPT_OPT
};
typedef struct suma_checkpoint_section {
  uint32_t id, reserved;
  uint64_t bytes;  /* payload bytes, without the padding to 64 */
  uint64_t digest; /* as the directory states it */
} suma_checkpoint_section;
/* a struct tag only (no typedef): the entry that fills it has the same name */
struct suma_checkpoint_info {
  uint32_t version;
  uint32_t timestamp;  /* scans processed */
  uint32_t n_active;   /* records of the active map */
  uint32_t n_tiles;    /* non-empty parked tiles */
  uint64_t n_parked;   /* their records */
  uint32_t n_nodes, n_edges; /* pose graph; 0 without LOOP */
  int32_t has_loop, has_opt;
  uint32_t n_sections, reserved;
  uint64_t total_bytes;
  suma_checkpoint_section sections[SUMA_CHECKPOINT_MAX_SECTIONS];
};
/* the size the image would have now.  Only between scans (SUMA_ERR_INVALID otherwise, as the save). */
int suma_pipeline_checkpoint_size(suma_pipeline* s, uint64_t* bytes);
/* writes the image to host_dst; *written = its size.  SUMA_ERR_INVALID between suma_pipeline_begin_scan and
 * suma_pipeline_update_map, or while a scan staged with suma_pipeline_prefetch_scan is pending; SUMA_ERR_CAPACITY with
 * the needed size in *written when capacity is too small (nothing is written; capacity 0 is a size query), or when the
 * map has overflowed one of its capacities.  Resolves a pending statistics record and joins a running pose-graph
 * optimisation; changes nothing else: a pipeline that saves computes what one that never does computes.  A save refused
 * with SUMA_ERR_INVALID has not joined the optimisation; one refused with SUMA_ERR_CAPACITY has, as the size it reports
 * needs the optimisation's result to be final. */
int suma_pipeline_checkpoint_save(suma_pipeline* s, void* host_dst, uint64_t capacity, uint64_t* written);
/* replaces the state of s by the image's.  The image is parsed and bounds-checked on the host, then staged and its
 * section digests verified on the device, BEFORE anything of the pipeline is written: a refused load leaves the pipeline
 * exactly as it was.  SUMA_ERR_INVALID: wrong phase, malformed image, unsupported version, digest mismatch (the message
 * names the section), parameters that differ from the pipeline's (the message names the first such field);
 * SUMA_ERR_CAPACITY: n_active > max_surfels, parked records beyond the arena, more tiles than slots, timestamp >
 * max_poses.  A successful load joins and drops a running optimisation, drains the ingest, resets what
 * suma_pipeline_reset resets, installs the state, clears every de-duplication cache, and switches loop closing on with
 * the stored parameters if the image has a LOOP section, off if not (a graph handle borrowed before is dead). */
int suma_pipeline_checkpoint_load(suma_pipeline* s, const void* image, uint64_t bytes);
/* host only, no device: parses an image (the same checks as the load's first step) and reports what it holds; on failure
 * the text is suma_last_error(NULL) */
int suma_checkpoint_info(const void* image, uint64_t bytes, struct suma_checkpoint_info* out);
/* the PARAMS section of a valid image (suma_pipeline_create with them gives a pipeline that can load it) */
int suma_checkpoint_params(const void* image, uint64_t bytes, suma_params* out);
/* host only: the digest of a payload read as little-endian 64-bit words w[k], a shorter tail zero-extended:
 * sum over k of (w[k] + 0x9E3779B97F4A7C15) * (2 k + 1) mod 2^64 */
uint64_t suma_checkpoint_digest(const void* payload, uint64_t bytes);

/* ---- localisation in a finished map: "here is yesterday's map (suma_map_export_world / mapio), tell me where the sensor
 *      is in it, and leave the map alone".  The reference has no such mode; its nearest relative is the loop-closure
 *      verification, which renders the inactive map from a pose and minimises against it -- and that is what one scan
 *      does here.  A localiser owns a suma_ctx of its own.  It keeps the world records on the device, binned into the
 *      reference's submap tiles, and fills that ctx's active surfel buffer with the tiles around the sensor
 *      (csrc/k_localize.hip states the specification; tests/localize_shim.c restates it on the host).  The window's
 *      surfels have creation stamp 0 and row 0 of the ctx's pose table is the identity, so the world frame is their
 *      creation frame; the ctx's timestamp is the constant T_loc = active_timestamps + 10.  Nothing is ever fused: the
 *      map, the pose table and the world records are not written, and a run has no length limit (max_poses is not
 *      consumed).  DESIGN.md 12 has the step order and its limit: a window smaller than the model image's range
 *      localises on what it has.  The start pose is the caller's (suma_localizer_set_pose), or comes from place
 *      recognition against the mapping session's scans (suma_localizer_relocalize, below).
 *      Calls on one localiser are serialised by the caller.  Errors: the library's codes; the text is
 *      suma_last_error(suma_localizer_ctx(l)), or suma_last_error(NULL) after a failed create.
 *      (Kept here, not in suma_types.h, for the reason given at suma_semantic_params.) */
typedef struct suma_localizer suma_localizer;
typedef struct suma_localizer_params {
  float conf_threshold;        /* render threshold; default suma_params.confidence_threshold */
  float min_valid_ratio;       /* default 0.2  (the reference's closure gate literals, */
  float max_outlier_ratio;     /* default 0.85  SurfelMapping.cpp:567) */
  int32_t constant_velocity;   /* default 1: guess = pose * last_increment; 0: guess = pose */
} suma_localizer_params;
typedef struct suma_localizer_result {
  double guess[16], pose[16], increment[16];
  suma_icp_stats stats;        /* the objective as the minimisation left it */
  float valid_ratio, outlier_ratio;   /* as closure_gate forms them: valid / (valid + invalid), outlier / (outlier +
                                         inlier) in fp32; 0 / 0 = NaN, which passes no gate */
  int32_t tracked;             /* both gates passed */
  int32_t window_rebuilt;      /* this scan moved the window's origin and gathered the window again */
  int32_t origin_ij[2];
  uint32_t n_window;
} suma_localizer_result;

/* conf_threshold = params->confidence_threshold (0 when params is NULL), 0.2, 0.85, 1 */
void suma_localizer_params_default(const suma_params* params, suma_localizer_params* lp);
/* lp NULL = the defaults.  SUMA_ERR_INVALID: a NaN threshold or ratio, submap_dimension < 0 or > 64, a submap_extent
 * that is not finite and > 0, active_timestamps outside 91 .. 2^31 - 11 (the inactive render selects creation stamps
 * below T_loc - 100, the reference's literal, SurfelMap.cpp:873: with less, no record of the window would render) */
int suma_localizer_create(const suma_params* params, const suma_localizer_params* lp, int hip_device, suma_localizer** out);
void suma_localizer_destroy(suma_localizer* l);
/* the localiser's own ctx, borrowed: frames (suma_map_frame(ctx, SUMA_FRAME_OLD) is the rendered model), profiling,
 * the stream, the error text.  Do not update or upload its map. */
suma_ctx* suma_localizer_ctx(suma_localizer* l);
/* the map: n records as suma_map_export_world / mapio give them.  Binned once (a key per record, one stable sort, a tile
 * directory that is read back); blocking, off the scan path.  *n_dropped (optional) = records with a non-finite position
 * or outside the tile grid, which no window will hold.  The localiser keeps its own copy (48 bytes a kept record); the
 * caller's buffer is only read.  n = 0 is legal.  A new map forgets the pose: call suma_localizer_set_pose next. */
int suma_localizer_set_map(suma_localizer* l, const suma_world_surfel* host, uint32_t n, uint32_t* n_dropped);
int suma_localizer_set_map_device(suma_localizer* l, const suma_world_surfel* d_records, uint32_t n, uint32_t* n_dropped);
/* the start pose (sensor in the world frame, column-major): resets the increment to identity, puts the window's origin
 * on the pose's own tile and gathers the window.  SUMA_ERR_CAPACITY when the window holds more than max_surfels
 * records: detected on the host before anything is launched, the localiser is left exactly as it was. */
int suma_localizer_set_pose(suma_localizer* l, const double T[16]);
/* one scan (points / labels / probs as suma_preprocess takes them).  fixed_iterations has the pipeline's meaning.
 * SUMA_ERR_INVALID before suma_localizer_set_map / _set_pose, or with a NULL result.  An empty window is legal: nothing is
 * minimised, stats are zero, tracked = 0, pose = guess and the increment stays; the same holds for a chain that ends on
 * a non-finite pose.
 * The pose is kept orthonormal (Gram-Schmidt on the rotation's columns after every scan): the increment is formed with
 * the rigid inverse, which is the inverse of an orthonormal rotation only.
 * The _device entry reads scan buffers that must be complete when the call is made (suma_preprocess_device). */
int suma_localizer_process_scan(suma_localizer* l, const suma_float4* points, const float* labels, const float* probs,
                                uint32_t n, int32_t fixed_iterations, suma_localizer_result* result);
int suma_localizer_process_scan_device(suma_localizer* l, const suma_float4* d_points, const float* d_labels,
                                       const float* d_probs, uint32_t n, int32_t fixed_iterations,
                                       suma_localizer_result* result);
/* the window now: origin tile, records, and how often it has been gathered since the last suma_localizer_set_map
 * (suma_localizer_set_pose counts).  Any output may be NULL. */
int suma_localizer_window(suma_localizer* l, int32_t origin_ij[2], uint32_t* n_window, uint32_t* rebuilds);
/* the window's surfels as the ctx holds them: *n = their number, min(*n, capacity) are copied */
int suma_localizer_download_window(suma_localizer* l, suma_surfel* host, uint32_t capacity, uint32_t* n);

/* ---- map maintenance, first step: "which records of yesterday's map are still true?"  While a localiser tracks, each
 *      record of the world map collects evidence from the scans that look at it: confirmed (a return on it: hit), seen
 *      through (a return well behind it: miss) or hidden (a return well in front of it: occluded).  The map is still not
 *      written: the evidence is an array of its own, it comes back in the order of the records suma_localizer_set_map was
 *      given, and suma_change_prune_mask turns it into the records to keep.  csrc/k_change.hip states the fp32
 *      specification, tests/change_shim.c restates it; DESIGN.md 14 has the scenario it was measured on and what is out
 *      of scope (removing records from the live window, evidence in checkpoints).  Evidence is off
 *      unless switched on, and with it on every result of the localiser is bit-identical to a run with it off. */
typedef struct suma_change_params {
  float free_margin;     /* default 0.5 m: how much farther than the record a return must lie before the record counts
                            as seen through (and how much nearer before it counts as hidden); finite, > 0 */
  float min_view_cos;    /* default 0.3: a record seen at a grazing angle collects no miss; finite, in [0, 1) */
  float max_range;       /* default 50 m: records farther than this collect nothing; finite, > 0 */
  int32_t tracked_only;  /* default 1: a scan whose tracked == 0 adds nothing */
} suma_change_params;
typedef struct suma_change_evidence {
  uint32_t hits, misses, occluded, label_changes; /* label_changes: hits whose measured label differs from the record's */
} suma_change_evidence;
/* what one observation did with the records of the window; unseen + no_return + occluded + misses + grazing + hits +
 * near = n_window */
typedef struct suma_change_counts {
  uint32_t n_window, unseen, no_return, occluded, misses, grazing, hits, near, label_changes;
} suma_change_counts;
typedef struct suma_change_rule {
  uint32_t min_misses;   /* default 3 */
  float miss_ratio;      /* default 2.0f */
} suma_change_rule;
/* 0.5f, 0.3f, 50.0f, 1 */
void suma_change_params_default(suma_change_params* cp);
/* 3, 2.0f */
void suma_change_rule_default(suma_change_rule* rule);
/* switches evidence on (cp NULL = the defaults).  SUMA_ERR_INVALID with a message for values outside the ranges above.
 * It takes effect with the next suma_localizer_set_map, which allocates and zeroes the evidence (16 bytes a kept record)
 * and keeps the sort's source index (4 bytes a kept record); until then the evidence entries below are SUMA_ERR_INVALID.
 * Enabling again only replaces the parameters. */
int suma_localizer_enable_evidence(suma_localizer* l, const suma_change_params* cp);
/* switches it off and gives the evidence and the source index back */
int suma_localizer_disable_evidence(suma_localizer* l);
/* the primitive: one observation of a frame of the localiser's ctx (data image size) at the sensor pose T (column-major,
 * world frame, finite) over the current window, on the ctx stream behind the work that made the frame; *counts
 * (optional) = its totals.  It is what a host with poses from elsewhere calls.  An empty window observes nothing. */
int suma_localizer_observe_frame(suma_localizer* l, const suma_frame* frame, const double T[16], suma_change_counts* counts);
/* With evidence on, suma_localizer_process_scan(_device) ends with one observation of the scan's own frame at the final
 * pose, unless the window is empty or tracked_only && !tracked; suma_localizer_relocalize observes nothing (its
 * candidates are hypotheses).  This returns the last scan's totals and whether it observed (both optional). */
int suma_localizer_last_observation(suma_localizer* l, suma_change_counts* counts, int32_t* observed);
/* the evidence in the order of suma_localizer_set_map's records: *n = that call's n (dropped records included, which
 * stay zero), min(*n, capacity) are copied (suma_map_download's convention).  Blocking. */
int suma_localizer_evidence(suma_localizer* l, suma_change_evidence* host, uint32_t capacity, uint32_t* n);
int suma_localizer_evidence_device(suma_localizer* l, suma_change_evidence* d_out, uint32_t capacity, uint32_t* n);
/* back to zero; a new suma_localizer_set_map clears too */
int suma_localizer_clear_evidence(suma_localizer* l);
/* host only, no device -- the rule's one home for C, C++ and Python hosts: keep[k] = 0 iff misses >= min_misses &&
 * (float)misses > miss_ratio * (float)hits (rule NULL = the defaults; a NaN ratio removes nothing); *n_removed
 * (optional) = the zeros.  SUMA_ERR_INVALID for NULL arrays with n > 0; the text is suma_last_error(NULL). */
int suma_change_prune_mask(const suma_change_evidence* evidence, uint32_t n, const suma_change_rule* rule, uint8_t* keep,
                           uint32_t* n_removed);

/* ---- map maintenance, second step: "what is there today that yesterday's map does not have?"  While a localiser
 *      tracks, the texels of each scan that no record of the window explains are collected on the device as world-frame
 *      candidate surfels; on request they are fused per voxel and kept where several scans agree.  The fused records
 *      concatenate with the records the prune rule keeps into the updated map, which goes into the next
 *      suma_localizer_set_map, a file or a picture.  The map is still not written.  csrc/k_novel.hip states the fp32
 *      specification, tests/novel_shim.c restates it; DESIGN.md 15 has the scenario and what is out of scope (candidates
 *      in checkpoints, inserting into the live window, free-space checks of old candidates).  Novelty is off unless
 *      switched on, and with it on every other output of the localiser is bit-identical to a run with it off. */
typedef struct suma_novel_params {
  float agree_margin;      /* default 0.5 m: a record explains a texel whose range differs by no more; finite, > 0 */
  float max_range;         /* default 50 m: texels with range + agree_margin >= this collect nothing; finite, > 0 */
  int32_t tracked_only;    /* default 1: a scan whose tracked == 0 collects nothing */
  uint32_t max_candidates; /* default 4 194 304 (48 bytes each, 201 MB, allocated by the enable); 1 .. 2^30 */
} suma_novel_params;
typedef struct suma_novel_fuse_params {
  float voxel_size;        /* default 0.2 m; finite, > 0 */
  uint32_t min_views;      /* default 2: distinct scans (timestamps) that must have put a candidate into the voxel; >= 1 */
  float confidence;        /* default confidence_threshold + 1.0f: the localiser renders only records with confidence >
                              conf_threshold, so a new record at the mapping prior (log_prior, what a candidate carries)
                              would never be matched against; not NaN */
} suma_novel_fuse_params;
/* what one collection did with the texels of the frame; no_return + out_of_range + grazing + explained + novel =
 * n_texels; stored = the novel ones that fitted into the buffer */
typedef struct suma_novel_counts {
  uint32_t n_texels, no_return, out_of_range, grazing, explained, novel, stored;
} suma_novel_counts;
typedef struct suma_novel_stats {
  uint32_t n_candidates;   /* held now */
  uint32_t n_overflow;     /* novel texels that did not fit since the last clear */
  uint32_t n_dropped;      /* candidates outside the voxel grid */
  uint32_t n_voxels;       /* distinct voxels */
  uint32_t n_out;          /* voxels with views >= min_views: the size of the result */
} suma_novel_stats;
/* 0.5f, 50.0f, 1, 4194304 */
void suma_novel_params_default(suma_novel_params* np);
/* 0.2f, 2, params->confidence_threshold + 1.0f (params NULL: 1.0f) */
void suma_novel_fuse_params_default(const suma_params* params, suma_novel_fuse_params* fp);
/* switches novelty on (np NULL = the defaults) and allocates the candidate buffer, the mark image and the flags.
 * SUMA_ERR_INVALID with a message for values outside the ranges above, and nothing launched.  Enabling again replaces
 * the parameters; a different max_candidates clears the candidates. */
int suma_localizer_enable_novelty(suma_localizer* l, const suma_novel_params* np);
/* switches it off and gives the buffers back */
int suma_localizer_disable_novelty(suma_localizer* l);
/* the primitive: one collection of a frame of the localiser's ctx (data image size) at the sensor pose T (column-major,
 * world frame, finite) over the current window, enqueued on the ctx stream; the candidates carry scan_id as their
 * timestamp.  *counts (optional) = its totals, which makes the call blocking.  An empty window collects nothing. */
int suma_localizer_collect_frame(suma_localizer* l, const suma_frame* frame, const double T[16], uint32_t scan_id,
                                 suma_novel_counts* counts);
/* With novelty on, suma_localizer_process_scan(_device) ends with one collection of the scan's own frame at the final
 * pose (behind the observation, when evidence is on too), unless the window is empty, tracked_only && !tracked, or the
 * pose is not finite; its scan_id is the number of process_scan(_device) calls since the last suma_localizer_set_map,
 * counted from 0 whether or not they collected.  The scan path does not wait for it.  suma_localizer_relocalize collects
 * nothing and does not count.  This returns the totals of the last collection -- a scan's or
 * suma_localizer_collect_frame's -- and whether it collected (both optional).  Blocking. */
int suma_localizer_last_collection(suma_localizer* l, suma_novel_counts* counts, int32_t* collected);
/* the candidates in creation order: *n = their number, min(*n, capacity) are copied.  Blocking. */
int suma_localizer_novel_candidates(suma_localizer* l, suma_world_surfel* host, uint32_t capacity, uint32_t* n);
int suma_localizer_novel_candidates_device(suma_localizer* l, suma_world_surfel* d_out, uint32_t capacity, uint32_t* n);
/* replaces the candidates by n records of the caller's (a session's candidates saved by suma_localizer_novel_candidates and
 * taken up again: checkpoints do not hold them).  SUMA_ERR_CAPACITY, nothing changed, when n > max_candidates. */
int suma_localizer_set_novel_candidates(suma_localizer* l, const suma_world_surfel* host, uint32_t n);
/* the fused records in ascending voxel order and their views (fp NULL = the defaults of the localiser's suma_params):
 * stats->n_out = their number, min(n_out, capacity) are written (suma_map_export_world's convention); host / views may
 * be NULL with capacity 0.  Blocking; the candidates stay.  Two calls give the same bytes. */
int suma_localizer_novel(suma_localizer* l, const suma_novel_fuse_params* fp, suma_world_surfel* host, uint32_t* views,
                         uint32_t capacity, suma_novel_stats* stats);
int suma_localizer_novel_device(suma_localizer* l, const suma_novel_fuse_params* fp, suma_world_surfel* d_out,
                                uint32_t* d_views, uint32_t capacity, suma_novel_stats* stats);
/* the mark image of the last collection (one byte a texel of the data image): *n = its size, min(*n, capacity) are copied */
int suma_localizer_novel_marks(suma_localizer* l, uint8_t* host, uint32_t capacity, uint32_t* n);
/* no candidates, n_overflow = 0; a new suma_localizer_set_map clears too and restarts the scan count.
 * _last_collection, _novel_candidates(_device) and _novel(_device) return SUMA_ERR_CAPACITY after filling their outputs
 * when n_overflow > 0 (the downloads' convention). */
int suma_localizer_clear_novelty(suma_localizer* l);

/* ---- objects in front of the robot: "what stands there now that yesterday's map does not contain?"  With novelty on,
 *      every collection ends with a flag byte per texel, 1 = no record of the window explains the return.  With objects
 *      on as well, each collection is followed on the ctx stream by one segmentation of those texels into connected
 *      components of the wrapped range image, and every component of at least min_texels texels is reduced to one
 *      64-byte record: class, box, centroid, nearest range.  The records are those of the LAST segmentation; they are
 *      not accumulated, enter no checkpoint, and neither the grid nor the planner reads them.  csrc/k_objects.hip states
 *      the fp32 specification, tests/object_shim.c restates it; DESIGN.md 19 has the decomposition and what is out of
 *      scope (oriented boxes; tracking across scans and velocities are the tracks block below).  With objects on every
 *      other output of the localiser is bit-identical to a run with them off. */
typedef struct suma_object_params {
  float link_base;       /* default 0.3 m: neighbouring texels this close belong together at any range; finite, >= 0 */
  float link_slope;      /* default 0.03: ... plus this much per metre of the nearer texel's range; finite, >= 0 */
  uint32_t min_texels;   /* default 5: a component of fewer texels is no object; >= 1 */
  uint32_t max_objects;  /* default 4096 (64 bytes each); 1 .. 65 536 */
} suma_object_params;
typedef struct suma_scan_object {
  uint32_t root;         /* the smallest texel index (ty * width + tx) of the object: objects ascend by it */
  uint32_t n_texels;
  uint32_t label;        /* the weighted vote of the members (suma_world_surfel's rule) */
  float prob;
  uint32_t n_dynamic;    /* members whose own label is one of the moving classes */
  float min[3], max[3];  /* the box of the members' world positions */
  float centroid[3];     /* their mean, from integer sums of 1/1024 m */
  float r_min;           /* the smallest range of a member: how near the object is to the sensor */
  uint32_t scan_id;
} suma_scan_object;
/* n_small + n_objects = n_components; stored = min(n_objects, max_objects) */
typedef struct suma_object_counts {
  uint32_t n_texels, n_members, n_components, n_small, n_objects, stored;
} suma_object_counts;
/* 0.3f, 0.03f, 5, 4096 */
void suma_object_params_default(suma_object_params* op);
/* host only, no device: SUMA_OK, or SUMA_ERR_INVALID for values outside the ranges above, the text in
 * suma_last_error(NULL).  suma_localizer_enable_objects applies the same rule. */
int suma_object_params_check(const suma_object_params* op);
/* switches objects on (op NULL = the defaults) and allocates their blocks (about 130 bytes a texel of the data image and
 * 64 bytes an object).  Needs novelty on: SUMA_ERR_INVALID otherwise, and for values outside the ranges above or a data
 * image of more than 2^22 texels, with a message and nothing launched.  Enabling again replaces the parameters and
 * forgets the last segmentation. */
int suma_localizer_enable_objects(suma_localizer* l, const suma_object_params* op);
/* switches them off and gives the blocks back; suma_localizer_disable_novelty does this too */
int suma_localizer_disable_objects(suma_localizer* l);
/* With objects on, every collection -- a scan's own or suma_localizer_collect_frame's -- is followed by one segmentation
 * of that collection's flags, frame, pose and scan_id; it is only enqueued, the scan path does not wait for it.  A scan
 * or a call that collects nothing leaves "no segmentation".  These return the objects of the last segmentation in
 * ascending root order: *n = the objects stored, min(*n, capacity) are copied; *counts and *segmented are optional;
 * without a segmentation *n = 0, the counts are 0 and *segmented = 0.  Blocking.  SUMA_ERR_CAPACITY after filling the
 * outputs when n_objects > max_objects (the downloads' convention). */
int suma_localizer_objects(suma_localizer* l, suma_scan_object* host, uint32_t capacity, uint32_t* n,
                           suma_object_counts* counts, int32_t* segmented);
int suma_localizer_objects_device(suma_localizer* l, suma_scan_object* d_out, uint32_t capacity, uint32_t* n,
                                  suma_object_counts* counts, int32_t* segmented);
/* the id image of the last segmentation, one uint32 a texel of the data image: the object number of a member of a stored
 * object, else 0xffffffff.  *n = its size (0 without a segmentation), min(*n, capacity) are copied.  Blocking. */
int suma_localizer_object_ids(suma_localizer* l, uint32_t* host, uint32_t capacity, uint32_t* n);
/* the flag image of the last collection, one byte a texel of the data image, 1 = novel: what the segmentation behind that
 * collection read (suma_localizer_novel_marks' convention; needs novelty on, not objects).  Blocking. */
int suma_localizer_novel_flags(suma_localizer* l, uint8_t* host, uint32_t capacity, uint32_t* n);
/* the data frame the localiser preprocesses its scans into (K1-K3 of the last suma_localizer_process_scan): what that
 * scan's collection and segmentation read.  Owned by the localiser; NULL for a NULL handle. */
suma_frame* suma_localizer_frame(suma_localizer* l);
/* the primitive on a caller's flag image (host, one byte a texel of the data image) in place of a collection's: one
 * segmentation of a frame of the localiser's ctx at the sensor pose T (column-major, world frame, finite).  It needs no
 * map and no window and touches no candidate.  *counts is optional.  Blocking (the flags are uploaded). */
int suma_localizer_segment_flags(suma_localizer* l, const suma_frame* frame, const double T[16], const uint8_t* host_flags,
                                 uint32_t scan_id, suma_object_counts* counts);

/* ---- live obstacles for the planner: "what stands there now goes into the grid the planner reads".  A live layer holds
 *      16 bytes of state per cell over the raster of a static traversability grid (suma_world_grid's cells).  With the
 *      layer on, every collection -- after its segmentation when objects are on -- is followed on the ctx stream by one
 *      update: the unexplained texels that stand between step_height and clearance above a cell's ground enter a hit into
 *      that cell, and the scan's rays clear the cells they pass through below the top of what was seen there earlier.
 *      Composing gives the static cells with the live obstacles written into them, in the suma_grid_cell layout:
 *      suma_grid_plan_field takes the result unchanged.  csrc/k_live.hip states the specification, tests/live_shim.c
 *      restates it; DESIGN.md 20 has the decomposition and what is out of scope (the layer in checkpoints and during
 *      mapping, exact cell traversal; the objects are tracked by the tracks block below, the layer does not read
 *      them).  The scan path, the candidates, the objects, the grid and the planner keep their results bit for bit. */
typedef struct suma_live_params {
  uint32_t hold_scans;   /* default 10: a hit keeps its cell an obstacle for this many scans; 1 .. 65 535 */
  uint32_t min_hits;     /* default 2: hits in a row (none further apart than hold_scans) before a cell is live; 1 .. 65 535 */
  float carve_range;     /* default 20 m: how far along a ray cells are cleared; finite, >= 0; 0 switches carving off */
  float carve_margin;    /* default 0.5 m: a ray stops clearing this far in front of its return; finite, >= 0 */
} suma_live_params;
/* the raw state of one cell (suma_localizer_live_state): stamp = scan_id + 1 of an update, 0 = never */
typedef struct suma_live_cell {
  uint64_t hit;          /* stamp of the last hit << 32 | the highest hit z of that scan as an ordered integer */
  uint32_t clear;        /* stamp of the last scan a ray cleared the cell in */
  uint32_t hits;         /* hits in a row, saturating at 65 535 */
} suma_live_cell;
/* one update.  n_members = n_outside + n_no_ground + n_low + n_high + n_hit_texels; n_rays = 0 with carving off */
typedef struct suma_live_counts {
  uint32_t n_texels, n_members, n_outside, n_no_ground, n_low, n_high, n_hit_texels, n_hit_cells, n_rays, n_cleared;
} suma_live_counts;
/* one compose: the cells with a hit are live, pending (too few hits yet), carved (a ray cleared them after the hit) or
 * expired (the hit is hold_scans old) */
typedef struct suma_live_stats {
  uint32_t n_live, n_pending, n_expired, n_carved;
} suma_live_stats;
/* 10, 2, 20.0f, 0.5f */
void suma_live_params_default(suma_live_params* lp);
/* host only, no device: SUMA_OK, or SUMA_ERR_INVALID for values outside the ranges above, the text in
 * suma_last_error(NULL).  suma_localizer_enable_live_grid applies the same rule. */
int suma_live_params_check(const suma_live_params* lp);
/* switches the layer on over the raster gp (lp NULL = the defaults).  d_cells: the gp->width * gp->height DEVICE cells
 * suma_world_grid wrote for gp, 16-byte aligned; they may come from another ctx on the same device and are only read: the
 * layer keeps a copy (48 bytes a cell) and allocates and zeroes 20 bytes a cell of state.  Blocking.  Needs novelty on;
 * objects are optional.  SUMA_ERR_INVALID with a message, nothing launched: novelty off, a NULL or misaligned d_cells,
 * gp outside the ranges stated at suma_grid_params, lp outside the ranges above.  Enabling again replaces the layer. */
int suma_localizer_enable_live_grid(suma_localizer* l, const suma_grid_params* gp, const suma_grid_cell* d_cells,
                                    const suma_live_params* lp);
/* switches it off and gives the blocks back; suma_localizer_disable_novelty does this too */
int suma_localizer_disable_live_grid(suma_localizer* l);
/* zeroes the state (no cell has a hit, the last stamp is 0); suma_localizer_set_map does this too */
int suma_localizer_clear_live_grid(suma_localizer* l);
/* the primitive on a caller's flag image (host, one byte a texel of the data image), the counterpart of
 * suma_localizer_segment_flags: uploads the flags, segments them when objects are on, then updates the layer with the
 * frame (of the localiser's ctx, data-sized) at the sensor pose T (column-major, world frame, finite).  It needs no map.
 * *counts is optional.  Blocking.  A scan_id whose stamp scan_id + 1 is not greater than the last update's returns
 * SUMA_ERR_INVALID and launches nothing; so does a collection's own update (suma_localizer_process_scan counts its
 * scans from the last suma_localizer_set_map; suma_localizer_collect_frame takes the caller's scan_id). */
int suma_localizer_live_update_flags(suma_localizer* l, const suma_frame* frame, const double T[16], const uint8_t* host_flags,
                                     uint32_t scan_id, suma_live_counts* counts);
/* the counts of the last update; *updated = 0 and zero counts when there was none since the layer was enabled or cleared.
 * Both outputs are optional.  Blocking. */
int suma_localizer_live_counts(suma_localizer* l, suma_live_counts* counts, int32_t* updated);
/* composes: d_out_cells = width * height cells (DEVICE, 16-byte aligned), the static cells with state = OBSTACLE and
 * obstacle_z raised to the hit's top where the cell is live; d_out_mask (DEVICE, optional) = one byte a cell, 1 live,
 * 2 pending, 0 otherwise.  Writes only the caller's buffers; two calls give the same bytes.  Blocking. */
int suma_localizer_live_cells_device(suma_localizer* l, suma_grid_cell* d_out_cells, uint8_t* d_out_mask,
                                     suma_live_stats* stats);
/* the raw state, one suma_live_cell a cell: *n = width * height, min(*n, capacity) are copied.  Blocking. */
int suma_localizer_live_state(suma_localizer* l, suma_live_cell* host, uint32_t capacity, uint32_t* n);
/* replaces the raw state (n = width * height cells) and the last stamp: a saved layer put back, and how the tests reach
 * states that would take 65 535 updates.  Blocking. */
int suma_localizer_set_live_state(suma_localizer* l, const suma_live_cell* host, uint32_t n, uint32_t last_stamp);

/* ---- tracks: "is the car of this scan the car of the last one, and where is it going?"  With objects on, a tracker
 *      can follow every segmentation on the ctx stream with one update: the objects of the scan are joined into
 *      detections (fragments of one thing: same class, boxes no further apart than join_dist), the detections are
 *      associated to the tracks of the scans before (greedy by distance to the predicted position, inside a gate that
 *      widens while a track is not seen), matched tracks are filtered (alpha-beta), unmatched ones coast and expire,
 *      unmatched detections found new tracks.  A track keeps its id while it lives.  The update is enqueued only; the
 *      scan path does not wait for it, and everything else the localiser gives is bit-identical to a run with tracks
 *      off.  csrc/k_tracks.hip states the fp32 specification, tests/track_shim.c restates it; DESIGN.md 21 has the
 *      decomposition and what is out of scope (oriented boxes, optimal assignment, class- or size-aware gating,
 *      predicted occupancy, tracks in checkpoints and during mapping). */
typedef struct suma_track_params {
  float join_dist;       /* default 2 m: objects of one class whose boxes are this close are one detection; not NaN,
                            <= 1e6; negative: joining off */
  float gate_base;       /* default 1.5 m: a detection this close to a track's predicted position may be the track; 0 .. 1e6 */
  float gate_speed;      /* default 0.5 m: ... plus this much per scan-id step since the track was last matched; 0 .. 1e6 */
  float alpha;           /* default 0.5: the share of the residual the position takes; 0 .. 1 */
  float beta;            /* default 0.2: ... and the velocity, per step; 0 .. 2 */
  uint32_t confirm_hits; /* default 3: matches (the founding one included) before a track is confirmed; 1 .. 65 535 */
  uint32_t max_missed;   /* default 3: a track is dropped at its (max_missed + 1)-th update in a row without a match; 0 .. 65 535 */
  uint32_t max_tracks;   /* default 1024 (112 bytes each): the slots of the table; 1 .. 4096 */
  uint32_t max_rounds;   /* default 16: the rounds of mutual picks one association runs at most; 1 .. 64 */
} suma_track_params;
#define SUMA_TRACK_FREE 0u
#define SUMA_TRACK_TENTATIVE 1u
#define SUMA_TRACK_CONFIRMED 2u
#define SUMA_TRACK_NO_DETECTION 0xffffffffu
/* one slot of the table, 112 bytes; stamps are scan_id + 1 of an update; velocities in metres per scan-id step */
typedef struct suma_object_track {
  uint32_t id;           /* 1, 2, ...: never given twice between two clears; 0 in a free slot */
  uint32_t slot;         /* the index of this record in the table */
  uint32_t state;        /* SUMA_TRACK_FREE, _TENTATIVE or _CONFIRMED */
  uint32_t label;        /* of the detection matched last, as are n_texels .. r_min below */
  uint32_t n_texels, n_dynamic;
  uint32_t n_objects;    /* the fragments (suma_scan_object records) that detection was joined from */
  uint32_t hits;         /* matches, the founding one included; saturates at 65 535 */
  uint32_t missed;       /* updates in a row without a match */
  uint32_t first_stamp;  /* of the founding update */
  uint32_t last_matched; /* stamp of the last match */
  float position[3];     /* filtered; the prediction while the track is not seen */
  float velocity[3];
  float origin[3];       /* the founding detection's centroid: (position - origin) / (last_matched - first_stamp) is
                            the net velocity over the track's life */
  float min[3], max[3];  /* the joined box */
  float r_min;
  uint32_t detection;    /* the detection of this update the track matched or was founded by, else 0xffffffff */
} suma_object_track;
/* one update.  n_objects = n_detections + n_joined; n_detections = n_matched + n_born + n_dropped;
 * n_tracks_before = n_matched + n_missed; n_expired <= n_missed; the tracks alive afterwards number
 * n_tracks_before - n_expired + n_born, n_confirmed of them confirmed; rounds <= max_rounds, and n_unresolved > 0 only
 * with rounds = max_rounds */
typedef struct suma_track_counts {
  uint32_t n_objects, n_detections, n_joined, n_tracks_before, n_matched, n_missed, n_expired, n_born, n_dropped,
      n_confirmed, n_unresolved, rounds;
} suma_track_counts;
/* 2.0f, 1.5f, 0.5f, 0.5f, 0.2f, 3, 3, 1024, 16 */
void suma_track_params_default(suma_track_params* tp);
/* host only, no device: SUMA_OK, or SUMA_ERR_INVALID for values outside the ranges above, the text in
 * suma_last_error(NULL).  suma_localizer_enable_tracks applies the same rule. */
int suma_track_params_check(const suma_track_params* tp);
/* switches tracks on (tp NULL = the defaults) and allocates their blocks (about 160 bytes an object of max_objects, 250
 * bytes a slot).  Needs objects on: SUMA_ERR_INVALID otherwise, and for values outside the ranges above, with a message
 * and nothing launched.  Enabling again replaces the parameters and forgets the tracks; so does enabling objects again
 * with another max_objects. */
int suma_localizer_enable_tracks(suma_localizer* l, const suma_track_params* tp);
/* switches them off and gives the blocks back; suma_localizer_disable_objects and _disable_novelty do this too */
int suma_localizer_disable_tracks(suma_localizer* l);
/* no tracks, the last stamp is 0, the next id is 1; suma_localizer_set_map and _clear_novelty do this too */
int suma_localizer_clear_tracks(suma_localizer* l);
/* With tracks on, every segmentation -- a collection's, suma_localizer_segment_flags' or _live_update_flags' -- is
 * followed by one update at the stamp scan_id + 1; it is only enqueued.  A scan_id whose stamp is not greater than the
 * last update's returns SUMA_ERR_INVALID and launches nothing, the segmentation included.  These return the live
 * tracks of the last update in ascending slot order: *n = their number, min(*n, capacity) are copied; *counts and
 * *updated are optional; without an update since the tracks were enabled, cleared or set, *n = 0, the counts are 0 and
 * *updated = 0.  Blocking.  SUMA_ERR_CAPACITY after filling the outputs when n_dropped > 0 (the downloads' convention). */
int suma_localizer_tracks(suma_localizer* l, suma_object_track* host, uint32_t capacity, uint32_t* n,
                          suma_track_counts* counts, int32_t* updated);
int suma_localizer_tracks_device(suma_localizer* l, suma_object_track* d_out, uint32_t capacity, uint32_t* n,
                                 suma_track_counts* counts, int32_t* updated);
/* per object the last update read (the stored objects of its segmentation, in their order): the id of the track its
 * detection matched or founded, 0 for none (the detection was dropped).  *n = their number (0 without an update),
 * min(*n, capacity) are copied.  Blocking.  Texel -> object (suma_localizer_object_ids) -> track is two look-ups. */
int suma_localizer_object_tracks(suma_localizer* l, uint32_t* host, uint32_t capacity, uint32_t* n);
/* the primitive on a caller's records (host) in place of a segmentation's, the counterpart of
 * suma_localizer_segment_flags: one update at the stamp scan_id + 1 over n <= max_objects records.  It needs no map,
 * frame or pose.  *counts is optional.  Blocking.  The stamp rule above applies. */
int suma_localizer_track_objects(suma_localizer* l, const suma_scan_object* host_objects, uint32_t n, uint32_t scan_id,
                                 suma_track_counts* counts);
/* the raw table, one suma_object_track a slot: *n = max_tracks, min(*n, capacity) are copied; *last_stamp and *next_id
 * are optional.  Blocking. */
int suma_localizer_track_state(suma_localizer* l, suma_object_track* host, uint32_t capacity, uint32_t* n,
                               uint32_t* last_stamp, uint32_t* next_id);
/* replaces the raw table (n = max_tracks slots), the last stamp and the next id: a saved tracker put back, and how the
 * tests reach saturated hits, non-finite states and a full table.  A slot is checked for: state <= 2, and in a live
 * slot 1 <= id < next_id, first_stamp <= last_matched <= last_stamp; ids are not checked for being distinct.
 * Afterwards there is "no update" until the next one.  Blocking. */
int suma_localizer_set_track_state(suma_localizer* l, const suma_object_track* host, uint32_t n, uint32_t last_stamp,
                                   uint32_t next_id);

/* ---- place recognition and global relocalisation: "the sensor was switched on somewhere inside yesterday's map".  A
 *      place index holds one descriptor per scan of a mapping session: a polar height map about the sensor (sectors x
 *      rings, the highest kept point of each cell), made on the device from the vertex map of a frame the pipeline
 *      already holds (suma_pipeline_frame(s, 0) after a scan).  A query scores every entry under every cyclic shift of
 *      the sectors (one wave per entry, one lane per shift: hence sectors <= 64) and returns the K best places with the
 *      yaw the shift stands for.  csrc/k_place.hip states the fp32 specification, tests/place_shim.c restates it;
 *      DESIGN.md 13 has the decomposition and the limits.  The reference has nothing like it.
 *      The index is an object beside the pipeline: nothing of it enters a pipeline, a checkpoint image or any other
 *      entry.  It lives on one device; entries that take a ctx run on that ctx's stream (a ctx on another device is
 *      SUMA_ERR_INVALID), the others on a stream of the index; the index orders its own work across those streams.
 *      Calls on one index are serialised by the caller.  Errors: the library's codes; the text is
 *      suma_place_index_last_error(idx) (and suma_last_error(ctx) where a ctx was passed), or suma_last_error(NULL)
 *      after a failed create.
 *      (Kept here, not in suma_types.h, for the reason given at suma_semantic_params.) */
#define SUMA_PLACE_MAX_DIM 64        /* rings and sectors */
#define SUMA_PLACE_MAX_MATCHES 32    /* K of a query; candidates of a relocalisation */
typedef struct suma_place_index suma_place_index;
typedef struct suma_place_params {
  uint32_t rings;       /* default 20; 1 .. 64 */
  uint32_t sectors;     /* default 60; 1 .. 64 */
  float max_range;      /* default 80.0f; finite, > 0: points at or beyond it are left out */
  float height_offset;  /* default 2.0f; finite: the sensor's height above the ground, so that heights are positive */
  uint8_t keep_label[SUMA_DRAW_COLORS]; /* a point counts iff keep_label[label] != 0; default all 1 */
} suma_place_params;
typedef struct suma_place_match {
  uint32_t index;   /* entry index: position in the order of insertion */
  uint32_t id;      /* the caller's id of that entry */
  float distance;   /* 0 .. 2: 1 - the mean cosine of the column pairs at the best shift */
  int32_t shift;    /* 0 .. sectors - 1 */
  float yaw;        /* radians; the pose hypothesis is T_entry * Rz(yaw) */
} suma_place_match;
/* 20, 60, 80.0f, 2.0f, all labels kept */
void suma_place_params_default(suma_place_params* pp);
/* params NULL = the defaults; capacity = entries to make room for now (it grows).  SUMA_ERR_INVALID before any device is
 * touched: rings or sectors outside 1 .. 64, a max_range that is not finite and > 0, a height_offset that is not finite */
int suma_place_index_create(const suma_place_params* params, int hip_device, uint32_t capacity, suma_place_index** out);
void suma_place_index_destroy(suma_place_index* idx);
int suma_place_index_clear(suma_place_index* idx);
uint32_t suma_place_index_size(const suma_place_index* idx);
const char* suma_place_index_last_error(const suma_place_index* idx);
/* appends the descriptor of frame's vertex map (labels from its semantic map) with the caller's id; enqueued on the ctx
 * stream behind the work that made the frame, not waited for (it blocks only when the storage has to grow) */
int suma_place_index_add_frame(suma_place_index* idx, suma_ctx* ctx, const suma_frame* frame, uint32_t id);
/* entries first .. first + n - 1: cells n x sectors x rings floats (sector-major), norms n x sectors, ids n; any output
 * may be NULL.  Blocking. */
int suma_place_index_download(suma_place_index* idx, uint32_t first, uint32_t n, float* cells, float* norms, uint32_t* ids);
/* appends n entries from host cells (every cell 0 or in (0, 1000], else SUMA_ERR_INVALID); the norms are made on the
 * device.  Blocking. */
int suma_place_index_upload(suma_place_index* idx, const float* cells, const uint32_t* ids, uint32_t n);
/* the k best entries (1 <= k <= 32) for frame's descriptor, by (distance ascending, entry index ascending), leaving out
 * the entries whose id lies in [exclude_lo, exclude_hi] (lo > hi: none); *n_out = min(k, entries left).  Blocking. */
int suma_place_index_query_frame(suma_place_index* idx, suma_ctx* ctx, const suma_frame* frame, uint32_t exclude_lo,
                                 uint32_t exclude_hi, uint32_t k, suma_place_match* matches, uint32_t* n_out);
/* the same search for a descriptor given on the host (sectors x rings cells; its norms are made on the device) */
int suma_place_index_query(suma_place_index* idx, const float* cells_host, uint32_t exclude_lo, uint32_t exclude_hi,
                           uint32_t k, suma_place_match* matches, uint32_t* n_out);
/* unsorted: every entry's least distance and its shift for frame's descriptor (size() floats / int32s).  Blocking. */
int suma_place_index_query_all(suma_place_index* idx, suma_ctx* ctx, const suma_frame* frame, float* dist, int32_t* shift);

/* global relocalisation of a localiser that has a map: (1) K1-K3 of the scan into the localiser's frame, as
 * suma_localizer_process_scan does; (2) suma_place_index_query_frame with k = max_candidates (1 .. 32), nothing left
 * out; (3) for each match in order: suma_localizer_set_pose(poses16[index] * Rz(yaw)) and one localisation scan -- each
 * result is, to the bit, what suma_localizer_set_pose followed by suma_localizer_process_scan gives; (4) among the
 * candidates with tracked = 1 the one with the least stats.error / (double)stats.valid wins, the earlier one on a tie,
 * and the localiser is left in its state (pose, identity increment, window, rendered model): the next
 * suma_localizer_process_scan continues from there.  If none is tracked, found = 0 and the localiser is as it was
 * before the call: pose, increment, whether it has a pose, window origin, window contents, gather count.
 * poses16: one column-major 4x4 pose per ENTRY INDEX (the mapping session's trajectory); n_poses must equal the index's
 * size.  A candidate whose pose suma_localizer_set_pose refuses (outside the grid, window beyond max_surfels) ends the
 * call with that error and the localiser restored. */
typedef struct suma_relocalize_candidate {
  suma_place_match match;
  int32_t reserved;
  suma_localizer_result result;
} suma_relocalize_candidate;
typedef struct suma_relocalize_result {
  int32_t found;
  uint32_t n_tried;   /* candidates tried = matches returned */
  int32_t winner;     /* index into candidates, -1 when found = 0 */
  int32_t reserved;
  suma_place_match match;        /* the winner's (zero when found = 0) */
  int32_t reserved2;
  suma_localizer_result result;  /* the winner's */
  suma_relocalize_candidate candidates[SUMA_PLACE_MAX_MATCHES];
} suma_relocalize_result;
int suma_localizer_relocalize(suma_localizer* l, suma_place_index* idx, const double* poses16, uint32_t n_poses,
                              const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                              uint32_t max_candidates, int32_t fixed_iterations, suma_relocalize_result* result);
int suma_localizer_relocalize_device(suma_localizer* l, suma_place_index* idx, const double* poses16, uint32_t n_poses,
                                     const suma_float4* d_points, const float* d_labels, const float* d_probs, uint32_t n,
                                     uint32_t max_candidates, int32_t fixed_iterations, suma_relocalize_result* result);

/* ---- motion compensation (deskewing) of raw sweeps (csrc/k_deskew.hip states the operation).
 *      A point measured at sweep fraction s in [0, 1], in the sensor frame of that instant, is moved into the sensor
 *      frame at fraction t_ref:  p' = Exp((s - t_ref) * scale * Log(motion)) * p,  motion = pose_prev^-1 * pose, the
 *      sensor's rigid motion over one sweep period (column-major double[16]).  The fourth component is copied bit for
 *      bit; a point with a non-finite coordinate or time keeps all its bits.  s comes from the point's azimuth
 *      (suma_deskew_params, below) or from the caller's times[n].
 *   suma_deskew_points(_device): n points (host / device), out may equal the input; the device entry enqueues on the ctx
 *      stream and returns.  dp NULL = the defaults (azimuth time, counter-clockwise, start_azimuth 0, t_ref 0.5, scale 1).
 *      A motion that is bitwise the identity launches nothing and leaves every bit alone.  n = 0 is SUMA_OK.
 *      SUMA_ERR_INVALID with a message: t_ref outside [0, 1], a non-finite field, start_azimuth outside [-2 pi, 2 pi], an
 *      unknown time source, the `times` source without times, a NULL or non-finite motion, device points that are not
 *      16-byte aligned.
 *   Pipeline: while enabled, suma_pipeline_process_scan(_device) and suma_pipeline_begin_scan(_device) correct the scan
 *      in front of K1 with the motion suma_pipeline_last_increment returns at that moment (the identity before the first
 *      pose update, so the first scan keeps its bits), on the stream K1 reads the points from and without any new
 *      synchronisation.  The caller's points are never written: the corrected scan lives in a block the pipeline owns.
 *      The scan entries carry no times, so only the azimuth source can be enabled.
 *      suma_pipeline_set_deskew_motion: a one-shot override for the next scan (an IMU, wheel odometry, the first scans);
 *      it is dropped by _disable_deskew and suma_pipeline_reset.  suma_pipeline_deskew_motion: what the last corrected
 *      scan used and where it came from (SUMA_DESKEW_MOTION_*; NONE and the identity before any).
 *      While enabled, the entries that hand a scan over before the previous pose exists return SUMA_ERR_INVALID and
 *      change nothing: suma_pipeline_prefetch_scan, _process_prefetched, _begin_prefetched, _process_scan_async, the four
 *      *_scan_scores* entries and suma_pipeline_run_scans.  enable is refused between begin_scan and update_map and
 *      while prefetched scans are pending.  With the correction never enabled nothing of it runs.
 *   Checkpoints hold no deskew state: the image is unchanged, a host enables the correction again after a load, and
 *      since last_increment is in the image the resumed run continues bit for bit.  A pending one-shot override is NOT
 *      saved.
 *   Localiser: the same switch on suma_localizer_process_scan(_device), with the `increment` of its step 7 as the motion
 *      (kept with constant_velocity = 0 too; the identity after suma_localizer_set_pose).  suma_localizer_relocalize
 *      does not correct.  Evidence and novelty read the frame the localiser holds, hence the corrected one. */
/* The parameters (they live here and not in suma_types.h, which belongs to the CPU oracle as well).
 * 20 bytes: int32 time_source @0, int32 clockwise @4, float start_azimuth @8, t_ref @12, scale @16. */
enum { SUMA_DESKEW_TIME_AZIMUTH = 0, SUMA_DESKEW_TIME_TIMES = 1 };
/* where the motion of the last corrected scan came from */
enum { SUMA_DESKEW_MOTION_NONE = 0, SUMA_DESKEW_MOTION_INCREMENT = 1, SUMA_DESKEW_MOTION_OVERRIDE = 2 };
typedef struct suma_deskew_params {
  int32_t time_source;  /* SUMA_DESKEW_TIME_AZIMUTH: the sweep fraction of a point is its azimuth's share of the turn;
                           SUMA_DESKEW_TIME_TIMES: the caller's times[n] */
  int32_t clockwise;    /* azimuth time only: 0 = the beam turns counter-clockwise seen from +z (atan2(y, x) grows) */
  float start_azimuth;  /* azimuth time only: atan2(y, x) of the sweep's first column, radians, in [-2 pi, 2 pi] */
  float t_ref;          /* the sweep fraction whose sensor frame the points are moved into, in [0, 1] */
  float scale;          /* the sweep period as a fraction of the interval `motion` spans (1: one sweep per scan) */
} suma_deskew_params;
void suma_deskew_params_default(suma_deskew_params* dp);
/* host only, no device needed: SUMA_OK, or the SUMA_ERR_INVALID suma_deskew_points(_device) would return for these
 * parameters, this motion and (for the `times` source) times present or not; the text is suma_last_error(NULL) */
int suma_deskew_check(const suma_deskew_params* dp, int have_times, const double motion[16]);
int suma_deskew_points(suma_ctx* ctx, const suma_deskew_params* dp, const suma_float4* points, const float* times_or_null,
                       uint32_t n, const double motion[16], suma_float4* out);
int suma_deskew_points_device(suma_ctx* ctx, const suma_deskew_params* dp, const suma_float4* d_points,
                              const float* d_times_or_null, uint32_t n, const double motion[16], suma_float4* d_out);
int suma_pipeline_enable_deskew(suma_pipeline* s, const suma_deskew_params* dp);
int suma_pipeline_disable_deskew(suma_pipeline* s);
int suma_pipeline_set_deskew_motion(suma_pipeline* s, const double motion[16]);
int suma_pipeline_deskew_motion(const suma_pipeline* s, double motion[16], int32_t* source);
int suma_localizer_enable_deskew(suma_localizer* l, const suma_deskew_params* dp);
int suma_localizer_disable_deskew(suma_localizer* l);
int suma_localizer_set_deskew_motion(suma_localizer* l, const double motion[16]);
int suma_localizer_deskew_motion(const suma_localizer* l, double motion[16], int32_t* source);

/* ---- per-kernel timing (rv::Stopwatch / SurfelMapping::Stats, SurfelMapping.cpp:183-207):
 *      on = 1: every kernel group is bracketed by HIP events on the ctx stream; on = 2: only the
 *      Gauss-Newton chain (the kernel with the largest share of GPU time), which costs two event
 *      records per scan (each costs the stream a ~6 us bubble); on = 3: the same on every 4th scan; on = 0: off.
 *      suma_profile_get fills up to cap entries, returns the number of distinct kernels. */
typedef struct suma_kernel_time {
  char name[48];
  uint64_t launches;
  double total_ms;
  double bytes; /* algorithmic bytes summed over the launches (SURVEY.md 8d formulas) */
} suma_kernel_time;
/* Where the calls of the blocking host-vector entry (suma_pipeline_process_scan / suma_pipeline_begin_scan: the
 * reference's processScan(const rv::Laserscan&), SurfelMapping.cpp:175, 323-331) spent their time ON THE CALLER'S THREAD,
 * summed since the last reset: out = {calls, whole calls, wait for the staging slot, pageable -> pinned copies, upload
 * enqueue, kernel enqueue, wait for the minimisation result, threads that share the copies}; seconds.  The copy helpers
 * are sized from the CPUs the process may use (affinity mask and cgroup quota; SUMA_COPY_HELPERS overrides). */
int suma_pipeline_host_entry_times(suma_pipeline* s, double out[8], int reset);
int suma_profile_enable(suma_ctx* ctx, int on);
int suma_profile_reset(suma_ctx* ctx);
int suma_profile_get(suma_ctx* ctx, suma_kernel_time* out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SUMA_HIP_H_ */
