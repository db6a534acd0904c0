/*
 * suma_internal.h -- host-side state of the gfx950 core and the launcher prototypes shared by
 * the translation units (k_preprocess.hip, k_icp.hip, k_render.hip, k_update.hip, suma_api.hip).
 */
#ifndef SUMA_INTERNAL_H_
#define SUMA_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include <rocprim/types/double_buffer.hpp>

#include "../../include/suma_hip.h"
#include "dev_math.h"

#ifndef SUMA_TILE
#define SUMA_TILE 1024u       /* items per compaction tile = threads per block (16 waves) */
#endif
#ifndef SUMA_COMPACT_BLOCKS
#define SUMA_COMPACT_BLOCKS 256u /* grid of the ticketed compaction kernels: ONE block per CU -- their 1024-thread blocks are
                                    resident one per CU (registers / LDS), every block draws tickets until none is left, so
                                    a second generation of blocks only starts to draw failing tickets at the kernel's
                                    tail (512: K9 76 -> 74 us slower, -0.7 % scans/s) */
#endif
#define SUMA_STREAM_BLOCKS 2048u /* grid cap of the grid-stride surfel kernels: 8 blocks of 256 per CU */
#define SUMA_EXTRACT_CAPACITY 500000u /* SurfelMap.cpp:279 */
#define SUMA_MAX_MODEL_WIDTH 5461u /* floor((2^21 - 1) / (1.5 * 256)): k_render's window coordinates */
#define SUMA_MAX_HYP 64u

/* An owned device (or, with Pinned, pinned host) block of cap elements of T: freed by the destructor, moved but never
 * copied, and read as a plain T* wherever the block is used.  A failed allocation leaves it empty. */
template <class T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  T* operator->() const { return p; }
  void reset() {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr, cap = 0;
  }
  /* replaces the block by one of n elements */
  hipError_t alloc(size_t n) {
    reset();
    void* q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
    if (e == hipSuccess) p = (T*)q, cap = n;
    return e;
  }
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

/* Counters that live in HBM so that no kernel launch needs a host round trip. */
struct DevState {
  uint32_t n_surfels;      /* S: size of the active map */
  uint32_t n_updated;      /* S': survivors of K9 (before the K11 area filter) */
  uint32_t n_kept_updated; /* survivors of K9 and K11 */
  uint32_t n_data;         /* D: new surfels emitted by K10 (before the K11 area filter) */
  uint32_t n_kept_data;
  uint32_t n_extracted;    /* K12: surfels written by the last extraction */
  uint32_t overflow;       /* bit 0: surfel capacity, bit 1: cache arena, bit 2: extract capacity, bit 3: compaction spin limit */
  uint32_t ticket;         /* dynamic tile id of the look-back compaction kernels */
  uint32_t reserved0;      /* blocks-done counter of a self-closing objective pass (k_icp.hip) */
  uint32_t cache_used;     /* surfels allocated from the submap cache arena */
  uint32_t fault_site;     /* which bounded spin gave up (bit per site; reported with overflow bit 3) */
  uint32_t n_ext_update;   /* extraction fused into the update: records K9 sent to the cache arena (K10's come behind) */
  uint32_t pad[4];
};

/* one stretch of the world export's source sequence: count records at base, the first with source index start */
struct WorldSpan {
  const suma_surfel* base;
  uint32_t start, count;
};

/* one cached submap tile in the device arena */
struct CacheSlot {
  uint32_t offset, count;
};

/* Gauss-Newton state of one minimisation, device resident (LieGaussNewton members,
 * LieGaussNewton.h:56-72, plus Frame2Model's iteration counter and row 7 of its blend target) */
struct GnState {
  double Tk[16];
  double last_error;
  double F, F_inlier;
  uint32_t iteration; /* Frame2Model::iteration_ */
  uint32_t k;         /* LieGaussNewton::k_ */
  uint32_t done, converged;
  uint32_t valid, outlier, invalid, n_hist;
  uint32_t pending; /* a pixel phase has left partial sums that the next launch must consume */
  uint32_t pad[3];
  int64_t acc[SUMA_ACC_WORDS];
  double JtJ[36];
  double Jtr[6];
};

/* What the host reads back after a minimisation of the scan pipeline.  The closing launch of the chain
 * writes it straight into pinned host memory (seq last, behind a system-scope fence), so the result
 * costs no copy commands in the stream: the re-rendering that follows the minimisation starts right
 * behind the closing launch, and the host polls seq. */
struct HostResult {
  double Tk[16];
  double F, F_inlier;
  uint32_t valid, outlier, invalid, k, converged, iteration;
  DevState ds;
  uint32_t seq;
  uint32_t n_hist;
  /* only filled for the class-by-class entries (suma_icp_minimize / suma_icp_jacobian_products), not by the scan
   * pipeline's launches: the fixed-point sums of the last step with the bias removed (JtJ / Jtr / F are these words
   * times 2^-28, formed on the host exactly as the device forms them) */
  int64_t acc[SUMA_ACC_WORDS];
  double JtJ[36], Jtr[6]; /* of the last step (LieGaussNewton::information); closing launch of suma_icp_minimize only */
};

/* One Gauss-Newton chain as its caller describes it: filled once, passed to enqueue_minimize (suma_api.hip),
 * launch_gn_init and launch_icp_iteration, and nothing of it is kept on the context. */
struct GnChain {
  const suma_frame *current, *model;
  suma_icp_objective obj; /* resolved: the adapter's object or the ctx parameters (Frame2Model.cpp:66-67) */
  /* LieGaussNewton's budget (0: until convergence) and stopping tests; an eval-only launch reads none of them */
  uint32_t max_iterations;
  double epsilon, delta;
  /* start state: n_hyp poses, read by launch_gn_init (batch) or by the chain's first launch (single chain), and
   * Frame2Model::iteration_ of the first / every other chain (0 right behind a setData; > 0 for a minimisation that
   * follows another one on the same setData, SurfelMapping.cpp:693-700) */
  const double* T0s;
  uint32_t n_hyp;
  uint32_t iteration0, iteration0_rest;
  int with_history; /* LieGaussNewton::history() into gn_history (single chain) */
  /* if set: the chain reports to this pinned host record, stamped with report_seq -- from its closing launch, or from
   * the eval-only pixel pass of a single chain, which then closes itself.  report_full: also acc / JtJ / Jtr / n_hist */
  HostResult* report;
  uint32_t report_seq;
  int report_full;
  const double* pose_base; /* if set: the closing launch writes pose_base * increment to pose_block */
  int fuse_k8; /* the self-closing eval-only pass also runs K8's per-pixel work and the counter resets */
};

struct MapConsts {
  float pixel_size, log_prior, log_unstable, p_unstable;
  float radconf_angle_thresh, update_angle_thresh;
};

struct suma_frame {
  suma_ctx* ctx;
  uint32_t width, height;
  DevBuf<float4> block; /* 3 x width x height */
  float4* map[3];       /* vertex, normal, semantic: views into block */
  /* bumped by every call of the C-ABI that writes the frame (upload / copy / swap / preprocess / render / touch): what
   * the render de-duplication and the fused K8 products compare instead of assuming that a caller-owned frame changed */
  uint64_t version;
  /* ctx-stream accesses (suma_ctx.enq_seq) -- lets suma_preprocess put its side-stream work in front of everything
   * the ctx stream still holds, unless that includes an access to this very frame */
  uint64_t last_access;
};

struct ProfEvent {
  hipEvent_t a, b;
  hipStream_t stream; /* the launch stream the pair brackets */
  int id;
  double bytes;
  uint32_t launches; /* kernel launches bracketed by this event pair (a chain of identical launches) */
};

/* host-side time of the blocking host-vector entry (suma_pipeline_process_scan), summed since the last reset:
 * where a call of the reference-shaped entry spends its time on the CALLER's thread (suma_pipeline_host_entry_times) */
struct HostEntryTimes {
  double slot_wait_s;  /* waiting for the staging slot of the scan before last to be read */
  double copy_s;       /* pageable -> pinned copies (caller + helper threads) */
  double enqueue_s;    /* hipMemcpyAsync + event record of the upload */
  double launch_s;     /* enqueueing the scan's kernels (everything else that is not a wait) */
  double result_wait_s; /* polling for the minimisation result: the GPU is the one being waited for */
  double call_s;       /* whole calls */
  uint64_t calls;
  uint32_t copy_threads; /* caller + helpers that took a share of the copies */
};

struct suma_ctx {
  suma_params p;
  int device;
  hipStream_t stream;      /* the ctx stream: everything the C-ABI promises to order */
  hipStream_t ls;          /* stream the launchers enqueue on: == stream, except while the scan pipeline enqueues side work */
  hipStream_t side_stream; /* work that is off the critical path of a scan (the next scan's upload + preprocessing) */
  int side_stream_off;     /* SUMA_NO_SIDE_STREAM / a serialising tool: everything on the ctx stream */
  DevBuf<uint32_t> sync_flags; /* device: sequence words of the in-memory stream hand-offs (k_sync.hip) */
  uint32_t pre_seq;        /* preprocessing hand-offs issued so far */
  uint32_t gate_pending;   /* != 0: the ctx stream has not yet waited for this preprocessing hand-off (flush_gate) */
  int gate_by_event;       /* the pending hand-off is a runtime event (pre_event), not the in-memory word: several
                              pipelines in one process, see side_handoff (k_sync.hip) */
  hipEvent_t pre_event;
  hipEvent_t order_event;  /* ctx stream -> side stream, only when a frame's last access may still be in flight */
  uint64_t enq_seq, done_seq; /* frame accesses enqueued on the ctx stream / known complete at the last host wait */
  bool cache_nothing_stale; /* the last compaction attempt found no stale block: no point in synchronising again */
  const suma_frame* gate_frame; /* the frame the pending side-stream work writes */
  struct Ingest* ingest;   /* pinned double-buffered scan staging + copy stream + helper threads (suma_ingest.hip) */
  PinnedBuf<HostResult> h_rec; /* results of suma_icp_minimize / suma_icp_jacobian_products ([0] / [1]) */
  uint32_t rec_seq;
  std::string err;

  proj_t pd, pm; /* data / model projection */
  MapConsts mc;
  size_t P, Pm;

  /* preprocessing scratch */
  DevBuf<unsigned long long> zbuf_data; /* P keys: K7 (and K1 outside the scan pipeline's side stream) */
  DevBuf<unsigned long long> zbuf_k1;   /* P keys: K1 of the scan pipeline -- preprocessing of scan t+1 overlaps K7 / K10 of scan t */
  DevBuf<float4> eroded;                /* P: raw labels of K1 (scratch between k1_resolve and the fused K2/K3) */
  /* optional vertex-map filters (k_filters.hip), allocated on first use */
  DevBuf<float4> filt_temp;             /* P: the reference's temp_vertices_ */
  DevBuf<unsigned long long> filt_sort; /* 2 x (cap / 2) keys (pixel << 32 | point index), unsorted / sorted */
  DevBuf<char> filt_sort_tmp;           /* rocprim's temporary storage of a sort of filt_sort.cap / 2 keys (cap: bytes) */
  DevBuf<float4> scan_points;           /* staging for host scans */
  DevBuf<float> scan_labels, scan_probs;
  /* semantic front end (k_semantic.hip), allocated on first use */
  DevBuf<unsigned long long> sem_zbuf;  /* left cleared by every resolve */
  DevBuf<float> sem_labels, sem_probs;  /* the back-projection of the scan pipeline's scores entry */
  /* KNN post-processing (k_semantic_knn.hip): record image P x {class, prob bits} then P ranges; [0]
   * suma_semantic_unproject_knn (ctx stream), [1] the pipeline's scores_knn entry (its input stream); each only grows */
  DevBuf<char> sem_knn[2];
  /* SurfelMap::draw (k_draw.hip), allocated on first use: z-buffer of the largest image drawn (left cleared by every
   * resolve) and the large-quad queue, max_surfels ids + its counter (left at 0) */
  DevBuf<unsigned long long> draw_zbuf;
  DevBuf<uint32_t> draw_queue;
  /* suma_map_export_world (k_world.hip), allocated on first use: the span table of the source sequence, the per-source
   * scratch (8 bytes a source surfel, 48 with voxel fusion), the library sort / scan's temporary storage (histograms and
   * partial sums: the sorts run in double buffers inside the scratch), the counters */
  DevBuf<struct WorldSpan> world_spans;
  DevBuf<char> world_scratch, world_tmp;
  DevBuf<uint32_t> world_counters;
  PinnedBuf<uint32_t> world_counters_h;
  /* suma_world_grid / _fit (k_grid.hip), allocated on first use: 16 bytes a raster cell and the counters; the per-record
   * arrays and the sorts' storage are world_scratch and world_tmp (both run on the ctx stream, one behind the other) */
  DevBuf<uint4> grid_runs;
  DevBuf<uint32_t> grid_counters;
  PinnedBuf<uint32_t> grid_counters_h;
  /* suma_grid_plan_field / _paths (k_plan.hip), allocated on first use: PLAN_SCRATCH_PER_CELL bytes a raster cell, the
   * counters and round flags, and the goals / starts / paths exchanged with the host (words; pinned on the way in) */
  DevBuf<char> plan_scratch;
  DevBuf<uint32_t> plan_counters, plan_io;
  PinnedBuf<uint32_t> plan_counters_h, plan_io_h;
  /* suma_pipeline_checkpoint_save / _load (k_checkpoint.hip), allocated on first use: the staged image, the span table
   * of kc_pack and one digest word per section */
  DevBuf<char> ckpt_image;
  DevBuf<struct WorldSpan> ckpt_spans;
  DevBuf<unsigned long long> ckpt_digests;

  /* ICP */
  const suma_frame *icp_current, *icp_model;
  suma_icp_objective obj; /* per-object Frame2Model parameters of the adapter (suma_icp_set_objective) */
  bool obj_set;
  DevBuf<GnState> gn; /* 2 x SUMA_MAX_HYP states, alternating with the launch parity */
  DevBuf<int64_t> gn_partial; /* 3 rotating sets of SUMA_MAX_HYP x ICP_RECORDS x SUMA_ACC_WORDS accumulators (k_icp.hip) */
  uint32_t gn_part_launch;   /* rotation counter, never reset */
  uint32_t gn_part_dirty[3]; /* hypotheses with possibly non-zero records, per set */
  uint32_t gn_launch;  /* launches since the last gn_init */
  /* per-pixel K8 products already written for (frame, stamp) by the statistics pass, see launch_map_update */
  const suma_frame* k8_fused_frame;
  uint64_t k8_fused_version; /* suma_frame.version the products were made from */
  uint32_t k8_fused_stamp;
  uint64_t k8_fused_params;
  DevBuf<float> pose_block; /* 16 floats pose + 16 floats inverse for the post-ICP render */
  HostEntryTimes het;
  uint32_t icp_iteration0; /* suma_icp_set_iteration: Frame2Model::iteration_ for the NEXT suma_icp_minimize (one shot) */
  DevBuf<double> gn_history; /* (max_iterations + 1) x 16 doubles (single minimise only) */
  DevBuf<double> gn_T0s;     /* SUMA_MAX_HYP x 16 staging for batched starts */
  uint32_t gn_history_cap;
  uint32_t last_n_hist; /* LieGaussNewton::history() entries of the last suma_icp_minimize */
  uint64_t hist_seq;    /* minimisations that recorded a history on this context (suma_icp_history_sequence) */
  uint32_t icp_blocks;
  PinnedBuf<GnState> h_gn;

  /* surfel map */
  DevBuf<suma_surfel> surfels[2]; /* double buffer: active map / compaction target */
  int cur;
  DevBuf<float> poses;     /* max_poses x 16 */
  DevBuf<float> poses_inv; /* max_poses x 16 */
  suma_frame *old_frame, *new_frame, *composed_frame;
  DevBuf<unsigned long long> zbuf_a, zbuf_b; /* Pm */
  DevBuf<float4> radius_conf;                /* P */
  DevBuf<float4> pixrec;                     /* P x 4: packed measurement record for K9 (one 64-byte line per pixel) */
  DevBuf<uint8_t> integrated;                /* P */
  /* one byte per surfel of the compaction target: "lies in the submap tile that is extracted right after this update"
   * (written by K9 / K10 at the surfel's final index, read by K12 instead of a pass over the whole map) */
  DevBuf<uint8_t> extract_flags;       /* max_surfels */
  struct {
    bool valid;                        /* the last update flagged the tile (i, j) */
    int32_t i, j;
    bool fused;    /* ... and K9 / K10 have already written and committed the tile's cache block (slot below) */
    uint32_t slot;
  } flagged;
  DevBuf<uint32_t> index_map;            /* P: K7 winners as surfel id + 1 (exported by K10) */
  DevBuf<unsigned long long> tile_status; /* look-back status words */
  DevBuf<unsigned long long> tile_group;  /* 2 x group_words, per 64 tiles: {arrived, sum}; launches alternate halves */
  uint32_t group_words;
  uint32_t n_tiles_cap;
  uint32_t epoch;
  DevBuf<DevState> ds;
  PinnedBuf<DevState> h_ds;
  uint32_t timestamp; /* SurfelMap::timestamp_ (host copy; kernels get it by value) */
  /* submaps (SurfelMap.cpp:744-824): caches live in a device arena, the index on the host */
  int32_t origin_i, origin_j;
  DevBuf<suma_surfel> cache_arena;
  uint32_t cache_cap;
  DevBuf<CacheSlot> cache_slots; /* device table */
  uint32_t cache_compactions; /* times the arena has been compacted (cache_compact, suma_api.hip) */
  uint64_t cache_bound;       /* host-side upper bound of DevState.cache_used: exact value at the last read-back + the
                                 most every extraction since can have added */
  uint32_t cache_slots_cap;
  std::map<std::pair<int32_t, int32_t>, uint32_t> cache_index; /* (i,j) -> slot */
  std::vector<std::pair<int32_t, int32_t>> extraction;        /* pending tiles, used as a stack */

  /* profiling */
  int profiling; /* 0 off, 1 every kernel group, 2 only the group named prof_filter, 3 every 4th occurrence of that group */
  uint32_t prof_tick;
  std::string prof_filter;
  std::vector<ProfEvent> prof_events;
  std::vector<hipEvent_t> prof_pool;
  std::vector<std::string> prof_names;
  std::vector<double> prof_ms, prof_bytes;
  std::vector<uint64_t> prof_launches;
  uint32_t known_surfels; /* last S read back (for the algorithmic-byte model) */

  /* what the OLD / NEW frames and the last render() target currently hold: lets render() skip a
   * call that would reproduce them bit for bit (the reference renders the same map from the same
   * pose at the end of scan t and again at the start of scan t+1, SurfelMapping.cpp:351,803) */
  uint64_t map_version, params_version;
  /* K7 splat already in zbuf_data (fused into the post-ICP render pass of the pipeline) */
  struct {
    bool valid;
    float pose[16];
    uint64_t map_version, params_version;
  } k7;
  /* suma_map_render_active splats the index map speculatively (the reference's updatePose renders the active map at
   * the pose that updateMap then passes to update(), SurfelMapping.cpp:406 / :799); a splat nobody consumed switches the
   * speculation off until an update arrives that WOULD have consumed one */
  struct {
    bool on;
    bool have_last;
    float last_pose[16];
    uint64_t map_version, params_version;
  } k7_spec;
  struct {
    bool valid;
    float pose_old[16], pose_new[16], conf_threshold;
    uint64_t map_version, params_version;
    const suma_frame* out;
    uint64_t out_version, old_version, new_version; /* suma_frame.version of the three targets after the render */
  } rendered;
};

struct suma_pipeline {
  suma_ctx* c;
  suma_frame *last_frame, *current_frame, *current_model, *last_model;
  double current_pose[16], last_pose[16], pose_old[16], pose_new[16], last_increment[16];
  double last_pose_old[16]; /* lastPose_old_, SurfelMapping.cpp:456 */
  uint32_t timestamp;
  int phase; /* 0: between scans, 1: begin_scan done, 2: update_pose done (suma_pipeline_begin_scan / _update_pose / _update_map) */
  float log_unstable;
  suma_icp_stats stats;
  uint32_t track_loss;
  /* the statistics pass of updatePose (SurfelMapping.cpp:411-423) is read back lazily: its copy is
   * enqueued, and resolved at the next synchronisation point instead of stalling the scan */
  PinnedBuf<HostResult> h_res; /* [0] minimisation result, [1..2] statistics pass (alternating) */
  uint32_t res_seq, stats_seq;
  bool stats_pending;
  uint32_t stats_slot;
  suma_icp_stats stats_mst;
  struct LoopState* loop; /* suma_pipeline_enable_loop_closing; NULL: off, and nothing of the loop closing runs */
  struct Deskew* deskew;  /* suma_pipeline_enable_deskew (suma_deskew.hip); NULL until first enabled, and nothing of it runs while off */
};

int pipeline_process_scan_impl(suma_pipeline* s, const suma_float4* d_points, const float* d_labels, const float* d_probs,
                               uint32_t n, int32_t fixed_iterations, hipEvent_t upload_done);
int pipeline_begin_scan_impl(suma_pipeline* s, const suma_float4* d_points, const float* d_labels, const float* d_probs,
                             uint32_t n, hipEvent_t upload_done);
int pipeline_update_pose_impl(suma_pipeline* s, int32_t fixed_iterations);
int pipeline_update_map_impl(suma_pipeline* s);
/* closes a scan whose begin returned r: update_pose + update_map unless r failed or begin_only; a failed scan resets
 * the phase, so that it does not wedge the phase check */
int pipeline_finish_scan(suma_pipeline* s, int r, int32_t fixed_iterations, bool begin_only);
/* the stream behind which a scan's input buffers are free again (the preprocessing that read them runs there) */
hipStream_t pipeline_input_stream(suma_pipeline* s);
/* sets c->err and returns code */
int fail(suma_ctx* c, int code, const std::string& msg);
/* the same for entries without a ctx: the text suma_last_error(NULL) returns on this thread */
int fail_without_ctx(int code, const std::string& msg);
/* the overflow bits of the counters last read into c->h_ds: SUMA_OK, or the error every download reports (sets c->err) */
int check_overflow(suma_ctx* c);
/* k_semantic.hip: parameter check of the semantic entries (sets c->err) */
int semantic_check(suma_ctx* c, const suma_semantic_params* sp);
/* the scan input of the pipeline's scores entries: the phase check, sem_labels / sem_probs for n points and the wait
 * for the scores' producer; *st = the stream the back-projection and the preprocessing run on */
int semantic_scan_input(suma_pipeline* s, uint32_t n, void* producer_event, hipStream_t* st);
/* suma_ingest.hip */
void ingest_destroy(suma_ctx* c);
void ingest_drain(suma_ctx* c);
/* scans staged with suma_pipeline_prefetch_scan that have not been processed */
uint32_t ingest_pending(suma_ctx* c);
/* host scan -> pinned staging -> copy stream; *d_base = device block (points | labels | probs), *uploaded = the event the
 * consumer stream waits for, *slot = token for ingest_consumed */
int ingest_stage_blocking(suma_ctx* c, const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                          const suma_float4** d_points, const float** d_labels, const float** d_probs, hipEvent_t* uploaded,
                          void** slot);
void ingest_consumed(suma_ctx* c, void* slot, hipStream_t reader);
/* side stream of a ctx (created on first use; NULL under SUMA_NO_SIDE_STREAM / serialising tools) */
int ensure_side_stream(suma_ctx* c);
/* after side-stream work that writes `frame`: the ctx stream's next reader waits for it (flush_gate) */
int side_handoff(suma_ctx* c, const suma_frame* frame);
void side_stream_released(suma_ctx* c);
int pipeline_process_host_scan(suma_pipeline* s, const suma_float4* points, const float* labels, const float* probs,
                               uint32_t n, int32_t fixed_iterations);

#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                           \
      return SUMA_ERR_HIP;                                                                       \
    }                                                                                            \
  } while (0)

/* Makes b hold at least n elements: nothing if it already does; else the streams in drain that exist are synchronised
 * (work there may still use the block; only if there is one), the block is freed and one of alloc (default: n) elements
 * is made.  Returns 1 for a new block, 0 for none, SUMA_ERR_HIP with c->err set on failure (b is then empty). */
template <class T, bool Pinned>
int grow(suma_ctx* c, DevBuf<T, Pinned>& b, size_t n, std::initializer_list<hipStream_t> drain, size_t alloc = 0) {
  if (n <= b.cap) return 0;
  if (b)
    for (hipStream_t st : drain)
      if (st) HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, b.alloc(alloc ? alloc : n));
  return 1;
}

/* profiling scope: brackets the launches of one named kernel with events on the ctx stream */
int prof_begin(suma_ctx* c, const char* name, double bytes, uint32_t launches);
void prof_end(suma_ctx* c, int token);
struct ProfScope {
  suma_ctx* c;
  int tok;
  ProfScope(suma_ctx* c_, const char* name, double bytes, uint32_t launches = 1)
      : c(c_), tok(wanted(c_, name) ? prof_begin(c_, name, bytes, launches) : -1) {}
  static bool wanted(suma_ctx* c, const char* name) {
    if (c->profiling == 1) return true;
    if (c->profiling < 2 || c->prof_filter != name) return false;
    /* an event record is a barrier + signal packet: ~6 us of bubble in front of the kernel behind it (rocprofv3
     * timeline).  Mode 3 samples one occurrence in four so that the measurement costs the measured run < 1 % */
    return c->profiling == 2 || (c->prof_tick++ & 3u) == 0;
  }
  ~ProfScope() {
    if (tok >= 0) prof_end(c, tok);
  }
};

/* ---- launchers (each enqueues on c->stream, returns hipGetLastError()) ---- */
/* k_preprocess.hip */
hipError_t launch_preprocess(suma_ctx* c, const float4* d_pts, const float* d_labels, const float* d_probs, uint32_t n,
                             uint32_t timestamp, suma_frame* out);
/* k_icp.hip */
hipError_t launch_k1_average(suma_ctx* c, const float4* d_pts, const float* d_labels, const float* d_probs, uint32_t n,
                             uint32_t timestamp, float4* vertex, float4* raw_semantic);
hipError_t launch_k1c_bilateral(suma_ctx* c, float4* vertex);
hipError_t launch_gn_init(suma_ctx* c, const GnChain& ch);
hipError_t launch_icp_iteration(suma_ctx* c, const GnChain& ch, int eval_only, int pixel);
const GnState* gn_result(suma_ctx* c);
/* k_render.hip */
hipError_t launch_map_render(suma_ctx* c, const float* pose_old, const float* pose_new, float conf_threshold,
                             suma_frame* out);
hipError_t launch_map_render_single(suma_ctx* c, const float* pose, float conf_threshold, int active, int fuse_k7,
                                    suma_frame* mirror);
hipError_t launch_map_render_composed(suma_ctx* c, const float* pose_old, const float* pose_new,
                                      float conf_threshold);
/* k_update.hip */
/* ex: optional centre (x, y) + half-width of the submap tile that will be extracted right after this update;
 * fused_slot >= 0: the update performs that extraction itself, into this slot of the cache table */
hipError_t launch_map_update(suma_ctx* c, const float* pose, const float* inv_pose, const suma_frame* f, float cx,
                             float cy, float extent, int k7_done, const float* ex, int fused_slot);
hipError_t launch_clear_index_zbuf(suma_ctx* c);
K8Out launch_k8_out(suma_ctx* c);
hipError_t launch_set_poses(suma_ctx* c, const float* d_src, uint32_t first, uint32_t n);
hipError_t launch_fill_identity_poses(suma_ctx* c);
hipError_t launch_extract(suma_ctx* c, uint32_t slot, float cx, float cy, float extent, int use_flags);
hipError_t launch_append_cached(suma_ctx* c, uint32_t slot);

/* k_sync.hip: in-memory hand-offs between the ctx stream and the side stream.  A runtime event dependency between two
 * HIP streams costs ~10 us of stall on this platform (tools/xstream.hip: ping-pong 42 us vs 22 us for the same two
 * 10 us kernels on one stream); a one-wave gate kernel that polls a sequence word costs ~2 us. */
hipError_t launch_signal(suma_ctx* c, hipStream_t st, uint32_t word, uint32_t seq);
hipError_t launch_gate(suma_ctx* c, hipStream_t st, uint32_t word, uint32_t seq);
/* makes the ctx stream wait for the pending preprocessing hand-off (one-wave gate kernel) */
hipError_t flush_gate(suma_ctx* c);

/* k_checkpoint.hip (the image and the kernels are specified there).  Spans are in units of 16 bytes. */
hipError_t launch_kc_pack(suma_ctx* c, const WorldSpan* d_spans, uint32_t n_spans, uint32_t n_quads, void* d_dst,
                          unsigned long long* d_digest);
hipError_t launch_kc_verify(suma_ctx* c, const void* d_src, uint64_t bytes, unsigned long long* d_digest);
/* counters: n_updated, n_kept_updated, n_data, n_kept_data */
hipError_t launch_kc_unpack(suma_ctx* c, const void* d_tiles, uint32_t n_parked, const void* d_tile_dir, uint32_t n_tiles,
                            uint32_t n_active, const uint32_t counters[4]);

/* k_posegraph.hip: a graph's poses where they lie (12 doubles a node, R row-major | t) */
const double* posegraph_host_poses(const suma_posegraph* g, uint32_t* n);
const double* posegraph_device_poses(const suma_posegraph* g, uint32_t* n);
const double* posegraph_host_initial(const suma_posegraph* g, uint32_t* n);
/* replaces a graph's nodes by n nodes with these initial values and current estimates (12 doubles a node); to_device:
 * also prepares the device side, so that posegraph_device_poses holds `result` (a restored optimisation result) */
int posegraph_install_nodes(suma_posegraph* g, const double* initial12, const double* result12, uint32_t n, bool to_device);
/* k_loop.hip: integrateLoopClosures' pose table (SurfelMapping.cpp:219-233) written on the ctx stream: rows < n_opt =
 * float(opt), rows n_opt .. n_opt + n_tail - 1 = float(difference * tail) */
hipError_t launch_loop_integrate(suma_ctx* c, const double* d_opt12, uint32_t n_opt, const double* d_tail16,
                                 uint32_t n_tail, const double difference[16]);
/* suma_loop.hip: the loop-closing state of a pipeline (NULL: off) and its three hooks */
struct LoopState;
int loop_integrate(suma_pipeline* s);               /* integrateLoopClosures, at the start of every begin_scan */
int loop_odometry_edge(suma_pipeline* s);           /* SurfelMapping.cpp:461-471, at the end of updatePose */
int loop_check(suma_pipeline* s);                   /* checkLoopClosure */
void loop_destroy(suma_pipeline* s);                /* joins the worker, frees the graph */
int loop_reset(suma_pipeline* s);                   /* the constructor's state */
/* checkpoint (suma_checkpoint.hip): the LOOP / GRAPH / OPT payloads of checkpoint_format.h.  join: waits for a running
 * optimisation; write: appends the payloads (opt stays empty when none is in flight); check: everything that can refuse
 * the payloads, without touching the pipeline; install: on a pipeline whose loop closing has just been enabled with the
 * stored parameters */
void loop_ckpt_join(suma_pipeline* s);
uint64_t loop_ckpt_sizes(const suma_pipeline* s, uint64_t* graph_bytes, uint64_t* opt_bytes);
int loop_ckpt_write(suma_pipeline* s, std::vector<char>* loop, std::vector<char>* graph, std::vector<char>* opt);
int loop_ckpt_check(suma_ctx* c, const char* loop, const char* graph, const char* opt, uint32_t timestamp,
                    suma_loop_params* params);
int loop_ckpt_install(suma_pipeline* s, const char* loop, const char* graph, const char* opt);

/* k_group.hip: records grouped by a key, for the world export, the novelty fusion and the localiser's binning.  Every
 * entry enqueues on st, in the caller's arrays and in the caller's temporary block of tmp_bytes >= group_tmp_bytes(n);
 * current() of each pair is the sorted array afterwards. */
/* sorts == false: only group_scan will be called */
hipError_t group_tmp_bytes(uint32_t n, bool sorts, hipStream_t st, size_t* bytes);
/* stable sort of (key, idx) by the low key_bits of key */
hipError_t group_sort(void* tmp, size_t tmp_bytes, rocprim::double_buffer<unsigned long long>& key,
                      rocprim::double_buffer<uint32_t>& idx, uint32_t n, unsigned key_bits, hipStream_t st);
/* stable sort of (val, idx) by value_bits of val; key.current()[j] = key0[idx[j]] (key0 may be key's other half); stable
 * sort of (key, idx) by key_bits: idx is then ordered by (key, val, its order on entry) */
hipError_t group_sort_by_value_then_key(void* tmp, size_t tmp_bytes, rocprim::double_buffer<uint32_t>& val,
                                        unsigned value_bits, const unsigned long long* key0,
                                        rocprim::double_buffer<unsigned long long>& key, unsigned key_bits,
                                        rocprim::double_buffer<uint32_t>& idx, uint32_t n, hipStream_t st);
/* pos = the exclusive prefix sum of flag */
hipError_t group_scan(void* tmp, size_t tmp_bytes, const uint32_t* flag, uint32_t* pos, uint32_t n, hipStream_t st);
/* flag[j] = 1 where a run of sorted keys begins (keys[j] != no_key, and j == 0 or keys[j - 1] != keys[j]), then
 * group_scan: pos = the run's rank */
hipError_t group_heads(void* tmp, size_t tmp_bytes, const unsigned long long* keys, unsigned long long no_key,
                       uint32_t* flag, uint32_t* pos, uint32_t n, hipStream_t st);

/* k_grid.hip (the specification is there): the traversability grid of world-frame records.  Both enqueue on c->stream. */
enum { GRID_DROPPED = 0, GRID_OUTSIDE, GRID_OCCUPIED, GRID_FREE, GRID_OBSTACLE, GRID_NO_GROUND, GRID_FILLED,
       GRID_FIT_MIN_X, GRID_FIT_MIN_Y, GRID_FIT_MAX_X, GRID_FIT_MAX_Y, GRID_COUNTERS = 16 };
#define GRID_SCRATCH_PER_RECORD 48u
/* the caller has grown c->world_scratch to GRID_SCRATCH_PER_RECORD * n bytes, c->world_tmp to group_tmp_bytes(n, true),
 * c->grid_runs to width * height entries and c->grid_counters to GRID_COUNTERS words (zeroed here) */
hipError_t launch_grid(suma_ctx* c, const suma_grid_params& gp, const suma_world_surfel* d_records, uint32_t n,
                       suma_grid_cell* d_cells);
/* c->grid_counters[GRID_FIT_*] = the extent of the finite records as ordered integers (grid_ordered_float inverts them);
 * MIN_X stays 0xffffffff when there is none */
hipError_t launch_grid_fit(suma_ctx* c, const suma_world_surfel* d_records, uint32_t n);
float grid_ordered_float(uint32_t o);
/* suma_grid.hip: SUMA_OK, or SUMA_ERR_INVALID with "who: ..." for a raster or a rule outside the ranges of suma_grid_params */
int grid_check_params(suma_ctx* c, const std::string& who, const suma_grid_params& gp);

/* k_plan.hip (the specification is there): clearance, cost-to-go field and paths on the traversability grid.  All enqueue
 * on c->stream; only launch_plan_relax waits, once per batch of rounds, for the batch's flags. */
enum { PLAN_BLOCKED = 0, PLAN_TRAVERSABLE, PLAN_REACHED, PLAN_GOALS_IGNORED, PLAN_MAX_COST, PLAN_ROUND_FLAGS = 8,
       PLAN_ROUND_BATCH = 8, PLAN_COUNTERS = 16 };
#define PLAN_TILE 32u /* the relaxation's tile: PLAN_TILE x PLAN_TILE cells a block, one cell of halo */
#define PLAN_SCRATCH_PER_CELL 21u
/* bytes of c->plan_scratch for a raster: PLAN_SCRATCH_PER_CELL a cell (each array 16-byte aligned) and two flags a tile */
size_t plan_scratch_bytes(uint32_t width, uint32_t height);
/* classify, clearance, edges, goals (c->plan_io holds n_goals cell indices): everything in front of the relaxation;
 * zeroes c->plan_counters (PLAN_COUNTERS words) and starts every cell of d_field */
hipError_t launch_plan_prepare(suma_ctx* c, const suma_grid_params& gp, const suma_plan_params& pp, const suma_grid_cell* d_cells,
                               uint32_t n_goals, suma_plan_cell* d_field);
/* rounds until one changes nothing; SUMA_OK, SUMA_ERR_HIP, or SUMA_ERR_CAPACITY at the bound of width * height rounds */
int launch_plan_relax(suma_ctx* c, const suma_grid_params& gp, uint32_t* n_rounds);
hipError_t launch_plan_next(suma_ctx* c, const suma_grid_params& gp, suma_plan_cell* d_field);
/* c->plan_io: 4 words a result, then the n_starts cell indices (0xffffffff: outside), then n_starts * capacity path cells */
hipError_t launch_plan_walk(suma_ctx* c, const suma_grid_params& gp, const suma_plan_cell* d_field, uint32_t n_starts,
                            uint32_t capacity);

/* k_localize.hip (the specification is there): the world map binned into submap tiles, and the window gather */
struct LocTile { /* one occupied tile of the directory, ascending by key */
  unsigned long long key;
  uint32_t start, count; /* its records in LocMap.sorted */
};
struct LocSpan { /* one tile of a window: count records from sorted[src] to the active buffer at dst */
  uint32_t src, dst, count, pad;
};
struct LocMap {
  DevBuf<float4> sorted;    /* 3 float4 a record: the kept records by (key, source index) */
  std::vector<LocTile> dir; /* the host's copy of the directory */
  uint32_t n_kept = 0, n_dropped = 0;
  DevBuf<LocSpan> spans;    /* the span table of the last gather */
  /* change evidence (k_change.hip), only in a map binned with keep_evidence: one zeroed word per sorted record, and the
   * sort's source index (4 bytes a record), which a map without evidence gives back */
  bool has_evidence = false;
  uint32_t n_total = 0;     /* records of the caller's array, dropped ones included */
  DevBuf<suma_change_evidence> evidence;
  DevBuf<uint32_t> src_idx;
};
/* bins n device records (only read) into *m on the ctx stream; blocking.  A failure leaves *m as it was */
int localize_bin(suma_ctx* c, const suma_world_surfel* d_records, uint32_t n, LocMap* m, bool keep_evidence = false);
/* the window's tiles looked up in the directory: spans ascending by (i, then j), *total = records */
void localize_window_spans(const LocMap& m, int32_t oi, int32_t oj, int32_t dim, std::vector<LocSpan>* spans,
                           uint64_t* total);
/* spans -> the ctx's active surfel buffer, DevState.n_surfels = total; total <= max_surfels is the caller's check */
int localize_gather(suma_ctx* c, LocMap* m, const std::vector<LocSpan>& spans, uint32_t total);
/* the cell (i, j) of a position; false: non-finite or outside the grid */
bool localize_cell(float extent, float x, float y, float z, int32_t* i, int32_t* j);

/* k_change.hip (the specification is there): one observation of frame f at pose T over the first `total` window records
 * of the span table in m.spans, totals added to the 9 words at d_totals; and m's evidence into source order, into a zeroed
 * block of m.n_total words */
hipError_t launch_kc_observe(suma_ctx* c, const LocMap& m, uint32_t n_spans, uint32_t total, const suma_frame* f,
                             const double T[16], const suma_change_params& cp, uint32_t* d_totals);
hipError_t launch_kc_scatter(suma_ctx* c, const LocMap& m, suma_change_evidence* d_out);

/* k_novel.hip (the specification is there): the candidates a localiser collects beside its map */
struct NovelState {      /* device resident: no collection needs a host round trip */
  uint32_t count;        /* candidates held */
  uint32_t n_overflow;   /* novel texels that did not fit */
  uint32_t done;         /* blocks of kn_emit that have finished; back to 0 when the launch ends */
  uint32_t pad;
  uint32_t counts[8];    /* suma_novel_counts of the last collection */
};
struct Novel {
  bool on = false;
  suma_novel_params np;
  DevBuf<float4> cand;           /* 3 float4 a candidate, np.max_candidates of them */
  DevBuf<uint8_t> mark, flag;    /* one byte a texel of the data image */
  DevBuf<uint32_t> block_counts; /* kn_collect's counts, 8 words a block of 256 texels */
  DevBuf<NovelState> state;
  DevBuf<char> scratch, tmp;     /* the fusion's arrays and rocPRIM's temporary storage */
  DevBuf<float4> fused;          /* the fusion's output on its way to the host */
  DevBuf<uint32_t> fused_views;
};
/* one collection of frame f at pose T over the first `total` window records of the span table in m.spans, enqueued */
int novel_collect(suma_ctx* c, Novel& nv, const LocMap& m, uint32_t n_spans, uint32_t total, const suma_frame* f,
                  const double T[16], uint32_t scan_id);
/* candidates 0 .. n - 1 fused into d_out / d_views (device, capacity records); blocking.  counters_h: three words of the
 * caller's pinned block, which hold n_dropped, n_voxels, n_out when the call returns */
int novel_fuse(suma_ctx* c, Novel& nv, uint32_t n, const suma_novel_fuse_params& fp, suma_world_surfel* d_out,
               uint32_t* d_views, uint32_t capacity, uint32_t* counters_h);

/* k_objects.hip (the specification is there): the objects of one scan's unexplained texels */
struct ObjAcc { /* what the members of a component add up at their root, 96 bytes */
  uint32_t n, n_dyn, obj, rmin;           /* members, dynamic members, the object number (or none), ordered r_min */
  uint32_t mn[3], pad0, mx[3], pad1;      /* the box as ordered integers */
  unsigned long long S[3], sum_all, best; /* centroid sums (int64), the vote's total, its best sum << 9 | 511 - label */
  unsigned long long pad2;
};
struct Objects {
  bool on = false;
  suma_object_params op;
  uint32_t n_texels = 0;         /* of the data image the blocks below were made for */
  int32_t segmented = 0;         /* the blocks hold a segmentation */
  DevBuf<uint32_t> label;        /* one a texel: a member's root, or none */
  DevBuf<ObjAcc> acc;            /* one a texel, used at roots */
  DevBuf<uint32_t> hkey;         /* the vote table, two slots a texel: root * 512 + label + 1 */
  DevBuf<unsigned long long> hsum;
  DevBuf<uint32_t> block_counts; /* kob_vote's counts, 4 words a block of 256 texels */
  DevBuf<uint32_t> state;        /* suma_object_counts of the last segmentation */
  DevBuf<float4> rec;            /* 4 float4 a record, op.max_objects of them */
  DevBuf<uint32_t> ids;
  DevBuf<uint8_t> flags_in;      /* suma_localizer_segment_flags' flag image */
};
/* the blocks for P texels and op.max_objects records; the caller has drained the stream */
int objects_alloc(suma_ctx* c, Objects& ob, const suma_object_params& op, uint32_t P);
/* one segmentation of frame f's flagged texels (d_flags: P bytes on the device) at pose T, enqueued */
int objects_segment(suma_ctx* c, Objects& ob, const suma_frame* f, const uint8_t* d_flags, const double T[16],
                    uint32_t scan_id);

/* k_live.hip (the specification is there): the live obstacle layer over a static traversability grid */
enum { LIVE_COUNT_WORDS = 10, LIVE_ANY_HIT = 10, LIVE_STAT_WORDS = 4, LIVE_STATS = 12, LIVE_WORDS = 16 };
struct Live {
  bool on = false;
  suma_live_params lp;
  suma_grid_params gp;
  uint32_t n_cells = 0;
  uint32_t last_stamp = 0;       /* of the last update; 0: none */
  int32_t updated = 0;           /* words 0 .. 9 hold an update's counts */
  DevBuf<float4> cells;          /* the static cells, 3 float4 a cell */
  DevBuf<float> ground;          /* their ground_z, what the rays read */
  DevBuf<suma_live_cell> state;
  DevBuf<uint32_t> words;        /* LIVE_WORDS: the counts of the last update, "some cell has a hit", a compose's stats */
  DevBuf<uint8_t> flags_in;      /* suma_localizer_live_update_flags' flag image, without objects */
};
/* the blocks for gp's raster, the static cells copied from d_cells, the state zeroed; blocking */
int live_alloc(suma_ctx* c, Live& lv, const suma_grid_params& gp, const suma_grid_cell* d_cells);
/* state and words to zero, enqueued */
int live_clear(suma_ctx* c, Live& lv);
/* one update with stamp s of frame f's flagged texels (d_flags: one byte a texel; d_ids: the segmentation's id image, or
 * NULL without objects) at pose T, enqueued: the hits, then the carve */
int live_update(suma_ctx* c, Live& lv, const suma_frame* f, const uint8_t* d_flags, const uint32_t* d_ids, const double T[16],
                uint32_t s);
/* the composed cells and the mask (or NULL) into the caller's device blocks, the stats into words LIVE_STATS ..; enqueued */
int live_compose(suma_ctx* c, Live& lv, suma_grid_cell* d_out, uint8_t* d_mask);

/* k_tracks.hip (the specification is there): the objects of the scans tied together */
enum { TRK_COUNT_WORDS = 12, TRK_N_LIVE = 12, TRK_BORN_TOTAL = 13, TRK_N_IN = 14, TRK_WORDS = 16 };
struct TrkAcc { /* what the objects of a detection add up at their root, 80 bytes */
  uint32_t count, rmin;                 /* members, ordered r_min */
  uint32_t mn[3], mx[3];                /* the box as ordered integers */
  unsigned long long ntex, ndyn, W, S[3]; /* sums of n_texels, n_dynamic and the weights; centroid sums (int64) */
};
struct Tracks {
  bool on = false;
  suma_track_params tp;
  uint32_t max_objects = 0;      /* of the segmentation the blocks below were made for */
  uint32_t last_stamp = 0;       /* of the last update; 0: none */
  int32_t updated = 0;           /* out, objtrack and words 0 .. 12 hold an update's results */
  DevBuf<uint32_t> parent;       /* one an object: its root */
  DevBuf<TrkAcc> acc;            /* one an object, used at roots */
  DevBuf<uint32_t> det;          /* 16 words a detection */
  DevBuf<uint32_t> objdet, objtrack, detmatch, dettrack;
  DevBuf<unsigned long long> detpick;
  DevBuf<float4> rec_in;         /* suma_localizer_track_objects' records */
  DevBuf<suma_object_track> slots, out;
  DevBuf<uint32_t> words;        /* TRK_WORDS: the counts of the last update, its live tracks, births since the clear, n of rec_in */
};
/* the blocks for max_objects objects and tp.max_tracks slots, cleared; the caller has drained the stream */
int tracks_alloc(suma_ctx* c, Tracks& tk, const suma_track_params& tp, uint32_t max_objects);
/* no tracks, last stamp 0, next id 1; enqueued */
int tracks_clear(suma_ctx* c, Tracks& tk);
/* one update with stamp s (above tk.last_stamp: the caller has checked) of the records at d_rec, *d_n of them (a device
 * word), enqueued */
int tracks_update(suma_ctx* c, Tracks& tk, const float4* d_rec, const uint32_t* d_n, uint32_t s);

/* k_deskew.hip (the specification is there): what kd_deskew receives by value -- the twist of one sweep, made once on the
 * host in fp64 (deskew_twist) and rounded to fp32 */
#define SUMA_DESKEW_SMALL_THETA 1e-6
struct DeskewArgs {
  float v[3], a[3], b[3], c[3]; /* scale * v0, the unit axis, a x v, a x (a x v) */
  float theta, inv_theta;       /* both 0 for a pure translation */
  float t_ref, start_azimuth;
  int32_t clockwise, use_times;
};
bool deskew_is_identity(const double motion[16]);
void deskew_twist(const suma_deskew_params& dp, const double motion[16], DeskewArgs* out);
hipError_t launch_kd_deskew(hipStream_t st, const float4* in, const float* times, uint32_t n, const DeskewArgs& a,
                            float4* out);
/* suma_deskew.hip: the correction a pipeline or a localiser applies to its scans */
struct Deskew {
  bool on = false;
  suma_deskew_params dp;
  bool have_override = false; /* suma_*_set_deskew_motion: one shot, for the next scan */
  double override_motion[16];
  double last_motion[16];     /* what the last scan used */
  int32_t last_source = 0;    /* SUMA_DESKEW_MOTION_* */
  DevBuf<float4> points;      /* the corrected scan: the caller's buffer is never written */
};
/* sets c->err; for_scans: the entries that take no times (pipeline, localiser) refuse the times source */
int deskew_params_check(suma_ctx* c, const suma_deskew_params* dp, bool for_scans, const char* who);
/* the motion of the next scan (the override once, else `increment`), noted in dk as the last one used; then n points at
 * d_in corrected into dk.points on stream st, *d_out = the points K1 reads: d_in itself for the identity motion (nothing is
 * launched).  Growing dk.points waits for both streams of c -- only when a larger scan than any before arrives */
int deskew_scan(suma_ctx* c, Deskew& dk, const double increment[16], hipStream_t st, const suma_float4* d_in, uint32_t n,
                const suma_float4** d_out);
void deskew_destroy(suma_pipeline* s);
/* the entries that hand a scan over before the previous pose exists have no motion to use */
#define SUMA_REFUSE_WHILE_DESKEW(s, who)                                                                        \
  do {                                                                                                           \
    if ((s) && (s)->deskew && (s)->deskew->on)                                                                   \
      return fail((s)->c, SUMA_ERR_INVALID, who ": not while motion compensation is enabled (the scan is handed " \
                                                 "over before the previous pose exists; suma_pipeline_disable_deskew)"); \
  } while (0)

/* k_place.hip (the specification is there): what kp_describe reads of suma_place_params, with the two quotients made
 * once on the host and the label mask as bits */
struct PlaceArgs {
  uint32_t R, S;
  float max_range, height_offset;
  float ring_scale;   /* (float)R / max_range */
  float sector_scale; /* (float)S / (2.0f * SUMA_PI_F) */
  uint32_t keep[(SUMA_DRAW_COLORS + 31) / 32];
};
/* zeroes the entry (S*R cells + S norms), then cells and norms of frame f into it */
hipError_t launch_kp_describe(hipStream_t st, const suma_frame* f, const PlaceArgs& a, float* entry);
hipError_t launch_kp_norms(hipStream_t st, float* entries, uint32_t n_entries, uint32_t S, uint32_t R);
/* per entry: the least distance over the shifts and the shift */
hipError_t launch_kp_search(hipStream_t st, const float* db, uint32_t n_entries, const float* q, uint32_t S, uint32_t R,
                            float* dist, int32_t* shift);
/* the K best by (dist, index) outside the id window into out (yaw left 0), *n_out = how many */
hipError_t launch_kp_topk(hipStream_t st, const float* dist, const int32_t* shift, const uint32_t* ids, uint32_t n_entries,
                          uint32_t lo, uint32_t hi, uint32_t K, suma_place_match* out, uint32_t* n_out);
/* suma_place.hip: the pose hypothesis of a match, T_entry * Rz(yaw), in mat4_mul's operation order with
 * sdm_cos_d / sdm_sin_d of (double)yaw */
void place_hypothesis(const double T_entry[16], float yaw, double out[16]);

/* suma_api.hip: suma_icp_set_data + suma_icp_minimize on the given frames with processScan's fixed-iteration override
 * (fixed_iterations > 0: exactly that many iterations, no stopping test) */
int icp_minimize_frames(suma_ctx* c, const suma_frame* current, const suma_frame* model, const double T0[16],
                        int32_t fixed_iterations, double T_out[16], suma_icp_stats* stats);

/* host helper shared by api + pipeline */
void rigid_inverse_f(const float* m, float* out);

/* host-side 4 x 4 double matrices, column-major (suma_api.hip, suma_runner.hip).  Every product has the one fixed
 * operation order all ranks use, ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (distributed.py mul4). */
static inline void mat4_eye(double* T) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}
/* C = A * B */
static inline void mat4_mul(const double* A, const double* B, double* C) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      C[4 * c + r] = ((A[r] * B[4 * c] + A[4 + r] * B[4 * c + 1]) + A[8 + r] * B[4 * c + 2]) + A[12 + r] * B[4 * c + 3];
}
static inline void mat4_rigid_inv(const double* m, double* out) {
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) out[4 * c + r] = m[4 * r + c];
  for (int r = 0; r < 3; ++r) out[12 + r] = -((m[4 * r] * m[12] + m[4 * r + 1] * m[13]) + m[4 * r + 2] * m[14]);
  out[3] = out[7] = out[11] = 0.0;
  out[15] = 1.0;
}
/* makes the rotation of a pose orthonormal again, in one fixed operation order (tests/localize_host.py orthonormalize):
 * Gram-Schmidt on its columns -- c0 normalised, c1 made orthogonal to c0 and normalised, c2 = c0 x c1; the translation
 * is kept, the last row becomes 0 0 0 1.  A recursion that inverts poses by mat4_rigid_inv needs it: the transpose is
 * the inverse of an orthonormal rotation only, and what is missing is fed back (suma_localize.hip) */
static inline void mat4_orthonormalize(double* T) {
  double a[3] = {T[0], T[1], T[2]}, b[3] = {T[4], T[5], T[6]};
  double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  for (int r = 0; r < 3; ++r) a[r] = a[r] / n;
  const double d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
  for (int r = 0; r < 3; ++r) b[r] = b[r] - d * a[r];
  n = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  for (int r = 0; r < 3; ++r) b[r] = b[r] / n;
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  for (int r = 0; r < 3; ++r) T[r] = a[r], T[4 + r] = b[r], T[8 + r] = c[r];
  T[3] = T[7] = T[11] = 0.0;
  T[15] = 1.0;
}
static inline void mat4_cast_f(const double* T, float* out) {
  for (int i = 0; i < 16; ++i) out[i] = (float)T[i];
}

#endif
