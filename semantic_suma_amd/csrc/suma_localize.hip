/*
 * suma_localize.hip -- localisation of scans in a finished world map, without changing it (include/suma_hip.h,
 * suma_localizer_*).  Host code: a localiser is a suma_ctx of its own whose active surfel buffer holds a window of the
 * binned world map (k_localize.hip states the specification), one data frame, and the pose bookkeeping below.  One scan
 * is the composition the loop-closure verification uses (SurfelMapping.cpp:546-558): render the inactive map from the
 * predicted pose, minimise the scan against it from identity, gate on the objective's counters -- through the library's
 * own entries (suma_preprocess*, suma_map_render_inactive, icp_minimize_frames), which is all the device work there is
 * besides the window gather.  4x4 products and rigid inverses are mat4_mul / mat4_rigid_inv, the library's one fixed
 * operation order; tests/localize_host.py is the same sequence over the CPU oracle.
 */
#include <math.h>
#include <string.h>

#include <cmath>
#include <new>
#include <vector>

#include "suma_internal.h"

enum { STAGE_WORDS = 16 };

struct suma_localizer {
  suma_ctx* c = nullptr;
  suma_frame* frame = nullptr; /* the scan, K1-K3 */
  PinnedBuf<uint32_t> stage_h; /* STAGE_WORDS: whatever few device words a call reads back, on their way to the host */
  suma_localizer_params lp;
  LocMap map;
  bool have_map = false, have_pose = false, first = true;
  double pose[16], increment[16];
  int32_t oi = 0, oj = 0;
  uint32_t n_window = 0, rebuilds = 0;
  std::vector<LocSpan> spans;
  /* change evidence (k_change.hip): wanted from the next set_map on; the map says whether it has it */
  bool ev_wanted = false;
  suma_change_params cp;
  DevBuf<uint32_t> ev_totals;             /* the nine totals of one observation */
  DevBuf<suma_change_evidence> ev_source; /* the evidence in source order, made by every download */
  suma_change_counts last_counts;
  int32_t last_observed = 0;
  /* novelty (k_novel.hip): the candidates beside the map */
  Novel nv;
  uint32_t scan_count = 0;     /* process_scan calls since the last set_map */
  int32_t last_collected = 0;
  /* objects (k_objects.hip): the segmentation behind every collection */
  Objects ob;
  /* the live obstacle layer (k_live.hip): one update behind every collection and its segmentation */
  Live lv;
  /* tracks (k_tracks.hip): one update behind every segmentation */
  Tracks tk;
  /* motion compensation (k_deskew.hip): the correction of process_scan's points, and the staging of a host scan that is
   * corrected (an uncorrected one goes through suma_preprocess's own staging) */
  Deskew dk;
  DevBuf<float4> dk_points;
  DevBuf<float> dk_labels, dk_probs;
};

namespace {

bool finite16(const double* T) {
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(T[k])) return false;
  return true;
}

/* ---- the decisions every layer's entries share, each stated once ---- */

/* what a caller's frame and pose must satisfy before a layer reads them */
int frame_pose_check(suma_localizer* l, const suma_frame* frame, const double* T, const char* who) {
  suma_ctx* c = l->c;
  if (!frame || !T) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  if (frame->ctx != c) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": the frame belongs to another ctx");
  if (frame->width != c->p.data_width || frame->height != c->p.data_height)
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": the frame must have the data image's size");
  if (!finite16(T)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": non-finite pose");
  return SUMA_OK;
}

/* in front of the first launch that reads frame f on the ctx stream: an earlier suma_preprocess on the side stream comes
 * first, and the frame counts as used */
int frame_read_begin(suma_ctx* c, const suma_frame* f) {
  if (c->gate_pending) HIP_TRY(c, flush_gate(c));
  const_cast<suma_frame*>(f)->last_access = ++c->enq_seq;
  return SUMA_OK;
}

/* a few words (at most STAGE_WORDS) at d_src into host words, blocking: through the localiser's one pinned block */
int read_words(suma_localizer* l, const void* d_src, size_t bytes, void* out) {
  suma_ctx* c = l->c;
  HIP_TRY(c, hipMemcpyAsync(l->stage_h, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(out, l->stage_h.p, bytes);
  return SUMA_OK;
}
static_assert(sizeof(NovelState) <= STAGE_WORDS * 4 && LIVE_WORDS <= STAGE_WORDS && TRK_WORDS <= STAGE_WORDS &&
              sizeof(suma_change_counts) <= STAGE_WORDS * 4 && sizeof(suma_object_counts) <= STAGE_WORDS * 4,
              "the largest read-back fits the pinned block");

/* a capacity-bounded download: *n is the total whatever the capacity, the first min(total, capacity) elements of d_src
 * go to out (a device block, or host memory), blocking.  What a site reports beyond that -- an overflow, after the
 * outputs are filled -- is the site's */
int download(suma_ctx* c, void* out, uint32_t capacity, uint32_t* n, const void* d_src, uint32_t total, size_t elem_bytes,
             bool to_device) {
  *n = total;
  const uint32_t m = total < capacity ? total : capacity;
  if (!m) return SUMA_OK;
  HIP_TRY(c, hipMemcpyAsync(out, d_src, (size_t)m * elem_bytes, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SUMA_OK;
}

/* an update's stamp must lie above the last one's */
int stamp_check(suma_localizer* l, uint32_t scan_id, uint32_t last_stamp, const char* whose, const char* who) {
  const uint32_t s = scan_id + 1u;
  if (s > last_stamp) return SUMA_OK;
  return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": scan_id " + std::to_string(scan_id) + " gives " + whose + " the stamp " +
                                      std::to_string(s) + ", not above the last update's " + std::to_string(last_stamp));
}

/* the stamps of every layer run_layers will update, checked in front of everything the call launches or writes: a
 * refusal leaves all layers as they were.  with_live: the entry updates the live layer (suma_hip.h) */
int stamps_check(suma_localizer* l, uint32_t scan_id, const char* who, bool with_live) {
  int r = SUMA_OK;
  if (with_live && l->lv.on) r = stamp_check(l, scan_id, l->lv.last_stamp, "the live layer", who);
  if (!r && l->tk.on) r = stamp_check(l, scan_id, l->tk.last_stamp, "the tracks", who);
  return r;
}

/* what runs behind a flag image (d_flags: one byte a texel, on the device) of frame f at pose T, enqueued on the ctx
 * stream in this order: with objects on, the segmentation; with tracks on, their update behind it; with with_live and
 * the live layer on, its update behind all.  The caller has passed stamps_check and frame_read_begin.  ob.segmented is
 * set as soon as the segmentation is enqueued, whatever fails behind it */
int run_layers(suma_localizer* l, const suma_frame* f, const uint8_t* d_flags, const double T[16], uint32_t scan_id,
               bool with_live) {
  suma_ctx* c = l->c;
  Objects& ob = l->ob;
  int r = SUMA_OK;
  if (ob.on) {
    if ((r = objects_segment(c, ob, f, d_flags, T, scan_id))) return r;
    ob.segmented = 1;
    /* word 5: the objects stored */
    if (l->tk.on && (r = tracks_update(c, l->tk, ob.rec, ob.state.p + 5, scan_id + 1u))) return r;
  }
  if (with_live && l->lv.on) r = live_update(c, l->lv, f, d_flags, ob.on ? ob.ids.p : nullptr, T, scan_id + 1u);
  return r;
}

/* which layer is made of which: novelty's flags feed the objects and the live layer, the objects' records feed the
 * tracks (the enables refuse a layer whose source is off).  A layer's blocks go with those of everything made of it; the
 * caller has drained the stream */
enum Layer { LAYER_NOVELTY, LAYER_OBJECTS, LAYER_LIVE, LAYER_TRACKS };
void release_layer(suma_localizer* l, Layer which) {
  const bool novelty = which == LAYER_NOVELTY, objects = novelty || which == LAYER_OBJECTS;
  if (novelty) l->nv = Novel();
  if (objects) l->ob = Objects();
  if (novelty || which == LAYER_LIVE) l->lv = Live();
  if (objects || which == LAYER_TRACKS) l->tk = Tracks();
}

bool layer_on(const suma_localizer* l, Layer which) {
  if (which == LAYER_NOVELTY) return l->nv.on;
  if (which == LAYER_OBJECTS) return l->ob.on;
  if (which == LAYER_LIVE) return l->lv.on;
  return l->tk.on;
}

/* a suma_localizer_disable_*: nothing when the layer is off */
int disable_layer(suma_localizer* l, Layer which) {
  if (!layer_on(l, which)) return SUMA_OK;
  HIP_TRY(l->c, hipStreamSynchronize(l->c->stream)); /* a scan's work may still write the blocks */
  release_layer(l, which);
  return SUMA_OK;
}

/* the last scan's results, as the entries report them: the observation (last_counts, last_observed), the collection
 * (last_collected) and the segmentation (ob.segmented: the objects' blocks hold one) */
enum { LAST_OBSERVATION = 1, LAST_COLLECTION = 2, LAST_SEGMENTATION = 4, LAST_ALL = 7 };
void forget_last(suma_localizer* l, unsigned what) {
  if (what & LAST_OBSERVATION) {
    memset(&l->last_counts, 0, sizeof(l->last_counts));
    l->last_observed = 0;
  }
  if (what & LAST_COLLECTION) l->last_collected = 0;
  if (what & LAST_SEGMENTATION) l->ob.segmented = 0;
}

/* the window around (oi, oj) into the ctx's active buffer; a window beyond max_surfels is refused before anything is
 * launched or written */
int gather_window(suma_localizer* l, int32_t oi, int32_t oj) {
  suma_ctx* c = l->c;
  uint64_t total = 0;
  std::vector<LocSpan> spans;
  localize_window_spans(l->map, oi, oj, c->p.submap_dimension, &spans, &total);
  if (total > c->p.max_surfels)
    return fail(c, SUMA_ERR_CAPACITY, "suma_localizer: the window around tile (" + std::to_string(oi) + ", " +
                                      std::to_string(oj) + ") holds " + std::to_string(total) + " records, max_surfels = " +
                                      std::to_string(c->p.max_surfels));
  int r = localize_gather(c, &l->map, spans, (uint32_t)total);
  if (r) return r;
  l->spans.swap(spans);
  l->oi = oi, l->oj = oj;
  l->n_window = (uint32_t)total;
  l->rebuilds += 1;
  return SUMA_OK;
}

/* one observation over the current window; counts may be NULL.  The caller has checked that the map has evidence */
int observe(suma_localizer* l, const suma_frame* f, const double T[16], suma_change_counts* counts) {
  suma_ctx* c = l->c;
  suma_change_counts out;
  memset(&out, 0, sizeof(out));
  if (l->n_window) {
    int r = grow(c, l->ev_totals, 9, {c->stream});
    if (r < 0) return r;
    if ((r = frame_read_begin(c, f))) return r;
    HIP_TRY(c, hipMemsetAsync(l->ev_totals, 0, 9 * sizeof(uint32_t), c->stream));
    {
      ProfScope ps(c, "change_observe", 64.0 * l->n_window + 48.0 * f->width * f->height);
      HIP_TRY(c, launch_kc_observe(c, l->map, (uint32_t)l->spans.size(), l->n_window, f, T, l->cp, l->ev_totals));
    }
    if ((r = read_words(l, l->ev_totals, sizeof(out), &out))) return r;
  }
  if (counts) *counts = out;
  return SUMA_OK;
}

/* one collection over the current window, enqueued on the ctx stream, and the layers behind its flags.  The caller has
 * forgotten the last collection and segmentation: a call that collects nothing leaves none */
int collect(suma_localizer* l, const suma_frame* f, const double T[16], uint32_t scan_id) {
  suma_ctx* c = l->c;
  if (!l->n_window) return SUMA_OK;
  int r = stamps_check(l, scan_id, "suma_localizer: the collection", true);
  if (r) return r;
  if ((r = frame_read_begin(c, f))) return r;
  r = novel_collect(c, l->nv, l->map, (uint32_t)l->spans.size(), l->n_window, f, T, scan_id);
  if (r) return r;
  return run_layers(l, f, l->nv.flag, T, scan_id, true);
}

/* NULL, or what is wrong with the values */
const char* change_params_why(const suma_change_params& q) {
  if (!(std::isfinite(q.free_margin) && q.free_margin > 0.0f)) return "free_margin must be finite and > 0";
  if (!(std::isfinite(q.min_view_cos) && q.min_view_cos >= 0.0f && q.min_view_cos < 1.0f)) return "min_view_cos must lie in [0, 1)";
  if (!(std::isfinite(q.max_range) && q.max_range > 0.0f)) return "max_range must be finite and > 0";
  return nullptr;
}

}  // namespace

extern "C" void suma_localizer_params_default(const suma_params* params, suma_localizer_params* lp) {
  if (!lp) return;
  lp->conf_threshold = params ? params->confidence_threshold : 0.0f;
  lp->min_valid_ratio = 0.2f; /* SurfelMapping.cpp:567 */
  lp->max_outlier_ratio = 0.85f;
  lp->constant_velocity = 1;
}

extern "C" int suma_localizer_create(const suma_params* params, const suma_localizer_params* lp, int hip_device,
                                     suma_localizer** out) {
  if (!params || !out) return SUMA_ERR_INVALID;
  *out = nullptr;
  suma_localizer_params q;
  suma_localizer_params_default(params, &q);
  if (lp) q = *lp;
  if (std::isnan(q.conf_threshold) || std::isnan(q.min_valid_ratio) || std::isnan(q.max_outlier_ratio))
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_localizer_create: a NaN threshold or ratio");
  if (params->submap_dimension < 0 || params->submap_dimension > 64)
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_localizer_create: submap_dimension must be 0 .. 64");
  if (!(params->submap_extent > 0.0f) || std::isinf(params->submap_extent))
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_localizer_create: submap_extent must be finite and > 0");
  if (params->active_timestamps < 91 || params->active_timestamps > 0x7fffffff - 10)
    return fail_without_ctx(SUMA_ERR_INVALID,
                            "suma_localizer_create: active_timestamps must be at least 91 (the inactive render selects "
                            "creation stamps below timestamp - 100)");
  suma_localizer* l = new (std::nothrow) suma_localizer();
  if (!l) return fail_without_ctx(SUMA_ERR_NOMEM, "out of host memory");
  int r = suma_ctx_create(params, hip_device, &l->c); /* leaves its text for suma_last_error(NULL) */
  if (r) {
    delete l;
    return r;
  }
  r = suma_frame_create(l->c, params->data_width, params->data_height, &l->frame);
  if (r) {
    fail_without_ctx(r, std::string("suma_localizer_create: ") + suma_last_error(l->c));
    suma_localizer_destroy(l);
    return r;
  }
  if (l->stage_h.alloc(STAGE_WORDS) != hipSuccess) {
    (void)hipGetLastError();
    suma_localizer_destroy(l);
    return fail_without_ctx(SUMA_ERR_NOMEM, "suma_localizer_create: no pinned memory for the read-back block");
  }
  l->lp = q;
  suma_change_params_default(&l->cp);
  memset(&l->last_counts, 0, sizeof(l->last_counts));
  l->c->timestamp = (uint32_t)params->active_timestamps + 10u; /* T_loc (k_localize.hip) */
  mat4_eye(l->pose);
  mat4_eye(l->increment);
  *out = l;
  return SUMA_OK;
}

extern "C" void suma_localizer_destroy(suma_localizer* l) {
  if (!l) return;
  if (l->c && l->c->stream) hipStreamSynchronize(l->c->stream);
  l->map = LocMap(); /* device blocks go before the ctx */
  l->ev_totals.reset(), l->ev_source.reset(), l->stage_h.reset();
  release_layer(l, LAYER_NOVELTY);
  l->dk.points.reset(), l->dk_points.reset(), l->dk_labels.reset(), l->dk_probs.reset();
  suma_frame_destroy(l->frame);
  suma_ctx_destroy(l->c);
  delete l;
}

extern "C" suma_ctx* suma_localizer_ctx(suma_localizer* l) { return l ? l->c : nullptr; }

extern "C" int suma_localizer_set_map_device(suma_localizer* l, const suma_world_surfel* d_records, uint32_t n,
                                             uint32_t* n_dropped) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (n && !d_records) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_map: NULL records with n > 0");
  if (n && ((uintptr_t)d_records & 15u)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_map: records must be 16-byte aligned");
  int r = localize_bin(c, d_records, n, &l->map, l->ev_wanted);
  if (r) return r;
  if (l->nv.on) HIP_TRY(c, hipMemsetAsync(l->nv.state, 0, sizeof(NovelState), c->stream));
  if (l->lv.on && (r = live_clear(c, l->lv))) return r;
  if (l->tk.on && (r = tracks_clear(c, l->tk))) return r;
  l->scan_count = 0;
  forget_last(l, LAST_ALL);
  l->have_map = true;
  l->have_pose = false;
  l->n_window = 0, l->rebuilds = 0;
  l->spans.clear();
  if (n_dropped) *n_dropped = l->map.n_dropped;
  return SUMA_OK;
}

extern "C" int suma_localizer_set_map(suma_localizer* l, const suma_world_surfel* host, uint32_t n, uint32_t* n_dropped) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (n && !host) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_map: NULL records with n > 0");
  DevBuf<suma_world_surfel> staged; /* given back when the call returns: the localiser keeps the binned copy only */
  if (n) {
    HIP_TRY(c, staged.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(staged, host, (size_t)n * sizeof(suma_world_surfel), hipMemcpyHostToDevice, c->stream));
  }
  const int r = suma_localizer_set_map_device(l, staged, n, n_dropped);
  hipStreamSynchronize(c->stream); /* nothing reads `staged` behind this */
  return r;
}

extern "C" int suma_localizer_set_pose(suma_localizer* l, const double T[16]) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!T) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_pose: NULL pose");
  if (!l->have_map) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_pose: no map (suma_localizer_set_map)");
  if (!finite16(T)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_pose: non-finite pose");
  int32_t i, j;
  if (!localize_cell(c->p.submap_extent, (float)T[12], (float)T[13], (float)T[14], &i, &j))
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_pose: the pose lies outside the tile grid");
  int r = gather_window(l, i, j);
  if (r) return r;
  memcpy(l->pose, T, sizeof(l->pose));
  mat4_eye(l->increment);
  l->have_pose = true;
  l->first = true;
  return SUMA_OK;
}

/* step 3 with motion compensation on: the points are corrected with the increment of the previous scan's step 7 (or the
 * one-shot override) in front of K1, all on the ctx stream; a host scan is staged in the localiser's own blocks first */
static int preprocess_deskewed(suma_localizer* l, const suma_float4* points, const float* labels, const float* probs,
                               uint32_t n, bool on_device) {
  suma_ctx* c = l->c;
  if (!on_device && n) {
    const size_t cap = (size_t)n + n / 4 + 1024;
    if (grow(c, l->dk_points, n, {c->stream}, cap) < 0 || (labels && grow(c, l->dk_labels, n, {c->stream}, cap) < 0) ||
        (probs && grow(c, l->dk_probs, n, {c->stream}, cap) < 0))
      return SUMA_ERR_HIP; /* grow has left its text in the ctx */
    HIP_TRY(c, hipMemcpyAsync(l->dk_points, points, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (labels) HIP_TRY(c, hipMemcpyAsync(l->dk_labels, labels, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (probs) HIP_TRY(c, hipMemcpyAsync(l->dk_probs, probs, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    points = (const suma_float4*)l->dk_points.p;
    if (labels) labels = l->dk_labels;
    if (probs) probs = l->dk_probs;
  }
  if (c->gate_pending) HIP_TRY(c, flush_gate(c)); /* an earlier suma_preprocess on the side stream comes first */
  int r = deskew_scan(c, l->dk, l->increment, c->stream, points, n, &points);
  if (r) return r;
  return suma_preprocess_device(c, points, labels, probs, n, c->timestamp, l->frame);
}

/* frame_ready: a candidate of a relocalisation -- K1-K3 are made, and a hypothesis observes nothing */
static int process_scan(suma_localizer* l, const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                        int32_t fixed_iterations, suma_localizer_result* res, bool on_device, bool frame_ready = false) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!res) return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: NULL result");
  if (n && !points) return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: NULL points with n > 0");
  if (!l->have_map) return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: no map (suma_localizer_set_map)");
  if (!l->have_pose) return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: no start pose (suma_localizer_set_pose)");
  memset(res, 0, sizeof(*res));
  /* 1. the predicted pose */
  double guess[16];
  if (l->lp.constant_velocity)
    mat4_mul(l->pose, l->increment, guess);
  else
    memcpy(guess, l->pose, sizeof(guess));
  if (!finite16(guess)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: the predicted pose is not finite");
  float gf[16];
  mat4_cast_f(guess, gf);
  /* 2. re-centre the window (updateActiveSubmaps' rule, SurfelMap.cpp:750-790) */
  {
    const float e = c->p.submap_extent, factor = 1.1f;
    const float cx = (float)(2.0 * l->oi * e), cy = (float)(2.0 * l->oj * e);
    const float changex = gf[12] - cx, changey = gf[13] - cy;
    int32_t oi = l->oi, oj = l->oj;
    if (fabsf(changex) > factor * e) oi += (changex < 0) ? -1 : 1;
    if (fabsf(changey) > factor * e) oj += (changey < 0) ? -1 : 1;
    if (oi != l->oi || oj != l->oj) {
      if (oi <= -1048576 || oi >= 1048576 || oj <= -1048576 || oj >= 1048576)
        return fail(c, SUMA_ERR_INVALID, "suma_localizer_process_scan: the predicted pose leaves the tile grid");
      int r = gather_window(l, oi, oj);
      if (r) return r;
      res->window_rebuilt = 1;
    }
  }
  double T_gn[16];
  mat4_eye(T_gn);
  bool minimised = false;
  suma_icp_stats st;
  memset(&st, 0, sizeof(st));
  if (l->n_window) {
    /* 3. K1-K3 at T_loc (a relocalisation has made them once for all its candidates) */
    int r = frame_ready  ? SUMA_OK
            : l->dk.on   ? preprocess_deskewed(l, points, labels, probs, n, on_device)
            : on_device  ? suma_preprocess_device(c, points, labels, probs, n, c->timestamp, l->frame)
                         : suma_preprocess(c, points, labels, probs, n, c->timestamp, l->frame);
    if (r) return r;
    /* 4. the model: the window seen from the guess */
    r = suma_map_render_inactive(c, gf, l->lp.conf_threshold);
    if (r) return r;
    /* 5. frame-to-model from identity */
    double I[16];
    mat4_eye(I);
    r = icp_minimize_frames(c, l->frame, c->old_frame, I, fixed_iterations, T_gn, &st);
    if (r) return r;
    minimised = finite16(T_gn);
  }
  /* 6, 7. */
  double pose[16], inv[16];
  if (minimised) {
    mat4_mul(guess, T_gn, pose);
    /* kept orthonormal: step 7 inverts the pose by transposition, and what a rotation lacks to be orthonormal would
     * come back in the next guess twice and once more (pose * pose_prev^T * pose): a factor of 2.4 per scan, from 1e-16
     * to a lost run within 40 scans */
    mat4_orthonormalize(pose);
    if (l->first) {
      mat4_eye(l->increment);
    } else {
      mat4_rigid_inv(l->pose, inv);
      mat4_mul(inv, pose, l->increment);
    }
  } else {
    /* nothing was minimised (empty window, or a chain that ended on a non-finite pose): pose = guess, and the increment
     * stays what it is -- rigid_inverse(pose_prev) * (pose_prev * increment) without the rounding */
    memcpy(pose, guess, sizeof(pose));
  }
  memcpy(l->pose, pose, sizeof(pose));
  l->first = false;

  memcpy(res->guess, guess, sizeof(guess));
  memcpy(res->pose, pose, sizeof(pose));
  memcpy(res->increment, l->increment, sizeof(l->increment));
  res->stats = st;
  res->valid_ratio = (float)st.valid / (float)(st.valid + st.invalid); /* closure_gate (suma_api.hip) */
  res->outlier_ratio = (float)st.outlier / (float)(st.outlier + st.inlier);
  res->tracked = ((double)res->valid_ratio > (double)l->lp.min_valid_ratio &&
                  (double)res->outlier_ratio < (double)l->lp.max_outlier_ratio) ? 1 : 0;
  res->origin_ij[0] = l->oi, res->origin_ij[1] = l->oj;
  res->n_window = l->n_window;
  /* 8. with evidence on: one observation of the scan's own frame at the final pose (k_change.hip) */
  if (l->map.has_evidence && !frame_ready) {
    forget_last(l, LAST_OBSERVATION);
    if (l->n_window && (res->tracked || !l->cp.tracked_only) && finite16(pose)) {
      int r = observe(l, l->frame, pose, &l->last_counts);
      if (r) return r;
      l->last_observed = 1;
    }
  }
  /* 9. with novelty on: one collection of the scan's own frame at the final pose (k_novel.hip), enqueued only */
  if (!frame_ready) {
    const uint32_t scan_id = l->scan_count++;
    if (l->nv.on) {
      forget_last(l, LAST_COLLECTION | LAST_SEGMENTATION);
      if (l->n_window && (res->tracked || !l->nv.np.tracked_only) && finite16(pose)) {
        int r = collect(l, l->frame, pose, scan_id);
        if (r) return r;
        l->last_collected = 1;
      }
    }
  }
  return SUMA_OK;
}

extern "C" int suma_localizer_process_scan(suma_localizer* l, const suma_float4* points, const float* labels,
                                           const float* probs, uint32_t n, int32_t fixed_iterations,
                                           suma_localizer_result* result) {
  return process_scan(l, points, labels, probs, n, fixed_iterations, result, false);
}

extern "C" int suma_localizer_process_scan_device(suma_localizer* l, const suma_float4* d_points, const float* d_labels,
                                                  const float* d_probs, uint32_t n, int32_t fixed_iterations,
                                                  suma_localizer_result* result) {
  return process_scan(l, d_points, d_labels, d_probs, n, fixed_iterations, result, true);
}

/* ---- motion compensation (k_deskew.hip; the pipeline's entries are in suma_deskew.hip) ---- */
extern "C" int suma_localizer_enable_deskew(suma_localizer* l, const suma_deskew_params* dp) {
  if (!l) return SUMA_ERR_INVALID;
  int r = deskew_params_check(l->c, dp, true, "suma_localizer_enable_deskew");
  if (r) return r;
  suma_deskew_params_default(&l->dk.dp);
  if (dp) l->dk.dp = *dp;
  if (!l->dk.on) mat4_eye(l->dk.last_motion), l->dk.last_source = SUMA_DESKEW_MOTION_NONE;
  l->dk.on = true;
  return SUMA_OK;
}
extern "C" int suma_localizer_disable_deskew(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  l->dk.on = false;
  l->dk.have_override = false;
  return SUMA_OK;
}
extern "C" int suma_localizer_set_deskew_motion(suma_localizer* l, const double motion[16]) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!l->dk.on) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_deskew_motion: motion compensation is not enabled");
  if (!motion) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_deskew_motion: NULL motion");
  if (!finite16(motion)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_deskew_motion: non-finite motion");
  memcpy(l->dk.override_motion, motion, 16 * sizeof(double));
  l->dk.have_override = true;
  return SUMA_OK;
}
extern "C" int suma_localizer_deskew_motion(const suma_localizer* l, double motion[16], int32_t* source) {
  if (!l || !motion) return SUMA_ERR_INVALID;
  if (l->dk.last_source == SUMA_DESKEW_MOTION_NONE) mat4_eye(motion);
  else memcpy(motion, l->dk.last_motion, 16 * sizeof(double));
  if (source) *source = l->dk.last_source;
  return SUMA_OK;
}

/* ---- global relocalisation (include/suma_hip.h states the steps) ---- */
namespace {

/* what a relocalisation that finds nothing has to put back */
struct LocSaved {
  double pose[16], increment[16];
  bool have_pose, first;
  int32_t oi, oj;
  uint32_t n_window, rebuilds;
  std::vector<LocSpan> spans;
};

void loc_save(const suma_localizer* l, LocSaved* s) {
  memcpy(s->pose, l->pose, sizeof(s->pose));
  memcpy(s->increment, l->increment, sizeof(s->increment));
  s->have_pose = l->have_pose, s->first = l->first;
  s->oi = l->oi, s->oj = l->oj;
  s->n_window = l->n_window, s->rebuilds = l->rebuilds;
  s->spans = l->spans;
}

/* the window is a function of the map and the origin: gathering it again at the saved origin gives the saved bytes */
int loc_restore(suma_localizer* l, const LocSaved& s) {
  int r = SUMA_OK;
  if (s.have_pose && (l->oi != s.oi || l->oj != s.oj || !l->have_pose)) r = gather_window(l, s.oi, s.oj);
  memcpy(l->pose, s.pose, sizeof(s.pose));
  memcpy(l->increment, s.increment, sizeof(s.increment));
  l->have_pose = s.have_pose, l->first = s.first;
  l->oi = s.oi, l->oj = s.oj;
  l->n_window = s.n_window, l->rebuilds = s.rebuilds;
  l->spans = s.spans;
  return r;
}

int relocalize(suma_localizer* l, suma_place_index* idx, const double* poses16, uint32_t n_poses, const suma_float4* points,
               const float* labels, const float* probs, uint32_t n, uint32_t max_candidates, int32_t fixed_iterations,
               suma_relocalize_result* res, bool on_device) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!res) return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: NULL result");
  if (!idx) return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: NULL place index");
  if (n && !points) return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: NULL points with n > 0");
  if (!l->have_map) return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: no map (suma_localizer_set_map)");
  if (max_candidates < 1 || max_candidates > SUMA_PLACE_MAX_MATCHES)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: max_candidates must be 1 .. 32");
  if (n_poses != suma_place_index_size(idx) || (n_poses && !poses16))
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_relocalize: one pose per entry of the index is needed (n_poses = " +
                                     std::to_string(n_poses) + ", entries = " + std::to_string(suma_place_index_size(idx)) + ")");
  memset(res, 0, sizeof(*res));
  res->winner = -1;
  /* 1. K1-K3 at T_loc */
  int r = on_device ? suma_preprocess_device(c, points, labels, probs, n, c->timestamp, l->frame)
                    : suma_preprocess(c, points, labels, probs, n, c->timestamp, l->frame);
  if (r) return r;
  /* 2. the candidate places */
  suma_place_match matches[SUMA_PLACE_MAX_MATCHES];
  uint32_t n_matches = 0;
  r = suma_place_index_query_frame(idx, c, l->frame, 1u, 0u, max_candidates, matches, &n_matches);
  if (r) return r;
  LocSaved saved;
  loc_save(l, &saved);
  /* 3. each candidate is a start pose and one scan */
  int best = -1;
  double best_score = 0.0;
  for (uint32_t k = 0; k < n_matches; ++k) {
    double T[16];
    place_hypothesis(poses16 + 16 * (size_t)matches[k].index, matches[k].yaw, T);
    suma_relocalize_candidate* cand = &res->candidates[k];
    cand->match = matches[k];
    r = suma_localizer_set_pose(l, T);
    if (!r) r = process_scan(l, points, labels, probs, n, fixed_iterations, &cand->result, on_device, true);
    if (r) {
      const std::string why = c->err;
      loc_restore(l, saved);
      return fail(c, r, why);
    }
    res->n_tried = k + 1u;
    if (!cand->result.tracked) continue;
    const double score = cand->result.stats.error / (double)cand->result.stats.valid;
    if (best < 0 || score < best_score) best = (int)k, best_score = score;
  }
  /* 4. */
  if (best < 0) return loc_restore(l, saved);
  const suma_localizer_result& w = res->candidates[best].result;
  if ((uint32_t)best + 1u != n_matches) { /* a later candidate has left its state: back to the winner's */
    if (l->oi != w.origin_ij[0] || l->oj != w.origin_ij[1]) {
      r = gather_window(l, w.origin_ij[0], w.origin_ij[1]);
      if (r) return r;
    }
    memcpy(l->pose, w.pose, sizeof(l->pose));
    memcpy(l->increment, w.increment, sizeof(l->increment));
    l->first = false;
    float gf[16];
    mat4_cast_f(w.guess, gf);
    r = suma_map_render_inactive(c, gf, l->lp.conf_threshold); /* the model frame as the winner's scan left it */
    if (r) return r;
  }
  res->found = 1;
  res->winner = best;
  res->match = res->candidates[best].match;
  res->result = w;
  return SUMA_OK;
}

}  // namespace

extern "C" int suma_localizer_relocalize(suma_localizer* l, suma_place_index* idx, const double* poses16, uint32_t n_poses,
                                         const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                                         uint32_t max_candidates, int32_t fixed_iterations, suma_relocalize_result* result) {
  return relocalize(l, idx, poses16, n_poses, points, labels, probs, n, max_candidates, fixed_iterations, result, false);
}

extern "C" int suma_localizer_relocalize_device(suma_localizer* l, suma_place_index* idx, const double* poses16,
                                                uint32_t n_poses, const suma_float4* d_points, const float* d_labels,
                                                const float* d_probs, uint32_t n, uint32_t max_candidates,
                                                int32_t fixed_iterations, suma_relocalize_result* result) {
  return relocalize(l, idx, poses16, n_poses, d_points, d_labels, d_probs, n, max_candidates, fixed_iterations, result, true);
}

extern "C" int suma_localizer_window(suma_localizer* l, int32_t origin_ij[2], uint32_t* n_window, uint32_t* rebuilds) {
  if (!l) return SUMA_ERR_INVALID;
  if (origin_ij) origin_ij[0] = l->oi, origin_ij[1] = l->oj;
  if (n_window) *n_window = l->n_window;
  if (rebuilds) *rebuilds = l->rebuilds;
  return SUMA_OK;
}

extern "C" int suma_localizer_download_window(suma_localizer* l, suma_surfel* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  if (!n || (capacity && !host)) return fail(l->c, SUMA_ERR_INVALID, "suma_localizer_download_window: NULL argument");
  if (!l->have_pose) { /* nothing has been gathered */
    *n = 0;
    return SUMA_OK;
  }
  return suma_map_download(l->c, host, capacity, n);
}

/* ---- change evidence (include/suma_hip.h states the entries, k_change.hip the specification) ---- */
extern "C" void suma_change_params_default(suma_change_params* cp) {
  if (!cp) return;
  cp->free_margin = 0.5f;
  cp->min_view_cos = 0.3f;
  cp->max_range = 50.0f;
  cp->tracked_only = 1;
}

extern "C" void suma_change_rule_default(suma_change_rule* rule) {
  if (!rule) return;
  rule->min_misses = 3u;
  rule->miss_ratio = 2.0f;
}

extern "C" int suma_localizer_enable_evidence(suma_localizer* l, const suma_change_params* cp) {
  if (!l) return SUMA_ERR_INVALID;
  suma_change_params q;
  suma_change_params_default(&q);
  if (cp) q = *cp;
  if (const char* why = change_params_why(q)) return fail(l->c, SUMA_ERR_INVALID, std::string("suma_localizer_enable_evidence: ") + why);
  l->cp = q;
  l->ev_wanted = true;
  return SUMA_OK;
}

extern "C" int suma_localizer_disable_evidence(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  l->ev_wanted = false;
  if (l->map.has_evidence) {
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* an observation may still read them */
    l->map.has_evidence = false;
    l->map.evidence.reset();
    l->map.src_idx.reset();
    l->ev_source.reset();
  }
  forget_last(l, LAST_OBSERVATION);
  return SUMA_OK;
}

static int evidence_ready(suma_localizer* l, const char* who) {
  if (!l->have_map || !l->map.has_evidence)
    return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": no evidence (suma_localizer_enable_evidence, then "
                                        "suma_localizer_set_map)");
  return SUMA_OK;
}

extern "C" int suma_localizer_observe_frame(suma_localizer* l, const suma_frame* frame, const double T[16],
                                            suma_change_counts* counts) {
  if (!l) return SUMA_ERR_INVALID;
  int r = evidence_ready(l, "suma_localizer_observe_frame");
  if (!r) r = frame_pose_check(l, frame, T, "suma_localizer_observe_frame");
  if (r) return r;
  return observe(l, frame, T, counts);
}

extern "C" int suma_localizer_last_observation(suma_localizer* l, suma_change_counts* counts, int32_t* observed) {
  if (!l) return SUMA_ERR_INVALID;
  int r = evidence_ready(l, "suma_localizer_last_observation");
  if (r) return r;
  if (counts) *counts = l->last_counts;
  if (observed) *observed = l->last_observed;
  return SUMA_OK;
}

/* the evidence in source order into l->ev_source (n_total words), enqueued */
static int evidence_to_source_order(suma_localizer* l) {
  suma_ctx* c = l->c;
  const uint32_t n = l->map.n_total;
  if (!n) return SUMA_OK;
  int r = grow(c, l->ev_source, n, {c->stream});
  if (r < 0) return r;
  HIP_TRY(c, hipMemsetAsync(l->ev_source, 0, (size_t)n * sizeof(suma_change_evidence), c->stream));
  ProfScope ps(c, "change_scatter", 36.0 * l->map.n_kept + 16.0 * n);
  HIP_TRY(c, launch_kc_scatter(c, l->map, l->ev_source));
  return SUMA_OK;
}

static int evidence_download(suma_localizer* l, suma_change_evidence* out, uint32_t capacity, uint32_t* n, bool to_device,
                             const char* who) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = evidence_ready(l, who);
  if (r) return r;
  if (!n || (capacity && !out)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  *n = l->map.n_total; /* also when the scatter below fails */
  if (capacity && (r = evidence_to_source_order(l))) return r; /* nothing is made for a call that only asks for n */
  return download(c, out, capacity, n, l->ev_source, l->map.n_total, sizeof(suma_change_evidence), to_device);
}

extern "C" int suma_localizer_evidence(suma_localizer* l, suma_change_evidence* host, uint32_t capacity, uint32_t* n) {
  return evidence_download(l, host, capacity, n, false, "suma_localizer_evidence");
}

extern "C" int suma_localizer_evidence_device(suma_localizer* l, suma_change_evidence* d_out, uint32_t capacity, uint32_t* n) {
  return evidence_download(l, d_out, capacity, n, true, "suma_localizer_evidence_device");
}

extern "C" int suma_localizer_clear_evidence(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = evidence_ready(l, "suma_localizer_clear_evidence");
  if (r) return r;
  if (l->map.n_kept)
    HIP_TRY(c, hipMemsetAsync(l->map.evidence, 0, (size_t)l->map.n_kept * sizeof(suma_change_evidence), c->stream));
  forget_last(l, LAST_OBSERVATION);
  return SUMA_OK;
}

extern "C" int suma_change_prune_mask(const suma_change_evidence* evidence, uint32_t n, const suma_change_rule* rule,
                                      uint8_t* keep, uint32_t* n_removed) {
  if (n && (!evidence || !keep)) return fail_without_ctx(SUMA_ERR_INVALID, "suma_change_prune_mask: NULL array with n > 0");
  suma_change_rule q;
  suma_change_rule_default(&q);
  if (rule) q = *rule;
  uint32_t removed = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const suma_change_evidence& e = evidence[k];
    const bool gone = e.misses >= q.min_misses && (float)e.misses > q.miss_ratio * (float)e.hits;
    keep[k] = gone ? 0 : 1;
    removed += gone ? 1u : 0u;
  }
  if (n_removed) *n_removed = removed;
  return SUMA_OK;
}

/* ---- novelty (include/suma_hip.h states the entries, k_novel.hip the specification) ---- */
extern "C" void suma_novel_params_default(suma_novel_params* np) {
  if (!np) return;
  np->agree_margin = 0.5f;
  np->max_range = 50.0f;
  np->tracked_only = 1;
  np->max_candidates = 4194304u;
}

extern "C" void suma_novel_fuse_params_default(const suma_params* params, suma_novel_fuse_params* fp) {
  if (!fp) return;
  fp->voxel_size = 0.2f;
  fp->min_views = 2u;
  fp->confidence = (params ? params->confidence_threshold : 0.0f) + 1.0f;
}

/* NULL, or what is wrong with the values */
static const char* novel_params_why(const suma_novel_params& q) {
  if (!(std::isfinite(q.agree_margin) && q.agree_margin > 0.0f)) return "agree_margin must be finite and > 0";
  if (!(std::isfinite(q.max_range) && q.max_range > 0.0f)) return "max_range must be finite and > 0";
  if (q.max_candidates < 1u || q.max_candidates > (1u << 30)) return "max_candidates must be 1 .. 2^30";
  return nullptr;
}

static int novelty_ready(suma_localizer* l, const char* who) {
  if (!l->nv.on) return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": novelty is off (suma_localizer_enable_novelty)");
  return SUMA_OK;
}

extern "C" int suma_localizer_enable_novelty(suma_localizer* l, const suma_novel_params* np) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  suma_novel_params q;
  suma_novel_params_default(&q);
  if (np) q = *np;
  if (const char* why = novel_params_why(q)) return fail(c, SUMA_ERR_INVALID, std::string("suma_localizer_enable_novelty: ") + why);
  Novel& nv = l->nv;
  const size_t P = (size_t)c->p.data_width * (size_t)c->p.data_height;
  const size_t blocks = (P + 255) / 256;
  const bool fresh = !nv.on || nv.np.max_candidates != q.max_candidates;
  if (fresh) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    Novel nw;
    hipError_t e = nw.cand.alloc(3 * (size_t)q.max_candidates);
    if (e == hipSuccess) e = nw.mark.alloc(P);
    if (e == hipSuccess) e = nw.flag.alloc(P);
    if (e == hipSuccess) e = nw.block_counts.alloc(8 * blocks);
    if (e == hipSuccess) e = nw.state.alloc(1);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, SUMA_ERR_NOMEM, "suma_localizer_enable_novelty: no device memory for " +
                                     std::to_string(q.max_candidates) + " candidates");
    }
    HIP_TRY(c, hipMemsetAsync(nw.state, 0, sizeof(NovelState), c->stream));
    HIP_TRY(c, hipMemsetAsync(nw.mark, 0, P, c->stream));
    HIP_TRY(c, hipMemsetAsync(nw.flag, 0, P, c->stream)); /* suma_localizer_novel_flags in front of the first collection */
    nv = std::move(nw);
    forget_last(l, LAST_COLLECTION);
  }
  nv.np = q;
  nv.on = true;
  return SUMA_OK;
}

extern "C" int suma_localizer_disable_novelty(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  const int r = disable_layer(l, LAYER_NOVELTY);
  if (r) return r;
  forget_last(l, LAST_COLLECTION);
  return SUMA_OK;
}

/* the device state into host words (blocking): count, n_overflow, done, pad, counts[8] */
static int novel_state(suma_localizer* l, NovelState* out) { return read_words(l, l->nv.state, sizeof(NovelState), out); }

static int novel_overflow(suma_localizer* l, const NovelState& s, const char* who) {
  if (!s.n_overflow) return SUMA_OK;
  return fail(l->c, SUMA_ERR_CAPACITY, std::string(who) + ": " + std::to_string(s.n_overflow) +
                                       " novel texels did not fit into max_candidates = " +
                                       std::to_string(l->nv.np.max_candidates));
}

extern "C" int suma_localizer_collect_frame(suma_localizer* l, const suma_frame* frame, const double T[16], uint32_t scan_id,
                                            suma_novel_counts* counts) {
  if (!l) return SUMA_ERR_INVALID;
  int r = novelty_ready(l, "suma_localizer_collect_frame");
  if (!r) r = frame_pose_check(l, frame, T, "suma_localizer_collect_frame");
  if (r) return r;
  if (counts) memset(counts, 0, sizeof(*counts));
  forget_last(l, LAST_COLLECTION | LAST_SEGMENTATION);
  if (!l->have_map || !l->n_window) return SUMA_OK;
  r = collect(l, frame, T, scan_id);
  if (r) return r;
  l->last_collected = 1;
  if (counts) {
    NovelState s;
    r = novel_state(l, &s);
    if (r) return r;
    memcpy(counts, s.counts, sizeof(*counts));
  }
  return SUMA_OK;
}

extern "C" int suma_localizer_last_collection(suma_localizer* l, suma_novel_counts* counts, int32_t* collected) {
  if (!l) return SUMA_ERR_INVALID;
  int r = novelty_ready(l, "suma_localizer_last_collection");
  if (r) return r;
  NovelState s;
  r = novel_state(l, &s);
  if (r) return r;
  if (counts) {
    memset(counts, 0, sizeof(*counts));
    if (l->last_collected) memcpy(counts, s.counts, sizeof(*counts));
  }
  if (collected) *collected = l->last_collected;
  return novel_overflow(l, s, "suma_localizer_last_collection");
}

static int candidates_download(suma_localizer* l, suma_world_surfel* out, uint32_t capacity, uint32_t* n, bool to_device,
                               const char* who) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, who);
  if (r) return r;
  if (!n || (capacity && !out)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  NovelState s;
  r = novel_state(l, &s);
  if (r) return r;
  if ((r = download(c, out, capacity, n, l->nv.cand, s.count, sizeof(suma_world_surfel), to_device))) return r;
  return novel_overflow(l, s, who);
}

extern "C" int suma_localizer_novel_candidates(suma_localizer* l, suma_world_surfel* host, uint32_t capacity, uint32_t* n) {
  return candidates_download(l, host, capacity, n, false, "suma_localizer_novel_candidates");
}

extern "C" int suma_localizer_novel_candidates_device(suma_localizer* l, suma_world_surfel* d_out, uint32_t capacity,
                                                      uint32_t* n) {
  return candidates_download(l, d_out, capacity, n, true, "suma_localizer_novel_candidates_device");
}

extern "C" int suma_localizer_set_novel_candidates(suma_localizer* l, const suma_world_surfel* host, uint32_t n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, "suma_localizer_set_novel_candidates");
  if (r) return r;
  if (n && !host) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_novel_candidates: NULL records with n > 0");
  if (n > l->nv.np.max_candidates)
    return fail(c, SUMA_ERR_CAPACITY, "suma_localizer_set_novel_candidates: " + std::to_string(n) + " records, max_candidates = " +
                                      std::to_string(l->nv.np.max_candidates));
  HIP_TRY(c, hipMemsetAsync(l->nv.state, 0, sizeof(NovelState), c->stream));
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(l->nv.cand, host, (size_t)n * sizeof(suma_world_surfel), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&l->nv.state->count, &n, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* pageable sources: the copies have left them */
  forget_last(l, LAST_COLLECTION);
  return SUMA_OK;
}

static int novel_fused(suma_localizer* l, const suma_novel_fuse_params* fp, suma_world_surfel* out, uint32_t* views,
                       uint32_t capacity, suma_novel_stats* stats, bool to_device, const char* who) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, who);
  if (r) return r;
  if (!stats || (capacity && (!out || !views))) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  suma_novel_fuse_params q;
  suma_novel_fuse_params_default(&c->p, &q);
  if (fp) q = *fp;
  if (!(std::isfinite(q.voxel_size) && q.voxel_size > 0.0f))
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": voxel_size must be finite and > 0");
  if (q.min_views < 1u) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": min_views must be at least 1");
  if (std::isnan(q.confidence)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": confidence is NaN");
  memset(stats, 0, sizeof(*stats));
  NovelState s;
  r = novel_state(l, &s);
  if (r) return r;
  stats->n_candidates = s.count;
  stats->n_overflow = s.n_overflow;
  suma_world_surfel* d_out = out;
  uint32_t* d_views = views;
  const uint32_t cap = capacity < s.count ? capacity : s.count; /* no more voxels than candidates */
  if (!to_device && cap) {
    if ((r = grow(c, l->nv.fused, 3 * (size_t)cap, {c->stream})) < 0) return r;
    if ((r = grow(c, l->nv.fused_views, cap, {c->stream})) < 0) return r;
    d_out = reinterpret_cast<suma_world_surfel*>(l->nv.fused.p);
    d_views = l->nv.fused_views;
  }
  r = novel_fuse(c, l->nv, s.count, q, d_out, d_views, cap, l->stage_h);
  if (r) return r;
  stats->n_dropped = l->stage_h.p[0];
  stats->n_voxels = l->stage_h.p[1];
  stats->n_out = l->stage_h.p[2];
  /* the kernel has written a device caller's blocks itself; a host caller's two arrays go under one synchronise, which
   * is why this site does not call download() twice */
  const uint32_t m = stats->n_out < cap ? stats->n_out : cap;
  if (!to_device && m) {
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (size_t)m * sizeof(suma_world_surfel), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(views, d_views, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return novel_overflow(l, s, who);
}

extern "C" int suma_localizer_novel(suma_localizer* l, const suma_novel_fuse_params* fp, suma_world_surfel* host,
                                    uint32_t* views, uint32_t capacity, suma_novel_stats* stats) {
  return novel_fused(l, fp, host, views, capacity, stats, false, "suma_localizer_novel");
}

extern "C" int suma_localizer_novel_device(suma_localizer* l, const suma_novel_fuse_params* fp, suma_world_surfel* d_out,
                                           uint32_t* d_views, uint32_t capacity, suma_novel_stats* stats) {
  return novel_fused(l, fp, d_out, d_views, capacity, stats, true, "suma_localizer_novel_device");
}

extern "C" int suma_localizer_novel_marks(suma_localizer* l, uint8_t* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, "suma_localizer_novel_marks");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_novel_marks: NULL argument");
  return download(c, host, capacity, n, l->nv.mark, (uint32_t)c->p.data_width * (uint32_t)c->p.data_height, 1, false);
}

extern "C" int suma_localizer_clear_novelty(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, "suma_localizer_clear_novelty");
  if (r) return r;
  HIP_TRY(c, hipMemsetAsync(l->nv.state, 0, sizeof(NovelState), c->stream));
  forget_last(l, LAST_COLLECTION | LAST_SEGMENTATION);
  if (l->tk.on && (r = tracks_clear(c, l->tk))) return r;
  return SUMA_OK;
}

/* ---- objects (include/suma_hip.h states the entries, k_objects.hip the specification) ---- */
extern "C" void suma_object_params_default(suma_object_params* op) {
  if (!op) return;
  op->link_base = 0.3f;
  op->link_slope = 0.03f;
  op->min_texels = 5u;
  op->max_objects = 4096u;
}

/* NULL, or what is wrong with the values */
static const char* object_params_why(const suma_object_params& q) {
  if (!(std::isfinite(q.link_base) && q.link_base >= 0.0f)) return "link_base must be finite and >= 0";
  if (!(std::isfinite(q.link_slope) && q.link_slope >= 0.0f)) return "link_slope must be finite and >= 0";
  if (q.min_texels < 1u) return "min_texels must be at least 1";
  if (q.max_objects < 1u || q.max_objects > 65536u) return "max_objects must be 1 .. 65536";
  return nullptr;
}

extern "C" int suma_object_params_check(const suma_object_params* op) {
  if (!op) return fail_without_ctx(SUMA_ERR_INVALID, "suma_object_params_check: NULL parameters");
  if (const char* why = object_params_why(*op)) return fail_without_ctx(SUMA_ERR_INVALID, std::string("suma_object_params_check: ") + why);
  return SUMA_OK;
}

static int objects_ready(suma_localizer* l, const char* who) {
  if (!l->ob.on) return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": objects are off (suma_localizer_enable_objects)");
  return SUMA_OK;
}

extern "C" int suma_localizer_enable_objects(suma_localizer* l, const suma_object_params* op) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!l->nv.on)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_objects: novelty is off (suma_localizer_enable_novelty): the "
                                     "objects are made of its flags");
  suma_object_params q;
  suma_object_params_default(&q);
  if (op) q = *op;
  if (const char* why = object_params_why(q)) return fail(c, SUMA_ERR_INVALID, std::string("suma_localizer_enable_objects: ") + why);
  const uint64_t P = (uint64_t)c->p.data_width * (uint64_t)c->p.data_height;
  if (P > (1u << 22)) /* the bound that keeps the centroid's int64 sums from overflowing (k_objects.hip, step 5) */
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_objects: the data image has " + std::to_string(P) +
                                     " texels, more than 2^22");
  Objects& ob = l->ob;
  if (!ob.on || ob.op.max_objects != q.max_objects || ob.n_texels != (uint32_t)P) {
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* a segmentation may still write the old blocks */
    int r = objects_alloc(c, ob, q, (uint32_t)P);
    if (r) return r;
  }
  ob.op = q;
  ob.on = true;
  forget_last(l, LAST_SEGMENTATION);
  if (l->tk.on && l->tk.max_objects != q.max_objects) { /* the tracker's blocks are sized by max_objects: made again */
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const suma_track_params tp = l->tk.tp;
    int r = tracks_alloc(c, l->tk, tp, q.max_objects);
    if (r) {
      l->tk = Tracks();
      return r;
    }
    l->tk.on = true;
  }
  return SUMA_OK;
}

extern "C" int suma_localizer_disable_objects(suma_localizer* l) {
  return l ? disable_layer(l, LAYER_OBJECTS) : SUMA_ERR_INVALID;
}

/* the counts of the last segmentation into host words (blocking) */
static int objects_counts(suma_localizer* l, suma_object_counts* out) {
  return read_words(l, l->ob.state, sizeof(suma_object_counts), out);
}

static int objects_download(suma_localizer* l, suma_scan_object* out, uint32_t capacity, uint32_t* n,
                            suma_object_counts* counts, int32_t* segmented, bool to_device, const char* who) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = objects_ready(l, who);
  if (r) return r;
  if (!n || (capacity && !out)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  *n = 0;
  if (counts) memset(counts, 0, sizeof(*counts));
  if (segmented) *segmented = l->ob.segmented;
  if (!l->ob.segmented) return SUMA_OK;
  suma_object_counts cnt;
  r = objects_counts(l, &cnt);
  if (r) return r;
  if (counts) *counts = cnt;
  if ((r = download(c, out, capacity, n, l->ob.rec, cnt.stored, sizeof(suma_scan_object), to_device))) return r;
  if (cnt.n_objects > cnt.stored)
    return fail(c, SUMA_ERR_CAPACITY, std::string(who) + ": " + std::to_string(cnt.n_objects - cnt.stored) +
                                      " objects did not fit into max_objects = " + std::to_string(l->ob.op.max_objects));
  return SUMA_OK;
}

extern "C" int suma_localizer_objects(suma_localizer* l, suma_scan_object* host, uint32_t capacity, uint32_t* n,
                                      suma_object_counts* counts, int32_t* segmented) {
  return objects_download(l, host, capacity, n, counts, segmented, false, "suma_localizer_objects");
}

extern "C" int suma_localizer_objects_device(suma_localizer* l, suma_scan_object* d_out, uint32_t capacity, uint32_t* n,
                                             suma_object_counts* counts, int32_t* segmented) {
  return objects_download(l, d_out, capacity, n, counts, segmented, true, "suma_localizer_objects_device");
}

extern "C" int suma_localizer_object_ids(suma_localizer* l, uint32_t* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = objects_ready(l, "suma_localizer_object_ids");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_object_ids: NULL argument");
  return download(c, host, capacity, n, l->ob.ids, l->ob.segmented ? l->ob.n_texels : 0u, sizeof(uint32_t), false);
}

extern "C" suma_frame* suma_localizer_frame(suma_localizer* l) { return l ? l->frame : nullptr; }

extern "C" int suma_localizer_novel_flags(suma_localizer* l, uint8_t* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = novelty_ready(l, "suma_localizer_novel_flags");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_novel_flags: NULL argument");
  return download(c, host, capacity, n, l->nv.flag, (uint32_t)c->p.data_width * (uint32_t)c->p.data_height, 1, false);
}

extern "C" int suma_localizer_segment_flags(suma_localizer* l, const suma_frame* frame, const double T[16],
                                            const uint8_t* host_flags, uint32_t scan_id, suma_object_counts* counts) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  const char* who = "suma_localizer_segment_flags";
  int r = objects_ready(l, who);
  if (r) return r;
  if (!host_flags) return fail(c, SUMA_ERR_INVALID, "suma_localizer_segment_flags: NULL argument");
  if ((r = frame_pose_check(l, frame, T, who))) return r;
  if ((r = stamps_check(l, scan_id, who, false))) return r;
  if (counts) memset(counts, 0, sizeof(*counts));
  Objects& ob = l->ob;
  forget_last(l, LAST_SEGMENTATION);
  if ((r = frame_read_begin(c, frame))) return r;
  HIP_TRY(c, hipMemcpyAsync(ob.flags_in, host_flags, ob.n_texels, hipMemcpyHostToDevice, c->stream));
  r = run_layers(l, frame, ob.flags_in, T, scan_id, false);
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* a pageable source: the copy has left it */
  if (r) return r;
  return counts ? objects_counts(l, counts) : SUMA_OK;
}

/* ---- the live obstacle layer (include/suma_hip.h states the entries, k_live.hip the specification) ---- */
extern "C" void suma_live_params_default(suma_live_params* lp) {
  if (!lp) return;
  lp->hold_scans = 10u;
  lp->min_hits = 2u;
  lp->carve_range = 20.0f;
  lp->carve_margin = 0.5f;
}

/* NULL, or what is wrong with the values */
static const char* live_params_why(const suma_live_params& q) {
  if (q.hold_scans < 1u || q.hold_scans > 65535u) return "hold_scans must be 1 .. 65535";
  if (q.min_hits < 1u || q.min_hits > 65535u) return "min_hits must be 1 .. 65535";
  if (!(std::isfinite(q.carve_range) && q.carve_range >= 0.0f)) return "carve_range must be finite and >= 0";
  if (!(std::isfinite(q.carve_margin) && q.carve_margin >= 0.0f)) return "carve_margin must be finite and >= 0";
  return nullptr;
}

extern "C" int suma_live_params_check(const suma_live_params* lp) {
  if (!lp) return fail_without_ctx(SUMA_ERR_INVALID, "suma_live_params_check: NULL parameters");
  if (const char* why = live_params_why(*lp)) return fail_without_ctx(SUMA_ERR_INVALID, std::string("suma_live_params_check: ") + why);
  return SUMA_OK;
}

static int live_ready(suma_localizer* l, const char* who) {
  if (!l->lv.on) return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": the live layer is off (suma_localizer_enable_live_grid)");
  return SUMA_OK;
}

extern "C" int suma_localizer_enable_live_grid(suma_localizer* l, const suma_grid_params* gp, const suma_grid_cell* d_cells,
                                               const suma_live_params* lp) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  const char* who = "suma_localizer_enable_live_grid";
  if (!l->nv.on)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_live_grid: novelty is off (suma_localizer_enable_novelty): the "
                                     "hits are made of its flags");
  if (!gp) return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_live_grid: NULL grid parameters");
  if (!d_cells) return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_live_grid: NULL cells");
  if ((uintptr_t)d_cells & 15u) return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_live_grid: cells not 16-byte aligned");
  int r = grid_check_params(c, who, *gp);
  if (r) return r;
  suma_live_params q;
  suma_live_params_default(&q);
  if (lp) q = *lp;
  if (const char* why = live_params_why(q)) return fail(c, SUMA_ERR_INVALID, std::string("suma_localizer_enable_live_grid: ") + why);
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* an update may still write the old blocks */
  r = live_alloc(c, l->lv, *gp, d_cells);
  if (r) return r;
  l->lv.lp = q;
  l->lv.on = true;
  return SUMA_OK;
}

extern "C" int suma_localizer_disable_live_grid(suma_localizer* l) {
  return l ? disable_layer(l, LAYER_LIVE) : SUMA_ERR_INVALID;
}

extern "C" int suma_localizer_clear_live_grid(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  int r = live_ready(l, "suma_localizer_clear_live_grid");
  if (r) return r;
  return live_clear(l->c, l->lv);
}

/* words first .. first + n - 1 of the layer into host words (blocking) */
static int live_words(suma_localizer* l, uint32_t first, uint32_t n, void* out) {
  return read_words(l, l->lv.words.p + first, n * sizeof(uint32_t), out);
}

extern "C" int suma_localizer_live_update_flags(suma_localizer* l, const suma_frame* frame, const double T[16],
                                                const uint8_t* host_flags, uint32_t scan_id, suma_live_counts* counts) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  const char* who = "suma_localizer_live_update_flags";
  int r = live_ready(l, who);
  if (r) return r;
  if (!host_flags) return fail(c, SUMA_ERR_INVALID, "suma_localizer_live_update_flags: NULL argument");
  if ((r = frame_pose_check(l, frame, T, who))) return r;
  if ((r = stamps_check(l, scan_id, who, true))) return r;
  if (counts) memset(counts, 0, sizeof(*counts));
  Objects& ob = l->ob;
  Live& lv = l->lv;
  const size_t P = (size_t)c->p.data_width * (size_t)c->p.data_height;
  uint8_t* d_flags = ob.flags_in;
  if (!ob.on) {
    if ((r = grow(c, lv.flags_in, P, {c->stream})) < 0) return r;
    d_flags = lv.flags_in;
  }
  forget_last(l, LAST_SEGMENTATION);
  if ((r = frame_read_begin(c, frame))) return r;
  HIP_TRY(c, hipMemcpyAsync(d_flags, host_flags, P, hipMemcpyHostToDevice, c->stream));
  r = run_layers(l, frame, d_flags, T, scan_id, true);
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* a pageable source: the copy has left it */
  if (r) return r;
  return counts ? live_words(l, 0, LIVE_COUNT_WORDS, counts) : SUMA_OK;
}

extern "C" int suma_localizer_live_counts(suma_localizer* l, suma_live_counts* counts, int32_t* updated) {
  if (!l) return SUMA_ERR_INVALID;
  int r = live_ready(l, "suma_localizer_live_counts");
  if (r) return r;
  if (counts) memset(counts, 0, sizeof(*counts));
  if (updated) *updated = l->lv.updated;
  if (!l->lv.updated || !counts) return SUMA_OK;
  return live_words(l, 0, LIVE_COUNT_WORDS, counts);
}

extern "C" int suma_localizer_live_cells_device(suma_localizer* l, suma_grid_cell* d_out_cells, uint8_t* d_out_mask,
                                                suma_live_stats* stats) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = live_ready(l, "suma_localizer_live_cells_device");
  if (r) return r;
  if (!d_out_cells) return fail(c, SUMA_ERR_INVALID, "suma_localizer_live_cells_device: NULL cells");
  if ((uintptr_t)d_out_cells & 15u) return fail(c, SUMA_ERR_INVALID, "suma_localizer_live_cells_device: cells not 16-byte aligned");
  if (stats) memset(stats, 0, sizeof(*stats));
  if ((r = live_compose(c, l->lv, d_out_cells, d_out_mask))) return r;
  suma_live_stats st;
  if ((r = live_words(l, LIVE_STATS, LIVE_STAT_WORDS, &st))) return r;
  if (stats) *stats = st;
  return SUMA_OK;
}

extern "C" int suma_localizer_live_state(suma_localizer* l, suma_live_cell* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = live_ready(l, "suma_localizer_live_state");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_live_state: NULL argument");
  return download(c, host, capacity, n, l->lv.state, l->lv.n_cells, sizeof(suma_live_cell), false);
}

extern "C" int suma_localizer_set_live_state(suma_localizer* l, const suma_live_cell* host, uint32_t n, uint32_t last_stamp) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = live_ready(l, "suma_localizer_set_live_state");
  if (r) return r;
  if (!host) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_live_state: NULL argument");
  Live& lv = l->lv;
  if (n != lv.n_cells)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_live_state: " + std::to_string(n) + " cells, the raster has " +
                                     std::to_string(lv.n_cells));
  uint32_t any = 0u;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t H = (uint32_t)(host[k].hit >> 32);
    if (H > last_stamp || host[k].clear > last_stamp)
      return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_live_state: cell " + std::to_string(k) + " carries a stamp above last_stamp");
    any |= H != 0u ? 1u : 0u;
  }
  if ((r = live_clear(c, lv))) return r;
  HIP_TRY(c, hipMemcpyAsync(lv.state, host, (size_t)n * sizeof(suma_live_cell), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(lv.words.p + LIVE_ANY_HIT, &any, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* pageable sources: the copies have left them */
  lv.last_stamp = last_stamp;
  return SUMA_OK;
}

/* ---- tracks (include/suma_hip.h states the entries, k_tracks.hip the specification) ---- */
extern "C" void suma_track_params_default(suma_track_params* tp) {
  if (!tp) return;
  tp->join_dist = 2.0f;
  tp->gate_base = 1.5f;
  tp->gate_speed = 0.5f;
  tp->alpha = 0.5f;
  tp->beta = 0.2f;
  tp->confirm_hits = 3u;
  tp->max_missed = 3u;
  tp->max_tracks = 1024u;
  tp->max_rounds = 16u;
}

/* NULL, or what is wrong with the values */
static const char* track_params_why(const suma_track_params& q) {
  if (!(q.join_dist <= 1e6f)) return "join_dist must not be a NaN and at most 1e6 (negative: joining off)";
  if (!(q.gate_base >= 0.0f && q.gate_base <= 1e6f)) return "gate_base must lie in 0 .. 1e6";
  if (!(q.gate_speed >= 0.0f && q.gate_speed <= 1e6f)) return "gate_speed must lie in 0 .. 1e6";
  if (!(q.alpha >= 0.0f && q.alpha <= 1.0f)) return "alpha must lie in 0 .. 1";
  if (!(q.beta >= 0.0f && q.beta <= 2.0f)) return "beta must lie in 0 .. 2";
  if (q.confirm_hits < 1u || q.confirm_hits > 65535u) return "confirm_hits must be 1 .. 65535";
  if (q.max_missed > 65535u) return "max_missed must be 0 .. 65535";
  if (q.max_tracks < 1u || q.max_tracks > 4096u) return "max_tracks must be 1 .. 4096";
  if (q.max_rounds < 1u || q.max_rounds > 64u) return "max_rounds must be 1 .. 64";
  return nullptr;
}

extern "C" int suma_track_params_check(const suma_track_params* tp) {
  if (!tp) return fail_without_ctx(SUMA_ERR_INVALID, "suma_track_params_check: NULL parameters");
  if (const char* why = track_params_why(*tp)) return fail_without_ctx(SUMA_ERR_INVALID, std::string("suma_track_params_check: ") + why);
  return SUMA_OK;
}

static int tracks_ready(suma_localizer* l, const char* who) {
  if (!l->tk.on) return fail(l->c, SUMA_ERR_INVALID, std::string(who) + ": tracks are off (suma_localizer_enable_tracks)");
  return SUMA_OK;
}

extern "C" int suma_localizer_enable_tracks(suma_localizer* l, const suma_track_params* tp) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  if (!l->ob.on)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_enable_tracks: objects are off (suma_localizer_enable_objects): the "
                                     "tracks are made of their records");
  suma_track_params q;
  suma_track_params_default(&q);
  if (tp) q = *tp;
  if (const char* why = track_params_why(q)) return fail(c, SUMA_ERR_INVALID, std::string("suma_localizer_enable_tracks: ") + why);
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* an update may still write the old blocks */
  l->tk.on = false;
  int r = tracks_alloc(c, l->tk, q, l->ob.op.max_objects);
  if (r) return r;
  l->tk.on = true;
  return SUMA_OK;
}

extern "C" int suma_localizer_disable_tracks(suma_localizer* l) {
  return l ? disable_layer(l, LAYER_TRACKS) : SUMA_ERR_INVALID;
}

extern "C" int suma_localizer_clear_tracks(suma_localizer* l) {
  if (!l) return SUMA_ERR_INVALID;
  int r = tracks_ready(l, "suma_localizer_clear_tracks");
  if (r) return r;
  return tracks_clear(l->c, l->tk);
}

/* the words of the tracker into host words (blocking) */
static int tracks_words(suma_localizer* l, uint32_t* out) {
  return read_words(l, l->tk.words, TRK_WORDS * sizeof(uint32_t), out);
}

static int tracks_download(suma_localizer* l, suma_object_track* out, uint32_t capacity, uint32_t* n, suma_track_counts* counts,
                           int32_t* updated, bool to_device, const char* who) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = tracks_ready(l, who);
  if (r) return r;
  if (!n || (capacity && !out)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL argument");
  *n = 0;
  if (counts) memset(counts, 0, sizeof(*counts));
  if (updated) *updated = l->tk.updated;
  if (!l->tk.updated) return SUMA_OK;
  uint32_t w[TRK_WORDS];
  if ((r = tracks_words(l, w))) return r;
  suma_track_counts cnt;
  memcpy(&cnt, w, sizeof(cnt));
  if (counts) *counts = cnt;
  if ((r = download(c, out, capacity, n, l->tk.out, w[TRK_N_LIVE], sizeof(suma_object_track), to_device))) return r;
  if (cnt.n_dropped)
    return fail(c, SUMA_ERR_CAPACITY, std::string(who) + ": " + std::to_string(cnt.n_dropped) +
                                      " detections found no free slot among max_tracks = " + std::to_string(l->tk.tp.max_tracks));
  return SUMA_OK;
}

extern "C" int suma_localizer_tracks(suma_localizer* l, suma_object_track* host, uint32_t capacity, uint32_t* n,
                                     suma_track_counts* counts, int32_t* updated) {
  return tracks_download(l, host, capacity, n, counts, updated, false, "suma_localizer_tracks");
}

extern "C" int suma_localizer_tracks_device(suma_localizer* l, suma_object_track* d_out, uint32_t capacity, uint32_t* n,
                                            suma_track_counts* counts, int32_t* updated) {
  return tracks_download(l, d_out, capacity, n, counts, updated, true, "suma_localizer_tracks_device");
}

extern "C" int suma_localizer_object_tracks(suma_localizer* l, uint32_t* host, uint32_t capacity, uint32_t* n) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = tracks_ready(l, "suma_localizer_object_tracks");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_object_tracks: NULL argument");
  *n = 0;
  if (!l->tk.updated) return SUMA_OK;
  uint32_t w[TRK_WORDS];
  if ((r = tracks_words(l, w))) return r;
  return download(c, host, capacity, n, l->tk.objtrack, w[0] /* n_objects */, sizeof(uint32_t), false);
}

extern "C" int suma_localizer_track_objects(suma_localizer* l, const suma_scan_object* host_objects, uint32_t n, uint32_t scan_id,
                                            suma_track_counts* counts) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  const char* who = "suma_localizer_track_objects";
  int r = tracks_ready(l, who);
  if (r) return r;
  if (n && !host_objects) return fail(c, SUMA_ERR_INVALID, "suma_localizer_track_objects: NULL records with n > 0");
  Tracks& tk = l->tk;
  if (n > tk.max_objects)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_track_objects: " + std::to_string(n) + " records, max_objects = " +
                                     std::to_string(tk.max_objects));
  if ((r = stamp_check(l, scan_id, tk.last_stamp, "the tracks", who))) return r;
  if (counts) memset(counts, 0, sizeof(*counts));
  if (n) HIP_TRY(c, hipMemcpyAsync(tk.rec_in, host_objects, (size_t)n * sizeof(suma_scan_object), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(tk.words.p + TRK_N_IN, &n, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  r = tracks_update(c, tk, tk.rec_in, tk.words.p + TRK_N_IN, scan_id + 1u);
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* pageable sources: the copies have left them */
  if (r) return r;
  if (!counts) return SUMA_OK;
  uint32_t w[TRK_WORDS];
  if ((r = tracks_words(l, w))) return r;
  memcpy(counts, w, sizeof(*counts));
  return SUMA_OK;
}

extern "C" int suma_localizer_track_state(suma_localizer* l, suma_object_track* host, uint32_t capacity, uint32_t* n,
                                          uint32_t* last_stamp, uint32_t* next_id) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = tracks_ready(l, "suma_localizer_track_state");
  if (r) return r;
  if (!n || (capacity && !host)) return fail(c, SUMA_ERR_INVALID, "suma_localizer_track_state: NULL argument");
  *n = l->tk.tp.max_tracks; /* also when the read below fails */
  uint32_t w[TRK_WORDS];
  if ((r = tracks_words(l, w))) return r;
  if (last_stamp) *last_stamp = l->tk.last_stamp;
  if (next_id) *next_id = w[TRK_BORN_TOTAL] + 1u;
  return download(c, host, capacity, n, l->tk.slots, l->tk.tp.max_tracks, sizeof(suma_object_track), false);
}

extern "C" int suma_localizer_set_track_state(suma_localizer* l, const suma_object_track* host, uint32_t n, uint32_t last_stamp,
                                              uint32_t next_id) {
  if (!l) return SUMA_ERR_INVALID;
  suma_ctx* c = l->c;
  int r = tracks_ready(l, "suma_localizer_set_track_state");
  if (r) return r;
  if (!host) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: NULL argument");
  Tracks& tk = l->tk;
  if (n != tk.tp.max_tracks)
    return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: " + std::to_string(n) + " slots, max_tracks = " +
                                     std::to_string(tk.tp.max_tracks));
  if (next_id < 1u) return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: next_id must be at least 1");
  for (uint32_t k = 0; k < n; ++k) {
    const suma_object_track& t = host[k];
    if (t.state > SUMA_TRACK_CONFIRMED)
      return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: slot " + std::to_string(k) + " has no valid state");
    if (t.state == SUMA_TRACK_FREE) continue;
    if (t.id < 1u || t.id >= next_id)
      return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: slot " + std::to_string(k) + " carries an id outside 1 .. next_id - 1");
    if (t.first_stamp > t.last_matched || t.last_matched > last_stamp)
      return fail(c, SUMA_ERR_INVALID, "suma_localizer_set_track_state: slot " + std::to_string(k) + " carries a stamp above last_stamp");
  }
  if ((r = tracks_clear(c, tk))) return r;
  const uint32_t born = next_id - 1u;
  HIP_TRY(c, hipMemcpyAsync(tk.slots, host, (size_t)n * sizeof(suma_object_track), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(tk.words.p + TRK_BORN_TOTAL, &born, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* pageable sources: the copies have left them */
  tk.last_stamp = last_stamp;
  return SUMA_OK;
}
