/*
 * suma_loop.hip -- loop closing inside the scan pipeline: SurfelMapping::checkLoopClosure and the pose-graph bookkeeping
 * around it (SurfelMapping.cpp:42-60, :212-253, :461-471, :478-518, :527-795, :819-826).  Host code: the state machine is
 * the reference's, statement for statement; its device work goes through suma_pipeline_verify_loop_closure,
 * suma_pipeline_track_loop_closure, suma_posegraph_* and k_loop.hip.  `float` where the reference has float: every
 * ratio below is IEEE fp32 arithmetic (0 / 0 = NaN, comparisons with it are false).  4x4 products and rigid inverses are
 * mat4_mul / mat4_rigid_inv (suma_internal.h), the library's one fixed operation order.
 *
 * Left out: loopClosurePoses_ (bookkeeping for the visualizer) and genResidualPlot.
 */
#include <math.h>
#include <string.h>

#include <cmath>

#include <atomic>
#include <new>
#include <thread>
#include <vector>

#include "suma_internal.h"

namespace {

struct LoopCandidate { /* SurfelMapping.h:124-128 */
  int32_t from, to;
  double rel_pose[16];
};

struct OptResult { /* SurfelMapping.h:112-122 */
  double error = 10000.0, residual = 10000.0, inlier_residual = 10000.0;
  uint32_t inlier = 0, outlier = 0, valid = 0, invalid = 0;
  float outlier_ratio = 1.0f;
};

}  // namespace

struct LoopState {
  suma_loop_params p;
  suma_posegraph* graph = nullptr;
  std::vector<float> trajectory_distances; /* a float accumulator over double norms (:461-471) */
  std::vector<LoopCandidate> unverified, verified;
  bool already_verified = false;
  uint32_t loop_count = 0, time_without = 0;
  /* optimizeAsync (:819-826).  The reference's worker reads timestamp_ and loopCount_ whenever it gets to run; here they
   * are the values at the start (:657-658) */
  bool optimizing = false;
  suma_posegraph* opt_graph = nullptr;
  std::thread worker;
  std::atomic<int> worker_done{0};
  int worker_rc = SUMA_OK;
  int32_t before_id = 0;
  uint32_t before_loop_count = 0, started_at = 0;
  double before_pose[16];
  DevBuf<double> d_tail; /* the tail rows of an integration, column-major doubles */
  bool checked = false;  /* checkLoopClosure has run for the scan in flight */
  /* per-scan part of suma_loop_status */
  bool found = false, use = false, started = false, integrated = false;
  int32_t candidate_to = -1;
  uint32_t edges_added = 0;
  OptResult result_old;
  float loop_valid_ratio = 0, loop_outlier_ratio = 0, loop_relative_error_all = 0;
  double posegraph_error = 0;
};

namespace {

int pg_fail_to_ctx(suma_ctx* c, const suma_posegraph* g, int rc, const char* what) {
  return fail(c, rc, std::string(what) + ": " + suma_posegraph_last_error(g));
}
#define PG_TRY(c, g, expr)                                   \
  do {                                                       \
    int rc__ = (expr);                                       \
    if (rc__ != SUMA_OK) return pg_fail_to_ctx(c, g, rc__, #expr); \
  } while (0)

/* |a.col(3) - b.col(3)| (pose_distance, :499-501); the fourth components are both 1 */
double translation_distance(const double* ta, const double* tb) {
  const double dx = ta[0] - tb[0], dy = ta[1] - tb[1], dz = ta[2] - tb[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

/* getCandidateIndexes / getClosestIndex (:478-518): one loop, twice in the reference.  base + j * stride = t of pose j */
int32_t find_candidate(const double* base, size_t stride, const float* traj, uint32_t timestamp, const double* t_current,
                       float radius, float min_trajectory_distance, int32_t delta_timestamp) {
  int32_t closest_idx = -1;
  float min_distance = radius;
  for (int64_t j = (int64_t)timestamp - delta_timestamp; j >= 0; --j) {
    const float distance = (float)translation_distance(t_current, base + (size_t)j * stride);
    const float tdistance = traj[timestamp] - traj[j];
    if (distance < min_distance && tdistance > min_trajectory_distance) {
      closest_idx = (int32_t)j;
      min_distance = distance;
    }
  }
  return closest_idx;
}

int32_t closest_index(const suma_pipeline* s) {
  const LoopState* L = s->loop;
  uint32_t n = 0;
  const double* P = posegraph_host_poses(L->graph, &n);
  if (s->timestamp >= n || s->timestamp >= L->trajectory_distances.size()) return -1;
  int64_t first = (int64_t)s->timestamp - L->p.delta_timestamp;
  if (first >= (int64_t)n) return -1;
  return find_candidate(P + 9, 12, L->trajectory_distances.data(), s->timestamp, s->current_pose + 12,
                        L->p.search_distance, L->p.min_trajectory_distance, L->p.delta_timestamp);
}

/* the graph grows with the sequence: capacities double when the next node / edges would not fit */
int graph_room(suma_ctx* c, LoopState* L, uint32_t more_edges) {
  const uint32_t n = (uint32_t)suma_posegraph_size(L->graph), m = suma_posegraph_edge_count(L->graph);
  uint32_t nc = L->p.node_capacity ? L->p.node_capacity : 1u;
  while (nc < n + 1) nc *= 2;
  uint32_t ec = 2 * nc;
  while (ec < m + more_edges) ec *= 2;
  PG_TRY(c, L->graph, suma_posegraph_reserve(L->graph, nc, ec));
  return SUMA_OK;
}

void join_worker(LoopState* L) {
  if (L->worker.joinable()) L->worker.join();
}

void drop_optimisation(LoopState* L) {
  join_worker(L);
  if (L->opt_graph) suma_posegraph_destroy(L->opt_graph);
  L->opt_graph = nullptr;
  L->optimizing = false;
  L->worker_done.store(0);
}

}  // namespace

void loop_destroy(suma_pipeline* s) {
  LoopState* L = s->loop;
  if (!L) return;
  drop_optimisation(L); /* ~SurfelMapping waits for the future (:64-66) */
  if (L->graph) suma_posegraph_destroy(L->graph);
  delete L;
  s->loop = nullptr;
}

/* the constructor's state (:42-47; reset(), :158-164) */
int loop_reset(suma_pipeline* s) {
  LoopState* L = s->loop;
  if (!L) return SUMA_OK;
  suma_ctx* c = s->c;
  drop_optimisation(L);
  PG_TRY(c, L->graph, suma_posegraph_clear(L->graph));
  double I[16];
  mat4_eye(I);
  PG_TRY(c, L->graph, suma_posegraph_set_initial(L->graph, 0, I));
  L->trajectory_distances.assign(1, 0.0f);
  L->unverified.clear(), L->verified.clear();
  L->already_verified = false;
  L->loop_count = 0, L->time_without = 0;
  L->checked = false;
  L->found = L->use = L->started = L->integrated = false;
  L->candidate_to = -1, L->edges_added = 0;
  L->result_old = OptResult();
  L->loop_valid_ratio = L->loop_outlier_ratio = L->loop_relative_error_all = 0.0f;
  L->posegraph_error = 0.0;
  return SUMA_OK;
}

extern "C" void suma_loop_params_default(suma_loop_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->residual_threshold = 1.05f; /* SurfelMapping.h:221-228 */
  p->outlier_threshold = 1.1f;
  p->valid_threshold = 0.9f;
  p->search_distance = 20.0f;
  p->min_trajectory_distance = 200.0f;
  p->min_verifications = 3;
  p->delta_timestamp = 100;
  p->optimize_wait = 1;
  p->min_valid_ratio = 0.2; /* :567, :713 */
  p->max_outlier_ratio = 0.85;
  p->max_increment_difference = 0.1;
  for (int k = 0; k < 6; ++k) p->information[7 * k] = 1.0; /* :49-59, transNoise = rotNoise = 1 */
  p->optimize_iterations = 100;
  p->integrate_lag = 0;
  p->node_capacity = 1024;
}

extern "C" int suma_pipeline_enable_loop_closing(suma_pipeline* s, const suma_loop_params* params) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  if (s->phase != 0) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_enable_loop_closing: only between scans");
  if (!params) {
    loop_destroy(s);
    return SUMA_OK;
  }
  bool finite = true;
  for (int i = 0; i < 36; ++i) finite = finite && std::isfinite(params->information[i]);
  if (!finite || params->node_capacity == 0 || params->node_capacity > (1u << 30) || params->delta_timestamp < 0 ||
      params->min_verifications < 0)
    return fail(c, SUMA_ERR_INVALID, "suma_pipeline_enable_loop_closing: bad parameters");
  loop_destroy(s);
  LoopState* L = new (std::nothrow) LoopState();
  if (!L) return fail(c, SUMA_ERR_NOMEM, "out of host memory");
  L->p = *params;
  int rc = suma_posegraph_create(c->device, params->node_capacity, 2 * params->node_capacity, &L->graph);
  if (rc != SUMA_OK) {
    delete L;
    return fail(c, rc, std::string("suma_posegraph_create: ") + suma_posegraph_last_error(nullptr));
  }
  s->loop = L;
  rc = loop_reset(s);
  if (rc != SUMA_OK) loop_destroy(s);
  return rc;
}

extern "C" suma_posegraph* suma_pipeline_posegraph(suma_pipeline* s) { return s && s->loop ? s->loop->graph : nullptr; }

extern "C" int suma_pipeline_trajectory_distances(const suma_pipeline* s, float* out, uint32_t capacity, uint32_t* n) {
  if (!s || !n || (!out && capacity)) return SUMA_ERR_INVALID;
  if (!s->loop) return fail(s->c, SUMA_ERR_INVALID, "suma_pipeline_trajectory_distances: loop closing is not enabled");
  const std::vector<float>& t = s->loop->trajectory_distances;
  *n = (uint32_t)t.size();
  const size_t k = t.size() < capacity ? t.size() : capacity;
  if (k) memcpy(out, t.data(), k * sizeof(float));
  return SUMA_OK;
}

extern "C" int32_t suma_loop_find_candidate(const double* poses16, const float* trajectory_distances, uint32_t timestamp,
                                            const double current_pose[16], float radius, float min_trajectory_distance,
                                            int32_t delta_timestamp) {
  if (!poses16 || !trajectory_distances || !current_pose) return -1;
  return find_candidate(poses16 + 12, 16, trajectory_distances, timestamp, current_pose + 12, radius,
                        min_trajectory_distance, delta_timestamp);
}

extern "C" int suma_pipeline_loop_status(const suma_pipeline* s, suma_loop_status* o) {
  if (!s || !o) return SUMA_ERR_INVALID;
  const LoopState* L = s->loop;
  if (!L) return fail(s->c, SUMA_ERR_INVALID, "suma_pipeline_loop_status: loop closing is not enabled");
  memset(o, 0, sizeof(*o));
  o->found_candidate = L->found, o->use_candidate = L->use;
  o->candidate_to = L->candidate_to;
  o->n_unverified = (uint32_t)L->unverified.size();
  o->already_verified = L->already_verified;
  o->loop_count = (int32_t)L->loop_count;
  o->time_without_loop_closure = L->time_without;
  o->currently_optimizing = L->optimizing;
  o->started_optimization = L->started, o->integrated = L->integrated;
  o->edges_added = L->edges_added;
  o->result_old_outlier_ratio = L->result_old.outlier_ratio;
  o->result_old.error = L->result_old.error;
  o->result_old.inlier_residual = L->result_old.inlier_residual;
  o->result_old.valid = L->result_old.valid, o->result_old.outlier = L->result_old.outlier;
  o->result_old.inlier = L->result_old.inlier, o->result_old.invalid = L->result_old.invalid;
  o->result_old_residual = L->result_old.residual;
  o->loop_valid_ratio = L->loop_valid_ratio, o->loop_outlier_ratio = L->loop_outlier_ratio;
  o->loop_relative_error_all = L->loop_relative_error_all;
  o->posegraph_error = L->posegraph_error;
  return SUMA_OK;
}

namespace {

/* the body of integrateLoopClosures (:219-250) for the finished optimisation in L->opt_graph */
int integrate_result(suma_pipeline* s) {
  LoopState* L = s->loop;
  suma_ctx* c = s->c;
  suma_posegraph* og = L->opt_graph;
  if (L->worker_rc != SUMA_OK) return pg_fail_to_ctx(c, og, L->worker_rc, "suma_posegraph_optimize (loop closing)");
  uint32_t n_opt = 0, n_before = 0, n_dev = 0;
  const double* opt = posegraph_host_poses(og, &n_opt); /* the host copy the optimiser fetched */
  const double* d_opt = posegraph_device_poses(og, &n_dev);
  (void)posegraph_host_poses(L->graph, &n_before);
  /* checked before the first pose is handed over, so that a refused result leaves the pipeline's graph as it was */
  if (n_dev != n_opt || n_before < n_opt || (uint32_t)L->before_id >= n_opt)
    return fail(c, SUMA_ERR_INVALID, "loop closing: the optimised graph does not fit the pipeline's graph");
  for (size_t i = 0; i < 12 * (size_t)n_opt; ++i)
    if (!std::isfinite(opt[i])) return fail(c, SUMA_ERR_INVALID, "loop closing: the optimisation gave a non-finite pose");
  double T[16], before_inv[16], difference[16];
  for (uint32_t i = 0; i < n_opt; ++i) { /* :219-222 */
    PG_TRY(c, og, suma_posegraph_pose(og, (int32_t)i, T));
    PG_TRY(c, L->graph, suma_posegraph_set_initial(L->graph, (int32_t)i, T));
  }
  L->loop_count -= L->before_loop_count; /* :224 */
  PG_TRY(c, og, suma_posegraph_pose(og, L->before_id, T));
  mat4_rigid_inv(L->before_pose, before_inv);
  mat4_mul(T, before_inv, difference); /* :225 */
  const uint32_t n_tail = n_before - n_opt;
  std::vector<double> tail(16 * (size_t)n_tail);
  for (uint32_t i = 0; i < n_tail; ++i) { /* :227-231 */
    double* B = tail.data() + 16 * (size_t)i;
    PG_TRY(c, L->graph, suma_posegraph_pose(L->graph, (int32_t)(n_opt + i), B));
    mat4_mul(difference, B, T);
    PG_TRY(c, L->graph, suma_posegraph_set_initial(L->graph, (int32_t)(n_opt + i), T));
  }
  /* map_->updatePoses (:233): from the optimiser's device buffer; only the tail's inputs are uploaded */
  if (n_tail) {
    if (grow(c, L->d_tail, 16 * (size_t)n_tail, {c->stream}) < 0) return SUMA_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(L->d_tail, tail.data(), tail.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, launch_loop_integrate(c, d_opt, n_opt, L->d_tail, n_tail, difference));
  HIP_TRY(c, hipStreamSynchronize(c->stream)); /* `tail` and the clone's buffer go away below */
  c->map_version++;
  drop_optimisation(L); /* currentlyOptimizing_ = false (:235) */
  double np[16];
  mat4_mul(difference, s->current_pose, np); /* :236 */
  memcpy(s->current_pose, np, sizeof(np));
  memcpy(s->pose_old, np, sizeof(np)); /* :240 */
  memcpy(s->pose_new, np, sizeof(np));
  /* :242-250 */
  uint32_t n = 0;
  const double* P = posegraph_host_poses(L->graph, &n);
  L->trajectory_distances.resize(n);
  const double* last = P + 9;
  float distance = 0;
  for (uint32_t t = 0; t < n; ++t) {
    distance += translation_distance(last, P + 12 * (size_t)t + 9);
    L->trajectory_distances[t] = distance;
    last = P + 12 * (size_t)t + 9;
  }
  L->integrated = true;
  return SUMA_OK;
}

}  // namespace

/* integrateLoopClosures (:212-253) at the start of a scan; also opens the scan's status record */
int loop_integrate(suma_pipeline* s) {
  LoopState* L = s->loop;
  L->checked = false;
  L->found = L->use = L->started = L->integrated = false;
  L->candidate_to = -1, L->edges_added = 0;
  L->result_old = OptResult();
  L->loop_valid_ratio = L->loop_outlier_ratio = L->loop_relative_error_all = 0.0f;
  L->posegraph_error = 0.0;
  if (!L->optimizing) return SUMA_OK;
  if (L->p.optimize_wait) {
    if (s->timestamp < L->started_at + 1u + L->p.integrate_lag) return SUMA_OK;
  } else if (!L->worker_done.load(std::memory_order_acquire)) {
    return SUMA_OK; /* the reference gives the future 5 ms (:214); here the poll does not wait at all */
  }
  join_worker(L);
  const int rc = integrate_result(s);
  /* a result that could not be integrated is given up with its error reported once: the next scans go on, and a later
   * optimisation may start (:655-660) */
  if (rc != SUMA_OK) drop_optimisation(L);
  return rc;
}

/* the tail of updatePose (:461-471), after the pose bookkeeping; last_increment is the applied increment (the
 * fallback's when it fired) */
int loop_odometry_edge(suma_pipeline* s) {
  LoopState* L = s->loop;
  suma_ctx* c = s->c;
  const uint32_t t = s->timestamp;
  if (t == 0) return SUMA_OK;
  if ((uint32_t)suma_posegraph_size(L->graph) != t || L->trajectory_distances.size() != t)
    return fail(c, SUMA_ERR_INVALID, "loop closing: the graph is not in step with the pipeline (enable it before the first scan or after a reset)");
  int r = graph_room(c, L, 1);
  if (r) return r;
  double prev[16], T[16];
  PG_TRY(c, L->graph, suma_posegraph_pose(L->graph, (int32_t)t - 1, prev));
  mat4_mul(prev, s->last_increment, T);
  PG_TRY(c, L->graph, suma_posegraph_set_initial(L->graph, (int32_t)t, T)); /* :464 */
  PG_TRY(c, L->graph, suma_posegraph_add_edge(L->graph, (int32_t)t - 1, (int32_t)t, s->last_increment, L->p.information));
  float distance = 0;
  distance = (float)translation_distance(prev + 12, s->current_pose + 12); /* :467 */
  distance += L->trajectory_distances[t - 1];
  L->trajectory_distances.push_back(distance);
  return SUMA_OK;
}

static void worker_main(LoopState* L) {
  L->worker_rc = suma_posegraph_optimize(L->opt_graph, L->p.optimize_iterations, nullptr, nullptr); /* :825 */
  L->worker_done.store(1, std::memory_order_release);
}

/* checkLoopClosure (:527-795) */
int loop_check(suma_pipeline* s) {
  LoopState* L = s->loop;
  suma_ctx* c = s->c;
  const suma_loop_params& p = L->p;
  const uint32_t timestamp = s->timestamp;
  suma_icp_stats rn; /* result_new_ (:417-423) */
  int r = suma_pipeline_result_new(s, &rn);
  if (r) return r;
  const double result_new_residual = rn.error / (double)(rn.inlier + rn.outlier); /* :420 */

  L->found = false;
  L->result_old = OptResult(); /* reset. */
  L->use = false;
  OptResult& ro = L->result_old;

  bool candidateAdded = false;
  bool haveMinCandidate = false; /* minCandidate > -1 */

  const float outlier_ratio_new = (float)rn.outlier / (float)(rn.outlier + rn.inlier);
  const float valid_ratio_new = (float)rn.valid / (float)(rn.invalid + rn.valid);

  L->time_without += 1;

  /* 1. verify loop closure if there are unverified loop closures (:551-625) */
  if (L->unverified.size() > 0 || L->already_verified) {
    suma_loop_track tr;
    r = suma_pipeline_track_loop_closure(s, p.min_valid_ratio, p.max_outlier_ratio, p.max_increment_difference, &tr);
    if (r) return r;
    if (tr.passed) {
      const float error = (float)tr.composed.error;
      const float residual = error / (float)(tr.composed.inlier + tr.composed.outlier);
      ro.error = error;
      ro.inlier = tr.composed.inlier;
      ro.outlier = tr.composed.outlier;
      ro.residual = ro.error / (float)(ro.inlier + ro.outlier); /* :582 */
      ro.inlier_residual = (float)tr.composed.inlier_residual / (float)ro.inlier;
      ro.valid = tr.composed.valid;
      ro.invalid = tr.composed.invalid;

      const float rel_error_all = (float)(residual / result_new_residual);

      L->found = true;
      memcpy(s->pose_old, tr.pose_old, sizeof(s->pose_old)); /* currentPose_old_ = lastPose_old_ * increment_old (:590) */

      const bool loop_closure = (rel_error_all < p.residual_threshold) || ((double)residual - result_new_residual) < 0.1;
      if (loop_closure) {
        L->time_without = 0;
        const int32_t index = closest_index(s); /* getClosestIndex ignores its argument (:508) */
        if (index > -1) {
          LoopCandidate cand;
          cand.from = (int32_t)timestamp;
          cand.to = index;
          double nearest[16], inv[16];
          PG_TRY(c, L->graph, suma_posegraph_pose(L->graph, index, nearest));
          mat4_rigid_inv(s->pose_old, inv);
          mat4_mul(inv, nearest, cand.rel_pose); /* :606 */
          L->candidate_to = index;
          (L->already_verified ? L->verified : L->unverified).push_back(cand);
        }
        L->use = true;
      }
    }
  }

  /* enough verified loop closures (:628-633) */
  if (!L->already_verified && (int32_t)L->unverified.size() >= (p.min_verifications + 1)) {
    for (size_t i = 0; i < L->unverified.size(); ++i) L->verified.push_back(L->unverified[i]);
    L->unverified.clear();
    L->already_verified = true;
  }

  /* 2. Add verified loop closures (:635-653) */
  int32_t lastFrom = -1;
  if (!L->verified.empty()) {
    r = graph_room(c, L, (uint32_t)L->verified.size());
    if (r) return r;
  }
  for (const LoopCandidate& cand : L->verified) {
    if (lastFrom != cand.from) {
      lastFrom = cand.from;
      L->loop_count += 1;
    }
    PG_TRY(c, L->graph, suma_posegraph_add_edge(L->graph, cand.from, cand.to, cand.rel_pose, p.information));
    L->edges_added += 1;
  }
  L->verified.clear();

  /* :655-660 */
  if ((L->loop_count > 6 && !L->optimizing) || (L->loop_count > 0 && !L->optimizing && (L->time_without > 3))) {
    PG_TRY(c, L->graph, suma_posegraph_clone(L->graph, &L->opt_graph));
    L->optimizing = true; /* optimizeAsync (:820-823) */
    L->before_id = (int32_t)timestamp;
    L->before_loop_count = L->loop_count;
    L->started_at = timestamp;
    PG_TRY(c, L->opt_graph, suma_posegraph_pose(L->opt_graph, (int32_t)timestamp, L->before_pose));
    L->worker_done.store(0);
    L->worker_rc = SUMA_OK;
    L->worker = std::thread(worker_main, L);
    L->started = true;
  }

  if (L->time_without > 3) { /* :662-779 */
    L->unverified.clear(); /* drop unverified. */
    L->use = false;
    L->already_verified = false;

    const int32_t to = closest_index(s); /* getCandidateIndexes(loopClosureSearchDist_): at most one */
    int32_t loopClosureTimestamp = -1;
    if (to > -1) {
      double pose_prior[16], prior_inv[16], inits[3 * 16];
      PG_TRY(c, L->graph, suma_posegraph_pose(L->graph, to, pose_prior));
      mat4_rigid_inv(pose_prior, prior_inv);
      double* O = inits;
      mat4_mul(prior_inv, s->current_pose, O); /* :680 */
      O[14] = 0.0;                             /* O(2, 3) = 0 */
      memcpy(inits + 16, O, 16 * sizeof(double)); /* R(O), :520-525 */
      inits[16 + 12] = inits[16 + 13] = inits[16 + 14] = 0.0;
      memcpy(inits + 32, O, 16 * sizeof(double)); /* :687-689 */
      inits[32 + 12] = 0.5 * O[12];
      inits[32 + 13] = 0.5 * O[13];
      suma_loop_result res[3];
      r = suma_pipeline_verify_loop_closure(s, pose_prior, inits, 3, (float)p.min_valid_ratio, (float)p.max_outlier_ratio,
                                            res);
      if (r) return r;
      for (int i = 0; i < 3; ++i) {
        L->found = true; /* :709 */
        if (!res[i].passed) continue;
        const suma_icp_stats& cs = res[i].composed;
        const float error = (float)cs.error;
        const float residual = error / (float)(cs.inlier + cs.outlier);
        const float outlier_ratio_old = (float)cs.outlier / (float)(cs.outlier + cs.inlier);
        const float valid_ratio_old = (float)cs.valid / (float)(cs.valid + cs.invalid);

        const float rel_error_all = (float)(residual / result_new_residual);
        const float rel_valid_ratio = valid_ratio_old / valid_ratio_new;
        const float rel_outlier_ratio = outlier_ratio_old / outlier_ratio_new;

        if (!candidateAdded || ((double)residual < ro.residual && outlier_ratio_old < ro.outlier_ratio)) {
          if (rel_valid_ratio >= p.valid_threshold && rel_outlier_ratio < p.outlier_threshold) {
            candidateAdded = true;
            loopClosureTimestamp = to;
            haveMinCandidate = true;

            ro.error = error;
            ro.inlier = cs.inlier;
            ro.outlier = cs.outlier;
            ro.outlier_ratio = outlier_ratio_old;
            ro.valid = cs.valid;
            ro.residual = ro.error / (double)ro.valid; /* :746: by valid, not by inlier + outlier */
            ro.inlier_residual = (float)cs.inlier_residual / (float)ro.inlier;
            ro.invalid = cs.invalid;

            const bool loop_closure =
                (rel_error_all < p.residual_threshold) || ((double)residual - result_new_residual) < 0.1;
            if (loop_closure) mat4_mul(pose_prior, res[i].gn_pose, s->pose_old); /* :752 */
          }
        }
      }
    }

    if (haveMinCandidate) { /* :762-774 */
      LoopCandidate cand;
      cand.from = (int32_t)timestamp;
      cand.to = loopClosureTimestamp;
      double target[16], inv[16];
      PG_TRY(c, L->graph, suma_posegraph_pose(L->graph, cand.to, target));
      mat4_rigid_inv(s->pose_old, inv);
      mat4_mul(inv, target, cand.rel_pose);
      L->candidate_to = cand.to;
      L->unverified.push_back(cand);
    }
  }

  /* :781-793 */
  const float valid_ratio_old = (float)ro.valid / (float)(ro.valid + ro.invalid);
  const float outlier_ratio_old = (float)ro.outlier / (float)(ro.outlier + ro.inlier);
  L->loop_valid_ratio = valid_ratio_old / valid_ratio_new;
  L->loop_outlier_ratio = outlier_ratio_old / outlier_ratio_new;
  L->loop_relative_error_all = (float)(ro.residual / result_new_residual);
  PG_TRY(c, L->graph, suma_posegraph_error(L->graph, &L->posegraph_error));
  L->checked = true;
  return SUMA_OK;
}

extern "C" int suma_pipeline_check_loop_closure(suma_pipeline* s) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  if (!s->loop) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_check_loop_closure: loop closing is not enabled (suma_pipeline_enable_loop_closing)");
  if (s->phase != 2) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_check_loop_closure: between suma_pipeline_update_pose and suma_pipeline_update_map (SurfelMapping.cpp:196)");
  if (s->loop->checked) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_check_loop_closure: already run for this scan");
  if (s->timestamp == 0) { /* :190: nothing to check, but the scan's one call has been made */
    s->loop->checked = true;
    return SUMA_OK;
  }
  return loop_check(s);
}

/* ---- checkpoint: the LOOP / GRAPH / OPT payloads (checkpoint_format.h; k_checkpoint.hip states the image) ---- */
#include "checkpoint_format.h"

static_assert(sizeof(suma_loop_params) % 8 == 0, "the LOOP payload keeps its doubles aligned");

namespace {

template <class T>
void put(std::vector<char>* v, const T* p, size_t n = 1) {
  const char* b = reinterpret_cast<const char*>(p);
  v->insert(v->end(), b, b + n * sizeof(T));
}
void put_candidates(std::vector<char>* v, const std::vector<LoopCandidate>& cs) {
  for (const LoopCandidate& q : cs) {
    ckpt::Candidate o;
    o.from = q.from, o.to = q.to;
    memcpy(o.rel_pose, q.rel_pose, sizeof(o.rel_pose));
    put(v, &o);
  }
}
bool finite_all(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}
bool loop_params_ok(const suma_loop_params& p) {
  return finite_all(p.information, 36) && p.node_capacity != 0 && p.node_capacity <= (1u << 30) && p.delta_timestamp >= 0 &&
         p.min_verifications >= 0;
}
void rigid12_to_mat4(const double* o, double* T) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[j * 4 + i] = o[i * 3 + j];
    T[12 + i] = o[9 + i];
    T[i * 4 + 3] = 0.0;
  }
  T[15] = 1.0;
}

}  // namespace

void loop_ckpt_join(suma_pipeline* s) {
  if (s->loop) join_worker(s->loop);
}

uint64_t loop_ckpt_sizes(const suma_pipeline* s, uint64_t* graph_bytes, uint64_t* opt_bytes) {
  const LoopState* L = s->loop;
  *graph_bytes = *opt_bytes = 0;
  if (!L) return 0;
  uint32_t n = 0, n_opt = 0;
  (void)posegraph_host_poses(L->graph, &n);
  *graph_bytes = sizeof(ckpt::GraphHead) + 192ull * n + (uint64_t)sizeof(ckpt::Edge) * suma_posegraph_edge_count(L->graph);
  if (L->optimizing && L->opt_graph) {
    (void)posegraph_host_poses(L->opt_graph, &n_opt);
    *opt_bytes = sizeof(ckpt::OptHead) + 96ull * n_opt;
  }
  return sizeof(ckpt::LoopHead) + sizeof(suma_loop_params) + ((4ull * L->trajectory_distances.size() + 7) & ~7ull) +
         (uint64_t)sizeof(ckpt::Candidate) * (L->unverified.size() + L->verified.size());
}

int loop_ckpt_write(suma_pipeline* s, std::vector<char>* loop, std::vector<char>* graph, std::vector<char>* opt) {
  LoopState* L = s->loop;
  suma_ctx* c = s->c;
  ckpt::LoopHead h;
  memset(&h, 0, sizeof(h));
  h.params_bytes = (uint32_t)sizeof(suma_loop_params);
  h.n_traj = (uint32_t)L->trajectory_distances.size();
  h.n_unverified = (uint32_t)L->unverified.size(), h.n_verified = (uint32_t)L->verified.size();
  h.already_verified = L->already_verified;
  h.loop_count = L->loop_count, h.time_without = L->time_without;
  h.found = L->found, h.use = L->use, h.started = L->started, h.integrated = L->integrated;
  h.candidate_to = L->candidate_to, h.edges_added = L->edges_added;
  h.result_old_outlier_ratio = L->result_old.outlier_ratio;
  h.loop_valid_ratio = L->loop_valid_ratio, h.loop_outlier_ratio = L->loop_outlier_ratio;
  h.loop_relative_error_all = L->loop_relative_error_all;
  h.result_old_inlier = L->result_old.inlier, h.result_old_outlier = L->result_old.outlier;
  h.result_old_valid = L->result_old.valid, h.result_old_invalid = L->result_old.invalid;
  h.result_old_error = L->result_old.error, h.result_old_residual = L->result_old.residual;
  h.result_old_inlier_residual = L->result_old.inlier_residual;
  h.posegraph_error = L->posegraph_error;
  put(loop, &h);
  put(loop, &L->p);
  put(loop, L->trajectory_distances.data(), L->trajectory_distances.size());
  if (L->trajectory_distances.size() & 1u) {
    const float zero = 0.0f;
    put(loop, &zero);
  }
  put_candidates(loop, L->unverified);
  put_candidates(loop, L->verified);

  uint32_t n = 0, ni = 0;
  const double* R = posegraph_host_poses(L->graph, &n);
  const double* I = posegraph_host_initial(L->graph, &ni);
  if (ni != n) return fail(c, SUMA_ERR_INVALID, "checkpoint: the pose graph's initial values and estimates differ in number");
  ckpt::GraphHead gh;
  gh.n_nodes = n, gh.n_edges = suma_posegraph_edge_count(L->graph);
  put(graph, &gh);
  for (uint32_t i = 0; i < n; ++i) {
    put(graph, I + 12 * (size_t)i, 12);
    put(graph, R + 12 * (size_t)i, 12);
  }
  for (uint32_t e = 0; e < gh.n_edges; ++e) {
    ckpt::Edge o;
    double Z[16];
    PG_TRY(c, L->graph, suma_posegraph_edge(L->graph, e, &o.from, &o.to, Z, o.information));
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) o.Z[i * 3 + j] = Z[j * 4 + i];
    o.Z[9] = Z[12], o.Z[10] = Z[13], o.Z[11] = Z[14];
    put(graph, &o);
  }
  if (L->optimizing && L->opt_graph) {
    uint32_t n_opt = 0;
    const double* X = posegraph_host_poses(L->opt_graph, &n_opt);
    ckpt::OptHead oh;
    memset(&oh, 0, sizeof(oh));
    oh.before_id = L->before_id, oh.before_loop_count = L->before_loop_count, oh.started_at = L->started_at;
    oh.worker_rc = L->worker_rc, oh.n_opt = n_opt;
    memcpy(oh.before_pose, L->before_pose, sizeof(oh.before_pose));
    put(opt, &oh);
    put(opt, X, 12 * (size_t)n_opt);
  }
  return SUMA_OK;
}

int loop_ckpt_check(suma_ctx* c, const char* loop, const char* graph, const char* opt, uint32_t timestamp,
                    suma_loop_params* params) {
  ckpt::LoopHead h;
  memcpy(&h, loop, sizeof(h));
  if (h.params_bytes != sizeof(suma_loop_params))
    return fail(c, SUMA_ERR_INVALID, "checkpoint: section LOOP holds loop parameters of another size");
  memcpy(params, loop + sizeof(h), sizeof(*params));
  if (!loop_params_ok(*params)) return fail(c, SUMA_ERR_INVALID, "checkpoint: section LOOP: bad loop parameters");
  ckpt::GraphHead gh;
  memcpy(&gh, graph, sizeof(gh));
  const uint32_t want = timestamp ? timestamp : 1u;
  if (gh.n_nodes != want || h.n_traj != want)
    return fail(c, SUMA_ERR_INVALID, "checkpoint: the pose graph is not in step with the timestamp");
  if (gh.n_nodes > (1u << 30) || gh.n_edges > (1u << 29)) return fail(c, SUMA_ERR_CAPACITY, "checkpoint: pose graph too large");
  std::vector<double> buf(24 * (size_t)gh.n_nodes);
  memcpy(buf.data(), graph + sizeof(gh), buf.size() * sizeof(double));
  if (!finite_all(buf.data(), buf.size())) return fail(c, SUMA_ERR_INVALID, "checkpoint: section GRAPH: non-finite pose");
  const char* ep = graph + sizeof(gh) + 192 * (size_t)gh.n_nodes;
  for (uint32_t e = 0; e < gh.n_edges; ++e) {
    ckpt::Edge o;
    memcpy(&o, ep + sizeof(o) * (size_t)e, sizeof(o));
    if (!finite_all(o.Z, 12) || !finite_all(o.information, 36))
      return fail(c, SUMA_ERR_INVALID, "checkpoint: section GRAPH: non-finite edge");
  }
  const char* cp = loop + sizeof(h) + sizeof(suma_loop_params) + ((4 * (size_t)h.n_traj + 7) & ~(size_t)7);
  for (uint32_t k = 0; k < h.n_unverified + h.n_verified; ++k) {
    ckpt::Candidate q;
    memcpy(&q, cp + sizeof(q) * (size_t)k, sizeof(q));
    if (q.from < 0 || q.to < 0 || (uint32_t)q.from > timestamp || (uint32_t)q.to > timestamp || !finite_all(q.rel_pose, 16))
      return fail(c, SUMA_ERR_INVALID, "checkpoint: section LOOP: bad candidate");
  }
  if (opt) {
    ckpt::OptHead oh;
    memcpy(&oh, opt, sizeof(oh));
    if (oh.n_opt == 0 || !finite_all(oh.before_pose, 16))
      return fail(c, SUMA_ERR_INVALID, "checkpoint: section OPT: bad record");
    /* a record the optimiser refused (worker_rc) may hold anything: the integration reports worker_rc before it reads.
     * One it accepted is installed into the clone, which takes finite poses only -- an uninterrupted run would stop at
     * the integration with the same code; here the image is refused before anything is written */
    if (oh.worker_rc == SUMA_OK) {
      std::vector<double> X(12 * (size_t)oh.n_opt);
      memcpy(X.data(), opt + sizeof(oh), X.size() * sizeof(double));
      if (!finite_all(X.data(), X.size())) return fail(c, SUMA_ERR_INVALID, "checkpoint: section OPT: non-finite pose");
    }
  }
  return SUMA_OK;
}

int loop_ckpt_install(suma_pipeline* s, const char* loop, const char* graph, const char* opt) {
  LoopState* L = s->loop;
  suma_ctx* c = s->c;
  ckpt::LoopHead h;
  memcpy(&h, loop, sizeof(h));
  ckpt::GraphHead gh;
  memcpy(&gh, graph, sizeof(gh));
  uint32_t nc = L->p.node_capacity ? L->p.node_capacity : 1u;
  while (nc < gh.n_nodes + 1) nc *= 2;
  uint32_t ec = 2 * nc;
  while (ec < gh.n_edges + 1) ec *= 2;
  PG_TRY(c, L->graph, suma_posegraph_reserve(L->graph, nc, ec));
  std::vector<double> initial(12 * (size_t)gh.n_nodes), result(12 * (size_t)gh.n_nodes);
  for (uint32_t i = 0; i < gh.n_nodes; ++i) {
    memcpy(initial.data() + 12 * (size_t)i, graph + sizeof(gh) + 192 * (size_t)i, 96);
    memcpy(result.data() + 12 * (size_t)i, graph + sizeof(gh) + 192 * (size_t)i + 96, 96);
  }
  PG_TRY(c, L->graph, posegraph_install_nodes(L->graph, initial.data(), result.data(), gh.n_nodes, false));
  const char* ep = graph + sizeof(gh) + 192 * (size_t)gh.n_nodes;
  for (uint32_t e = 0; e < gh.n_edges; ++e) { /* through the graph's own entry, in insertion order */
    ckpt::Edge o;
    memcpy(&o, ep + sizeof(o) * (size_t)e, sizeof(o));
    double Z[16];
    rigid12_to_mat4(o.Z, Z);
    PG_TRY(c, L->graph, suma_posegraph_add_edge(L->graph, o.from, o.to, Z, o.information));
  }
  const char* tp = loop + sizeof(h) + sizeof(suma_loop_params);
  L->trajectory_distances.resize(h.n_traj);
  if (h.n_traj) memcpy(L->trajectory_distances.data(), tp, 4 * (size_t)h.n_traj);
  const char* cp = tp + ((4 * (size_t)h.n_traj + 7) & ~(size_t)7);
  L->unverified.clear(), L->verified.clear();
  for (uint32_t k = 0; k < h.n_unverified + h.n_verified; ++k) {
    ckpt::Candidate q;
    memcpy(&q, cp + sizeof(q) * (size_t)k, sizeof(q));
    LoopCandidate cand;
    cand.from = q.from, cand.to = q.to;
    memcpy(cand.rel_pose, q.rel_pose, sizeof(cand.rel_pose));
    (k < h.n_unverified ? L->unverified : L->verified).push_back(cand);
  }
  L->already_verified = h.already_verified != 0;
  L->loop_count = h.loop_count, L->time_without = h.time_without;
  L->found = h.found != 0, L->use = h.use != 0, L->started = h.started != 0, L->integrated = h.integrated != 0;
  L->candidate_to = h.candidate_to, L->edges_added = h.edges_added;
  L->result_old.outlier_ratio = h.result_old_outlier_ratio;
  L->loop_valid_ratio = h.loop_valid_ratio, L->loop_outlier_ratio = h.loop_outlier_ratio;
  L->loop_relative_error_all = h.loop_relative_error_all;
  L->result_old.inlier = h.result_old_inlier, L->result_old.outlier = h.result_old_outlier;
  L->result_old.valid = h.result_old_valid, L->result_old.invalid = h.result_old_invalid;
  L->result_old.error = h.result_old_error, L->result_old.residual = h.result_old_residual;
  L->result_old.inlier_residual = h.result_old_inlier_residual;
  L->posegraph_error = h.posegraph_error;
  L->checked = false;
  if (opt) {
    /* the clone as the worker left it: only its poses are read by the integration (host record and device buffer) */
    ckpt::OptHead oh;
    memcpy(&oh, opt, sizeof(oh));
    std::vector<double> X(12 * (size_t)oh.n_opt);
    memcpy(X.data(), opt + sizeof(oh), X.size() * sizeof(double));
    int rc = suma_posegraph_create(c->device, oh.n_opt, 1, &L->opt_graph);
    if (rc != SUMA_OK) return fail(c, rc, std::string("suma_posegraph_create: ") + suma_posegraph_last_error(nullptr));
    /* loop_ckpt_check has seen that an accepted record (worker_rc) is finite; a refused one is never read */
    if (oh.worker_rc == SUMA_OK)
      PG_TRY(c, L->opt_graph, posegraph_install_nodes(L->opt_graph, X.data(), X.data(), oh.n_opt, true));
    L->optimizing = true;
    L->before_id = oh.before_id, L->before_loop_count = oh.before_loop_count, L->started_at = oh.started_at;
    memcpy(L->before_pose, oh.before_pose, sizeof(L->before_pose));
    L->worker_rc = oh.worker_rc;
    L->worker_done.store(1, std::memory_order_release);
  }
  return SUMA_OK;
}
