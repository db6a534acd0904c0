/*
 * suma_adapter.hpp -- C++ adapter that keeps the reference's class interfaces (src/core) and forwards to
 * the C-ABI of include/suma_hip.h.  A maintainer of PRBonn/semantic_suma compiles this in place of
 * the method bodies of Preprocessing.cpp / Frame2Model.cpp / LieGaussNewton.cpp / SurfelMap.cpp; the
 * caller (SurfelMapping.cpp) and everything above it stay untouched.  Header-only, C++11, no Eigen /
 * glow dependency: matrices cross as column-major pointers (Eigen::Matrix4f::data() is exactly that).
 *
 * Error behaviour mirrors the reference: failures throw std::runtime_error (Frame2Model.cpp:132,
 * Objective.h:31, SurfelMapping.cpp:98).
 */
#ifndef SUMA_ADAPTER_HPP_
#define SUMA_ADAPTER_HPP_

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "suma_hip.h"

namespace suma_hip {

inline void check(suma_ctx* c, int rc, const char* what) {
  if (rc != SUMA_OK) throw std::runtime_error(std::string(what) + ": " + suma_last_error(c));
}

/* one per GPU; shared by the adapter objects below (the reference shares one GL context the same way) */
class Context {
 public:
  explicit Context(const suma_params& p, int device = 0) : params_(p) {
    if (suma_ctx_create(&p, device, &c_) != SUMA_OK)
      throw std::runtime_error(std::string("suma_ctx_create: ") + suma_last_error(nullptr));
  }
  ~Context() { suma_ctx_destroy(c_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  suma_ctx* get() const { return c_; }
  const suma_params& params() const { return params_; }
  void setParameters(const suma_params& p) {  /* every class' setParameters(const rv::ParameterList&) */
    check(c_, suma_set_params(c_, &p), "suma_set_params");
    params_ = p;
  }

 private:
  suma_ctx* c_{nullptr};
  suma_params params_;
};

/* src/core/Frame.h:21-79 */
class Frame {
 public:
  Frame(Context& ctx, uint32_t w, uint32_t h) : ctx_(ctx), owned_(true) {
    check(ctx.get(), suma_frame_create(ctx.get(), w, h, &f_), "suma_frame_create");
  }
  Frame(Context& ctx, suma_frame* borrowed) : ctx_(ctx), f_(borrowed), owned_(false) {}
  ~Frame() {
    if (owned_) suma_frame_destroy(f_);
  }
  void copy(const Frame& other) { check(ctx_.get(), suma_frame_copy(ctx_.get(), f_, other.f_), "Frame::copy"); }
  void download(int which, std::vector<suma_float4>& out) const {
    out.resize((size_t)suma_frame_width(f_) * suma_frame_height(f_));
    check(ctx_.get(), suma_frame_download(ctx_.get(), f_, which, out.data()), "suma_frame_download");
  }
  suma_frame* get() const { return f_; }
  float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; /* Frame::pose, Frame.h:74 */
  bool valid{false};

 private:
  Context& ctx_;
  suma_frame* f_{nullptr};
  bool owned_;
};

/* src/core/Preprocessing.h:47-58 */
class Preprocessing {
 public:
  explicit Preprocessing(Context& ctx) : ctx_(ctx) {}
  /* reference: process(GlBuffer<rv::Point3f>& points, Frame&, GlBuffer<float>& labels, GlBuffer<float>& probs, t) */
  void process(const suma_float4* points, uint32_t n, Frame& frame, const float* labels, const float* probs,
               uint32_t timestamp) {
    check(ctx_.get(), suma_preprocess(ctx_.get(), points, labels, probs, n, timestamp, frame.get()),
          "Preprocessing::process");
    frame.valid = true;
  }

 private:
  Context& ctx_;
};

/* SE3::exp (src/core/lie_algebra.cpp:4-34) for Objective::increment on the host side of the adapter; column-major */
inline void se3_exp(const double* x, double* T) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  const double v[3] = {x[0], x[1], x[2]}, o[3] = {x[3], x[4], x[5]};
  const double theta = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
  if (theta > 1e-10) {
    const double K[9] = {0, -o[2], o[1], o[2], 0, -o[0], -o[1], o[0], 0}; /* row-major skew matrix */
    double K2[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
    const double alpha = std::sin(theta) / theta, beta = (1 - std::cos(theta)) / (theta * theta);
    const double delta = (theta - std::sin(theta)) / (theta * theta * theta);
    for (int r = 0; r < 3; ++r) {
      double t = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double I = (r == c) ? 1.0 : 0.0;
        T[4 * c + r] = I + alpha * K[3 * r + c] + beta * K2[3 * r + c];
        t += (I + beta * K[3 * r + c] + delta * K2[3 * r + c]) * v[c];
      }
      T[12 + r] = t;
    }
  } else {
    T[12] = v[0];
    T[13] = v[1];
    T[14] = v[2];
  }
}

/* src/core/Objective.h:14-82 as implemented by src/core/Frame2Model.h:28-73.
 * Like the reference's object, an instance OWNS its parameters (Frame2Model::updateParameters,
 * Frame2Model.cpp:65-110) and its frame pair and sends both to the device before every launch: objective_ and
 * recovery_ = Frame2Model(fallback_params) (SurfelMapping.cpp:87-94, used at :438-449) can share one Context. */
class Frame2Model {
 public:
  explicit Frame2Model(Context& ctx) : Frame2Model(ctx, ctx.params()) {}
  /* Frame2Model(const rv::ParameterList&): the parameter block this objective is built from */
  Frame2Model(Context& ctx, const suma_params& p) : ctx_(ctx) {
    std::memset(&stats_, 0, sizeof(stats_));
    eye(pose_);
    objective_.icp_max_distance = p.icp_max_distance;
    objective_.icp_max_angle = p.icp_max_angle;
    objective_.weight_function = p.weight_function;
    objective_.factor = p.factor;
    objective_.bilinear_sampling = p.bilinear_sampling;
  }
  uint32_t num_parameters() const { return 6; }
  /* Objective::setParameter(const rv::Parameter&) -> Frame2Model::setParameter (Frame2Model.cpp:112-115): the keys
   * this objective reads; "weighting" takes huber / turkey / stability / anything else = none */
  void setParameter(const std::string& name, double value) {
    if (name == "icp-max-distance") objective_.icp_max_distance = (float)value;
    else if (name == "icp-max-angle") objective_.icp_max_angle = (float)value;
    else if (name == "factor") objective_.factor = (float)value;
    else if (name == "bilinear_sampling") objective_.bilinear_sampling = value != 0.0;
  }
  void setParameter(const std::string& name, const std::string& value) {
    if (name != "weighting") return;
    objective_.weight_function = value == "huber" ? SUMA_WEIGHT_HUBER
                               : value == "turkey" ? SUMA_WEIGHT_TUKEY
                               : value == "stability" ? SUMA_WEIGHT_STABILITY : SUMA_WEIGHT_NONE;
  }
  void setData(const std::shared_ptr<Frame>& current, const std::shared_ptr<Frame>& last) {
    current_ = current;
    last_ = last;
    iteration_ = 0;
  }
  /* Objective::initialize (Objective.h:58) sets the pose and nothing else: iteration_ is reset by setData only */
  void initialize(const double* pose16) { std::memcpy(pose_, pose16, sizeof(pose_)); }
  /* Objective::residual is "not implemented" in the reference too (Frame2Model.cpp:131-134) */
  double residual(const double* /*delta6*/) { throw std::runtime_error("not implemented."); }
  /* returns F; JtJ 6x6 column-major, Jtf 6 (Eigen::MatrixXd::data() of the reference's arguments) */
  double jacobianProducts(double* JtJ, double* Jtf) {
    bind();
    check(ctx_.get(), suma_icp_jacobian_products(ctx_.get(), pose_, iteration_, JtJ, Jtf, nullptr, &stats_),
          "Frame2Model::jacobianProducts");
    return stats_.error;
  }
  /* Objective::increment (Objective.h:45-48): pose_ = SE3::exp(delta) * pose_ */
  void increment(const double* delta6) {
    double E[16], P[16];
    se3_exp(delta6, E);
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r)
        P[4 * c + r] = E[r] * pose_[4 * c] + E[4 + r] * pose_[4 * c + 1] + E[8 + r] * pose_[4 * c + 2] + E[12 + r] * pose_[4 * c + 3];
    std::memcpy(pose_, P, sizeof(P));
    iteration_ += 1;
  }
  const double* pose() const { return pose_; }
  uint32_t inlier() const { return stats_.inlier; }
  uint32_t outlier() const { return stats_.outlier; }
  uint32_t valid() const { return stats_.valid; }
  uint32_t invalid() const { return stats_.invalid; }
  double inlier_residual() const { return stats_.inlier_residual; }
  void setLevel(uint32_t) {}                 /* Frame2Model.cpp:125 */
  uint32_t getMaxLevel() const { return 0; } /* Frame2Model.cpp:127-129 */
  void reset() {}

 private:
  friend class LieGaussNewton;
  static void eye(double* T) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0; }
  /* this object's frames and parameters become the ones the next launch uses */
  void bind() {
    if (!current_ || !last_) throw std::runtime_error("Frame2Model::setData has not been called");
    check(ctx_.get(), suma_icp_set_data(ctx_.get(), current_->get(), last_->get()), "Frame2Model::setData");
    check(ctx_.get(), suma_icp_set_objective(ctx_.get(), &objective_), "Frame2Model parameters");
  }
  Context& ctx_;
  std::shared_ptr<Frame> current_, last_;
  suma_icp_objective objective_;
  double pose_[16];
  uint32_t iteration_{0};
  suma_icp_stats stats_;
};

/* src/core/LieGaussNewton.h:25-76: the whole loop runs on the device */
class LieGaussNewton {
 public:
  static const int32_t CONVERGED = 0;
  explicit LieGaussNewton(Context& ctx) : ctx_(ctx) { std::memset(&stats_, 0, sizeof(stats_)); }
  int32_t minimize(Frame2Model& F, const double* T0) {
    F.bind();
    /* Frame2Model::iteration_ runs on across minimisations on one setData (SurfelMapping.cpp:693-700) */
    check(ctx_.get(), suma_icp_set_iteration(ctx_.get(), F.iteration_), "Frame2Model::iteration_");
    /* the pose history stays on the device until history() is called (the reference's caller only draws it,
     * SurfelMapping.cpp:391): the minimisation costs the host one poll of a pinned record, no copy */
    check(ctx_.get(), suma_icp_minimize(ctx_.get(), T0, pose_, nullptr, 0, &n_hist_, &stats_), "LieGaussNewton::minimize");
    history_valid_ = false;
    history_seq_ = suma_icp_history_sequence(ctx_.get());
    std::memcpy(F.pose_, pose_, sizeof(pose_));
    F.stats_ = stats_;
    F.iteration_ += stats_.iterations + (stats_.converged ? 1u : 0u); /* one Objective::increment per step, Objective.h:45-48 */
    check(ctx_.get(), suma_icp_information(ctx_.get(), information_), "LieGaussNewton::information");
    return 0; /* the reference returns 0 from every path of minimize (LieGaussNewton.cpp:37) */
  }
  const double* pose() const { return pose_; }
  double residual() const { return stats_.error; }
  /* LieGaussNewton::reason (LieGaussNewton.cpp:110-115), called by SurfelMapping.cpp:428,448 */
  std::string reason(int32_t errorno) const {
    if (errorno == -1) return "Maximum number of iterations reached.";
    if (errorno == -2) return "Diverging.";
    return "no error";
  }
  /* information(): J^T W J of the last step, 6x6 column-major (LieGaussNewton.cpp:75,103-105) */
  const double* information() const { return information_; }
  /* 16 doubles per entry; fetched from the device on first use after a minimisation */
  const std::vector<double>& history() {
    if (!history_valid_) {
      /* one history buffer per context: another optimizer object (or a loop-closure verification) that has minimised
       * since would be read here instead of this object's chain */
      if (suma_icp_history_sequence(ctx_.get()) != history_seq_)
        throw std::runtime_error("LieGaussNewton::history: a later minimisation on this context has overwritten the "
                                 "device-side history; call history() before it");
      const uint32_t n = n_hist_ < 1025 ? n_hist_ : 1025;
      history_.assign(16 * (size_t)n, 0.0);
      if (n) check(ctx_.get(), suma_icp_history(ctx_.get(), history_.data(), n, nullptr), "LieGaussNewton::history");
      history_valid_ = true;
    }
    return history_;
  }
  uint32_t iterationCount() const { return stats_.iterations; }

 private:
  Context& ctx_;
  double pose_[16];
  double information_[36];
  std::vector<double> history_;
  uint32_t n_hist_{0};
  bool history_valid_{true};
  uint64_t history_seq_{0};
  suma_icp_stats stats_;
};

/* The 2.5-D semantic traversability grid of n world-frame records on the device (suma_world_grid; what exportWorld
 * writes, or a caller's records after suma_device_upload): gp.width * gp.height cells, row-major, row = y, computed on
 * the device and returned on the host.  fit_margin >= 0: the raster is first fitted to the records with that many empty
 * cells around them (suma_world_grid_fit), and gp receives it. */
inline std::vector<suma_grid_cell> worldGrid(Context& ctx, suma_grid_params& gp, const suma_world_surfel* d_records, uint32_t n,
                                             int fit_margin = -1, suma_grid_stats* stats = nullptr) {
  if (fit_margin >= 0) check(ctx.get(), suma_world_grid_fit(ctx.get(), d_records, n, (uint32_t)fit_margin, &gp), "worldGrid");
  std::vector<suma_grid_cell> out((size_t)gp.width * gp.height);
  suma_grid_stats st;
  void* d = nullptr;
  check(ctx.get(), suma_device_alloc(ctx.get(), (uint64_t)(out.size() ? out.size() : 1) * sizeof(suma_grid_cell), &d), "worldGrid");
  int rc = suma_world_grid(ctx.get(), &gp, d_records, n, (suma_grid_cell*)d, &st);
  if (rc == SUMA_OK) rc = suma_device_download(ctx.get(), out.data(), d, (uint64_t)out.size() * sizeof(suma_grid_cell));
  suma_device_free(ctx.get(), d);
  check(ctx.get(), rc, "worldGrid");
  if (stats) *stats = st;
  return out;
}

/* Planning on a traversability grid (suma_grid_plan_field): clearance, traversability and the cost-to-go to `goals` (cell
 * indices; suma_grid_cell_index makes one of a world position) of the gp.width * gp.height cells in `cells`, computed on
 * the device and returned on the host, row-major like the grid. */
inline std::vector<suma_plan_cell> planField(Context& ctx, const suma_grid_params& gp, const suma_plan_params& pp,
                                             const std::vector<suma_grid_cell>& cells, const std::vector<int64_t>& goals,
                                             suma_plan_stats* stats = nullptr) {
  if (cells.size() != (size_t)gp.width * gp.height) throw std::runtime_error("planField: cells do not match the raster");
  std::vector<suma_plan_cell> out(cells.size());
  suma_plan_stats st;
  void *d_cells = nullptr, *d_field = nullptr;
  const uint64_t cell_bytes = (uint64_t)(cells.size() ? cells.size() : 1) * sizeof(suma_grid_cell);
  check(ctx.get(), suma_device_alloc(ctx.get(), cell_bytes, &d_cells), "planField");
  int rc = suma_device_alloc(ctx.get(), (uint64_t)(out.size() ? out.size() : 1) * sizeof(suma_plan_cell), &d_field);
  if (rc == SUMA_OK) rc = suma_device_upload(ctx.get(), d_cells, cells.data(), (uint64_t)cells.size() * sizeof(suma_grid_cell));
  if (rc == SUMA_OK)
    rc = suma_grid_plan_field(ctx.get(), &gp, &pp, (const suma_grid_cell*)d_cells, goals.data(), (uint32_t)goals.size(),
                              (suma_plan_cell*)d_field, &st);
  if (rc == SUMA_OK) rc = suma_device_download(ctx.get(), out.data(), d_field, (uint64_t)out.size() * sizeof(suma_plan_cell));
  if (d_field) suma_device_free(ctx.get(), d_field);
  suma_device_free(ctx.get(), d_cells);
  check(ctx.get(), rc, "planField");
  if (stats) *stats = st;
  return out;
}

/* The paths from `starts` (cell indices; negative or beyond the raster: SUMA_PATH_START_OUTSIDE) down a field of planField
 * (suma_grid_plan_paths): one result per start, and in path_cells one row of path_capacity cell indices per start, the
 * start first, 0xffffffff behind the path's end. */
inline std::vector<suma_plan_path> planPaths(Context& ctx, const suma_grid_params& gp, const std::vector<suma_plan_cell>& field,
                                             const std::vector<int64_t>& starts, uint32_t path_capacity,
                                             std::vector<uint32_t>& path_cells) {
  if (field.size() != (size_t)gp.width * gp.height) throw std::runtime_error("planPaths: the field does not match the raster");
  std::vector<suma_plan_path> out(starts.size());
  path_cells.assign(starts.size() * (size_t)path_capacity, 0xffffffffu);
  void* d_field = nullptr;
  check(ctx.get(), suma_device_alloc(ctx.get(), (uint64_t)(field.size() ? field.size() : 1) * sizeof(suma_plan_cell), &d_field),
        "planPaths");
  int rc = suma_device_upload(ctx.get(), d_field, field.data(), (uint64_t)field.size() * sizeof(suma_plan_cell));
  if (rc == SUMA_OK)
    rc = suma_grid_plan_paths(ctx.get(), &gp, (const suma_plan_cell*)d_field, starts.data(), (uint32_t)starts.size(), path_capacity,
                              path_cells.data(), out.data());
  suma_device_free(ctx.get(), d_field);
  check(ctx.get(), rc, "planPaths");
  return out;
}

/* src/core/SurfelMap.h:36-78 (draw / setColorMap are visualisation and stay with the GL code) */
class SurfelMap {
 public:
  explicit SurfelMap(Context& ctx) : ctx_(ctx) {}
  void reset() { check(ctx_.get(), suma_map_reset(ctx_.get()), "SurfelMap::reset"); }
  void update(const float* pose, Frame& frame) {
    check(ctx_.get(), suma_map_update(ctx_.get(), pose, frame.get()), "SurfelMap::update");
  }
  void render(const float* pose, Frame& frame, float ct) { render(pose, pose, frame, ct); }
  void render(const float* pose_old, const float* pose_new, Frame& frame, float ct) {
    check(ctx_.get(), suma_map_render(ctx_.get(), pose_old, pose_new, ct, frame.get()), "SurfelMap::render");
  }
  void render_active(const float* pose, float ct) {
    check(ctx_.get(), suma_map_render_active(ctx_.get(), pose, ct), "SurfelMap::render_active");
  }
  void render_inactive(const float* pose, float ct) {
    check(ctx_.get(), suma_map_render_inactive(ctx_.get(), pose, ct), "SurfelMap::render_inactive");
  }
  void render_composed(const float* pose_old, const float* pose_new, float ct) {
    check(ctx_.get(), suma_map_render_composed(ctx_.get(), pose_old, pose_new, ct), "SurfelMap::render_composed");
  }
  std::shared_ptr<Frame> oldMapFrame() { return borrowed(SUMA_FRAME_OLD); }
  std::shared_ptr<Frame> newMapFrame() { return borrowed(SUMA_FRAME_NEW); }
  std::shared_ptr<Frame> composedFrame() { return borrowed(SUMA_FRAME_COMPOSED); }
  void updatePoses(const std::vector<float>& poses16) {
    check(ctx_.get(), suma_map_update_poses(ctx_.get(), poses16.data(), (uint32_t)(poses16.size() / 16)),
          "SurfelMap::updatePoses");
  }
  uint32_t size() const {
    uint32_t n = 0;
    check(ctx_.get(), suma_map_size(ctx_.get(), &n), "SurfelMap::size");
    return n;
  }
  /* getModelSurfels() / getDataSurfels() (SurfelMap.h:64-67) return glow::GlBuffer handles in the reference; here the
   * device buffer of the active map (64-byte records, valid until the next update), for hipGraphicsGLRegisterBuffer
   * or a device-to-device copy into the viewer's VBO.  The data surfels are the tail [first, first + n). */
  struct DeviceSurfels {
    const suma_surfel* d_ptr;
    uint32_t first, n;
  };
  DeviceSurfels getModelSurfels() {
    void* p = nullptr;
    uint32_t n = 0;
    check(ctx_.get(), suma_map_export_surfels(ctx_.get(), &p, &n), "SurfelMap::getModelSurfels");
    return DeviceSurfels{(const suma_surfel*)p, 0, n};
  }
  DeviceSurfels getDataSurfels() {
    void* p = nullptr;
    uint32_t first = 0, n = 0;
    check(ctx_.get(), suma_map_export_data_surfels(ctx_.get(), &p, &first, &n), "SurfelMap::getDataSurfels");
    return DeviceSurfels{(const suma_surfel*)p, first, n};
  }
  std::vector<suma_surfel> getAllSurfels() {
    std::vector<suma_surfel> out(size());
    uint32_t n = 0;
    check(ctx_.get(), suma_map_download(ctx_.get(), out.data(), (uint32_t)out.size(), &n), "SurfelMap::getAllSurfels");
    return out;
  }
  /* the (i, j) of every parked submap tile that holds records, ascending by (i, then j) */
  std::vector<std::pair<int32_t, int32_t>> cachedTiles() {
    uint32_t n = 0;
    check(ctx_.get(), suma_map_cached_tiles(ctx_.get(), nullptr, 0, &n), "SurfelMap::cachedTiles");
    std::vector<int32_t> ij(2 * (size_t)n);
    if (n) check(ctx_.get(), suma_map_cached_tiles(ctx_.get(), ij.data(), n, &n), "SurfelMap::cachedTiles");
    std::vector<std::pair<int32_t, int32_t>> out;
    for (uint32_t k = 0; k < n && 2 * (size_t)k + 1 < ij.size(); ++k) out.emplace_back(ij[2 * k], ij[2 * k + 1]);
    return out;
  }
  /* the whole map (active surfels and every parked tile) in the world frame, filtered and optionally fused to voxels
   * (suma_map_export_world); computed on the device, returned on the host */
  std::vector<suma_world_surfel> exportWorld(const suma_world_params& wp, suma_world_stats* stats = nullptr) {
    /* once into a buffer of a guessed size (what the last export needed, with headroom), again only if it was too small */
    suma_world_stats st;
    std::vector<suma_world_surfel> out;
    uint32_t cap = world_capacity_ > 65536u ? world_capacity_ : 65536u;
    for (int attempt = 0; attempt < 2; ++attempt) {
      void* d = nullptr;
      check(ctx_.get(), suma_device_alloc(ctx_.get(), (uint64_t)cap * sizeof(suma_world_surfel), &d), "SurfelMap::exportWorld");
      int rc = suma_map_export_world(ctx_.get(), &wp, (suma_world_surfel*)d, cap, &st);
      const bool fits = rc == SUMA_OK && st.n_out <= cap;
      if (fits) {
        out.resize(st.n_out);
        if (st.n_out) rc = suma_device_download(ctx_.get(), out.data(), d, (uint64_t)st.n_out * sizeof(suma_world_surfel));
      }
      suma_device_free(ctx_.get(), d);
      check(ctx_.get(), rc, "SurfelMap::exportWorld");
      if (fits) break;
      if (attempt) throw std::runtime_error("SurfelMap::exportWorld: the map changed between two exports");
      cap = st.n_out;
    }
    world_capacity_ = st.n_out + st.n_out / 4;
    if (stats) *stats = st;
    return out;
  }
  /* the traversability grid of the whole map (worldGrid above): the flat world export wp selects goes into a device
   * buffer and is gridded there, so the records never visit the host */
  std::vector<suma_grid_cell> exportGrid(suma_grid_params& gp, const suma_world_params& wp, int fit_margin = -1,
                                         suma_grid_stats* stats = nullptr) {
    if (wp.voxel_size != 0.0f) throw std::runtime_error("SurfelMap::exportGrid: the grid takes the flat export (voxel_size 0)");
    suma_world_stats st, st2;
    check(ctx_.get(), suma_map_export_world(ctx_.get(), &wp, nullptr, 0, &st), "SurfelMap::exportGrid"); /* the size */
    void* d = nullptr;
    check(ctx_.get(), suma_device_alloc(ctx_.get(), (uint64_t)(st.n_out ? st.n_out : 1) * sizeof(suma_world_surfel), &d),
          "SurfelMap::exportGrid");
    std::vector<suma_grid_cell> out;
    try {
      check(ctx_.get(), suma_map_export_world(ctx_.get(), &wp, (suma_world_surfel*)d, st.n_out, &st2), "SurfelMap::exportGrid");
      if (st2.n_out != st.n_out) throw std::runtime_error("SurfelMap::exportGrid: the map changed between two exports");
      out = worldGrid(ctx_, gp, (const suma_world_surfel*)d, st.n_out, fit_margin, stats);
    } catch (...) {
      suma_device_free(ctx_.get(), d);
      throw;
    }
    suma_device_free(ctx_.get(), d);
    return out;
  }

 private:
  std::shared_ptr<Frame> borrowed(int which) {
    return std::make_shared<Frame>(ctx_, suma_map_frame(ctx_.get(), which));
  }
  Context& ctx_;
  uint32_t world_capacity_ = 0; /* exportWorld's next buffer size, in records */
};

/* src/core/SurfelMapping.h: the per-scan sequencing (SurfelMapping.cpp:175-210) on the scan pipeline of the library --
 * K1-K3 on a side stream, the Gauss-Newton chain resident on the device, K7 / K8 fused into the passes around them,
 * renders de-duplicated.  processScan keeps the reference's shape: integrateLoopClosures and checkLoopClosure stay the
 * maintainer's functions (pose graph, candidate search, gtsam: untouched) and call the hooks below for their device
 * parts.  Poses cross as column-major double[16] (Eigen::Matrix4d::data()). */
class SurfelMapping {
 public:
  explicit SurfelMapping(const suma_params& p, int device = 0) {
    if (suma_pipeline_create(&p, device, &s_) != SUMA_OK)
      throw std::runtime_error(std::string("suma_pipeline_create: ") + suma_last_error(nullptr));
  }
  ~SurfelMapping() { suma_pipeline_destroy(s_); }
  SurfelMapping(const SurfelMapping&) = delete;
  SurfelMapping& operator=(const SurfelMapping&) = delete;

  /* processScan(const rv::Laserscan&), SurfelMapping.cpp:175-210.  The two std::function hooks are where the
   * reference calls integrateLoopClosures() (:179) and checkLoopClosure() (:196); leave them empty for
   * close-loops = false.  fixed_iterations = 0: the stopping tests of LieGaussNewton decide. */
  template <class Before, class Between>
  void processScan(const suma_float4* points, const float* labels, const float* probs, uint32_t n, Before integrate,
                   Between check_loop_closure, int32_t fixed_iterations = 0) {
    const double t_all = now();
    integrate(*this);                                                                            /* :179 */
    double t = now();
    chk(suma_pipeline_begin_scan(s_, points, labels, probs, n), "SurfelMapping::initialize/preprocess"); /* :181-187 */
    statistics_["initialize-time"] = 0.0; /* the frame swaps of initialize() (:323-331) are pointer swaps inside begin_scan */
    statistics_["preprocessing-time"] = now() - t;                                              /* :187 */
    const bool tracked = timestamp() > 0;
    t = now();
    chk(suma_pipeline_update_pose(s_, fixed_iterations), "SurfelMapping::updatePose");          /* :192 */
    if (tracked) {
      const double dt = now() - t;
      statistics_["icp-time"] = dt;                                                             /* :193 (and :425) */
      statistics_["opt-time"] = dt;                                                             /* :393 */
      statistics_["icp-overall"] = dt;                                                          /* :475 */
      suma_icp_stats st;
      std::memset(&st, 0, sizeof(st));
      suma_pipeline_minimize_stats(s_, &st);
      statistics_["num_iterations"] = (double)st.iterations;                                    /* :394 */
      t = now();
      check_loop_closure(*this);                                                                /* :196 */
      statistics_["loop-time"] = now() - t;                                                     /* :197 */
    }
    t = now();
    chk(suma_pipeline_update_map(s_), "SurfelMapping::updateMap");                               /* :201, :209 */
    const double dt_map = now() - t;
    statistics_["map-update"] = dt_map;                                                          /* :800 */
    statistics_["mapping-time"] = dt_map;                                                        /* :202 */
    const double complete = now() - t_all;
    statistics_["complete-time"] = complete;                                                     /* :206 */
    statistics_["icp_percentage"] = complete > 0.0 ? statistics_["opt-time"] / complete : 0.0;  /* :207 */
  }
  void processScan(const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                   int32_t fixed_iterations = 0) {
    auto nop = [](SurfelMapping&) {};
    processScan(points, labels, probs, n, nop, nop, fixed_iterations);
  }
  /* SurfelMapping::Stats (SurfelMapping.h; filled at SurfelMapping.cpp:183-207, 393-394, 425, 475, 800): the keys the
   * untouched GUI plots (VisualizerWindow.cpp:705), in seconds like rv::Stopwatch::toc().  They are HOST clocks around
   * the phase calls, as the reference's are around its GL calls -- with one difference in meaning: the reference
   * drains the GL pipeline inside every phase (glFinish), this library only waits where the host needs a result (the
   * minimisation), so "mapping-time" is the time to ENQUEUE the update and the post-update rendering, whose GPU work
   * overlaps the next scan's upload.  Per-kernel GPU times: gpuTimes(). */
  const std::map<std::string, double>& getStatistics() const { return statistics_; }
  /* GPU time per kernel group from suma_profile_get (ms summed since the last reset; needs suma_profile_enable(ctx, 1),
   * which costs a few percent of throughput) */
  std::map<std::string, double> gpuTimes() {
    std::map<std::string, double> out;
    suma_kernel_time kt[64];
    const int n = suma_profile_get(ctx(), kt, 64);
    for (int i = 0; i < n && i < 64; ++i) out[kt[i].name] = kt[i].total_ms;
    return out;
  }
  /* SurfelMapping::reset(), SurfelMapping.cpp:131-169 */
  void reset() { chk(suma_pipeline_reset(s_), "SurfelMapping::reset"); }
  /* ---- checkpoint / resume (suma_pipeline_checkpoint_save / _load): nothing in the reference to mirror -- its
   *      Posegraph::save / load are empty (Posegraph.cpp:118-119) and its tile cache cannot be written out.  Between
   *      two processScan calls only.  The file is written under a temporary name and renamed, so `path` never holds
   *      half an image; loadCheckpoint needs a SurfelMapping made with the parameters the image was saved with
   *      (suma_checkpoint_params reads them from an image) and leaves it untouched when the image is refused. ---- */
  void saveCheckpoint(const std::string& path) {
    uint64_t need = 0, written = 0;
    chk(suma_pipeline_checkpoint_size(s_, &need), "SurfelMapping::saveCheckpoint");
    std::vector<char> image((size_t)need);
    chk(suma_pipeline_checkpoint_save(s_, image.data(), image.size(), &written), "SurfelMapping::saveCheckpoint");
    const std::string tmp = path + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) throw std::runtime_error("SurfelMapping::saveCheckpoint: cannot write " + tmp);
    const bool ok = std::fwrite(image.data(), 1, (size_t)written, f) == (size_t)written;
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) {
      std::remove(tmp.c_str());
      throw std::runtime_error("SurfelMapping::saveCheckpoint: cannot write " + path);
    }
  }
  void loadCheckpoint(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("SurfelMapping::loadCheckpoint: cannot read " + path);
    std::vector<char> image;
    char block[65536];
    for (size_t n; (n = std::fread(block, 1, sizeof(block), f)) > 0;) image.insert(image.end(), block, block + n);
    const bool ok = std::ferror(f) == 0;
    std::fclose(f);
    if (!ok) throw std::runtime_error("SurfelMapping::loadCheckpoint: cannot read " + path);
    chk(suma_pipeline_checkpoint_load(s_, image.data(), image.size()), "SurfelMapping::loadCheckpoint");
  }
  /* ---- motion compensation of raw sweeps (suma_pipeline_*deskew*, csrc/k_deskew.hip): nothing in the reference to
   *      mirror, its KITTI scans are compensated already.  While enabled, processScan corrects the points in front of
   *      the preprocessing with the last increment as the motion over one sweep; setDeskewMotion overrides it once
   *      (column-major double[16]: an IMU, wheel odometry, the first scans).  A checkpoint holds none of this: enable it
   *      again after loadCheckpoint. ---- */
  void enableDeskew(const suma_deskew_params* dp = nullptr) { chk(suma_pipeline_enable_deskew(s_, dp), "SurfelMapping::enableDeskew"); }
  void disableDeskew() { chk(suma_pipeline_disable_deskew(s_), "SurfelMapping::disableDeskew"); }
  void setDeskewMotion(const double* motion16) { chk(suma_pipeline_set_deskew_motion(s_, motion16), "SurfelMapping::setDeskewMotion"); }
  /* what the last corrected scan used; returns its source (SUMA_DESKEW_MOTION_*) */
  int32_t deskewMotion(double* motion16) const {
    int32_t source = SUMA_DESKEW_MOTION_NONE;
    chk(suma_pipeline_deskew_motion(s_, motion16, &source), "SurfelMapping::deskewMotion");
    return source;
  }
  /* ---- device parts of checkLoopClosure ---- */
  /* :546-574, a tracked closure verified again; on success the caller sets currentPose_old_ = out.pose_old (:581) */
  suma_loop_track trackLoopClosure(double min_valid = 0.2, double max_outlier = 0.85, double max_diff = 0.1) {
    suma_loop_track t;
    chk(suma_pipeline_track_loop_closure(s_, min_valid, max_outlier, max_diff, &t), "checkLoopClosure (tracking)");
    return t;
  }
  /* :679-757, a candidate verified from n_init initial guesses (16 doubles each) */
  std::vector<suma_loop_result> verifyLoopClosure(const double* pose_prior, const double* initializations,
                                                  uint32_t n_init, float min_valid = 0.2f, float max_outlier = 0.85f) {
    std::vector<suma_loop_result> out(n_init);
    chk(suma_pipeline_verify_loop_closure(s_, pose_prior, initializations, n_init, min_valid, max_outlier, out.data()),
        "checkLoopClosure (candidates)");
    return out;
  }
  void setCurrentPoseOld(const double* pose_old) { chk(suma_pipeline_set_pose_old(s_, pose_old), "currentPose_old_"); }
  /* ---- integrateLoopClosures, :211-250: casted_poses (16 floats each), difference ---- */
  void integrateLoopClosures(const std::vector<float>& casted_poses, const double* difference) {
    chk(suma_pipeline_integrate_loop_closures(s_, casted_poses.data(), (uint32_t)(casted_poses.size() / 16), difference),
        "SurfelMapping::integrateLoopClosures");
  }
  /* which: 0 currentPose_, 1 currentPose_old_, 2 currentPose_new_, 3 lastPose_old_, 4 lastPose_ */
  void getPose(int which, double* pose16) const { suma_pipeline_get_pose(s_, which, pose16); }
  void getCurrentPose(double* pose16) const { suma_pipeline_pose(s_, pose16); }
  suma_icp_stats resultNew() {
    suma_icp_stats st;
    chk(suma_pipeline_result_new(s_, &st), "result_new_");
    return st;
  }
  uint32_t timestamp() const { return suma_pipeline_timestamp(s_); }
  uint32_t trackLoss() const { return suma_pipeline_track_loss(s_); }
  suma_pipeline* get() const { return s_; }
  suma_ctx* ctx() const { return suma_pipeline_ctx(s_); }

 private:
  void chk(int rc, const char* what) const { check(suma_pipeline_ctx(s_), rc, what); }
  static double now() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  suma_pipeline* s_{nullptr};
  std::map<std::string, double> statistics_;
};

/* Posegraph (src/core/Posegraph.h:10-78) on the device optimiser (suma_posegraph_*): the same method names and
 * meaning, Eigen::Matrix4d / Matrix6d replaced by column-major double* (Matrix::data()).  Not needed by SurfelMapping
 * and not provided: setMEstimator, save / load (empty in the reference, Posegraph.cpp:118-119), graph() / initial() /
 * result() (gtsam types). */
class Posegraph {
 public:
  typedef std::shared_ptr<Posegraph> Ptr;
  typedef std::shared_ptr<const Posegraph> ConstPtr;

  explicit Posegraph(int device = 0, uint32_t node_capacity = 1u << 17, uint32_t edge_capacity = 1u << 18) {
    if (suma_posegraph_create(device, node_capacity, edge_capacity, &g_) != SUMA_OK)
      throw std::runtime_error(std::string("suma_posegraph_create: ") + suma_posegraph_last_error(nullptr));
  }
  ~Posegraph() { suma_posegraph_destroy(g_); }
  Posegraph(const Posegraph&) = delete;
  Posegraph& operator=(const Posegraph&) = delete;

  Ptr clone() const {
    suma_posegraph* c = nullptr;
    check(suma_posegraph_clone(g_, &c), "Posegraph::clone");
    return Ptr(new Posegraph(c));
  }
  double error() const {
    double e = 0.0;
    check(suma_posegraph_error(g_, &e), "Posegraph::error");
    return e;
  }
  void clear() { check(suma_posegraph_clear(g_), "Posegraph::clear"); }
  void setInitial(int32_t id, const double* initial_estimate16) {
    check(suma_posegraph_set_initial(g_, id, initial_estimate16), "Posegraph::setInitial");
  }
  void addEdge(int32_t from, int32_t to, const double* measurement16, const double* information36) {
    check(suma_posegraph_add_edge(g_, from, to, measurement16, information36), "Posegraph::addEdge");
  }
  void pose(int32_t id, double* out16) const { check(suma_posegraph_pose(g_, id, out16), "Posegraph::pose"); }
  /* size() x 16 doubles, sorted by id */
  std::vector<double> poses() const {
    std::vector<double> out(16 * (size_t)size());
    uint32_t n = 0;
    check(suma_posegraph_poses(g_, out.data(), (uint32_t)size(), &n), "Posegraph::poses");
    return out;
  }
  int32_t size() const { return suma_posegraph_size(g_); }
  void reinitialize() { check(suma_posegraph_reinitialize(g_), "Posegraph::reinitialize"); }
  bool optimize(uint32_t num_iters) {
    check(suma_posegraph_optimize(g_, num_iters, nullptr, &stats_), "Posegraph::optimize");
    return true;
  }
  const suma_posegraph_stats& lastStats() const { return stats_; }
  suma_posegraph* handle() const { return g_; }

 private:
  explicit Posegraph(suma_posegraph* g) : g_(g) {}
  void check(int rc, const char* what) const {
    if (rc != SUMA_OK) throw std::runtime_error(std::string(what) + ": " + suma_posegraph_last_error(g_));
  }
  suma_posegraph* g_ = nullptr;
  suma_posegraph_stats stats_{};
};

/* Place recognition over the scans of a mapping session (suma_place_*, csrc/k_place.hip): addFrame after a scan
 * (suma_pipeline_frame(s, 0)), queryFrame / query for the k best places with a yaw, Localizer::relocalize to turn them
 * into a pose. */
class PlaceIndex {
 public:
  explicit PlaceIndex(const suma_place_params* pp = nullptr, int device = 0, uint32_t capacity = 0) {
    if (suma_place_index_create(pp, device, capacity, &i_) != SUMA_OK)
      throw std::runtime_error(std::string("suma_place_index_create: ") + suma_last_error(nullptr));
  }
  ~PlaceIndex() { suma_place_index_destroy(i_); }
  PlaceIndex(const PlaceIndex&) = delete;
  PlaceIndex& operator=(const PlaceIndex&) = delete;

  uint32_t size() const { return suma_place_index_size(i_); }
  void clear() { chk(suma_place_index_clear(i_), "PlaceIndex::clear"); }
  void addFrame(suma_ctx* ctx, const suma_frame* frame, uint32_t id) {
    chk(suma_place_index_add_frame(i_, ctx, frame, id), "PlaceIndex::addFrame");
  }
  /* cells n x sectors x rings (sector-major); the norms are made on the device */
  void upload(const std::vector<float>& cells, const std::vector<uint32_t>& ids) {
    chk(suma_place_index_upload(i_, cells.data(), ids.data(), (uint32_t)ids.size()), "PlaceIndex::upload");
  }
  void download(uint32_t first, uint32_t n, float* cells, float* norms, uint32_t* ids) {
    chk(suma_place_index_download(i_, first, n, cells, norms, ids), "PlaceIndex::download");
  }
  /* the k best (k <= SUMA_PLACE_MAX_MATCHES), leaving out ids in [exclude_lo, exclude_hi] (lo > hi: none) */
  std::vector<suma_place_match> queryFrame(suma_ctx* ctx, const suma_frame* frame, uint32_t k, uint32_t exclude_lo = 1,
                                           uint32_t exclude_hi = 0) {
    std::vector<suma_place_match> m(SUMA_PLACE_MAX_MATCHES);
    uint32_t n = 0;
    chk(suma_place_index_query_frame(i_, ctx, frame, exclude_lo, exclude_hi, k, m.data(), &n), "PlaceIndex::queryFrame");
    m.resize(n);
    return m;
  }
  std::vector<suma_place_match> query(const float* cells, uint32_t k, uint32_t exclude_lo = 1, uint32_t exclude_hi = 0) {
    std::vector<suma_place_match> m(SUMA_PLACE_MAX_MATCHES);
    uint32_t n = 0;
    chk(suma_place_index_query(i_, cells, exclude_lo, exclude_hi, k, m.data(), &n), "PlaceIndex::query");
    m.resize(n);
    return m;
  }
  suma_place_index* get() const { return i_; }

 private:
  void chk(int rc, const char* what) const {
    if (rc != SUMA_OK) throw std::runtime_error(std::string(what) + ": " + suma_place_index_last_error(i_));
  }
  suma_place_index* i_ = nullptr;
};

/* Localisation in a finished world map, which is left alone (suma_localizer_*, csrc/k_localize.hip): setMap bins the
 * records of SurfelMap::exportWorld / a map file into submap tiles on the device, setPose gives the start pose and
 * gathers the tiles around it (relocalize finds one from a PlaceIndex instead), processScan renders that window from the
 * predicted pose and minimises the scan against it.  Poses cross as column-major double[16] (Eigen::Matrix4d::data()). */
class Localizer {
 public:
  explicit Localizer(const suma_params& p, const suma_localizer_params* lp = nullptr, int device = 0) {
    if (suma_localizer_create(&p, lp, device, &l_) != SUMA_OK)
      throw std::runtime_error(std::string("suma_localizer_create: ") + suma_last_error(nullptr));
  }
  ~Localizer() { suma_localizer_destroy(l_); }
  Localizer(const Localizer&) = delete;
  Localizer& operator=(const Localizer&) = delete;

  /* returns the records that were dropped (non-finite position, outside the tile grid) */
  uint32_t setMap(const std::vector<suma_world_surfel>& records) {
    uint32_t dropped = 0;
    chk(suma_localizer_set_map(l_, records.data(), (uint32_t)records.size(), &dropped), "Localizer::setMap");
    return dropped;
  }
  uint32_t setMapDevice(const suma_world_surfel* d_records, uint32_t n) {
    uint32_t dropped = 0;
    chk(suma_localizer_set_map_device(l_, d_records, n, &dropped), "Localizer::setMapDevice");
    return dropped;
  }
  void setPose(const double T[16]) { chk(suma_localizer_set_pose(l_, T), "Localizer::setPose"); }
  suma_localizer_result processScan(const suma_float4* points, const float* labels, const float* probs, uint32_t n,
                                    int32_t fixed_iterations = 0) {
    suma_localizer_result r;
    chk(suma_localizer_process_scan(l_, points, labels, probs, n, fixed_iterations, &r), "Localizer::processScan");
    return r;
  }
  /* global relocalisation (suma_localizer_relocalize): no setPose is needed.  poses16: one column-major pose per entry
   * of the index, by entry index.  The result is large (every candidate's match and scan result): it is returned through
   * the caller's object.  found = 0 leaves the localiser as it was. */
  void relocalize(const PlaceIndex& index, const std::vector<double>& poses16, const suma_float4* points,
                  const float* labels, const float* probs, uint32_t n, uint32_t max_candidates,
                  suma_relocalize_result* out, int32_t fixed_iterations = 0) {
    chk(suma_localizer_relocalize(l_, index.get(), poses16.data(), (uint32_t)(poses16.size() / 16), points, labels, probs, n,
                                  max_candidates, fixed_iterations, out),
        "Localizer::relocalize");
  }
  /* origin tile, records in the window, gathers since setMap */
  void window(int32_t origin_ij[2], uint32_t* n_window, uint32_t* rebuilds) {
    chk(suma_localizer_window(l_, origin_ij, n_window, rebuilds), "Localizer::window");
  }
  std::vector<suma_surfel> downloadWindow() {
    uint32_t n = 0;
    chk(suma_localizer_window(l_, nullptr, &n, nullptr), "Localizer::downloadWindow");
    std::vector<suma_surfel> out(n);
    chk(suma_localizer_download_window(l_, out.data(), n, &n), "Localizer::downloadWindow");
    out.resize(n < out.size() ? n : out.size());
    return out;
  }
  /* change evidence (csrc/k_change.hip): from the next setMap on, every record collects hits / misses / occluded /
   * label_changes from each tracked scan and from every observeFrame; cp NULL = the defaults */
  void enableEvidence(const suma_change_params* cp = nullptr) {
    chk(suma_localizer_enable_evidence(l_, cp), "Localizer::enableEvidence");
  }
  void disableEvidence() { chk(suma_localizer_disable_evidence(l_), "Localizer::disableEvidence"); }
  /* one observation of a data-sized frame of ctx() at the sensor pose T (column-major, world frame) */
  suma_change_counts observeFrame(const suma_frame* frame, const double T[16]) {
    suma_change_counts c;
    chk(suma_localizer_observe_frame(l_, frame, T, &c), "Localizer::observeFrame");
    return c;
  }
  /* the totals of the last processScan's observation; *observed (optional): whether it observed */
  suma_change_counts lastObservation(bool* observed = nullptr) {
    suma_change_counts c;
    int32_t o = 0;
    chk(suma_localizer_last_observation(l_, &c, &o), "Localizer::lastObservation");
    if (observed) *observed = o != 0;
    return c;
  }
  /* one entry per record setMap was given, in that order */
  std::vector<suma_change_evidence> evidence() {
    uint32_t n = 0;
    chk(suma_localizer_evidence(l_, nullptr, 0, &n), "Localizer::evidence");
    std::vector<suma_change_evidence> out(n);
    if (n) chk(suma_localizer_evidence(l_, out.data(), n, &n), "Localizer::evidence");
    return out;
  }
  void clearEvidence() { chk(suma_localizer_clear_evidence(l_), "Localizer::clearEvidence"); }
  /* the records the rule keeps (suma_change_prune_mask over evidence(); rule NULL = the defaults); *keep (optional): the
   * mask, one byte per record */
  std::vector<suma_world_surfel> prunedMap(const std::vector<suma_world_surfel>& records,
                                           const suma_change_rule* rule = nullptr, std::vector<uint8_t>* keep = nullptr) {
    const std::vector<suma_change_evidence> ev = evidence();
    if (ev.size() != records.size()) throw std::runtime_error("Localizer::prunedMap: one evidence entry per record is needed");
    std::vector<uint8_t> k(ev.size());
    if (suma_change_prune_mask(ev.data(), (uint32_t)ev.size(), rule, k.data(), nullptr) != SUMA_OK)
      throw std::runtime_error(std::string("suma_change_prune_mask: ") + suma_last_error(nullptr));
    std::vector<suma_world_surfel> out;
    for (size_t i = 0; i < records.size(); ++i)
      if (k[i]) out.push_back(records[i]);
    if (keep) keep->swap(k);
    return out;
  }
  /* newly seen surfaces (csrc/k_novel.hip): from now on every tracked scan ends with one collection of the texels no
   * record of the window explains; np NULL = the defaults (201 MB of candidates are allocated) */
  void enableNovelty(const suma_novel_params* np = nullptr) {
    chk(suma_localizer_enable_novelty(l_, np), "Localizer::enableNovelty");
  }
  void disableNovelty() { chk(suma_localizer_disable_novelty(l_), "Localizer::disableNovelty"); }
  /* ---- motion compensation of raw sweeps: as SurfelMapping's, with the localiser's increment as the motion (the
   *      identity after setPose); relocalize does not correct ---- */
  void enableDeskew(const suma_deskew_params* dp = nullptr) { chk(suma_localizer_enable_deskew(l_, dp), "Localizer::enableDeskew"); }
  void disableDeskew() { chk(suma_localizer_disable_deskew(l_), "Localizer::disableDeskew"); }
  void setDeskewMotion(const double* motion16) { chk(suma_localizer_set_deskew_motion(l_, motion16), "Localizer::setDeskewMotion"); }
  int32_t deskewMotion(double* motion16) {
    int32_t source = SUMA_DESKEW_MOTION_NONE;
    chk(suma_localizer_deskew_motion(l_, motion16, &source), "Localizer::deskewMotion");
    return source;
  }
  /* one collection of a data-sized frame of ctx() at the sensor pose T (column-major, world frame) */
  suma_novel_counts collectFrame(const suma_frame* frame, const double T[16], uint32_t scan_id) {
    suma_novel_counts c;
    chk(suma_localizer_collect_frame(l_, frame, T, scan_id, &c), "Localizer::collectFrame");
    return c;
  }
  /* the counts of the last processScan's collection; *collected (optional): whether it collected */
  suma_novel_counts lastCollection(bool* collected = nullptr) {
    suma_novel_counts c;
    int32_t o = 0;
    chk(suma_localizer_last_collection(l_, &c, &o), "Localizer::lastCollection");
    if (collected) *collected = o != 0;
    return c;
  }
  /* the candidates in creation order */
  std::vector<suma_world_surfel> novelCandidates() {
    uint32_t n = 0;
    chk(suma_localizer_novel_candidates(l_, nullptr, 0, &n), "Localizer::novelCandidates");
    std::vector<suma_world_surfel> out(n);
    if (n) chk(suma_localizer_novel_candidates(l_, out.data(), n, &n), "Localizer::novelCandidates");
    return out;
  }
  /* the candidates fused per voxel, kept where min_views scans agree (fp NULL = the defaults); *views (optional): how
   * many scans each record was seen by; *stats (optional) */
  std::vector<suma_world_surfel> novel(const suma_novel_fuse_params* fp = nullptr, std::vector<uint32_t>* views = nullptr,
                                       suma_novel_stats* stats = nullptr) {
    suma_novel_stats st;
    chk(suma_localizer_novel(l_, fp, nullptr, nullptr, 0, &st), "Localizer::novel");
    std::vector<suma_world_surfel> out(st.n_out);
    std::vector<uint32_t> v(st.n_out);
    if (st.n_out) chk(suma_localizer_novel(l_, fp, out.data(), v.data(), st.n_out, &st), "Localizer::novel");
    if (views) views->swap(v);
    if (stats) *stats = st;
    return out;
  }
  void clearNovelty() { chk(suma_localizer_clear_novelty(l_), "Localizer::clearNovelty"); }
  /* the records prunedMap keeps (all of them while the map has no evidence) followed by novel()'s: what goes into the
   * next setMap */
  std::vector<suma_world_surfel> updatedMap(const std::vector<suma_world_surfel>& records,
                                            const suma_change_rule* rule = nullptr,
                                            const suma_novel_fuse_params* fp = nullptr) {
    uint32_t n = 0;
    std::vector<suma_world_surfel> out =
        suma_localizer_evidence(l_, nullptr, 0, &n) == SUMA_OK ? prunedMap(records, rule) : records;
    const std::vector<suma_world_surfel> fresh = novel(fp);
    out.insert(out.end(), fresh.begin(), fresh.end());
    return out;
  }
  /* objects in front of the robot (csrc/k_objects.hip): with novelty on, every collection is followed by one
   * segmentation of its unexplained texels into objects; nothing else the localiser gives changes */
  void enableObjects(const suma_object_params* op = nullptr) {
    chk(suma_localizer_enable_objects(l_, op), "Localizer::enableObjects");
  }
  void disableObjects() { chk(suma_localizer_disable_objects(l_), "Localizer::disableObjects"); }
  /* the objects of the last segmentation in ascending root order; *segmented = false (and nothing returned) when the
   * last scan or collectFrame segmented nothing.  Throws when more than max_objects were found */
  std::vector<suma_scan_object> objects(suma_object_counts* counts = nullptr, bool* segmented = nullptr) {
    uint32_t n = 0;
    int32_t seg = 0;
    suma_object_counts c;
    int rc = suma_localizer_objects(l_, nullptr, 0, &n, &c, &seg);
    if (rc != SUMA_ERR_CAPACITY) chk(rc, "Localizer::objects");
    std::vector<suma_scan_object> out(n);
    if (n) chk(suma_localizer_objects(l_, out.data(), n, &n, &c, &seg), "Localizer::objects");
    else chk(rc, "Localizer::objects");
    if (counts) *counts = c;
    if (segmented) *segmented = seg != 0;
    return out;
  }
  /* the id image of the last segmentation: the object number of every texel, 0xffffffff for none */
  std::vector<uint32_t> objectIds() {
    uint32_t n = 0;
    chk(suma_localizer_object_ids(l_, nullptr, 0, &n), "Localizer::objectIds");
    std::vector<uint32_t> out(n);
    if (n) chk(suma_localizer_object_ids(l_, out.data(), n, &n), "Localizer::objectIds");
    return out;
  }
  /* the primitive on a caller's flag image (one byte a texel of the data image) */
  suma_object_counts segmentFlags(const suma_frame* frame, const double T[16], const uint8_t* flags, uint32_t scan_id) {
    suma_object_counts c;
    chk(suma_localizer_segment_flags(l_, frame, T, flags, scan_id, &c), "Localizer::segmentFlags");
    return c;
  }
  /* tracks (csrc/k_tracks.hip): with objects on, every segmentation is followed by one tracker update -- fragments joined
   * into detections, detections associated to tracks, ids kept, velocities filtered; nothing else the localiser gives
   * changes */
  void enableTracks(const suma_track_params* tp = nullptr) { chk(suma_localizer_enable_tracks(l_, tp), "Localizer::enableTracks"); }
  void disableTracks() { chk(suma_localizer_disable_tracks(l_), "Localizer::disableTracks"); }
  void clearTracks() { chk(suma_localizer_clear_tracks(l_), "Localizer::clearTracks"); }
  /* the live tracks of the last update in ascending slot order; *updated = false (and nothing returned) when there was
   * none.  Throws when detections found no free slot */
  std::vector<suma_object_track> tracks(suma_track_counts* counts = nullptr, bool* updated = nullptr) {
    uint32_t n = 0;
    int32_t upd = 0;
    suma_track_counts c;
    int rc = suma_localizer_tracks(l_, nullptr, 0, &n, &c, &upd);
    if (rc != SUMA_ERR_CAPACITY) chk(rc, "Localizer::tracks");
    std::vector<suma_object_track> out(n);
    if (n) chk(suma_localizer_tracks(l_, out.data(), n, &n, &c, &upd), "Localizer::tracks");
    else chk(rc, "Localizer::tracks");
    if (counts) *counts = c;
    if (updated) *updated = upd != 0;
    return out;
  }
  /* per object of the last update the id of its track, 0 for none: objectTracks()[objectIds()[texel]] is a texel's track */
  std::vector<uint32_t> objectTracks() {
    uint32_t n = 0;
    chk(suma_localizer_object_tracks(l_, nullptr, 0, &n), "Localizer::objectTracks");
    std::vector<uint32_t> out(n);
    if (n) chk(suma_localizer_object_tracks(l_, out.data(), n, &n), "Localizer::objectTracks");
    return out;
  }
  /* the primitive on a caller's records in place of a segmentation's */
  suma_track_counts trackObjects(const std::vector<suma_scan_object>& objects, uint32_t scan_id) {
    suma_track_counts c;
    chk(suma_localizer_track_objects(l_, objects.data(), (uint32_t)objects.size(), scan_id, &c), "Localizer::trackObjects");
    return c;
  }
  /* live obstacles for the planner (csrc/k_live.hip): with novelty on, every collection is followed by one update of a
   * layer over the static grid gp / cells (host cells, uploaded for the call); nothing else the localiser gives changes */
  void enableLiveGrid(const suma_grid_params& gp, const std::vector<suma_grid_cell>& cells, const suma_live_params* lp = nullptr) {
    if (cells.size() != (size_t)gp.width * gp.height) throw std::runtime_error("Localizer::enableLiveGrid: cells do not fit the raster");
    void* d = nullptr;
    chk(suma_device_alloc(ctx(), cells.size() * sizeof(suma_grid_cell), &d), "Localizer::enableLiveGrid");
    int rc = suma_device_upload(ctx(), d, cells.data(), cells.size() * sizeof(suma_grid_cell));
    if (rc == SUMA_OK) rc = suma_localizer_enable_live_grid(l_, &gp, (const suma_grid_cell*)d, lp);
    std::string why = rc == SUMA_OK ? "" : suma_last_error(ctx());
    suma_device_free(ctx(), d);
    if (rc != SUMA_OK) throw std::runtime_error("Localizer::enableLiveGrid: " + why);
    live_cells_ = cells.size();
  }
  /* the device form: d_cells = what suma_world_grid wrote for gp, only read */
  void enableLiveGridDevice(const suma_grid_params& gp, const suma_grid_cell* d_cells, const suma_live_params* lp = nullptr) {
    chk(suma_localizer_enable_live_grid(l_, &gp, d_cells, lp), "Localizer::enableLiveGrid");
    live_cells_ = (size_t)gp.width * gp.height;
  }
  void disableLiveGrid() {
    chk(suma_localizer_disable_live_grid(l_), "Localizer::disableLiveGrid");
    live_cells_ = 0;
  }
  void clearLiveGrid() { chk(suma_localizer_clear_live_grid(l_), "Localizer::clearLiveGrid"); }
  suma_live_counts liveUpdateFlags(const suma_frame* frame, const double T[16], const uint8_t* flags, uint32_t scan_id) {
    suma_live_counts c;
    chk(suma_localizer_live_update_flags(l_, frame, T, flags, scan_id, &c), "Localizer::liveUpdateFlags");
    return c;
  }
  /* the counts of the last update; *updated = false when there was none */
  suma_live_counts liveCounts(bool* updated = nullptr) {
    suma_live_counts c;
    int32_t u = 0;
    chk(suma_localizer_live_counts(l_, &c, &u), "Localizer::liveCounts");
    if (updated) *updated = u != 0;
    return c;
  }
  /* composes: the static cells with the live obstacles written into them, what suma_grid_plan_field takes; mask: one byte
   * a cell, 1 live, 2 pending */
  std::vector<suma_grid_cell> liveCells(std::vector<uint8_t>* mask = nullptr, suma_live_stats* stats = nullptr) {
    std::vector<suma_grid_cell> out(live_cells_);
    void *d = nullptr, *dm = nullptr;
    chk(suma_device_alloc(ctx(), live_cells_ * sizeof(suma_grid_cell) + 48, &d), "Localizer::liveCells");
    int rc = suma_device_alloc(ctx(), live_cells_ + 16, &dm);
    if (rc == SUMA_OK) rc = suma_localizer_live_cells_device(l_, (suma_grid_cell*)d, (uint8_t*)dm, stats);
    if (rc == SUMA_OK && live_cells_) rc = suma_device_download(ctx(), out.data(), d, live_cells_ * sizeof(suma_grid_cell));
    if (rc == SUMA_OK && mask) {
      mask->resize(live_cells_);
      if (live_cells_) rc = suma_device_download(ctx(), mask->data(), dm, live_cells_);
    }
    std::string why = rc == SUMA_OK ? "" : suma_last_error(ctx());
    suma_device_free(ctx(), d);
    if (dm) suma_device_free(ctx(), dm);
    if (rc != SUMA_OK) throw std::runtime_error("Localizer::liveCells: " + why);
    return out;
  }
  /* the device form, for suma_grid_plan_field to read the cells where they are */
  void liveCellsDevice(suma_grid_cell* d_out, uint8_t* d_mask = nullptr, suma_live_stats* stats = nullptr) {
    chk(suma_localizer_live_cells_device(l_, d_out, d_mask, stats), "Localizer::liveCells");
  }
  suma_localizer* get() const { return l_; }
  suma_ctx* ctx() const { return suma_localizer_ctx(l_); }

 private:
  void chk(int rc, const char* what) { check(suma_localizer_ctx(l_), rc, what); }
  suma_localizer* l_ = nullptr;
  size_t live_cells_ = 0; /* of the live layer's raster; 0: off */
};

}  // namespace suma_hip
#endif
