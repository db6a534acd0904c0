/*
 * suma_checkpoint.hip -- suma_pipeline_checkpoint_size / _save / _load, suma_checkpoint_info / _params / _digest: the host
 * side of a pipeline checkpoint.  The image is specified at the top of k_checkpoint.hip, its container and parser are
 * checkpoint_format.h, the loop-closing payloads are written and installed by suma_loop.hip.
 *
 * Save: the small sections are built on the host; POSES, ACTIVE, FRAME and TILES are packed where they lie by kc_pack,
 * which also accumulates their digests; the finished image leaves the device in ONE copy.  Load: parse and check on the
 * host, stage the image, verify every section's digest on the device (kc_verify), and only then write the pipeline.
 * The staged image is a DevBuf of the ctx grown by the one rule (grow); it is kept for the next save -- releasing it
 * would be a hipFree, which synchronises the whole device (acceptable off the scan path, but pointless between
 * periodic saves).  Nothing here runs unless one of these entries is called.
 */
#include <string.h>

#include <string>
#include <vector>

#include "suma_internal.h"
#include "checkpoint_format.h"

static_assert(sizeof(ckpt::IcpStats) == sizeof(suma_icp_stats), "checkpoint_format.h mirrors suma_icp_stats");
static_assert(sizeof(ckpt::Tile) == 16 && sizeof(suma_surfel) == 64 && sizeof(CacheSlot) == 8, "record sizes");
static_assert(sizeof(suma_params) % 4 == 0, "suma_params is compared word by word");
static_assert(SUMA_CHECKPOINT_MAX_SECTIONS == ckpt::MAX_SECTIONS && SUMA_CHECKPOINT_VERSION == ckpt::VERSION, "header");

namespace {

/* suma_params, one name per 32-bit word, in declaration order */
const char* const kParamNames[] = {
    "data_width", "data_height", "data_fov_up", "data_fov_down", "min_depth", "max_depth", "model_width", "model_height",
    "model_fov_up", "model_fov_down", "model_min_depth", "model_max_depth", "max_iterations", "stopping_threshold", "delta",
    "icp_max_distance", "icp_max_angle", "weight_function", "factor", "bilinear_sampling", "initialize_identity",
    "fallback_mode", "fallback_max_distance", "fallback_max_angle", "compose_rendering", "max_loop_closure_distance",
    "min_radius", "max_radius", "max_angle", "map_max_distance", "map_max_angle", "unstable_age", "confidence_mode",
    "confidence_threshold", "p_stable", "p_prior", "sigma_angle", "sigma_distance", "use_stability", "active_timestamps",
    "max_weight", "weighting_scheme", "averaging_scheme", "update_always", "submap_dimension", "submap_extent",
    "partial_extraction", "max_surfels", "max_poses", "label_offset", "prob_offset", "cache_surfels", "avg_vertexmap",
    "filter_vertexmap", "use_filtered_vertexmap", "bilateral_sigma_space", "bilateral_sigma_range", "filter_sampling"};
static_assert(sizeof(kParamNames) / sizeof(kParamNames[0]) == sizeof(suma_params) / 4, "one name per field of suma_params");

struct TileRef {
  int32_t i, j;
  CacheSlot slot;
};

/* what a save needs to know before it sizes the image */
struct Gathered {
  uint32_t n_active = 0;
  std::vector<TileRef> tiles;
  uint64_t n_parked = 0;
  uint64_t loop_bytes = 0, graph_bytes = 0, opt_bytes = 0;
};

struct Section {
  uint32_t id;
  uint64_t bytes, count;
};

/* the refusals that need no device work and no join: a refused save has changed nothing, not even when the optimiser's
 * worker is joined */
int refuse(suma_pipeline* s, const char* who) {
  suma_ctx* c = s->c;
  if (s->phase != 0)
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": only between scans (after suma_pipeline_update_map)");
  if (ingest_pending(c)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": a prefetched scan is pending");
  if (s->timestamp != c->timestamp)
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": the map's timestamp differs from the pipeline's");
  return SUMA_OK;
}

int gather(suma_pipeline* s, const char* who, Gathered* g) {
  suma_ctx* c = s->c;
  int rr = refuse(s, who);
  if (rr) return rr;
  if (c->gate_pending) HIP_TRY(c, flush_gate(c));
  const uint32_t ns = (uint32_t)c->cache_index.size();
  std::vector<CacheSlot> slots(ns);
  HIP_TRY(c, hipMemcpyAsync(c->h_ds, c->ds, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
  if (ns) HIP_TRY(c, hipMemcpyAsync(slots.data(), c->cache_slots, ns * sizeof(CacheSlot), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int r = check_overflow(c); /* a truncated map is not a state to resume from */
  if (r) return r;
  if (c->h_ds->n_surfels > c->p.max_surfels) return fail(c, SUMA_ERR_CAPACITY, std::string(who) + ": the map exceeds max_surfels");
  g->n_active = c->h_ds->n_surfels;
  for (const auto& kv : c->cache_index) { /* std::map: ascending by (i, then j) */
    const CacheSlot q = slots[kv.second];
    if (q.count == 0) continue;
    if ((uint64_t)q.offset + q.count > c->cache_cap)
      return fail(c, SUMA_ERR_HIP, "submap cache slot outside the arena (internal error)");
    g->tiles.push_back({kv.first.first, kv.first.second, q});
    g->n_parked += q.count;
  }
  if (g->n_parked >= (1ull << 30) || g->n_active >= (1u << 30))
    return fail(c, SUMA_ERR_CAPACITY, std::string(who) + ": 2^30 records or more in one section");
  g->loop_bytes = loop_ckpt_sizes(s, &g->graph_bytes, &g->opt_bytes);
  return SUMA_OK;
}

std::vector<Section> sections_of(const suma_pipeline* s, const Gathered& g) {
  const suma_ctx* c = s->c;
  std::vector<Section> v;
  v.push_back({ckpt::PARAMS, sizeof(suma_params), 1});
  v.push_back({ckpt::PIPELINE, sizeof(ckpt::Pipeline), 1});
  v.push_back({ckpt::MAP_STATE, sizeof(ckpt::MapState) + 8ull * c->extraction.size(), 1});
  v.push_back({ckpt::POSES, 64ull * c->timestamp, c->timestamp});
  v.push_back({ckpt::ACTIVE, 64ull * g.n_active, g.n_active});
  v.push_back({ckpt::FRAME, 48ull * c->P, 3ull * c->P});
  v.push_back({ckpt::TILE_DIR, 16ull * g.tiles.size(), g.tiles.size()});
  v.push_back({ckpt::TILES, 64ull * g.n_parked, g.n_parked});
  if (s->loop) {
    uint32_t n = 0;
    (void)posegraph_host_poses(suma_pipeline_posegraph(const_cast<suma_pipeline*>(s)), &n);
    v.push_back({ckpt::LOOP, g.loop_bytes, 1});
    v.push_back({ckpt::GRAPH, g.graph_bytes, n});
    if (g.opt_bytes) v.push_back({ckpt::OPT, g.opt_bytes, (g.opt_bytes - sizeof(ckpt::OptHead)) / 96});
  }
  return v;
}

uint64_t layout(const std::vector<Section>& v, ckpt::DirEntry* dir) {
  uint64_t at = ckpt::head_bytes((uint32_t)v.size());
  for (size_t k = 0; k < v.size(); ++k) {
    memset(&dir[k], 0, sizeof(dir[k]));
    dir[k].id = v[k].id, dir[k].offset = at, dir[k].bytes = v[k].bytes, dir[k].count = v[k].count;
    at = ckpt::round_up(at + v[k].bytes);
  }
  return at;
}

}  // namespace

extern "C" uint64_t suma_checkpoint_digest(const void* payload, uint64_t bytes) {
  return (payload || bytes == 0) ? ckpt::digest(payload, bytes) : 0;
}

extern "C" int suma_checkpoint_info(const void* image, uint64_t bytes, struct suma_checkpoint_info* out) {
  if (!image || !out) return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_info: NULL argument");
  ckpt::Parsed P;
  std::string err;
  if (!ckpt::parse(image, bytes, &P, &err)) return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_info: " + err);
  memset(out, 0, sizeof(*out));
  out->version = P.h.version;
  out->timestamp = P.map.timestamp;
  out->n_active = P.map.n_active;
  out->n_tiles = (uint32_t)P.find(ckpt::TILE_DIR)->count;
  out->n_parked = P.find(ckpt::TILES)->count;
  out->has_loop = P.find(ckpt::LOOP) != nullptr, out->has_opt = P.find(ckpt::OPT) != nullptr;
  if (const ckpt::DirEntry* gr = P.find(ckpt::GRAPH)) {
    ckpt::GraphHead gh;
    memcpy(&gh, static_cast<const char*>(image) + gr->offset, sizeof(gh));
    out->n_nodes = gh.n_nodes, out->n_edges = gh.n_edges;
  }
  out->n_sections = P.h.n_sections;
  out->total_bytes = P.h.total_bytes;
  for (uint32_t k = 0; k < P.h.n_sections; ++k) {
    out->sections[k].id = P.dir[k].id;
    out->sections[k].bytes = P.dir[k].bytes;
    out->sections[k].digest = P.dir[k].digest;
  }
  return SUMA_OK;
}

extern "C" int suma_checkpoint_params(const void* image, uint64_t bytes, suma_params* out) {
  if (!image || !out) return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_params: NULL argument");
  ckpt::Parsed P;
  std::string err;
  if (!ckpt::parse(image, bytes, &P, &err)) return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_params: " + err);
  const ckpt::DirEntry* pa = P.find(ckpt::PARAMS);
  if (pa->bytes != sizeof(suma_params))
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_params: section PARAMS holds parameters of another size");
  if (ckpt::digest(static_cast<const char*>(image) + pa->offset, pa->bytes) != pa->digest)
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_checkpoint_params: digest mismatch in section PARAMS");
  memcpy(out, static_cast<const char*>(image) + pa->offset, sizeof(*out));
  return SUMA_OK;
}

extern "C" int suma_pipeline_checkpoint_size(suma_pipeline* s, uint64_t* bytes) {
  if (!s || !bytes) return SUMA_ERR_INVALID;
  Gathered g;
  int r = gather(s, "suma_pipeline_checkpoint_size", &g);
  if (r) return r;
  ckpt::DirEntry dir[ckpt::MAX_SECTIONS];
  *bytes = layout(sections_of(s, g), dir);
  return SUMA_OK;
}

extern "C" int suma_pipeline_checkpoint_save(suma_pipeline* s, void* host_dst, uint64_t capacity, uint64_t* written) {
  if (!s || !written || (capacity && !host_dst)) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  *written = 0;
  int r = refuse(s, "suma_pipeline_checkpoint_save");
  if (r) return r;
  loop_ckpt_join(s); /* an optimisation in flight is saved finished (OPT); the size below needs its result */
  Gathered g;
  r = gather(s, "suma_pipeline_checkpoint_save", &g);
  if (r) return r;
  const std::vector<Section> secs = sections_of(s, g);
  ckpt::DirEntry dir[ckpt::MAX_SECTIONS];
  const uint64_t total = layout(secs, dir);
  *written = total;
  if (capacity < total) return fail(c, SUMA_ERR_CAPACITY, "suma_pipeline_checkpoint_save: the image needs " + std::to_string(total) + " bytes");
  suma_icp_stats resolved;
  r = suma_pipeline_last_stats(s, &resolved); /* resolves a pending statistics record */
  if (r) return r;

  /* ---- the host-built payloads ---- */
  std::vector<char> host[ckpt::N_IDS];
  {
    host[ckpt::PARAMS].assign(reinterpret_cast<const char*>(&c->p), reinterpret_cast<const char*>(&c->p) + sizeof(suma_params));
    ckpt::Pipeline pp;
    memset(&pp, 0, sizeof(pp));
    memcpy(pp.current_pose, s->current_pose, 128), memcpy(pp.last_pose, s->last_pose, 128);
    memcpy(pp.pose_old, s->pose_old, 128), memcpy(pp.pose_new, s->pose_new, 128);
    memcpy(pp.last_increment, s->last_increment, 128), memcpy(pp.last_pose_old, s->last_pose_old, 128);
    pp.timestamp = s->timestamp, pp.track_loss = s->track_loss;
    memcpy(&pp.stats, &s->stats, sizeof(pp.stats)), memcpy(&pp.stats_mst, &s->stats_mst, sizeof(pp.stats_mst));
    host[ckpt::PIPELINE].assign(reinterpret_cast<char*>(&pp), reinterpret_cast<char*>(&pp) + sizeof(pp));
    ckpt::MapState ms;
    memset(&ms, 0, sizeof(ms));
    ms.timestamp = c->timestamp, ms.origin_i = c->origin_i, ms.origin_j = c->origin_j, ms.n_active = g.n_active;
    ms.n_updated = c->h_ds->n_updated, ms.n_kept_updated = c->h_ds->n_kept_updated;
    ms.n_data = c->h_ds->n_data, ms.n_kept_data = c->h_ds->n_kept_data;
    ms.n_extraction = (uint32_t)c->extraction.size();
    std::vector<char>& m = host[ckpt::MAP_STATE];
    m.assign(reinterpret_cast<char*>(&ms), reinterpret_cast<char*>(&ms) + sizeof(ms));
    for (const auto& ij : c->extraction) {
      const int32_t e[2] = {ij.first, ij.second};
      m.insert(m.end(), reinterpret_cast<const char*>(e), reinterpret_cast<const char*>(e) + 8);
    }
    std::vector<char>& td = host[ckpt::TILE_DIR];
    uint32_t first = 0;
    for (const TileRef& t : g.tiles) {
      const ckpt::Tile e = {t.i, t.j, first, t.slot.count};
      td.insert(td.end(), reinterpret_cast<const char*>(&e), reinterpret_cast<const char*>(&e) + sizeof(e));
      first += t.slot.count;
    }
    if (s->loop && (r = loop_ckpt_write(s, &host[ckpt::LOOP], &host[ckpt::GRAPH], &host[ckpt::OPT])) != SUMA_OK) return r;
  }
  for (size_t k = 0; k < secs.size(); ++k) {
    const uint32_t id = secs[k].id;
    const bool on_device = id == ckpt::POSES || id == ckpt::ACTIVE || id == ckpt::FRAME || id == ckpt::TILES;
    if (!on_device && host[id].size() != secs[k].bytes)
      return fail(c, SUMA_ERR_INVALID, std::string("suma_pipeline_checkpoint_save: internal: size of section ") + ckpt::section_name(id));
    if (!on_device) dir[k].digest = ckpt::digest(host[id].data(), host[id].size());
  }

  /* ---- the device sections, where the records lie ---- */
  std::vector<WorldSpan> spans; /* in units of 16 bytes; each section's spans start at 0 */
  spans.push_back({reinterpret_cast<const suma_surfel*>(c->poses.p), 0u, 4u * c->timestamp});
  spans.push_back({c->surfels[c->cur].p, 0u, 4u * g.n_active});
  spans.push_back({reinterpret_cast<const suma_surfel*>(s->current_frame->block.p), 0u, (uint32_t)(3 * c->P)});
  {
    uint32_t start = 0;
    for (const TileRef& t : g.tiles) {
      spans.push_back({c->cache_arena.p + t.slot.offset, start, 4u * t.slot.count});
      start += 4u * t.slot.count;
    }
  }
  if (3 * c->P > 0xffffffffull) return fail(c, SUMA_ERR_CAPACITY, "suma_pipeline_checkpoint_save: frame too large");
  if ((r = grow(c, c->ckpt_image, total, {c->stream})) < 0) return r;
  if ((r = grow(c, c->ckpt_spans, spans.size(), {c->stream}, spans.size() + spans.size() / 4 + 64)) < 0) return r;
  if ((r = grow(c, c->ckpt_digests, ckpt::MAX_SECTIONS, {c->stream})) < 0) return r;
  hipStream_t st = c->stream;
  char* img = c->ckpt_image;
  for (size_t k = 0; k < secs.size(); ++k) { /* the padding behind each payload (at most 63 bytes); the rest is overwritten */
    const uint64_t end = dir[k].offset + dir[k].bytes, pad = ckpt::round_up(end) - end;
    if (pad) HIP_TRY(c, hipMemsetAsync(img + end, 0, pad, st));
  }
  HIP_TRY(c, hipMemsetAsync(c->ckpt_digests, 0, ckpt::MAX_SECTIONS * sizeof(unsigned long long), st));
  HIP_TRY(c, hipMemcpyAsync(c->ckpt_spans, spans.data(), spans.size() * sizeof(WorldSpan), hipMemcpyHostToDevice, st));
  for (size_t k = 0; k < secs.size(); ++k) {
    const uint32_t id = secs[k].id;
    unsigned long long* dg = c->ckpt_digests + k;
    const WorldSpan* sp = c->ckpt_spans;
    if (id == ckpt::POSES) HIP_TRY(c, launch_kc_pack(c, sp + 0, 1, 4u * c->timestamp, img + dir[k].offset, dg));
    else if (id == ckpt::ACTIVE) HIP_TRY(c, launch_kc_pack(c, sp + 1, 1, 4u * g.n_active, img + dir[k].offset, dg));
    else if (id == ckpt::FRAME) HIP_TRY(c, launch_kc_pack(c, sp + 2, 1, (uint32_t)(3 * c->P), img + dir[k].offset, dg));
    else if (id == ckpt::TILES)
      HIP_TRY(c, launch_kc_pack(c, sp + 3, (uint32_t)g.tiles.size(), (uint32_t)(4 * g.n_parked), img + dir[k].offset, dg));
    else if (!host[id].empty())
      HIP_TRY(c, hipMemcpyAsync(img + dir[k].offset, host[id].data(), host[id].size(), hipMemcpyHostToDevice, st));
  }
  unsigned long long dig[ckpt::MAX_SECTIONS];
  HIP_TRY(c, hipMemcpyAsync(dig, c->ckpt_digests, sizeof(dig), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (size_t k = 0; k < secs.size(); ++k) {
    const uint32_t id = secs[k].id;
    if (id == ckpt::POSES || id == ckpt::ACTIVE || id == ckpt::FRAME || id == ckpt::TILES) dir[k].digest = dig[k];
  }
  /* ---- header + directory + their digest, then the one copy of the finished image ---- */
  std::vector<char> head(ckpt::head_bytes((uint32_t)secs.size()), 0);
  ckpt::Header h;
  h.magic = ckpt::MAGIC, h.version = ckpt::VERSION, h.n_sections = (uint32_t)secs.size(), h.total_bytes = total;
  memcpy(head.data(), &h, sizeof(h));
  memcpy(head.data() + sizeof(h), dir, secs.size() * sizeof(ckpt::DirEntry));
  const uint64_t dig_at = sizeof(h) + secs.size() * sizeof(ckpt::DirEntry), hd = ckpt::digest(head.data(), dig_at);
  memcpy(head.data() + dig_at, &hd, 8);
  HIP_TRY(c, hipMemcpyAsync(img, head.data(), head.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(host_dst, img, total, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return SUMA_OK;
}

extern "C" int suma_pipeline_checkpoint_load(suma_pipeline* s, const void* image, uint64_t bytes) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  const char* who = "suma_pipeline_checkpoint_load: ";
  if (!image) return fail(c, SUMA_ERR_INVALID, std::string(who) + "NULL image");
  if (s->phase != 0) return fail(c, SUMA_ERR_INVALID, std::string(who) + "only between scans (after suma_pipeline_update_map)");
  /* ---- 1. the host parser: nothing below reads through an offset it has not checked ---- */
  ckpt::Parsed P;
  std::string err;
  if (!ckpt::parse(image, bytes, &P, &err)) return fail(c, SUMA_ERR_INVALID, who + err);
  const char* b = static_cast<const char*>(image);
  const ckpt::DirEntry &pa = *P.find(ckpt::PARAMS), &po = *P.find(ckpt::POSES), &ac = *P.find(ckpt::ACTIVE),
                       &fr = *P.find(ckpt::FRAME), &td = *P.find(ckpt::TILE_DIR), &ti = *P.find(ckpt::TILES),
                       &ms = *P.find(ckpt::MAP_STATE);
  if (pa.bytes != sizeof(suma_params)) return fail(c, SUMA_ERR_INVALID, std::string(who) + "section PARAMS holds parameters of another size");
  {
    uint32_t theirs[sizeof(suma_params) / 4], ours[sizeof(suma_params) / 4];
    memcpy(theirs, b + pa.offset, sizeof(theirs));
    memcpy(ours, &c->p, sizeof(ours));
    for (size_t k = 0; k < sizeof(suma_params) / 4; ++k)
      if (theirs[k] != ours[k])
        return fail(c, SUMA_ERR_INVALID, std::string(who) + "the image was made with other parameters: " + kParamNames[k] + " differs");
  }
  if (fr.count != 3ull * c->P) return fail(c, SUMA_ERR_INVALID, std::string(who) + "section FRAME does not have the size of a data frame");
  if (P.map.n_active > c->p.max_surfels) return fail(c, SUMA_ERR_CAPACITY, std::string(who) + "n_active exceeds max_surfels");
  if (ti.count > c->cache_cap || ti.count >= (1ull << 30)) return fail(c, SUMA_ERR_CAPACITY, std::string(who) + "the parked records exceed the cache arena");
  if (td.count > c->cache_slots_cap) return fail(c, SUMA_ERR_CAPACITY, std::string(who) + "more tiles than cache slots");
  if (P.map.timestamp > c->p.max_poses) return fail(c, SUMA_ERR_CAPACITY, std::string(who) + "timestamp exceeds max_poses");
  const ckpt::DirEntry *lo = P.find(ckpt::LOOP), *gr = P.find(ckpt::GRAPH), *op = P.find(ckpt::OPT);
  suma_loop_params lp;
  int r;
  if (lo && (r = loop_ckpt_check(c, b + lo->offset, b + gr->offset, op ? b + op->offset : nullptr, P.map.timestamp, &lp)) != SUMA_OK)
    return r;
  /* ---- 2. stage the image and verify every section where it lies; the pipeline is still untouched ---- */
  if ((r = grow(c, c->ckpt_image, bytes, {c->stream})) < 0) return r;
  if ((r = grow(c, c->ckpt_digests, ckpt::MAX_SECTIONS, {c->stream})) < 0) return r;
  hipStream_t st = c->stream;
  char* img = c->ckpt_image;
  HIP_TRY(c, hipMemcpyAsync(img, image, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(c->ckpt_digests, 0, ckpt::MAX_SECTIONS * sizeof(unsigned long long), st));
  for (uint32_t k = 0; k < P.h.n_sections; ++k)
    HIP_TRY(c, launch_kc_verify(c, img + P.dir[k].offset, P.dir[k].bytes, c->ckpt_digests + k));
  unsigned long long dig[ckpt::MAX_SECTIONS];
  HIP_TRY(c, hipMemcpyAsync(dig, c->ckpt_digests, sizeof(dig), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (uint32_t k = 0; k < P.h.n_sections; ++k)
    if (dig[k] != P.dir[k].digest)
      return fail(c, SUMA_ERR_INVALID, std::string(who) + "digest mismatch in section " + ckpt::section_name(P.dir[k].id));
  /* ---- 3. write ---- */
  if ((r = suma_pipeline_enable_loop_closing(s, nullptr)) != SUMA_OK) return r; /* joins and drops an optimisation */
  if ((r = suma_pipeline_reset(s)) != SUMA_OK) return r; /* drains both streams and the ingest; clears every cache */
  if (lo && (r = suma_pipeline_enable_loop_closing(s, &lp)) != SUMA_OK) return r;
  const uint32_t T = P.map.timestamp, n_active = P.map.n_active, n_parked = (uint32_t)ti.count, n_tiles = (uint32_t)td.count;
  HIP_TRY(c, launch_set_poses(c, reinterpret_cast<const float*>(img + po.offset), 0, T)); /* and the inverse table */
  if (n_active)
    HIP_TRY(c, hipMemcpyAsync(c->surfels[c->cur], img + ac.offset, ac.bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(s->current_frame->block, img + fr.offset, fr.bytes, hipMemcpyDeviceToDevice, st));
  s->current_frame->version++;
  s->current_frame->last_access = ++c->enq_seq;
  const uint32_t counters[4] = {P.map.n_updated, P.map.n_kept_updated, P.map.n_data, P.map.n_kept_data};
  HIP_TRY(c, launch_kc_unpack(c, img + ti.offset, n_parked, img + td.offset, n_tiles, n_active, counters));
  c->timestamp = T;
  c->origin_i = P.map.origin_i, c->origin_j = P.map.origin_j;
  c->extraction.clear();
  for (uint32_t k = 0; k < P.map.n_extraction; ++k) {
    int32_t e[2];
    memcpy(e, b + ms.offset + sizeof(ckpt::MapState) + 8ull * k, 8);
    c->extraction.push_back({e[0], e[1]});
  }
  c->cache_index.clear();
  for (uint32_t k = 0; k < n_tiles; ++k) {
    ckpt::Tile t;
    memcpy(&t, b + td.offset + sizeof(t) * (uint64_t)k, sizeof(t));
    c->cache_index[{t.i, t.j}] = k; /* slot s is the s-th tile of the directory */
  }
  c->cache_bound = n_parked; /* exact */
  c->cache_nothing_stale = false;
  c->cache_compactions = 0;
  c->known_surfels = n_active;
  memset(c->h_ds.p, 0, sizeof(DevState));
  c->h_ds->n_surfels = n_active, c->h_ds->cache_used = n_parked;
  c->h_ds->n_updated = counters[0], c->h_ds->n_kept_updated = counters[1];
  c->h_ds->n_data = counters[2], c->h_ds->n_kept_data = counters[3];
  c->map_version++;
  const ckpt::Pipeline& pp = P.pipeline;
  memcpy(s->current_pose, pp.current_pose, 128), memcpy(s->last_pose, pp.last_pose, 128);
  memcpy(s->pose_old, pp.pose_old, 128), memcpy(s->pose_new, pp.pose_new, 128);
  memcpy(s->last_increment, pp.last_increment, 128), memcpy(s->last_pose_old, pp.last_pose_old, 128);
  s->timestamp = pp.timestamp, s->track_loss = pp.track_loss;
  memcpy(&s->stats, &pp.stats, sizeof(s->stats)), memcpy(&s->stats_mst, &pp.stats_mst, sizeof(s->stats_mst));
  s->stats_pending = false;
  if (lo && (r = loop_ckpt_install(s, b + lo->offset, b + gr->offset, op ? b + op->offset : nullptr)) != SUMA_OK) return r;
  HIP_TRY(c, hipStreamSynchronize(st));
  return SUMA_OK;
}
