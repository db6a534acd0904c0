/*
 * checkpoint_format.h -- the container of a pipeline checkpoint (k_checkpoint.hip states the image in full): header,
 * directory, the fixed payload records, the digest and a bounds-checked parser.  Plain C++, no HIP: the library
 * (suma_checkpoint.hip) and the stand-alone parser test (tests/cpp/checkpoint_parse_driver.cpp) both include it.
 * Little-endian hosts only, as the rest of the library.
 */
#ifndef SUMA_CHECKPOINT_FORMAT_H_
#define SUMA_CHECKPOINT_FORMAT_H_

#include <stdint.h>
#include <string.h>

#include <string>

namespace ckpt {

constexpr uint64_t MAGIC = 0x3150434b414d5553ull; /* the bytes "SUMAKCP1" */
constexpr uint32_t VERSION = 1;
constexpr uint64_t ALIGN = 64;
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr uint32_t MAX_SECTIONS = 16;

enum : uint32_t { PARAMS = 1, PIPELINE, MAP_STATE, POSES, ACTIVE, FRAME, TILE_DIR, TILES, LOOP, GRAPH, OPT, N_IDS };

inline const char* section_name(uint32_t id) {
  static const char* const names[N_IDS] = {"?",     "PARAMS",   "PIPELINE", "MAP_STATE", "POSES", "ACTIVE",
                                           "FRAME", "TILE_DIR", "TILES",    "LOOP",      "GRAPH", "OPT"};
  return id < N_IDS ? names[id] : "?";
}

struct Header { /* 24 bytes; the directory follows, then the 64-bit digest of every byte before it */
  uint64_t magic;
  uint32_t version, n_sections;
  uint64_t total_bytes;
};
struct DirEntry { /* 40 bytes */
  uint32_t id, reserved;
  uint64_t offset, bytes, count, digest; /* payload bytes (without the padding), records, digest of the payload */
};

/* ---- payload records ---- */
struct IcpStats { /* = suma_icp_stats */
  double error, inlier_residual;
  uint32_t valid, outlier, inlier, invalid, iterations, converged;
};
struct Pipeline {
  double current_pose[16], last_pose[16], pose_old[16], pose_new[16], last_increment[16], last_pose_old[16];
  uint32_t timestamp, track_loss;
  IcpStats stats, stats_mst;
};
struct MapState { /* followed by n_extraction x {int32 i, j}, in stack order (the back of the stack last) */
  uint32_t timestamp;
  int32_t origin_i, origin_j;
  uint32_t n_active;
  /* the counters of the last update that the C-ABI shows (suma_map_counts, suma_map_export_data_surfels) */
  uint32_t n_updated, n_kept_updated, n_data, n_kept_data;
  uint32_t n_extraction, reserved;
};
struct Tile {
  int32_t i, j;
  uint32_t first, count; /* records [first, first + count) of TILES */
};
struct LoopHead { /* followed by: suma_loop_params (params_bytes), n_traj floats (padded to 8 bytes), the unverified
                     then the verified candidates */
  uint32_t params_bytes, n_traj, n_unverified, n_verified;
  int32_t already_verified;
  uint32_t loop_count, time_without;
  /* the per-scan status of the last scan */
  int32_t found, use, started, integrated, candidate_to;
  uint32_t edges_added;
  float result_old_outlier_ratio, loop_valid_ratio, loop_outlier_ratio, loop_relative_error_all;
  uint32_t result_old_inlier, result_old_outlier, result_old_valid, result_old_invalid;
  uint32_t reserved;
  double result_old_error, result_old_residual, result_old_inlier_residual, posegraph_error;
};
struct Candidate {
  int32_t from, to;
  double rel_pose[16];
};
struct GraphHead { /* followed by n_nodes x {initial[12], result[12]} (R row-major | t), then n_edges x Edge */
  uint32_t n_nodes, n_edges;
};
struct Edge {
  int32_t from, to;
  double Z[12], information[36]; /* as stored: R row-major | t; symmetrised, row-major */
};
struct OptHead { /* followed by n_opt x 12 doubles: the clone's optimised poses */
  int32_t before_id;
  uint32_t before_loop_count, started_at;
  int32_t worker_rc;
  uint32_t n_opt, reserved;
  double before_pose[16];
};

static_assert(sizeof(Header) == 24 && sizeof(DirEntry) == 40 && sizeof(IcpStats) == 40, "packed");
static_assert(sizeof(Pipeline) == 856 && sizeof(MapState) == 40 && sizeof(Tile) == 16, "packed");
static_assert(sizeof(LoopHead) == 120 && sizeof(Candidate) == 136 && sizeof(Edge) == 392 && sizeof(OptHead) == 152,
              "packed");

inline uint64_t round_up(uint64_t v) { return (v + (ALIGN - 1)) & ~(ALIGN - 1); }
/* header + directory + their digest, padded */
inline uint64_t head_bytes(uint32_t n_sections) {
  return round_up(sizeof(Header) + (uint64_t)n_sections * sizeof(DirEntry) + 8);
}

/* The digest of a payload read as n little-endian 64-bit words w[k] (a tail shorter than a word is zero-extended):
 * sum over k of (w[k] + GOLDEN) * (2 k + 1) mod 2^64.  An integer sum: any order of accumulation gives the same value. */
inline uint64_t digest(const void* payload, uint64_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(payload);
  const uint64_t n = bytes / 8;
  uint64_t sum = 0, w;
  for (uint64_t k = 0; k < n; ++k) {
    memcpy(&w, b + 8 * k, 8);
    sum += (w + GOLDEN) * (2 * k + 1);
  }
  if (bytes % 8) {
    w = 0;
    memcpy(&w, b + 8 * n, bytes % 8);
    sum += (w + GOLDEN) * (2 * n + 1);
  }
  return sum;
}

struct Parsed {
  Header h;
  DirEntry dir[MAX_SECTIONS];
  int index[N_IDS]; /* id -> position in dir, -1: absent */
  Pipeline pipeline;
  MapState map;
  const DirEntry* find(uint32_t id) const { return (id < N_IDS && index[id] >= 0) ? &dir[index[id]] : nullptr; }
};

namespace detail {
inline bool bad(std::string* err, const std::string& msg) {
  if (err) *err = msg;
  return false;
}
inline bool all_zero(const unsigned char* b, uint64_t n) {
  for (uint64_t k = 0; k < n; ++k)
    if (b[k]) return false;
  return true;
}
}  // namespace detail

/* Validates everything about the container that can be told without the pipeline it is meant for: every offset, size
 * and count against the image length and against each other, BEFORE anything is read through them.  Accepts only the
 * canonical layout: sections in ascending id order, back to back at 64-byte boundaries, zero padding, no gaps.
 * The payload digests are NOT compared here (verify_digests, or kc_verify on the device). */
inline bool parse(const void* image, uint64_t bytes, Parsed* out, std::string* err) {
  using detail::bad;
  const unsigned char* b = static_cast<const unsigned char*>(image);
  if (!image || !out) return bad(err, "no image");
  if (bytes < sizeof(Header)) return bad(err, "image shorter than its header");
  Parsed& P = *out;
  memcpy(&P.h, b, sizeof(Header));
  if (P.h.magic != MAGIC) return bad(err, "not a checkpoint image (magic)");
  if (P.h.version != VERSION) return bad(err, "format version " + std::to_string(P.h.version) + " is not supported");
  if (P.h.n_sections < 8 || P.h.n_sections > MAX_SECTIONS) return bad(err, "header: bad section count");
  if (P.h.total_bytes != bytes) return bad(err, "header: total bytes differ from the image length (truncated?)");
  if (bytes % ALIGN) return bad(err, "header: image length is not a multiple of 64");
  const uint64_t head = head_bytes(P.h.n_sections), dig_at = sizeof(Header) + (uint64_t)P.h.n_sections * sizeof(DirEntry);
  if (head > bytes) return bad(err, "image shorter than its directory");
  uint64_t hd;
  memcpy(&hd, b + dig_at, 8);
  if (hd != digest(b, dig_at)) return bad(err, "header: digest mismatch");
  if (!detail::all_zero(b + dig_at + 8, head - dig_at - 8)) return bad(err, "header: padding is not zero");
  for (uint32_t k = 0; k < N_IDS; ++k) P.index[k] = -1;
  uint64_t at = head;
  uint32_t last_id = 0;
  for (uint32_t s = 0; s < P.h.n_sections; ++s) {
    DirEntry& e = P.dir[s];
    memcpy(&e, b + sizeof(Header) + (uint64_t)s * sizeof(DirEntry), sizeof(DirEntry));
    const std::string name = section_name(e.id);
    if (e.id == 0 || e.id >= N_IDS || e.id <= last_id) return bad(err, "directory: section ids must ascend");
    if (e.reserved != 0) return bad(err, "directory: reserved word of " + name);
    last_id = e.id;
    P.index[e.id] = (int)s;
    if (e.offset != at) return bad(err, "directory: " + name + " does not start where the section before it ends");
    if (e.bytes > bytes - e.offset) return bad(err, "directory: " + name + " runs past the end of the image");
    const uint64_t end = round_up(e.offset + e.bytes); /* <= bytes: bytes is a multiple of 64 */
    if (!detail::all_zero(b + e.offset + e.bytes, end - (e.offset + e.bytes)))
      return bad(err, "section " + name + ": padding is not zero");
    at = end;
  }
  if (at != bytes) return bad(err, "directory: the sections do not cover the image");
  for (uint32_t id = PARAMS; id <= TILES; ++id)
    if (P.index[id] < 0) return bad(err, std::string("directory: section ") + section_name(id) + " is missing");
  if ((P.index[LOOP] < 0) != (P.index[GRAPH] < 0)) return bad(err, "directory: LOOP and GRAPH come together");
  if (P.index[OPT] >= 0 && P.index[LOOP] < 0) return bad(err, "directory: OPT without LOOP");

  const DirEntry &pa = *P.find(PARAMS), &pi = *P.find(PIPELINE), &ms = *P.find(MAP_STATE), &po = *P.find(POSES),
                 &ac = *P.find(ACTIVE), &fr = *P.find(FRAME), &td = *P.find(TILE_DIR), &ti = *P.find(TILES);
  if (pa.count != 1 || pa.bytes == 0) return bad(err, "section PARAMS: bad size");
  if (pi.count != 1 || pi.bytes != sizeof(Pipeline)) return bad(err, "section PIPELINE: bad size");
  memcpy(&P.pipeline, b + pi.offset, sizeof(Pipeline));
  if (ms.count != 1 || ms.bytes < sizeof(MapState)) return bad(err, "section MAP_STATE: bad size");
  memcpy(&P.map, b + ms.offset, sizeof(MapState));
  if ((ms.bytes - sizeof(MapState)) / 8 != P.map.n_extraction || (ms.bytes - sizeof(MapState)) % 8 || P.map.reserved)
    return bad(err, "section MAP_STATE: the extraction stack does not fit its size");
  if (P.pipeline.timestamp != P.map.timestamp) return bad(err, "PIPELINE and MAP_STATE disagree on the timestamp");
  if (po.count != P.map.timestamp || po.bytes / 64 != po.count || po.bytes % 64)
    return bad(err, "section POSES: one 64-byte row per scan");
  if (ac.count != P.map.n_active || ac.bytes / 64 != ac.count || ac.bytes % 64)
    return bad(err, "section ACTIVE: one 64-byte record per active surfel");
  if (fr.bytes / 16 != fr.count || fr.bytes % 16 || fr.count % 3) return bad(err, "section FRAME: three maps of 16-byte texels");
  if (td.bytes / sizeof(Tile) != td.count || td.bytes % sizeof(Tile)) return bad(err, "section TILE_DIR: bad size");
  if (ti.bytes / 64 != ti.count || ti.bytes % 64) return bad(err, "section TILES: 64-byte records");
  if (ti.count > 0xffffffffull) return bad(err, "section TILES: more than 2^32 - 1 records");
  uint64_t next = 0;
  Tile prev{};
  for (uint64_t k = 0; k < td.count; ++k) {
    Tile t;
    memcpy(&t, b + td.offset + k * sizeof(Tile), sizeof(Tile));
    if (t.count == 0) return bad(err, "TILE_DIR: an empty tile");
    if (t.first != next) return bad(err, "TILE_DIR: tile runs must be disjoint, in order, and cover TILES exactly");
    if (t.count > ti.count - next) return bad(err, "TILE_DIR: a tile run leaves TILES");
    if (k && !(t.i > prev.i || (t.i == prev.i && t.j > prev.j))) return bad(err, "TILE_DIR: tiles must ascend by (i, j)");
    next += t.count;
    prev = t;
  }
  if (next != ti.count) return bad(err, "TILE_DIR: tile runs must be disjoint, in order, and cover TILES exactly");

  if (const DirEntry* lo = P.find(LOOP)) {
    LoopHead lh;
    if (lo->count != 1 || lo->bytes < sizeof(LoopHead)) return bad(err, "section LOOP: bad size");
    memcpy(&lh, b + lo->offset, sizeof(LoopHead));
    const uint64_t want = sizeof(LoopHead) + (uint64_t)lh.params_bytes + (((uint64_t)lh.n_traj * 4 + 7) & ~7ull) +
                          ((uint64_t)lh.n_unverified + lh.n_verified) * sizeof(Candidate);
    if (lh.params_bytes % 8 || lo->bytes != want) return bad(err, "section LOOP: its counts do not fit its size");
    const DirEntry* gr = P.find(GRAPH);
    GraphHead gh;
    if (gr->bytes < sizeof(GraphHead)) return bad(err, "section GRAPH: bad size");
    memcpy(&gh, b + gr->offset, sizeof(GraphHead));
    if (gr->count != gh.n_nodes || gr->bytes != sizeof(GraphHead) + (uint64_t)gh.n_nodes * 192 + (uint64_t)gh.n_edges * sizeof(Edge))
      return bad(err, "section GRAPH: its counts do not fit its size");
    for (uint64_t k = 0; k < gh.n_edges; ++k) {
      int32_t ft[2];
      memcpy(ft, b + gr->offset + sizeof(GraphHead) + (uint64_t)gh.n_nodes * 192 + k * sizeof(Edge), 8);
      if (ft[0] < 0 || ft[1] < 0 || (uint32_t)ft[0] >= gh.n_nodes || (uint32_t)ft[1] >= gh.n_nodes || ft[0] == ft[1])
        return bad(err, "section GRAPH: an edge between nodes that do not exist");
    }
    if (const DirEntry* op = P.find(OPT)) {
      OptHead oh;
      if (op->bytes < sizeof(OptHead)) return bad(err, "section OPT: bad size");
      memcpy(&oh, b + op->offset, sizeof(OptHead));
      if (op->count != oh.n_opt || op->bytes != sizeof(OptHead) + (uint64_t)oh.n_opt * 96 || oh.reserved)
        return bad(err, "section OPT: its count does not fit its size");
      if (oh.n_opt > gh.n_nodes || oh.before_id < 0 || (uint32_t)oh.before_id >= oh.n_opt)
        return bad(err, "section OPT: the optimised graph does not fit the pipeline's graph");
    }
  }
  return true;
}

/* host-side comparison of every payload digest with the directory; *bad_id = the first section that differs */
inline bool verify_digests(const void* image, const Parsed& P, uint32_t* bad_id) {
  const unsigned char* b = static_cast<const unsigned char*>(image);
  for (uint32_t s = 0; s < P.h.n_sections; ++s)
    if (digest(b + P.dir[s].offset, P.dir[s].bytes) != P.dir[s].digest) {
      if (bad_id) *bad_id = P.dir[s].id;
      return false;
    }
  return true;
}

}  // namespace ckpt

#endif
