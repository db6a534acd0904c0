// Stand-alone check of the checkpoint container's parser (semantic_suma_amd/csrc/checkpoint_format.h): builds a minimal
// valid image and runs ckpt::parse over deterministic mutations of it.  Every mutation must be refused -- by the parser,
// or, where it keeps the container well formed, by the comparison of the payload digests with the directory.  Each candidate lives in a heap block of exactly
// its length, so a read outside the image is a sanitizer error (the test compiles this with -fsanitize=address,undefined).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "checkpoint_format.h"

namespace {

struct Sec {
  uint32_t id;
  std::vector<unsigned char> data;
  uint64_t count;
};

uint64_t rng_state = 0x1234567887654321ull;
unsigned char rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned char)(rng_state >> 56);
}
std::vector<unsigned char> noise(size_t n) {
  std::vector<unsigned char> v(n);
  for (auto& b : v) b = rnd();
  return v;
}
template <class T>
std::vector<unsigned char> bytes_of(const T& t) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&t);
  return std::vector<unsigned char>(p, p + sizeof(T));
}

std::vector<unsigned char> build(const std::vector<Sec>& secs) {
  const uint32_t n = (uint32_t)secs.size();
  std::vector<ckpt::DirEntry> dir(n);
  uint64_t at = ckpt::head_bytes(n);
  for (uint32_t k = 0; k < n; ++k) {
    memset(&dir[k], 0, sizeof(dir[k]));
    dir[k].id = secs[k].id, dir[k].offset = at, dir[k].bytes = secs[k].data.size(), dir[k].count = secs[k].count;
    dir[k].digest = ckpt::digest(secs[k].data.data(), secs[k].data.size());
    at = ckpt::round_up(at + secs[k].data.size());
  }
  std::vector<unsigned char> img(at, 0);
  ckpt::Header h;
  h.magic = ckpt::MAGIC, h.version = ckpt::VERSION, h.n_sections = n, h.total_bytes = at;
  memcpy(img.data(), &h, sizeof(h));
  memcpy(img.data() + sizeof(h), dir.data(), n * sizeof(ckpt::DirEntry));
  const uint64_t dig_at = sizeof(h) + n * sizeof(ckpt::DirEntry), hd = ckpt::digest(img.data(), dig_at);
  memcpy(img.data() + dig_at, &hd, 8);
  for (uint32_t k = 0; k < n; ++k)
    if (!secs[k].data.empty()) memcpy(img.data() + dir[k].offset, secs[k].data.data(), secs[k].data.size());
  return img;
}

std::vector<Sec> minimal(const std::vector<ckpt::Tile>& tiles, uint64_t n_tile_records) {
  const uint32_t T = 2, n_active = 3, P = 4;
  ckpt::Pipeline pp;
  memset(&pp, 0, sizeof(pp));
  pp.timestamp = T;
  ckpt::MapState ms;
  memset(&ms, 0, sizeof(ms));
  ms.timestamp = T, ms.n_active = n_active, ms.n_extraction = 1;
  std::vector<unsigned char> msb = bytes_of(ms);
  const int32_t ext[2] = {1, -1};
  msb.insert(msb.end(), reinterpret_cast<const unsigned char*>(ext), reinterpret_cast<const unsigned char*>(ext) + 8);
  std::vector<unsigned char> td;
  for (const ckpt::Tile& t : tiles) {
    const std::vector<unsigned char> b = bytes_of(t);
    td.insert(td.end(), b.begin(), b.end());
  }
  return {{ckpt::PARAMS, noise(232), 1},
          {ckpt::PIPELINE, bytes_of(pp), 1},
          {ckpt::MAP_STATE, msb, 1},
          {ckpt::POSES, noise(64 * T), T},
          {ckpt::ACTIVE, noise(64 * n_active), n_active},
          {ckpt::FRAME, noise(48 * P), 3 * P},
          {ckpt::TILE_DIR, td, tiles.size()},
          {ckpt::TILES, noise(64 * n_tile_records), n_tile_records}};
}

unsigned long n_tried = 0, n_accepted = 0;

// parses a copy of exactly `len` bytes and, if the parser accepts it, compares every payload digest with the directory
// (the load's two gates).  most: the most that may happen to this candidate -- 0: the parser must refuse it;
// 1: it must be refused by the parser or by the digests; 2: it may pass both
bool try_image(const unsigned char* src, size_t len, int most) {
  unsigned char* block = static_cast<unsigned char*>(malloc(len ? len : 1));
  if (len) memcpy(block, src, len);
  ckpt::Parsed P;
  std::string err;
  const bool ok = ckpt::parse(len ? block : nullptr, len, &P, &err);
  int got = 0;
  bool fine = true;
  ++n_tried;
  if (ok) {
    uint32_t bad = 0;
    got = ckpt::verify_digests(block, P, &bad) ? 2 : 1;
    n_accepted += got == 2;
  } else if (err.empty()) {
    printf("rejected without a message\n");
    fine = false;
  }
  if (got > most) {
    printf("a candidate that must be refused %s\n", got == 2 ? "passed the parser and the digests" : "passed the parser");
    fine = false;
  }
  free(block);
  return fine;
}

}  // namespace

int main() {
  const std::vector<ckpt::Tile> good = {{-1, 0, 0, 2}, {-1, 3, 2, 1}, {4, -2, 3, 3}};
  const std::vector<unsigned char> img = build(minimal(good, 6));
  int failures = 0;
  {
    ckpt::Parsed P;
    std::string err;
    if (!ckpt::parse(img.data(), img.size(), &P, &err) || !ckpt::verify_digests(img.data(), P, nullptr)) {
      printf("the minimal image is refused: %s\n", err.c_str());
      return 1;
    }
    // every truncation length around each boundary (header, directory, every section start and end)
    std::vector<uint64_t> cuts = {0, sizeof(ckpt::Header), ckpt::head_bytes(P.h.n_sections), img.size()};
    for (uint32_t k = 0; k < P.h.n_sections; ++k) {
      cuts.push_back(P.dir[k].offset);
      cuts.push_back(P.dir[k].offset + P.dir[k].bytes);
    }
    for (uint64_t cut : cuts)
      for (int64_t d = -9; d <= 9; ++d) {
        const int64_t len = (int64_t)cut + d;
        if (len < 0 || (uint64_t)len >= img.size()) continue;
        failures += !try_image(img.data(), (size_t)len, 0);
      }
    // a longer buffer than the header states
    std::vector<unsigned char> longer(img);
    longer.resize(img.size() + 64, 0);
    failures += !try_image(longer.data(), longer.size(), 0);
    // every single-byte change of the header and directory (and their digest and padding) to 0x00, 0xFF and value + 1
    const uint64_t head = ckpt::head_bytes(P.h.n_sections);
    std::vector<unsigned char> m(img);
    for (uint64_t at = 0; at < head; ++at) {
      const unsigned char keep = m[at];
      const unsigned char vals[3] = {0x00, 0xFF, (unsigned char)(keep + 1)};
      for (unsigned char v : vals) {
        if (v == keep) continue;
        m[at] = v;
        failures += !try_image(m.data(), m.size(), 0); /* the header's own digest notices every one */
      }
      m[at] = keep;
    }
    // the same with the header's digest made right again: the directory's own checks must hold without it
    const uint64_t dig_at = sizeof(ckpt::Header) + (uint64_t)P.h.n_sections * sizeof(ckpt::DirEntry);
    for (uint64_t at = 0; at < dig_at; ++at) {
      const unsigned char keep = m[at];
      const unsigned char vals[3] = {0x00, 0xFF, (unsigned char)(keep + 1)};
      for (unsigned char v : vals) {
        if (v == keep) continue;
        m[at] = v;
        const uint64_t hd = ckpt::digest(m.data(), dig_at);
        memcpy(m.data() + dig_at, &hd, 8);
        failures += !try_image(m.data(), m.size(), 1);
      }
      m[at] = keep;
    }
    {
      const uint64_t hd = ckpt::digest(m.data(), dig_at);
      memcpy(m.data() + dig_at, &hd, 8);
      failures += !try_image(m.data(), m.size(), 2);
      if (n_accepted != 1) printf("the restored image is refused\n"), ++failures;
    }
    // single-byte changes of the fixed records the parser reads through (MAP_STATE, TILE_DIR)
    for (uint32_t id : {(uint32_t)ckpt::MAP_STATE, (uint32_t)ckpt::TILE_DIR, (uint32_t)ckpt::PIPELINE}) {
      const ckpt::DirEntry* e = P.find(id);
      std::vector<unsigned char> q(img);
      for (uint64_t at = e->offset; at < e->offset + e->bytes; ++at) {
        const unsigned char keep = q[at];
        const unsigned char vals[3] = {0x00, 0xFF, (unsigned char)(keep + 1)};
        for (unsigned char v : vals) {
          if (v == keep) continue;
          q[at] = v;
          failures += !try_image(q.data(), q.size(), 1);
        }
        q[at] = keep;
      }
    }
  }
  // overlapping, reversed, out-of-range, empty and unsorted tile runs: all must be refused
  const std::vector<std::vector<ckpt::Tile>> bad_runs = {
      {{-1, 0, 0, 2}, {-1, 3, 1, 2}, {4, -2, 3, 3}},           // overlapping
      {{-1, 0, 3, 3}, {-1, 3, 2, 1}, {4, -2, 0, 2}},           // reversed
      {{-1, 0, 0, 2}, {-1, 3, 2, 1}, {4, -2, 3, 4}},           // leaves TILES
      {{-1, 0, 0, 2}, {-1, 3, 2, 1}, {4, -2, 0xfffffff0u, 3}}, // far out of range
      {{-1, 0, 0, 2}, {-1, 3, 2, 1}, {4, -2, 3, 0xffffffffu}}, // count wraps
      {{-1, 0, 0, 2}, {-1, 3, 2, 1}, {4, -2, 3, 2}},           // does not cover TILES
      {{-1, 0, 0, 2}, {-1, 3, 2, 0}, {4, -2, 2, 4}},           // an empty tile
      {{-1, 3, 0, 2}, {-1, 0, 2, 1}, {4, -2, 3, 3}},           // not ascending by (i, j)
      {{-1, 0, 0, 2}, {-1, 0, 2, 1}, {4, -2, 3, 3}},           // the same tile twice
      {{-1, 0, 1, 2}, {-1, 3, 3, 1}, {4, -2, 4, 2}},           // a gap at the start
  };
  for (const auto& runs : bad_runs) {
    const std::vector<unsigned char> b = build(minimal(runs, 6));
    failures += !try_image(b.data(), b.size(), 0);
  }
  printf("%lu mutations, %lu accepted, %d failures\n", n_tried, n_accepted, failures);
  return failures ? 1 : 0;
}
