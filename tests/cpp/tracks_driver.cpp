// Drives the tracks of suma_hip::Localizer (include/suma_adapter.hpp) the way a C++ host would:
//   tracks_driver <updates.bin> <max_tracks> <join_dist> <max_missed>
// updates.bin: per update uint32 scan_id, uint32 n, then n suma_scan_object records.  Switches novelty, objects and tracks
// on, plays the updates through trackObjects and prints per update
//   "<the twelve suma_track_counts>",
//   "<tracks> <FNV-1a 64 of the live tracks' bytes, hex> <FNV-1a 64 of the per-object track ids' bytes, hex>";
// then clears the tracks, plays the first update again and prints its two lines once more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "suma_adapter.hpp"

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static unsigned long long fnv(const void* data, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return (unsigned long long)h;
}

static void play(suma_hip::Localizer& loc, const std::vector<suma_scan_object>& rec, uint32_t scan_id) {
  const suma_track_counts c = loc.trackObjects(rec, scan_id);
  std::printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", c.n_objects, c.n_detections, c.n_joined, c.n_tracks_before, c.n_matched,
              c.n_missed, c.n_expired, c.n_born, c.n_dropped, c.n_confirmed, c.n_unresolved, c.rounds);
  suma_track_counts again;
  bool updated = false;
  const std::vector<suma_object_track> tracks = loc.tracks(&again, &updated);
  const std::vector<uint32_t> ids = loc.objectTracks();
  if (!updated || std::memcmp(&again, &c, sizeof(c)) != 0 || ids.size() != rec.size()) throw std::runtime_error("tracks() disagrees");
  std::printf("%zu %016llx %016llx\n", tracks.size(), fnv(tracks.data(), tracks.size() * sizeof(suma_object_track)),
              fnv(ids.data(), ids.size() * sizeof(uint32_t)));
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s updates.bin max_tracks join_dist max_missed\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> ub = slurp(argv[1]);
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = 70;
    p.data_height = p.model_height = 3;
    suma_hip::Localizer loc(p);
    suma_novel_params np;
    suma_novel_params_default(&np);
    np.max_candidates = 1024;
    loc.enableNovelty(&np);
    loc.enableObjects();
    suma_track_params tp;
    suma_track_params_default(&tp);
    tp.max_tracks = (uint32_t)std::atoi(argv[2]);
    tp.join_dist = (float)std::atof(argv[3]);
    tp.max_missed = (uint32_t)std::atoi(argv[4]);
    loc.enableTracks(&tp);
    bool updated = true;
    if (!loc.tracks(nullptr, &updated).empty() || updated) throw std::runtime_error("tracks before an update");
    std::vector<suma_scan_object> first;
    uint32_t first_id = 0;
    for (size_t at = 0, k = 0; at < ub.size(); ++k) {
      uint32_t head[2];
      if (at + sizeof(head) > ub.size()) throw std::runtime_error("updates.bin: a header is cut short");
      std::memcpy(head, ub.data() + at, sizeof(head));
      at += sizeof(head);
      if (at + (size_t)head[1] * sizeof(suma_scan_object) > ub.size()) throw std::runtime_error("updates.bin: records are cut short");
      std::vector<suma_scan_object> rec(head[1]);
      if (head[1]) std::memcpy(rec.data(), ub.data() + at, (size_t)head[1] * sizeof(suma_scan_object));
      at += (size_t)head[1] * sizeof(suma_scan_object);
      if (k == 0) first = rec, first_id = head[0];
      play(loc, rec, head[0]);
    }
    loc.clearTracks();
    play(loc, first, first_id);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "tracks_driver: %s\n", e.what());
    return 1;
  }
}
