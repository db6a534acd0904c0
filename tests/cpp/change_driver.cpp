// Drives the change evidence of suma_hip::Localizer (include/suma_adapter.hpp) the way a C++ host would:
//   change_driver <map.bin> <start.bin> <scan dir> <n scans> <width> <height> <extent> <dimension>
// map.bin: 48-byte suma_world_surfel records; start.bin: the start pose, column-major double[16]; the scan directory
// holds %06d.bin (x, y, z, 1 floats), %06d.label and %06d.prob (one float a point).  Prints per scan
//   <observed> <n_window> <unseen> <no_return> <occluded> <misses> <grazing> <hits> <near> <label_changes>
// and a last line "<records> <FNV-1a 64 of the evidence's bytes, hex> <records the default rule removes> <records kept>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "suma_adapter.hpp"

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s map.bin start.bin scan_dir n_scans width height extent dimension\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> mb = slurp(argv[1]), sb = slurp(argv[2]);
    if (sb.size() != 16 * sizeof(double)) throw std::runtime_error("start.bin: 16 doubles expected");
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[5]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[6]);
    p.submap_extent = (float)std::atof(argv[7]);
    p.submap_dimension = std::atoi(argv[8]);
    suma_hip::Localizer loc(p);
    loc.enableEvidence();
    const suma_world_surfel* recs = (const suma_world_surfel*)mb.data();
    const std::vector<suma_world_surfel> records(recs, recs + mb.size() / sizeof(suma_world_surfel));
    loc.setMap(records);
    loc.setPose((const double*)sb.data());
    const int n_scans = std::atoi(argv[4]);
    for (int k = 0; k < n_scans; ++k) {
      char name[32];
      std::snprintf(name, sizeof(name), "/%06d", k);
      const std::string base = std::string(argv[3]) + name;
      const std::vector<char> pts = slurp(base + ".bin"), lab = slurp(base + ".label"), prob = slurp(base + ".prob");
      const uint32_t n = (uint32_t)(pts.size() / sizeof(suma_float4));
      if (lab.size() != n * sizeof(float) || prob.size() != n * sizeof(float)) throw std::runtime_error("scan files differ in length");
      loc.processScan((const suma_float4*)pts.data(), (const float*)lab.data(), (const float*)prob.data(), n);
      bool observed = false;
      const suma_change_counts c = loc.lastObservation(&observed);
      std::printf("%d %u %u %u %u %u %u %u %u %u\n", observed ? 1 : 0, c.n_window, c.unseen, c.no_return, c.occluded, c.misses,
                  c.grazing, c.hits, c.near, c.label_changes);
    }
    const std::vector<suma_change_evidence> ev = loc.evidence();
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)ev.data();
    for (size_t i = 0; i < ev.size() * sizeof(suma_change_evidence); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::vector<uint8_t> keep;
    const std::vector<suma_world_surfel> kept = loc.prunedMap(records, nullptr, &keep);
    size_t removed = 0;
    for (size_t i = 0; i < keep.size(); ++i) removed += keep[i] ? 0 : 1;
    std::printf("%zu %016llx %zu %zu\n", ev.size(), (unsigned long long)h, removed, kept.size());
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "change_driver: %s\n", e.what());
    return 1;
  }
}
