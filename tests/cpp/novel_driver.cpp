// Drives the collection of newly seen surfaces of suma_hip::Localizer (include/suma_adapter.hpp) the way a C++ host would:
//   novel_driver <map.bin> <pose.bin> <frame.bin> <width> <height> <extent> <dimension> <max_range> <max_angle> <evidence>
// map.bin: 48-byte suma_world_surfel records; pose.bin: the sensor pose, column-major double[16]; frame.bin: the vertex,
// normal and semantic maps of one data-sized frame, height x width x 4 floats each.  Sets the map and the pose, observes
// the frame three times when <evidence> is 1, collects
// the frame twice (scan ids 0 and 1) and prints
//   "<n_texels> <no_return> <out_of_range> <grazing> <explained> <novel> <stored>" of the second collection,
//   "<candidates> <fused records> <records of updatedMap> <FNV-1a 64 of updatedMap's bytes, hex>".
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
  if (argc != 11) {
    std::fprintf(stderr, "usage: %s map.bin pose.bin frame.bin width height extent dimension max_range max_angle evidence\n",
                 argv[0]);
    return 2;
  }
  try {
    const std::vector<char> mb = slurp(argv[1]), pb = slurp(argv[2]), fb = slurp(argv[3]);
    if (pb.size() != 16 * sizeof(double)) throw std::runtime_error("pose.bin: 16 doubles expected");
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[4]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[5]);
    p.submap_extent = (float)std::atof(argv[6]);
    p.submap_dimension = std::atoi(argv[7]);
    p.max_angle = (float)std::atof(argv[9]);
    const size_t texels = (size_t)p.data_width * p.data_height;
    if (fb.size() != 3 * texels * sizeof(suma_float4)) throw std::runtime_error("frame.bin: three maps expected");
    suma_hip::Localizer loc(p);
    suma_novel_params np;
    suma_novel_params_default(&np);
    np.max_range = (float)std::atof(argv[8]);
    np.max_candidates = 4096;
    loc.enableNovelty(&np);
    if (std::atoi(argv[10])) loc.enableEvidence();
    const suma_world_surfel* recs = (const suma_world_surfel*)mb.data();
    const std::vector<suma_world_surfel> records(recs, recs + mb.size() / sizeof(suma_world_surfel));
    loc.setMap(records);
    const double* T = (const double*)pb.data();
    loc.setPose(T);
    suma_frame* f = nullptr;
    suma_hip::check(loc.ctx(), suma_frame_create(loc.ctx(), p.data_width, p.data_height, &f), "suma_frame_create");
    const suma_float4* maps = (const suma_float4*)fb.data();
    for (int which = 0; which < 3; ++which)
      suma_hip::check(loc.ctx(), suma_frame_upload(loc.ctx(), f, which, maps + which * texels), "suma_frame_upload");
    if (std::atoi(argv[10]))
      for (int k = 0; k < 3; ++k) loc.observeFrame(f, T); /* the default rule removes nothing below three misses */
    loc.collectFrame(f, T, 0);
    const suma_novel_counts c = loc.collectFrame(f, T, 1);
    std::printf("%u %u %u %u %u %u %u\n", c.n_texels, c.no_return, c.out_of_range, c.grazing, c.explained, c.novel, c.stored);
    const std::vector<suma_world_surfel> cand = loc.novelCandidates(), fused = loc.novel(), upd = loc.updatedMap(records);
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)upd.data();
    for (size_t i = 0; i < upd.size() * sizeof(suma_world_surfel); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::printf("%zu %zu %zu %016llx\n", cand.size(), fused.size(), upd.size(), (unsigned long long)h);
    suma_frame_destroy(f);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "novel_driver: %s\n", e.what());
    return 1;
  }
}
