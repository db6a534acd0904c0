// Drives the per-scan objects of suma_hip::Localizer (include/suma_adapter.hpp) the way a C++ host would:
//   objects_driver <frame.bin> <flags.bin> <pose.bin> <width> <height> <link_base> <link_slope> <min_texels> <max_objects>
// frame.bin: the vertex, normal and semantic maps of one data-sized frame, height x width x 4 floats each; flags.bin: one
// byte a texel; pose.bin: the sensor pose, column-major double[16].  Switches novelty and objects on, segments the frame's
// flagged texels and prints
//   "<n_texels> <n_members> <n_components> <n_small> <n_objects> <stored>",
//   "<records> <FNV-1a 64 of the records' bytes, hex> <FNV-1a 64 of the id image's bytes, hex>".
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

static unsigned long long fnv(const void* data, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return (unsigned long long)h;
}

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s frame.bin flags.bin pose.bin width height link_base link_slope min_texels max_objects\n",
                 argv[0]);
    return 2;
  }
  try {
    const std::vector<char> fb = slurp(argv[1]), gb = slurp(argv[2]), pb = slurp(argv[3]);
    if (pb.size() != 16 * sizeof(double)) throw std::runtime_error("pose.bin: 16 doubles expected");
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[4]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[5]);
    const size_t texels = (size_t)p.data_width * p.data_height;
    if (fb.size() != 3 * texels * sizeof(suma_float4)) throw std::runtime_error("frame.bin: three maps expected");
    if (gb.size() != texels) throw std::runtime_error("flags.bin: one byte a texel expected");
    suma_hip::Localizer loc(p);
    suma_novel_params np;
    suma_novel_params_default(&np);
    np.max_candidates = 1024;
    loc.enableNovelty(&np);
    suma_object_params op;
    suma_object_params_default(&op);
    op.link_base = (float)std::atof(argv[6]);
    op.link_slope = (float)std::atof(argv[7]);
    op.min_texels = (uint32_t)std::atoi(argv[8]);
    op.max_objects = (uint32_t)std::atoi(argv[9]);
    loc.enableObjects(&op);
    suma_frame* f = nullptr;
    suma_hip::check(loc.ctx(), suma_frame_create(loc.ctx(), p.data_width, p.data_height, &f), "suma_frame_create");
    const suma_float4* maps = (const suma_float4*)fb.data();
    for (int which = 0; which < 3; ++which)
      suma_hip::check(loc.ctx(), suma_frame_upload(loc.ctx(), f, which, maps + which * texels), "suma_frame_upload");
    const suma_object_counts c = loc.segmentFlags(f, (const double*)pb.data(), (const uint8_t*)gb.data(), 7u);
    std::printf("%u %u %u %u %u %u\n", c.n_texels, c.n_members, c.n_components, c.n_small, c.n_objects, c.stored);
    suma_object_counts again;
    bool segmented = false;
    const std::vector<suma_scan_object> rec = loc.objects(&again, &segmented);
    const std::vector<uint32_t> ids = loc.objectIds();
    if (!segmented || again.n_objects != c.n_objects || ids.size() != texels) throw std::runtime_error("objects() disagrees");
    std::printf("%zu %016llx %016llx\n", rec.size(), fnv(rec.data(), rec.size() * sizeof(suma_scan_object)),
                fnv(ids.data(), ids.size() * sizeof(uint32_t)));
    suma_frame_destroy(f);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "objects_driver: %s\n", e.what());
    return 1;
  }
}
