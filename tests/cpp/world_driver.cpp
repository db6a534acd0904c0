// Drives suma_hip::SurfelMap::exportWorld / cachedTiles (include/suma_adapter.hpp) the way a C++ host would:
//   world_driver <surfels.bin> <poses.bin> <voxel_size>
// surfels.bin: 64-byte suma_surfel records; poses.bin: column-major float[16] per pose.  Prints one line:
//   <n_out> <n_passed> <n_dropped> <tiles> <FNV-1a 64 of the records' bytes, hex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "suma_adapter.hpp"

static std::vector<char> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s surfels.bin poses.bin voxel_size\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> sb = slurp(argv[1]), pb = slurp(argv[2]);
    suma_params p;
    suma_params_default(&p);
    suma_hip::Context ctx(p);
    suma_hip::SurfelMap map(ctx);
    const uint32_t n = (uint32_t)(sb.size() / sizeof(suma_surfel)), n_poses = (uint32_t)(pb.size() / 64);
    suma_hip::check(ctx.get(), suma_map_upload(ctx.get(), (const suma_surfel*)sb.data(), n, n_poses), "suma_map_upload");
    map.updatePoses(std::vector<float>((const float*)pb.data(), (const float*)pb.data() + 16 * (size_t)n_poses));
    suma_world_params wp;
    suma_world_params_default(&wp);
    wp.voxel_size = (float)std::atof(argv[3]);
    suma_world_stats st;
    const std::vector<suma_world_surfel> out = map.exportWorld(wp, &st);
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)out.data();
    for (size_t i = 0; i < out.size() * sizeof(suma_world_surfel); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::printf("%u %u %u %zu %016llx\n", st.n_out, st.n_passed, st.n_dropped, map.cachedTiles().size(),
                (unsigned long long)h);
    return out.size() == st.n_out ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "world_driver: %s\n", e.what());
    return 1;
  }
}
