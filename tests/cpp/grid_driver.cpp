// Drives suma_hip::SurfelMap::exportGrid (include/suma_adapter.hpp) the way a C++ host would:
//   grid_driver <surfels.bin> <poses.bin> <cell_size> <fit_margin>
// surfels.bin: 64-byte suma_surfel records; poses.bin: column-major float[16] per pose.  Prints one line:
//   <width> <height> <the nine stats> <FNV-1a 64 of the cells' bytes, hex>
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
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s surfels.bin poses.bin cell_size fit_margin\n", argv[0]);
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
    suma_grid_params gp;
    suma_grid_params_default(&gp);
    gp.cell_size = (float)std::atof(argv[3]);
    suma_grid_stats st;
    const std::vector<suma_grid_cell> out = map.exportGrid(gp, wp, std::atoi(argv[4]), &st);
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)out.data();
    for (size_t i = 0; i < out.size() * sizeof(suma_grid_cell); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::printf("%u %u %u %u %u %u %u %u %u %u %u %016llx\n", gp.width, gp.height, st.n_records, st.n_dropped, st.n_outside,
                st.n_binned, st.n_occupied, st.n_free, st.n_obstacle, st.n_no_ground, st.n_filled, (unsigned long long)h);
    return out.size() == (size_t)gp.width * gp.height ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "grid_driver: %s\n", e.what());
    return 1;
  }
}
