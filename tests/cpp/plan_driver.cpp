// Drives suma_hip::planField / planPaths (include/suma_adapter.hpp) the way a C++ host would:
//   plan_driver <cells.bin> <width> <height> <cell_size> <robot_radius> <path_capacity> <goal> <start> [<start> ...]
// cells.bin: width * height 48-byte suma_grid_cell records; goal and starts are cell indices.  Prints one line:
//   <the six specified stats> <FNV-1a 64 of the field's bytes> <FNV-1a 64 of the results' bytes> <FNV-1a 64 of the rows' bytes>
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

static unsigned long long fnv(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return (unsigned long long)h;
}

int main(int argc, char** argv) {
  if (argc < 9) {
    std::fprintf(stderr, "usage: %s cells.bin width height cell_size robot_radius path_capacity goal start...\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> cb = slurp(argv[1]);
    suma_params p;
    suma_params_default(&p);
    suma_hip::Context ctx(p);
    suma_grid_params gp;
    suma_grid_params_default(&gp);
    gp.width = (uint32_t)std::atoi(argv[2]), gp.height = (uint32_t)std::atoi(argv[3]), gp.cell_size = (float)std::atof(argv[4]);
    suma_plan_params pp;
    suma_plan_params_default(&pp);
    pp.robot_radius = (float)std::atof(argv[5]);
    const uint32_t capacity = (uint32_t)std::atoi(argv[6]);
    const std::vector<suma_grid_cell> cells((const suma_grid_cell*)cb.data(),
                                            (const suma_grid_cell*)cb.data() + cb.size() / sizeof(suma_grid_cell));
    const std::vector<int64_t> goals(1, std::atoll(argv[7]));
    std::vector<int64_t> starts;
    for (int i = 8; i < argc; ++i) starts.push_back(std::atoll(argv[i]));
    suma_plan_stats st;
    const std::vector<suma_plan_cell> field = suma_hip::planField(ctx, gp, pp, cells, goals, &st);
    std::vector<uint32_t> rows;
    const std::vector<suma_plan_path> res = suma_hip::planPaths(ctx, gp, field, starts, capacity, rows);
    std::printf("%u %u %u %u %u %u %016llx %016llx %016llx\n", st.n_blocked, st.n_traversable, st.n_reached, st.n_goals,
                st.n_goals_ignored, st.max_cost, fnv(field.data(), field.size() * sizeof(suma_plan_cell)),
                fnv(res.data(), res.size() * sizeof(suma_plan_path)), fnv(rows.data(), rows.size() * sizeof(uint32_t)));
    return field.size() == (size_t)gp.width * gp.height && st.n_rounds >= 1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "plan_driver: %s\n", e.what());
    return 1;
  }
}
