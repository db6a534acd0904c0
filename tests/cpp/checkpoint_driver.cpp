// Drives suma_hip::SurfelMapping::saveCheckpoint / loadCheckpoint (include/suma_adapter.hpp) the way a C++ host would:
//   checkpoint_driver <velodyne_dir> <n_scans> <save_after> <width> <file>
// Pipeline A runs all n_scans and saves to <file> after scan number save_after - 1; pipeline B is created afterwards,
// loads <file> and runs the remaining scans.  One line per scan on stdout: the scan number and the 16 doubles of the
// pose as bit patterns, first A's n_scans lines, then B's n_scans - save_after lines.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "suma_adapter.hpp"

static std::vector<suma_float4> read_scan(const char* dir, int k) {
  char path[4096];
  std::snprintf(path, sizeof(path), "%s/%06d.bin", dir, k);
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  std::fseek(f, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(f) / sizeof(suma_float4);
  std::fseek(f, 0, SEEK_SET);
  std::vector<suma_float4> pts(n);
  const bool ok = std::fread(pts.data(), sizeof(suma_float4), n, f) == n;
  std::fclose(f);
  if (!ok) throw std::runtime_error(std::string("short read: ") + path);
  return pts;
}

static void step(suma_hip::SurfelMapping& m, const char* dir, int k) {
  const std::vector<suma_float4> pts = read_scan(dir, k);
  const std::vector<float> zero(pts.size(), 0.0f);
  m.processScan(pts.data(), zero.data(), zero.data(), (uint32_t)pts.size(), 6);
  double T[16];
  m.getCurrentPose(T);
  std::printf("%d", k);
  for (int i = 0; i < 16; ++i) {
    uint64_t u;
    std::memcpy(&u, &T[i], 8);
    std::printf(" %016" PRIx64, u);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s velodyne_dir n_scans save_after width file\n", argv[0]);
    return 2;
  }
  const char* dir = argv[1];
  const int n_scans = std::atoi(argv[2]), save_after = std::atoi(argv[3]);
  suma_params p;
  suma_params_default(&p);
  p.data_width = p.model_width = (uint32_t)std::atoi(argv[4]);
  try {
    {
      suma_hip::SurfelMapping a(p);
      for (int k = 0; k < n_scans; ++k) {
        step(a, dir, k);
        if (k + 1 == save_after) a.saveCheckpoint(argv[5]);
      }
    }
    suma_hip::SurfelMapping b(p);
    b.loadCheckpoint(argv[5]);
    if ((int)b.timestamp() != save_after) throw std::runtime_error("the loaded pipeline is at another scan");
    for (int k = save_after; k < n_scans; ++k) step(b, dir, k);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "checkpoint_driver: %s\n", e.what());
    return 1;
  }
}
