// Drives suma_hip::SurfelMapping (include/suma_adapter.hpp) with motion compensation on, the way a C++ host with raw
// sweeps would:
//   deskew_driver <scan dir> <n scans> <width> <height> <override scan> <motion.bin>
// The scan directory holds %06d.bin (x, y, z, 1 floats), %06d.label and %06d.prob (one float a point); motion.bin is the
// one-shot override given before scan <override scan>, column-major double[16].  Prints per scan
//   <16 pose doubles as hex bit patterns> <source of the motion the scan used> <its translation's x as a hex bit pattern>
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

static unsigned long long bits(double d) {
  unsigned long long u;
  std::memcpy(&u, &d, 8);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s scan_dir n_scans width height override_scan motion.bin\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> mb = slurp(argv[6]);
    if (mb.size() != 16 * sizeof(double)) throw std::runtime_error("motion.bin: 16 doubles expected");
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[3]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[4]);
    suma_hip::SurfelMapping sm(p);
    suma_deskew_params dp;
    suma_deskew_params_default(&dp);
    sm.enableDeskew(&dp);
    const int n_scans = std::atoi(argv[2]), k_override = std::atoi(argv[5]);
    for (int k = 0; k < n_scans; ++k) {
      char name[32];
      std::snprintf(name, sizeof(name), "/%06d", k);
      const std::string base = std::string(argv[1]) + name;
      const std::vector<char> pts = slurp(base + ".bin"), lab = slurp(base + ".label"), prob = slurp(base + ".prob");
      const uint32_t n = (uint32_t)(pts.size() / sizeof(suma_float4));
      if (lab.size() != n * sizeof(float) || prob.size() != n * sizeof(float)) throw std::runtime_error("scan files differ in length");
      if (k == k_override) sm.setDeskewMotion((const double*)mb.data());
      sm.processScan((const suma_float4*)pts.data(), (const float*)lab.data(), (const float*)prob.data(), n);
      double pose[16], motion[16];
      sm.getCurrentPose(pose);
      const int32_t source = sm.deskewMotion(motion);
      for (int i = 0; i < 16; ++i) std::printf("%016llx ", bits(pose[i]));
      std::printf("%d %016llx\n", source, bits(motion[12]));
    }
    sm.disableDeskew();
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "deskew_driver: %s\n", e.what());
    return 1;
  }
}
