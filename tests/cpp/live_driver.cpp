// Drives the live obstacle layer of suma_hip::Localizer (include/suma_adapter.hpp) the way a C++ host would:
//   live_driver <frame.bin> <flags.bin> <pose.bin> <cells.bin> <width> <height> <grid_width> <grid_height> <cell_size>
//               <origin_x> <origin_y> <step_height> <clearance> <hold_scans> <min_hits> <carve_range> <carve_margin>
// frame.bin: the vertex, normal and semantic maps of one data-sized frame, height x width x 4 floats each; flags.bin: one
// byte a texel; pose.bin: the sensor pose, column-major double[16]; cells.bin: grid_width * grid_height suma_grid_cell.
// Switches novelty and the layer on, updates it with the frame as scans 0 and 1, composes and prints
//   the ten counts of the second update,
//   "<n_live> <n_pending> <n_expired> <n_carved>",
//   "<FNV-1a 64 of the composed cells' bytes, hex> <FNV-1a 64 of the mask's bytes, hex>".
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
  if (argc != 18) {
    std::fprintf(stderr, "usage: %s frame.bin flags.bin pose.bin cells.bin width height grid_width grid_height cell_size "
                         "origin_x origin_y step_height clearance hold_scans min_hits carve_range carve_margin\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> fb = slurp(argv[1]), gb = slurp(argv[2]), pb = slurp(argv[3]), cb = slurp(argv[4]);
    if (pb.size() != 16 * sizeof(double)) throw std::runtime_error("pose.bin: 16 doubles expected");
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[5]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[6]);
    const size_t texels = (size_t)p.data_width * p.data_height;
    if (fb.size() != 3 * texels * sizeof(suma_float4)) throw std::runtime_error("frame.bin: three maps expected");
    if (gb.size() != texels) throw std::runtime_error("flags.bin: one byte a texel expected");
    suma_grid_params gp;
    suma_grid_params_default(&gp);
    gp.width = (uint32_t)std::atoi(argv[7]), gp.height = (uint32_t)std::atoi(argv[8]);
    gp.cell_size = (float)std::atof(argv[9]);
    gp.origin_x = (float)std::atof(argv[10]), gp.origin_y = (float)std::atof(argv[11]);
    gp.step_height = (float)std::atof(argv[12]), gp.clearance = (float)std::atof(argv[13]);
    const size_t n_cells = (size_t)gp.width * gp.height;
    if (cb.size() != n_cells * sizeof(suma_grid_cell)) throw std::runtime_error("cells.bin: one cell a raster cell expected");
    const std::vector<suma_grid_cell> cells((const suma_grid_cell*)cb.data(), (const suma_grid_cell*)cb.data() + n_cells);
    suma_live_params lp;
    suma_live_params_default(&lp);
    lp.hold_scans = (uint32_t)std::atoi(argv[14]), lp.min_hits = (uint32_t)std::atoi(argv[15]);
    lp.carve_range = (float)std::atof(argv[16]), lp.carve_margin = (float)std::atof(argv[17]);
    suma_hip::Localizer loc(p);
    suma_novel_params np;
    suma_novel_params_default(&np);
    np.max_candidates = 1024;
    loc.enableNovelty(&np);
    loc.enableLiveGrid(gp, cells, &lp);
    bool updated = true;
    loc.liveCounts(&updated);
    if (updated) throw std::runtime_error("liveCounts() reports an update before the first one");
    suma_frame* f = nullptr;
    suma_hip::check(loc.ctx(), suma_frame_create(loc.ctx(), p.data_width, p.data_height, &f), "suma_frame_create");
    const suma_float4* maps = (const suma_float4*)fb.data();
    for (int which = 0; which < 3; ++which)
      suma_hip::check(loc.ctx(), suma_frame_upload(loc.ctx(), f, which, maps + which * texels), "suma_frame_upload");
    loc.liveUpdateFlags(f, (const double*)pb.data(), (const uint8_t*)gb.data(), 0u);
    const suma_live_counts c = loc.liveUpdateFlags(f, (const double*)pb.data(), (const uint8_t*)gb.data(), 1u);
    const suma_live_counts again = loc.liveCounts(&updated);
    if (!updated || again.n_hit_cells != c.n_hit_cells) throw std::runtime_error("liveCounts() disagrees");
    std::printf("%u %u %u %u %u %u %u %u %u %u\n", c.n_texels, c.n_members, c.n_outside, c.n_no_ground, c.n_low, c.n_high,
                c.n_hit_texels, c.n_hit_cells, c.n_rays, c.n_cleared);
    std::vector<uint8_t> mask;
    suma_live_stats st;
    const std::vector<suma_grid_cell> out = loc.liveCells(&mask, &st);
    std::printf("%u %u %u %u\n", st.n_live, st.n_pending, st.n_expired, st.n_carved);
    std::printf("%016llx %016llx\n", fnv(out.data(), out.size() * sizeof(suma_grid_cell)), fnv(mask.data(), mask.size()));
    suma_frame_destroy(f);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "live_driver: %s\n", e.what());
    return 1;
  }
}
