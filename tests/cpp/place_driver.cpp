// Drives suma_hip::PlaceIndex and suma_hip::Localizer::relocalize (include/suma_adapter.hpp) the way a C++ host would:
//   place_driver <map.bin> <cells.bin> <ids.bin> <poses.bin> <scan base> <width> <height> <extent> <dimension>
//                <max_range> <k>
// map.bin: 48-byte suma_world_surfel records; cells.bin: n x 60 x 20 floats; ids.bin: n uint32; poses.bin: n column-major
// double[16]; <scan base>.bin / .label / .prob: the query scan.  Prints
//   "<n matches>", then per match "<index> <id> <distance bits, hex> <shift> <yaw bits, hex>"   (queryFrame, k best)
//   "<index> <id> <distance bits> <shift> <index with id 4242 left out> <size>"   (the best match once the query's own
//                                                frame was added with id 4242)
//   "<found> <n_tried> <winner>", then per candidate "<index> <tracked> <16 pose doubles as hex bit patterns>"
//   "<16 pose doubles of the result>"            (only when found)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>

#include "suma_adapter.hpp"

static std::vector<char> slurp(const std::string& path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static unsigned bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, 4);
  return u;
}

static void print_pose(const double* T) {
  for (int i = 0; i < 16; ++i) {
    unsigned long long u;
    std::memcpy(&u, &T[i], 8);
    std::printf(" %016llx", u);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 12) {
    std::fprintf(stderr, "usage: %s map.bin cells.bin ids.bin poses.bin scan_base width height extent dimension max_range k\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> mb = slurp(argv[1]), cb = slurp(argv[2]), ib = slurp(argv[3]), pb = slurp(argv[4]);
    suma_params p;
    suma_params_default(&p);
    p.data_width = p.model_width = (uint32_t)std::atoi(argv[6]);
    p.data_height = p.model_height = (uint32_t)std::atoi(argv[7]);
    p.submap_extent = (float)std::atof(argv[8]);
    p.submap_dimension = std::atoi(argv[9]);
    suma_place_params pp;
    suma_place_params_default(&pp);
    pp.max_range = (float)std::atof(argv[10]);
    const uint32_t k = (uint32_t)std::atoi(argv[11]);

    suma_hip::PlaceIndex index(&pp);
    const uint32_t n_entries = (uint32_t)(ib.size() / sizeof(uint32_t));
    if (cb.size() != (size_t)n_entries * pp.sectors * pp.rings * sizeof(float) || pb.size() != (size_t)n_entries * 16 * sizeof(double))
      throw std::runtime_error("cells / ids / poses differ in length");
    index.upload(std::vector<float>((const float*)cb.data(), (const float*)(cb.data() + cb.size())),
                 std::vector<uint32_t>((const uint32_t*)ib.data(), (const uint32_t*)(ib.data() + ib.size())));
    const std::vector<double> poses((const double*)pb.data(), (const double*)(pb.data() + pb.size()));

    suma_hip::Localizer loc(p);
    const suma_world_surfel* recs = (const suma_world_surfel*)mb.data();
    loc.setMap(std::vector<suma_world_surfel>(recs, recs + mb.size() / sizeof(suma_world_surfel)));

    const std::string base = argv[5];
    const std::vector<char> pts = slurp(base + ".bin"), lab = slurp(base + ".label"), prob = slurp(base + ".prob");
    const uint32_t n = (uint32_t)(pts.size() / sizeof(suma_float4));
    if (lab.size() != n * sizeof(float) || prob.size() != n * sizeof(float)) throw std::runtime_error("scan files differ in length");

    // the query's frame on the localiser's ctx, at the stamp a localiser preprocesses with
    suma_frame* frame = nullptr;
    suma_hip::check(loc.ctx(), suma_frame_create(loc.ctx(), p.data_width, p.data_height, &frame), "suma_frame_create");
    suma_hip::check(loc.ctx(),
                    suma_preprocess(loc.ctx(), (const suma_float4*)pts.data(), (const float*)lab.data(),
                                    (const float*)prob.data(), n, (uint32_t)p.active_timestamps + 10u, frame),
                    "suma_preprocess");
    const std::vector<suma_place_match> m = index.queryFrame(loc.ctx(), frame, k);
    std::printf("%zu\n", m.size());
    for (const suma_place_match& x : m) std::printf("%u %u %08x %d %08x\n", x.index, x.id, bits(x.distance), x.shift, bits(x.yaw));

    std::unique_ptr<suma_relocalize_result> res(new suma_relocalize_result);
    loc.relocalize(index, poses, (const suma_float4*)pts.data(), (const float*)lab.data(), (const float*)prob.data(), n, k,
                   res.get());

    // the query's own frame as one more entry: it is its own best match, and the window leaves it out again
    index.addFrame(loc.ctx(), frame, 4242u);
    const std::vector<suma_place_match> own = index.queryFrame(loc.ctx(), frame, 1);
    const std::vector<suma_place_match> without = index.queryFrame(loc.ctx(), frame, 1, 4242u, 4242u);
    std::printf("%u %u %08x %d %u %u\n", own.at(0).index, own.at(0).id, bits(own.at(0).distance), own.at(0).shift,
                without.at(0).index, index.size());
    suma_frame_destroy(frame);

    std::printf("%d %u %d\n", res->found, res->n_tried, res->winner);
    for (uint32_t c = 0; c < res->n_tried; ++c) {
      std::printf("%u %d", res->candidates[c].match.index, res->candidates[c].result.tracked);
      print_pose(res->candidates[c].result.pose);
    }
    if (res->found) print_pose(res->result.pose);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "place_driver: %s\n", e.what());
    return 1;
  }
}
