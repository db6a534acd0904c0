/*
 * examples/odometry.c -- the smallest host program on top of the C-ABI (include/suma_hip.h):
 * SuMa++ odometry over a directory of KITTI velodyne scans, one pose per line on stdout
 * (KITTI devkit format: the upper 3x4 of the sensor pose, row-major).
 *
 *   cc -O2 -Iinclude examples/odometry.c -Lsemantic_suma_amd -lsuma_hip -Wl,-rpath,$PWD/semantic_suma_amd -o odometry
 *   ./odometry [--close-loops] [--deskew [--clockwise] [--t-ref X]] [--checkpoint FILE --checkpoint-every N]
 *              [--resume FILE] /data/kitti/sequences/00/velodyne 4541 [labels_dir]
 *
 * --close-loops: the reference's close-loops = true (config/default.xml:71).  The pipeline keeps a pose graph, verifies
 * loop closures and integrates the optimised trajectory while it runs; the poses are then printed once, at the end, from
 * the pose graph (SurfelMapping::getOptimizedPoses) instead of scan by scan from the odometry.
 *
 * --deskew: the scans are RAW sweeps of a moving sensor (KITTI's odometry scans are compensated already and need none of
 * this): every scan is motion compensated in front of the preprocessing, with the previous scan's increment as the motion
 * over one sweep (suma_pipeline_enable_deskew).  The point's azimuth gives its time; --clockwise for a sensor that turns
 * clockwise seen from above (Velodyne), --t-ref X for the instant of the sweep the pose refers to (default 0.5).  A
 * checkpoint holds none of this: give the options again with --resume.
 *
 * --checkpoint FILE --checkpoint-every N: after every N-th scan the whole session (suma_pipeline_checkpoint_save) is
 * written to FILE.tmp and renamed to FILE, so FILE is always a complete image.
 * --resume FILE: the pipeline is created from the image's parameters and loads it; the run starts at the image's
 * timestamp (the scan file of that number) and prints only the remaining poses, so the output of the first run followed
 * by the output of the resumed run is the output of one uninterrupted run.  Loop closing is on if the image says so;
 * with it, the resumed run prints the graph's poses from the image's timestamp on (the earlier ones may have moved).
 *
 * Scan files: <dir>/%06d.bin, N x 4 float32 (x, y, z, remission) as read by the reference's
 * KITTIReader (src/io/KITTIReader.cpp:140-167).  Optional SemanticKITTI labels: <labels_dir>/%06d.label,
 * N x uint32 (lower 16 bits = class id); without them the run is plain SuMa (labels 0, probabilities 0).
 * This mirrors what SurfelMapping::processScan is fed by the reference's visualizer (src/visualizer/visualizer.cpp)
 * minus RangeNet++ inference, which is outside the hot path this library replaces.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "suma_hip.h"

static size_t file_size(FILE* f) {
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  return n < 0 ? 0 : (size_t)n;
}

static void print_pose(const double* T) { /* column-major in, KITTI row-major 3 x 4 out */
  printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", T[0], T[4], T[8], T[12], T[1], T[5], T[9],
         T[13], T[2], T[6], T[10], T[14]);
}

/* the whole session into <file>.tmp, then renamed: a reader never sees half an image */
static int write_checkpoint(suma_pipeline* pipe, const char* file, void** buf, uint64_t* buf_cap) {
  uint64_t need = 0, written = 0;
  if (suma_pipeline_checkpoint_size(pipe, &need) != SUMA_OK) return -1;
  if (need > *buf_cap) {
    void* grown = realloc(*buf, (size_t)need);
    if (!grown) return -1;
    *buf = grown, *buf_cap = need;
  }
  if (suma_pipeline_checkpoint_save(pipe, *buf, *buf_cap, &written) != SUMA_OK) return -1;
  char tmp[4096];
  if (snprintf(tmp, sizeof(tmp), "%s.tmp", file) >= (int)sizeof(tmp)) return -2;
  FILE* f = fopen(tmp, "wb");
  if (!f) return -2;
  const int ok = fwrite(*buf, 1, (size_t)written, f) == (size_t)written;
  if (fclose(f) != 0 || !ok || rename(tmp, file) != 0) {
    remove(tmp);
    return -2;
  }
  return 0;
}

static void* read_file(const char* file, uint64_t* bytes) {
  FILE* f = fopen(file, "rb");
  if (!f) return NULL;
  const size_t n = file_size(f);
  void* b = malloc(n ? n : 1);
  if (b && fread(b, 1, n, f) != n) {
    free(b);
    b = NULL;
  }
  fclose(f);
  *bytes = n;
  return b;
}

int main(int argc, char** argv) {
  int close_loops = 0, checkpoint_every = 0, deskew = 0;
  suma_deskew_params dp;
  suma_deskew_params_default(&dp);
  const char *prog = argv[0], *checkpoint_file = NULL, *resume_file = NULL;
  while (argc > 1 && strncmp(argv[1], "--", 2) == 0) {
    int used = 1;
    if (strcmp(argv[1], "--close-loops") == 0) close_loops = 1;
    else if (strcmp(argv[1], "--deskew") == 0) deskew = 1;
    else if (strcmp(argv[1], "--clockwise") == 0) dp.clockwise = 1;
    else if (strcmp(argv[1], "--t-ref") == 0 && argc > 2) dp.t_ref = (float)atof(argv[2]), used = 2;
    else if (strcmp(argv[1], "--checkpoint") == 0 && argc > 2) checkpoint_file = argv[2], used = 2;
    else if (strcmp(argv[1], "--checkpoint-every") == 0 && argc > 2) checkpoint_every = atoi(argv[2]), used = 2;
    else if (strcmp(argv[1], "--resume") == 0 && argc > 2) resume_file = argv[2], used = 2;
    else break; /* an option this program does not know: the usage below */
    argc -= used, argv += used;
  }
  if (argc < 3 || (argc > 1 && strncmp(argv[1], "--", 2) == 0) || (checkpoint_file != NULL) != (checkpoint_every > 0)) {
    fprintf(stderr, "usage: %s [--close-loops] [--deskew [--clockwise] [--t-ref X]] [--checkpoint FILE --checkpoint-every N] [--resume FILE] <velodyne_dir> "
                    "<n_scans> [labels_dir]\n", prog);
    return 2;
  }
  const char* dir = argv[1];
  const int n_scans = atoi(argv[2]);
  const char* label_dir = argc > 3 ? argv[3] : NULL;

  suma_params p;
  suma_params_default(&p); /* config/default.xml of the reference; 64 x 900 images */
  p.data_width = p.model_width = 2048;

  void* image = NULL; /* the image to resume from; afterwards the buffer the checkpoints are saved into */
  uint64_t image_bytes = 0;
  struct suma_checkpoint_info info;
  memset(&info, 0, sizeof(info));
  if (resume_file) {
    image = read_file(resume_file, &image_bytes);
    if (!image) {
      fprintf(stderr, "cannot read %s\n", resume_file);
      return 1;
    }
    /* the pipeline an image loads into has the image's parameters */
    if (suma_checkpoint_info(image, image_bytes, &info) != SUMA_OK || suma_checkpoint_params(image, image_bytes, &p) != SUMA_OK) {
      fprintf(stderr, "%s: %s\n", resume_file, suma_last_error(NULL));
      free(image);
      return 1;
    }
  }

  suma_pipeline* pipe = NULL;
  if (suma_pipeline_create(&p, /*hip_device=*/0, &pipe) != SUMA_OK) {
    fprintf(stderr, "suma_pipeline_create: %s\n", suma_last_error(NULL));
    return 1;
  }

  int first_scan = 0;
  if (resume_file) { /* switches loop closing on or off as the image has it */
    if (suma_pipeline_checkpoint_load(pipe, image, image_bytes) != SUMA_OK) {
      fprintf(stderr, "%s: %s\n", resume_file, suma_last_error(suma_pipeline_ctx(pipe)));
      suma_pipeline_destroy(pipe);
      free(image);
      return 1;
    }
    first_scan = (int)info.timestamp;
    close_loops = info.has_loop != 0;
    fprintf(stderr, "resumed from %s at scan %d\n", resume_file, first_scan);
  } else if (close_loops) {
    suma_loop_params lp;
    suma_loop_params_default(&lp); /* the reference's thresholds (SurfelMapping.h:221-228) */
    if (suma_pipeline_enable_loop_closing(pipe, &lp) != SUMA_OK) {
      fprintf(stderr, "suma_pipeline_enable_loop_closing: %s\n", suma_last_error(suma_pipeline_ctx(pipe)));
      suma_pipeline_destroy(pipe);
      return 1;
    }
  }

  if (deskew && suma_pipeline_enable_deskew(pipe, &dp) != SUMA_OK) { /* after a load: the image holds no deskew state */
    fprintf(stderr, "suma_pipeline_enable_deskew: %s\n", suma_last_error(suma_pipeline_ctx(pipe)));
    suma_pipeline_destroy(pipe);
    free(image);
    return 1;
  }

  suma_float4* pts = NULL;
  float *labels = NULL, *probs = NULL;
  uint32_t* raw = NULL;
  size_t cap = 0;
  char path[4096];
  int status = 0;
  for (int k = first_scan; k < n_scans; ++k) {
    snprintf(path, sizeof(path), "%s/%06d.bin", dir, k);
    FILE* f = fopen(path, "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", path);
      break;
    }
    const size_t n = file_size(f) / (4 * sizeof(float));
    if (n > cap) {
      cap = n;
      pts = (suma_float4*)realloc(pts, cap * sizeof(suma_float4));
      labels = (float*)realloc(labels, cap * sizeof(float));
      probs = (float*)realloc(probs, cap * sizeof(float));
      raw = (uint32_t*)realloc(raw, cap * sizeof(uint32_t));
    }
    if (fread(pts, sizeof(suma_float4), n, f) != n) n == 0 ? (void)0 : (void)fprintf(stderr, "short read: %s\n", path);
    fclose(f);
    memset(labels, 0, n * sizeof(float));
    memset(probs, 0, n * sizeof(float));
    if (label_dir) {
      snprintf(path, sizeof(path), "%s/%06d.label", label_dir, k);
      FILE* g = fopen(path, "rb");
      if (g) {
        const size_t m = fread(raw, sizeof(uint32_t), n, g);
        fclose(g);
        for (size_t i = 0; i < m; ++i) {
          labels[i] = (float)(raw[i] & 0xffffu);
          probs[i] = 1.0f; /* ground-truth labels: full confidence */
        }
      }
    }
    /* fixed_iterations = 0: the stopping tests of LieGaussNewton decide (max iterations from the params) */
    const int r = suma_pipeline_process_scan(pipe, pts, labels, probs, (uint32_t)n, 0);
    if (r != SUMA_OK) {
      fprintf(stderr, "scan %d: %s\n", k, suma_last_error(suma_pipeline_ctx(pipe)));
      break;
    }
    if (close_loops) {
      suma_loop_status ls;
      if (suma_pipeline_loop_status(pipe, &ls) == SUMA_OK && (ls.edges_added || ls.integrated))
        fprintf(stderr, "scan %d: %u loop edge(s) added%s\n", k, ls.edges_added,
                ls.integrated ? ", optimised trajectory integrated" : "");
    } else {
      double T[16]; /* column-major */
      suma_pipeline_pose(pipe, T);
      print_pose(T);
    }
    if (checkpoint_file && (k + 1) % checkpoint_every == 0) {
      const int w = write_checkpoint(pipe, checkpoint_file, &image, &image_bytes);
      if (w != 0) {
        fprintf(stderr, "checkpoint after scan %d: %s\n", k, w == -1 ? suma_last_error(suma_pipeline_ctx(pipe)) : "cannot write the file");
        status = 1;
        break;
      }
    }
  }
  if (close_loops) { /* the pose graph's poses: optimised up to the last integration, odometry behind it */
    const suma_posegraph* g = suma_pipeline_posegraph(pipe);
    const int32_t n = suma_posegraph_size(g);
    for (int32_t k = first_scan; k < n; ++k) {
      double T[16];
      if (suma_posegraph_pose(g, k, T) == SUMA_OK) print_pose(T);
    }
  }
  fprintf(stderr, "frame-to-frame fallbacks: %u\n", suma_pipeline_track_loss(pipe));
  free(pts);
  free(labels);
  free(probs);
  free(raw);
  free(image);
  suma_pipeline_destroy(pipe);
  return status;
}
