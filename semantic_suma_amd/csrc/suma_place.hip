/*
 * suma_place.hip -- the place index (include/suma_hip.h, suma_place_*): host code around k_place.hip, which states the
 * specification.  The database is one DevBuf of entries (S*R cells then S norms each) and one of ids; it grows by the
 * library's one rule (the streams that may still use the block are drained, then a block of n + n/4 + 32 is made), with
 * the entries copied over.  Work is enqueued on the stream of the ctx passed in, or on the index's own stream; an event
 * recorded behind every piece of work orders the index's work across those streams.
 */
#include <string.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "suma_internal.h"

struct suma_place_index {
  suma_place_params p;
  PlaceArgs args;
  int device = 0;
  uint32_t n = 0, capacity = 0, stride = 0; /* entries, room for entries, floats an entry */
  DevBuf<float> db;
  DevBuf<uint32_t> ids;
  DevBuf<float> q;        /* the query's descriptor */
  DevBuf<float> dist;     /* per-entry results, capacity each */
  DevBuf<int32_t> shift;
  DevBuf<suma_place_match> d_matches; /* SUMA_PLACE_MAX_MATCHES */
  DevBuf<uint32_t> d_count;
  hipStream_t own = nullptr;
  hipEvent_t last = nullptr; /* behind the last work enqueued, on last_stream */
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  std::string err;
};

namespace {

int pfail(suma_place_index* idx, suma_ctx* c, int code, const std::string& msg) {
  idx->err = msg;
  if (c) c->err = msg;
  return code;
}

#define PLACE_TRY(idx, c, expr)                                                                  \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess)                                                                       \
      return pfail(idx, c, SUMA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));    \
  } while (0)

/* work on st comes behind whatever the index enqueued last, on whichever stream */
int enter(suma_place_index* idx, suma_ctx* c, hipStream_t st) {
  if (idx->have_last && idx->last_stream != st) PLACE_TRY(idx, c, hipStreamWaitEvent(st, idx->last, 0));
  return SUMA_OK;
}
int leave(suma_place_index* idx, suma_ctx* c, hipStream_t st) {
  PLACE_TRY(idx, c, hipEventRecord(idx->last, st));
  idx->last_stream = st;
  idx->have_last = true;
  return SUMA_OK;
}

/* room for n entries; the entries there are kept.  Blocking when it grows. */
int reserve(suma_place_index* idx, suma_ctx* c, uint32_t n, hipStream_t st) {
  if (n <= idx->capacity) return SUMA_OK;
  if (idx->have_last) PLACE_TRY(idx, c, hipEventSynchronize(idx->last)); /* nothing uses the old blocks any more */
  const size_t cap = (size_t)n + n / 4 + 32;
  if (cap > 0x7fffffffu) return pfail(idx, c, SUMA_ERR_CAPACITY, "suma_place_index: more than 2^31 entries");
  DevBuf<float> db, dist;
  DevBuf<uint32_t> ids;
  DevBuf<int32_t> shift;
  PLACE_TRY(idx, c, db.alloc(cap * idx->stride));
  PLACE_TRY(idx, c, ids.alloc(cap));
  PLACE_TRY(idx, c, dist.alloc(cap));
  PLACE_TRY(idx, c, shift.alloc(cap));
  if (idx->n) {
    PLACE_TRY(idx, c, hipMemcpyAsync(db, idx->db, (size_t)idx->n * idx->stride * sizeof(float), hipMemcpyDeviceToDevice, st));
    PLACE_TRY(idx, c, hipMemcpyAsync(ids, idx->ids, (size_t)idx->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    PLACE_TRY(idx, c, hipStreamSynchronize(st));
  }
  idx->db = std::move(db), idx->ids = std::move(ids), idx->dist = std::move(dist), idx->shift = std::move(shift);
  idx->capacity = (uint32_t)cap;
  return SUMA_OK;
}

int check_ctx(suma_place_index* idx, suma_ctx* c, const suma_frame* f, const char* who) {
  if (!c) return pfail(idx, nullptr, SUMA_ERR_INVALID, std::string(who) + ": NULL ctx");
  if (c->device != idx->device)
    return pfail(idx, c, SUMA_ERR_INVALID, std::string(who) + ": the ctx is on device " + std::to_string(c->device) +
                                           ", the index on device " + std::to_string(idx->device));
  if (!f) return pfail(idx, c, SUMA_ERR_INVALID, std::string(who) + ": NULL frame");
  return SUMA_OK;
}

/* frame f's descriptor into `entry`, on the ctx stream behind the work that made the frame */
int describe(suma_place_index* idx, suma_ctx* c, const suma_frame* f, float* entry) {
  if (c->gate_pending) PLACE_TRY(idx, c, flush_gate(c));
  const_cast<suma_frame*>(f)->last_access = ++c->enq_seq;
  ProfScope ps(c, "place_describe", 32.0 * f->width * f->height);
  PLACE_TRY(idx, c, launch_kp_describe(c->stream, f, idx->args, entry));
  return SUMA_OK;
}

void fill_yaw(const suma_place_index* idx, suma_place_match* m, uint32_t n) {
  const int32_t S = (int32_t)idx->p.sectors;
  const float D = (2.0f * SUMA_PI_F) / (float)S;
  for (uint32_t k = 0; k < n; ++k)
    m[k].yaw = m[k].shift <= S / 2 ? -(float)m[k].shift * D : (float)(S - m[k].shift) * D;
}

/* a profiling scope where there is a ctx to report to */
struct Scope {
  suma_ctx* c;
  int tok;
  Scope(suma_ctx* c_, const char* name, double bytes)
      : c(c_), tok(c_ && ProfScope::wanted(c_, name) ? prof_begin(c_, name, bytes, 1) : -1) {}
  ~Scope() {
    if (tok >= 0) prof_end(c, tok);
  }
};

/* idx->q holds the query: every entry's least distance and shift into idx->dist / idx->shift */
int scored(suma_place_index* idx, suma_ctx* c, hipStream_t st) {
  Scope ps(c, "place_search", 4.0 * idx->stride * idx->n);
  PLACE_TRY(idx, c, launch_kp_search(st, idx->db, idx->n, idx->q, idx->p.sectors, idx->p.rings, idx->dist, idx->shift));
  return SUMA_OK;
}

/* idx->q holds the query: search, top-k, read back.  Blocking. */
int search(suma_place_index* idx, suma_ctx* c, hipStream_t st, uint32_t lo, uint32_t hi, uint32_t k,
           suma_place_match* matches, uint32_t* n_out) {
  uint32_t count = 0;
  if (idx->n) {
    int r = scored(idx, c, st);
    if (r) return r;
    {
      Scope ps(c, "place_topk", 8.0 * idx->n * k);
      PLACE_TRY(idx, c, launch_kp_topk(st, idx->dist, idx->shift, idx->ids, idx->n, lo, hi, k, idx->d_matches, idx->d_count));
    }
    PLACE_TRY(idx, c, hipMemcpyAsync(&count, idx->d_count, sizeof(count), hipMemcpyDeviceToHost, st));
    PLACE_TRY(idx, c, hipMemcpyAsync(matches, idx->d_matches, k * sizeof(suma_place_match), hipMemcpyDeviceToHost, st));
  }
  int r = leave(idx, c, st);
  if (r) return r;
  PLACE_TRY(idx, c, hipStreamSynchronize(st));
  if (count > k) return pfail(idx, c, SUMA_ERR_HIP, "suma_place_index: inconsistent match count (internal error)");
  fill_yaw(idx, matches, count);
  *n_out = count;
  return SUMA_OK;
}

int check_query(suma_place_index* idx, suma_ctx* c, uint32_t k, const suma_place_match* matches, const uint32_t* n_out,
                const char* who) {
  if (k < 1 || k > SUMA_PLACE_MAX_MATCHES)
    return pfail(idx, c, SUMA_ERR_INVALID, std::string(who) + ": k must be 1 .. 32");
  if (!matches || !n_out) return pfail(idx, c, SUMA_ERR_INVALID, std::string(who) + ": NULL output");
  return SUMA_OK;
}

}  // namespace

void place_hypothesis(const double T_entry[16], float yaw, double out[16]) {
  double Rz[16];
  mat4_eye(Rz);
  const double cy = sdm_cos_d((double)yaw), sy = sdm_sin_d((double)yaw);
  Rz[0] = cy, Rz[1] = sy, Rz[4] = -sy, Rz[5] = cy;
  mat4_mul(T_entry, Rz, out);
}

extern "C" void suma_place_params_default(suma_place_params* pp) {
  if (!pp) return;
  pp->rings = 20;
  pp->sectors = 60;
  pp->max_range = 80.0f;
  pp->height_offset = 2.0f;
  memset(pp->keep_label, 1, sizeof(pp->keep_label));
}

extern "C" int suma_place_index_create(const suma_place_params* params, int hip_device, uint32_t capacity,
                                       suma_place_index** out) {
  if (!out) return SUMA_ERR_INVALID;
  *out = nullptr;
  suma_place_params p;
  suma_place_params_default(&p);
  if (params) p = *params;
  if (p.rings < 1 || p.rings > SUMA_PLACE_MAX_DIM)
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_place_index_create: rings must be 1 .. 64");
  if (p.sectors < 1 || p.sectors > SUMA_PLACE_MAX_DIM)
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_place_index_create: sectors must be 1 .. 64 (one lane per shift)");
  if (!(p.max_range > 0.0f) || !std::isfinite(p.max_range))
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_place_index_create: max_range must be finite and > 0");
  if (!std::isfinite(p.height_offset))
    return fail_without_ctx(SUMA_ERR_INVALID, "suma_place_index_create: height_offset must be finite");
  suma_place_index* idx = new (std::nothrow) suma_place_index();
  if (!idx) return fail_without_ctx(SUMA_ERR_NOMEM, "out of host memory");
  idx->p = p;
  idx->device = hip_device;
  idx->stride = p.sectors * p.rings + p.sectors;
  PlaceArgs& a = idx->args;
  memset(&a, 0, sizeof(a));
  a.R = p.rings, a.S = p.sectors;
  a.max_range = p.max_range, a.height_offset = p.height_offset;
  a.ring_scale = (float)p.rings / p.max_range;
  a.sector_scale = (float)p.sectors / (2.0f * SUMA_PI_F);
  for (uint32_t l = 0; l < SUMA_DRAW_COLORS; ++l)
    if (p.keep_label[l]) a.keep[l >> 5] |= 1u << (l & 31u);
  hipError_t e = hipSetDevice(hip_device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&idx->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&idx->last, hipEventDisableTiming);
  if (e == hipSuccess) e = idx->q.alloc(idx->stride);
  if (e == hipSuccess) e = idx->d_matches.alloc(SUMA_PLACE_MAX_MATCHES);
  if (e == hipSuccess) e = idx->d_count.alloc(1);
  int r = SUMA_OK;
  if (e != hipSuccess) {
    r = fail_without_ctx(SUMA_ERR_HIP, std::string("suma_place_index_create: ") + hipGetErrorString(e));
  } else if (capacity && (r = reserve(idx, nullptr, capacity, idx->own)) != SUMA_OK) {
    fail_without_ctx(r, "suma_place_index_create: " + idx->err);
  }
  if (r) {
    suma_place_index_destroy(idx);
    return r;
  }
  *out = idx;
  return SUMA_OK;
}

extern "C" void suma_place_index_destroy(suma_place_index* idx) {
  if (!idx) return;
  if (idx->have_last) hipEventSynchronize(idx->last);
  if (idx->own) hipStreamSynchronize(idx->own), hipStreamDestroy(idx->own);
  if (idx->last) hipEventDestroy(idx->last);
  delete idx;
}

extern "C" int suma_place_index_clear(suma_place_index* idx) {
  if (!idx) return SUMA_ERR_INVALID;
  idx->n = 0; /* the index orders its own work: a slot is rewritten behind whatever read it */
  return SUMA_OK;
}

extern "C" uint32_t suma_place_index_size(const suma_place_index* idx) { return idx ? idx->n : 0u; }

extern "C" const char* suma_place_index_last_error(const suma_place_index* idx) {
  return idx ? idx->err.c_str() : suma_last_error(nullptr);
}

extern "C" int suma_place_index_add_frame(suma_place_index* idx, suma_ctx* c, const suma_frame* frame, uint32_t id) {
  if (!idx) return SUMA_ERR_INVALID;
  int r = check_ctx(idx, c, frame, "suma_place_index_add_frame");
  if (r) return r;
  if ((r = reserve(idx, c, idx->n + 1u, c->stream)) != SUMA_OK) return r;
  if ((r = enter(idx, c, c->stream)) != SUMA_OK) return r;
  if ((r = describe(idx, c, frame, idx->db + (size_t)idx->n * idx->stride)) != SUMA_OK) return r;
  /* a pageable source: the copy has left `id` when the call returns */
  PLACE_TRY(idx, c, hipMemcpyAsync(idx->ids + idx->n, &id, sizeof(id), hipMemcpyHostToDevice, c->stream));
  if ((r = leave(idx, c, c->stream)) != SUMA_OK) return r;
  idx->n += 1u;
  return SUMA_OK;
}

extern "C" int suma_place_index_download(suma_place_index* idx, uint32_t first, uint32_t n, float* cells, float* norms,
                                         uint32_t* ids) {
  if (!idx) return SUMA_ERR_INVALID;
  if ((uint64_t)first + n > idx->n)
    return pfail(idx, nullptr, SUMA_ERR_INVALID, "suma_place_index_download: entries beyond the index's size");
  if (!n) return SUMA_OK;
  hipStream_t st = idx->own;
  int r = enter(idx, nullptr, st);
  if (r) return r;
  const size_t SR = (size_t)idx->p.sectors * idx->p.rings, S = idx->p.sectors, pitch = idx->stride * sizeof(float);
  const float* src = idx->db + (size_t)first * idx->stride;
  if (cells)
    PLACE_TRY(idx, nullptr, hipMemcpy2DAsync(cells, SR * sizeof(float), src, pitch, SR * sizeof(float), n, hipMemcpyDeviceToHost, st));
  if (norms)
    PLACE_TRY(idx, nullptr, hipMemcpy2DAsync(norms, S * sizeof(float), src + SR, pitch, S * sizeof(float), n, hipMemcpyDeviceToHost, st));
  if (ids) PLACE_TRY(idx, nullptr, hipMemcpyAsync(ids, idx->ids + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if ((r = leave(idx, nullptr, st)) != SUMA_OK) return r;
  PLACE_TRY(idx, nullptr, hipStreamSynchronize(st));
  return SUMA_OK;
}

static int check_cells(suma_place_index* idx, const float* cells, size_t count, const char* who) {
  for (size_t k = 0; k < count; ++k)
    if (!(cells[k] == 0.0f || (cells[k] > 0.0f && cells[k] <= 1000.0f)))
      return pfail(idx, nullptr, SUMA_ERR_INVALID, std::string(who) + ": cell " + std::to_string(k) + " is neither 0 nor in (0, 1000]");
  return SUMA_OK;
}

extern "C" int suma_place_index_upload(suma_place_index* idx, const float* cells, const uint32_t* ids, uint32_t n) {
  if (!idx) return SUMA_ERR_INVALID;
  if (!n) return SUMA_OK;
  if (!cells || !ids) return pfail(idx, nullptr, SUMA_ERR_INVALID, "suma_place_index_upload: NULL argument with n > 0");
  if ((uint64_t)idx->n + n > 0x7fffffffu) return pfail(idx, nullptr, SUMA_ERR_CAPACITY, "suma_place_index_upload: more than 2^31 entries");
  const size_t SR = (size_t)idx->p.sectors * idx->p.rings, pitch = idx->stride * sizeof(float);
  int r = check_cells(idx, cells, SR * n, "suma_place_index_upload");
  if (r) return r;
  hipStream_t st = idx->own;
  if ((r = reserve(idx, nullptr, idx->n + n, st)) != SUMA_OK) return r;
  if ((r = enter(idx, nullptr, st)) != SUMA_OK) return r;
  float* dst = idx->db + (size_t)idx->n * idx->stride;
  PLACE_TRY(idx, nullptr, hipMemcpy2DAsync(dst, pitch, cells, SR * sizeof(float), SR * sizeof(float), n, hipMemcpyHostToDevice, st));
  PLACE_TRY(idx, nullptr, hipMemcpyAsync(idx->ids + idx->n, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  PLACE_TRY(idx, nullptr, launch_kp_norms(st, dst, n, idx->p.sectors, idx->p.rings));
  if ((r = leave(idx, nullptr, st)) != SUMA_OK) return r;
  PLACE_TRY(idx, nullptr, hipStreamSynchronize(st));
  idx->n += n;
  return SUMA_OK;
}

extern "C" int suma_place_index_query_frame(suma_place_index* idx, suma_ctx* c, const suma_frame* frame, uint32_t exclude_lo,
                                            uint32_t exclude_hi, uint32_t k, suma_place_match* matches, uint32_t* n_out) {
  if (!idx) return SUMA_ERR_INVALID;
  int r = check_ctx(idx, c, frame, "suma_place_index_query_frame");
  if (r) return r;
  if ((r = check_query(idx, c, k, matches, n_out, "suma_place_index_query_frame")) != SUMA_OK) return r;
  if ((r = enter(idx, c, c->stream)) != SUMA_OK) return r;
  if ((r = describe(idx, c, frame, idx->q)) != SUMA_OK) return r;
  return search(idx, c, c->stream, exclude_lo, exclude_hi, k, matches, n_out);
}

extern "C" int suma_place_index_query(suma_place_index* idx, const float* cells_host, uint32_t exclude_lo,
                                      uint32_t exclude_hi, uint32_t k, suma_place_match* matches, uint32_t* n_out) {
  if (!idx) return SUMA_ERR_INVALID;
  if (!cells_host) return pfail(idx, nullptr, SUMA_ERR_INVALID, "suma_place_index_query: NULL cells");
  int r = check_query(idx, nullptr, k, matches, n_out, "suma_place_index_query");
  if (r) return r;
  const size_t SR = (size_t)idx->p.sectors * idx->p.rings;
  if ((r = check_cells(idx, cells_host, SR, "suma_place_index_query")) != SUMA_OK) return r;
  hipStream_t st = idx->own;
  if ((r = enter(idx, nullptr, st)) != SUMA_OK) return r;
  PLACE_TRY(idx, nullptr, hipMemcpyAsync(idx->q, cells_host, SR * sizeof(float), hipMemcpyHostToDevice, st));
  PLACE_TRY(idx, nullptr, launch_kp_norms(st, idx->q, 1u, idx->p.sectors, idx->p.rings));
  return search(idx, nullptr, st, exclude_lo, exclude_hi, k, matches, n_out);
}

extern "C" int suma_place_index_query_all(suma_place_index* idx, suma_ctx* c, const suma_frame* frame, float* dist,
                                          int32_t* shift) {
  if (!idx) return SUMA_ERR_INVALID;
  int r = check_ctx(idx, c, frame, "suma_place_index_query_all");
  if (r) return r;
  if (idx->n && (!dist || !shift)) return pfail(idx, c, SUMA_ERR_INVALID, "suma_place_index_query_all: NULL output");
  hipStream_t st = c->stream;
  if ((r = enter(idx, c, st)) != SUMA_OK) return r;
  if ((r = describe(idx, c, frame, idx->q)) != SUMA_OK) return r;
  if (idx->n) {
    if ((r = scored(idx, c, st)) != SUMA_OK) return r;
    PLACE_TRY(idx, c, hipMemcpyAsync(dist, idx->dist, idx->n * sizeof(float), hipMemcpyDeviceToHost, st));
    PLACE_TRY(idx, c, hipMemcpyAsync(shift, idx->shift, idx->n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  if ((r = leave(idx, c, st)) != SUMA_OK) return r;
  PLACE_TRY(idx, c, hipStreamSynchronize(st));
  return SUMA_OK;
}
