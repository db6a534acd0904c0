/*
 * track_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_tracks.hip restated on the host, one object,
 * one detection and one slot after the other: the join by a flood fill from each unvisited object in ascending index
 * order (the library unites by atomics), the association round by round with two plain loops a round (the library has
 * one workgroup and LDS atomics), the update, the births and the counts.  Compiled by the tests with
 * gcc -O2 -ffp-contract=off; the library's tracks, raw state, per-object ids and counts must equal it byte for byte.
 * It shares no code with the library; the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  uint32_t root, n_texels, label;
  float prob;
  uint32_t n_dynamic;
  float min[3], max[3], centroid[3];
  float r_min;
  uint32_t scan_id;
} tobject_t;

typedef struct {
  float join_dist, gate_base, gate_speed, alpha, beta;
  uint32_t confirm_hits, max_missed, max_tracks, max_rounds;
} tparams_t;

typedef struct {
  uint32_t id, slot, state, label, n_texels, n_dynamic, n_objects, hits, missed, first_stamp, last_matched;
  float position[3], velocity[3], origin[3], min[3], max[3];
  float r_min;
  uint32_t detection;
} ttrack_t;

typedef struct {
  uint32_t n_objects, n_detections, n_joined, n_tracks_before, n_matched, n_missed, n_expired, n_born, n_dropped,
      n_confirmed, n_unresolved, rounds;
} tcounts_t;

typedef struct {
  uint32_t label, n_objects, n_texels, n_dynamic;
  float min[3], max[3], centroid[3], r_min;
} tdet_t;

#define T_NONE 0xffffffffu

size_t track_shim_sizeof_object(void) { return sizeof(tobject_t); }
size_t track_shim_sizeof_params(void) { return sizeof(tparams_t); }
size_t track_shim_sizeof_track(void) { return sizeof(ttrack_t); }
size_t track_shim_sizeof_counts(void) { return sizeof(tcounts_t); }

static float fmax_(float a, float b) { return (a < b) ? b : a; }
static float fclampf(float x, float lo, float hi) {
  const float t = (x < lo) ? lo : x;
  return (t > hi) ? hi : t;
}
static float len3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }
static uint32_t bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
/* the order of the joined box and of r_min: the float's bits as an integer of the same order, -0 below +0 */
static uint32_t ordered(float f) {
  const uint32_t b = bits(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static int box_finite(const tobject_t* o) {
  for (int a = 0; a < 3; ++a)
    if (!isfinite(o->min[a]) || !isfinite(o->max[a])) return 0;
  return 1;
}
static int joined(const tobject_t* a, const tobject_t* b, float join_dist) {
  if (a->label != b->label || !box_finite(a) || !box_finite(b)) return 0;
  float g[3];
  for (int k = 0; k < 3; ++k) g[k] = fmax_(fmax_(0.0f, a->min[k] - b->max[k]), b->min[k] - a->max[k]);
  return len3(g[0], g[1], g[2]) <= join_dist;
}

/* step 1: obj_det[i] = the detection of object i; det: room for n records; returns the number of detections */
uint32_t track_shim_join(const tobject_t* obj, uint32_t n, float join_dist, tdet_t* det, uint32_t* obj_det) {
  uint32_t* stack = (uint32_t*)malloc(((size_t)n + 1) * sizeof(uint32_t));
  uint32_t D = 0;
  for (uint32_t i = 0; i < n; ++i) obj_det[i] = T_NONE;
  for (uint32_t first = 0; first < n; ++first) {
    if (obj_det[first] != T_NONE) continue;
    tdet_t* d = &det[D];
    memset(d, 0, sizeof(*d));
    uint64_t n_tex = 0, n_dyn = 0, W = 0;
    int64_t S[3] = {0, 0, 0};
    uint32_t top = 0, members = 0;
    stack[top++] = first;
    obj_det[first] = D;
    while (top) {
      const uint32_t i = stack[--top];
      const tobject_t* o = &obj[i];
      if (!(join_dist < 0.0f))
        for (uint32_t j = 0; j < n; ++j)
          if (obj_det[j] == T_NONE && joined(i < j ? o : &obj[j], i < j ? &obj[j] : o, join_dist)) {
            obj_det[j] = D;
            stack[top++] = j;
          }
      const uint32_t w = o->n_texels < 1u ? 1u : (o->n_texels > (1u << 22) ? (1u << 22) : o->n_texels);
      for (int a = 0; a < 3; ++a) {
        if (!members || ordered(o->min[a]) < ordered(d->min[a])) d->min[a] = o->min[a];
        if (!members || ordered(o->max[a]) > ordered(d->max[a])) d->max[a] = o->max[a];
        float q = fclampf(o->centroid[a] * 1024.0f, -16777216.0f, 16777216.0f);
        if (q != q) q = 0.0f;
        S[a] += (int64_t)w * (int64_t)llrintf(q);
      }
      if (!members || ordered(o->r_min) < ordered(d->r_min)) d->r_min = o->r_min;
      n_tex += o->n_texels, n_dyn += o->n_dynamic, W += w;
      members += 1;
    }
    d->label = obj[first].label;
    d->n_objects = members;
    d->n_texels = n_tex > 0xffffffffull ? 0xffffffffu : (uint32_t)n_tex;
    d->n_dynamic = n_dyn > 0xffffffffull ? 0xffffffffu : (uint32_t)n_dyn;
    for (int a = 0; a < 3; ++a) d->centroid[a] = (float)((double)S[a] / ((double)W * 1024.0));
    D += 1;
  }
  free(stack);
  return D;
}

/* One update at the stamp scan_id + 1.  slots: tp->max_tracks records, the raw state; out: room for tp->max_tracks
 * records; obj_tracks, obj_dets: n words each.  Returns 0, or 1 when the stamp is refused: nothing is written then. */
int track_shim_update(const tobject_t* obj, uint32_t n, uint32_t scan_id, const tparams_t* tp, ttrack_t* slots,
                      uint32_t* last_stamp, uint32_t* next_id, ttrack_t* out, uint32_t* n_out, uint32_t* obj_tracks,
                      uint32_t* obj_dets, tcounts_t* counts) {
  const uint32_t s = scan_id + 1u, T = tp->max_tracks;
  if (!(s > *last_stamp)) return 1;
  tdet_t* det = (tdet_t*)malloc(((size_t)n + 1) * sizeof(tdet_t));
  uint32_t* det_slot = (uint32_t*)malloc(((size_t)n + 1) * sizeof(uint32_t));  /* the slot a detection matched */
  uint32_t* det_track = (uint32_t*)malloc(((size_t)n + 1) * sizeof(uint32_t)); /* the id it matched or founded */
  uint32_t* det_pick = (uint32_t*)malloc(((size_t)n + 1) * sizeof(uint32_t));
  uint32_t* trk_det = (uint32_t*)malloc(((size_t)T + 1) * sizeof(uint32_t));
  uint32_t* trk_pick = (uint32_t*)malloc(((size_t)T + 1) * sizeof(uint32_t));
  float* pred = (float*)malloc(((size_t)T + 1) * 4 * sizeof(float));
  memset(counts, 0, sizeof(*counts));
  const uint32_t D = track_shim_join(obj, n, tp->join_dist, det, obj_dets);
  counts->n_objects = n, counts->n_detections = D, counts->n_joined = n - D;
  const float dt = (float)(s - *last_stamp);

  /* step 2 */
  for (uint32_t t = 0; t < T; ++t) {
    trk_det[t] = T_NONE;
    if (!slots[t].state) continue;
    counts->n_tracks_before += 1;
    for (int a = 0; a < 3; ++a) {
      const float step = slots[t].velocity[a] * dt;
      pred[4 * t + a] = slots[t].position[a] + step;
    }
    const float age = tp->gate_speed * (float)(s - slots[t].last_matched);
    pred[4 * t + 3] = tp->gate_base + age;
  }
  for (uint32_t d = 0; d < D; ++d) det_slot[d] = T_NONE;

  /* step 3 */
  uint32_t r = 0;
  for (;; ++r) {
    uint32_t candidates = 0;
    for (uint32_t t = 0; t < T; ++t) trk_pick[t] = T_NONE;
    for (uint32_t d = 0; d < D; ++d) {
      det_pick[d] = T_NONE;
      if (det_slot[d] != T_NONE) continue;
      uint32_t best_bits = 0;
      for (uint32_t t = 0; t < T; ++t) {
        if (!slots[t].state || trk_det[t] != T_NONE) continue;
        const float dist = len3(det[d].centroid[0] - pred[4 * t], det[d].centroid[1] - pred[4 * t + 1],
                                det[d].centroid[2] - pred[4 * t + 2]);
        if (!(dist <= pred[4 * t + 3])) continue;
        const uint32_t b = bits(dist);
        if (det_pick[d] == T_NONE || b < best_bits) det_pick[d] = t, best_bits = b; /* ascending t: a tie keeps the lower */
      }
      candidates += det_pick[d] != T_NONE;
    }
    if (candidates == 0 || r == tp->max_rounds) {
      counts->n_unresolved = candidates;
      break;
    }
    for (uint32_t t = 0; t < T; ++t) {
      if (!slots[t].state || trk_det[t] != T_NONE) continue;
      uint32_t best_bits = 0;
      for (uint32_t d = 0; d < D; ++d) {
        if (det_slot[d] != T_NONE) continue;
        const float dist = len3(det[d].centroid[0] - pred[4 * t], det[d].centroid[1] - pred[4 * t + 1],
                                det[d].centroid[2] - pred[4 * t + 2]);
        if (!(dist <= pred[4 * t + 3])) continue;
        const uint32_t b = bits(dist);
        if (trk_pick[t] == T_NONE || b < best_bits) trk_pick[t] = d, best_bits = b;
      }
    }
    for (uint32_t d = 0; d < D; ++d)
      if (det_pick[d] != T_NONE && trk_pick[det_pick[d]] == d) det_slot[d] = det_pick[d], trk_det[det_pick[d]] = d;
  }
  counts->rounds = r;

  /* step 4 */
  for (uint32_t t = 0; t < T; ++t) {
    ttrack_t* k = &slots[t];
    if (!k->state) continue;
    if (trk_det[t] != T_NONE) {
      const tdet_t* d = &det[trk_det[t]];
      for (int a = 0; a < 3; ++a) {
        const float res = d->centroid[a] - pred[4 * t + a];
        if (k->hits == 1u) {
          k->position[a] = d->centroid[a];
          k->velocity[a] = res / dt;
        } else {
          const float gain = tp->beta / dt;
          const float dp = tp->alpha * res, dv = gain * res;
          k->position[a] = pred[4 * t + a] + dp;
          k->velocity[a] = k->velocity[a] + dv;
        }
        k->min[a] = d->min[a], k->max[a] = d->max[a];
      }
      if (k->hits < 65535u) k->hits += 1;
      k->missed = 0;
      k->label = d->label, k->n_texels = d->n_texels, k->n_dynamic = d->n_dynamic, k->n_objects = d->n_objects;
      k->r_min = d->r_min;
      k->last_matched = s;
      k->detection = trk_det[t];
      if (k->hits >= tp->confirm_hits) k->state = 2;
      det_track[trk_det[t]] = k->id;
      counts->n_matched += 1;
    } else {
      for (int a = 0; a < 3; ++a) k->position[a] = pred[4 * t + a];
      k->missed += 1;
      k->detection = T_NONE;
      counts->n_missed += 1;
      if (k->missed > tp->max_missed) {
        memset(k, 0, sizeof(*k));
        counts->n_expired += 1;
      }
    }
  }
  uint32_t slot = 0;
  for (uint32_t d = 0; d < D; ++d) {
    if (det_slot[d] != T_NONE) continue;
    while (slot < T && slots[slot].state) ++slot;
    if (slot == T) {
      det_track[d] = 0;
      counts->n_dropped += 1;
      continue;
    }
    ttrack_t* k = &slots[slot];
    memset(k, 0, sizeof(*k));
    k->id = *next_id + counts->n_born;
    k->slot = slot;
    k->state = (1u >= tp->confirm_hits) ? 2 : 1;
    k->label = det[d].label, k->n_texels = det[d].n_texels, k->n_dynamic = det[d].n_dynamic, k->n_objects = det[d].n_objects;
    k->hits = 1, k->first_stamp = s, k->last_matched = s;
    for (int a = 0; a < 3; ++a) {
      k->position[a] = k->origin[a] = det[d].centroid[a];
      k->min[a] = det[d].min[a], k->max[a] = det[d].max[a];
    }
    k->r_min = det[d].r_min;
    k->detection = d;
    det_track[d] = k->id;
    counts->n_born += 1;
  }
  *next_id += counts->n_born;
  *last_stamp = s;
  *n_out = 0;
  for (uint32_t t = 0; t < T; ++t)
    if (slots[t].state) {
      out[(*n_out)++] = slots[t];
      counts->n_confirmed += slots[t].state == 2;
    }
  for (uint32_t i = 0; i < n; ++i) obj_tracks[i] = det_track[obj_dets[i]];
  free(pred), free(trk_pick), free(trk_det), free(det_pick), free(det_track), free(det_slot), free(det);
  return 0;
}

#ifdef TRACK_SHIM_MAIN
/* the stand-alone run for the sanitizers: a few hundred random objects through a dozen updates on a small table */
#include <stdio.h>
static uint32_t lcg(uint32_t* x) { return *x = *x * 1664525u + 1013904223u; }
int main(void) {
  enum { N = 300, T = 65 };
  tparams_t tp = {2.0f, 1.5f, 0.5f, 0.5f, 0.2f, 3, 3, T, 16};
  tobject_t* obj = (tobject_t*)calloc(N, sizeof(tobject_t));
  ttrack_t* slots = (ttrack_t*)calloc(T, sizeof(ttrack_t));
  ttrack_t* out = (ttrack_t*)calloc(T, sizeof(ttrack_t));
  uint32_t* ot = (uint32_t*)calloc(N, 4);
  uint32_t* od = (uint32_t*)calloc(N, 4);
  uint32_t last = 0, next = 1, n_out = 0, x = 7u, sum = 0;
  tcounts_t cnt;
  for (uint32_t scan = 0; scan < 12; ++scan) {
    const uint32_t n = scan == 3 ? 0 : (scan & 1 ? N : 70);
    for (uint32_t i = 0; i < n; ++i) {
      tobject_t* o = &obj[i];
      o->root = i, o->n_texels = 1 + lcg(&x) % 50, o->label = 10 * (lcg(&x) % 3), o->n_dynamic = lcg(&x) % 3;
      for (int a = 0; a < 3; ++a) {
        o->min[a] = (float)(lcg(&x) % 256) * 0.125f + (float)scan * 0.25f;
        o->max[a] = o->min[a] + (float)(lcg(&x) % 8) * 0.125f;
        o->centroid[a] = 0.5f * (o->min[a] + o->max[a]);
      }
      o->r_min = (float)(lcg(&x) % 100);
    }
    if (track_shim_update(obj, n, scan == 5 ? 2 : scan * 2, &tp, slots, &last, &next, out, &n_out, ot, od, &cnt) != (scan == 5))
      return 1;
    sum += cnt.n_matched + cnt.n_born + n_out;
  }
  printf("track_shim ok %u\n", sum);
  free(od), free(ot), free(out), free(slots), free(obj);
  return 0;
}
#endif
