/*
 * group_by_key.h -- the device pieces every feature that groups records by a key shares: the voxel key, the vote
 * weight, the weighted label vote over a run ordered by (label, index), and the two span look-ups.  The world export
 * (k_world.hip), the novelty fusion (k_novel.hip), the localiser's window (k_localize.hip, k_change.hip) and the
 * checkpoint packer (k_checkpoint.hip) use them; each host shim under tests/ restates them independently.  The host
 * half -- the sorts, the run heads and the scan -- is k_group.hip.
 *
 * fp32, every operation as written (-ffp-contract=off; `/` correctly rounded): these bodies are specification.
 */
#ifndef SUMA_GROUP_BY_KEY_H_
#define SUMA_GROUP_BY_KEY_H_

#include "suma_internal.h"

/* the key of a record that belongs to no voxel: it sorts behind every voxel */
#define VOXEL_NO_KEY 0xffffffffffffffffull

/* f_a = floorf(p_a / voxel_size) per axis; false (the record is DROPPED) when any |f_a| >= 2^20, NaN and infinite
 * quotients included; else i_a = (int)f_a and *key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20) */
SDEV bool voxel_key(float x, float y, float z, float voxel_size, unsigned long long* key) {
  const float fx = sdm_floor(x / voxel_size), fy = sdm_floor(y / voxel_size), fz = sdm_floor(z / voxel_size);
  if (!(fabsf(fx) < 1048576.0f && fabsf(fy) < 1048576.0f && fabsf(fz) < 1048576.0f)) return false;
  const unsigned long long ix = (unsigned long long)((int32_t)fx + 1048576), iy = (unsigned long long)((int32_t)fy + 1048576),
                           iz = (unsigned long long)((int32_t)fz + 1048576);
  *key = (ix << 42) | (iy << 21) | iz;
  return true;
}

/* the weight a member votes with: q = (uint32)rintf(clamp(w, 0, 1) * 65535.0f) */
SDEV uint32_t vote_weight(float w) {
  const float c = (w > 0.0f) ? ((w < 1.0f) ? w : 1.0f) : 0.0f; /* NaN: 0 */
  return (uint32_t)__builtin_rintf(c * 65535.0f);
}

/* The weighted label vote over the members of one run, which come ordered by label: add() every member, then close()
 * once.  The weights are summed per label in uint64 (exact, order-free); the label with the greatest sum wins, on a tie
 * the smallest id (labels ascend and a later one must be strictly greater).  When every weight is 0 there is no winner:
 * the label is the representative's -- whose rule is the caller's -- and prob is 0. */
struct LabelVote {
  unsigned long long sum_all = 0, sum_cur = 0, sum_best = 0;
  uint32_t lab_cur = 0xffffffffu, lab_best = 0;
  SDEV void add(uint32_t L, uint32_t q) {
    if (L != lab_cur) {
      if (sum_cur > sum_best) sum_best = sum_cur, lab_best = lab_cur;
      lab_cur = L, sum_cur = 0;
    }
    sum_cur += q;
    sum_all += q;
  }
  /* behind the last member: returns prob and sets *label */
  SDEV float close(uint32_t rep_label, uint32_t* label) {
    if (sum_cur > sum_best) sum_best = sum_cur, lab_best = lab_cur;
    float prob = 0.0f;
    if (sum_all != 0) prob = (float)sum_best / (float)sum_all; else lab_best = rep_label;
    *label = lab_best;
    return prob;
  }
};

/* the index into LocMap.sorted of window position o: the last span that starts at or before o, then the offset into
 * it.  Precondition: n_spans >= 1, no span is empty, o < the window's total */
SDEV size_t loc_window_record(const LocSpan* spans, uint32_t n_spans, uint32_t o) {
  uint32_t lo = 0, hi = n_spans;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (spans[mid].dst <= o) lo = mid; else hi = mid;
  }
  const LocSpan sp = spans[lo];
  return (size_t)(sp.src + (o - sp.dst)); /* < 2^31, the most records a map holds */
}

/* the last span that starts at or before q (empty spans share their start; n_spans >= 1).  The unit of start -- records,
 * or 16-byte pieces -- is the caller's */
SDEV WorldSpan world_span_find(const WorldSpan* spans, uint32_t n_spans, uint32_t q) {
  uint32_t lo = 0, hi = n_spans;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (spans[mid].start <= q) lo = mid; else hi = mid;
  }
  return spans[lo];
}

#endif
