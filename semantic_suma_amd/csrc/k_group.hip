/*
 * k_group.hip -- records grouped by a key, the host half (the device inlines are group_by_key.h): stable radix sorts of
 * (key, index) pairs, the keys gathered through a sorted index, the heads of the runs of equal keys and their ranks.
 * The world export (k_world.hip), the novelty fusion (k_novel.hip) and the localiser's tile binning (k_localize.hip)
 * are built from these; rocPRIM's radix_sort_pairs and exclusive_scan are instantiated for them here and nowhere else.
 *
 * Every entry works in the caller's arrays, in the caller's temporary block (group_tmp_bytes says how large) and on the
 * caller's stream; it only enqueues, owns no memory and opens no profile scope.  The sorts ping-pong inside the caller's
 * rocprim::double_buffer pairs, so their temporary storage is histograms only, and current() of each pair is the sorted
 * array afterwards.
 *
 * Kernels (VGPRs: tools/isa_stats.py k_group.hip; neither uses scratch):
 *   kg_gather   lane per sorted position: key1[j] = key0[idx[j]], the keys in the order a sort left the indices in.
 *   kg_heads    lane per sorted position: 1 where a run begins -- the key is not no_key and differs from the one before.
 */
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "suma_internal.h"

#define GROUP_THREADS 256

__global__ void __launch_bounds__(GROUP_THREADS)
    kg_gather(uint32_t n, const unsigned long long* __restrict__ key0, const uint32_t* __restrict__ idx,
              unsigned long long* __restrict__ key1) {
  const uint32_t j = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (j < n) key1[j] = key0[idx[j]];
}

__global__ void __launch_bounds__(GROUP_THREADS)
    kg_heads(uint32_t n, const unsigned long long* __restrict__ keys, unsigned long long no_key, uint32_t* __restrict__ flag) {
  const uint32_t j = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (j >= n) return;
  const unsigned long long key = keys[j];
  flag[j] = (key != no_key && (j == 0 || keys[j - 1] != key)) ? 1u : 0u;
}

static unsigned group_blocks(uint32_t n) { return (unsigned)(((size_t)n + GROUP_THREADS - 1) / GROUP_THREADS); }

/* what rocPRIM asks for grows with the number of bits sorted by, so the full widths cover every call */
hipError_t group_tmp_bytes(uint32_t n, bool sorts, hipStream_t st, size_t* bytes) {
  size_t need = 16, b = 0;
  hipError_t e = hipSuccess;
  if (n) {
    e = rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                                rocprim::plus<uint32_t>(), st);
    need = b > need ? b : need;
    if (e == hipSuccess && sorts) {
      rocprim::double_buffer<uint32_t> val, idx;
      rocprim::double_buffer<unsigned long long> key;
      e = rocprim::radix_sort_pairs(nullptr, b, val, idx, (size_t)n, 0u, 32u, st);
      need = b > need ? b : need;
      if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, b, key, idx, (size_t)n, 0u, 64u, st);
      need = b > need ? b : need;
    }
  }
  *bytes = need;
  return e;
}

hipError_t group_sort(void* tmp, size_t tmp_bytes, rocprim::double_buffer<unsigned long long>& key,
                      rocprim::double_buffer<uint32_t>& idx, uint32_t n, unsigned key_bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, key, idx, (size_t)n, 0u, key_bits, st);
}

hipError_t group_sort_by_value_then_key(void* tmp, size_t tmp_bytes, rocprim::double_buffer<uint32_t>& val,
                                        unsigned value_bits, const unsigned long long* key0,
                                        rocprim::double_buffer<unsigned long long>& key, unsigned key_bits,
                                        rocprim::double_buffer<uint32_t>& idx, uint32_t n, hipStream_t st) {
  size_t bytes = tmp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, val, idx, (size_t)n, 0u, value_bits, st);
  if (e != hipSuccess) return e;
  kg_gather<<<group_blocks(n), GROUP_THREADS, 0, st>>>(n, key0, idx.current(), key.current());
  return group_sort(tmp, tmp_bytes, key, idx, n, key_bits, st);
}

hipError_t group_scan(void* tmp, size_t tmp_bytes, const uint32_t* flag, uint32_t* pos, uint32_t n, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
}

hipError_t group_heads(void* tmp, size_t tmp_bytes, const unsigned long long* keys, unsigned long long no_key,
                       uint32_t* flag, uint32_t* pos, uint32_t n, hipStream_t st) {
  kg_heads<<<group_blocks(n), GROUP_THREADS, 0, st>>>(n, keys, no_key, flag);
  return group_scan(tmp, tmp_bytes, flag, pos, n, st);
}
