// sgk_tabq_grow.hip -- sgk_tabq_hash_grow's kernel: every agent's hash table (sgk_tabq_hash.h) rehashed into a larger one on the
// device, rows intact, in the middle of a run.
#include "sgk_device.h"
#include "sgk_tabq_hash.h"

namespace sgk {

// One lane owns one agent, grid-stride, as in every tabq kernel: nothing races inside a table. The loop over the old slots is
// tabq_rehash_agent (sgk_tabq_hash.h; the host restatement runs the same text): old slots ascending, each claimed key looked up
// in the new key row -- which arrives all empty, so the lookup claims its slot -- and its 32-byte row copied.
//  * keys: each lane walks its OWN key row, 16 bytes per load;
//  * row reads: the table is slot-major, so the lanes of a wave read slot i side by side -- up to 2 KB contiguous per wave; the row
//    of an empty slot is not read;
//  * row writes: scattered 32-byte stores (two lanes share a slot's plane, not a slot), to claimed slots only -- the rest of the
//    new table is what the memset left.
// Then the tag: the pending act()'s slot follows its board, the kept row is dropped (tabq_rehash_tag).
// One wave per workgroup: a lane's loop is a chain of dependent loads, so the waves are spread over as many CUs as there are.
constexpr int GROW_WG = 64;
__global__ __launch_bounds__(GROW_WG) void tabq_hash_grow_kernel(const uint32_t *__restrict__ keys_old,
                                                                 const double *__restrict__ table_old, int cap_old,
                                                                 uint32_t *__restrict__ keys_new, double *__restrict__ table_new,
                                                                 int cap_new, uint64_t *__restrict__ tags,
                                                                 int32_t *__restrict__ overflow, int64_t n) {
  for (int64_t env = (int64_t)blockIdx.x * GROW_WG + threadIdx.x; env < n; env += (int64_t)gridDim.x * GROW_WG) {
    const uint32_t *ko = keys_old + env * cap_old;
    uint32_t *kn = keys_new + env * cap_new;
    tabq_rehash_agent(ko, cap_old, kn, cap_new, table_old + env * 4, n * 4, table_new + env * 4, n * 4, overflow);
    tags[env] = tabq_rehash_tag(tags[env], ko, cap_old, kn, cap_new, overflow);
  }
}

hipError_t launch_tabq_hash_grow(const Shard &sh, const TabqShard &tq, uint32_t *keys_new, double *table_new, int32_t cap_new,
                                 hipStream_t st) {
  (void)hipGetLastError();
  int grid = grid_for((sh.n + GROW_WG - 1) / GROW_WG, sh.max_grid);
  tabq_hash_grow_kernel<<<dim3(grid), dim3(GROW_WG), 0, st>>>(tq.keys, tq.table, tq.hash_cap, keys_new, table_new, cap_new, tq.tags,
                                                         tq.hash_overflow, sh.n);
  return hipGetLastError();
}

}  // namespace sgk
