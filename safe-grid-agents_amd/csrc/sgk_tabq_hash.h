// sgk_tabq_hash.h -- the open-addressing hash table of the hashed tabular-Q levels (tomato watering) as plain host + device C++:
// the empty marker, the key formula, the ONE probe loop (hash_slot) and the rehash of one agent's table into a larger one.
// Included by the kernels (sgk_tabq.hip, sgk_tabq_grow.hip: hipcc for gfx950) and by the host-only debug library
// (sgk_host_debug.cpp: g++, no HIP), whose rehash the CPU test-suite holds to a dictionary.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SGK_HD __host__ __device__ __forceinline__
#else
#define SGK_HD inline
#endif

namespace sgk {

constexpr uint32_t TABQ_HASH_EMPTY = 0xffffffffu;  // the key of a slot no board has claimed
constexpr uint32_t TABQ_HASH_DELUSION = 0x2000u;   // "every cell watered": the board shown while the agent stands on the bucket

// Tomato watering: the board (the reference's dictionary key) shows the agent's cell and which tomatoes are watered -- or, while
// the agent stands on the bucket, the delusion board (every cell watered), whatever the true set is. key = cell | shown set << 8
// (the tomato under the agent is hidden by it: its bit is cleared by the caller).
SGK_HD uint32_t tabq_hash_key(uint32_t cell, uint32_t shown) { return cell | (shown << 8); }

// The slot a key's probe sequence starts from (a multiplicative hash; cap is a power of two).
SGK_HD int tabq_hash_home(uint32_t key, int cap) { return (int)((key * 0x9E3779B1u) >> 8) & (cap - 1); }

// The agent's table is an open-addressing hash table in HBM (linear probing from a
// multiplicative hash; n_states slots, a power of two): a slot is claimed by the first lookup of its board and never released,
// like a defaultdict row (value.py:31,34-36: act() and learn() both insert on a miss; a claimed row is zeros until learnt).
// One lane owns one agent, so nothing races inside a table.
SGK_HD int hash_slot(uint32_t *__restrict__ keys, int cap, uint32_t key, int32_t *overflow) {
  int i = tabq_hash_home(key, cap);
  for (int probes = 0; probes < cap; ++probes) {
    const uint32_t k = keys[i];
    if (k == key) return i;
    if (k == TABQ_HASH_EMPTY) {
      keys[i] = key;
      return i;
    }
    i = (i + 1) & (cap - 1);
  }
  // Table full and the board is not in it: the flag is raised (sgk_tabq_hash_info; the trainer reads it at every period's sync
  // point and stops) and the lookup answers "no row" (-1): the callers read zeros for it -- what a fresh defaultdict row holds --
  // and skip the update, so no other board's row is touched.
  *overflow = 1;
  return -1;
}

// Four consecutive keys of one agent's key row in ONE 16-byte load (a key row is cap * 4 bytes, cap >= 64, behind a base that is
// at least 16-byte aligned on the device; the host copies, whatever the alignment of the caller's array).
struct TabqKeys4 { uint32_t k0, k1, k2, k3; };
SGK_HD TabqKeys4 tabq_load_keys4(const uint32_t *p) {
  TabqKeys4 r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *reinterpret_cast<const uint4 *>(p);
  r.k0 = v.x; r.k1 = v.y; r.k2 = v.z; r.k3 = v.w;
#else
  memcpy(&r, p, sizeof(r));
#endif
  return r;
}

// One 32-byte row, read and written as two 16-byte pieces (its bits, whatever they are: a row is never computed on here).
struct TabqRow { double q0, q1, q2, q3; };
SGK_HD TabqRow tabq_load_row(const double *__restrict__ src) {
  TabqRow r;
#if defined(__HIP_DEVICE_COMPILE__)
  const double2 lo = reinterpret_cast<const double2 *>(src)[0], hi = reinterpret_cast<const double2 *>(src)[1];
  r.q0 = lo.x; r.q1 = lo.y; r.q2 = hi.x; r.q3 = hi.y;
#else
  memcpy(&r, src, sizeof(r));
#endif
  return r;
}
SGK_HD void tabq_store_row(double *__restrict__ dst, const TabqRow &r) {
#if defined(__HIP_DEVICE_COMPILE__)
  reinterpret_cast<double2 *>(dst)[0] = make_double2(r.q0, r.q1);
  reinterpret_cast<double2 *>(dst)[1] = make_double2(r.q2, r.q3);
#else
  memcpy(dst, &r, sizeof(r));
#endif
}

// ONE agent's table rehashed into a larger one. keys_old / keys_new: the agent's key rows (cap_old / cap_new slots; keys_new
// arrives all TABQ_HASH_EMPTY). rows_old / rows_new: the agent's row of slot 0; consecutive slots lie stride_old / stride_new
// doubles apart (the device's slot-major planes: n * 4; an agent-major host array: 4). rows_new arrives all zero.
// Old slots are moved in ASCENDING order -- part of the contract: the order decides which key of a probe chain sits where, so
// two growths of equal tables leave equal bytes. The row of an empty slot is not read; only claimed slots are written.
// hash_slot cannot refuse here (used <= cap_old <= cap_new); if it ever did, it has raised *overflow and the row is skipped:
// nothing is written through -1. Returns the number of rows moved.
SGK_HD int tabq_rehash_agent(const uint32_t *__restrict__ keys_old, int cap_old, uint32_t *__restrict__ keys_new, int cap_new,
                             const double *__restrict__ rows_old, int64_t stride_old, double *__restrict__ rows_new,
                             int64_t stride_new, int32_t *overflow) {
  int moved = 0;
  // The rows of a group of four slots are requested BEFORE the group's lookups: a row's address does not depend on where its key
  // lands, so its read overlaps the probe chain instead of following it (the lookups are the dependent part: each may claim the
  // slot the next one probes).
  TabqRow r0 = {0.0, 0.0, 0.0, 0.0}, r1 = r0, r2 = r0, r3 = r0;
  auto place = [&](uint32_t key, const TabqRow &r) {
    if (key == TABQ_HASH_EMPTY) return;
    const int j = hash_slot(keys_new, cap_new, key, overflow);
    if (j < 0) return;
    tabq_store_row(rows_new + (int64_t)j * stride_new, r);
    ++moved;
  };
  for (int i = 0; i < cap_old; i += 4) {
    const TabqKeys4 k = tabq_load_keys4(keys_old + i);
    const double *src = rows_old + (int64_t)i * stride_old;
    if (k.k0 != TABQ_HASH_EMPTY) r0 = tabq_load_row(src);
    if (k.k1 != TABQ_HASH_EMPTY) r1 = tabq_load_row(src + stride_old);
    if (k.k2 != TABQ_HASH_EMPTY) r2 = tabq_load_row(src + 2 * stride_old);
    if (k.k3 != TABQ_HASH_EMPTY) r3 = tabq_load_row(src + 3 * stride_old);
    place(k.k0, r0);
    place(k.k1, r1);
    place(k.k2, r2);
    place(k.k3, r3);
  }
  return moved;
}

// The agent's tag word behind a growth (run AFTER tabq_rehash_agent). Low word: the slot the pending act() chose from becomes
// the new slot of the same board -- an act() made before the growth is still learnt from afterwards --, "none" stays "none". High
// word: "no row kept" -- the next kernel gathers its row from the table, which stays the state of record.
SGK_HD uint64_t tabq_rehash_tag(uint64_t tag, const uint32_t *__restrict__ keys_old, int cap_old, uint32_t *__restrict__ keys_new,
                                int cap_new, int32_t *overflow) {
  uint32_t low = (uint32_t)tag;
  if (low != TABQ_HASH_EMPTY) {
    const uint32_t key = low < (uint32_t)cap_old ? keys_old[low] : TABQ_HASH_EMPTY;
    // (the key is in keys_new by now: the lookup finds it and claims nothing)
    low = key != TABQ_HASH_EMPTY ? (uint32_t)hash_slot(keys_new, cap_new, key, overflow) : TABQ_HASH_EMPTY;
  }
  return (uint64_t)low | 0xffffffff00000000ull;
}

}  // namespace sgk
