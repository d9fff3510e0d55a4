// sgk_tabq_vote.h -- the rule of the tabular agents' consensus as plain host + device C++: what a row votes (vote_of_row, shared by
// sgk_tabq_consensus.hip and sgk_tabq_hash_consensus.hip, kernels and host restatements alike) and, for the hashed levels, the rank
// of a voted key in ascending key order from a presence bitmap and its prefix popcount (tabq_key_rank).
#pragma once
#include <stdint.h>

#include "sgk_tabq_hash.h"

namespace sgk {

// A row's vote: -1 for a row that is all zeros (either sign: a row the agent never learnt, the reference's fresh defaultdict row,
// whose argmax of 0 is no opinion), else the greedy action of sgk_tabq_act(explore = 0) -- the first maximum, as np.argmax picks.
SGK_HD int vote_of_row(double q0, double q1, double q2, double q3) {
  if (!(q0 != 0.0 || q1 != 0.0 || q2 != 0.0 || q3 != 0.0)) return -1;
  int best = 0;
  double bv = q0;
  if (q1 > bv) { bv = q1; best = 1; }
  if (q2 > bv) { bv = q2; best = 2; }
  if (q3 > bv) { bv = q3; best = 3; }
  return best;
}

// Every key of a hashed level is below 1 << 22 (sgk_tabq_hash.h: cell | shown << 8, shown <= 0x2000), so the set of voted keys is
// a bitmap of 2^22 bits: 65 536 words of 64.
constexpr int TABQ_VOTE_KEY_BITS = 22;
constexpr int TABQ_VOTE_WORDS = 1 << (TABQ_VOTE_KEY_BITS - 6);
constexpr uint8_t TABQ_VOTE_NONE = 0xff;  // the vote code of a (slot, agent) that casts no vote

SGK_HD bool tabq_key_votable(uint32_t key) { return key < (1u << TABQ_VOTE_KEY_BITS); }  // (the empty marker is not)

// The rank of a voted key among the voted keys, ascending: the set bits in the words before its word (prefix[word], an exclusive
// prefix sum of the words' popcounts) plus the set bits BELOW its bit in its own word.
SGK_HD int64_t tabq_key_rank(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ prefix, uint32_t key) {
  const uint32_t word = key >> 6, bit = key & 63u;
  const uint64_t below = bitmap[word] & ((1ull << bit) - 1ull);
  return (int64_t)prefix[word] + __builtin_popcountll(below);
}

}  // namespace sgk
