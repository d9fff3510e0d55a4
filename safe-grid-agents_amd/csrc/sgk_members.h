// sgk_members.h -- the arithmetic of the exploit / explore step (include/sgk.h: sgk_members_select) as plain host + device C++: the
// ranking's total order, the explore step's coin and the perturbed value. The kernels of sgk_members.hip and the host-only entry
// points (sgk_members_select_host, sgk_members_explore_pick) run this very code.
#pragma once
#include <stdint.h>

#include "sgk_transition.h"

namespace sgk {

#define SGK_RNG_STREAM_EXPLORE 7u

// the score the ranking reads: NaN counts as -inf
SGK_HD double members_score(double s) { return s != s ? -__builtin_inf() : s; }

// member j (score sj) ranks above member m (score sm): a total order (-0.0 == 0.0 and equal scores fall back on the index)
SGK_HD bool members_above(double sj, int j, double sm, int m) { return sj > sm || (sj == sm && j < m); }

// the explore step's coin for (member, column) at `generation`: 1 = factor_up, 0 = factor_down
SGK_HD int members_explore_pick(uint64_t key, uint64_t generation, uint32_t member, uint32_t column) {
  const Philox4 x = philox4x32_10_v(member, column, (uint32_t)generation, SGK_RNG_STREAM_EXPLORE, (uint32_t)key, (uint32_t)(key >> 32));
  return (int)(x.x0 & 1u);
}

// min(max(v * f, lo), hi): one IEEE multiply (never contracted), then the two comparisons
SGK_HD double members_perturb(double v, double f, double lo, double hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  double p = __dmul_rn(v, f);
#else
  double p = v * f;
#endif
  p = p < lo ? lo : p;
  return p > hi ? hi : p;
}

// ---- the ensemble's vote (include/sgk.h: sgk_members_vote; the kernel and sgk_members_vote_host run this) -------------------------------
// One env's four counts in one 64-bit word, 16 bits per action, action 0 lowest: SGK_MEMBERS_MAX = 4096 voters fit, and the word is
// the env's row of votes_out as it lies in memory. A byte that is no action (> 3) casts no vote.
SGK_HD uint64_t members_vote_cast(uint64_t counts, uint32_t action) { return action < 4u ? counts + (1ull << (16u * action)) : counts; }
SGK_HD uint32_t members_vote_count(uint64_t counts, int action) { return (uint32_t)(counts >> (16 * action)) & 0xffffu; }
SGK_HD uint32_t members_vote_total(uint64_t counts) {
  return members_vote_count(counts, 0) + members_vote_count(counts, 1) + members_vote_count(counts, 2) + members_vote_count(counts, 3);
}
// the first action with the most votes: np.argmax's tie rule
SGK_HD int members_vote_winner(uint64_t counts) {
  int best = 0;
  uint32_t most = members_vote_count(counts, 0);
  for (int a = 1; a < 4; ++a) {
    const uint32_t c = members_vote_count(counts, a);
    if (c > most) most = c, best = a;
  }
  return best;
}

}  // namespace sgk
