// sgk_crmdp.h -- corrupt-reward detection for PPOCRMDPAgent (reference spiky/agents.py:74-270) as plain host + device C++ on INTEGER
// keys and INTEGER rewards: the metric, the Lipschitz violation, the trajectory-local detect walk and the steps of the per-agent
// merge. Included by the kernels (sgk_crmdp.hip: hipcc for gfx950), whose wave-parallel detect and workgroup-parallel merge use the
// metric, the violation and the table steps, and compiled for the host in the same file, where sgk_crmdp_filter_host runs the serial
// walk below. The semantics are include/sgk.h's (sgk_crmdp_filter).
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SGK_CRMDP_HD __host__ __device__ __forceinline__
#else
#define SGK_CRMDP_HD inline
#endif

namespace sgk {

constexpr int CRMDP_T_MAX = 128;        // steps of a trajectory: a lane of the detect kernel owns steps lane and lane + 64
constexpr int CRMDP_MAX_KEYS = 4096;    // keys of an agent's memory: 9 bytes each in the merge kernel's LDS
constexpr uint8_t CRMDP_UNKNOWN = 0, CRMDP_SAFE = 1, CRMDP_CORRUPT = 2;
constexpr int32_t CRMDP_NONE = INT32_MIN;  // "no bound": the reference's None

struct CrmdpMetric {
  int32_t kind, width, n_cells;
};
SGK_CRMDP_HD int crmdp_n_keys(const CrmdpMetric &m) { return m.n_cells * m.n_cells; }

// d_trans_boat (spiky/agents.py:41-63) on keys = prev cell * n_cells + cur cell, cells row-major: the Manhattan distance of the two
// previous cells plus one for each axis on which the two moves differ. (The only kind so far; a second metric is a second case.)
SGK_CRMDP_HD int crmdp_d(const CrmdpMetric &m, int a, int b) {
  const int pa = a / m.n_cells, ca = a - pa * m.n_cells, pb = b / m.n_cells, cb = b - pb * m.n_cells;
  const int par = pa / m.width, pac = pa - par * m.width, car = ca / m.width, cac = ca - car * m.width;
  const int pbr = pb / m.width, pbc = pb - pbr * m.width, cbr = cb / m.width, cbc = cb - cbr * m.width;
  const int dr = par - pbr, dc = pac - pbc;
  return (dr < 0 ? -dr : dr) + (dc < 0 ? -dc : dc) + ((car - par) != (cbr - pbr) ? 1 : 0) + ((cac - pac) != (cbc - pbc) ? 1 : 0);
}

// max(0, |r_i - r_j| - d(k_j, k_i)): what state j adds to the total Lipschitz violation of state i (_get_TLV, :124-133)
SGK_CRMDP_HD int crmdp_viol(const CrmdpMetric &m, int ki, int ri, int kj, int rj) {
  const int dr = ri - rj, v = (dr < 0 ? -dr : dr) - crmdp_d(m, kj, ki);
  return v > 0 ? v : 0;
}

// A float32 reward of the raw call as the integer the detector works on: round to nearest (the header asks for integer values).
SGK_CRMDP_HD int crmdp_reward(float r) { return (int)(r < 0.0f ? r - 0.5f : r + 0.5f); }

// The length a call works with: lengths[i] clamped to 0 .. t_max, or t_max without the array.
SGK_CRMDP_HD int crmdp_length(const int32_t *lengths, int64_t i, int t_max) {
  if (!lengths) return t_max;
  const int l = lengths[i];
  return l < 0 ? 0 : (l > t_max ? t_max : l);
}

// ---- detect, serially (the host call; the kernel's wave-parallel form computes the same) ------------------------------------------------
// keys / rewards: the trajectory's L <= CRMDP_T_MAX steps. order_out [t_max]: the corrupt indices in marking order, then -1.
// Returns n_corrupt (-1: a key outside [0, n_keys): nothing is marked); *safe_out: the safe index or -1.
SGK_CRMDP_HD int crmdp_detect_serial(const CrmdpMetric &m, const int32_t *keys, const int32_t *rewards, int L, int t_max,
                                     int32_t *order_out, int32_t *safe_out) {
  const int n_keys = crmdp_n_keys(m);
  for (int t = 0; t < t_max; ++t) order_out[t] = -1;
  *safe_out = -1;
  for (int i = 0; i < L; ++i)
    if (keys[i] < 0 || keys[i] >= n_keys) return -1;
  bool alive[CRMDP_T_MAX], first[CRMDP_T_MAX], done[CRMDP_T_MAX];  // first: alive and the first alive occurrence of its key
  int tlv0[CRMDP_T_MAX];
  // the TLV of idx over the first occurrence of each key among the alive indices
  auto tlv = [&](int idx) {
    int sum = 0;
    for (int j = 0; j < L; ++j)
      if (first[j]) sum += crmdp_viol(m, keys[idx], rewards[idx], keys[j], rewards[j]);
    return sum;
  };
  for (int i = 0; i < L; ++i) {
    alive[i] = true, done[i] = false, first[i] = true;
    for (int e = 0; e < i && first[i]; ++e) first[i] = keys[e] != keys[i];
  }
  for (int i = 0; i < L; ++i) tlv0[i] = tlv(i);
  int n_corrupt = 0;
  for (int it = 0; it < L; ++it) {
    int idx = -1;  // descending TLV0, equal values by descending index
    for (int i = 0; i < L; ++i)
      if (!done[i] && (idx < 0 || tlv0[i] >= tlv0[idx])) idx = i;
    done[idx] = true;
    const int value = n_corrupt == 0 ? tlv0[idx] : tlv(idx);
    if (value <= 0) {
      *safe_out = idx;
      break;
    }
    order_out[n_corrupt++] = idx;
    alive[idx] = false;
    if (first[idx]) {  // the key's next alive occurrence takes its place, with its own reward
      first[idx] = false;
      for (int j = 0; j < L; ++j)
        if (alive[j] && keys[j] == keys[idx]) {
          first[j] = true;
          break;
        }
    }
  }
  return n_corrupt;
}

// ---- merge: the steps on ONE agent's tables flag / reward / rllb [n_keys] -----------------------------------------------------------------
// steps 1 and 2: the corrupt marks in marking order (they overwrite, a SAFE entry included), then the safe candidate unless memory
// has its key corrupt. (An index outside the trajectory's L steps -- detect writes none -- is skipped: no table access out of range.)
SGK_CRMDP_HD void crmdp_mark(uint8_t *flag, int32_t *reward, const int32_t *keys, const int32_t *rewards, const int32_t *order,
                             int n_corrupt, int safe_index, int L) {
  for (int c = 0; c < n_corrupt; ++c) {
    const int i = order[c];
    if (i < 0 || i >= L) continue;
    const int k = keys[i];
    flag[k] = CRMDP_CORRUPT;
    reward[k] = rewards[i];
  }
  if (safe_index >= 0 && safe_index < L) {
    const int k = keys[safe_index];
    if (flag[k] != CRMDP_CORRUPT) flag[k] = CRMDP_SAFE, reward[k] = rewards[safe_index];
  }
}
// step 3 for ONE corrupt key c: its bound raised to max_s (reward[s] - d(s, c)) over the safe keys listed in `safe` (_update_rllb)
SGK_CRMDP_HD int32_t crmdp_raise_bound(const CrmdpMetric &m, int32_t bound, int c, const int32_t *reward, const uint16_t *safe,
                                       int n_safe) {
  for (int i = 0; i < n_safe; ++i) {
    const int s = safe[i], b = reward[s] - crmdp_d(m, s, c);
    if (b > bound) bound = b;
  }
  return bound;
}
// step 4 for ONE step: the reward PPO learns from; *unbounded is raised where a corrupt key has no bound (the reward is kept)
SGK_CRMDP_HD float crmdp_modified(const uint8_t *flag, const int32_t *rllb, int k, float r, int *unbounded) {
  if (flag[k] != CRMDP_CORRUPT) return r;
  if (rllb[k] == CRMDP_NONE) {
    *unbounded += 1;
    return r;
  }
  return (float)rllb[k];
}

}  // namespace sgk
