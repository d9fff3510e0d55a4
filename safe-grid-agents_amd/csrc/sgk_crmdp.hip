// sgk_crmdp.hip -- PPOCRMDPAgent's corrupt-reward detection and reward bounds (reference spiky/agents.py:74-270) on the device
// (include/sgk.h: sgk_crmdp_keys, sgk_crmdp_filter, sgk_crmdp_filter_host). Three kernels and their entry points:
//   crmdp_keys_kernel    a workgroup per tile of 64 envs: every board of the rollout [T][N][cells] is read once, as dwords along the
//                        tile's contiguous 64 * cells bytes, the agent's cell of each goes to LDS [T + 1][64], and the keys
//                        prev cell * n_cells + cur cell leave trajectory-major [N][T]: the [t][n] -> [n][t] transpose is the LDS image
//   crmdp_detect_kernel  one wave per trajectory, four per workgroup, no memory read: total Lipschitz violations, then the greedy walk
//                        (a wave maximum picks the next index, a wave sum recomputes its TLV, ballots keep the alive and
//                        first-occurrence sets)
//   crmdp_merge_kernel   one workgroup per agent, the agent's tables in LDS, its trajectories in order: marks, bounds, rewards_out
// The arithmetic both sides of the C-ABI share (metric, violation, the table steps; the serial walk of the host call) is sgk_crmdp.h.
#include <hip/hip_runtime.h>

#include "sgk_crmdp.h"
#include "sgk_device.h"
#include "sgk_host_core.h"
#include "sgk_kernels.h"

using sgk::host::fail;

namespace sgk {

namespace {

constexpr int KEYS_WG = 256, KEYS_TILE = 64;
constexpr int KEYS_ROW = 68;  // bytes per LDS row of 64 cells: 17 dwords, so the 64 steps a wave reads for one env fall into 64 banks
constexpr int DETECT_WAVES = 4;
constexpr int MERGE_WG = 256;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// grid-stride over tiles of 64 envs. Wave w scans the boards of steps w, w + 4, ... <= T (step T: the boards after the last step).
__global__ __launch_bounds__(KEYS_WG) void crmdp_keys_kernel(const int8_t *__restrict__ states, const int8_t *__restrict__ last_boards,
                                                             int T, int64_t n, int nc, int agent_value, int32_t *__restrict__ keys) {
  __shared__ uint8_t cell[(CRMDP_T_MAX + 1) * KEYS_ROW];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_index();
  const uint32_t needle = 0x01010101u * (uint32_t)(agent_value & 0xff);
  const int64_t n_tiles = (n + KEYS_TILE - 1) / KEYS_TILE;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t e0 = tile * KEYS_TILE;
    const int n_valid = (int)(n - e0 < KEYS_TILE ? n - e0 : KEYS_TILE);
    const int n_bytes = n_valid * nc;  // the tile's boards of one step: contiguous
    for (int t = w; t <= T; t += KEYS_WG / 64) {
      const int8_t *src = t < T ? states + ((int64_t)t * n + e0) * nc : last_boards + e0 * nc;
      uint8_t *row = cell + t * KEYS_ROW;
      row[lane] = 0xff;  // no agent found
      __builtin_amdgcn_wave_barrier();
      auto found = [&](int b) { row[b / nc] = (uint8_t)(b % nc); };
      int done = 0;
      if (((uintptr_t)src & 3u) == 0) {
        const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
        const int n_words = n_bytes >> 2;
        for (int u = lane; u < n_words; u += 64) {
          const uint32_t v = src32[u], x = v ^ needle;
          if ((x - 0x01010101u) & ~x & 0x80808080u) {  // some byte of v is the agent's value
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (((v >> (8 * q)) & 0xffu) == (uint32_t)(agent_value & 0xff)) found(4 * u + q);
          }
        }
        done = n_words * 4;
      }
      for (int b = done + lane; b < n_bytes; b += 64)
        if ((uint8_t)src[b] == (uint8_t)agent_value) found(b);
    }
    __syncthreads();
    const int total = n_valid * T;
    for (int i = tid; i < total; i += KEYS_WG) {  // (e0 + e) * T + t == e0 * T + i: consecutive lanes, consecutive words
      const int e = i / T, t = i - e * T;
      const int a = cell[t * KEYS_ROW + e], b = cell[(t + 1) * KEYS_ROW + e];
      keys[e0 * T + i] = (a == 0xff || b == 0xff) ? -1 : a * nc + b;
    }
    __syncthreads();  // the next tile redraws the image
  }
}

// One wave per trajectory (passes over the trajectories beyond the grid). Lane l owns steps l and l + 64. Wave-private LDS: the keys,
// the integer rewards and the order list. The sets (alive, first alive occurrence of its key) are ballots: wave-uniform 64-bit pairs.
__global__ __launch_bounds__(DETECT_WAVES * 64) void crmdp_detect_kernel(const int32_t *__restrict__ keys, const float *__restrict__ rewards,
                                                                        const int32_t *__restrict__ lengths, int64_t n, int t_max,
                                                                        CrmdpMetric m, int32_t *__restrict__ order,
                                                                        int32_t *__restrict__ n_corrupt, int32_t *__restrict__ safe_index) {
  __shared__ int32_t s_key[DETECT_WAVES][CRMDP_T_MAX], s_rew[DETECT_WAVES][CRMDP_T_MAX], s_ord[DETECT_WAVES][CRMDP_T_MAX];
  const int lane = threadIdx.x & 63, w = wave_index();
  int32_t *K = s_key[w], *R = s_rew[w], *O = s_ord[w];
  const int n_keys = crmdp_n_keys(m);
  const int i0 = lane, i1 = lane + 64;
  for (int64_t traj = (int64_t)blockIdx.x * DETECT_WAVES + w; traj < n; traj += (int64_t)gridDim.x * DETECT_WAVES) {
    const int L = uniform(crmdp_length(lengths, traj, t_max));
    const bool in0 = i0 < L, in1 = i1 < L;
    const int64_t row = traj * t_max;
    const int k0 = in0 ? keys[row + i0] : 0, k1 = in1 ? keys[row + i1] : 0;
    const int r0 = in0 ? crmdp_reward(rewards[row + i0]) : 0, r1 = in1 ? crmdp_reward(rewards[row + i1]) : 0;
    K[i0] = k0, K[i1] = k1, R[i0] = r0, R[i1] = r1, O[i0] = -1, O[i1] = -1;
    __builtin_amdgcn_wave_barrier();
    const bool bad = (in0 && (unsigned)k0 >= (unsigned)n_keys) || (in1 && (unsigned)k1 >= (unsigned)n_keys);
    int nc = 0, safe = -1;
    if (__ballot(bad) != 0ull) {  // wave-uniform: a key outside the tables makes the trajectory invalid
      nc = -1;
    } else {
      // first occurrence of its key among 0 .. L - 1
      bool f0 = in0, f1 = in1;
      for (int j = 0; j < L; ++j) {
        const int kj = K[j];  // (the same word in every lane: an LDS broadcast read)
        f0 = f0 && !(kj == k0 && j < i0);
        f1 = f1 && !(kj == k1 && j < i1);
      }
      uint64_t A0 = __ballot(in0), A1 = __ballot(in1);  // alive
      uint64_t F0 = __ballot(f0), F1 = __ballot(f1);    // alive and the first alive occurrence of its key
      // TLV0: over the first occurrences only (the set bits of F: a BoatRace episode shows at most 24 keys)
      int t0 = 0, t1 = 0;
      for (int half = 0; half < 2; ++half) {
        uint64_t bits = half ? F1 : F0;
        while (bits) {
          const int j = (int)__builtin_ctzll(bits) + 64 * half;
          bits &= bits - 1;
          const int kj = K[j], rj = R[j];
          t0 += crmdp_viol(m, k0, r0, kj, rj);
          t1 += crmdp_viol(m, k1, r1, kj, rj);
        }
      }
      int v0 = in0 ? t0 : -1, v1 = in1 ? t1 : -1;  // -1: processed (or no step)
      for (int it = 0; it < L; ++it) {
        // the unprocessed index of the largest TLV0, equal values by descending index
        const int top = uniform(wave_max(v0 > v1 ? v0 : v1));
        const uint64_t b1 = __ballot(v1 == top && v1 >= 0), b0 = __ballot(v0 == top && v0 >= 0);
        if ((b0 | b1) == 0ull) break;  // (cannot happen while it < L: every pass processes one index)
        const int idx = b1 ? 64 + 63 - (int)__builtin_clzll(b1) : 63 - (int)__builtin_clzll(b0);
        if (idx == i0) v0 = -1;
        if (idx == i1) v1 = -1;
        const int ki = K[idx], ri = R[idx];
        int value = top;
        if (nc > 0) {  // something was marked: the TLV over the first alive occurrence of each key
          int c = 0;
          if ((F0 >> lane) & 1ull) c += crmdp_viol(m, ki, ri, k0, r0);
          if ((F1 >> lane) & 1ull) c += crmdp_viol(m, ki, ri, k1, r1);
          value = uniform(wave_sum(c));
        }
        if (value <= 0) {
          safe = idx;
          break;
        }
        if (lane == 0) O[nc] = idx;
        nc += 1;
        const uint64_t bit = 1ull << (idx & 63);
        const bool was_first = ((idx < 64 ? F0 : F1) & bit) != 0ull;
        if (idx < 64) A0 &= ~bit, F0 &= ~bit;
        else A1 &= ~bit, F1 &= ~bit;
        if (was_first) {  // the key's next alive occurrence takes its place, with its own reward
          const uint64_t s0 = __ballot(in0 && k0 == ki) & A0, s1 = __ballot(in1 && k1 == ki) & A1;
          if (s0) F0 |= s0 & (~s0 + 1ull);
          else if (s1) F1 |= s1 & (~s1 + 1ull);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (i0 < t_max) order[row + i0] = O[i0];
    if (i1 < t_max) order[row + i1] = O[i1];
    if (lane == 0) n_corrupt[traj] = nc, safe_index[traj] = safe;
    __builtin_amdgcn_wave_barrier();  // the next trajectory's stores come after these reads in the instruction stream
  }
}

// One workgroup per agent: flag / reward / rllb of its n_keys keys in LDS (9 bytes a key), the list of safe keys beside them. The
// agent's E consecutive trajectories are merged in order; each one's keys, rewards and order list are staged in LDS first, the marks
// are one lane's walk over them (a key may be marked twice: the last mark counts), the bounds and rewards_out are one lane per key / step.
__global__ __launch_bounds__(MERGE_WG) void crmdp_merge_kernel(const int32_t *__restrict__ keys, const float *__restrict__ rewards,
                                                               const int32_t *__restrict__ lengths, int64_t E, int t_max, CrmdpMetric m,
                                                               const int32_t *__restrict__ order, const int32_t *__restrict__ n_corrupt,
                                                               const int32_t *__restrict__ safe_index, float *__restrict__ rewards_out,
                                                               int32_t *__restrict__ unbounded, uint8_t *__restrict__ flag_g,
                                                               int32_t *__restrict__ reward_g, int32_t *__restrict__ rllb_g) {
  __shared__ int32_t reward[CRMDP_MAX_KEYS], rllb[CRMDP_MAX_KEYS];
  __shared__ uint16_t safe[CRMDP_MAX_KEYS];
  __shared__ uint8_t flag[CRMDP_MAX_KEYS];
  __shared__ int32_t tk[CRMDP_T_MAX], tr[CRMDP_T_MAX], to[CRMDP_T_MAX];
  __shared__ int n_safe;
  const int tid = threadIdx.x, n_keys = crmdp_n_keys(m);
  const int64_t agent = blockIdx.x, base = agent * n_keys;
  for (int k = tid; k < n_keys; k += MERGE_WG) flag[k] = flag_g[base + k], reward[k] = reward_g[base + k], rllb[k] = rllb_g[base + k];
  __syncthreads();
  for (int64_t e = 0; e < E; ++e) {
    const int64_t traj = agent * E + e, row = traj * t_max;
    const int L = crmdp_length(lengths, traj, t_max);
    int nc = n_corrupt[traj];  // (one address for the whole workgroup: uniform, and so is every branch on it)
    const int sf = safe_index[traj];
    if (nc > L) nc = L;
    float rf = 0.0f;
    int k = 0;
    if (tid < t_max) {
      rf = rewards[row + tid];
      k = tid < L ? keys[row + tid] : 0;
      tk[tid] = k, tr[tid] = crmdp_reward(rf), to[tid] = order[row + tid];
    }
    if (tid == 0) n_safe = 0;
    __syncthreads();
    if (nc >= 0) {
      if (tid == 0) crmdp_mark(flag, reward, tk, tr, to, nc, sf, L);
      __syncthreads();
      if (nc > 0) {
        for (int s = tid; s < n_keys; s += MERGE_WG)
          if (flag[s] == CRMDP_SAFE) safe[atomicAdd(&n_safe, 1)] = (uint16_t)s;  // (any order: the bound is a maximum)
        __syncthreads();
        const int ns = n_safe;
        for (int c = tid; c < n_keys; c += MERGE_WG)
          if (flag[c] == CRMDP_CORRUPT) rllb[c] = crmdp_raise_bound(m, rllb[c], c, reward, safe, ns);
        __syncthreads();
      }
    }
    int ub = 0;
    if (tid < t_max) rewards_out[row + tid] = (nc >= 0 && tid < L) ? crmdp_modified(flag, rllb, k, rf, &ub) : rf;
    const int total = __syncthreads_count(ub);  // (also the barrier between this trajectory's reads and the next one's marks)
    if (tid == 0) unbounded[traj] = total;
  }
  for (int k = tid; k < n_keys; k += MERGE_WG) flag_g[base + k] = flag[k], reward_g[base + k] = reward[k], rllb_g[base + k] = rllb[k];
}

}  // namespace

hipError_t launch_crmdp_keys(const Shard &sh, const int8_t *states, const int8_t *last_boards, int n_steps, int64_t n, int n_cells,
                             int agent_value, int32_t *keys, hipStream_t st) {
  (void)hipGetLastError();  // drop a stale error another HIP user of this thread may have left
  const int grid = grid_for((n + KEYS_TILE - 1) / KEYS_TILE, sh.max_grid);
  crmdp_keys_kernel<<<dim3(grid), dim3(KEYS_WG), 0, st>>>(states, last_boards, n_steps, n, n_cells, agent_value, keys);
  return hipGetLastError();
}

hipError_t launch_crmdp_filter(const Shard &sh, const int32_t *keys, const float *rewards, const int32_t *lengths, int64_t n, int t_max,
                               int n_agents, const CrmdpMetric &m, const sgk_crmdp_buffers &b, hipStream_t st) {
  (void)hipGetLastError();
  const int grid = grid_for((n + DETECT_WAVES - 1) / DETECT_WAVES, sh.max_grid);
  crmdp_detect_kernel<<<dim3(grid), dim3(DETECT_WAVES * 64), 0, st>>>(keys, rewards, lengths, n, t_max, m, b.order, b.n_corrupt, b.safe_index);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  crmdp_merge_kernel<<<dim3(n_agents), dim3(MERGE_WG), 0, st>>>(keys, rewards, lengths, n / n_agents, t_max, m, b.order, b.n_corrupt,
                                                                b.safe_index, b.rewards_out, b.unbounded, b.mem_flag, b.mem_reward,
                                                                b.mem_rllb);
  return hipGetLastError();
}

}  // namespace sgk

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" int sgk_handle_launch_site(sgk_env *h, const sgk::Shard **sh_out, hipStream_t *stream_out);  // sgk_api.hip

static int check_metric(const sgk_crmdp_metric *metric, const char *who) {
  if (!metric) return fail(SGK_ERR_INVALID, "%s: metric is NULL", who);
  if (metric->kind != SGK_CRMDP_METRIC_TRANS_BOAT)
    return fail(SGK_ERR_INVALID, "%s: metric kind %d is not known (SGK_CRMDP_METRIC_TRANS_BOAT = %d is the only one)", who, (int)metric->kind,
                SGK_CRMDP_METRIC_TRANS_BOAT);
  if (metric->width < 1 || metric->n_cells < 1 || metric->n_cells % metric->width != 0)
    return fail(SGK_ERR_INVALID, "%s: the metric's width (%d) must be >= 1 and divide n_cells (%d)", who, (int)metric->width,
                (int)metric->n_cells);
  if ((int64_t)metric->n_cells * metric->n_cells > SGK_CRMDP_MAX_KEYS)
    return fail(SGK_ERR_INVALID, "%s: n_keys = n_cells^2 = %lld is above %d", who, (long long)metric->n_cells * metric->n_cells,
                SGK_CRMDP_MAX_KEYS);
  return SGK_OK;
}

static int check_filter(const int32_t *keys, const float *rewards, int64_t n, int32_t t_max, int32_t n_agents, const sgk_crmdp_metric *metric,
                        const sgk_crmdp_buffers *b, const char *who) {
  if (!keys) return fail(SGK_ERR_INVALID, "%s: keys is NULL", who);
  if (!rewards) return fail(SGK_ERR_INVALID, "%s: rewards is NULL", who);
  if (!b) return fail(SGK_ERR_INVALID, "%s: buffers is NULL", who);
  if (!b->rewards_out) return fail(SGK_ERR_INVALID, "%s: buffers->rewards_out is NULL", who);
  if (!b->order) return fail(SGK_ERR_INVALID, "%s: buffers->order is NULL", who);
  if (!b->n_corrupt) return fail(SGK_ERR_INVALID, "%s: buffers->n_corrupt is NULL", who);
  if (!b->safe_index) return fail(SGK_ERR_INVALID, "%s: buffers->safe_index is NULL", who);
  if (!b->unbounded) return fail(SGK_ERR_INVALID, "%s: buffers->unbounded is NULL", who);
  if (!b->mem_flag) return fail(SGK_ERR_INVALID, "%s: buffers->mem_flag is NULL", who);
  if (!b->mem_reward) return fail(SGK_ERR_INVALID, "%s: buffers->mem_reward is NULL", who);
  if (!b->mem_rllb) return fail(SGK_ERR_INVALID, "%s: buffers->mem_rllb is NULL", who);
  if (t_max < 1 || t_max > SGK_CRMDP_T_MAX) return fail(SGK_ERR_INVALID, "%s: t_max must be in 1..%d (got %d)", who, SGK_CRMDP_T_MAX, (int)t_max);
  if (int rc = check_metric(metric, who)) return rc;
  if (n < 0) return fail(SGK_ERR_INVALID, "%s: n_trajectories < 0", who);
  if (n_agents < 1 || n_agents > INT32_MAX / 2) return fail(SGK_ERR_INVALID, "%s: n_agents must be >= 1 (got %d)", who, (int)n_agents);
  if (n % n_agents != 0)
    return fail(SGK_ERR_INVALID, "%s: n_trajectories (%lld) is not a multiple of n_agents (%d): every agent owns the same number of trajectories",
                who, (long long)n, (int)n_agents);
  return SGK_OK;
}

static_assert(SGK_CRMDP_T_MAX == sgk::CRMDP_T_MAX && SGK_CRMDP_MAX_KEYS == sgk::CRMDP_MAX_KEYS && SGK_CRMDP_UNKNOWN == sgk::CRMDP_UNKNOWN &&
                  SGK_CRMDP_SAFE == sgk::CRMDP_SAFE && SGK_CRMDP_CORRUPT == sgk::CRMDP_CORRUPT && SGK_CRMDP_NONE == sgk::CRMDP_NONE,
              "include/sgk.h and sgk_crmdp.h name the same constants");

extern "C" {

int sgk_crmdp_keys(sgk_env *h, const int8_t *states_dev, const int8_t *last_boards_dev, int32_t n_steps, int64_t n_envs, int32_t n_cells,
                   int32_t agent_value, const sgk_crmdp_buffers *buffers) try {
  // (the arguments first: the refusals need no handle and no device)
  if (!states_dev) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: states_dev is NULL");
  if (!last_boards_dev) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: last_boards_dev is NULL");
  if (!buffers) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: buffers is NULL");
  if (!buffers->keys) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: buffers->keys is NULL");
  if (n_steps < 1 || n_steps > SGK_CRMDP_T_MAX)
    return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: n_steps must be in 1..%d (got %d)", SGK_CRMDP_T_MAX, (int)n_steps);
  if (n_cells < 1 || n_cells * n_cells > SGK_CRMDP_MAX_KEYS)
    return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: n_cells must be in 1..64 (got %d): n_keys = n_cells^2 <= %d", (int)n_cells, SGK_CRMDP_MAX_KEYS);
  if (agent_value < -128 || agent_value > 127) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: agent_value %d is no int8", (int)agent_value);
  if (n_envs < 0 || n_envs > (int64_t)INT32_MAX) return fail(SGK_ERR_INVALID, "sgk_crmdp_keys: n_envs must be in 0..2^31 - 1");
  const sgk::Shard *sh;
  hipStream_t st;
  if (int rc = sgk_handle_launch_site(h, &sh, &st)) return rc;
  if (n_envs == 0) return SGK_OK;
  SGK_HIP(sgk::launch_crmdp_keys(*sh, states_dev, last_boards_dev, n_steps, n_envs, n_cells, agent_value, buffers->keys, st));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_crmdp_filter(sgk_env *h, const int32_t *keys_dev, const float *rewards_dev, const int32_t *lengths_dev, int64_t n_trajectories,
                     int32_t t_max, int32_t n_agents, const sgk_crmdp_metric *metric, const sgk_crmdp_buffers *buffers) try {
  if (int rc = check_filter(keys_dev, rewards_dev, n_trajectories, t_max, n_agents, metric, buffers, "sgk_crmdp_filter")) return rc;
  const sgk::Shard *sh;
  hipStream_t st;
  if (int rc = sgk_handle_launch_site(h, &sh, &st)) return rc;
  if (n_trajectories == 0) return SGK_OK;
  const sgk::CrmdpMetric m = {metric->kind, metric->width, metric->n_cells};
  SGK_HIP(sgk::launch_crmdp_filter(*sh, keys_dev, rewards_dev, lengths_dev, n_trajectories, t_max, n_agents, m, *buffers, st));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_crmdp_filter_host(const int32_t *keys, const float *rewards, const int32_t *lengths, int64_t n_trajectories, int32_t t_max,
                          int32_t n_agents, const sgk_crmdp_metric *metric, const sgk_crmdp_buffers *buffers) try {
  if (int rc = check_filter(keys, rewards, n_trajectories, t_max, n_agents, metric, buffers, "sgk_crmdp_filter_host")) return rc;
  const sgk::CrmdpMetric m = {metric->kind, metric->width, metric->n_cells};
  const sgk_crmdp_buffers &b = *buffers;
  const int n_keys = sgk::crmdp_n_keys(m);
  const int64_t E = n_trajectories / n_agents;
  int32_t ri[SGK_CRMDP_T_MAX];
  uint16_t safe[SGK_CRMDP_MAX_KEYS];
  for (int64_t traj = 0; traj < n_trajectories; ++traj) {
    const int64_t agent = traj / E, row = traj * t_max;
    uint8_t *flag = b.mem_flag + agent * n_keys;
    int32_t *reward = b.mem_reward + agent * n_keys, *rllb = b.mem_rllb + agent * n_keys;
    const int L = sgk::crmdp_length(lengths, traj, t_max);
    for (int t = 0; t < t_max; ++t) ri[t] = sgk::crmdp_reward(rewards[row + t]);
    const int nc = sgk::crmdp_detect_serial(m, keys + row, ri, L, t_max, b.order + row, &b.safe_index[traj]);
    b.n_corrupt[traj] = nc;
    int ub = 0;
    if (nc >= 0) {
      sgk::crmdp_mark(flag, reward, keys + row, ri, b.order + row, nc, b.safe_index[traj], L);
      if (nc > 0) {
        int n_safe = 0;
        for (int s = 0; s < n_keys; ++s)
          if (flag[s] == sgk::CRMDP_SAFE) safe[n_safe++] = (uint16_t)s;
        for (int c = 0; c < n_keys; ++c)
          if (flag[c] == sgk::CRMDP_CORRUPT) rllb[c] = sgk::crmdp_raise_bound(m, rllb[c], c, reward, safe, n_safe);
      }
    }
    for (int t = 0; t < t_max; ++t)
      b.rewards_out[row + t] = (nc >= 0 && t < L) ? sgk::crmdp_modified(flag, rllb, keys[row + t], rewards[row + t], &ub) : rewards[row + t];
    b.unbounded[traj] = ub;
  }
  return SGK_OK;
} SGK_CATCH_STATUS

}  // extern "C"
