// sgk_members.hip -- population-based training on the device (include/sgk.h: sgk_members_select, sgk_members_clone): "member d becomes
// member s" over a population's stacked [n_members][...] tensors. Two kernels and their entry points:
//   members_select_kernel  one workgroup: ranks the members by counting against the scores in LDS, names every member's source and,
//                          optionally, writes the replaced members' perturbed hyper-parameter rows (the explore step)
//   members_clone_kernel   grid (chunks, n_members): the workgroups of a replaced member copy its source's slabs over its own, tensor
//                          by tensor, from descriptors that arrive as kernel arguments
// and the ensemble's vote (sgk_members_vote) over the [n_members][n_envs] actions of sgk_policy_act_members_all (sgk_policy.hip):
//   members_vote_kernel    one lane per env counts the voters' action bytes, names the first action with the most votes and adds the
//                          live envs' dissent to two global counters
// The arithmetic both sides of the C-ABI share (the order, the coin, the perturbed value) is sgk_members.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sgk_device.h"
#include "sgk_host_core.h"
#include "sgk_kernels.h"
#include "sgk_members.h"

using sgk::host::fail;

namespace sgk {

namespace {

constexpr int SELECT_WG = 1024;
constexpr int SELECT_PER_LANE = SGK_MEMBERS_MAX / SELECT_WG;  // members a lane ranks at most (the kernel is instantiated for 1, 2 and 4)
constexpr int CLONE_WG = 256;
constexpr int VOTE_WG = 256;

// One workgroup. LDS: the scores (32 KB) and the order (16 KB) of up to 4096 members. A lane ranks the members tid, tid + 1024, ...
// in ONE pass over the scores (every lane reads the same score: an LDS broadcast), scatters order[rank] = member, and after the
// barrier the lane that holds rank r writes src of the member at rank r -- every element of src_out is written once, by one lane.
// PER: the members a lane ranks, ceil(n_members / 1024) rounded up to 1, 2 or 4 -- the pass costs PER comparisons per score and lane.
template <int PER>
__global__ __launch_bounds__(SELECT_WG) void members_select_kernel(const double *__restrict__ scores, int n_members, int n_replace,
                                                                   int32_t *__restrict__ src_out, int with_explore, MembersExplore ex) {
  __shared__ double s[SGK_MEMBERS_MAX];
  __shared__ int32_t order[SGK_MEMBERS_MAX];
  const int tid = threadIdx.x, M = n_members;
  const uint64_t generation = with_explore ? (uint64_t)*ex.generation : 0;  // (read before the barriers, stored after the last)
  for (int m = tid; m < M; m += SELECT_WG) s[m] = members_score(scores[m]);
  __syncthreads();
  double mine[PER];
  int rank[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int m = tid + i * SELECT_WG;
    mine[i] = m < M ? s[m] : 0.0;
    rank[i] = 0;
  }
  if ((tid & ~63) < M) {  // (a wave without a member skips the pass and leaves the SIMD's issue slots to the waves that have some)
#pragma unroll 8
    for (int j = 0; j < M; ++j) {  // (unrolled: the LDS reads of eight scores are in flight together)
      const double sj = s[j];
#pragma unroll
      for (int i = 0; i < PER; ++i) rank[i] += members_above(sj, j, mine[i], tid + i * SELECT_WG) ? 1 : 0;
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int m = tid + i * SELECT_WG;
    if (m < M) order[rank[i]] = m;  // (a total order: the ranks of the M members are a permutation of 0 .. M - 1)
  }
  __syncthreads();
  for (int r = tid; r < M; r += SELECT_WG) {
    const int m = order[r];
    src_out[m] = r >= M - n_replace ? order[M - 1 - r] : m;
  }
  if (!with_explore) return;
  const int C = ex.n_columns;
  for (int idx = tid; idx < n_replace * C; idx += SELECT_WG) {
    const int i = idx / C, k = idx - i * C;
    const int d = order[M - 1 - i], src = order[i];  // (d is in the bottom n_replace, src in the top: rows of sources are never written)
    double v = ex.hyper[(size_t)src * C + k];
    if ((ex.mask >> k) & 1u) {
      const double f = members_explore_pick(ex.key, generation, (uint32_t)d, (uint32_t)k) ? ex.factor_up : ex.factor_down;
      v = members_perturb(v, f, ex.lo[k], ex.hi[k]);
    }
    ex.hyper[(size_t)d * C + k] = v;
  }
  __syncthreads();
  if (tid == 0) *ex.generation = (long long)(generation + 1);
}

template <class T>
__device__ __forceinline__ void copy_tiles(const char *src, char *dst, uint64_t units, uint32_t first_tile, uint32_t chunks) {
  const T *__restrict__ s = reinterpret_cast<const T *>(src);
  T *__restrict__ d = reinterpret_cast<T *>(dst);
  for (uint64_t i = (uint64_t)first_tile * CLONE_WG + threadIdx.x; i < units; i += (uint64_t)chunks * CLONE_WG) d[i] = s[i];
}

// grid (chunks, n_members), 256 lanes. The member's tensors are cut into tiles of 256 lane-units (16 bytes where the tensor's base and
// slab size allow, else 4) and the tiles of ALL its tensors are dealt round-robin to the member's `chunks` workgroups, so the many
// small tensors (biases, the step counter) do not all land on workgroup 0. Everything but the lane's unit index is wave-uniform.
__global__ __launch_bounds__(CLONE_WG) void members_clone_kernel(const MembersCloneArgs a) {
  const int d = blockIdx.y, M = a.n_members;
  const int sm = a.src[d];
  if (sm == d) return;
  if (sm < 0 || sm >= M || a.src[sm] != sm) {  // no member, or a source that is itself being overwritten: copy nothing, say so
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.status = *a.status | SGK_MEMBERS_BAD_SOURCE;
    return;
  }
  const uint32_t chunks = gridDim.x, c = blockIdx.x;
  uint32_t dealt = 0;  // tiles of the earlier tensors, mod chunks: the next tile goes to workgroup `dealt`
  for (int t = 0; t < a.n_tensors; ++t) {
    char *base = a.t[t].base;
    const uint64_t bytes = a.t[t].bytes;
    const bool wide = (((uint64_t)(uintptr_t)base | bytes) & 15u) == 0;
    const uint64_t units = wide ? bytes >> 4 : bytes >> 2;
    const uint32_t first = (c + chunks - dealt) % chunks;  // this workgroup's first tile of the tensor
    const char *from = base + (uint64_t)sm * bytes;
    char *to = base + (uint64_t)d * bytes;
    if (wide) copy_tiles<uint4>(from, to, units, first, chunks);
    else copy_tiles<uint32_t>(from, to, units, first, chunks);
    dealt = (uint32_t)((dealt + (units + CLONE_WG - 1) / CLONE_WG) % chunks);
  }
}

// One lane per env, grid-stride. Voter i is member ids[i] (null: member i) -- wave-uniform, so the voter loop's only vector load is the
// action byte: row m of member_actions [n_members][n] is contiguous across the lanes (64 bytes a wave). An id outside 0 .. n_members - 1
// casts no vote. The four counts travel as one word (sgk_members.h) and are stored as the env's 8-byte row of votes_out. dissent gains
// {voters that did not vote for the winner, votes cast} over the envs whose episode is not over: per-lane sums, a wavefront reduction
// after the loop, then one atomic instruction per wave (lane c adds counter c) -- skipped by a wave whose envs were all over.
__global__ __launch_bounds__(VOTE_WG) void members_vote_kernel(const uint8_t *__restrict__ member_actions, int n_members,
                                                               const int32_t *__restrict__ ids, int n_voters, int64_t n,
                                                               const uint64_t *__restrict__ state, uint8_t *__restrict__ actions_out,
                                                               uint64_t *__restrict__ votes_out, unsigned long long *__restrict__ dissent) {
  long long lost = 0, cast = 0;
  for (int64_t env = (int64_t)blockIdx.x * VOTE_WG + threadIdx.x; env < n; env += (int64_t)gridDim.x * VOTE_WG) {
    uint64_t counts = 0;
#pragma unroll 4
    for (int i = 0; i < n_voters; ++i) {
      const int m = ids ? ids[i] : i;
      if ((unsigned)m < (unsigned)n_members) counts = members_vote_cast(counts, member_actions[(size_t)m * (size_t)n + (size_t)env]);
    }
    const int winner = members_vote_winner(counts);
    actions_out[env] = (uint8_t)winner;
    if (votes_out) votes_out[env] = counts;
    if (dissent && !unpack_state(state[env]).over) {
      const uint32_t total = members_vote_total(counts);
      lost += total - members_vote_count(counts, winner);
      cast += total;
    }
  }
  if (!dissent) return;  // (uniform: a kernel argument)
  lost = wave_sum64(lost);
  cast = wave_sum64(cast);
  const int c = threadIdx.x & 63;
  if (c < 2 && cast > 0) atomicAdd(&dissent[c], (unsigned long long)(c == 0 ? lost : cast));
}

}  // namespace

hipError_t launch_members_select(const double *scores, int n_members, int n_replace, int32_t *src_out, const MembersExplore *explore,
                                 hipStream_t st) {
  (void)hipGetLastError();  // drop a stale error another HIP user of this thread may have left
  MembersExplore ex = {};
  if (explore) ex = *explore;
  const int with_explore = explore ? 1 : 0;
  if (n_members <= SELECT_WG)
    members_select_kernel<1><<<dim3(1), dim3(SELECT_WG), 0, st>>>(scores, n_members, n_replace, src_out, with_explore, ex);
  else if (n_members <= 2 * SELECT_WG)
    members_select_kernel<2><<<dim3(1), dim3(SELECT_WG), 0, st>>>(scores, n_members, n_replace, src_out, with_explore, ex);
  else
    members_select_kernel<SELECT_PER_LANE><<<dim3(1), dim3(SELECT_WG), 0, st>>>(scores, n_members, n_replace, src_out, with_explore, ex);
  return hipGetLastError();
}

// chunks: workgroups per member. A quarter of the members replaced is PBT's usual step, so n_members / 4 members have work; four
// workgroups per CU from them (16 waves a CU: enough loads in flight to cover HBM latency with a handful of 16-byte loads per lane)
// is the aim, within 4 .. 64 -- a ppo-mlp member of H = 100 is ~80 tiles, so 64 workgroups still get a tile each.
static int clone_chunks(int n_cus, int n_members) {
  const int busy = n_members / 4 > 0 ? n_members / 4 : 1;
  const int chunks = (4 * n_cus + busy - 1) / busy;
  return chunks < 4 ? 4 : (chunks > 64 ? 64 : chunks);
}

hipError_t launch_members_clone(const Shard &sh, const MembersCloneArgs &a, hipStream_t st) {
  (void)hipGetLastError();
  members_clone_kernel<<<dim3(clone_chunks(sh.n_cus, a.n_members), a.n_members), dim3(CLONE_WG), 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_members_vote(const Shard &sh, const uint8_t *member_actions, int n_members, const int32_t *ids, int n_voters,
                               uint8_t *actions_out, uint16_t *votes_out, int64_t *dissent, hipStream_t st) {
  (void)hipGetLastError();
  const int grid = grid_for((sh.n + VOTE_WG - 1) / VOTE_WG, sh.max_grid);
  members_vote_kernel<<<dim3(grid), dim3(VOTE_WG), 0, st>>>(member_actions, n_members, ids, n_voters, sh.n, sh.state, actions_out,
                                                            reinterpret_cast<uint64_t *>(votes_out),
                                                            reinterpret_cast<unsigned long long *>(dissent));
  return hipGetLastError();
}

}  // namespace sgk

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" int sgk_handle_launch_site(sgk_env *h, const sgk::Shard **sh_out, hipStream_t *stream_out);  // sgk_api.hip

static int check_select(const double *scores, int32_t n_members, int32_t n_replace, const int32_t *src_out, const char *who) {
  if (!scores) return fail(SGK_ERR_INVALID, "%s: scores is NULL", who);
  if (!src_out) return fail(SGK_ERR_INVALID, "%s: src_out is NULL", who);
  if (n_members < 1 || n_members > SGK_MEMBERS_MAX)
    return fail(SGK_ERR_INVALID, "%s: n_members must be in 1..%d (got %d)", who, SGK_MEMBERS_MAX, (int)n_members);
  if (n_replace < 0 || n_replace > n_members / 2)
    return fail(SGK_ERR_INVALID, "%s: n_replace must be in 0..n_members / 2 = %d (got %d): the replaced and their sources are disjoint",
                who, (int)(n_members / 2), (int)n_replace);
  return SGK_OK;
}

// sgk_members_vote and sgk_members_vote_host: the voters are all members (ids NULL, n_voters 0 or n_members) or the n_voters listed
static int check_vote(const uint8_t *member_actions, int32_t n_members, const int32_t *ids, int32_t n_voters, const uint8_t *actions_out,
                      const uint16_t *votes_out, const char *who) {
  if (!member_actions) return fail(SGK_ERR_INVALID, "%s: member_actions is NULL", who);
  if (!actions_out) return fail(SGK_ERR_INVALID, "%s: actions_out is NULL", who);
  if (n_members < 1 || n_members > SGK_MEMBERS_MAX)
    return fail(SGK_ERR_INVALID, "%s: n_members must be in 1..%d (got %d)", who, SGK_MEMBERS_MAX, (int)n_members);
  if (!ids && n_voters != 0 && n_voters != n_members)
    return fail(SGK_ERR_INVALID, "%s: without member_ids every member votes: n_voters must be 0 or n_members = %d (got %d)", who,
                (int)n_members, (int)n_voters);
  if (ids && (n_voters < 1 || n_voters > n_members))
    return fail(SGK_ERR_INVALID, "%s: n_voters must be in 1..n_members = %d (got %d)", who, (int)n_members, (int)n_voters);
  if ((uintptr_t)votes_out & 7u) return fail(SGK_ERR_INVALID, "%s: votes_out must be 8-byte aligned (one env's four counts are stored at once)", who);
  return SGK_OK;
}

extern "C" {

int sgk_members_select(sgk_env *h, const double *scores_dev, int32_t n_members, int32_t n_replace, int32_t *src_out_dev,
                       const sgk_members_explore *explore) try {
  // (the arguments first: the refusals need no handle and no device)
  if (int rc = check_select(scores_dev, n_members, n_replace, src_out_dev, "sgk_members_select")) return rc;
  sgk::MembersExplore ex = {};
  if (explore) {
    if (!explore->hyper_dev) return fail(SGK_ERR_INVALID, "sgk_members_select: explore->hyper_dev is NULL");
    if (!explore->generation_dev) return fail(SGK_ERR_INVALID, "sgk_members_select: explore->generation_dev is NULL");
    if (explore->n_columns < 1 || explore->n_columns > SGK_MEMBERS_MAX_COLUMNS)
      return fail(SGK_ERR_INVALID, "sgk_members_select: n_columns must be in 1..%d (got %d)", SGK_MEMBERS_MAX_COLUMNS, (int)explore->n_columns);
    for (double f : {explore->factor_down, explore->factor_up})
      if (!std::isfinite(f) || !(f > 0.0)) return fail(SGK_ERR_INVALID, "sgk_members_select: a factor must be finite and > 0 (got %g)", f);
    for (int k = 0; k < explore->n_columns; ++k)
      if (!(explore->lo[k] <= explore->hi[k]))  // (false for a NaN bound too)
        return fail(SGK_ERR_INVALID, "sgk_members_select: the bounds of column %d need lo <= hi, neither a NaN (got %g, %g)", k, explore->lo[k],
                    explore->hi[k]);
    ex.hyper = explore->hyper_dev;
    ex.n_columns = explore->n_columns;
    ex.mask = explore->perturb_mask & ((1u << explore->n_columns) - 1u);
    ex.factor_down = explore->factor_down;
    ex.factor_up = explore->factor_up;
    for (int k = 0; k < 8; ++k) ex.lo[k] = explore->lo[k], ex.hi[k] = explore->hi[k];
    ex.key = explore->key;
    ex.generation = reinterpret_cast<long long *>(explore->generation_dev);
  }
  const sgk::Shard *sh;
  hipStream_t st;
  if (int rc = sgk_handle_launch_site(h, &sh, &st)) return rc;
  SGK_HIP(sgk::launch_members_select(scores_dev, n_members, n_replace, src_out_dev, explore ? &ex : nullptr, st));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_members_clone(sgk_env *h, const int32_t *src_dev, int32_t n_members, const sgk_members_tensor *descs, int32_t n_tensors,
                      int32_t *status_dev) try {
  if (!src_dev) return fail(SGK_ERR_INVALID, "sgk_members_clone: src_dev is NULL");
  if (!status_dev) return fail(SGK_ERR_INVALID, "sgk_members_clone: status_dev is NULL");
  if (n_members < 1 || n_members > SGK_MEMBERS_MAX)
    return fail(SGK_ERR_INVALID, "sgk_members_clone: n_members must be in 1..%d (got %d)", SGK_MEMBERS_MAX, (int)n_members);
  if (n_tensors < 0 || n_tensors > SGK_MEMBERS_MAX_TENSORS)
    return fail(SGK_ERR_INVALID, "sgk_members_clone: n_tensors must be in 0..%d (got %d): split the list over several calls",
                SGK_MEMBERS_MAX_TENSORS, (int)n_tensors);
  if (n_tensors > 0 && !descs) return fail(SGK_ERR_INVALID, "sgk_members_clone: descs is NULL");
  sgk::MembersCloneArgs a = {};
  a.src = src_dev, a.status = status_dev, a.n_members = n_members, a.n_tensors = n_tensors;
  for (int t = 0; t < n_tensors; ++t) {
    if (!descs[t].base) return fail(SGK_ERR_INVALID, "sgk_members_clone: descs[%d].base is NULL", t);
    if ((uintptr_t)descs[t].base & 3u) return fail(SGK_ERR_INVALID, "sgk_members_clone: descs[%d].base is not 4-byte aligned", t);
    if (descs[t].bytes_per_member & 3u)
      return fail(SGK_ERR_INVALID, "sgk_members_clone: descs[%d].bytes_per_member = %llu is no multiple of 4", t,
                  (unsigned long long)descs[t].bytes_per_member);
    a.t[t].base = static_cast<char *>(descs[t].base);
    a.t[t].bytes = descs[t].bytes_per_member;
  }
  const sgk::Shard *sh;
  hipStream_t st;
  if (int rc = sgk_handle_launch_site(h, &sh, &st)) return rc;
  if (n_tensors == 0) return SGK_OK;
  SGK_HIP(sgk::launch_members_clone(*sh, a, st));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_members_select_host(const double *scores, int32_t n_members, int32_t n_replace, int32_t *src_out) try {
  if (int rc = check_select(scores, n_members, n_replace, src_out, "sgk_members_select_host")) return rc;
  const int M = n_members;
  int32_t order[SGK_MEMBERS_MAX];
  for (int m = 0; m < M; ++m) {
    const double sm = sgk::members_score(scores[m]);
    int rank = 0;
    for (int j = 0; j < M; ++j) rank += sgk::members_above(sgk::members_score(scores[j]), j, sm, m) ? 1 : 0;
    order[rank] = m;
  }
  for (int r = 0; r < M; ++r) src_out[order[r]] = r >= M - n_replace ? order[M - 1 - r] : order[r];
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_members_vote(sgk_env *h, const uint8_t *member_actions_dev, int32_t n_members, const int32_t *member_ids_dev, int32_t n_voters,
                     uint8_t *actions_out_dev, uint16_t *votes_out_dev, int64_t *dissent_dev) try {
  // (the arguments first: the refusals need no handle and no device)
  if (int rc = check_vote(member_actions_dev, n_members, member_ids_dev, n_voters, actions_out_dev, votes_out_dev, "sgk_members_vote")) return rc;
  if ((uintptr_t)dissent_dev & 7u) return fail(SGK_ERR_INVALID, "sgk_members_vote: dissent_dev must be 8-byte aligned");
  const sgk::Shard *sh;
  hipStream_t st;
  if (int rc = sgk_handle_launch_site(h, &sh, &st)) return rc;
  SGK_HIP(sgk::launch_members_vote(*sh, member_actions_dev, n_members, member_ids_dev, member_ids_dev ? n_voters : n_members, actions_out_dev,
                                   votes_out_dev, dissent_dev, st));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_members_vote_host(const uint8_t *member_actions, int32_t n_members, int64_t n_envs, const int32_t *member_ids, int32_t n_voters,
                          const uint8_t *live, uint8_t *actions_out, uint16_t *votes_out, int64_t *dissent) try {
  if (int rc = check_vote(member_actions, n_members, member_ids, n_voters, actions_out, votes_out, "sgk_members_vote_host")) return rc;
  if (n_envs < 0) return fail(SGK_ERR_INVALID, "sgk_members_vote_host: n_envs < 0");
  const int voters = member_ids ? n_voters : n_members;
  long long lost = 0, cast = 0;
  for (int64_t env = 0; env < n_envs; ++env) {
    uint64_t counts = 0;
    for (int i = 0; i < voters; ++i) {
      const int m = member_ids ? member_ids[i] : i;
      if ((unsigned)m < (unsigned)n_members) counts = sgk::members_vote_cast(counts, member_actions[(size_t)m * (size_t)n_envs + (size_t)env]);
    }
    const int winner = sgk::members_vote_winner(counts);
    actions_out[env] = (uint8_t)winner;
    if (votes_out)
      for (int a = 0; a < 4; ++a) votes_out[env * 4 + a] = (uint16_t)sgk::members_vote_count(counts, a);
    if (dissent && (!live || live[env])) {
      const uint32_t total = sgk::members_vote_total(counts);
      lost += total - sgk::members_vote_count(counts, winner);
      cast += total;
    }
  }
  if (dissent) dissent[0] += lost, dissent[1] += cast;
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_members_explore_pick(uint64_t key, int64_t generation, int32_t member, int32_t column) try {
  return sgk::members_explore_pick(key, (uint64_t)generation, (uint32_t)member, (uint32_t)column);
} SGK_CATCH_STATUS

}  // extern "C"
