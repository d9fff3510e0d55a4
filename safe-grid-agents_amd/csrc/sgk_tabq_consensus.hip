// sgk_tabq_consensus.hip -- what N private tabular-Q agents recommend TOGETHER (include/sgk.h: sgk_tabq_consensus, sgk_tabq_load_shared,
// sgk_tabq_consensus_host). The tables are state-major, table[state][agent][4] float64 (sgk_tabq.hip: row_of), so the N rows of one
// state are one contiguous run of 32 * N bytes; both kernels stream over them once:
//   tabq_vote_kernel    one lane = one agent: its row (two 16-byte loads), its first-max argmax and whether the row holds anything but
//                       zeros; a ballot + popcount per action combines the wave's lanes in scalar registers, the four waves of the
//                       workgroup meet in LDS, and the workgroup adds its four counts to votes[state][.] -- plain stores where one
//                       workgroup covers the whole state, at most four 64-bit atomics where several share it
//   tabq_voters_kernel  voters[state] = the sum of votes[state][.] (only behind the shared-state form; the other writes it itself)
//   tabq_load_kernel    the mirror: every agent's row of a state := the shared table's row, 16-byte stores, a wave's 1 KB contiguous
// The counts are integers: the result does not depend on the grid's shape or on the order of the atomics.
// The vote's rule (vote_of_row, sgk_tabq_vote.h) is shared with the host restatement below, which needs no GPU, and with the hashed
// levels' vote by board key (sgk_tabq_hash_consensus.hip).
#include <hip/hip_runtime.h>

#include "sgk_host_core.h"
#include "sgk_kernels.h"
#include "sgk_tabq_vote.h"

using sgk::host::fail;

namespace sgk {

namespace {

constexpr int VOTE_WG = 256;           // four waves
constexpr int VOTE_UNROLL = 4;         // rows a lane has in flight: 8 x 16 bytes
constexpr int64_t VOTE_TARGET_WGS = 2048;  // 256 CUs x 8 resident workgroups: what a 25-state level and a 1 296-state level both reach

// How the (state, agent) plane is cut into workgroups: `chunks` workgroups per state, each a run of `per` agents -- a whole number of
// the workgroup's passes (256 lanes x 4 rows in flight = 1 024 agents), so every pass but the batch's last is full and every wave's 64
// rows stay one aligned 2 KB piece. Few states: many chunks per state; many states, or a state's run of one pass: one chunk, and then
// the workgroup stores the state's counts itself (one launch, no atomics).
struct VoteGrid {
  int64_t per = 0;
  int chunks = 0;
  int64_t blocks = 0;
};
VoteGrid vote_grid(int64_t n, int64_t n_states) {
  VoteGrid g;
  constexpr int64_t PASS = (int64_t)VOTE_WG * VOTE_UNROLL;
  const int64_t passes = (n + PASS - 1) / PASS;  // passes one state's run takes
  int64_t chunks = (VOTE_TARGET_WGS + n_states - 1) / n_states;
  if (chunks > passes) chunks = passes;
  if (chunks < 1) chunks = 1;
  const int64_t passes_per = (passes + chunks - 1) / chunks;
  g.per = passes_per * PASS;
  g.chunks = (int)((passes + passes_per - 1) / passes_per);  // (no chunk without an agent)
  g.blocks = n_states * (int64_t)g.chunks;
  return g;
}

template <bool SHARED_STATE>
__global__ __launch_bounds__(VOTE_WG) void tabq_vote_kernel(const double *__restrict__ table, const uint8_t *__restrict__ mask, int64_t n,
                                                            int64_t per, int chunks, unsigned long long *__restrict__ votes,
                                                            unsigned long long *__restrict__ voters) {
  __shared__ unsigned long long part[VOTE_WG / 64][4];
  const int tid = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x / chunks, c = (int64_t)blockIdx.x % chunks;
  const int64_t begin = c * per, end = begin + per < n ? begin + per : n;
  const double2 *__restrict__ plane = reinterpret_cast<const double2 *>(table + s * n * 4);  // this state's N rows
  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;  // wave-uniform: the wave's votes per action
  for (int64_t base = begin; base < end; base += VOTE_WG * VOTE_UNROLL) {  // (workgroup-uniform trip count: every lane reaches the ballots)
    double2 q01[VOTE_UNROLL], q23[VOTE_UNROLL];
    bool may[VOTE_UNROLL];
#pragma unroll
    for (int u = 0; u < VOTE_UNROLL; ++u) {  // every load of the pass requested before the first is used
      const int64_t e = base + u * VOTE_WG + tid;
      may[u] = e < end;
      q01[u] = q23[u] = make_double2(0.0, 0.0);
      if (may[u]) {
        q01[u] = plane[2 * e];
        q23[u] = plane[2 * e + 1];
        if (mask) may[u] = mask[e] != 0;
      }
    }
#pragma unroll
    for (int u = 0; u < VOTE_UNROLL; ++u) {
      const int v = may[u] ? vote_of_row(q01[u].x, q01[u].y, q23[u].x, q23[u].y) : -1;
      c0 += (unsigned)__popcll(__ballot(v == 0));
      c1 += (unsigned)__popcll(__ballot(v == 1));
      c2 += (unsigned)__popcll(__ballot(v == 2));
      c3 += (unsigned)__popcll(__ballot(v == 3));
    }
  }
  if ((tid & 63) == 0) {
    unsigned long long *p = part[tid >> 6];
    p[0] = c0; p[1] = c1; p[2] = c2; p[3] = c3;
  }
  __syncthreads();
  if (tid < 4) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < VOTE_WG / 64; ++w) total += part[w][tid];
    if (SHARED_STATE) {
      if (total) atomicAdd(&votes[s * 4 + tid], total);  // (the counts were zeroed on the stream before the launch)
    } else {
      votes[s * 4 + tid] = total;
    }
  }
  if (!SHARED_STATE && voters && tid == 0) {
    unsigned long long all = 0;
#pragma unroll
    for (int w = 0; w < VOTE_WG / 64; ++w) all += part[w][0] + part[w][1] + part[w][2] + part[w][3];
    voters[s] = all;
  }
}

__global__ __launch_bounds__(VOTE_WG) void tabq_voters_kernel(const unsigned long long *__restrict__ votes, int64_t n_states,
                                                              unsigned long long *__restrict__ voters) {
  for (int64_t s = (int64_t)blockIdx.x * VOTE_WG + threadIdx.x; s < n_states; s += (int64_t)gridDim.x * VOTE_WG)
    voters[s] = votes[s * 4] + votes[s * 4 + 1] + votes[s * 4 + 2] + votes[s * 4 + 3];
}

__global__ __launch_bounds__(VOTE_WG) void tabq_load_kernel(double *__restrict__ table, const double *__restrict__ shared, int64_t n, int64_t per,
                                                            int chunks) {
  const int64_t s = (int64_t)blockIdx.x / chunks, c = (int64_t)blockIdx.x % chunks;
  const int64_t begin = c * per, end = begin + per < n ? begin + per : n;
  // (the shared row is read as four doubles: the caller's table need only be 8-byte aligned)
  const double2 r01 = make_double2(shared[s * 4], shared[s * 4 + 1]), r23 = make_double2(shared[s * 4 + 2], shared[s * 4 + 3]);
  double2 *__restrict__ plane = reinterpret_cast<double2 *>(table + s * n * 4);
  // the run as 16-byte halves of rows: a lane stores every 256th half, always the same half of a row (256 is even), so a wave's store is
  // 1 KB contiguous and whole lines leave together
  const double2 mine = (threadIdx.x & 1) ? r23 : r01;
  for (int64_t i = 2 * begin + threadIdx.x; i < 2 * end; i += VOTE_WG) plane[i] = mine;
}

}  // namespace

hipError_t launch_tabq_consensus(const double *table, int64_t n, int64_t n_states, const uint8_t *mask, int64_t *votes, int64_t *voters,
                                 hipStream_t st) {
  const VoteGrid g = vote_grid(n, n_states);
  unsigned long long *v = reinterpret_cast<unsigned long long *>(votes), *w = reinterpret_cast<unsigned long long *>(voters);
  (void)hipGetLastError();
  if (g.chunks == 1) {  // one workgroup per state: it stores the state's counts itself
    tabq_vote_kernel<false><<<dim3((unsigned)g.blocks), dim3(VOTE_WG), 0, st>>>(table, mask, n, g.per, g.chunks, v, w);
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(votes, 0, sizeof(int64_t) * 4 * (size_t)n_states, st);
  if (e != hipSuccess) return e;
  tabq_vote_kernel<true><<<dim3((unsigned)g.blocks), dim3(VOTE_WG), 0, st>>>(table, mask, n, g.per, g.chunks, v, nullptr);
  e = hipGetLastError();
  if (e != hipSuccess || !voters) return e;
  const int64_t blocks = (n_states + VOTE_WG - 1) / VOTE_WG;
  tabq_voters_kernel<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(VOTE_WG), 0, st>>>(v, n_states, w);
  return hipGetLastError();
}

hipError_t launch_tabq_load_shared(double *table, int64_t n, int64_t n_states, const double *shared, hipStream_t st) {
  const VoteGrid g = vote_grid(n, n_states);
  (void)hipGetLastError();
  tabq_load_kernel<<<dim3((unsigned)g.blocks), dim3(VOTE_WG), 0, st>>>(table, shared, n, g.per, g.chunks);
  return hipGetLastError();
}

}  // namespace sgk

extern "C" int sgk_handle_launch_site(sgk_env *h, const sgk::Shard **sh_out, hipStream_t *stream_out);  // sgk_api.hip

namespace {

// The handle's definition is private to sgk_api.hip; these are its first two members. What this file reads through the view is
// checked against what the public accessor answers (site_of), so a handle whose layout has moved is refused, not misread.
struct TabqHandleHead {
  sgk_env *env;
  sgk::TabqShard tq;
};

struct TabqSite {
  const sgk::Shard *sh = nullptr;
  hipStream_t stream = nullptr;
  double *table = nullptr;
  int64_t n_states = 0;
};

// the handle's checks; its env's shard and current stream; its table. (sgk_tabq_table_dev also tells the per-step kernels to forget
// the rows they keep: needed behind a load, harmless behind a vote -- the table is written through, a re-read row is the same row.)
int site_of(sgk_tabq *q, const char *who, TabqSite *out) {
  int64_t n_actions = 0;
  if (int rc = sgk_tabq_table_dev(q, &out->table, &out->n_states, &n_actions)) return rc;
  const TabqHandleHead *head = reinterpret_cast<const TabqHandleHead *>(q);
  if (head->tq.table != out->table || head->tq.n_states != out->n_states || n_actions != SGK_ACTIONS)
    return fail(SGK_ERR_INTERNAL, "%s: the tabular-Q handle is not laid out as this file reads it", who);
  if (head->tq.hash_cap)
    return fail(SGK_ERR_INVALID, "%s: this level's tables are hash tables (TomatoWatering): an agent's slots are its own, so the agents' "
                                 "rows do not line up by state", who);
  if (int rc = sgk_handle_launch_site(head->env, &out->sh, &out->stream)) return rc;
  if (out->n_states < 1 || out->sh->n < 1 || sgk::vote_grid(out->sh->n, out->n_states).blocks > INT32_MAX)
    return fail(SGK_ERR_INVALID, "%s: %lld states x %lld agents is more than one launch covers", who, (long long)out->n_states,
                (long long)out->sh->n);
  return SGK_OK;
}

}  // namespace

extern "C" {

int sgk_tabq_consensus(sgk_tabq *q, const uint8_t *voters_mask_dev, int64_t *votes_out_dev, int64_t *voters_out_dev) try {
  if (!q) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus: handle is NULL");
  if (!votes_out_dev) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus: votes_out_dev is NULL");
  if (((uintptr_t)votes_out_dev | (uintptr_t)voters_out_dev) & 7u)
    return fail(SGK_ERR_INVALID, "sgk_tabq_consensus: votes_out_dev and voters_out_dev must be 8-byte aligned");
  TabqSite site;
  if (int rc = site_of(q, "sgk_tabq_consensus", &site)) return rc;
  SGK_HIP(sgk::launch_tabq_consensus(site.table, site.sh->n, site.n_states, voters_mask_dev, votes_out_dev, voters_out_dev, site.stream));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_tabq_load_shared(sgk_tabq *q, const double *table_dev) try {
  if (!q) return fail(SGK_ERR_INVALID, "sgk_tabq_load_shared: handle is NULL");
  if (!table_dev) return fail(SGK_ERR_INVALID, "sgk_tabq_load_shared: table_dev is NULL");
  if ((uintptr_t)table_dev & 7u) return fail(SGK_ERR_INVALID, "sgk_tabq_load_shared: table_dev must be 8-byte aligned");
  TabqSite site;
  if (int rc = site_of(q, "sgk_tabq_load_shared", &site)) return rc;
  SGK_HIP(sgk::launch_tabq_load_shared(site.table, site.sh->n, site.n_states, table_dev, site.stream));
  return sgk_tabq_invalidate_rows(q);  // the per-step kernels' kept rows mirror a table that is gone
} SGK_CATCH_STATUS

int sgk_tabq_consensus_host(const double *table_host, int64_t n_agents, int64_t n_states, const uint8_t *voters_mask_host,
                            int64_t *votes_out_host, int64_t *voters_out_host) try {
  if (!votes_out_host) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus_host: votes_out_host is NULL");
  if (!table_host) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus_host: table_host is NULL");
  if (n_agents < 0) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus_host: n_agents < 0");
  if (n_states < 0) return fail(SGK_ERR_INVALID, "sgk_tabq_consensus_host: n_states < 0");
  for (int64_t s = 0; s < n_states; ++s) {
    int64_t count[4] = {0, 0, 0, 0};
    for (int64_t e = 0; e < n_agents; ++e) {
      if (voters_mask_host && !voters_mask_host[e]) continue;
      const double *row = table_host + (e * n_states + s) * 4;
      const int v = sgk::vote_of_row(row[0], row[1], row[2], row[3]);
      if (v >= 0) count[v] += 1;
    }
    for (int a = 0; a < 4; ++a) votes_out_host[s * 4 + a] = count[a];
    if (voters_out_host) voters_out_host[s] = count[0] + count[1] + count[2] + count[3];
  }
  return SGK_OK;
} SGK_CATCH_STATUS

}  // extern "C"
