// sgk_tabq_hash_consensus.hip -- the consensus of N private tabular-Q agents on the HASHED levels (tomato watering), voted by board
// key (include/sgk.h: sgk_tabq_hash_consensus, sgk_tabq_hash_load_shared and their host restatements). An agent's slots are its own,
// so the agents' rows do not line up by slot; they do line up by KEY: a slot's key names its board, and every key is below 2^22
// (sgk_tabq_vote.h). A presence bitmap of 2^22 bits and its prefix popcount give every voted key a rank in ascending key order.
// Keys are agent-major, keys[n][cap]; rows are slot-major, table[cap][n][4] -- one lane = one agent, so for one slot a wave's rows
// are 2 KB contiguous and each lane walks its own key row, 16 bytes per load. The vote (memsets, then three launches):
//   tabq_hash_mark_kernel   a wave = 64 agents x 16 slots. Per claimed slot of an agent that may vote: the row (read ONCE), its vote
//                           code (0..3, 0xff = none) stored as one byte per (slot, agent) in the workspace, and the key's bit set
//                           in the bitmap -- an atomic OR only where a plain read does not already show the bit
//   tabq_hash_scan_kernel   ONE workgroup: popcount of the 65 536 words, exclusive prefix, *count, keys[rank] for every set bit
//   tabq_hash_count_kernel  the same tiling over the key rows and the code bytes. Equal keys sit at equal slots in most agents (same
//                           home slot), so the lanes that hold the first pending lane's key are combined before the atomics --
//                           balloted per action, one lane adds up to four 64-bit counts (and the voters) --, twice; the lanes
//                           still pending then add their own vote each (count_one)
// The counts are integers: the result depends neither on the grid nor on the order of the atomics.
// The load, the mirror (two launches behind the template):
//   tabq_hash_template_kernel  ONE workgroup builds ONE table by sequential insertion through hash_slot -- the key row (in LDS where it
//                              fits) and, per slot, the index of the row it takes -- so the serial chain is paid once, not per agent
//   tabq_hash_put_keys_kernel  every selected agent's key row := the template's, 16 bytes per lane; its tag := "nothing pending"
//   tabq_hash_put_rows_kernel  every slot's plane := its source row (or zeros) as contiguous 16-byte halves, masked agents skipped
// Every grid honours the shard's max_grid (grid_for): the kernels are grid-stride over their tiles.
#include <hip/hip_runtime.h>

#include <vector>

#include "sgk_device.h"
#include "sgk_host_core.h"
#include "sgk_kernels.h"
#include "sgk_tabq_hash.h"
#include "sgk_tabq_vote.h"

using sgk::host::fail;

static_assert(SGK_TABQ_HASH_KEY_BITS == sgk::TABQ_VOTE_KEY_BITS, "include/sgk.h and sgk_tabq_vote.h disagree on the key width");

namespace sgk {

namespace {

constexpr int HC_WG = 256;          // four waves, each on a tile of its own: no barrier in the vote's kernels
constexpr int HC_WAVES = HC_WG / 64;
constexpr int HC_SLOTS = 16;        // slots per tile (a capacity is a power of two >= 64): four key loads of 16 bytes per lane
constexpr int COMBINE_ROUNDS = 2;   // key groups of a slot index that the count kernel combines before the lanes vote one by one
constexpr int SCAN_WG = 1024;
constexpr int SCAN_PER = TABQ_VOTE_WORDS / (SCAN_WG / 64);  // 4 096 consecutive words per wave
constexpr int TMPL_WG = 256;
constexpr int TMPL_STAGE = 1024;    // keys staged in LDS per round of the template's insertion
constexpr int TMPL_LDS_MAX_CAP = 32768;  // 4 * cap + the stage = 132 KB of the CU's 160 KB
constexpr int64_t PUT_PER = 1024;   // agents per unit of the row broadcast: 2 048 halves, eight full passes of the workgroup

// the workspace: bitmap | prefix | template keys [cap] | template sources [cap] | vote codes [cap][n], every part 16-byte aligned
struct Workspace {
  uint64_t *bitmap;
  uint32_t *prefix;
  uint32_t *tmpl_keys;
  int32_t *tmpl_src;
  uint8_t *codes;
};
constexpr int64_t WS_BITMAP_BYTES = (int64_t)TABQ_VOTE_WORDS * 8, WS_PREFIX_BYTES = (int64_t)TABQ_VOTE_WORDS * 4;
int64_t hash_workspace_bytes(int64_t n, int cap) {
  return WS_BITMAP_BYTES + WS_PREFIX_BYTES + 8 * (int64_t)cap + (((int64_t)cap * n + 15) & ~(int64_t)15);
}
Workspace workspace_of(void *base, int cap) {
  char *p = static_cast<char *>(base);
  Workspace w;
  w.bitmap = reinterpret_cast<uint64_t *>(p);
  w.prefix = reinterpret_cast<uint32_t *>(p + WS_BITMAP_BYTES);
  w.tmpl_keys = reinterpret_cast<uint32_t *>(p + WS_BITMAP_BYTES + WS_PREFIX_BYTES);
  w.tmpl_src = reinterpret_cast<int32_t *>(p + WS_BITMAP_BYTES + WS_PREFIX_BYTES + 4 * (int64_t)cap);
  w.codes = reinterpret_cast<uint8_t *>(p + WS_BITMAP_BYTES + WS_PREFIX_BYTES + 8 * (int64_t)cap);
  return w;
}

__device__ __forceinline__ void mark_one(uint32_t key, bool held, const TabqRow &r, uint64_t *__restrict__ bitmap, uint8_t *code_out) {
  uint8_t code = TABQ_VOTE_NONE;
  if (held) {
    const int v = vote_of_row(r.q0, r.q1, r.q2, r.q3);
    if (v >= 0) {
      code = (uint8_t)v;
      unsigned long long *word = reinterpret_cast<unsigned long long *>(bitmap + (key >> 6));
      const unsigned long long bit = 1ull << (key & 63u);
      // (bits are only ever set: a read that already shows the bit saves the atomic; one that does not yet costs nothing but it)
      if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
    }
  }
  *code_out = code;
}

__global__ __launch_bounds__(HC_WG) void tabq_hash_mark_kernel(const uint32_t *__restrict__ keys, const double *__restrict__ table,
                                                               const uint8_t *__restrict__ mask, int64_t n, int cap,
                                                               uint64_t *__restrict__ bitmap, uint8_t *__restrict__ codes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = cap / HC_SLOTS;
  const int64_t tiles = ((n + 63) / 64) * chunks;
  for (int64_t tile = (int64_t)blockIdx.x * HC_WAVES + wave; tile < tiles; tile += (int64_t)gridDim.x * HC_WAVES) {
    const int64_t e = (tile / chunks) * 64 + lane;
    const int s0 = (int)(tile % chunks) * HC_SLOTS;
    if (e >= n) continue;
    const bool may = !mask || mask[e] != 0;
    const uint32_t *kr = keys + e * cap + s0;
    for (int i = 0; i < HC_SLOTS; i += 4) {
      TabqKeys4 k = {TABQ_HASH_EMPTY, TABQ_HASH_EMPTY, TABQ_HASH_EMPTY, TABQ_HASH_EMPTY};
      if (may) k = tabq_load_keys4(kr + i);
      // a key that cannot be (>= 1 << 22 and not the empty marker) is skipped like an empty slot: nothing indexes past the bitmap
      const bool h0 = tabq_key_votable(k.k0), h1 = tabq_key_votable(k.k1), h2 = tabq_key_votable(k.k2), h3 = tabq_key_votable(k.k3);
      const double *src = table + ((int64_t)(s0 + i) * n + e) * 4;
      TabqRow r0 = {0.0, 0.0, 0.0, 0.0}, r1 = r0, r2 = r0, r3 = r0;  // the group's rows requested before the first is used
      if (h0) r0 = tabq_load_row(src);
      if (h1) r1 = tabq_load_row(src + n * 4);
      if (h2) r2 = tabq_load_row(src + 2 * n * 4);
      if (h3) r3 = tabq_load_row(src + 3 * n * 4);
      uint8_t *c = codes + (int64_t)(s0 + i) * n + e;
      mark_one(k.k0, h0, r0, bitmap, c);
      mark_one(k.k1, h1, r1, bitmap, c + n);
      mark_one(k.k2, h2, r2, bitmap, c + 2 * n);
      mark_one(k.k3, h3, r3, bitmap, c + 3 * n);
    }
  }
}

__global__ __launch_bounds__(SCAN_WG) void tabq_hash_scan_kernel(const uint64_t *__restrict__ bitmap, uint32_t *__restrict__ prefix,
                                                                 uint32_t *__restrict__ keys_out, int64_t max_keys,
                                                                 int64_t *__restrict__ count) {
  // A wave owns SCAN_PER consecutive words and walks them 64 at a time, lane = word: every load and every prefix store is one
  // contiguous 512- / 256-byte piece. First the wave's total, the workgroup's exclusive prefix over the 16 totals, then the walk again
  // (the words come from L2) with a wave scan per 64 words.
  __shared__ uint32_t wave_sum[SCAN_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first = wave * SCAN_PER;
  uint32_t sum = 0;
#pragma unroll 8
  for (int r = 0; r < SCAN_PER / 64; ++r) sum += (uint32_t)__popcll(bitmap[first + r * 64 + lane]);
  for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);  // every lane: the wave's total
  if (lane == 0) wave_sum[wave] = sum;
  __syncthreads();
  uint32_t run = 0;  // set bits before the wave's next 64 words (wave-uniform)
  for (int w = 0; w < wave; ++w) run += wave_sum[w];
  if (tid == SCAN_WG - 1) *count = (int64_t)(run + sum);  // the TRUE number of voted keys, whatever max_keys
#pragma unroll 2
  for (int r = 0; r < SCAN_PER / 64; ++r) {
    const int w = first + r * 64 + lane;
    uint64_t word = bitmap[w];
    const uint32_t pop = (uint32_t)__popcll(word);
    uint32_t inc = pop;  // the wave's inclusive prefix over these 64 words
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    uint32_t at = run + inc - pop;
    prefix[w] = at;
    while (word) {
      const int b = __ffsll((unsigned long long)word) - 1;
      if ((int64_t)at < max_keys) keys_out[at] = (uint32_t)w * 64u + (uint32_t)b;
      ++at;
      word &= word - 1;
    }
    run += __shfl(inc, 63);
  }
}

// One slot index of the wave's 64 agents. Every voting lane finds its own key's rank (the lanes' loads run side by side). Then the
// lanes that hold the key of the first pending lane are combined -- balloted per action, that lane adds up to four 64-bit counts and
// the voters --, COMBINE_ROUNDS times: equal keys sit at equal slots in most agents (same home slot), and without this the start
// board is N serial atomics on one address. What is still pending afterwards holds keys few lanes share: each lane adds its own vote.
// (A loop over ALL the groups would be a serial chain of up to 64 rounds per slot where the keys differ -- most slots.)
__device__ __forceinline__ void count_one(uint32_t key, uint8_t code, int lane, const uint64_t *__restrict__ bitmap,
                                          const uint32_t *__restrict__ prefix, int64_t max_keys, unsigned long long *__restrict__ votes,
                                          unsigned long long *__restrict__ voters) {
  bool pending = code != TABQ_VOTE_NONE;
  unsigned long long todo = __ballot(pending);
  if (!todo) return;  // (wave-uniform)
  const int64_t rank = pending ? tabq_key_rank(bitmap, prefix, key) : max_keys;
  if (rank >= max_keys) pending = false;  // (behind max_keys the key is counted in *count only)
  todo = __ballot(pending);
  for (int round = 0; round < COMBINE_ROUNDS && todo; ++round) {  // (the condition is a ballot: every lane reaches every ballot)
    const int leader = __ffsll(todo) - 1;
    const uint32_t k = (uint32_t)__shfl((int)key, leader);
    const bool same = pending && key == k;
    const unsigned long long c0 = (unsigned)__popcll(__ballot(same && code == 0)), c1 = (unsigned)__popcll(__ballot(same && code == 1)),
                             c2 = (unsigned)__popcll(__ballot(same && code == 2)), c3 = (unsigned)__popcll(__ballot(same && code == 3));
    if (lane == leader && pending) {
      if (c0) atomicAdd(&votes[rank * 4], c0);
      if (c1) atomicAdd(&votes[rank * 4 + 1], c1);
      if (c2) atomicAdd(&votes[rank * 4 + 2], c2);
      if (c3) atomicAdd(&votes[rank * 4 + 3], c3);
      if (voters) atomicAdd(&voters[rank], c0 + c1 + c2 + c3);
    }
    pending = pending && !same;
    todo = __ballot(pending);
  }
  if (pending) {
    atomicAdd(&votes[rank * 4 + code], 1ull);
    if (voters) atomicAdd(&voters[rank], 1ull);
  }
}

__global__ __launch_bounds__(HC_WG) void tabq_hash_count_kernel(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ codes,
                                                                int64_t n, int cap, const uint64_t *__restrict__ bitmap,
                                                                const uint32_t *__restrict__ prefix, int64_t max_keys,
                                                                unsigned long long *__restrict__ votes,
                                                                unsigned long long *__restrict__ voters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = cap / HC_SLOTS;
  const int64_t tiles = ((n + 63) / 64) * chunks;
  for (int64_t tile = (int64_t)blockIdx.x * HC_WAVES + wave; tile < tiles; tile += (int64_t)gridDim.x * HC_WAVES) {  // (wave-uniform)
    const int64_t e = (tile / chunks) * 64 + lane;
    const int s0 = (int)(tile % chunks) * HC_SLOTS;
    const bool in = e < n;
    const uint32_t *kr = keys + (in ? e : 0) * cap + s0;
    for (int i = 0; i < HC_SLOTS; i += 4) {
      const uint8_t *c = codes + (int64_t)(s0 + i) * n + e;
      uint8_t c0 = TABQ_VOTE_NONE, c1 = TABQ_VOTE_NONE, c2 = TABQ_VOTE_NONE, c3 = TABQ_VOTE_NONE;
      TabqKeys4 k = {TABQ_HASH_EMPTY, TABQ_HASH_EMPTY, TABQ_HASH_EMPTY, TABQ_HASH_EMPTY};
      if (in) {
        c0 = c[0]; c1 = c[n]; c2 = c[2 * n]; c3 = c[3 * n];
        if ((c0 & c1 & c2 & c3) != TABQ_VOTE_NONE) k = tabq_load_keys4(kr + i);  // (keys are needed only where somebody votes)
      }
      count_one(k.k0, c0, lane, bitmap, prefix, max_keys, votes, voters);
      count_one(k.k1, c1, lane, bitmap, prefix, max_keys, votes, voters);
      count_one(k.k2, c2, lane, bitmap, prefix, max_keys, votes, voters);
      count_one(k.k3, c3, lane, bitmap, prefix, max_keys, votes, voters);
    }
  }
}

// ONE table built by sequential insertion of keys_in[0 .. min(*count, max_keys)) through hash_slot: tmpl_keys[cap] the key row,
// tmpl_src[cap] the index of the row each slot takes (-1: an empty slot, a zero row; a later duplicate overwrites the earlier index).
// Lane 0 inserts; the workgroup stages the keys in LDS, TMPL_STAGE at a time, so the chain does not wait on HBM per key. LDS_KEYS:
// the key row under construction lives in LDS too and is written out at the end.
template <bool LDS_KEYS>
__global__ __launch_bounds__(TMPL_WG) void tabq_hash_template_kernel(const uint32_t *__restrict__ keys_in, const int64_t *__restrict__ count_dev,
                                                                     int64_t max_keys, int cap, uint32_t *__restrict__ tmpl_keys,
                                                                     int32_t *__restrict__ tmpl_src, int32_t *__restrict__ overflow) {
  extern __shared__ uint32_t lds[];  // [TMPL_STAGE] the staged keys, then [cap] the key row (LDS_KEYS)
  uint32_t *stage = lds, *kt = LDS_KEYS ? lds + TMPL_STAGE : tmpl_keys;
  const int tid = threadIdx.x;
  for (int i = tid; i < cap; i += TMPL_WG) {
    kt[i] = TABQ_HASH_EMPTY;
    tmpl_src[i] = -1;
  }
  int64_t count = *count_dev;
  if (count > max_keys) count = max_keys;
  __syncthreads();
  for (int64_t base = 0; base < count; base += TMPL_STAGE) {  // (workgroup-uniform trip count)
    const int m = (int)(count - base < TMPL_STAGE ? count - base : TMPL_STAGE);
    for (int i = tid; i < m; i += TMPL_WG) stage[i] = keys_in[base + i];
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < m; ++i) {
        const uint32_t key = stage[i];
        if (key == TABQ_HASH_EMPTY) continue;  // the empty marker names no board
        const int j = hash_slot(kt, cap, key, overflow);  // (a full table: the sticky flag is raised and the key dropped)
        if (j >= 0) tmpl_src[j] = (int32_t)(base + i);
      }
    }
    __syncthreads();
  }
  if (LDS_KEYS)
    for (int i = tid; i < cap; i += TMPL_WG) tmpl_keys[i] = kt[i];
}

__global__ __launch_bounds__(HC_WG) void tabq_hash_put_keys_kernel(uint32_t *__restrict__ keys, uint64_t *__restrict__ tags,
                                                                   const uint8_t *__restrict__ mask, int64_t n, int cap,
                                                                   const uint32_t *__restrict__ tmpl_keys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(tmpl_keys);
  for (int64_t e = (int64_t)blockIdx.x * HC_WAVES + wave; e < n; e += (int64_t)gridDim.x * HC_WAVES) {
    if (mask && !mask[e]) continue;
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(keys + e * cap);  // a whole key row: the wave's store is 1 KB contiguous
    for (int i = lane; i < cap / 4; i += 64) dst[i] = src[i];
    if (lane == 0) tags[e] = ~0ull;  // no pending act(), no kept row
  }
}

__global__ __launch_bounds__(HC_WG) void tabq_hash_put_rows_kernel(double *__restrict__ table, const uint8_t *__restrict__ mask, int64_t n,
                                                                   int cap, int chunks, const int32_t *__restrict__ tmpl_src,
                                                                   const double *__restrict__ rows) {
  const int64_t units = (int64_t)cap * chunks;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t s = u / chunks, begin = (u % chunks) * PUT_PER, end = begin + PUT_PER < n ? begin + PUT_PER : n;
    const int32_t from = tmpl_src[s];
    double2 r01 = make_double2(0.0, 0.0), r23 = r01;
    if (from >= 0) {  // (read as four doubles: the caller's rows need only be 8-byte aligned)
      const double *r = rows + (int64_t)from * 4;
      r01 = make_double2(r[0], r[1]);
      r23 = make_double2(r[2], r[3]);
    }
    double2 *__restrict__ plane = reinterpret_cast<double2 *>(table + s * n * 4);
    // the run as 16-byte halves of rows, as tabq_load_kernel stores them: a lane always holds the same half of a row
    const double2 mine = (threadIdx.x & 1) ? r23 : r01;
    for (int64_t i = 2 * begin + threadIdx.x; i < 2 * end; i += HC_WG)
      if (!mask || mask[i >> 1]) plane[i] = mine;
  }
}

}  // namespace

hipError_t launch_tabq_hash_consensus(const Shard &sh, const TabqShard &tq, const uint8_t *mask, const sgk_tabq_hash_votes &out, hipStream_t st) {
  const Workspace w = workspace_of(out.workspace, tq.hash_cap);
  const int64_t tiles = ((sh.n + 63) / 64) * (tq.hash_cap / HC_SLOTS);
  const int grid = grid_for((tiles + HC_WAVES - 1) / HC_WAVES, sh.max_grid);
  hipError_t e = hipMemsetAsync(w.bitmap, 0, (size_t)WS_BITMAP_BYTES, st);
  if (e == hipSuccess) e = hipMemsetAsync(out.keys, 0xff, sizeof(uint32_t) * (size_t)out.max_keys, st);
  if (e == hipSuccess) e = hipMemsetAsync(out.votes, 0, sizeof(int64_t) * 4 * (size_t)out.max_keys, st);
  if (e == hipSuccess && out.voters) e = hipMemsetAsync(out.voters, 0, sizeof(int64_t) * (size_t)out.max_keys, st);
  if (e != hipSuccess) return e;
  (void)hipGetLastError();
  tabq_hash_mark_kernel<<<dim3(grid), dim3(HC_WG), 0, st>>>(tq.keys, tq.table, mask, sh.n, tq.hash_cap, w.bitmap, w.codes);
  tabq_hash_scan_kernel<<<dim3(1), dim3(SCAN_WG), 0, st>>>(w.bitmap, w.prefix, out.keys, out.max_keys, out.count);
  tabq_hash_count_kernel<<<dim3(grid), dim3(HC_WG), 0, st>>>(tq.keys, w.codes, sh.n, tq.hash_cap, w.bitmap, w.prefix, out.max_keys,
                                                            reinterpret_cast<unsigned long long *>(out.votes),
                                                            reinterpret_cast<unsigned long long *>(out.voters));
  return hipGetLastError();
}

hipError_t launch_tabq_hash_load_shared(const Shard &sh, const TabqShard &tq, const uint8_t *mask, const uint32_t *keys_in, const double *rows,
                       const int64_t *count_dev, int64_t max_keys, void *workspace, hipStream_t st) {
  const Workspace w = workspace_of(workspace, tq.hash_cap);
  const int cap = tq.hash_cap;
  (void)hipGetLastError();
  bool lds_keys = cap <= TMPL_LDS_MAX_CAP;
  const size_t lds_bytes = sizeof(uint32_t) * ((size_t)TMPL_STAGE + (size_t)cap);
  if (lds_keys && lds_bytes > 64 * 1024) {  // above the default limit the kernel is told how much it may ask for
    const hipError_t allowed = hipFuncSetAttribute(reinterpret_cast<const void *>(&tabq_hash_template_kernel<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (TMPL_STAGE + TMPL_LDS_MAX_CAP));
    if (allowed != hipSuccess) {
      (void)hipGetLastError();
      lds_keys = false;  // the key row is then built in the workspace: the same insertion, slower
    }
  }
  if (lds_keys)
    tabq_hash_template_kernel<true><<<dim3(1), dim3(TMPL_WG), lds_bytes, st>>>(keys_in, count_dev, max_keys, cap, w.tmpl_keys, w.tmpl_src,
                                                                             tq.hash_overflow);
  else
    tabq_hash_template_kernel<false><<<dim3(1), dim3(TMPL_WG), sizeof(uint32_t) * TMPL_STAGE, st>>>(keys_in, count_dev, max_keys, cap,
                                                                                                    w.tmpl_keys, w.tmpl_src, tq.hash_overflow);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  tabq_hash_put_keys_kernel<<<dim3(grid_for((sh.n + HC_WAVES - 1) / HC_WAVES, sh.max_grid)), dim3(HC_WG), 0, st>>>(tq.keys, tq.tags, mask, sh.n,
                                                                                                                 cap, w.tmpl_keys);
  const int chunks = (int)((sh.n + PUT_PER - 1) / PUT_PER);
  tabq_hash_put_rows_kernel<<<dim3(grid_for((int64_t)cap * chunks, sh.max_grid)), dim3(HC_WG), 0, st>>>(tq.table, mask, sh.n, cap, chunks,
                                                                                                      w.tmpl_src, rows);
  return hipGetLastError();
}

}  // namespace sgk

extern "C" int sgk_tabq_launch_site(sgk_tabq *q, const sgk::Shard **sh_out, const sgk::TabqShard **tq_out, hipStream_t *stream_out);  // sgk_api.hip

namespace {

struct HashSite {
  const sgk::Shard *sh = nullptr;
  const sgk::TabqShard *tq = nullptr;
  hipStream_t stream = nullptr;
};

int site_of(sgk_tabq *q, const char *who, HashSite *out) {
  if (!q) return fail(SGK_ERR_INVALID, "%s: handle is NULL", who);
  if (int rc = sgk_tabq_launch_site(q, &out->sh, &out->tq, &out->stream)) return rc;
  if (!out->tq->hash_cap)
    return fail(SGK_ERR_INVALID, "%s: this level's tables are indexed by a perfect hash: there are no board keys to vote by "
                                 "(sgk_tabq_consensus and sgk_tabq_load_shared are the calls for it)", who);
  if (out->sh->n < 1 || out->tq->hash_cap % sgk::HC_SLOTS)
    return fail(SGK_ERR_INVALID, "%s: %lld agents x %d slots is nothing this call covers", who, (long long)out->sh->n, (int)out->tq->hash_cap);
  return SGK_OK;
}

// the part of the workspace's check that needs no handle, and the part that does (every check a NULL handle allows comes before it)
int check_workspace_pointer(const char *who, const sgk_tabq_hash_votes *d, const char *name) {
  if (!d->workspace) return fail(SGK_ERR_INVALID, "%s: %s->workspace is NULL", who, name);
  if ((uintptr_t)d->workspace & 15u) return fail(SGK_ERR_INVALID, "%s: %s->workspace must be 16-byte aligned", who, name);
  return SGK_OK;
}
int check_workspace_size(const char *who, const sgk_tabq_hash_votes *d, const char *name, int64_t need) {
  if (d->workspace_bytes < need)
    return fail(SGK_ERR_INVALID, "%s: %s->workspace_bytes is %lld, below the %lld sgk_tabq_hash_consensus_workspace_bytes asks for", who, name,
                (long long)d->workspace_bytes, (long long)need);
  return SGK_OK;
}

// what both forms of the vote ask of the output descriptor (the workspace is the device call's alone)
int check_votes(const char *who, const sgk_tabq_hash_votes *out) {
  if (!out) return fail(SGK_ERR_INVALID, "%s: out is NULL", who);
  if (!out->keys) return fail(SGK_ERR_INVALID, "%s: out->keys is NULL", who);
  if (!out->votes) return fail(SGK_ERR_INVALID, "%s: out->votes is NULL", who);
  if (!out->count) return fail(SGK_ERR_INVALID, "%s: out->count is NULL", who);
  if (out->max_keys < 1) return fail(SGK_ERR_INVALID, "%s: out->max_keys < 1", who);
  if ((uintptr_t)out->keys & 3u) return fail(SGK_ERR_INVALID, "%s: out->keys must be 4-byte aligned", who);
  if (((uintptr_t)out->votes | (uintptr_t)out->voters | (uintptr_t)out->count) & 7u)
    return fail(SGK_ERR_INVALID, "%s: out->votes, out->voters and out->count must be 8-byte aligned", who);
  return SGK_OK;
}

bool power_of_two_capacity(int32_t capacity) { return capacity >= 64 && capacity <= (1 << 24) && !(capacity & (capacity - 1)); }

}  // namespace

extern "C" {

int64_t sgk_tabq_hash_consensus_workspace_bytes(sgk_tabq *q) try {
  HashSite site;
  if (int rc = site_of(q, "sgk_tabq_hash_consensus_workspace_bytes", &site)) return rc;
  return sgk::hash_workspace_bytes(site.sh->n, site.tq->hash_cap);
} SGK_CATCH_STATUS

int sgk_tabq_hash_consensus(sgk_tabq *q, const uint8_t *voters_mask_dev, const sgk_tabq_hash_votes *out) try {
  const char *who = "sgk_tabq_hash_consensus";
  if (int rc = check_votes(who, out)) return rc;
  if (int rc = check_workspace_pointer(who, out, "out")) return rc;
  HashSite site;
  if (int rc = site_of(q, who, &site)) return rc;
  if (int rc = check_workspace_size(who, out, "out", sgk::hash_workspace_bytes(site.sh->n, site.tq->hash_cap))) return rc;
  SGK_HIP(sgk::launch_tabq_hash_consensus(*site.sh, *site.tq, voters_mask_dev, *out, site.stream));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_tabq_hash_load_shared(sgk_tabq *q, const uint8_t *agents_mask_dev, const uint32_t *keys_dev, const double *rows_dev,
                              const int64_t *count_dev, int64_t max_keys, const sgk_tabq_hash_votes *scratch) try {
  const char *who = "sgk_tabq_hash_load_shared";
  if (!keys_dev) return fail(SGK_ERR_INVALID, "%s: keys_dev is NULL", who);
  if (!rows_dev) return fail(SGK_ERR_INVALID, "%s: rows_dev is NULL", who);
  if (!count_dev) return fail(SGK_ERR_INVALID, "%s: count_dev is NULL", who);
  if (max_keys < 1 || max_keys > INT32_MAX) return fail(SGK_ERR_INVALID, "%s: max_keys must be in 1 .. 2^31 - 1", who);
  if (!scratch) return fail(SGK_ERR_INVALID, "%s: scratch is NULL", who);
  if ((uintptr_t)keys_dev & 3u) return fail(SGK_ERR_INVALID, "%s: keys_dev must be 4-byte aligned", who);
  if (((uintptr_t)rows_dev | (uintptr_t)count_dev) & 7u) return fail(SGK_ERR_INVALID, "%s: rows_dev and count_dev must be 8-byte aligned", who);
  if (int rc = check_workspace_pointer(who, scratch, "scratch")) return rc;
  HashSite site;
  if (int rc = site_of(q, who, &site)) return rc;
  if (int rc = check_workspace_size(who, scratch, "scratch", sgk::hash_workspace_bytes(site.sh->n, site.tq->hash_cap))) return rc;
  SGK_HIP(sgk::launch_tabq_hash_load_shared(*site.sh, *site.tq, agents_mask_dev, keys_dev, rows_dev, count_dev, max_keys, scratch->workspace, site.stream));
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_tabq_hash_consensus_host(const uint32_t *keys_host, const double *rows_host, int64_t n_agents, int32_t capacity,
                                 const uint8_t *voters_mask_host, const sgk_tabq_hash_votes *out) try {
  const char *who = "sgk_tabq_hash_consensus_host";
  if (int rc = check_votes(who, out)) return rc;
  if (!keys_host) return fail(SGK_ERR_INVALID, "%s: keys_host is NULL", who);
  if (!rows_host) return fail(SGK_ERR_INVALID, "%s: rows_host is NULL", who);
  if (n_agents < 0) return fail(SGK_ERR_INVALID, "%s: n_agents < 0", who);
  if (capacity < 1) return fail(SGK_ERR_INVALID, "%s: capacity < 1", who);
  // the device's three steps on [agent][slot] arrays: mark, scan, count
  std::vector<uint64_t> bitmap(sgk::TABQ_VOTE_WORDS, 0);
  std::vector<uint32_t> prefix(sgk::TABQ_VOTE_WORDS, 0);
  std::vector<uint8_t> codes((size_t)n_agents * (size_t)capacity, sgk::TABQ_VOTE_NONE);
  for (int64_t e = 0; e < n_agents; ++e) {
    if (voters_mask_host && !voters_mask_host[e]) continue;
    for (int32_t s = 0; s < capacity; ++s) {
      const uint32_t key = keys_host[e * capacity + s];
      if (!sgk::tabq_key_votable(key)) continue;
      const double *row = rows_host + (e * capacity + s) * 4;
      const int v = sgk::vote_of_row(row[0], row[1], row[2], row[3]);
      if (v < 0) continue;
      codes[(size_t)(e * capacity + s)] = (uint8_t)v;
      bitmap[key >> 6] |= 1ull << (key & 63u);
    }
  }
  for (int64_t j = 0; j < out->max_keys; ++j) {
    out->keys[j] = sgk::TABQ_HASH_EMPTY;
    for (int a = 0; a < 4; ++a) out->votes[j * 4 + a] = 0;
    if (out->voters) out->voters[j] = 0;
  }
  int64_t run = 0;
  for (int w = 0; w < sgk::TABQ_VOTE_WORDS; ++w) {
    prefix[w] = (uint32_t)run;
    for (uint64_t word = bitmap[w]; word; word &= word - 1) {
      if (run < out->max_keys) out->keys[run] = (uint32_t)w * 64u + (uint32_t)__builtin_ctzll(word);
      ++run;
    }
  }
  *out->count = run;
  for (size_t i = 0; i < codes.size(); ++i) {
    if (codes[i] == sgk::TABQ_VOTE_NONE) continue;
    const int64_t rank = sgk::tabq_key_rank(bitmap.data(), prefix.data(), keys_host[i]);
    if (rank >= out->max_keys) continue;
    out->votes[rank * 4 + codes[i]] += 1;
    if (out->voters) out->voters[rank] += 1;
  }
  return SGK_OK;
} SGK_CATCH_STATUS

int sgk_tabq_hash_load_shared_host(const uint32_t *keys_in, const double *rows_in, int64_t count, int32_t capacity,
                                   const sgk_tabq_hash_table *out) try {
  const char *who = "sgk_tabq_hash_load_shared_host";
  if (!out) return fail(SGK_ERR_INVALID, "%s: out is NULL", who);
  if (!out->keys) return fail(SGK_ERR_INVALID, "%s: out->keys is NULL", who);
  if (!out->rows) return fail(SGK_ERR_INVALID, "%s: out->rows is NULL", who);
  if (count < 0) return fail(SGK_ERR_INVALID, "%s: count < 0", who);
  if (count && !keys_in) return fail(SGK_ERR_INVALID, "%s: keys_in is NULL", who);
  if (count && !rows_in) return fail(SGK_ERR_INVALID, "%s: rows_in is NULL", who);
  if (!power_of_two_capacity(capacity)) return fail(SGK_ERR_INVALID, "%s: capacity must be a power of two in 64 .. 2^24", who);
  int32_t overflow = 0;
  for (int32_t s = 0; s < capacity; ++s) {
    out->keys[s] = sgk::TABQ_HASH_EMPTY;
    for (int a = 0; a < 4; ++a) out->rows[s * 4 + a] = 0.0;
  }
  for (int64_t j = 0; j < count; ++j) {
    if (keys_in[j] == sgk::TABQ_HASH_EMPTY) continue;
    const int s = sgk::hash_slot(out->keys, capacity, keys_in[j], &overflow);
    if (s >= 0) memcpy(out->rows + (int64_t)s * 4, rows_in + j * 4, 4 * sizeof(double));
  }
  if (out->overflowed) *out->overflowed = overflow;
  return SGK_OK;
} SGK_CATCH_STATUS

}  // extern "C"
