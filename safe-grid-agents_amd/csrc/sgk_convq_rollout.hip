// sgk_convq_rollout.hip -- n_steps of {conv body forward, action draw, env.step} in ONE launch (sgk_convq_rollout): the inner loop of
// PPOBaseAgent.gather_rollout (reference policy_base.py:142-163: old_policy.act_explore -> env.step -> store state / action / reward)
// for a PPOCNNAgent (policy_cnn.py:17-81), or acting with a frozen conv Q-network (the batched DeepQ agent's non-parity option). What
// sgk_policy_rollout (sgk_policy.hip) is for the MLP bodies, on the kernel pieces of sgk_convq.h.
//
// A workgroup owns the ENVS envs of a pass for ALL n_steps: their state words live in the registers of ENVS lanes of wave 0, their
// boards as int8 rows in LDS. Per step: all lanes turn the rows into plane 0 (and store them as the trajectory's `states`), the three
// convolutions run as in sgk_convq_act (four waves, three barriers), wave 0 sums the outputs and draws, and its owner lanes step their
// envs (the kernels' one step_one), store action and record, and re-draw their rows. No board, action or record crosses HBM between
// steps except as trajectory output: per lockstep step the caller's four launches (forward + draw, board copy, sgk_step, record copy)
// become one pass of this loop. sgk_convq_rollout_members runs the same loop for n_members independent bodies (ConvRolloutMemberArgs),
// sgk_convq_rollout_trans on the observation [previous board, board] (ConvRolloutTransArgs): ONE kernel template,
// convq_rollout_kernel<ENV, C, MEMBERS, CI>, and one launch sequence, convq_rollout_launch, for all three.
#include "sgk_convq.h"

namespace sgk {

struct ConvRolloutArgs {
  StepArgs env;          // state / rec / episode arrays / metrics / rules / n / seed / env_base / flags
  double eps;            // mode 0
  uint64_t draw0;        // draw index of the first step; step k uses draw0 + k
  int32_t n_steps, mode; // mode 0: epsilon-greedy (Philox stream 2), 1: Categorical sample (stream 3)
  int8_t *states_out;    // [n_steps][n][NC] boards the policy acted on, or null
  uint8_t *actions_out;  // [n_steps][n] or null
  uint32_t *recs_out;    // [n_steps][n] step records or null
};

// sgk_convq_rollout_members: n_members independent conv bodies in one launch. Member m owns the envs m * member_envs .. (m + 1) *
// member_envs - 1 and the m-th slice of each of the ten stacked weight tensors. A workgroup belongs to ONE member for the whole launch
// (member_wgs consecutive workgroups each: the grid is n_members * member_wgs, and the hardware queues what is not resident), reads
// that member's weights and walks that member's ceil(member_envs / ENVS) passes only, so a pass never straddles two members. Env
// indices -- RNG keys, trajectory columns, episode arrays -- stay the shard's own.
struct ConvRolloutMemberArgs : ConvRolloutArgs {
  int64_t member_envs;        // envs per member
  int32_t member_wgs;         // workgroups per member
  long long *member_metrics;  // [n_members][SGK_METRICS_LEN]: each member's own episode sums / counts / maxima, or null
};

// sgk_convq_rollout_trans: the same loop on the observation of a transition env, [previous board, board] (ConvQGeom's CI = 2: w1
// [C][2][3][3], wb [C][2][1][1]); no member form
struct ConvRolloutTransArgs : ConvRolloutArgs {
  int8_t *prev_boards;      // [n][NC]: read at entry unless `fresh`, written at exit (the previous-board channel the NEXT action would see)
  int8_t *prev_states_out;  // [n_steps][n][NC]: channel 0 beside states_out's channel 1, or null
  int32_t fresh;            // != 0: no env has stepped since its reset: previous := current at entry
};

template <bool MEMBERS, int CI>
using ConvRolloutArgsFor =
    typename std::conditional<CI == 2, ConvRolloutTransArgs, typename std::conditional<MEMBERS, ConvRolloutMemberArgs, ConvRolloutArgs>::type>::type;

// (CI = 1: no previous rows and two arrays of flags -- the offsets from before the two-board observation)
template <int ENV, int C, int CI = 1>
struct ConvRolloutLds {
  typedef ConvQGeom<Geom<ENV>::H, Geom<ENV>::W, C, CI> G;
  static constexpr size_t tile_bytes = (size_t)G::ENVS * G::NC;
  static constexpr size_t o_tile = (G::lds_bytes + 15) & ~(size_t)15;                      // int8 [ENVS][NC]: the current rows
  static constexpr size_t o_prev = (o_tile + tile_bytes + 15) & ~(size_t)15;               // CI = 2: int8 [ENVS][NC], the previous rows
  static constexpr size_t o_flags = (o_prev + (CI - 1) * tile_bytes + 15) & ~(size_t)15;   // int32 action[ENVS], over[ENVS](, CI = 2: fresh[ENVS])
  static constexpr size_t o_rules = (o_flags + (CI + 1) * sizeof(int) * G::ENVS + 15) & ~(size_t)15;
  static constexpr size_t bytes = o_rules + sizeof(SgkRules) + 16;
};

// The register budget of sgk_convq_act, although the env state, the episode accumulators and the step's temporaries then spill 16-256
// bytes per lane to scratch (outside the convolutions): one wave per SIMD fewer has no spills and is SLOWER -- 28.3 against 23.7 us per
// lockstep step at 32 768 Sokoban envs and five channels, 55 against 45 on DistributionalShift (tools/gpu_convq_ab.sh).
#ifndef CQ_ROLLOUT_WAVES_FOR
#define CQ_ROLLOUT_WAVES_FOR(C) CQ_WAVES_FOR(C)
#endif
// the distance between two passes of a workgroup: the grid, or its member's workgroups
template <bool MEMBERS, class Args>
__device__ __forceinline__ int64_t cr_pass_step(const Args &a) {
  if constexpr (MEMBERS) return a.member_wgs;
  else return gridDim.x;
}

// MEMBERS = false is sgk_convq_rollout's kernel, as it was before the member axis; MEMBERS = true (sgk_convq_rollout_members, with one
// member too) adds the member's offsets to the weight pointers and bounds the passes by the member's envs.
//
// CI = 2 (sgk_convq_rollout_trans) keeps a second tile, the previous rows, and a fresh flag per env. At the top of a step every lane
// turns ITS bytes of both tiles into planes 0 (previous) and 1 (current), stores them to the two trajectory outputs and then copies
// current -> previous. That order is race-free: a lane reads and writes only its own elements of the previous tile; the current rows and
// the per-env fresh flags are changed by the owner lanes alone and only behind the network's barriers, while every lane's reads of them
// lie between the barrier at the top of the step and the one in front of the network. An env that step_one reset (SGK_F_AUTO_RESET)
// acts next on [board, board]: its owner raises the env's fresh flag (next to over_sh), and the conversion then takes the current byte
// for plane 0 too. The one-board kernels are the instruction streams they were before CI (profiles/convq_one_kernel/resource_usage.log).
template <int ENV, int C, bool MEMBERS, int CI = 1>
__global__ __launch_bounds__(CQ_WG, CQ_ROLLOUT_WAVES_FOR(C)) void convq_rollout_kernel(
    ConvRolloutArgsFor<MEMBERS, CI> a, const float *__restrict__ w1r, const float *__restrict__ b1r, const float *__restrict__ w2r,
    const float *__restrict__ b2r, const float *__restrict__ wbr, const float *__restrict__ bbr, const float *__restrict__ whr,
    const float *__restrict__ bhr, const float *__restrict__ wlr, const float *__restrict__ blr) {
  static_assert(!(MEMBERS && CI == 2), "the two-board kernel has no member form");
  constexpr int WW = Geom<ENV>::W;
  typedef ConvRolloutLds<ENV, C, CI> LD;
  typedef typename LD::G G;
  static_assert(G::NC == Geom<ENV>::NC, "level geometry");
  extern __shared__ __attribute__((aligned(16))) unsigned char convq_smem[];
  float *Lf = reinterpret_cast<float *>(convq_smem);
  float *WL = Lf + G::O_WL, *act = Lf + G::O_ACT;
  int8_t *tile = reinterpret_cast<int8_t *>(convq_smem + LD::o_tile);
  int8_t *ptile = CI == 2 ? reinterpret_cast<int8_t *>(convq_smem + LD::o_prev) : nullptr;
  int *act_sh = reinterpret_cast<int *>(convq_smem + LD::o_flags), *over_sh = act_sh + G::ENVS;
  int *fresh_sh = CI == 2 ? over_sh + G::ENVS : nullptr;
  SgkRules &R = *reinterpret_cast<SgkRules *>(convq_smem + LD::o_rules);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int member = 0, member_wg = 0;
  if constexpr (MEMBERS) {
    member = (int)blockIdx.x / a.member_wgs;
    member_wg = (int)blockIdx.x - member * a.member_wgs;
    const size_t m = (size_t)member;  // this member's slice of the ten stacked tensors
    w1r += m * (C * G::K1); b1r += m * C; w2r += m * (C * G::K2); b2r += m * C; wbr += m * C; bbr += m * C; whr += m * (C * G::K2);
    bhr += m * C;
    wlr += m * (4 * G::NF); blr += m * 4;
  }
  CqLane<G> L;
  cq_setup<G, WW, C>(L, WL, act, w1r, w2r, whr, wlr);
  // this lane's board bytes of a pass: element i = t + CQ_WG * u = (env e, cell pos) of the row tile(s) -> its place in plane 0
  int b_lds[G::NB];
#pragma unroll
  for (int u = 0; u < G::NB; ++u) {
    const int i = t + CQ_WG * u;
    const bool live = i < G::ENVS * G::NC;
    const int e = live ? i / G::NC : 0, pos = live ? i - e * G::NC : 0;
    const int y = pos / WW, x = pos - y * WW;
    b_lds[u] = live ? e * G::ENV_F + G::CENTRE + y * G::PW + x : -1;
  }
  stage_rules(R, a.env.rules);  // ends with a workgroup barrier: weights, planes and rules are in place
  const int64_t n = a.env.n;
  // the envs this workgroup's passes cover (the batch's, or its member's) and which of their passes are its own
  int64_t first_env = 0, end_env = n;
  if constexpr (MEMBERS) {
    first_env = (int64_t)member * a.member_envs;
    end_env = first_env + a.member_envs;
  }
  const int64_t n_pass = (end_env - first_env + G::ENVS - 1) / G::ENVS;
  const bool mask_finished = (a.env.flags & SGK_F_MASK_FINISHED) != 0;
  const bool owner = t < G::ENVS;  // lanes of wave 0: one env each
  EpisodeAcc acc;
  acc_init(acc);
  for (int64_t pass = MEMBERS ? (int64_t)member_wg : (int64_t)blockIdx.x; pass < n_pass; pass += cr_pass_step<MEMBERS>(a)) {
    const int64_t env0 = first_env + pass * G::ENVS;
    const int hz = (int)(pass >> 44);  // (always 0: see cq_network)
    const int64_t env = env0 + t;
    const bool valid = owner && env < end_env;
    EnvState s = initial_state(R);
    if (valid) s = unpack_state(a.env.state[env]);
    load_episode_index<ENV>(s, a.env.n_resets, env, valid);
    int8_t *row = tile + (owner ? t : 0) * G::NC;
    if (owner) {
      write_row_bytes<ENV, G::NC>(R, row, s);  // draw this env's board from its state word
      over_sh[t] = (mask_finished && s.over) ? 1 : 0;
      if constexpr (CI == 2) fresh_sh[t] = a.fresh ? 1 : 0;
    }
    uint32_t rec = 0;
    const int64_t left = end_env - env0;
    const int lim = left < G::ENVS ? (int)left : G::ENVS;  // envs of this pass that exist
    if constexpr (CI == 2) {
      // the caller's previous rows (not used where the fresh flag stands; zeros for envs that do not exist)
#pragma unroll
      for (int u = 0; u < G::NB; ++u)
        if (b_lds[u] >= 0) {
          const int i = t + CQ_WG * u;
          ptile[i] = (!a.fresh && i / G::NC < lim) ? a.prev_boards[env0 * G::NC + i] : (int8_t)0;
        }
    }
    for (int k = 0; k < a.n_steps; ++k) {
      __syncthreads();  // the rows (and the finished / fresh flags) of this step are complete; the previous step's sums have been read
      // ---- rows -> plane 0 (float; CI = 2: previous -> plane 0, current -> plane 1) and -> the trajectory's states (zeros for envs whose
      // episode is over, SGK_F_MASK_FINISHED) ----
      int8_t *dst = a.states_out ? a.states_out + ((int64_t)k * n + env0) * G::NC : nullptr;
      int8_t *pdst = nullptr;
      if constexpr (CI == 2) pdst = a.prev_states_out ? a.prev_states_out + ((int64_t)k * n + env0) * G::NC : nullptr;
#pragma unroll
      for (int u = 0; u < G::NB; ++u)
        if (b_lds[u] >= 0) {
          const int i = t + CQ_WG * u;
          const int8_t v = tile[i];
          if constexpr (CI == 2) {
            const int e = i / G::NC;
            const int8_t pv = fresh_sh[e] ? v : ptile[i];
            act[b_lds[u]] = (float)pv;
            act[b_lds[u] + G::PL] = (float)v;
            if (e < lim) {
              if (dst) dst[i] = over_sh[e] ? (int8_t)0 : v;
              if (pdst) pdst[i] = over_sh[e] ? (int8_t)0 : pv;
            }
            ptile[i] = v;  // current -> previous
          } else {
            act[b_lds[u]] = (float)v;
            if (dst) {
              const int e = i / G::NC;
              if (e < lim) dst[i] = over_sh[e] ? (int8_t)0 : v;
            }
          }
        }
      __syncthreads();
      cq_network<G, C>(L, act, WL, hz, w1r, b1r, w2r, b2r, wbr, bbr, whr, bhr);
      if (wave == 0) {
        // ---- the outputs and the draw per env (lane = (env, action) quads), handed to the env's owner lane through LDS ----
        constexpr int NIT = (G::ENVS * 4 + 63) / 64;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int idx = it * 64 + lane;
          float q0, q1, q2, q3;
          cq_outputs<G>(act, blr, idx, q0, q1, q2, q3);
          if (idx < G::ENVS * 4 && (idx & 3) == 0) {
            const uint64_t ge = a.env.env_base + (uint64_t)(env0 + (idx >> 2));
            act_sh[idx >> 2] = a.mode == 0 ? pick_action<0>(q0, q1, q2, q3, ge, a.draw0 + (uint64_t)k, a.env.seed, a.eps)
                                           : pick_action<1>(q0, q1, q2, q3, ge, a.draw0 + (uint64_t)k, a.env.seed, a.eps);
          }
        }
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS operations execute in order)
        // ---- env.step by the owner lanes; action and record into the trajectory; the row re-drawn ----
        if (owner) {
          const int action = act_sh[t];
          const bool was_over = mask_finished && s.over;
          const int old_pos = s.pos, old_box = s.box;
          const int old_alt = HasAltBackdrop<ENV>::value ? alt_backdrop<ENV>(R, s) : 0;
          step_one<ENV>(R, a.env, env, valid, action, s, rec, acc);
          if (valid) {
            if (a.actions_out) a.actions_out[(int64_t)k * n + env] = was_over ? (uint8_t)0 : (uint8_t)action;
            if (a.recs_out) a.recs_out[(int64_t)k * n + env] = rec;
          }
          const int new_alt = HasAltBackdrop<ENV>::value ? alt_backdrop<ENV>(R, s) : 0;
          if (HasMask<ENV>::value || (HasAltBackdrop<ENV>::value && new_alt != old_alt)) {
            // the other backdrop (an auto-reset flipped the supervisor's coin; the button was pressed; the agent stepped on or off the
            // bucket) or a level whose cells change by themselves (tomatoes dry): the whole row
            write_row_bytes<ENV, G::NC>(R, row, s);
          } else if (s.pos != old_pos || s.box != old_box) {  // re-draw the cells this step changed (a reset included)
            const uint8_t *backdrop = backdrop_of(R, new_alt);
            row[old_pos] = (int8_t)backdrop[old_pos];
            if (HasSprite2<ENV>::value) {
              if (old_box < G::NC) row[old_box] = (int8_t)backdrop[old_box];
              if (s.box < G::NC) row[s.box] = (int8_t)sprite2_value<ENV>(R, s);
            }
            row[s.pos] = (int8_t)R.agent_value[s.pos];
          }
          over_sh[t] = (mask_finished && s.over) ? 1 : 0;
          // frame 0 behind a step: step_one reset the env (every other step leaves frame >= 1; an idle env keeps its own)
          if constexpr (CI == 2) fresh_sh[t] = ((a.env.flags & SGK_F_AUTO_RESET) && valid && s.frame == 0) ? 1 : 0;
        }
      }
    }
    if (valid) {
      a.env.state[env] = pack_state(s);
      a.env.rec[env] = rec;  // the env's own boards are re-materialised by the caller (launch_reset mode 2)
    }
    if constexpr (CI == 2) {
      __syncthreads();  // the last step's rows and fresh flags are complete
      // the previous-board channel of the observation the next action would be chosen on, back to the caller's array
#pragma unroll
      for (int u = 0; u < G::NB; ++u)
        if (b_lds[u] >= 0) {
          const int i = t + CQ_WG * u, e = i / G::NC;
          if (e < lim) a.prev_boards[env0 * G::NC + i] = fresh_sh[e] ? tile[i] : ptile[i];
        }
    }
    __syncthreads();  // nobody still reads this pass's rows when the next pass's owners draw theirs
  }
  acc_flush(acc, a.env.metrics);
  if constexpr (MEMBERS) {
    if (a.member_metrics) acc_flush_row(acc, a.member_metrics + (size_t)member * SGK_METRICS_LEN);  // the same reduction, this member's row
  }
}

// One launch of convq_rollout_kernel<E, CV, MEMBERS, CI>. The grid: one workgroup per pass while they fit the chip; MEMBERS: a member's
// workgroups are one per pass while all members' fit the chip (one member: the single kernel's grid), at least one.
template <int E, int CV, bool MEMBERS, int CI>
static hipError_t convq_rollout_launch(const Shard &sh, const ConvQWeights &w, ConvRolloutArgsFor<MEMBERS, CI> a, int n_members, hipStream_t st) {
  typedef ConvRolloutLds<E, CV, CI> LD;
  constexpr size_t lds = LD::bytes;
  static_assert(lds <= 160u * 1024u, "convq rollout LDS plan");
  if (Geom<E>::H != sh.rules_host.height || Geom<E>::W != sh.rules_host.width) return hipErrorInvalidValue;
  hipError_t ae = allow_dynamic_lds<convq_rollout_kernel<E, CV, MEMBERS, CI>>(sh.device, (int)lds);
  if (ae != hipSuccess) return ae;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(CQ_ROLLOUT_WAVES_FOR(CV), (160u * 1024u) / lds));
  int grid = grid_for((sh.n + LD::G::ENVS - 1) / LD::G::ENVS, sh.n_cus * per_cu);
  if constexpr (MEMBERS) {
    a.member_wgs = grid_for((a.member_envs + LD::G::ENVS - 1) / LD::G::ENVS, std::max(sh.n_cus * per_cu / n_members, 1));
    if ((int64_t)n_members * a.member_wgs > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    grid = n_members * a.member_wgs;
  }
  convq_rollout_kernel<E, CV, MEMBERS, CI><<<dim3(grid), dim3(CQ_WG), lds, st>>>(a, w.w1, w.b1, w.w2, w.b2, w.wb, w.bb, w.wh, w.bh, w.wl, w.bl);
  return hipGetLastError();
}

static void convq_rollout_args(ConvRolloutArgs &a, const Shard &sh, int mode, double eps, uint64_t draw0, int32_t n_steps, uint32_t flags,
                               int8_t *states_out, uint8_t *actions_out, uint32_t *recs_out) {
  a.env = make_step_args(sh, nullptr, flags);
  a.eps = eps;
  a.draw0 = draw0;
  a.n_steps = n_steps;
  a.mode = mode;
  a.states_out = states_out;
  a.actions_out = actions_out;
  a.recs_out = recs_out;
}

// n_members == 0: sgk_convq_rollout's own kernel; >= 1: the member instantiation (sgk_convq_rollout_members)
hipError_t launch_convq_rollout(const Shard &sh, const ConvQWeights &w, int n_channels, int mode, double eps, uint64_t draw0, int32_t n_steps,
                                uint32_t flags, int8_t *states_out, uint8_t *actions_out, uint32_t *recs_out, hipStream_t st, int n_members,
                                int64_t *member_metrics) {
  (void)hipGetLastError();
  if (n_members < 0 || (n_members > 0 && sh.n % n_members != 0)) return hipErrorInvalidValue;
  ConvRolloutMemberArgs a;
  convq_rollout_args(a, sh, mode, eps, draw0, n_steps, flags, states_out, actions_out, recs_out);
  a.member_envs = n_members > 0 ? sh.n / n_members : sh.n;
  a.member_wgs = 0;
  a.member_metrics = reinterpret_cast<long long *>(member_metrics);
  hipError_t err = hipErrorInvalidValue;
  SGK_DISPATCH_ENV(sh.env_id, {
    err = cq_dispatch_channels(n_channels, [&](auto channels) {
      constexpr int CV = decltype(channels)::value;
      return n_members == 0 ? convq_rollout_launch<E, CV, false, 1>(sh, w, a, 0, st) : convq_rollout_launch<E, CV, true, 1>(sh, w, a, n_members, st);
    });
  });
  return err;
}

// BoatRace's 5 x 5 board (the level TransitionBoatRace wraps); another level is a dispatch line
hipError_t launch_convq_rollout_trans(const Shard &sh, const ConvQWeights &w, int n_channels, int mode, double eps, uint64_t draw0,
                                      int32_t n_steps, uint32_t flags, int8_t *prev_boards, int fresh, int8_t *states_out,
                                      int8_t *prev_states_out, uint8_t *actions_out, uint32_t *recs_out, hipStream_t st) {
  (void)hipGetLastError();
  if (sh.env_id != SGK_BOAT_RACE || !prev_boards) return hipErrorInvalidValue;
  ConvRolloutTransArgs a;
  convq_rollout_args(a, sh, mode, eps, draw0, n_steps, flags, states_out, actions_out, recs_out);
  a.prev_boards = prev_boards;
  a.prev_states_out = prev_states_out;
  a.fresh = fresh ? 1 : 0;
  return cq_dispatch_channels(n_channels, [&](auto channels) {
    return convq_rollout_launch<SGK_BOAT_RACE, decltype(channels)::value, false, 2>(sh, w, a, 0, st);
  });
}

}  // namespace sgk

