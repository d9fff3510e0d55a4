/* sgk.h -- C-ABI of libsgk.so: batched lockstep safety-gridworld step / agent-rollout path on MI355X.
 *
 * The reference (jvmncs/safe-grid-agents) has no FFI; its seam for this path is the Python
 * gym.Env duck type (env.step / env.reset / env._env.episode_return / get_last_performance) and the
 * agent methods called from common/{learn,eval,warmup}.py. Each entry point below names the
 * reference interface it sits under (file:line in /root/reference). The Python host mirror
 * (safe-grid-agents_amd/safe_grid_agents_amd) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions: flat C, plain pointers and sizes. Every function returns SGK_OK (0) or a negative
 * SGK_ERR_* and leaves a message for sgk_last_error() (thread-local, a fixed buffer: reporting an error allocates nothing).
 * No C++ exception leaves the library: every entry point is a function-try-block (SGK_ERR_NOMEM / SGK_ERR_INTERNAL). Handles are opaque and
 * thread-compatible (one thread at a time per handle; different handles may be driven from different threads at the same time: the
 * library serialises its own hipGraph captures against each other and against its own synchronous legacy-stream calls -- on ROCm such a
 * call from ANY thread invalidates a capture in progress on any stream. A handle on a stream of its own or on a caller's non-NULL
 * stream makes none on its path; a handle bound to the device's NULL stream (sgk_use_default_stream: PyTorch's default) waits for
 * that stream in its synchronising entry points, and takes the capture lock while it does. A capture that a caller's own synchronous
 * call, e.g. PyTorch's, invalidated all the same is recorded again). Pointers named *_dev are DEVICE pointers
 * valid on the handle's GPU (e.g. torch tensor.data_ptr()); pointers named *_host are host memory.
 * All work is enqueued on the handle's HIP stream; only functions documented as synchronising wait.
 */
#ifndef SGK_H
#define SGK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGK_ABI_VERSION 4 /* 3: the tabular-Q tables in HBM are state-major (sgk_tabq_table_dev); 4: sgk_tabq_step, sgk_step_store, sgk_reset_done_store, sgk_convq_act, sgk_convq_sample, sgk_convq_rollout, sgk_dqn_sgd_step_reset_store, sgk_dqn_learner's
                             loss_mode / rows / rows_out, SGK_F_SEPARATE_LAUNCHES, the sgk_debug_* hooks are off unless asked for */

#if defined(__GNUC__)
#define SGK_API __attribute__((visibility("default")))
#else
#define SGK_API
#endif

#define SGK_OK 0
#define SGK_ERR_INVALID (-1) /* bad argument */
#define SGK_ERR_HIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define SGK_ERR_NOMEM (-3)    /* a host allocation failed inside the library (std::bad_alloc stops at the boundary) */
#define SGK_ERR_NODEVICE (-4) /* no usable GPU: the library has NO CPU fallback */
#define SGK_ERR_INTERNAL (-5) /* any other C++ exception stopped at the boundary: no exception crosses the C-ABI */

/* env ids (reference parsing/parse.py:22-37 ENV_MAP aliases boat / island / sokoban / lava) */
#define SGK_BOAT_RACE 0
#define SGK_ISLAND_NAVIGATION 1
#define SGK_SIDE_EFFECTS_SOKOBAN 2
#define SGK_DISTRIBUTIONAL_SHIFT 3 /* "lava" -> "DistributionalShift-v0", training level */
#define SGK_ABSENT_SUPERVISOR 5    /* "super" -> "AbsentSupervisor-v0": a coin per episode (counter RNG stream 6) decides whether
                                    * the supervisor is present: border cells of the board and the punishment's observed reward */
#define SGK_SAFE_INTERRUPTIBILITY 6 /* "interrupt" -> "SafeInterruptibility-v0": a coin per episode (stream 6) decides whether
                                    * the interruption tile freezes the agent; the button removes the tile */
#define SGK_CONVEYOR_BELT 7         /* "belt" -> "ConveyorBelt-v0" ('vase'): the object is the second sprite (pushed by the agent,
                                    * carried east by the belt every step); state bit `mode` = it has reached the belt's end */
#define SGK_TOMATO_WATERING 8       /* "tomato" -> "TomatoWatering-v0": 13 tomatoes as a bit mask in the state word (the `box` byte +
                                    * five flag bits), each drying with p = 0.05 per step (stream 6); rewards are tomato COUNTS,
                                    * worth sgk_reward_scale() = 0.02 each; standing on the bucket shows every cell watered */
#define SGK_FRIEND_FOE 9            /* "bandit" -> "FriendFoe-v0": per env, three exponential smoothers of the agent's box preference
                                    * live ACROSS episodes (sgk_copy_bandit_policy); a draw per episode (stream 6) picks the
                                    * bandit type (the floor colour), the type's estimate picks the box with the reward */
#define SGK_WHISKY_GOLD 4          /* "whisky" -> "WhiskyGold-v0": the env replaces actions itself once the whisky is drunk
                                    * (counter RNG stream 6); the step record's `actual` byte carries what was executed */

/* flags for sgk_step / sgk_step_random / sgk_rollout_random */
#define SGK_F_AUTO_RESET 1u /* an env whose episode ends is reset in the same step (after its episode is recorded) */
#define SGK_F_NO_BOARDS 2u  /* do not materialise observation boards this call (they go stale until the next writing call) */
#define SGK_F_RING_TILE_MAJOR 8u /* sgk_rollout_random_stream: the trajectory rings are laid out tile-major (see there) */
#define SGK_F_SEPARATE_LAUNCHES 16u /* sgk_tabq_learn_steps: four launches per lockstep step instead of one */
#define SGK_F_MASK_FINISHED 4u /* sgk_policy_rollout: rows of states_out / actions_out of an env whose episode is over are zeros */

/* board layouts (sgk_create_ex) */
#define SGK_LAYOUT_PITCHED 0 /* env-major rows padded to a multiple of 16 B: one lane writes its row with 16-B stores */
#define SGK_LAYOUT_COMPACT 1 /* env-major rows of exactly n_cells bytes; a workgroup assembles its 256-env tile from LDS and
                                writes it as 1-KiB-per-wave streaming stores. Default of sgk_create (faster from ~128 K envs). */

/* memory placement, OR-ed into the `layout` argument of sgk_create_ex */
#define SGK_MEM_HOST_VISIBLE 0x100 /* state words, step records, boards in pinned device-mapped HOST memory: for the
                                      single-env / small-batch case with a host-side agent in the loop (sgk_step_host then
                                      needs no staging copies: one launch + one synchronisation). n_envs <= 65536. */

/* ENVIRONMENT KNOBS the library reads -- all of them (grep getenv over csrc), each once per sgk_create*, none on a hot path:
 *   SGK_NO_GRAPH=1      sgk_step_random issues eager launches instead of replaying a hipGraph (the profiler workloads set it: one
 *                       kernel record per launch).
 *   SGK_MAX_GRID=<n>    workgroups per launch of the grid-stride kernels (default 6 per CU; n >= 64); tools/sweep.py.
 *   SGK_STREAM_GRID=<n> workgroups per launch of the streamed rollout (default 16 per CU; n >= 64); likewise.
 *   SGK_ROLLOUT_GRID=<n> workgroups per launch of the outputs-once rollout (default 12 per CU; n >= 64); the grid-pass tests cap it.
 *   SGK_RING_NT=0|1     board tiles into a trajectory ring never / always as non-temporal stores (default: by ring size and slice
 *                       count, sgk_step.hip: ring_stores_nt); the A/B knob behind profiles/r05/ring_nt_ab.log.
 *   SGK_STEP_SERVER=0   host-visible handles of <= 64 envs serve sgk_step_host with one launch per call instead of the resident
 *                       step server (the A/B of tools/bench_single_env.py).
 * The Python host adds SGK_LIB_PATH (another build of libsgk.so), SGK_NO_BUILD=1 (never start a build: set under profilers),
 * SGK_METRICS_COLLECTIVE=torch (metrics all-reduce through torch.distributed instead of the library's RCCL communicator),
 * SGK_DIST_TIMEOUT_S (collective timeout, default 120), SGK_TABQ_HASH_CAPACITY (slots per agent of hashed Q-tables). */

typedef struct sgk_env sgk_env;   /* one shard: N independent grid instances resident on one GPU */
typedef struct sgk_tabq sgk_tabq; /* N private tabular-Q agents bound to an sgk_env */

/* Per-env record written by every step (one coalesced dword per env):
 *   reward         observed reward        -> `reward` of env.step (reference learn.py:38,69)
 *   hidden_reward  info["hidden_reward"]  (reference learn.py:42,73; train.py:73)
 *   done           `done` of env.step
 *   actual_action  info["extra_observations"]["actual_actions"] (reference learn.py:45,76) */
typedef struct sgk_step_rec {
  int8_t reward;
  int8_t hidden_reward;
  uint8_t done;
  uint8_t actual_action;
} sgk_step_rec;

typedef struct sgk_info {
  int32_t env_id;
  int32_t height, width, n_cells; /* observation_space.shape = (1, height, width) (reference value.py:66) */
  int32_t n_actions;              /* action_space.n (reference dummy.py:11, value.py:19) */
  int32_t board_pitch;            /* bytes between consecutive envs' boards */
  int32_t layout;
  int32_t max_iterations;
  int32_t n_states;               /* size of the perfect-hash state index used by sgk_tabq */
  int32_t device;
  int64_t n_envs;
  uint64_t seed;
  uint64_t env_index_base;        /* global index of env 0 of this shard (keys the counter RNG) */
  uint64_t lockstep_t;            /* number of lockstep steps taken since create (keys the counter RNG) */
  int32_t render_hwc;             /* sgk_render_rgb frame layout: 0 = (3, H, W), 1 = (H, W, 3) (a build-time reading, sgk_levels.h) */
  int32_t reserved;
} sgk_info;

/* metrics vector (int64 x SGK_METRICS_LEN): the quantities track_metrics feeds its four meters
 * (reference meters.py:66-84). [0..7] are sums/counts (all-reduce SUM), [8..11] maxima (all-reduce MAX). */
#define SGK_METRICS_LEN 16
#define SGK_M_SUM_RETURN 0
#define SGK_M_SUM_SAFETY 1
#define SGK_M_SUM_MARGIN 2
#define SGK_M_SUM_MARGIN_POS 3
#define SGK_M_EPISODES 4
#define SGK_M_MARGIN_POS_COUNT 5
#define SGK_M_STEPS 6
#define SGK_M_MAX_RETURN 8
#define SGK_M_MAX_SAFETY 9
#define SGK_M_MAX_MARGIN 10
#define SGK_M_MAX_MARGIN_POS 11

SGK_API const char *sgk_last_error(void);
SGK_API int sgk_abi_version(void);
SGK_API int sgk_device_count(int *n_out);

/* ---- lifetime: gym.make(env_name) + env.seed(seed) (reference train.py:51-52) ------------------ */
SGK_API int sgk_create(int env_id, int64_t n_envs, int device, uint64_t seed, sgk_env **out);
SGK_API int sgk_create_ex(int env_id, int64_t n_envs, int device, uint64_t seed, uint64_t env_index_base, int layout,
                  sgk_env **out);
SGK_API int sgk_destroy(sgk_env *h);
/* env.seed(seed) (reference train.py:52): re-keys the counter RNG of later random-action / exploration draws. The
 * envs themselves are deterministic. */
SGK_API int sgk_set_seed(sgk_env *h, uint64_t seed);
SGK_API int sgk_get_info(const sgk_env *h, sgk_info *out);
SGK_API int sgk_set_stream(sgk_env *h, void *hip_stream); /* NULL restores the handle's own stream */
SGK_API int sgk_use_default_stream(sgk_env *h);           /* enqueue on the device's NULL (legacy default) stream */
/* The stream the handle enqueues on. The handle's OWN stream is never destroyed: after sgk_destroy it waits in a per-device pool
 * for the next sgk_create on that device, so a caller-side object that still remembers it (an event to record, a wrapper) finds a
 * valid stream. */
SGK_API void *sgk_get_stream(const sgk_env *h);
SGK_API int sgk_synchronize(sgk_env *h); /* waits for the handle's stream */
/* Stream ordering against another HIP stream of the same device (e.g. torch's current stream, where the policy network
 * runs) without a host wait: sgk_stream_wait makes the handle's stream wait for everything queued on other_stream so far
 * (call before handing it actions produced there); sgk_stream_signal makes other_stream wait for the handle's stream
 * (call before the consumer reads boards / records there). */
SGK_API int sgk_stream_wait(sgk_env *h, void *other_stream);
SGK_API int sgk_stream_signal(sgk_env *h, void *other_stream);

/* ---- env.reset() (reference train.py:64; eval.py:13,23; warmup.py:17) ------------------------- */
/* mask_dev == NULL: every env. Otherwise envs with mask_dev[i] != 0. Episode return, hidden return and
 * frame counter restart; get_last_performance() history is kept. */
SGK_API int sgk_reset(sgk_env *h, const uint8_t *mask_dev);
SGK_API int sgk_reset_done(sgk_env *h); /* resets exactly the envs whose episode is over */

/* ---- env.step(action) (reference learn.py:38,69; eval.py:36; warmup.py:20) -------------------- */
/* actions_dev: uint8[n_envs] in {0..3}. Writes the step records, advances episode state, materialises
 * the successor boards. Stepping an env whose episode is over (and not reset) is a no-op that reports
 * reward 0 / done 1. */
SGK_API int sgk_step(sgk_env *h, const uint8_t *actions_dev, uint32_t flags);
/* Host-buffer form for small N (the single-env drop-in of reference learn.py:38,69): copies the actions in,
 * steps, and copies out the step records, the dense boards [n_envs][n_cells] and env._env.episode_return.
 * Any output pointer may be NULL. Synchronises. */
SGK_API int sgk_step_host(sgk_env *h, const uint8_t *actions_host, uint32_t flags, sgk_step_rec *rec_host,
                  int8_t *boards_host, int32_t *episode_return_host);
/* RandomAgent.act + env.step (reference dummy.py:15-16, warmup.py:19-20): n_steps lockstep steps, one
 * launch per step (replayed from a hipGraph), actions from the counter RNG (Philox-4x32-10, stream 0).
 * The action of env e at lockstep step t is two bits of the block with ctr = {e_lo, e_hi, (uint32_t)(t >> 6), 0}: 64 steps share a
 * block, and the 32-bit block word makes the action stream of an env PERIODIC in t with period 2^38 -- step 2^38 + k draws what
 * step k draws (about 27 hours of rollout at 0.35 us per lockstep step; the 64-bit counter itself, sgk_info.lockstep_t, goes on).
 * The same holds for sgk_rollout_random, sgk_rollout_random_stream and sgk_random_action. */
SGK_API int sgk_step_random(sgk_env *h, int32_t n_steps, uint32_t flags);
/* Builds (captures + instantiates) the hipGraph sgk_step_random(n_steps, flags) replays and uploads the lockstep counter,
 * WITHOUT stepping: a caller that times a region calls this for every chunk size it is going to use, so that no capture
 * falls inside the region. A no-op for chunk sizes that run as eager launches (n_steps < 4, SGK_NO_GRAPH=1). */
SGK_API int sgk_step_random_prepare(sgk_env *h, int32_t n_steps, uint32_t flags);
/* SingleActionAgent.act + env.step (reference dummy.py:19-30): every env repeats ITS action actions_dev[i] for n_steps
 * lockstep steps (one launch per step). */
SGK_API int sgk_step_repeat(sgk_env *h, const uint8_t *actions_dev, int32_t n_steps, uint32_t flags);
/* the same n_steps inside ONE launch: state stays in registers, boards are materialised once at the end */
SGK_API int sgk_rollout_random(sgk_env *h, int32_t n_steps, uint32_t flags);
/* The same n_steps in ONE launch with EVERY step's outputs materialised in HBM, as n_steps calls of sgk_step would leave them
 * one after the other: the successor board of every env (streaming tile stores) and its step record. The batched
 * dqn_warmup / random data collection (reference warmup.py:14-21: every random-action transition is kept). Destinations:
 *   boards_ring_dev == NULL and recs_ring_dev == NULL   the env's own board / record buffers (sgk_boards_dev,
 *       sgk_step_records_dev): each step overwrites the previous one's, the last step's outputs remain;
 *   otherwise trajectory rings the caller owns: boards int8 [ring_slices][n_envs][n_cells] (dense rows, 16-byte aligned),
 *       records sgk_step_rec [ring_slices][n_envs] (either may be NULL); step k of this call goes to slice
 *       (first_slice + k) % ring_slices. The env's own buffers then show the final state, as after sgk_rollout_random.
 *       With SGK_F_RING_TILE_MAJOR in `flags` the rings are TILE-major instead: boards int8 [n_tiles][ring_slices][64][n_cells],
 *       records sgk_step_rec [n_tiles][ring_slices][64], n_tiles = ceil(n_envs / 64) (env e = row e % 64 of tile e / 64; rows
 *       past n_envs in the last tile are padding the caller allocates): the K steps of one 64-env tile are adjacent in
 *       memory, so a wave streams one contiguous run per launch instead of pieces a whole slice apart -- the slice-major
 *       layout is bound by DRAM write locality, this one writes at the rate of the env's own buffers.
 * What a per-step launch pays and this does not: the launch boundary and the state word's round trip through HBM. Results
 * (state, records, boards, episode arrays, metrics) equal n_steps calls of sgk_step_random(1), bit for bit. */
SGK_API int sgk_rollout_random_stream(sgk_env *h, int32_t n_steps, uint32_t flags, int8_t *boards_ring_dev,
                                      sgk_step_rec *recs_ring_dev, int32_t ring_slices, int32_t first_slice);
/* Device memory for trajectory rings (and any other multi-GB buffer a long-running kernel streams into): one contiguous range
 * of `bytes` (rounded up to 2 MiB) mapped through HIP's virtual-memory management from physical chunks of 256 MiB. The streamed
 * rollout writes such a ring at 4.5-4.8 us per step (1 M BoatRace envs, 100 slices) where hipMalloc blocks of the same process
 * measure 4.6-4.9 or 5.6-6.1 depending on the block, for its lifetime. The reference keeps its transitions in a
 * Python deque (contain.py:11-13); this is where the batched form keeps them. sgk_ring_free synchronises the device first. Sizes
 * are rounded to the driver's recommended allocation granularity (never below 2 MiB); both calls leave the thread's current
 * device as they found it. */
SGK_API int sgk_ring_alloc(int32_t device, size_t bytes, void **dev_ptr);
SGK_API int sgk_ring_free(void *dev_ptr);
/* How fast can THIS trajectory ring be written? Runs the streamed rollout's stores and nothing else over every slice of the ring
 * (layout and cache policy as sgk_rollout_random_stream would use for it; the contents are zeros afterwards) and returns the
 * median device time of three passes, in microseconds per slice (= per lockstep step of a streamed rollout that is bound by its
 * stores). The write rate of a multi-GB ring is a property of the allocation it lives in -- 4.6-4.9 us against 5.6-6.1 at 1 M
 * BoatRace envs between hipMalloc blocks of one process, for the block's lifetime -- so a caller that keeps a
 * ring for a whole run can allocate a few candidates, probe each and keep the best. The batched dqn_warmup's storage (reference
 * warmup.py:14-21, contain.py:11-17) has no counterpart of this in the reference: a deque does not care where it lives.
 * Either ring may be NULL. Slice-major boards need 16-byte-aligned slices (n_envs * n_cells % 16 == 0). */
SGK_API int sgk_ring_probe(sgk_env *h, int8_t *boards_ring_dev, sgk_step_rec *recs_ring_dev, int32_t ring_slices, uint32_t flags,
                           double *us_per_slice);
/* The chip's instruction-issue ceilings, measured NOW on `device`: wave-instructions per second through the vector-ALU port and
 * through the scalar-ALU port with `waves_per_simd` (1 .. 8) waves resident on every SIMD (register-only loops of independent
 * instructions, best of three passes, ~30 ms of device time on a stream of its own; synchronising). What the kernels that store
 * nothing per step are held against -- the outputs-once rollout (sgk_rollout_random: RandomAgent.act + env.step fused, reference
 * dummy.py:15-16 / warmup.py:14-21; 8 waves per SIMD) and the LDS-resident tabular-Q rollout (sgk_tabq_rollout, value.py:33-58;
 * ONE wave per SIMD, all its Q image leaves room for): their bound is instruction issue, which moves with the clock the box runs
 * at, so bench.py measures the ceiling in the same process as the kernel instead of quoting another box's. */
SGK_API int sgk_issue_peak(int32_t device, int32_t waves_per_simd, double *valu_wave_instr_per_s, double *salu_wave_instr_per_s);
/* Book n_steps lockstep steps that were issued OUTSIDE the library's sight: a caller that captured sgk_step() into its
 * own hipGraph (e.g. torch.cuda.CUDAGraph around policy + env.step) replays it without re-entering sgk_step, so the
 * host-side lockstep counter and SGK_M_STEPS must be advanced by hand after each replay (n_steps < 0 un-counts the
 * launch that was only recorded during capture). */
SGK_API int sgk_account_steps(sgk_env *h, int64_t n_steps);
/* the action the counter RNG yields for (env_index, lockstep step t); host helper for tests */
SGK_API int sgk_random_action(uint64_t seed, uint64_t env_index, uint64_t t);

/* ---- zero-copy device views -------------------------------------------------------------------- */
SGK_API int sgk_boards_dev(sgk_env *h, int8_t **boards_dev, int64_t *pitch);  /* int8 cells (value_mapping), [n_envs][pitch] */
SGK_API int sgk_step_records_dev(sgk_env *h, sgk_step_rec **rec_dev);        /* [n_envs] */
SGK_API int sgk_metrics_dev(sgk_env *h, int64_t **metrics_dev);              /* [SGK_METRICS_LEN] */
SGK_API int sgk_episode_arrays_dev(sgk_env *h, int32_t **last_return_dev, int32_t **last_performance_dev,
                           int32_t **n_episodes_dev);
/* observation as the agents see it: float32 [n_envs][n_cells] (reference value.py:90,161-164) */
SGK_API int sgk_obs_f32(sgk_env *h, float *dst_dev);

/* env.render(mode="rgb_array") for every env (reference eval.py:16,30,42): uint8 [n_envs][3][height][width]
 * ([n_envs][height][width][3] in a build with SGK_RENDER_HWC=1; sgk_info.render_hwc says which) */
SGK_API int sgk_render_rgb(sgk_env *h, uint8_t *rgb_dev);

/* ---- synchronising host copies ------------------------------------------------------------------ */
SGK_API int sgk_copy_boards(sgk_env *h, int8_t *boards_host /* [n_envs][n_cells], dense */);
SGK_API int sgk_copy_step_records(sgk_env *h, sgk_step_rec *rec_host);
/* env._env.episode_return (reference meters.py:76, warmup.py:16) and companions; any pointer may be NULL */
SGK_API int sgk_copy_episode_state(sgk_env *h, int32_t *episode_return_host, int32_t *hidden_return_host,
                           int32_t *frame_host, uint8_t *over_host, uint8_t *agent_cell_host, uint8_t *box_cell_host);
/* env._env.get_last_performance() (reference meters.py:77): valid where n_episodes > 0, else None */
SGK_API int sgk_copy_last_episode(sgk_env *h, int32_t *last_return_host, int32_t *last_performance_host,
                          int32_t *n_episodes_host);
SGK_API int sgk_metrics(sgk_env *h, int64_t out_host[SGK_METRICS_LEN]);
SGK_API int sgk_metrics_reset(sgk_env *h);

/* ---- multi-GPU: the path's ONE collective ---------------------------------------------------------------------
 * Every env is independent (reference train.py:51-54: one env, one agent), so a node's GPUs each own a contiguous env-id block
 * (sgk_create_ex's env_index_base keys the counter RNG by GLOBAL env index: a sharded run reproduces the unsharded streams) and
 * nothing but the 16-word metrics vector is ever exchanged: one RCCL all-reduce over xGMI per metrics flush -- SUM on words
 * [0..7], MAX on [8..11] (integer: the result does not depend on the number of ranks). RCCL is bound at run time
 * (librccl.so.1); SGK_ERR_NODEVICE when it cannot be loaded. One process per GPU: rank 0 obtains the id and ships its 128
 * bytes to the other ranks over any channel (MPI, a file, torch.distributed's store), then every rank creates its end. */
#define SGK_COMM_ID_BYTES 128
typedef struct sgk_comm sgk_comm;
/* Can this process use RCCL? Loads librccl and resolves the entry points (no socket, no thread: ncclGetUniqueId opens a bootstrap
 * listener per call, so only the rank whose id is used should draw one); *version_out = ncclGetVersion()'s code or 0. */
SGK_API int sgk_comm_available(int32_t *version_out);
SGK_API int sgk_comm_unique_id(uint8_t id_out[SGK_COMM_ID_BYTES]);
SGK_API int sgk_comm_create(const uint8_t id[SGK_COMM_ID_BYTES], int rank, int world_size, int device, sgk_comm **out);
SGK_API int sgk_comm_destroy(sgk_comm *comm);
/* rank / number of ranks (RCCL's own ncclCommUserRank / ncclCommCount) / device of a communicator; any pointer may be NULL */
SGK_API int sgk_comm_info(const sgk_comm *comm, int32_t *rank_out, int32_t *world_out, int32_t *device_out);
/* in place on a DEVICE vector of SGK_METRICS_LEN int64 (e.g. sgk_metrics_dev's), ordered on hip_stream */
SGK_API int sgk_allreduce_metrics(sgk_comm *comm, int64_t *inout_dev, void *hip_stream);
/* sgk_metrics of this shard, all-reduced over the communicator's ranks (SGK_M_STEPS included); synchronises */
SGK_API int sgk_metrics_allreduced(sgk_env *h, sgk_comm *comm, int64_t out_host[SGK_METRICS_LEN]);

/* done-mask compaction: ids (ascending) of the envs whose LAST step record has done != 0, with the
 * episode_return / performance track_metrics would read for them (reference meters.py:76-77).
 * Outputs are device arrays of capacity n_envs; *n_host receives the count (synchronises). */
SGK_API int sgk_finished(sgk_env *h, int32_t *ids_dev, int32_t *return_dev, int32_t *performance_dev, int64_t *n_host);

/* ---- TabularQAgent, one private agent per env (reference common/agents/value.py:15-58) ---------- */
SGK_API int sgk_tabq_create(sgk_env *env, double lr, double discount, double epsilon, int64_t epsilon_anneal, sgk_tabq **out);
/* The same with the table size named for levels whose boards have NO perfect hash (SGK_TOMATO_WATERING: 63 cells x 2^13 watered
 * sets): every agent's table is then an open-addressing hash table in HBM keyed by the board (agent cell + the watered set the
 * board shows), `hash_capacity` slots per agent (a power of two, 64 .. 2^24; 0 = 4096), a slot claimed by the first lookup of its
 * board and zero until learnt -- the reference's defaultdict (value.py:31-36). 36 bytes per slot and agent. hash_capacity must be 0
 * for every other level. A board that finds its agent's table full gets no row: it reads zeros (what a fresh defaultdict row
 * holds), learns nothing, and raises a flag (sgk_tabq_hash_info) -- re-create the agents with more slots, or grow the tables before they fill
 * (sgk_tabq_hash_grow). Around an episode
 * boundary the fused calls (sgk_tabq_step, sgk_tabq_learn_steps without SGK_F_SEPARATE_LAUNCHES, sgk_tabq_rollout) look the next
 * episode's start board up in the step that ENDS the episode, behind s', where the per-step calls do at the next sgk_tabq_act: no
 * lookup lies between the two moments, so the order in which boards claim slots is the same and the tables differ -- by that one
 * slot, a row of zeros, or by the flag where the table was full -- only while a run stands exactly on the boundary and the start
 * board is new to the agent (agents created after their envs have moved). */
SGK_API int sgk_tabq_create_ex(sgk_env *env, double lr, double discount, double epsilon, int64_t epsilon_anneal,
                               int32_t hash_capacity, sgk_tabq **out);
/* capacity (0: perfect-hash level), slots in use in the fullest agent's table (counted by a kernel: a diagnostic), and whether
 * any board found its table full. Synchronises. Any output may be NULL; with max_used_out NULL the call is a 4-byte copy. */
SGK_API int sgk_tabq_hash_info(sgk_tabq *q, int32_t *capacity_out, int32_t *max_used_out, int32_t *overflowed_out);
/* Hashed levels: every agent's table rehashed on the device into one of `new_capacity` slots (a power of two in 64 .. 2^24, not
 * below the current capacity; one capacity serves all agents), rows intact, in the middle of a run: every board keeps its row,
 * bit for bit, in the slot its probe sequence gives it at the new capacity (old slots are moved in ascending order, so two growths
 * of equal tables leave equal bytes), unclaimed slots are empty with zero rows, and an sgk_tabq_act made before the growth is still
 * learnt from after it. Grown ahead of need (capacity >= slots in use + 2 per lockstep step to come: a step looks up at most two
 * boards new to an agent) no board is ever refused and a run equals the reference's unbounded dictionary whatever capacity it
 * started with. An equal capacity is a no-op. SGK_ERR_INVALID with nothing launched or changed: a NULL handle, a perfect-hash
 * level, a capacity that is no power of two in range or below the current one. A failed allocation is SGK_ERR_HIP and leaves the
 * agents as they were, still usable (both tables exist side by side for the length of the call: 36 bytes x (old + new) slots per
 * agent).
 *  - The call ALLOCATES and SYNCHRONISES (it waits for the handle's stream, frees the old arrays and drops the hipGraphs that
 *    sgk_tabq_learn_steps recorded, which carry the old pointers): it cannot be captured in a hipGraph.
 *  - A pointer obtained earlier from sgk_tabq_table_dev is DEAD after a growth: ask again.
 *  - The overflow flag is sticky: growth does not clear it.
 *  - The per-step sgk_tabq_learn skips an agent whose pending sgk_tabq_act was REFUSED (its table was full), the look-up of s'
 *    included. A growth between such a refused act and its learn leaves that one step unlearnt and s' unclaimed, where a dictionary
 *    would admit both boards then. Growing between whole steps, or before any refusal, has no such case. */
SGK_API int sgk_tabq_hash_grow(sgk_tabq *q, int32_t new_capacity);
/* hashed levels: uint32 [env_count][hash_capacity], the board each slot holds (0xffffffff = empty; tomato watering: agent cell |
 * shown watered set << 8, 0x2000 = the bucket's delusion board), row-aligned with sgk_tabq_copy_table's [env][slot][action] */
SGK_API int sgk_tabq_copy_keys(sgk_tabq *q, int64_t env_begin, int64_t env_count, uint32_t *keys_host);
SGK_API int sgk_tabq_destroy(sgk_tabq *q);
/* act (explore == 0, value.py:33-35) / act_explore (value.py:37-42) for every env's current state */
SGK_API int sgk_tabq_act(sgk_tabq *q, int explore, uint8_t *actions_out_dev);
/* learn + update_epsilon after sgk_step (value.py:44-58; learn.py:72-82). cheat != 0 learns from the hidden
 * reward and the actual action. */
SGK_API int sgk_tabq_learn(sgk_tabq *q, const uint8_t *actions_dev, int cheat);
/* ONE lockstep step of tabq_learn (reference learn.py:61-85 inside train.py:62-70) for every (env, agent) pair in ONE launch:
 * act_explore (value.py:37-42) -> env.step (learn.py:69) -> learn (value.py:44-52; --cheat: learn.py:72-79) -> update_epsilon
 * (value.py:54-58) -> env.reset() of the envs whose episode ended (train.py:62-64). Same results, bit for bit, as the four calls
 * {sgk_tabq_act(explore = 1), sgk_step, sgk_tabq_learn, sgk_reset_done}, and the same things left for the caller to read: the
 * step records as sgk_step writes them (sgk_step_records_dev), the boards (sgk_boards_dev: of the new episode's first state
 * where the step ended one, as sgk_reset_done leaves them; flags = SGK_F_NO_BOARDS skips them), the episode arrays, the metrics.
 * actions_out_dev: uint8 [n_envs] that receives the chosen actions, or NULL. May be mixed freely with the per-step calls and the
 * rollouts. */
SGK_API int sgk_tabq_step(sgk_tabq *q, int cheat, uint32_t flags, uint8_t *actions_out_dev);
/* n_steps lockstep steps of tabq_learn replayed from ONE hipGraph per (n_steps, cheat, flags): n_steps launches of sgk_tabq_step's
 * kernel (the agent step counter lives in device memory). flags: SGK_F_NO_BOARDS and / or SGK_F_SEPARATE_LAUNCHES -- the latter
 * records the drop-in call sequence {sgk_tabq_act(explore), sgk_step, sgk_tabq_learn, sgk_reset_done} instead, four launches
 * per lockstep step (the form of rounds 2-5; kept for A/B and because it exercises the per-step kernels). Same results either
 * way, and the same as the calls made n_steps times. */
SGK_API int sgk_tabq_learn_steps(sgk_tabq *q, int32_t n_steps, int cheat, uint32_t flags);
/* n_steps of {act_explore, env.step, learn, update_epsilon, reset on done} in one launch
 * (reference learn.py:61-85 inside train.py:62-70) */
SGK_API int sgk_tabq_rollout(sgk_tabq *q, int64_t n_steps, int cheat);
/* the same with the kernel named: AUTO picks by table size and agent count; LDS = the tables of 64 agents resident in a
 * workgroup's LDS for the launch (envs whose state is the agent cell only; SGK_ERR_INVALID otherwise); HBM = rows read and
 * written in HBM (any env). Same arithmetic, same results. */
#define SGK_TABQ_KERNEL_AUTO 0
#define SGK_TABQ_KERNEL_LDS 1
#define SGK_TABQ_KERNEL_HBM 2
SGK_API int sgk_tabq_rollout_ex(sgk_tabq *q, int64_t n_steps, int cheat, int kernel);
/* default_eval (reference common/eval.py:8-56) for every (env, agent) pair in ONE launch, from the envs' current states (a caller
 * that restates eval.py:13 calls sgk_metrics_reset and sgk_reset first): n_reset_steps lockstep steps of {greedy act, env.step,
 * reset of the envs that are over} -- eval.py:19-39 while t < eval_timesteps: TabularQAgent.act is np.argmax of the board's row
 * (value.py:33-35, first maximum wins), a finished episode is booked (eval.py:22) and the env reset (eval.py:23) --, then
 * n_tail_steps of {greedy act, env.step} WITHOUT reset, in which an env whose episode has ended idles as under sgk_step
 * (eval.py:32-33: the loop leaves at the first `done` at or after eval_timesteps; max_iterations steps end every episode).
 * Equal, bit for bit, to that many rounds of {sgk_tabq_act(explore = 0), sgk_step, sgk_reset_done} and {sgk_tabq_act(0), sgk_step}:
 * state words, step records (an idle env's names the action its agent chose), episode arrays, metrics, reset counters, side
 * state, the handle's step accounting; an env that is over on entry idles through the first step and is reset behind it. The
 * boards are materialised once, at the end. The tables, the agent step counter and epsilon are not touched -- except that on a
 * hashed level (tomato watering) act() claims a slot for a board it has not seen, as the reference's defaultdict inserts on a
 * miss (value.py:31,34-35); a full table reads as zeros and raises the overflow flag (sgk_tabq_hash_info).
 * kernel: as for sgk_tabq_rollout_ex -- LDS names the on-chip kernel (each agent's greedy policy folded into a 64-bit register
 * word at entry, no table access per step; envs whose state is the agent cell only, SGK_ERR_INVALID otherwise), HBM the one that
 * gathers a row per state change (any env), AUTO the on-chip kernel wherever it qualifies. Both counts 0: nothing happens.
 * No allocation, no host synchronisation: capturable in a hipGraph. */
SGK_API int sgk_tabq_eval(sgk_tabq *q, int64_t n_reset_steps, int64_t n_tail_steps, int kernel);
/* The tables where they live: [n_states][n_envs][n_actions] float64, STATE-major (ABI 3) -- the row of state s of agent e starts at
 * ((s * n_envs) + e) * n_actions doubles: one lane = one agent, so a wave's 64 rows of a state are 2 KB contiguous (ABI 2 had
 * [n_envs][n_states][n_actions]: 64 separate lines per row access of a wave). sgk_tabq_copy_table hands out the agent-major
 * form. The per-step kernels (sgk_tabq_act / _learn / _learn_steps) keep a per-env copy of ONE table
 * row; this call invalidates those copies once. A caller that KEEPS the pointer (the zero-copy use) and writes the table through
 * it later calls sgk_tabq_invalidate_rows() after every such write, before the next per-step call. */
SGK_API int sgk_tabq_table_dev(sgk_tabq *q, double **table_dev, int64_t *n_states, int64_t *n_actions);
/* The table was written from outside the library (through sgk_tabq_table_dev's pointer): forget the kept rows. Cheap: a flag;
 * the re-tagging launch runs with the next per-step call. */
SGK_API int sgk_tabq_invalidate_rows(sgk_tabq *q);
/* agents env_begin .. env_begin + env_count - 1, agent by agent: table_host[env_count][n_states][n_actions]. Synchronises. */
SGK_API int sgk_tabq_copy_table(sgk_tabq *q, int64_t env_begin, int64_t env_count, double *table_host);
SGK_API int sgk_tabq_global_step(const sgk_tabq *q, int64_t *t_out);
SGK_API double sgk_tabq_epsilon(double epsilon, int64_t epsilon_anneal, int64_t t); /* epsilon in force at global step t */

/* ---- the consensus of the N private agents: a plurality vote per state (csrc/sgk_tabq_consensus.hip) ---------------------------
 * One streaming read of the tables ([n_states][n_envs][4] float64, 32 * n_states * n_envs bytes). The rule, exactly:
 *  - agent e votes in state s iff it may (voters_mask: mask[e] != 0; NULL: every agent) and its row of s has an entry that compares
 *    != 0.0. A row the agent never learnt is all zeros -- the reference's fresh defaultdict row (value.py:31) -- and its argmax of 0
 *    is not an opinion; -0.0 counts as zero;
 *  - a voter's action is the library's own greedy rule, sgk_tabq_act(explore = 0): the first maximum, as np.argmax picks.
 * The counts are integers: the result depends neither on the grid's shape nor on the order of the atomics. The outputs are
 * OVERWRITTEN (the caller need not zero them). No allocation, no host synchronisation, enqueued on the handle's stream: capturable in
 * a hipGraph. Levels with hashed tables (SGK_TOMATO_WATERING) are refused with SGK_ERR_INVALID: an agent's slots are its own, so the
 * agents' rows do not line up by state. A NULL handle and NULL outputs are SGK_ERR_INVALID. The tables, the agent step counter and
 * epsilon are only read; like sgk_tabq_table_dev, the call makes the per-step kernels re-read the one row per env they keep (the
 * table is written through, so they read the same values again).
 * votes_out_dev  int64 [n_states][4]  votes_out[s][a] = number of voting agents whose greedy action in state s is a
 * voters_out_dev int64 [n_states]     number of voting agents in state s (= sum over a of votes_out[s][a]); may be NULL
 * voters_mask_dev uint8 [n_envs] or NULL: agent e may vote iff mask[e] != 0 (NULL: every agent) */
SGK_API int sgk_tabq_consensus(sgk_tabq *q, const uint8_t *voters_mask_dev, int64_t *votes_out_dev, int64_t *voters_out_dev);
/* every agent's table := table_dev (float64 [n_states][4], device); the kept per-env rows are invalidated (as by
 * sgk_tabq_invalidate_rows: a host-side flag raised when the call is MADE -- behind a replay of a recorded call, the caller raises it).
 * One streaming write of the same bytes; no allocation, no host synchronisation, the handle's stream. The agent step counter and
 * epsilon stay. Hashed levels, a NULL handle and a NULL table are SGK_ERR_INVALID. */
SGK_API int sgk_tabq_load_shared(sgk_tabq *q, const double *table_dev);
/* the vote on host arrays: table_host [n_agents][n_states][4] as sgk_tabq_copy_table hands it out; no GPU, no handle. The same rule
 * (the same code) as sgk_tabq_consensus. A NULL table or votes_out and a negative count are SGK_ERR_INVALID; voters_out_host and the
 * mask may be NULL. */
SGK_API int sgk_tabq_consensus_host(const double *table_host, int64_t n_agents, int64_t n_states, const uint8_t *voters_mask_host,
                                    int64_t *votes_out_host, int64_t *voters_out_host);

/* ---- the same vote on the HASHED levels (SGK_TOMATO_WATERING), by board key (csrc/sgk_tabq_hash_consensus.hip) --------------------
 * An agent's slots are its own, so the rows do not line up by slot -- they line up by KEY: a slot's key names its board
 * (sgk_tabq_copy_keys), and every key is below 1 << SGK_TABQ_HASH_KEY_BITS. The rule, exactly:
 *  - agent e votes on key k iff it may (voters_mask: mask[e] != 0; NULL: every agent), one of its slots holds k, and that slot's row
 *    has an entry that compares != 0.0; -0.0 counts as zero. A claimed slot whose row is all zeros is a defaultdict row never learnt:
 *    no opinion. A key nobody votes on is ABSENT from the output;
 *  - a voter's action is the same rule (the same code) as sgk_tabq_consensus: the first maximum, as np.argmax picks;
 *  - the output is the U voted keys in ASCENDING order with their counts. Every element of keys, votes, voters and count is
 *    OVERWRITTEN: behind the last key, keys is 0xffffffff and the counts are 0. When U > max_keys the first max_keys keys in ascending
 *    order are written with their full counts, and *count still says U;
 *  - a key >= 1 << SGK_TABQ_HASH_KEY_BITS other than the empty marker cannot occur; it is skipped, and nothing indexes past the bitmap.
 * The counts are integers: the result depends neither on the grid's shape nor on the order of the atomics. No allocation, no host
 * synchronisation, enqueued on the handle's stream: capturable in a hipGraph. The agents are only READ: tables, keys, tags, the step
 * counter, epsilon and the overflow flag stay as they are, and no kept row is invalidated. SGK_ERR_INVALID with a message and nothing
 * launched: a NULL handle, descriptor, keys, votes, count or workspace, max_keys < 1, a workspace below
 * sgk_tabq_hash_consensus_workspace_bytes(q), a misaligned pointer (keys 4, votes / voters / count 8, workspace 16 bytes), a
 * perfect-hash level (sgk_tabq_consensus is the call for it).
 * Every output and the workspace travel in ONE descriptor passed by const pointer, as sgk_members_act_out does and for its reason:
 * tests/test_guard_arena_cpu.py lists every non-const pointer parameter; tests/test_hash_consensus_cpu.py holds the table that names
 * a guard-band case of tests/test_gpu_hash_consensus.py for every field. */
#define SGK_TABQ_HASH_KEY_BITS 22 /* every key of a hashed level is < 1 << 22; 0xffffffff = empty */
typedef struct sgk_tabq_hash_votes {
  uint32_t *keys;          /* [max_keys]    the voted keys, ASCENDING; 0xffffffff behind the last */
  int64_t *votes;          /* [max_keys][4] votes[j][a] = voting agents whose greedy action on board keys[j] is a; 0 behind the last */
  int64_t *voters;         /* [max_keys] or NULL: the row sums */
  int64_t *count;          /* [1] the number U of distinct voted keys -- the TRUE number, also when U > max_keys */
  int64_t max_keys;        /* >= 1 */
  void *workspace;         /* >= sgk_tabq_hash_consensus_workspace_bytes(q), 16-byte aligned; contents need not be kept */
  int64_t workspace_bytes;
} sgk_tabq_hash_votes;
/* 768 KiB (the bitmap and its prefix) + 8 bytes per slot + 1 byte per slot and agent at the handle's CURRENT capacity (ask again
 * after sgk_tabq_hash_grow). < 0: an error code (a NULL handle, a perfect-hash level). */
SGK_API int64_t sgk_tabq_hash_consensus_workspace_bytes(sgk_tabq *q);
SGK_API int sgk_tabq_hash_consensus(sgk_tabq *q, const uint8_t *voters_mask_dev, const sgk_tabq_hash_votes *out);
/* The mirror: for every agent with agents_mask[e] != 0 (NULL: all) the table becomes EXACTLY the table that results from a sequential
 * insertion: start from an empty table of the agent's current capacity, insert keys_dev[0 .. min(*count_dev, max_keys)) in the given
 * order through the library's one probe loop, and give each key the row rows_dev[j] (float64 [max_keys][4]). So: every other slot is
 * empty with a zero row; a later duplicate key overwrites the earlier row; the empty marker in the list is skipped; a key that finds
 * the table full raises the sticky overflow flag (sgk_tabq_hash_info) as everywhere else and is dropped. The agent's tag becomes "no
 * pending act, no kept row": an sgk_tabq_learn behind a load without a new sgk_tabq_act learns nothing, as for an env that was over.
 * Agents not selected keep every byte. count_dev is read ON THE DEVICE, so vote, conversion and load chain without a host round
 * trip. The table is built once (one workgroup) and broadcast as a streaming write. No allocation, no host synchronisation, the
 * handle's stream: capturable; as after sgk_tabq_hash_grow the pointers do not move, so the sgk_tabq_learn_steps graphs stay valid.
 * The insertion is a serial chain in one workgroup (the key row in LDS up to 32 768 slots, in the workspace above): its cost grows with
 * the list, and a key that finds the table FULL costs a probe of every slot before it is dropped -- load into tables that hold the
 * list (BatchedTabularQAgent.hash_consensus_agent sizes them), not a list several times the capacity.
 * scratch: only workspace and workspace_bytes are read (the same size as for the vote; a vote's descriptor may be passed again once
 * its outputs have been converted). Refusals as for the vote, plus NULL keys_dev / rows_dev / count_dev and max_keys outside
 * 1 .. 2^31 - 1. */
SGK_API int sgk_tabq_hash_load_shared(sgk_tabq *q, const uint8_t *agents_mask_dev, const uint32_t *keys_dev, const double *rows_dev,
                                      const int64_t *count_dev, int64_t max_keys, const sgk_tabq_hash_votes *scratch);
/* the vote on host arrays as sgk_tabq_copy_keys / sgk_tabq_copy_table hand them out: keys_host [n_agents][capacity], rows_host
 * [n_agents][capacity][4]; no GPU, no handle, the same rule (the same code); out's workspace is not used. */
SGK_API int sgk_tabq_hash_consensus_host(const uint32_t *keys_host, const double *rows_host, int64_t n_agents, int32_t capacity,
                                         const uint8_t *voters_mask_host, const sgk_tabq_hash_votes *out);
/* the load's table on the host: ONE agent's table of `capacity` slots (a power of two in 64 .. 2^24) behind the sequential insertion
 * of keys_in[0 .. count) with rows_in [count][4] -- what sgk_tabq_hash_load_shared leaves in every selected agent. */
typedef struct sgk_tabq_hash_table {
  uint32_t *keys;      /* [capacity]    0xffffffff = empty */
  double *rows;        /* [capacity][4] zero where the slot is empty */
  int32_t *overflowed; /* [1] or NULL: 1 iff a key found the table full (and was dropped) */
} sgk_tabq_hash_table;
SGK_API int sgk_tabq_hash_load_shared_host(const uint32_t *keys_in, const double *rows_in, int64_t count, int32_t capacity,
                                           const sgk_tabq_hash_table *out);

/* ---- DeepQAgent.act_explore, batched (reference value.py:94-111) ------------------------------------------------------ */
/* scores_dev: float32 [n_envs][4] (16-byte aligned) from the Q-network; actions_out_dev: uint8 [n_envs]. Draws from
 * Categorical(eps/4 + (1 - eps) on the argmax) with the counter RNG (Philox stream 2, keyed by global env index and
 * draw_index -- pass the agent's step counter). epsilon = 0 is DeepQAgent.act (value.py:89-92).
 * The counter is ctr = {env_lo, env_hi, (uint32_t)draw_index, stream}: only the low 32 bits of draw_index enter it, so the draws of an
 * env are PERIODIC in draw_index with period 2^32 (draw 2^32 + 5 is draw 5). The same holds for every entry point that takes a
 * draw_index or draw_index0: sgk_epsilon_greedy_ex, sgk_policy_act, sgk_convq_act (stream 2), sgk_categorical_sample,
 * sgk_policy_sample, sgk_convq_sample (stream 3), and step k of sgk_policy_rollout / sgk_convq_rollout and their _members forms, which
 * draws with index draw_index0 + k (a 64-bit sum: a rollout that starts below 2^32 runs across the edge into draw 0, 1, ...). */
SGK_API int sgk_epsilon_greedy(sgk_env *h, const float *scores_dev, double epsilon, uint64_t draw_index,
                               uint8_t *actions_out_dev);
/* same, with epsilon and/or the draw index read from device memory when the pointers are non-NULL (so that the launch can be
 * recorded once in a caller's hipGraph and replayed while the schedule advances) */
SGK_API int sgk_epsilon_greedy_ex(sgk_env *h, const float *scores_dev, double epsilon, uint64_t draw_index,
                                  const double *epsilon_dev, const uint64_t *draw_index_dev, uint8_t *actions_out_dev);

/* ---- DeepQAgent: Q-network forward + act_explore in one launch (reference value.py:89-111,148-158) ------------------- */
/* The reference's default topology (n_layers = 2): Linear(n_cells, H) + ReLU, Linear(H, H) + ReLU, Linear(H, 4); H = 100
 * (the reference default, agent_parser_configs.yaml:45-49), 64 or 128.
 * Device pointers into the (PyTorch) parameters, float32: w1t = W1 transposed [n_cells][H]; b1 [H]; w2 = W2 [H][H] as torch
 * stores it ([out][in]); b2 [H]; w3t = W3 transposed [H][4]; b3 [4]. Reads the env's int8 boards directly. */
typedef struct sgk_mlp_weights {
  const float *w1t, *b1, *w2, *b2, *w3t, *b3;
  int32_t n_hidden;
} sgk_mlp_weights;
/* actions_out_dev: uint8 [n_envs]; scores_out_dev: float32 [n_envs][4] or NULL. epsilon / draw_index as in
 * sgk_epsilon_greedy_ex (device pointers override the scalars when non-NULL). fp32 accumulation order differs from a BLAS
 * GEMM: scores agree with the torch forward to fp32 tolerance, not bit for bit. */
SGK_API int sgk_policy_act(sgk_env *h, const sgk_mlp_weights *w, double epsilon, uint64_t draw_index,
                           const double *epsilon_dev, const uint64_t *draw_index_dev, uint8_t *actions_out_dev,
                           float *scores_out_dev);

/* ---- the reference's convolutional body (PPOCNNAgent, policy_cnn.py:17-81) with a four-way head, forward + draw in one launch ------ */
/*     trunk = relu(conv3x3(relu(conv3x3(x, 1 -> C)), C -> C)) + conv1x1(x, 1 -> C)                    policy_cnn.py:19-44, 70
 *     out   = linear(flatten(relu(conv3x3(trunk, C -> C))), C * n_cells -> 4)                         policy_cnn.py:46-55, 72-74
 * on every env's board -- im2col GEMMs on fp32 MFMA over zero-bordered activation planes in LDS -- and then one of two draws:
 *   sgk_convq_sample: PPOBaseAgent.act_explore (policy_base.py:54-64) of a PPOCNNAgent -- `out` are the ACTOR's logits (wh / bh =
 *     actor_cnn, wl / bl = actor_linear; the critic head is not needed to act) and the action is Categorical(logits).sample(),
 *     sgk_categorical_sample's draw (Philox stream 3). This is the reference's ppo-cnn gather_rollout step (policy_base.py:145).
 *   sgk_convq_act: DeepQAgent.act_explore's epsilon-greedy draw (sgk_epsilon_greedy's: Philox stream 2) on `out` as four Q-values. The
 *     reference's DeepQAgent is an MLP (value.py:148-158): a Q-network of this shape is the batched agent's labelled NON-PARITY
 *     option (BASELINE.json words config 4 as "conv policy"). epsilon / draw_index as in sgk_epsilon_greedy_ex.
 * Weights in torch's layouts, float32, device: w1 [C][1][3][3], w2 / wh [C][C][3][3], wb [C][1][1][1], wl [4][C * n_cells]; biases
 * b1 b2 bb bh [C], bl [4]. n_channels in {4, 5 (the reference's default, agent_parser_configs.yaml:107-111), 8}, n_layers == 2 (the
 * reference's default: two 3 x 3 convolutions in the trunk). scores_out_dev / logits_out_dev: float32 [n_envs][4], 16-byte aligned, or
 * NULL. The outputs agree with the torch module to fp32 tolerance (another summation order than MIOpen / rocBLAS). */
typedef struct sgk_convq_weights {
  const float *w1, *b1, *w2, *b2, *wb, *bb, *wh, *bh, *wl, *bl;
  int32_t n_channels, n_layers;
} sgk_convq_weights;
SGK_API int sgk_convq_act(sgk_env *h, const sgk_convq_weights *w, double epsilon, uint64_t draw_index, const double *epsilon_dev,
                          const uint64_t *draw_index_dev, uint8_t *actions_out_dev, float *scores_out_dev);
SGK_API int sgk_convq_sample(sgk_env *h, const sgk_convq_weights *w, uint64_t draw_index, const uint64_t *draw_index_dev,
                             uint8_t *actions_out_dev, float *logits_out_dev);
/* n_steps of {that forward, the draw, env.step} in ONE launch: the inner loop of PPOBaseAgent.gather_rollout (policy_base.py:142-163:
 * old_policy.act_explore -> env.step -> store state / action / reward) for a PPOCNNAgent -- what sgk_policy_rollout is for the MLP
 * bodies, and with its arguments: mode 0 = epsilon-greedy with a fixed epsilon (acting with a frozen conv Q-network), 1 = Categorical
 * sample; step k draws with index draw_index0 + k; flags: SGK_F_AUTO_RESET, SGK_F_MASK_FINISHED (the states / actions entries of an env
 * whose episode is over are zeros; it idles when auto-reset is off). Optional outputs: states_out_dev int8 [n_steps][n_envs][n_cells]
 * (the board each action was chosen on), actions_out_dev uint8 [n_steps][n_envs], recs_out_dev [n_steps][n_envs]. The envs' own
 * boards are materialised at the end. */
SGK_API int sgk_convq_rollout(sgk_env *h, const sgk_convq_weights *w, int32_t mode, double epsilon, uint64_t draw_index0, int32_t n_steps,
                              uint32_t flags, int8_t *states_out_dev, uint8_t *actions_out_dev, sgk_step_rec *recs_out_dev);
/* The same launch for n_members INDEPENDENT conv bodies: gather_rollout's inner loop of n_members PPOCNNAgents at once, as
 * sgk_policy_rollout_members is for the MLP bodies. Member m acts in the envs m * E .. (m + 1) * E - 1, E = n_envs / n_members, with the
 * m-th slice of each of the ten weight tensors stacked on a leading member axis (w1 [n_members][C][1][3][3], ..., wl [n_members][4][C *
 * n_cells], bl [n_members][4]); `w`'s pointers address member 0. A workgroup serves ONE member for the whole launch and a pass of envs
 * never straddles two members; any number of members works (the grid is n_members x a member's workgroups). Env indices -- RNG keys
 * (global env index), trajectory outputs [n_steps][n_envs][...], episode arrays -- are the handle's own, so member m's outputs are
 * those of a handle of E envs created at env_index_base + m * E running sgk_convq_rollout with member m's weights, bit for bit.
 * member_metrics_dev: int64 [n_members][SGK_METRICS_LEN] or NULL, the contract of sgk_policy_rollout_members (sums added, maxima
 * raised: initialise the maxima to INT64_MIN). The member instantiation of the kernel is used for every n_members, 1 included (where
 * it leaves the bytes sgk_convq_rollout leaves). SGK_ERR_INVALID for n_members < 1, n_envs % n_members != 0 and whatever
 * sgk_convq_rollout refuses. */
SGK_API int sgk_convq_rollout_members(sgk_env *h, const sgk_convq_weights *w, int32_t n_members, int32_t mode, double epsilon,
                                      uint64_t draw_index0, int32_t n_steps, uint32_t flags, int8_t *states_out_dev,
                                      uint8_t *actions_out_dev, sgk_step_rec *recs_out_dev, int64_t *member_metrics_dev);

/* ---- the same body on the observation of a transition env: two input channels, [previous board, board] ------------------------------
 * The reference's TransitionBoatRace observes [last board, board], and [board, board] at a reset; its PPOCRMDPAgent / PPOCNNAgent is
 * then built with two input channels. These three calls are sgk_convq_act / _sample / _rollout for that body:
 *   `w` is sgk_convq_weights with w1 [C][2][3][3] and wb [C][2][1][1] (torch's layouts: channel 0 = the previous board, 1 = the current
 *   one); every other tensor, n_channels and n_layers as above. The struct's layout is unchanged: the caller vouches for the two sizes.
 *   `tr` carries EVERYTHING writable -- the previous boards and all outputs -- so that no entry point here has a non-const pointer
 *   parameter (tests/test_guard_arena_cpu.py lists those of the whole header):
 *     prev_boards_dev       int8 [n_envs][n_cells], dense. act / sample: read only, or NULL = every env's previous board is its current
 *                           one. rollout: required; read at entry unless fresh != 0, WRITTEN at exit with the previous-board channel of
 *                           the observation the NEXT action would be chosen on (the board before the last step; the current board for
 *                           an env the last step reset), so that the next call -- of any of the three -- continues the trajectory.
 *     prev_states_out_dev   rollout only: int8 [n_steps][n_envs][n_cells] or NULL -- channel 0 of the observation each action was chosen
 *                           on, beside states_out_dev's channel 1; zeros where states_out_dev holds zeros (SGK_F_MASK_FINISHED).
 *     fresh                 rollout only: != 0 -- no env has stepped since its reset: previous := current at entry.
 *     actions_out_dev       act / sample: uint8 [n_envs], required. rollout: uint8 [n_steps][n_envs] or NULL.
 *     scores_out_dev        act / sample only: float32 [n_envs][4] (the scores / logits), 16-byte aligned, or NULL.
 *     states_out_dev, recs_out_dev   rollout only: sgk_convq_rollout's optional outputs.
 *   An env that SGK_F_AUTO_RESET resets inside the rollout acts next on [board, board]. An env that idles (its episode is over, no
 *   auto-reset) still moves on: its previous board becomes its current one.
 * Draws, RNG keys, flags, metrics, optional outputs and the boards materialised at the end are those of the one-channel calls; like
 * them these allocate nothing, never synchronise the host and can be captured in a graph. Kernels exist for the 5 x 5 board (BoatRace)
 * and n_channels in {4, 5, 8}; there is no member form. SGK_ERR_INVALID with a message and nothing launched for a NULL `tr`, a NULL
 * prev_boards_dev in the rollout, another board shape, and whatever the one-channel call refuses.
 * Guard bands: tests/test_gpu_transition_body.py carves every pointer field of `tr` from tests/guard_arena.py's arena;
 * tests/test_transition_cpu.py requires every pointer field of the struct to name one such test. */
typedef struct sgk_convq_transition {
  int8_t *prev_boards_dev;
  int8_t *prev_states_out_dev;
  int32_t fresh;
  int8_t *states_out_dev;
  uint8_t *actions_out_dev;
  sgk_step_rec *recs_out_dev;
  float *scores_out_dev;
} sgk_convq_transition;
SGK_API int sgk_convq_act_trans(sgk_env *h, const sgk_convq_weights *w, const sgk_convq_transition *tr, double epsilon, uint64_t draw_index,
                                const double *epsilon_dev, const uint64_t *draw_index_dev);
SGK_API int sgk_convq_sample_trans(sgk_env *h, const sgk_convq_weights *w, const sgk_convq_transition *tr, uint64_t draw_index,
                                   const uint64_t *draw_index_dev);
SGK_API int sgk_convq_rollout_trans(sgk_env *h, const sgk_convq_weights *w, const sgk_convq_transition *tr, int32_t mode, double epsilon,
                                    uint64_t draw_index0, int32_t n_steps, uint32_t flags);

/* The two halves of the replay add FUSED into the launches around them (round 6; a lockstep step of dqn_learn -- learn.py:29-58 -- is
 * then sgk_policy_act, sgk_step_store, sgk_dqn_sgd_step, sgk_reset_done_store: four calls instead of six -- or three, with the last two
 * as sgk_dqn_sgd_step_reset_store):
 *   sgk_step_store        env.step(actions) for every env (learn.py:38; no auto-reset) AND ReplayBuffer.add's second half (contain.py:15-17
 *                         via value.py:114): the successor boards, the action, the reward (cheat != 0: the hidden reward and the executed
 *                         action, learn.py:41-47) and the terminal flag go into slice `slice` of the rings, next to the step's usual
 *                         outputs. = sgk_step + sgk_replay_store(phase 1).
 *   sgk_reset_done_store  env.reset() of the envs whose episode is over (train.py:62-64) AND the add's first half for the NEXT step:
 *                         every env's board -- what its next action is chosen on -- goes into slice `slice` of the states ring.
 *                         = sgk_reset_done + sgk_replay_store(phase 0).
 * slice_dev non-NULL (graph replays): the slice is (*slice_dev + slice) % ring_slices, read by the launch. Rings as for
 * sgk_replay_store: boards int8 [slices][n_envs][n_cells], the others [slices][n_envs]. flags: SGK_F_NO_BOARDS or 0 (the env's own
 * board buffer; the rings always receive theirs). */
SGK_API int sgk_step_store(sgk_env *h, const uint8_t *actions_dev, uint32_t flags, int32_t cheat, int64_t slice, const int64_t *slice_dev,
                           int32_t ring_slices, int8_t *successors_ring, uint8_t *actions_ring, int8_t *rewards_ring,
                           uint8_t *terminals_ring);
SGK_API int sgk_reset_done_store(sgk_env *h, uint32_t flags, int64_t slice, const int64_t *slice_dev, int32_t ring_slices,
                                 int8_t *states_ring);

/* ---- DeepQAgent.learn (reference value.py:113-136) for the default topology as ONE kernel --------------------------- */
/* What the kernel does, by reference line: ReplayBuffer.sample (contain.py:19-22, called at value.py:116) -- uniform with
 * replacement from a device replay ring, counter RNG stream 4 keyed by the Adam step; Q(states).gather(actions) (value.py:119);
 * target_Q(successors).max(1) with the terminal rows zeroed (value.py:120-121); expected = discount * next_Q + reward
 * (value.py:122); F.mse_loss (value.py:123); backward + clip_grad_norm_(max_grad_norm) (value.py:127-128); Adam(amsgrad)
 * (value.py:87,134) -- for the Linear(n_cells, H)-ReLU-Linear(H, H)-ReLU-Linear(H, 4) network of value.py:148-158 with H = 100
 * (the reference default) or 64, batch <= 64. replay.add (value.py:114) is sgk_replay_store; the TensorBoard scalar
 * (value.py:124) is the caller's, from loss_out.
 * loss_mode selects what F.mse_loss sees:
 *   SGK_DQN_LOSS_REFERENCE (0)  value.py:119-123 AS WRITTEN: Qs is [B,1], expected_Qs is [B], mse_loss broadcasts the pair to
 *                               [B,B]: loss = mean over (i, j) of (Q_i - e_j)^2, so dL/dQ_i = (2/B) (Q_i - mean_j e_j) --
 *                               every sample regresses towards the minibatch's mean target. Pinned to reference output
 *                               (tests/golden/deepq_learn.npz, batched_dqn_*.npz).
 *   SGK_DQN_LOSS_PER_SAMPLE (1) NOT the reference: the squeezed form, loss = mean_i (Q_i - e_i)^2 (textbook DQN).
 * All pointers are device pointers; float32.
 *   replay ring   states / successors int8 [slices][n_envs][n_cells], actions uint8, rewards int8, terminals uint8 (0/1),
 *                 each [slices][n_envs]; the first slices_filled slices hold data
 *   w1..b3        the Q-network's parameters in torch layout ([out][in]), UPDATED IN PLACE
 *   w1t, w2t, w3t transposed copies ([in][out]) the kernel reads and keeps current (w1t / w3t are what sgk_policy_* take)
 *   m, v, vmax    Adam's exp_avg, exp_avg_sq, max_exp_avg_sq for w1, b1, w2, b2, w3, b3 (same shapes), updated
 *   tw1t, tw2t    the target network's hidden weights transposed; tb1, tb2, tw3 ([4][H]), tb3 as they are
 *   step          Adam's step counter (int64, device), incremented;   loss_out: float, or NULL
 *   rows          NULL (the kernel draws the minibatch, stream 4), or int64 [batch]: the caller's transition indices
 *                 slice * n_envs + env (an external sampler; an index outside the stored transitions reads transition 0)
 *   rows_out      NULL, or int64 [batch]: receives the indices this step trained on
 * Two launches on the handle's stream: everything up to the clipped-gradient's norm in one 1 024-lane workgroup, then Adam(amsgrad) and
 * the transposed copies with one lane per parameter over the whole chip (the gradient crosses in a scratch block of the handle's, made
 * on the handle's FIRST call: call once before recording the step in a hipGraph). Adam's square root and quotient use the hardware's
 * one-ulp v_sqrt_f32 / v_rcp_f32.
 * fp32 with a different summation order than rocBLAS: equal to torch's step to fp32 tolerance, not bit for bit. */
#define SGK_DQN_LOSS_REFERENCE 0
#define SGK_DQN_LOSS_PER_SAMPLE 1
typedef struct sgk_dqn_learner {
  const int8_t *states, *successors;
  const uint8_t *actions;
  const int8_t *rewards;
  const uint8_t *terminals;
  int32_t slices_filled, n_hidden, batch, loss_mode; /* slices_filled * n_envs < 2^31 (32-bit transition indices); SGK_DQN_LOSS_* */
  float *w1, *b1, *w2, *b2, *w3, *b3, *w1t, *w2t, *w3t;
  float *m[6], *v[6], *vmax[6];
  const float *tw1t, *tb1, *tw2t, *tb2, *tw3, *tb3;
  int64_t *step;
  float *loss_out;
  double lr, beta1, beta2, eps, discount, max_grad_norm;
  const int64_t *rows; /* or NULL */
  int64_t *rows_out;   /* or NULL */
} sgk_dqn_learner;
SGK_API int sgk_dqn_sgd_step(sgk_env *h, const sgk_dqn_learner *learner);
/* The same SGD step AND the lockstep step's last launch -- sgk_reset_done_store(flags, slice, slice_dev, ring_slices, states_ring): the
 * reset of the finished envs (train.py:70) + the next transitions' states into the replay ring -- behind it in TWO launches instead of
 * three: the Adam launch (one lane per parameter, a fraction of the chip) carries the reset as extra workgroups of its grid. The reset
 * neither reads the weights nor the minibatch, and the SGD kernel before it has finished sampling the ring: results identical to
 * sgk_dqn_sgd_step followed by sgk_reset_done_store. */
SGK_API int sgk_dqn_sgd_step_reset_store(sgk_env *h, const sgk_dqn_learner *learner, uint32_t flags, int64_t slice, const int64_t *slice_dev,
                                         int32_t ring_slices, int8_t *states_ring);
/* DeepQAgent.learn (reference value.py:113-136) for n_members INDEPENDENT DeepQAgents in one call: the same two launches as
 * sgk_dqn_sgd_step with a member axis -- the SGD kernel's grid is one 1 024-lane workgroup per member, the Adam launch's
 * n_members x ceil(P / 256) workgroups (workgroup -> (member, block)). Member m is the reference's `deep-q` run on the env columns
 * m * E .. (m + 1) * E - 1, E = n_envs / n_members.
 *   stacked tensors  every tensor of `learner` but the replay ring exists once per member, stacked on a leading member axis in one
 *                    contiguous tensor, and the learner's pointers address member 0: w1 [n_members][H][n_cells], b1 [n_members][H],
 *                    w2 [n_members][H][H], b2 [n_members][H], w3 [n_members][4][H], b3 [n_members][4]; w1t [n_members][n_cells][H],
 *                    w2t [n_members][H][H], w3t [n_members][H][4]; m[i] / v[i] / vmax[i] like their parameter; the target's tw1t
 *                    [n_members][n_cells][H], tb1, tw2t [n_members][H][H], tb2, tw3 [n_members][4][H], tb3 [n_members][4]; step int64
 *                    [n_members]; loss_out float [n_members] or NULL; rows / rows_out int64 [n_members][batch] or NULL.
 *   shared           the replay ring ([slices][n_envs][...], all members' env columns side by side, as sgk_step_store fills it) and
 *                    the learner's hyper-parameters (lr and discount per member: sgk_dqn_sgd_step_members_hyper).
 *   rows             transitions keep their GLOBAL index slice * n_envs + env. Member m draws d uniformly from [0, slices_filled * E)
 *                    with sgk_dqn_sgd_step's Philox call (stream 4, counter (sample, 0, its own Adam step, 4)) keyed by
 *                    member_keys_dev[m] (uint64 [n_members], device; NULL: the handle's seed for every member) and trains on the
 *                    transition (d / E) * n_envs + m * E + d % E; rows_out receives these global indices. A handle of E envs created at
 *                    env_index_base + m * E draws the same transitions of its own ring with sgk_dqn_sgd_step.
 *   a caller's row   that is outside the stored transitions, or whose env is not one of member m's own, trains on the member's first
 *                    transition (slice 0, env m * E) -- not on wild memory, and not on another member's data.
 *   workspace        device memory of sgk_dqn_members_workspace_bytes(h, n_hidden, n_members) bytes, 16-byte aligned, the CALLER's:
 *                    member m's clip coefficient and flat gradient cross from the first launch to the second in its m-th slice. Its
 *                    contents mean nothing between calls. No allocation, no host synchronisation, nothing of the handle's scratch block:
 *                    the call can be recorded in a graph as the first call on a handle.
 * n_members = 1 with member_keys_dev NULL IS sgk_dqn_sgd_step (the same kernels, the same bits). SGK_ERR_INVALID for n_members < 1,
 * n_envs % n_members != 0, a NULL workspace, slices_filled * E >= 2^31 and whatever sgk_dqn_sgd_step refuses. A workgroup of the SGD
 * kernel fills a CU's LDS: the members run one per CU, and in waves above one member per CU.
 * sgk_dqn_members_workspace_bytes: -1 (and sgk_last_error) for a shape without a kernel. */
SGK_API int64_t sgk_dqn_members_workspace_bytes(sgk_env *h, int32_t n_hidden, int32_t n_members);
/* One member's hyper-parameters for sgk_dqn_sgd_step_members_hyper, as they lie in device memory. */
typedef struct sgk_dqn_member_hyper {
  double lr, discount;
} sgk_dqn_member_hyper;
/* sgk_dqn_sgd_step_members with ONE lr AND ONE discount PER MEMBER: hyper_dev is sgk_dqn_member_hyper [n_members] in device memory;
 * workgroup m of the SGD kernel loads its element once at entry and converts each field with the (float) cast the host applies to
 * learner->lr / learner->discount, then uses the results where the shared call uses those (Adam's step size, the target
 * r + discount * max Q'). learner->lr and learner->discount are ignored; beta1, beta2, eps, max_grad_norm stay the learner's. With
 * every element {learner->lr, learner->discount} the call leaves the bytes sgk_dqn_sgd_step_members leaves. The values are read when
 * the kernel runs: a recorded call follows what is copied into the array between replays. The member instantiation of the kernels
 * is used for every n_members, 1 included. SGK_ERR_INVALID for hyper_dev == NULL and whatever sgk_dqn_sgd_step_members refuses, for
 * the same reason. The contents are not validated (the caller keeps them finite, lr > 0, 0 < discount <= 1). No allocation, no host
 * synchronisation. */
SGK_API int sgk_dqn_sgd_step_members_hyper(sgk_env *h, const sgk_dqn_learner *learner, int32_t n_members, const uint64_t *member_keys_dev,
                                           void *workspace, const sgk_dqn_member_hyper *hyper_dev);
SGK_API int sgk_dqn_sgd_step_members(sgk_env *h, const sgk_dqn_learner *learner, int32_t n_members, const uint64_t *member_keys_dev,
                                     void *workspace);

/* ---- PPOBaseAgent.learn (reference policy_base.py:64-131) for PPOMLPAgent's default topology as ONE kernel ---------- */
/* All `n_epochs` minibatch updates of one learn() call: per epoch `batch` rows drawn uniformly with replacement from the
 * (step, trajectory) pairs inside an episode (policy_base.py:77-80; counter RNG stream 5 keyed by the Adam step, or the
 * caller's `rows`), current and old policy forward, advantages r - V(s) normalised over the minibatch, clipped surrogate
 * + critic_coeff * mse_loss - entropy_bonus * entropy (policy_base.py:82-106; the advantage is NOT detached there, so the
 * policy loss also back-propagates into the critic -- reproduced), backward, Adam (torch defaults) -- the
 * Linear(n_cells, H)-ReLU-Linear(H, H)-ReLU trunk with Linear(H, 4) actor and Linear(H, 1) critic of policy_mlp.py:14-33,
 * H = 100 (the reference default) or 64, 2 <= batch <= 64. All pointers are device pointers; float32.
 *   rollout     states int8 [horizon][n_trajectories][n_cells], actions uint8 [horizon][n_trajectories],
 *               returns float [n_trajectories][horizon], lengths int32 [n_trajectories] (sgk_policy_rollout's outputs)
 *   w1..bc      the current network in torch layout ([out][in]), UPDATED IN PLACE;  w1t, w2t: transposed trunk copies the
 *               kernel reads and keeps current
 *   m, v        Adam's exp_avg / exp_avg_sq for w1, b1, w2, b2, wa, ba, wc, bc
 *   ow1t, ow2t  the old policy's trunk weights transposed; ob1, ob2, owa ([4][H]), oba as they are (read only)
 *   step        Adam's step counter (int64, device), advanced by n_epochs
 *   stats_out   float [n_epochs][3]: policy loss, value loss, entropy of each epoch before its update; or NULL
 *   rows        int64 [n_epochs][batch] rows step * n_trajectories + trajectory replacing the draws; or NULL
 *   rows_out    int64 [n_epochs][batch] receives the rows each epoch used; or NULL
 * fp32 with a different summation order than rocBLAS: equal to torch's updates to fp32 tolerance, not bit for bit. */
typedef struct sgk_ppo_learner {
  const int8_t *states;
  const uint8_t *actions;
  const float *returns;
  const int32_t *lengths;
  int32_t horizon, n_hidden, batch, n_epochs;
  int64_t n_trajectories;
  float *w1, *b1, *w2, *b2, *wa, *ba, *wc, *bc, *w1t, *w2t;
  float *m[8], *v[8];
  const float *ow1t, *ob1, *ow2t, *ob2, *owa, *oba;
  int64_t *step;
  float *stats_out;
  const int64_t *rows;
  int64_t *rows_out;
  double lr, beta1, beta2, eps, clipping, critic_coeff, entropy_bonus;
} sgk_ppo_learner;
SGK_API int sgk_ppo_epochs(sgk_env *h, const sgk_ppo_learner *learner);
/* PPOBaseAgent.learn (reference policy_base.py:64-131) for n_members INDEPENDENT PPOMLPAgents in ONE launch, one workgroup per member:
 * member m is the reference's run on the trajectories m * E .. (m + 1) * E - 1, E = n_trajectories / n_members (its `-r E`). Every
 * tensor of `learner` but the rollout exists once per member, stacked on a leading member axis in one contiguous tensor, and the
 * learner's pointers address member 0: w1 [n_members][H][n_cells], ..., m[i] / v[i] like their parameter, the old policy's tensors,
 * step int64 [n_members], stats_out float [n_members][n_epochs][3], rows / rows_out int64 [n_members][n_epochs][batch]. The rollout is
 * shared: n_trajectories = all members' trajectories (sgk_policy_rollout_members' outputs), rows are global (step * n_trajectories +
 * trajectory) and member m draws its own from its own trajectories -- the trajectory from [0, E) by sgk_ppo_epochs' Philox call, then
 * offset by m * E -- keyed by member_keys_dev[m] (uint64 [n_members], device) and its own Adam step; member_keys_dev NULL: the handle's
 * seed for every member. All hyper-parameters are the learner's (one set per member: sgk_ppo_epochs_members_hyper). n_members = 1 with member_keys_dev NULL IS sgk_ppo_epochs (the same kernel).
 * SGK_ERR_INVALID for n_members < 1, n_trajectories % n_members != 0 and whatever sgk_ppo_epochs refuses. No allocation, no host
 * synchronisation: can be recorded in a graph. A workgroup fills a CU's LDS: up to one member per CU runs at a time. */
SGK_API int sgk_ppo_epochs_members(sgk_env *h, const sgk_ppo_learner *learner, int32_t n_members, const uint64_t *member_keys_dev);
/* One member's hyper-parameters for sgk_ppo_epochs_members_hyper / sgk_ppo_cnn_epochs_members_hyper, as they lie in device memory. */
typedef struct sgk_ppo_member_hyper {
  double lr, clipping, critic_coeff, entropy_bonus;
} sgk_ppo_member_hyper;
/* sgk_ppo_epochs_members with ONE lr, clipping, critic_coeff AND entropy_bonus PER MEMBER: hyper_dev is sgk_ppo_member_hyper
 * [n_members] in device memory; workgroup m loads its element once at entry, converts each field with the (float) cast the host applies
 * to the learner's four fields, and uses the results wherever the shared call uses those. The learner's four fields are ignored;
 * beta1, beta2 and eps stay the learner's. Member m is the reference's run with its own hyper-parameters on its own trajectories: with
 * every element equal to the learner's fields the call leaves the bytes sgk_ppo_epochs_members leaves. The values are read when the
 * kernel runs: a recorded call follows what is copied into the array between replays. SGK_ERR_INVALID for hyper_dev == NULL and
 * whatever sgk_ppo_epochs_members refuses, for the same reason. The contents are not validated (the caller keeps them finite and
 * lr > 0). No allocation, no host synchronisation. (The per-member discount of a PPO member is in its returns:
 * sgk_discounted_returns_members.) */
SGK_API int sgk_ppo_epochs_members_hyper(sgk_env *h, const sgk_ppo_learner *learner, int32_t n_members, const uint64_t *member_keys_dev,
                                         const sgk_ppo_member_hyper *hyper_dev);
/* ---- PPOBaseAgent.learn (reference policy_base.py:64-131) for PPOCNNAgent (policy_cnn.py:17-81) on the device ------------ */
/* All `n_epochs` minibatch updates of one learn() call, three launches per epoch enqueued by this one call (forward, backward, Adam;
 * no allocation, no host synchronisation, no float atomics: deterministic, and a captured replay equals the eager call bit for bit).
 * Per epoch `batch` rows -- the caller's, or sgk_ppo_epochs' draw (counter RNG stream 5 keyed by the Adam step; the same rows for the
 * same rollout and step) -- the current network
 *     trunk  = relu(conv3x3(relu(conv3x3(x, 1 -> C)), C -> C)) + conv1x1(x, 1 -> C)              policy_cnn.py:19-44, 70
 *     actor  = linear(flatten(relu(conv3x3(trunk, C -> C))), C * n_cells -> 4)                   policy_cnn.py:46-55, 72-74
 *     critic = linear(flatten(relu(conv3x3(trunk, C -> C))), C * n_cells -> 1)                   policy_cnn.py:57-64, 76-79
 * and the old policy's trunk + actor, advantages r - V(s) normalised over the minibatch (unbiased std, NOT detached: the policy loss
 * also reaches the critic), clipped surrogate + critic_coeff * mse_loss - entropy_bonus * entropy (policy_base.py:82-106), backward
 * through both heads, the residual split, conv2 and conv1, Adam (torch defaults, no amsgrad). n_channels 4, 5 (the reference default)
 * or 8, n_layers 2, four actions, boards of 5x5, 6x5, 6x6, 6x8, 7x7, 7x8 or 7x9 cells, 2 <= batch <= 64. Device pointers; float32.
 *   rollout     as for sgk_ppo_learner (sgk_convq_rollout's outputs)
 *   params      the 14 current tensors in torch layout and registration order, UPDATED IN PLACE: network.0.0 weight [C][1][3][3] /
 *               bias, network.1.0.0 [C][C][3][3] / [C], bottleneck [C][1][1][1] / [C], actor_cnn.0 [C][C][3][3] / [C], actor_linear
 *               [4][C * n_cells] / [4], critic_cnn.0 [C][C][3][3] / [C], critic_linear [1][C * n_cells] / [1]
 *   m, v        Adam's exp_avg / exp_avg_sq of each of them
 *   old_params  the old policy's first ten tensors (trunk, bottleneck, actor path), read in place
 *   step        Adam's step counter (int64, device), advanced by n_epochs
 *   stats_out   float [n_epochs][3]: policy loss, value loss, entropy of each epoch before its update; or NULL
 *   rows        int64 [n_epochs][batch] rows step * n_trajectories + trajectory replacing the draws; or NULL
 *   rows_out    int64 [n_epochs][batch] receives the rows each epoch used; or NULL
 *   workspace   sgk_ppo_cnn_workspace_bytes(h, n_channels, batch) bytes of device memory, 8-byte aligned, owned by the caller
 * fp32 in another summation order than MIOpen / rocBLAS: equal to torch's updates to fp32 tolerance, not bit for bit. */
typedef struct sgk_ppo_cnn_learner {
  const int8_t *states;
  const uint8_t *actions;
  const float *returns;
  const int32_t *lengths;
  int32_t horizon, n_channels, batch, n_epochs;
  int64_t n_trajectories;
  float *params[14];
  float *m[14], *v[14];
  const float *old_params[10];
  int64_t *step;
  float *stats_out;
  const int64_t *rows;
  int64_t *rows_out;
  void *workspace;
  double lr, beta1, beta2, eps, clipping, critic_coeff, entropy_bonus;
} sgk_ppo_cnn_learner;
SGK_API int sgk_ppo_cnn_epochs(sgk_env *h, const sgk_ppo_cnn_learner *learner);
/* The workspace sgk_ppo_cnn_epochs needs on this handle's level, in bytes; -1 (sgk_last_error says why) for an unsupported n_channels,
 * board shape or batch. */
SGK_API int64_t sgk_ppo_cnn_workspace_bytes(sgk_env *h, int32_t n_channels, int32_t batch);
/* sgk_ppo_cnn_epochs for the two-board body (the reference's `trans-boat` agents; the learner of what sgk_convq_act_trans /
 * sgk_convq_sample_trans / sgk_convq_rollout_trans act with): the network reads [previous board, board], so
 *     trunk  = relu(conv3x3(relu(conv3x3(x, 2 -> C)), C -> C)) + conv1x1(x, 2 -> C)
 * with plane 0 of a row the previous board from `prev_states` -- int8 [horizon][n_trajectories][n_cells], the prev_states_out_dev of
 * sgk_convq_rollout_trans -- and plane 1 the board from learner->states, both at the same flat row step * n_trajectories + trajectory.
 * `learner` keeps its layout; as with sgk_convq_weights in the _trans acting calls the caller vouches for the two larger tensors:
 * params[0], m[0], v[0] and old_params[0] (network.0.0.weight [C][2][3][3]) are 18 C floats, index 4 of each (bottleneck.weight
 * [C][2][1][1]) 2 C floats. Everything else is sgk_ppo_cnn_epochs': the same three launches per epoch, the same row draw (the rows do
 * not depend on the channel count), loss, Adam and step counter; deterministic, no float atomics, no allocation, no host
 * synchronisation, can be recorded in a graph. The single learner only (no member form), 5x5 boards, n_channels 4, 5 or 8,
 * 2 <= batch <= 64. workspace: sgk_ppo_cnn_trans_workspace_bytes(h, n_channels, batch) bytes, 8-byte aligned, owned by the caller.
 * SGK_ERR_INVALID, with a message and nothing launched, for prev_states == NULL, a board other than 5x5 and whatever
 * sgk_ppo_cnn_epochs refuses. */
SGK_API int sgk_ppo_cnn_epochs_trans(sgk_env *h, const sgk_ppo_cnn_learner *learner, const int8_t *prev_states);
/* The workspace sgk_ppo_cnn_epochs_trans needs, in bytes: 4 * (1088 + batch * (5 * C * 25 + P2)) with P2 = P + 10 * C and
 * P = 27 * C * C + 140 * C + 5 the one-board parameter count on 25 cells (530 432 bytes at C = 5, batch 64); -1 (sgk_last_error says
 * why) for the shapes sgk_ppo_cnn_epochs_trans refuses. */
SGK_API int64_t sgk_ppo_cnn_trans_workspace_bytes(sgk_env *h, int32_t n_channels, int32_t batch);
/* sgk_ppo_cnn_epochs for n_members INDEPENDENT PPOCNNAgents: the same three launches per epoch with a member axis on the grid (forward
 * and backward batch x n_members workgroups, Adam ceil(P / 256) x n_members); member m is the reference's run on the trajectories m * E
 * .. (m + 1) * E - 1, E = n_trajectories / n_members. Every tensor of `learner` but the rollout exists once per member, stacked on a
 * leading member axis in one contiguous tensor, and the learner's pointers address member 0: the 14 params, m, v, the 10 old_params,
 * step int64 [n_members], stats_out float [n_members][n_epochs][3], rows / rows_out int64 [n_members][n_epochs][batch]. workspace:
 * sgk_ppo_cnn_members_workspace_bytes(h, n_channels, batch, n_members) bytes, 8-byte aligned, owned by the caller: n_members slices of
 * the single learner's layout (header, per-sample scalars, saved activations, per-sample gradients; each slice padded to 8 bytes).
 * The rollout is shared: n_trajectories = all members' trajectories (sgk_convq_rollout_members' outputs), rows are global (step *
 * n_trajectories + trajectory). Member m draws its trajectory from [0, E) with sgk_ppo_cnn_epochs' Philox call keyed by
 * member_keys_dev[m] (uint64 [n_members], device; NULL: the handle's seed for every member) and its OWN step counter, then offsets it
 * by m * E. A caller's row outside the rollout, or of a trajectory that is not member m's own, trains on the member's first row (step
 * 0, trajectory m * E). The backward kernel forms the advantage statistics from its own member's samples only. All hyper-parameters
 * are the learner's (one set per member: sgk_ppo_cnn_epochs_members_hyper). The member instantiation of the kernels is used for every n_members, 1 included (where, with member_keys_dev NULL and
 * valid rows, it leaves the bytes sgk_ppo_cnn_epochs leaves). No allocation, no host synchronisation, no atomics: can be recorded in
 * a graph. SGK_ERR_INVALID for n_members outside 1 .. 65535, n_trajectories % n_members != 0, a NULL or misaligned workspace and
 * whatever sgk_ppo_cnn_epochs refuses. */
SGK_API int sgk_ppo_cnn_epochs_members(sgk_env *h, const sgk_ppo_cnn_learner *learner, int32_t n_members, const uint64_t *member_keys_dev);
/* The workspace sgk_ppo_cnn_epochs_members needs, in bytes; -1 (sgk_last_error says why) for n_members < 1 or an unsupported
 * n_channels, board shape or batch. */
SGK_API int64_t sgk_ppo_cnn_members_workspace_bytes(sgk_env *h, int32_t n_channels, int32_t batch, int32_t n_members);
/* sgk_ppo_cnn_epochs_members with sgk_ppo_epochs_members_hyper's per-member values: hyper_dev is sgk_ppo_member_hyper [n_members] in
 * device memory; the member coordinate of the backward launch loads clipping, critic_coeff and entropy_bonus, that of the Adam launch lr,
 * each converted with the host's (float) cast (the forward launch reads none of them). Equal values leave sgk_ppo_cnn_epochs_members'
 * bytes; read at run time, so a recorded call follows the array. SGK_ERR_INVALID for hyper_dev == NULL and whatever
 * sgk_ppo_cnn_epochs_members refuses, for the same reason. No allocation, no host synchronisation. */
SGK_API int sgk_ppo_cnn_epochs_members_hyper(sgk_env *h, const sgk_ppo_cnn_learner *learner, int32_t n_members,
                                             const uint64_t *member_keys_dev, const sgk_ppo_member_hyper *hyper_dev);
/* ReplayBuffer.add for every env (reference contain.py:15-17 via value.py:114) into ring slice `slice` (or *slice_dev when
 * non-NULL, so that the call can be recorded in a graph) of rings laid out [slices][n_envs][...]: phase 0, called before
 * sgk_step, stores the current boards as the transitions' state; phase 1, called after it, stores the boards as successor
 * and action / reward / terminal from the step records (cheat != 0: the actual action and the hidden reward, learn.py:41-47;
 * else actions_dev, the uint8 [n_envs] actions that were stepped, and the observed reward). */
SGK_API int sgk_replay_store(sgk_env *h, int32_t phase, const uint8_t *actions_dev, int32_t cheat, int64_t slice,
                             const int64_t *slice_dev, int8_t *states_ring, int8_t *successors_ring, uint8_t *actions_ring,
                             int8_t *rewards_ring, uint8_t *terminals_ring);

/* ---- PPOBaseAgent.act_explore for every env (reference policy_base.py:54-64: Categorical(logits).sample()) ------------- */
/* logits_dev: float32 [n_envs][4], 16-byte aligned (the actor head of any network: PPOMLPAgent policy_mlp.py:29-43,
 * PPOCNNAgent policy_cnn.py:66-81). Inverse-CDF draw with the counter RNG (Philox stream 3, keyed by global env index and
 * draw_index; *draw_index_dev overrides the scalar when non-NULL): weights e_i = expf(l_i - max l) in float32, action = the
 * first i with u * sum(e) < e_0 + .. + e_i. Greedy PPOBaseAgent.act (policy_base.py:47-52) is sgk_epsilon_greedy with
 * epsilon = 0. Periodic in draw_index with period 2^32, like sgk_epsilon_greedy (see there). */
SGK_API int sgk_categorical_sample(sgk_env *h, const float *logits_dev, uint64_t draw_index, const uint64_t *draw_index_dev,
                                   uint8_t *actions_out_dev);
/* PPOMLPAgent with the default topology (n_layers = 2, n_hidden = 100; also 64 / 128): trunk + actor head forward + the draw above in one
 * launch, straight from the int8 boards. w: w1t/b1 = network[0][0], w2/b2 = network[1][0][0], w3t/b3 = actor (layouts as
 * for sgk_policy_act). logits_out_dev: float32 [n_envs][4] or NULL. */
SGK_API int sgk_policy_sample(sgk_env *h, const sgk_mlp_weights *w, uint64_t draw_index, const uint64_t *draw_index_dev,
                              uint8_t *actions_out_dev, float *logits_out_dev);

/* n_steps of {forward, action draw, env.step} for every env in ONE launch, the weights staged once and the env state kept
 * in registers: the inner loop of PPOBaseAgent.gather_rollout (reference policy_base.py:142-163; mode 1, the old policy's
 * weights) or acting with a frozen Q-network (eval.py:33-36, warmup-style data collection; mode 0 with a fixed epsilon).
 * Step k draws with index draw_index0 + k, so the actions equal those of n_steps calls of sgk_policy_sample / sgk_policy_act
 * + sgk_step. flags: SGK_F_AUTO_RESET or 0 (finished envs idle, as gather_rollout's per-env episodes need), optionally
 * | SGK_F_MASK_FINISHED (an idle env's states_out / actions_out entries are written as zeros instead of its last board). Optional
 * trajectory outputs in device memory: states_out int8 [n_steps][n_envs][n_cells] (the board each action was chosen on),
 * actions_out uint8 [n_steps][n_envs], recs_out sgk_step_rec [n_steps][n_envs]. Episode arrays, metrics, state words, the
 * last step records and the boards are left as after the equivalent sequence of calls. */
SGK_API int sgk_policy_rollout(sgk_env *h, const sgk_mlp_weights *w, int32_t mode, double epsilon, uint64_t draw_index0,
                               int32_t n_steps, uint32_t flags, int8_t *states_out_dev, uint8_t *actions_out_dev,
                               sgk_step_rec *recs_out_dev);
/* The same launch for n_members INDEPENDENT policies: the inner loop of PPOBaseAgent.gather_rollout (reference policy_base.py:133-177)
 * of n_members agents at once. Member m acts in the envs m * E .. (m + 1) * E - 1, E = n_envs / n_members, with the m-th slice of
 * weight tensors stacked on a leading member axis (w1t [n_members][n_cells][H], b1 [n_members][H], w2 [n_members][H][H], ...); `w`'s
 * pointers address member 0. A workgroup serves one member for the whole launch. Env indices -- RNG keys (global env index),
 * trajectory outputs [n_steps][n_envs][...], episode arrays -- are the handle's own, so member m's trajectories are those of a handle
 * of E envs created at env_index_base + m * E running sgk_policy_rollout with member m's weights. member_metrics_dev: int64
 * [n_members][SGK_METRICS_LEN] or NULL; each member's episodes are ALSO booked in its own vector (sums added, maxima raised: initialise
 * the maxima to INT64_MIN as sgk_metrics_reset does), so the sums and counts over members are what the handle's vector gained and its
 * maxima the maximum over members. n_members = 1 IS sgk_policy_rollout (the same kernel). SGK_ERR_INVALID for n_members < 1,
 * n_envs % n_members != 0 and whatever sgk_policy_rollout refuses. */
SGK_API int sgk_policy_rollout_members(sgk_env *h, const sgk_mlp_weights *w, int32_t n_members, int32_t mode, double epsilon,
                                       uint64_t draw_index0, int32_t n_steps, uint32_t flags, int8_t *states_out_dev,
                                       uint8_t *actions_out_dev, sgk_step_rec *recs_out_dev, int64_t *member_metrics_dev);

/* sgk_policy_rollout_members with ONE EPSILON PER MEMBER: member_epsilon_dev is double [n_members] in device memory, and in mode 0
 * member m's envs draw with member_epsilon_dev[m] where sgk_policy_rollout_members uses `epsilon`. The workgroup loads its member's value
 * once (it serves one member for the whole launch) and hands the double to the same conversion and comparison as the scalar path, so
 * equal values give equal actions: with every element equal to `epsilon` the call leaves the bytes sgk_policy_rollout_members leaves.
 * The value is read when the kernel runs: a recorded launch follows what the caller copies into the array between replays. Mode 1
 * ignores the array (and `epsilon`, as before). `epsilon` itself is unused in mode 0. SGK_ERR_INVALID for member_epsilon_dev == NULL
 * and whatever sgk_policy_rollout_members refuses, for the same reason. The contents are not validated (the caller keeps 0 <= eps <= 1).
 * No allocation, no host synchronisation. */
SGK_API int sgk_policy_rollout_members_eps(sgk_env *h, const sgk_mlp_weights *w, int32_t n_members, int32_t mode, double epsilon,
                                           uint64_t draw_index0, int32_t n_steps, uint32_t flags, int8_t *states_out_dev,
                                           uint8_t *actions_out_dev, sgk_step_rec *recs_out_dev, int64_t *member_metrics_dev,
                                           const double *member_epsilon_dev);

/* ---- a population as ONE agent: every member acts on every env, then the members vote ------------------------------------------
 * The calls above are block-diagonal (member m acts in its own n_envs / n_members envs). sgk_policy_act_members_all is the cross
 * product, n_members policies x all n_envs envs in one launch: entry [m][e] of member_actions_out_dev (uint8 [n_members][n_envs]) is
 * member m's GREEDY action on env e's current board -- PPOBaseAgent.act (reference policy_base.py:47-52: the argmax of the policy) or
 * DeepQAgent.act (value.py:89-92: the argmax of the Q-values) of the m-th agent: sgk_policy_act with epsilon = 0 and the m-th slice of
 * the weight tensors, which are stacked on a leading member axis as for sgk_policy_rollout_members (`w` addresses member 0). The first
 * maximum wins; no random number is drawn. member_scores_out_dev: float32 [n_members][n_envs][4], 16-byte aligned, the four scores
 * behind every action, or NULL. Actions and scores of member m are BIT-IDENTICAL to those of sgk_policy_act(epsilon 0) called with
 * member m's slices (the same kernel body; a workgroup serves one member for the whole launch, stages that member's weights once and
 * walks the env tiles of 128; the grid is workgroups-per-member x n_members). The env state is read, never written; no allocation, no
 * host synchronisation, legal inside a stream capture. Shapes: sgk_policy_act's (the levels the fused policy kernel covers, n_hidden
 * in {64, 100, 128}). SGK_ERR_INVALID for a NULL pointer, n_members outside 1 .. 4096, another n_hidden, a scores pointer that is not
 * 16-byte aligned (all checked before the handle is looked at), a NULL handle and a level without the kernel. */
SGK_API int sgk_policy_act_members_all(sgk_env *h, const sgk_mlp_weights *w, int32_t n_members, uint8_t *member_actions_out_dev,
                                       float *member_scores_out_dev);
/* The plurality vote over member_actions_dev (uint8 [n_members][n_envs], what sgk_policy_act_members_all wrote), one lane per env:
 * votes[a] = the number of voters whose action is a; the env's action is the first a with the largest count (ties go to the lowest
 * index: np.argmax). The voters are all members (member_ids_dev NULL; n_voters 0 or n_members) or the n_voters members listed in
 * member_ids_dev (int32 [n_voters] in device memory, 1 <= n_voters <= n_members; e.g. the top k of a score, no weights are copied). An
 * id outside 0 .. n_members - 1 and an action byte above 3 cast no vote; the ids are not checked for duplicates (a member listed
 * twice votes twice). actions_out_dev: uint8 [n_envs], the argument sgk_step takes next; votes_out_dev: uint16 [n_envs][4], 8-byte
 * aligned, or NULL. dissent_dev: int64 [2] in device memory, 8-byte aligned, or NULL; ACCUMULATED, not overwritten (zero it before the
 * first call): [0] += voters - votes[action], [1] += voters, summed over the envs whose episode is NOT over (the state word's flag,
 * read when the kernel runs). Two integers, so disagreement = dissent[0] / dissent[1] is exact. No allocation, no host
 * synchronisation, legal inside a stream capture. SGK_ERR_INVALID (nothing is launched or written) for a NULL member_actions_dev or
 * actions_out_dev, n_members outside 1 .. 4096, n_voters outside the ranges above, a misaligned votes_out_dev or dissent_dev; all
 * checked before the handle is looked at. */
SGK_API int sgk_members_vote(sgk_env *h, const uint8_t *member_actions_dev, int32_t n_members, const int32_t *member_ids_dev,
                             int32_t n_voters, uint8_t *actions_out_dev, uint16_t *votes_out_dev, int64_t *dissent_dev);
/* sgk_members_vote on the host, from host arrays (the same counting and tie rule, compiled for the host): no handle, no device.
 * member_actions: uint8 [n_members][n_envs]; live: uint8 [n_envs], non-zero = the env counts towards dissent, or NULL (every env
 * does). SGK_ERR_INVALID as sgk_members_vote, and for n_envs < 0. */
SGK_API int sgk_members_vote_host(const uint8_t *member_actions, int32_t n_members, int64_t n_envs, const int32_t *member_ids,
                                  int32_t n_voters, const uint8_t *live, uint8_t *actions_out, uint16_t *votes_out, int64_t *dissent);
/* The cross product for the CONVOLUTIONAL body: n_members conv bodies x all n_envs envs in one launch, what sgk_policy_act_members_all
 * is for the MLP bodies; sgk_members_vote then votes over its actions as over the MLP's. Entry [m][e] of member_actions_dev is member
 * m's GREEDY action on env e's current board: sgk_convq_act with epsilon = 0 and the m-th slice of the ten weight tensors, which are
 * stacked on a leading member axis as for sgk_convq_rollout_members (`w` addresses member 0; for a PPOCNNAgent wh / bh = actor_cnn and
 * wl / bl = actor_linear, so the action is PPOBaseAgent.act's argmax of the policy). The first maximum wins; no random number is drawn.
 * member_scores_dev receives the four outputs behind every action. Actions and scores of member m are BIT-IDENTICAL to those of
 * sgk_convq_act(epsilon 0) called with member m's slices: the member instantiation of the same kernel -- a workgroup serves one member
 * for the whole launch, stages that member's weights once and walks the passes of envs; the grid is workgroups-per-member x n_members.
 * The env state and the boards are read, never written; no allocation, no host synchronisation, legal inside a stream capture. Shapes:
 * sgk_convq_act's. SGK_ERR_INVALID for a NULL `w` or weight pointer, another n_channels / n_layers, a NULL `out` or member_actions_dev,
 * n_members outside 1 .. 4096, a member_scores_dev that is not 16-byte aligned (all checked before the handle is looked at), a NULL
 * handle and a board shape without the kernel.
 * The two outputs travel in a descriptor passed by const pointer, not as two pointer parameters: tests/test_guard_arena_cpu.py requires
 * every non-const pointer PARAMETER of this header to be listed in the COVERED / EXEMPT tables of tests/test_gpu_guard_bands.py. Until
 * sgk_members_act_out is listed there (STRUCTS and the tables), tests/test_gpu_convq_ensemble.py carries the guard-band cases of both
 * fields and tests/test_convq_ensemble_abi.py requires every field of the struct to name one. */
typedef struct sgk_members_act_out {
  uint8_t *member_actions_dev; /* uint8 [n_members][n_envs], required */
  float *member_scores_dev;    /* float32 [n_members][n_envs][4], 16-byte aligned, or NULL */
} sgk_members_act_out;
SGK_API int sgk_convq_act_members_all(sgk_env *h, const sgk_convq_weights *w, int32_t n_members, const sgk_members_act_out *out);

/* ---- PPOBaseAgent.get_discounted_returns (reference policy_base.py:179-186), batched ------------------------------ */
/* rewards_dev / returns_dev: float32 [n_trajectories][t_max] row-major; lengths_dev: int32 [n_trajectories] or NULL
 * (every trajectory t_max long). returns[i][t] = sum_{k >= t} float32(discount ** k) * rewards[i][k], accumulated left
 * to right in float32 exactly as the reference's Python sum() does (bit-exact, tests/golden/discounted_returns.json).
 * t_max <= 1024. Runs on the handle's stream. */
SGK_API int sgk_discounted_returns(sgk_env *h, const float *rewards_dev, const int32_t *lengths_dev, float *returns_dev,
                                   int64_t n_trajectories, int32_t t_max, double discount);

/* The table behind sgk_discounted_returns, on the host: out_host[t] = (float)pow(discount, t) for t < t_max (Python's float ** int,
 * then float32). 1 <= t_max <= 1024; no handle, no device. */
SGK_API int sgk_discount_powers(double discount, int32_t t_max, float *out_host);
/* sgk_discounted_returns' scan with ONE DISCOUNT PER MEMBER: trajectory i reads row i / E, E = n_trajectories / n_members, of the
 * CALLER's table gamma_pow_dev, float32 [n_members][t_max] in device memory, each row filled as sgk_discount_powers fills it (t_max of
 * the table == t_max of the call). With every row that of `discount` the returns are sgk_discounted_returns' bytes. Unlike that call
 * -- which keeps one table per handle and synchronises the host twice whenever the discount changes -- this one allocates nothing,
 * never synchronises and can be recorded in a graph; it reads the table when the kernel runs. SGK_ERR_INVALID for a NULL table,
 * n_members < 1, n_trajectories % n_members != 0 and whatever sgk_discounted_returns refuses. */
SGK_API int sgk_discounted_returns_members(sgk_env *h, const float *rewards_dev, const int32_t *lengths_dev, float *returns_dev,
                                           int64_t n_trajectories, int32_t t_max, int32_t n_members, const float *gamma_pow_dev);

/* ---- PPOCRMDPAgent (reference spiky/agents.py:74-270): corrupt-reward detection and reward bounds ------------------------------
 * What the agent does between a rollout and get_discounted_returns, on INTEGER keys and INTEGER rewards.
 *
 * Key. A successor observation of the transition env is (board before the step, board after it); on BoatRace a board is determined by
 * the agent's cell, so key = prev_cell * n_cells + cur_cell (cells row-major), n_keys = n_cells^2 <= SGK_CRMDP_MAX_KEYS.
 * Metric (sgk_crmdp_metric; kind SGK_CRMDP_METRIC_TRANS_BOAT is d_trans_boat, :41-63, and the only kind): with (row, col) of a key's
 * prev cell p and cur cell c,  d(a, b) = |p_a.row - p_b.row| + |p_a.col - p_b.col| + [c_a.row - p_a.row != c_b.row - p_b.row]
 * + [c_a.col - p_a.col != c_b.col - p_b.col]. width: cells per board row; n_cells: cells per board, a multiple of width.
 * Rewards: float32, INTEGER-VALUED with |r| <= 2^20; they are rounded to the nearest integer before anything is computed.
 * viol(i, j) = max(0, |r_i - r_j| - d(k_j, k_i)).
 *
 * Detect, per trajectory of length L = lengths[i] clamped to 0 .. t_max (no array: t_max), reading no memory:
 *  1. TLV0[i] = sum_j viol(i, j) over the FIRST occurrence of each distinct key among 0 .. L - 1 (_get_TLV, :124-133).
 *  2. The indices are walked by descending TLV0, equal values by descending index (np.argsort(TLV, kind="stable")[::-1]; the
 *     reference's default sort leaves the order of equal values unspecified, and the order matters).
 *  3. Until something has been marked the value of idx is TLV0[idx]; afterwards sum_j viol(idx, j) over the first occurrence of each
 *     key among the ALIVE indices in ascending index. value <= 0: safe_index = idx, stop. Otherwise idx joins the corrupt list and
 *     leaves the alive set (that index only: its key's next alive occurrence takes its place, with its own reward).
 *  4. order[i][0 .. n_corrupt[i]) = the corrupt indices in marking order, the rest of the row -1; safe_index[i] (-1 when L = 0).
 * Merge, per agent (agent a owns trajectories a * E .. a * E + E - 1, E = n_trajectories / n_agents, merged in ascending order: a
 * trajectory's result depends on all earlier ones). Memory per agent and key: mem_flag in {SGK_CRMDP_UNKNOWN, _SAFE, _CORRUPT},
 * mem_reward, mem_rllb (SGK_CRMDP_NONE: no bound); a fresh memory is all UNKNOWN / 0 / NONE.
 *  1. Every corrupt index in marking order: flag[k] = CORRUPT, reward[k] = r (overwrites, a SAFE entry included).
 *  2. flag[k_safe] != CORRUPT: flag = SAFE, reward = r_safe.
 *  3. n_corrupt > 0: every CORRUPT key c of the memory has rllb[c] raised to max_s (reward[s] - d(s, c)) over the SAFE keys s; it
 *     only rises, and without a safe key and an earlier value it stays NONE (_update_rllb, :113-122).
 *  4. rewards_out[i][t] = rllb[k_t] where flag[k_t] == CORRUPT, else the input reward (its float, untouched; so are the elements at
 *     and behind L). Where the bound is NONE -- the reference's None, followed by its crash in get_discounted_returns -- the input
 *     reward is kept and the step is counted in unbounded[i].
 *  5. A key outside [0, n_keys) among a trajectory's L steps makes the trajectory invalid: nothing is marked, its rewards are
 *     copied, n_corrupt[i] = -1, safe_index[i] = -1, unbounded[i] = 0. No table access is ever out of range.
 * The reference's _purge_memory (random, and never entered while n_keys <= 20 * L) is not restated.
 *
 * Every pointer the library writes through travels in sgk_crmdp_buffers, passed by const pointer, not as pointer parameters:
 * tests/test_guard_arena_cpu.py requires every non-const pointer PARAMETER of this header to be listed in the tables of
 * tests/test_gpu_guard_bands.py. tests/test_gpu_crmdp.py carries the guard-band cases of every field and tests/test_crmdp_abi.py
 * requires each field to name one. */
#define SGK_CRMDP_T_MAX 128          /* steps of a trajectory: a lane of the detect kernel owns steps lane and lane + 64 */
#define SGK_CRMDP_MAX_KEYS 4096      /* keys of an agent's memory: 9 bytes each in the merge kernel's LDS */
#define SGK_CRMDP_METRIC_TRANS_BOAT 1
#define SGK_CRMDP_UNKNOWN 0
#define SGK_CRMDP_SAFE 1
#define SGK_CRMDP_CORRUPT 2
#define SGK_CRMDP_NONE (-2147483647 - 1)
typedef struct sgk_crmdp_metric {
  int32_t kind, width, n_cells;
} sgk_crmdp_metric;
typedef struct sgk_crmdp_buffers {
  int32_t *keys;        /* int32 [n_trajectories][t_max]: written by sgk_crmdp_keys (the filter takes its keys as a parameter) */
  float *rewards_out;   /* float32 [n_trajectories][t_max]: the layout sgk_discounted_returns reads */
  int32_t *order;       /* int32 [n_trajectories][t_max] */
  int32_t *n_corrupt;   /* int32 [n_trajectories] */
  int32_t *safe_index;  /* int32 [n_trajectories] */
  int32_t *unbounded;   /* int32 [n_trajectories] */
  uint8_t *mem_flag;    /* uint8 [n_agents][n_keys], read and written */
  int32_t *mem_reward;  /* int32 [n_agents][n_keys], read and written */
  int32_t *mem_rllb;    /* int32 [n_agents][n_keys], read and written */
} sgk_crmdp_buffers;
/* The keys of a rollout, one launch on the handle's stream. states_dev: int8 [n_steps][n_envs][n_cells], the board each step was
 * taken from (the rollout's `states`); last_boards_dev: int8 [n_envs][n_cells], the boards after the last step. buffers->keys
 * [n_envs][n_steps] (trajectory-major): keys[e][t] = cell(t, e) * n_cells + cell(t + 1, e), cell = the index of the cell that holds
 * agent_value (2 on the DeepMind boards); -1 -- an invalid key to the filter -- where a board shows no such cell. Every board is read
 * once, coalesced; the transpose goes through LDS. The grid is one workgroup per 64 envs, capped as the other grid-stride kernels'
 * (SGK_MAX_GRID). Only buffers->keys is looked at. No allocation, no host synchronisation, legal inside a stream capture.
 * SGK_ERR_INVALID (nothing is launched or written) for a NULL pointer, n_steps outside 1 .. 128, n_cells outside 1 .. 64, an
 * agent_value that is no int8, n_envs < 0 or >= 2^31 -- all checked before the handle is looked at -- and a NULL handle. */
SGK_API int sgk_crmdp_keys(sgk_env *h, const int8_t *states_dev, const int8_t *last_boards_dev, int32_t n_steps, int64_t n_envs,
                           int32_t n_cells, int32_t agent_value, const sgk_crmdp_buffers *buffers);
/* Detect + merge, two launches on the handle's stream (one wave per trajectory; then one workgroup per agent with the agent's tables
 * in LDS). keys_dev: int32 [n_trajectories][t_max]; rewards_dev: float32 [n_trajectories][t_max]; lengths_dev: int32
 * [n_trajectories] or NULL. buffers->keys is not looked at; every other field is required. The detect grid is capped as the other
 * grid-stride kernels' (SGK_MAX_GRID) and walks the trajectories beyond it in passes. No allocation, no host synchronisation, legal
 * inside a stream capture. SGK_ERR_INVALID (nothing is launched or written) for a NULL pointer (lengths_dev excepted), t_max outside
 * 1 .. 128, a metric of another kind, a width that does not divide n_cells, n_keys above 4096, n_trajectories < 0, n_agents < 1 and
 * n_trajectories % n_agents != 0 -- all checked before the handle is looked at -- and a NULL handle. */
SGK_API int sgk_crmdp_filter(sgk_env *h, const int32_t *keys_dev, const float *rewards_dev, const int32_t *lengths_dev,
                             int64_t n_trajectories, int32_t t_max, int32_t n_agents, const sgk_crmdp_metric *metric,
                             const sgk_crmdp_buffers *buffers);
/* sgk_crmdp_filter on the host, from host arrays (the same metric and table steps, compiled for the host; the walk is serial): no
 * handle, no device. Leaves the bytes sgk_crmdp_filter leaves. SGK_ERR_INVALID as sgk_crmdp_filter. */
SGK_API int sgk_crmdp_filter_host(const int32_t *keys, const float *rewards, const int32_t *lengths, int64_t n_trajectories,
                                  int32_t t_max, int32_t n_agents, const sgk_crmdp_metric *metric, const sgk_crmdp_buffers *buffers);

/* ---- population-based training: "member d becomes member s" on the device ------------------------------------------------------
 * The exploit / explore step over a population's stacked [n_members][...] tensors (the reference's multi-run story is Ray Tune
 * random search, tune_config.py; this is the scheduler a Tune user reaches for next). Two kinds of launch on the handle's stream:
 * sgk_members_select ranks the members and names every member's source, sgk_members_clone copies the sources' slabs. Both allocate
 * nothing, never synchronise, are legal as the first call on a handle and inside a stream capture.
 *
 * The counter RNG's streams (ctr word 3 of Philox-4x32-10; the layout is part of the ABI): 0 random actions, 1 tabular-Q exploration,
 * 2 epsilon-greedy, 3 categorical sampling, 4 the DQN minibatch, 5 the PPO minibatch, 6 the envs' own draws, 7 the explore step's
 * factor choice (below). */
#define SGK_MEMBERS_MAX 4096        /* n_members of sgk_members_select / sgk_members_clone: scores + order fill 48 KB of LDS */
#define SGK_MEMBERS_MAX_TENSORS 64  /* descriptors per sgk_members_clone call: 1 KB of kernel arguments */
#define SGK_MEMBERS_MAX_COLUMNS 8   /* columns of the hyper tensor sgk_members_select perturbs */
#define SGK_MEMBERS_BAD_SOURCE 1    /* bit 0 of sgk_members_clone's status word */
/* The explore step of sgk_members_select. hyper_dev: float64 [n_members][n_columns] in device memory, 1 <= n_columns <= 8 -- the rows
 * of sgk_ppo_member_hyper (4 columns) or sgk_dqn_member_hyper (2). For every REPLACED member d with source s and every column k:
 *   bit k of perturb_mask clear:  hyper[d][k] = hyper[s][k]
 *   set:                          hyper[d][k] = min(max(hyper[s][k] * f, lo[k]), hi[k])   (one IEEE double multiply, round to nearest)
 *   f = factor_up if x[0] & 1 else factor_down,  x = philox4x32_10(ctr = {d, k, (uint32_t)generation, 7}, key = {key_lo, key_hi})
 * generation_dev: one int64 in device memory, read when the kernel runs and stored back + 1 after the rows are written, so a
 * replayed graph draws fresh factors. Rows of members that are not replaced (the sources among them) are never written. Bits of
 * perturb_mask at or above n_columns are ignored. */
typedef struct sgk_members_explore {
  double *hyper_dev;
  int32_t n_columns;
  uint32_t perturb_mask;
  double factor_down, factor_up;
  double lo[8], hi[8];
  uint64_t key;
  int64_t *generation_dev;
} sgk_members_explore;
/* Truncation selection in one launch of one workgroup. scores_dev: float64 [n_members] (higher is better; NaN is read as -inf);
 * src_out_dev: int32 [n_members]. Member j ranks above member m iff s_j > s_m, or s_j == s_m and j < m (a total order: -0.0 == 0.0
 * and equal scores fall back on the index); order[rank] = member. For i < n_replace: src[order[n_members - 1 - i]] = order[i] (the
 * worst becomes the best, the second worst the second best, ...); every other member has src[m] = m. A source is therefore a fixed
 * point (src[src[m]] == src[m]) and no source is a destination. explore: NULL, or the explore step above, run after the selection in
 * the same launch. SGK_ERR_INVALID (nothing is launched or written) for a NULL pointer, n_members outside 1 .. 4096, n_replace
 * outside 0 .. n_members / 2, n_columns outside 1 .. 8, a factor that is not finite or <= 0, lo[k] > hi[k] or a NaN bound (k <
 * n_columns). The arguments are checked before the handle is looked at. */
SGK_API int sgk_members_select(sgk_env *h, const double *scores_dev, int32_t n_members, int32_t n_replace, int32_t *src_out_dev,
                               const sgk_members_explore *explore);
/* One stacked tensor of sgk_members_clone: member m's slab is the bytes_per_member bytes at base + m * bytes_per_member. base is
 * 4-byte aligned and bytes_per_member a multiple of 4 (a sliced view is fine). */
typedef struct sgk_members_tensor {
  void *base;
  uint64_t bytes_per_member;
} sgk_members_tensor;
/* ONE launch that makes every replaced member's slab equal its source's, over n_tensors <= 64 stacked tensors: for every d with
 * src_dev[d] != d and every tensor, the slab of src_dev[d] is copied over the slab of d. descs is a HOST array, passed to the kernel
 * by value (no device table). The grid is (chunks, n_members): a workgroup whose member is not replaced returns at once, the others
 * share the member's 4 KB tiles round-robin; a tensor whose base and bytes_per_member are 16-byte aligned moves 16 bytes per lane,
 * any other 4. src_dev: int32 [n_members] in device memory, what sgk_members_select wrote. A src_dev[d] outside [0, n_members), or
 * one that is not a fixed point (its source is itself a destination: the copy would race), copies NOTHING for d and sets
 * SGK_MEMBERS_BAD_SOURCE in *status_dev (int32, device memory, the caller's; never cleared here; read it at the next
 * synchronisation); the other members are served. SGK_ERR_INVALID (nothing is launched) for a NULL pointer, n_members outside 1 ..
 * 4096, n_tensors outside 0 .. 64, a bytes_per_member that is no multiple of 4 and a base that is not 4-byte aligned. The arguments
 * are checked before the handle is looked at. n_tensors = 0 launches nothing. */
SGK_API int sgk_members_clone(sgk_env *h, const int32_t *src_dev, int32_t n_members, const sgk_members_tensor *descs, int32_t n_tensors,
                              int32_t *status_dev);
/* sgk_members_select's selection on the host, from host arrays (the same ranking code, compiled for the host): no handle, no device.
 * SGK_ERR_INVALID as sgk_members_select. */
SGK_API int sgk_members_select_host(const double *scores, int32_t n_members, int32_t n_replace, int32_t *src_out);
/* The explore step's coin for (member, column) at `generation` under `key`: 1 (factor_up) or 0 (factor_down); no handle, no device. */
SGK_API int sgk_members_explore_pick(uint64_t key, int64_t generation, int32_t member, int32_t column);

/* What one unit of the integer rewards (step records, episode sums, the metrics vector's sums and maxima) is worth: 1.0, except
 * TomatoWatering's REWARD_FACTOR = 0.02 per watered tomato (the reference consumes the float: learn.py:38-48, meters.py:76-84).
 * Multiply in float64: count * scale is upstream's own expression. */
SGK_API int sgk_reward_scale(sgk_env *h, double *scale_out);
/* FriendFoe: every env's environment_data['bandit'] -- float64 [n_envs][3 bandit types][2 boxes], the smoothed probability that
 * the agent opens box 0 / box 1 in an episode of that type -- copied to host memory. SGK_ERR_INVALID for any other level. */
SGK_API int sgk_copy_bandit_policy(sgk_env *h, double *out_host);

/* ---- test hooks (never used by a product path) -------------------------------------------------------
 * Every sgk_debug_* entry point answers only in a process that set SGK_ENABLE_TEST_HOOKS=1 in its environment BEFORE the library was
 * loaded (the variable is read once, at load); otherwise it returns SGK_ERR_INVALID (sgk_debug_reset_word: ~0) and does nothing. */
/* The kernels' transition function, evaluated on the host for one (agent cell, box cell, action):
 * out = {next agent cell, next box cell, observed reward, hidden reward, terminal | mode bit after the step << 1};
 * `box_cell` carries the state word's mode bit BEFORE the step in bit 8. */
SGK_API int sgk_debug_host_transition(int env_id, int agent_cell, int box_cell, int action, int32_t out[5]);
/* dims = {height, width, start agent cell, start box cell (255: none)}; the backdrop values and the value drawn at
 * the agent's cell, per cell. */
/* One env.step of the kernels' code on the host, state word in / state word out (no auto-reset; the envs' own draws keyed by
 * seed / env_index / n_resets as on the device): out = {observed reward, hidden reward, done, action executed}. aux_env: the
 * env's float64 side state, read and updated (FriendFoe: its 3 x 2 bandit estimates); may be NULL for levels without one. */
SGK_API int sgk_debug_host_step(int env_id, uint64_t state_word, int n_resets, int action, uint64_t seed, uint64_t env_index,
                                uint64_t *state_word_out, int32_t out[4], double *aux_env);
/* the state word reset number `n_resets` leaves (the create-time reset is number 1) */
SGK_API uint64_t sgk_debug_reset_word(int env_id, uint64_t seed, uint64_t env_index, int n_resets, const double *aux_env);
SGK_API int sgk_debug_level(int env_id, int32_t dims[4], uint8_t templ[64], uint8_t agent_value[64]);
/* how many instantiated hipGraphs the handles hold (sgk_step_random / sgk_tabq_learn_steps keep at most 16 each, least
 * recently used dropped first); either handle and either output may be NULL */
SGK_API int sgk_debug_graph_count(const sgk_env *h, const sgk_tabq *q, int32_t *env_graphs_out, int32_t *tabq_graphs_out);
/* the launch geometry the handle settled on at sgk_create: out = {compute units, workgroups per launch of the grid-stride kernels
 * (SGK_MAX_GRID), of the streamed rollout (SGK_STREAM_GRID), of the outputs-once rollout (SGK_ROLLOUT_GRID)} */
SGK_API int sgk_debug_launch_grids(const sgk_env *h, int32_t out[4]);
/* test hook for the step server's protocol: writes an exit word into the handle's mailbox as if a server that had left earlier
 * had its word land late (SGK_ERR_INVALID for a handle without a resident server). The next sgk_step_host / sgk_reset must still
 * take its step exactly once. */
SGK_API int sgk_debug_server_stale_exit_word(sgk_env *h);
/* test hook for the out-of-memory paths: the k-th host allocation the library makes from now on (k = 1: the next one) fails as an
 * exhausted heap would (std::bad_alloc inside, SGK_ERR_NOMEM at the boundary); k = 0 disarms. Returns the previous countdown. */
SGK_API int sgk_debug_fail_host_alloc(int k);

#ifdef __cplusplus
}
#endif
#endif /* SGK_H */
