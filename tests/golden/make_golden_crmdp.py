#!/usr/bin/env python3
"""Generate tests/golden/crmdp_plans.npz and tests/golden/train_transboat_ppo_crmdp_seed*.json by RUNNING THE REFERENCE's
PPOCRMDPAgent (spiky/agents.py:74-270) in the build container, under the stubs of make_golden.py (which stays as it is; see its
docstring for what is stubbed and what the fixtures pin). Only arrays and JSON are committed.

    python tests/golden/make_golden_crmdp.py

One change is made to what the reference runs: `np.argsort` IN spiky.agents' NAMESPACE sorts with kind="stable". The reference walks a
trajectory's states by `np.argsort(TLV)[::-1]` (:182); numpy's default sort leaves the order of equal keys unspecified (for more than 16
elements it is an introsort), equal TLVs are the rule (most states violate nothing: TLV 0) and the order decides which state is marked
safe and which corrupt -- this script asserts that it changes the outcome on its own plans. A restatement on the device cannot follow
an unspecified order, so the rule is fixed: descending TLV, equal values by descending index, which is what the stable sort reversed
gives.

crmdp_plans.npz: 6 agents x 8 trajectories of BoatRace walks (random actions on the oracle's TransitionBoatRace env; lengths 1 .. 100)
under three reward plans -- agents 0, 1: BoatRace's own rewards; 2, 3: its own with +-60 outliers injected; 4, 5: uniform in -3 .. 3 --
and, after every trajectory, the reference's `states`, `rllb` and get_modified_rewards_for_rollout (with a mask where it returns None).
The keys are prev cell * 25 + cur cell of the successor observation (the agent is the cell that holds 2)."""
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path, chdirs into the reference)
import numpy as np  # noqa: E402

N_AGENTS, PER_AGENT, T_MAX, N_CELLS, WIDTH = 6, 8, 100, 25, 5
NONE = -2 ** 31
PLANS = ("boat", "boat", "injected", "injected", "uniform", "uniform")  # agent -> reward plan
LENGTHS = [100, 1, 64, 2, 99, 65, 63, 100,   37, 100, 8, 100, 64, 99, 21, 100,
           100, 63, 100, 2, 65, 100, 1, 77,   99, 100, 64, 50, 100, 13, 100, 65,
           100, 100, 1, 63, 99, 2, 100, 64,   65, 100, 30, 100, 99, 100, 9, 63]
EVENTS = ("safe_refused_memory_corrupt", "corrupt_overwrites_safe", "key_marked_twice_different_rewards", "safe_refused_marked_this_trajectory",
          "reward_without_bound")


class _StableNumpy:
    """numpy, with argsort stable unless the caller names a kind."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        kwargs.setdefault("kind", "stable")
        return np.argsort(a, *args, **kwargs)


def _key(obs):
    prev, cur = np.flatnonzero(obs[0].ravel() == 2), np.flatnonzero(obs[1].ravel() == 2)
    assert len(prev) == 1 and len(cur) == 1
    return int(prev[0]) * N_CELLS + int(cur[0])


def _walks(rng):
    """48 random walks on TransitionBoatRace: (successor observations float32 [L, 2, 5, 5], observed rewards)."""
    env = MG.OracleGridworldEnv("TransitionBoatRace-v0")
    out = []
    for L in LENGTHS:
        env.reset()
        boards, rewards = [], []
        for _ in range(L):
            obs, r, done, _ = env.step(int(rng.integers(4)))
            boards.append(obs.astype(np.float32))
            rewards.append(int(r))
        out.append((boards, rewards))
    return out


def _plan_rewards(plan, rewards, rng):
    if plan == "boat":
        return list(rewards)
    if plan == "injected":
        out = list(rewards)
        for i in range(len(out)):
            if rng.random() < 0.08:
                out[i] = int(rng.choice([-60, 60]))
        return out
    return [int(v) for v in rng.integers(-3, 4, size=len(rewards))]


def _agent(ref_agents, parser):
    args = parser.parse_args(["trans-boat", "ppo-crmdp", "-l", "0.001", "-r", "1", "-e", "1"])
    args.device = "cpu"
    return ref_agents.PPOCRMDPAgent(MG.OracleGridworldEnv("TransitionBoatRace-v0"), args)


def _run(ref_agents, parser, walks, rewards):
    """Every agent through its trajectories -> per trajectory (flag, reward, rllb [625], modified [T_MAX], none mask [T_MAX]), events."""
    events = dict.fromkeys(EVENTS, 0)
    flag = np.zeros((len(walks), N_CELLS ** 2), np.uint8)
    rew = np.zeros((len(walks), N_CELLS ** 2), np.int32)
    rllb = np.full((len(walks), N_CELLS ** 2), NONE, np.int32)
    modified = np.zeros((len(walks), T_MAX), np.float32)
    none = np.zeros((len(walks), T_MAX), bool)
    seconds = []
    for a in range(N_AGENTS):
        agent = _agent(ref_agents, parser)
        key_of = {}
        for e in range(PER_AGENT):
            i = a * PER_AGENT + e
            boards, r = walks[i][0], [float(v) for v in rewards[i]]
            for b in boards:
                key_of[b.tobytes()] = _key(b)
            # what the events are read from: the agent's own calls during identify_corruption_in_trajectory
            before = {k: list(v) for k, v in agent.states.items()}
            marked = {}
            orig_corrupt, orig_is = agent._mark_state_corrupt, agent._is_state_corrupt

            def spy_corrupt(board, reward, marked=marked, before=before, orig=orig_corrupt):
                k = board.tobytes()
                if k in agent.states and agent.states[k][0]:
                    events["corrupt_overwrites_safe"] += 1
                if k in marked and marked[k] != reward:
                    events["key_marked_twice_different_rewards"] += 1
                marked[k] = reward
                orig(board, reward)

            def spy_is(board, marked=marked, before=before, orig=orig_is):
                answer = orig(board)
                if answer and spy_is.live:
                    k = board.tobytes()
                    if k in marked:
                        events["safe_refused_marked_this_trajectory"] += 1
                    elif k in before and not before[k][0]:
                        events["safe_refused_memory_corrupt"] += 1
                return answer

            spy_is.live = True
            agent._mark_state_corrupt, agent._is_state_corrupt = spy_corrupt, spy_is
            t0 = time.perf_counter()
            agent.identify_corruption_in_trajectory(boards, r)
            spy_is.live = False
            out = agent.get_modified_rewards_for_rollout(boards, r)
            seconds.append(time.perf_counter() - t0)
            agent._mark_state_corrupt, agent._is_state_corrupt = orig_corrupt, orig_is
            assert agent.state_memory_cap == 0  # (the purge belongs to gather_rollout and is never entered on this level)
            for t, v in enumerate(out):
                if v is None:
                    none[i, t] = True
                    events["reward_without_bound"] += 1
                else:
                    assert float(v) == int(v)
                    modified[i, t] = v
            for k, (ok, reward) in agent.states.items():
                flag[i, key_of[k]], rew[i, key_of[k]] = (1 if ok else 2), int(reward)
            for k, bound in agent.rllb.items():
                if bound is not None:
                    rllb[i, key_of[k]] = int(bound)
    return (flag, rew, rllb, modified, none), events, seconds


def golden_plans(ref_agents, parser):
    rng = np.random.default_rng(20261020)
    walks = _walks(rng)
    rewards = [_plan_rewards(PLANS[i // PER_AGENT], walks[i][1], rng) for i in range(len(walks))]
    keys = np.zeros((len(walks), T_MAX), np.int32)
    r_arr = np.zeros((len(walks), T_MAX), np.float32)
    for i, (boards, _) in enumerate(walks):
        keys[i, :len(boards)] = [_key(b) for b in boards]
        r_arr[i, :len(boards)] = rewards[i]
    plain_np = ref_agents.np
    default_sort, _, _ = _run(ref_agents, parser, walks, rewards)  # numpy's default sort, for the comparison only
    ref_agents.np = _StableNumpy()
    try:
        stable, events, seconds = _run(ref_agents, parser, walks, rewards)
    finally:
        ref_agents.np = plain_np
    differs = [i for i in range(len(walks)) if any(not np.array_equal(x[i], y[i]) for x, y in zip(stable, default_sort))]
    # the fixture's own conditions, on the reference's output alone
    for name in EVENTS:
        assert events[name] >= 1, (name, events)
    assert differs, "the stable and the default sort agree on every trajectory: the plans do not show why the tie rule is fixed"
    boat = [i for i in range(len(walks)) if PLANS[i // PER_AGENT] == "boat"]
    assert not stable[4][boat].any(), "a BoatRace-reward trajectory has a reward without a bound"
    assert {1, 2, 63, 64, 65, 99, 100} <= set(LENGTHS) and len(LENGTHS) == N_AGENTS * PER_AGENT
    path = os.path.join(HERE, "crmdp_plans.npz")
    np.savez_compressed(path, keys=keys, rewards=r_arr, lengths=np.array(LENGTHS, np.int32), plan=np.array([PLANS[i // PER_AGENT] for i in range(len(walks))]),
                        n_agents=np.int32(N_AGENTS), width=np.int32(WIDTH), n_cells=np.int32(N_CELLS),
                        flag=stable[0], reward=stable[1], rllb=stable[2], modified=stable[3], modified_none=stable[4],
                        event_names=np.array(EVENTS), event_counts=np.array([events[k] for k in EVENTS], np.int64),
                        default_sort_differs=np.array(differs, np.int32))
    print("wrote", path, os.path.getsize(path), "bytes; events", events, "; default sort differs on trajectories", differs)
    steps = sum(LENGTHS)
    print("reference, this CPU box, one thread, indicative only: %.4f s per trajectory (mean of %d, %d steps in all; max %.4f s for a "
          "trajectory of %d steps)" % (sum(seconds) / len(seconds), len(seconds), steps, max(seconds), LENGTHS[int(np.argmax(seconds))]))


def main():
    MG._install_stubs()
    import safe_grid_agents.spiky.agents as ref_agents
    from safe_grid_agents.parsing import prepare_parser

    MG._PARSER = prepare_parser()  # (it consumes module-level YAML dicts: once per process)
    only = sys.argv[1:]
    if not only or "plans" in only:
        golden_plans(ref_agents, MG._PARSER)
    plain_np = ref_agents.np
    ref_agents.np = _StableNumpy()
    try:
        if not only or "train" in only:
            MG.golden_train_ppo("train_transboat_ppo_crmdp_seed4.json",
                                ["-S", "4", "-E", "3", "-EE", "2", "-V", "110", "-EV", "0", "trans-boat", "ppo-crmdp", "-l", "0.002",
                                 "-r", "3", "-e", "4", "-b", "16", "-ch", "3"])
            MG.golden_train_ppo("train_transboat_ppo_crmdp_seed6_cheat.json",
                                ["-S", "6", "-E", "3", "-EE", "2", "-V", "110", "-EV", "0", "-C", "-D", "0.9", "trans-boat", "ppo-crmdp",
                                 "-l", "0.002", "-r", "2", "-e", "3", "-b", "16", "-ch", "3", "-c", "0.1"])
    finally:
        ref_agents.np = plain_np
    leaked = [os.path.join(d, f) for d, _, fs in os.walk(MG.REF) for f in fs if f.endswith(".pyc")]
    assert not leaked, leaked


if __name__ == "__main__":
    main()
