"""PPOCRMDPAgent's corrupt-reward detection without a GPU: the dictionary restatement (tests/crmdp_reference.py) equals the reference's
recorded output after every trajectory (tests/golden/crmdp_plans.npz), sgk_crmdp_filter_host equals the restatement in every output,
exactly, the refusals leave their outputs untouched, and the single-env agent's train() reproduces the reference's own run."""
import ctypes
import json
import os

import numpy as np
import pytest

import crmdp_plans as P
import crmdp_reference as R
import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib


def test_the_fixture_meets_its_own_conditions():
    g = P.plans()
    n, t_max = g["keys"].shape
    assert (n, t_max, int(g["n_agents"]), int(g["width"]), int(g["n_cells"])) == (48, 100, 6, 5, 25)
    assert {1, 2, 63, 64, 65, 99, 100} <= set(g["lengths"].tolist())
    assert list(g["event_names"]) == ["safe_refused_memory_corrupt", "corrupt_overwrites_safe", "key_marked_twice_different_rewards",
                                      "safe_refused_marked_this_trajectory", "reward_without_bound"]
    assert (g["event_counts"] >= 1).all(), dict(zip(g["event_names"], g["event_counts"]))
    assert len(g["default_sort_differs"]) >= 1  # numpy's default sort gives another outcome: why the tie rule is fixed
    boat = g["plan"] == "boat"
    assert boat.sum() == 16 and not g["modified_none"][boat].any()
    assert g["modified_none"][g["plan"] == "uniform"].any()
    assert int(g["modified_none"].sum()) == int(g["event_counts"][4])
    live = np.arange(t_max)[None, :] < g["lengths"][:, None]
    assert ((g["keys"] >= 0) & (g["keys"] < 625)).all() and (g["rewards"] == np.round(g["rewards"])).all()
    assert not g["modified_none"][~live].any()
    assert (g["flag"][boat] == R.CORRUPT).any()  # BoatRace's own rewards do mark states corrupt


def test_the_restatement_equals_the_reference_after_every_trajectory():
    g = P.plans()
    out, tables = P.restated()
    live = np.arange(g["keys"].shape[1])[None, :] < g["lengths"][:, None]
    for i in range(g["keys"].shape[0]):
        assert np.array_equal(tables["mem_flag"][i], g["flag"][i]), i
        assert np.array_equal(tables["mem_reward"][i], g["reward"][i]), i
        assert np.array_equal(tables["mem_rllb"][i], g["rllb"][i]), i
        assert np.array_equal(out["none"][i], g["modified_none"][i]), i
        keep = live[i] & ~g["modified_none"][i]
        assert np.array_equal(out["rewards_out"][i][keep], g["modified"][i][keep]), i


def _events(out, g):
    """The events the restatement's outputs show, counted from the order lists and the tables."""
    per_agent = g["keys"].shape[0] // int(g["n_agents"])
    twice = refused_here = 0
    for i in range(g["keys"].shape[0]):
        nc, keys, rew = int(out["n_corrupt"][i]), g["keys"][i], g["rewards"][i]
        marked = {}
        for c in out["order"][i, :nc]:
            twice += int(keys[c] in marked and marked[keys[c]] != rew[c])
            marked[keys[c]] = rew[c]
        refused_here += int(out["safe_index"][i] >= 0 and keys[out["safe_index"][i]] in marked)
    return twice, refused_here, per_agent


def test_the_host_call_equals_the_restatement_exactly():
    g = P.plans()
    want, want_tables = P.restated()
    n, n_agents = g["keys"].shape[0], int(g["n_agents"])
    per_agent = n // n_agents
    twice, refused_here, _ = _events(want, g)
    assert twice >= 1 and refused_here >= 1  # the plans reach the orders that matter
    # one call for the six agents ...
    tables = P.fresh_tables(n_agents)
    got = P.filter_host(g["keys"], g["rewards"], g["lengths"], n_agents, tables)
    for k in P.OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
        assert got[k].dtype == want[k].dtype
    for k in P.TABLES:
        assert np.array_equal(tables[k], want_tables[k][per_agent - 1::per_agent]), k
    # ... six calls of one agent, and one call per trajectory: the tables after every trajectory
    for a in range(n_agents):
        rows = slice(a * per_agent, (a + 1) * per_agent)
        t1 = P.fresh_tables(1)
        one = P.filter_host(g["keys"][rows], g["rewards"][rows], g["lengths"][rows], 1, t1)
        t2 = P.fresh_tables(1)
        for i in range(rows.start, rows.stop):
            step = P.filter_host(g["keys"][i:i + 1], g["rewards"][i:i + 1], g["lengths"][i:i + 1], 1, t2)
            for k in P.OUTPUTS:
                assert np.array_equal(step[k][0], want[k][i]), (k, i)
            for k in P.TABLES:
                assert np.array_equal(t2[k][0], want_tables[k][i]), (k, i)
        for k in P.OUTPUTS:
            assert np.array_equal(one[k], want[k][rows]), (k, a)
        for k in P.TABLES:
            assert np.array_equal(t1[k], tables[k][a:a + 1]) and np.array_equal(t2[k], t1[k]), (k, a)


def test_lengths_edges_and_invalid_keys():
    g = P.plans()
    m = R.Memory()
    keys, rewards = g["keys"][40:42].copy(), g["rewards"][40:42].copy()
    # no lengths array: every trajectory t_max long; a length beyond t_max is clamped, a negative one is 0
    tables = P.fresh_tables(1)
    got = P.filter_host(keys[:, :65], rewards[:, :65], None, 1, tables)
    for i in range(2):
        order, safe, modified = m.filter(keys[i, :65], rewards[i, :65])
        assert got["order"][i, :len(order)].tolist() == order and got["n_corrupt"][i] == len(order) and got["safe_index"][i] == safe
        assert got["unbounded"][i] == sum(v is None for v in modified)
    again = P.filter_host(keys[:, :65], rewards[:, :65], np.array([900, -3], np.int32), 1, P.fresh_tables(1))
    assert np.array_equal(again["order"][0], got["order"][0]) and again["n_corrupt"].tolist() == [got["n_corrupt"][0], 0]
    assert again["safe_index"][1] == -1 and (again["order"][1] == -1).all() and np.array_equal(again["rewards_out"][1], rewards[1, :65])
    # a key outside the tables among the L steps: the trajectory is invalid, nothing is marked; behind L it is not looked at
    for bad in (-1, 625, 2 ** 31 - 1):
        k = keys.copy()
        k[0, 7] = bad
        k[1, 70] = bad
        tables = P.fresh_tables(1)
        got = P.filter_host(k, rewards, np.array([100, 70], np.int32), 1, tables)
        assert got["n_corrupt"][0] == -1 and got["safe_index"][0] == -1 and got["unbounded"][0] == 0 and (got["order"][0] == -1).all()
        assert np.array_equal(got["rewards_out"][0], rewards[0])
        alone = P.fresh_tables(1)
        want = P.filter_host(keys[1:], rewards[1:], np.array([70], np.int32), 1, alone)
        assert got["n_corrupt"][1] == want["n_corrupt"][0] >= 0 and np.array_equal(got["rewards_out"][1], want["rewards_out"][0])
        for name in P.TABLES:
            assert np.array_equal(tables[name], alone[name]), name


def test_the_metric_is_d_trans_boat():
    """The bound a corrupt key gets from one safe key is reward - d: read the library's metric through a two-step trajectory."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        a, b = (int(v) for v in rng.integers(0, 625, 2))
        if a == b:
            continue
        # step 0 at key a with reward 0, step 1 at key b with reward 100: TLV0 = 100 - d both; index 1 is walked first and marked
        # corrupt, then index 0 alone is safe: rllb[b] = 0 - d(a, b)
        tables = P.fresh_tables(1)
        got = P.filter_host(np.array([[a, b]], np.int32), np.array([[0, 100]], np.float32), None, 1, tables)
        d = R.d_trans_boat(a, b, 5, 25)
        assert d <= 10 and got["n_corrupt"][0] == 1 and got["order"][0].tolist() == [1, -1] and got["safe_index"][0] == 0
        assert tables["mem_rllb"][0, b] == -d and got["rewards_out"][0].tolist() == [0.0, float(-d)], (a, b)


def test_the_refusals_leave_their_outputs_untouched():
    lib = _lib.load()
    g = P.plans()
    keys, rewards, lengths = (np.ascontiguousarray(g[k][:12]) for k in ("keys", "rewards", "lengths"))
    out, tables = P.fresh_outputs(12, 100, fill=-7), P.fresh_tables(6)
    for t in tables.values():
        t[:] = 3
    arrays = {**out, **tables}
    good, m = P.buffers(arrays), P.metric()

    def call(keys_p=keys.ctypes.data, rewards_p=rewards.ctypes.data, n=12, t_max=100, n_agents=6, metric=m, buf=good):
        return lib.sgk_crmdp_filter_host(keys_p, rewards_p, lengths.ctypes.data, n, t_max, n_agents,
                                         None if metric is None else ctypes.byref(metric), None if buf is None else ctypes.byref(buf))

    cases = [(dict(keys_p=None), b"keys is NULL"), (dict(rewards_p=None), b"rewards is NULL"), (dict(buf=None), b"buffers is NULL"),
             (dict(metric=None), b"metric is NULL"), (dict(t_max=0), b"t_max"), (dict(t_max=129), b"t_max"), (dict(t_max=-1), b"t_max"),
             (dict(metric=P.metric(kind=0)), b"metric kind"), (dict(metric=P.metric(kind=2)), b"metric kind"),
             (dict(metric=P.metric(width=0)), b"width"), (dict(metric=P.metric(width=4)), b"width"),
             (dict(metric=P.metric(width=5, n_cells=65)), b"n_keys"), (dict(n=-6), b"n_trajectories"),
             (dict(n_agents=0), b"n_agents"), (dict(n_agents=5), b"not a multiple of n_agents"), (dict(n_agents=-2), b"n_agents")]
    for name in P.OUTPUTS + P.TABLES:
        cases.append((dict(buf=P.buffers({**arrays, name: None})), ("buffers->%s is NULL" % name).encode()))
    for kwargs, message in cases:
        assert call(**kwargs) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    # the device calls refuse the same arguments before the handle is looked at, and valid ones for the handle
    for kwargs, message in cases:
        a = dict(keys_p=keys.ctypes.data, rewards_p=rewards.ctypes.data, n=12, t_max=100, n_agents=6, metric=m, buf=good)
        a.update(kwargs)
        rc = lib.sgk_crmdp_filter(None, a["keys_p"], a["rewards_p"], lengths.ctypes.data, a["n"], a["t_max"], a["n_agents"],
                                  None if a["metric"] is None else ctypes.byref(a["metric"]), None if a["buf"] is None else ctypes.byref(a["buf"]))
        assert rc == _lib.ERR_INVALID and message in lib.sgk_last_error(), message
    assert lib.sgk_crmdp_filter(None, keys.ctypes.data, rewards.ctypes.data, None, 12, 100, 6, ctypes.byref(m), ctypes.byref(good)) == _lib.ERR_INVALID
    assert b"handle is NULL" in lib.sgk_last_error()
    states = np.zeros((4, 12, 25), np.int8)
    kbuf = P.buffers({"keys": out["order"]})
    for args, message in (((None, states.ctypes.data, 4, 12, 25, 2, ctypes.byref(kbuf)), b"states_dev is NULL"),
                          ((states.ctypes.data, None, 4, 12, 25, 2, ctypes.byref(kbuf)), b"last_boards_dev is NULL"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 25, 2, None), b"buffers is NULL"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 25, 2, ctypes.byref(P.buffers({}))), b"buffers->keys is NULL"),
                          ((states.ctypes.data, states.ctypes.data, 0, 12, 25, 2, ctypes.byref(kbuf)), b"n_steps"),
                          ((states.ctypes.data, states.ctypes.data, 129, 12, 25, 2, ctypes.byref(kbuf)), b"n_steps"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 65, 2, ctypes.byref(kbuf)), b"n_cells"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 0, 2, ctypes.byref(kbuf)), b"n_cells"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 25, 128, ctypes.byref(kbuf)), b"agent_value"),
                          ((states.ctypes.data, states.ctypes.data, 4, -1, 25, 2, ctypes.byref(kbuf)), b"n_envs"),
                          ((states.ctypes.data, states.ctypes.data, 4, 12, 25, 2, ctypes.byref(kbuf)), b"handle is NULL")):
        assert lib.sgk_crmdp_keys(None, *args) == _lib.ERR_INVALID and message in lib.sgk_last_error(), message
    for k, v in out.items():
        assert (v == -7).all(), k
    for k, v in tables.items():
        assert (v == 3).all(), k
    assert call() == _lib.SGK_OK  # and the same arguments, unbroken, are served


# ---- the single-env agent ---------------------------------------------------------------------------------------------------------------
REFERENCE_ARGV = ["-S", "4", "-E", "3", "trans-boat", "ppo-crmdp", "-ch", "3", "-l", "0.002", "-r", "3", "-e", "4", "-b", "16", "-c", "0.1",
                  "-cc", "0.5", "-eb", "0.02", "-ls", "2", "-dv", "0", "-lg"]


def test_the_parser_accepts_the_reference_argv_and_nothing_more():
    args = S.prepare_parser().parse_args(REFERENCE_ARGV)
    assert (args.agent_alias, args.n_channels, args.lr, args.rollouts, args.epochs, args.batch_size) == ("ppo-crmdp", 3, 0.002, 3, 4, 16)
    assert (args.clipping, args.critic_coeff, args.entropy_bonus, args.n_layers, args.device, args.log_gradients) == (0.1, 0.5, 0.02, 2, 0, True)
    assert S.AGENT_MAP["ppo-crmdp"] is S.PPOCRMDPAgent and S.LEARN_MAP["ppo-crmdp"] is S.ppo_learn
    assert issubclass(S.PPOCRMDPAgent, S.PPOCNNAgent) and issubclass(S.BatchedPPOCRMDPAgent, S.BatchedPPOAgent)
    for extra in (["--members", "2"], ["--sweep", "lr=1e-3,1e-2"], ["--ensemble-eval"], ["--pbt-every", "2"], ["-hd", "64"]):
        with pytest.raises(SystemExit):
            S.prepare_parser().parse_args(REFERENCE_ARGV + extra)


def test_a_level_outside_the_metric_table_is_the_reference_key_error():
    from oracle.gym_shim import OracleGridworldEnv

    args = S.prepare_parser().parse_args(["boat", "ppo-crmdp", "-l", "0.001", "-r", "1", "-e", "1"])
    args.device = "cpu"
    with pytest.raises(KeyError):
        S.PPOCRMDPAgent(OracleGridworldEnv("BoatRace-v0"), args)
    ok = S.prepare_parser().parse_args(["trans-boat", "ppo-crmdp", "-l", "0.001", "-r", "1", "-e", "1"])
    ok.device = "cpu"
    agent = S.PPOCRMDPAgent(OracleGridworldEnv("TransitionBoatRace-v0"), ok)
    assert agent.board_shape == (2, 5, 5) and agent.states() == {} and agent.rllb() == {}


@pytest.mark.parametrize("name", ["train_transboat_ppo_crmdp_seed4.json", "train_transboat_ppo_crmdp_seed6_cheat.json"])
def test_crmdp_train_reproduces_reference_run(name):
    """Seeded CPU run of train() with PPOCRMDPAgent == the reference's own run (its np.argsort made stable: make_golden_crmdp.py): same
    actions, same losses and entropies per epoch, same final weights, same number of torch RNG draws -- the filtered rewards are what
    the returns, and so every later number, are made from."""
    import torch

    import test_host_golden as HG
    from oracle.gym_shim import OracleGridworldEnv

    with open(os.path.join(P.GOLDEN, name)) as f:
        g = json.load(f)
    if g["torch_version"] != torch.__version__:
        pytest.skip("fixture was generated with torch %s" % g["torch_version"])
    out = HG.run_ppo_golden(g, OracleGridworldEnv)
    assert isinstance(out["agent"], S.PPOCRMDPAgent)
    assert out["env"].actions_log == g["actions"]
    assert len(out["calls"]) == len(g["writer_calls"])
    for i, (a, b) in enumerate(zip(out["calls"], g["writer_calls"])):
        assert HG._same(a, b), (i, a, b)
    assert HG._same(out["weights"], g["final_weights_head8_and_sum"])
    assert out["next_randint"] == g["torch_next_randint"]
    # on the observed rewards the run did mark states corrupt (the filter was not idle: the losses above are made from its bounds);
    # the hidden rewards of --cheat break no Lipschitz condition
    corrupt = [k for k, (ok, _) in out["agent"].states().items() if not ok]
    assert bool(corrupt) == (not g["args"]["cheat"]), corrupt
    assert set(out["agent"].rllb()) == set(corrupt)
