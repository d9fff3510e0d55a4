"""The epoch-to-epoch machinery of the fused PPO-MLP learner (ppo_epochs_kernel: sgk_ppo_epochs through BatchedPPOAgent, and
sgk_ppo_epochs_members through BatchedPPOPopulation), which the one-epoch float64 tests never reach: epoch e's Adam stores (parameters,
moments, the transposed copies w1t / w2t) re-staged by epoch e + 1 behind one workgroup barrier, the rows of epoch e + 1 drawn one epoch
ahead into LDS that epoch e has just finished with, the bias corrections from step0 + epoch, and the [member][epoch] indexing of the
statistics and the rows.

(a) E epochs in one call == E calls of one epoch, bit for bit. The minibatch rows are keyed by the Adam step, so both forms draw the same
    rows and run the same code on them; between two launches every store is visible and nothing is drawn ahead. Twin agents on the same
    seeded inputs and Adam state: the 8 parameters, their first and second moments, w1t and w2t (kept by the kernel in the one call,
    re-derived by the wrapper in front of every launch in the other), the step counter, every epoch's three statistics and every
    epoch's rows, as bytes; w1t == w1.T, w2t == w2.T, everything finite, and the one call once more from the same state leaves the same
    bytes. Cases: K0 in {25, 36, 49, 63} (K0 % 4 != 0 and == 0: both ownership layouts of W1) x {64, 100} units from step 4999 on the
    caller's rows; batches 2 / 17 / 33 (padded minibatch rows in every epoch); 16 and 2 epochs from zero Adam state and step 0 (the bias
    corrections from their steepest end); the kernel's own draws on a ragged rollout (lengths 0 / 1 / 2 / 5) and on a sparse one (one
    valid candidate in 16: a third of the samples need a second Philox round), where every drawn row must also be a valid pair.
(b) the same for 3 members x 3 epochs in one launch against three launches of one epoch on a twin population: distinct member keys and
    step counters, the kernel's draws on the ragged rollout, all stacked tensors, stats [M][E][3] against E x [M][1][3], rows likewise.
(c) a float64 chain on top (learner_reference.ppo_chain64: 4 x (ppo_epoch64 + adam64) on the rows the kernel reported), against a fault
    both forms of (a) would share: per tensor err_k = max|w_4 - w64_4| / max|w64_4 - w_0| <= max(8 err_t, 4 x 2^-23 max|w_0| / max|w64_4
    - w_0|), err_t being the same chain in torch float32, and each epoch's statistics within bound(err_t).
    tests/test_learner_reference_cpu.py shows that an epoch that took its gradients at the previous epoch's parameters lies at least 10
    limits away on every trunk tensor.

Measured on an MI355X (profiles/ppo_epoch_chain/errors.log, printed by tools/learner_gradient_errors.py --chain): all 23 runs of (a) --
the 20 of its table and the three chain cases of (c) -- and all 4 of (b) were bit-identical, in every tensor, statistic and row, and so
was the one call run twice ("bit-identical: 27 of 27 runs"). (c): over the 24 tensors the worst err_k / err_t is 1.26 (w2 of Sokoban,
100 units: err_k 1.70e-7 of the tensor's movement against a limit of 1.08e-6, 0.16 of it: the largest share of all tensors); over the
36 statistics the worst err_k / err_t is 15.6 (the entropy of DistributionalShift's epoch 1: 8.9e-8 where torch-float32 happens to be
within 5.7e-9; bound()'s 16-ulp floor is for this) and the figure closest to its limit is BoatRace's policy loss of epoch 3, 1.19e-6 =
0.62 of that floor. err_t is what torch's float32 kernels give on the host's CPU: these ratios belong to the host of that run, and on
another one single err_t differ by up to 3x (Sokoban's policy loss of epoch 0: 8.5e-8 there, 2.8e-7 elsewhere). One tensor is in effect
unconstrained by (c): Sokoban's critic bias moves by 3.5e-5 in the four epochs, and the one-rounding-per-epoch floor of the limit is
5.4e-4 of that; (a) holds it. profiles/ppo_epoch_chain/mutations.log: five mutations of the kernel's epoch loop run against these tests
(all five fail them) and against the tests from before (which catch them as well, each through something coarser that it breaks).
"""
import collections
import types

import numpy as np
import pytest

import learner_reference as R
import test_gpu_learner_gradients as G

pytestmark = pytest.mark.gpu

STATS = ("policy_loss", "value_loss", "entropy")
N = R.N_ENVS
ChainRun = collections.namedtuple("ChainRun", "env hidden batch epochs step0 state rollout seed")
# state: "injected" (learner_reference.chain_state) or "zero"; rollout: "dense" (ppo_inputs, the caller's rows), "ragged", "sparse" (the
# kernel's draws)


def _runs():
    out = []

    def add(env, hidden, batch, epochs, step0=R.CHAIN_STEP0, state="injected", rollout="dense"):
        out.append(ChainRun(env + "-v0", hidden, batch, epochs, step0, state, rollout, 2500 + len(out)))

    for env in ("BoatRace", "SideEffectsSokoban", "ConveyorBelt", "DistributionalShift"):  # K0 = 25, 36, 49, 63
        for hidden in (64, 100):
            add(env, hidden, 64, 3)
    for batch in (2, 17, 33):
        add("SafeInterruptibility", 64, batch, 3)
        add("BoatRace", 100, batch, 3)
    add("SideEffectsSokoban", 100, 64, 16, step0=0, state="zero")
    add("SideEffectsSokoban", 100, 64, 2, step0=0, state="zero")
    add("DistributionalShift", 100, 64, 4, rollout="ragged")
    add("BoatRace", 64, 17, 4, rollout="ragged")
    add("SideEffectsSokoban", 64, 64, 4, rollout="sparse")
    add("BoatRace", 100, 33, 4, rollout="sparse")
    return out


RUNS = _runs()
CHAIN_RUNS = [ChainRun(c.env, c.hidden, c.batch, R.CHAIN_EPOCHS, R.CHAIN_STEP0, "injected", "dense", c.seed) for c in R.CHAIN_CASES]
MemberRun = collections.namedtuple("MemberRun", "env hidden batch seed")
MEMBER_RUNS = [MemberRun("BoatRace-v0", 64, 33, 2600), MemberRun("BoatRace-v0", 100, 33, 2601),
               MemberRun("DistributionalShift-v0", 64, 64, 2602), MemberRun("DistributionalShift-v0", 100, 64, 2603)]
MEMBERS, MEMBER_ENVS, MEMBER_EPOCHS = 3, 16, 3
MEMBER_KEYS, MEMBER_STEPS = (11, 2 ** 63 + 22, 33), (R.CHAIN_STEP0, 17, 1000)


def run_id(r):
    if isinstance(r, MemberRun):
        return "%s-h%d-b%d" % (r.env[:-3], r.hidden, r.batch)
    return "%s-h%d-b%d-e%d-step%d-%s" % (r.env[:-3], r.hidden, r.batch, r.epochs, r.step0, r.rollout)


def run_inputs(run):
    """(inputs, the caller's rows [epochs, batch] or None, the Adam state (m, v) or None) of a run."""
    case = R.PpoCase(run.env, run.hidden, run.batch, run.seed)
    if run.rollout == "dense":
        d = R.ppo_inputs(case)
        rows = R.chain_rows(case, d, run.epochs)
        first = rows[0]
    else:
        d = R.ppo_ragged_inputs(case, *((R.RAGGED_HORIZON, R.ragged_lengths(N)) if run.rollout == "ragged" else (R.SPARSE_HORIZON, R.sparse_lengths(N))))
        rows = None
        t, n = np.nonzero(np.arange(d["actions"].shape[0])[:, None] < d["lengths"][None, :])
        first = (t * N + n)[:run.batch]  # (only the scale of the injected state is taken from these rows' gradient)
    return d, rows, (R.chain_state(case, d, first) if run.state == "injected" else None)


def _bytes_differ(a, b):
    """The keys under which two results differ as bytes."""
    assert sorted(a) == sorted(b)
    bad = []
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.view(np.uint8).tobytes() != y.view(np.uint8).tobytes():
            bad.append(k)
    return bad


def run_single(run):
    """A run through twin BatchedPPOAgents: {"one": all epochs in one call, "again": the same call from the restored state, "chain": one
    call per epoch}, each {tensor name: array} with "stats" [epochs, 3] and "rows" [epochs, batch] among them; and the inputs."""
    import torch

    import safe_grid_agents_amd as S

    d, rows, state = run_inputs(run)
    E, B = run.epochs, run.batch
    envs, agents = [], []
    try:
        for _ in range(2):
            env = S.BatchedGridworldEnv(run.env, N, seed=3)
            env.bind_torch_stream()
            assert env.n_cells == R.ENV_CELLS[run.env]
            args = types.SimpleNamespace(discount=0.99, batch_size=B, rollouts=1, epochs=E, n_layers=2, n_hidden=run.hidden, n_channels=5,
                                         device=0, log_gradients=False, cheat=False, **R.PPO_HYPER)
            envs.append(env)
            agents.append(S.BatchedPPOAgent(env, args))
        dev = agents[0].device

        def put(dst, arrays):
            with torch.no_grad():
                for t, a in zip(dst, arrays):
                    t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dev))

        ro = types.SimpleNamespace(**{k: torch.as_tensor(d[k]).to(dev) for k in ("states", "actions", "returns", "lengths")})
        pick = None if rows is None else [torch.as_tensor(r).to(dev) for r in rows]

        def restore(agent):
            own, old = agent._own_tensors(), agent.net.old_policy
            l1, l2 = old.network[0][0], old.network[1][0][0]
            put([l1.weight.data, l1.bias.data, l2.weight.data, l2.bias.data, old.actor.weight.data, old.actor.bias.data], d["old"][:6])
            put(own, d["cur"])
            pl = agent._pl
            put(pl["m"], [np.zeros_like(p) for p in d["cur"]] if state is None else state[0])
            put(pl["v"], [np.zeros_like(p) for p in d["cur"]] if state is None else state[1])
            pl["step"].fill_(run.step0)
            for k in ("w1t", "w2t"):
                pl[k].fill_(float("nan"))  # (the wrapper refreshes them from the parameters in front of every launch)
            agent._stats.fill_(float("nan"))

        def snapshot(agent):
            pl = agent._pl
            out = {"step": pl["step"].cpu().numpy().copy(), "w1t": pl["w1t"].cpu().numpy().copy(), "w2t": pl["w2t"].cpu().numpy().copy()}
            for k, w, m, v in zip(R.PPO_TENSORS, agent._own_tensors(), pl["m"], pl["v"]):
                out.update({k: w.cpu().numpy().copy(), "m_" + k: m.cpu().numpy().copy(), "v_" + k: v.cpu().numpy().copy()})
            return out

        # (_learn_fused, not learn(): learn() has no rows_out argument. The twin that runs one epoch per call keeps its [E, 3]
        # statistics tensor -- _learn_fused does not look at its shape -- and the kernel writes row 0 of it in every call.)
        def call(agent, epochs, pick_e):
            used = torch.full((epochs, B), -1, dtype=torch.int64, device=dev)
            agent.epochs = epochs
            agent._learn_fused(ro, rows=pick_e, rows_out=used)
            return agent._stats.cpu().numpy()[:epochs].copy(), used.cpu().numpy().copy()

        one, chain = agents
        for agent in agents:  # the first call allocates the Adam state the runs below start from
            put(agent._own_tensors(), d["cur"])
            call(agent, agent.epochs, pick)
        out = {}
        for key in ("one", "again"):
            restore(one)
            stats, used = call(one, E, pick)
            out[key] = dict(snapshot(one), stats=stats, rows=used)
        restore(chain)
        stats, used = [], []
        for e in range(E):
            s, u = call(chain, 1, None if pick is None else [pick[e]])
            stats.append(s[0])
            used.append(u[0])
        out["chain"] = dict(snapshot(chain), stats=np.stack(stats), rows=np.stack(used))
        torch.cuda.synchronize()
        return out, d, rows
    finally:
        for env in envs:
            env.close()


def single_result(run):
    return G._once(("epoch chain", run), lambda: run_single(run))


def check_one_call(res, E, B, step0):
    """What must hold for an E-epoch call's outputs by themselves: finite, the step counter, the transposed copies."""
    for k, a in res.items():
        assert np.isfinite(a).all(), k
    assert res["step"].tolist() == [step0 + E] * res["step"].size
    assert res["stats"].shape[-2:] == (E, 3) and res["rows"].shape[-2:] == (E, B)
    assert (res["w1t"] == np.swapaxes(res["w1"], -1, -2)).all() and (res["w2t"] == np.swapaxes(res["w2"], -1, -2)).all()


def check_drawn_rows(rows, lengths, n_total, first=0, count=None, sparse=False):
    """rows [E, B] drawn by the kernel: each a valid (t, trajectory) pair of the member's trajectories first .. first + count - 1,
    consecutive epochs on different row sets, and on the sparse rollout more than one trajectory."""
    t, col = rows // n_total, rows % n_total
    count = n_total if count is None else count
    assert (rows >= 0).all() and ((col >= first) & (col < first + count)).all()
    assert (t < lengths[col]).all(), (t, col, lengths[col])
    for e in range(1, len(rows)):
        assert sorted(rows[e].tolist()) != sorted(rows[e - 1].tolist()), e
    if sparse:
        assert len(set(col.ravel().tolist())) > 1


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS + CHAIN_RUNS, ids=run_id)
def test_epochs_in_one_call_equal_calls_of_one_epoch_bit_for_bit(run):
    out, d, rows = single_result(run)
    check_one_call(out["one"], run.epochs, run.batch, run.step0)
    check_one_call(out["chain"], run.epochs, run.batch, run.step0)
    if rows is not None:
        assert (out["one"]["rows"] == rows).all()  # every pair of the dense rollout is valid: the index is the flat row
    else:
        check_drawn_rows(out["one"]["rows"], d["lengths"], N, sparse=run.rollout == "sparse")
    assert not np.array_equal(out["one"]["w2"], d["cur"][2]) and np.abs(out["one"]["m_w1"]).max() > 0
    assert _bytes_differ(out["one"], out["again"]) == []  # the same call from the same state
    assert _bytes_differ(out["one"], out["chain"]) == []


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
def run_members(run):
    """MEMBERS members x MEMBER_EPOCHS epochs in one launch ("one", "again") against MEMBER_EPOCHS launches of one epoch on a twin
    population ("chain"), on the ragged rollout with MEMBER_ENVS trajectories per member; every member its own weights (the seeded
    network plus seeded noise), Adam state, step counter and key."""
    import torch

    import safe_grid_agents_amd as S
    from safe_grid_agents_amd import ppo_population as PP

    M, E, B, n = MEMBERS, MEMBER_EPOCHS, run.batch, MEMBERS * MEMBER_ENVS
    case = R.PpoCase(run.env, run.hidden, run.batch, run.seed)
    d = R.ppo_ragged_inputs(case, R.RAGGED_HORIZON, R.ragged_lengths(n))
    rng = np.random.default_rng(run.seed + 77)
    noise = lambda a: (a + np.float32(0.05) * rng.standard_normal(a.shape).astype(np.float32)).astype(np.float32)  # noqa: E731
    cur = [d["cur"] if m == 0 else [noise(a) for a in d["cur"]] for m in range(M)]
    old = [d["old"] if m == 0 else [noise(a) for a in d["old"]] for m in range(M)]
    t, col = np.nonzero(np.arange(R.RAGGED_HORIZON)[:, None] < d["lengths"][None, :])
    g = R.ppo_epoch64(d["cur"], d["old"][:6], d["states"][t[:B], col[:B]], d["actions"][t[:B], col[:B]], d["returns"][col[:B], t[:B]],
                      **R._ppo_loss_kw())["grads"]  # (the scale of the injected states)
    states = [R.inject_adam_state([np.full(x.shape, np.abs(x).max()) for x in g], R.CHAIN_STATE_SEED + run.seed + m, False) for m in range(M)]
    envs, pops = [], []
    try:
        for epochs in (E, 1):
            env = S.BatchedGridworldEnv(run.env, n, seed=3)
            args = types.SimpleNamespace(discount=0.99, batch_size=B, rollouts=MEMBER_ENVS, epochs=epochs, n_layers=2, n_hidden=run.hidden,
                                         n_channels=5, device=0, log_gradients=False, cheat=False, seed=5, **R.PPO_HYPER)
            envs.append(env)
            pops.append(S.BatchedPPOPopulation(env, args, M, member_keys=MEMBER_KEYS))
        dev = pops[0].device
        ro = types.SimpleNamespace(**{k: torch.as_tensor(d[k]).to(dev) for k in ("states", "actions", "returns", "lengths")})

        def restore(pop):
            for m in range(M):
                sd = {k: torch.as_tensor(a) for k, a in zip(PP.MEMBER_KEYS, cur[m])}
                sd.update({"old_policy." + k: torch.as_tensor(a) for k, a in zip(PP.MEMBER_KEYS, old[m])})
                pop.load_member(m, sd)
                with torch.no_grad():
                    for i in range(8):
                        pop.adam_m[i][m].copy_(torch.as_tensor(np.ascontiguousarray(states[m][0][i])).to(dev))
                        pop.adam_v[i][m].copy_(torch.as_tensor(np.ascontiguousarray(states[m][1][i])).to(dev))
            pop.step.copy_(torch.as_tensor(MEMBER_STEPS, dtype=torch.int64).to(dev))
            pop.stats.fill_(float("nan"))

        # (unlike BatchedPPOAgent's wrapper, the population's does not re-derive w1t / w2t in front of a launch: the kernel alone keeps
        # them current, in both forms. A lost store of them shows in `w1t == w1.T`, not in the comparison of the two forms.)
        def call(pop):
            used = torch.full((M, pop.epochs, B), -1, dtype=torch.int64, device=dev)
            pop.learn(ro, rows_out=used)
            return pop.stats.cpu().numpy().copy(), used.cpu().numpy().copy()

        def snapshot(pop):
            return {k: v.cpu().numpy().copy() for k, v in pop.tensors().items()}

        one, chain = pops
        out = {}
        for key in ("one", "again"):
            restore(one)
            stats, used = call(one)
            out[key] = dict(snapshot(one), stats=stats, rows=used)
        restore(chain)
        parts = [call(chain) for _ in range(E)]
        out["chain"] = dict(snapshot(chain), stats=np.concatenate([p[0] for p in parts], axis=1), rows=np.concatenate([p[1] for p in parts], axis=1))
        torch.cuda.synchronize()
        return out, d, cur
    finally:
        for env in envs:
            env.close()


def members_result(run):
    return G._once(("epoch chain members", run), lambda: run_members(run))


@pytest.mark.parametrize("run", MEMBER_RUNS, ids=run_id)
def test_members_epochs_in_one_launch_equal_launches_of_one_epoch_bit_for_bit(run):
    out, d, cur = members_result(run)
    n = MEMBERS * MEMBER_ENVS
    for key in ("one", "chain"):
        res = out[key]
        for k, a in res.items():
            assert np.isfinite(a).all(), (key, k)
        assert res["step"].tolist() == [s + MEMBER_EPOCHS for s in MEMBER_STEPS]
        assert res["stats"].shape == (MEMBERS, MEMBER_EPOCHS, 3) and res["rows"].shape == (MEMBERS, MEMBER_EPOCHS, run.batch)
        assert (res["w1t"] == np.swapaxes(res["w1"], -1, -2)).all() and (res["w2t"] == np.swapaxes(res["w2"], -1, -2)).all()
    for m in range(MEMBERS):
        check_drawn_rows(out["one"]["rows"][m], d["lengths"], n, first=m * MEMBER_ENVS, count=MEMBER_ENVS)
        assert not np.array_equal(out["one"]["w2"][m], cur[m][2])  # every member did learn
        for other in range(m):  # from its own rows: the keys differ
            assert not np.array_equal(out["one"]["rows"][m] - m * MEMBER_ENVS, out["one"]["rows"][other] - other * MEMBER_ENVS)
    assert _bytes_differ(out["one"], out["again"]) == []
    assert _bytes_differ(out["one"], out["chain"]) == []


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
def chain_figures(case, res):
    """(what, err_k, limit, err_t) of a chain case: the eight tensors after the last epoch relative to their movement, and every epoch's
    three statistics."""
    d, rows, state, c64, err_t = R.chain_yardstick(case)
    figs = []
    for i, k in enumerate(R.PPO_TENSORS):
        want = c64["params"][-1][i]
        figs.append(("chain " + k, R.chain_err(res[k], want, d["cur"][i]), R.chain_limit(err_t[k], want, d["cur"][i], R.CHAIN_EPOCHS), err_t[k]))
    for e in range(R.CHAIN_EPOCHS):
        for i, k in enumerate(STATS):
            name = "%s %d" % (k, e)
            figs.append((name, R.rel_err(float(res["stats"][e, i]), c64["stats"][e][i]), R.bound(err_t[name]), err_t[name]))
    return figs


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=R.case_id)
def test_four_epochs_in_one_call_against_the_float64_chain(case):
    run = next(r for r in CHAIN_RUNS if r.seed == case.seed)
    out, d, rows = single_result(run)
    res = out["one"]
    assert (res["rows"] == R.chain_yardstick(case)[1]).all()  # the float64 chain ran on the rows the kernel reports
    check_one_call(res, R.CHAIN_EPOCHS, case.batch, R.CHAIN_STEP0)
    figs = chain_figures(case, res)
    for what, got, limit, err_t in figs:
        print("%-36s %-16s err_k %.3e  limit %.3e  err_t %.3e  err_k/err_t %.2f" % (R.case_id(case), what, got, limit, err_t, got / max(err_t, 1e-300)))
    G._check(figs)
