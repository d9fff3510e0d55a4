"""The DQN learner driven through one step from zero Adam state (A) and one from an injected state at step 4999 (B), on the seeded
inputs of tests/learner_reference.py: run_dqn_case() is what tests/test_gpu_learner_gradients.py calls in its own process, and this file
run as a script does the same for learner_reference.CHILD_CASES and writes the results to the .npz named on the command line -- the test
starts it as a fresh process with SGK_DQN_ONE_LAUNCH=1 (libsgk.so reads the variable once, when it is loaded), which puts Adam inside
dqn_sgd_kernel (the quad_ref ownership code) instead of the second launch.

    python tests/learner_child.py OUT.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import learner_reference as R  # noqa: E402

STEP_BEFORE_B = 4999
STATE_SEED = 77  # + the case's seed: the injected Adam state


def run_dqn_case(case, reset_store=False):
    """{"loss", "step_a", "m_a", "v_a", "x_a", "w_a", "step_b", "m_b", "v_b", "x_b", "w_b", "w1t", "w2t", "w3t"} (lists: one float32
    array per tensor, torch's parameter order); with reset_store also "m_r", "v_r", "x_r", "w_r", "step_r": step B once more through
    sgk_dqn_sgd_step_reset_store."""
    import torch

    import safe_grid_agents_amd as S

    d = R.dqn_inputs(case)
    env = S.BatchedGridworldEnv(case.env, R.N_ENVS, seed=3)
    env.bind_torch_stream()
    assert env.n_cells == R.ENV_CELLS[case.env] and float(env.reward_scale) == d["reward_scale"]
    args = types.SimpleNamespace(discount=R.DQN_DISCOUNT, lr=R.DQN_LR, batch_size=case.batch, sync_every=20, epsilon=0.05, epsilon_anneal=200,
                                 n_layers=2, n_hidden=case.hidden)
    agent = S.BatchedDeepQAgent(env, args, replay_slices=R.SLICES, reference_loss_broadcast=case.broadcast)
    assert agent.fused_learn
    dev, fl, rp = agent.device, agent._fl, agent.replay
    params = list(agent.Q.parameters())
    cpu = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]  # noqa: E731

    def put(dst, arrays):
        with torch.no_grad():
            for t, a in zip(dst, arrays):
                t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dev))

    def set_state(ms, vs, xs, step):
        put(params, d["q"])
        agent._refresh_fused_weights()
        fl["w2t"].copy_(agent.Q[1][0][0].weight.data.t())
        put(fl["m"], ms)
        put(fl["v"], vs)
        put(fl["vmax"], xs)
        fl["step"].fill_(step)

    put(list(agent.target_Q.parameters()), d["t"])
    agent._refresh_target_transposes()
    for key in ("states", "successors", "actions", "rewards", "terminals"):
        getattr(rp, key).copy_(torch.as_tensor(d[key]).to(dev))
    rp.filled = R.SLICES
    rows = torch.as_tensor(d["rows"]).to(dev)
    used = torch.zeros(case.batch, dtype=torch.int64, device=dev)
    zeros = [np.zeros_like(p) for p in d["q"]]
    out = {}
    # A: from zero state
    set_state(zeros, zeros, zeros, 0)
    out["loss"] = [np.float32(agent._learn_batch_fused(rows=rows, rows_out=used).cpu().numpy()).reshape(1)]
    assert (used.cpu().numpy() == d["rows"]).all()
    out["m_a"], out["v_a"], out["x_a"], out["w_a"] = cpu(fl["m"]), cpu(fl["v"]), cpu(fl["vmax"]), cpu(params)
    out["step_a"] = [fl["step"].cpu().numpy().copy()]
    # B: the same rows from an injected state around the kernel's own clipped gradient
    g_c = [m.astype(np.float64) / R.one_minus_beta1() for m in out["m_a"]]
    state = R.inject_adam_state(g_c, STATE_SEED + case.seed, True)
    set_state(*state, STEP_BEFORE_B)
    agent._learn_batch_fused(rows=rows)
    out["m_b"], out["v_b"], out["x_b"], out["w_b"] = cpu(fl["m"]), cpu(fl["v"]), cpu(fl["vmax"]), cpu(params)
    out["step_b"] = [fl["step"].cpu().numpy().copy()]
    out["w1t"], out["w2t"], out["w3t"] = cpu([agent._fw["w1t"]]), cpu([fl["w2t"]]), cpu([agent._fw["w3t"]])
    if reset_store:  # Adam inside dqn_adam_reset_kernel; the reset's next-states store goes to a ring of its own
        set_state(*state, STEP_BEFORE_B)
        agent._learn_batch_fused(rows=rows, reset_store=(rp.states.clone(), 0, None))
        out["m_r"], out["v_r"], out["x_r"], out["w_r"] = cpu(fl["m"]), cpu(fl["v"]), cpu(fl["vmax"]), cpu(params)
        out["step_r"] = [fl["step"].cpu().numpy().copy()]
    torch.cuda.synchronize()
    env.close()
    return out


def pack(results):
    """[{key: [arrays]}] per case -> one flat dict for np.savez."""
    return {"c%d.%s.%d" % (i, k, j): a for i, out in enumerate(results) for k, arrays in out.items() for j, a in enumerate(arrays)}


def unpack(z):
    results = {}
    for name in z.files:
        i, k, j = name.split(".")
        results.setdefault(int(i[1:]), {}).setdefault(k, {})[int(j)] = z[name]
    return [{k: [v[j] for j in sorted(v)] for k, v in results[i].items()} for i in sorted(results)]


if __name__ == "__main__":
    np.savez(sys.argv[1], **pack([run_dqn_case(c) for c in R.CHILD_CASES]))
