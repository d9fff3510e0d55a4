"""One fused greedy evaluation (sgk_tabq_eval) of a trained batch, for a kernel trace:
    SGK_NO_BUILD=1 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/prof_tabq_eval.py ENV N KERNEL
KERNEL: auto | lds | hbm. The trace then holds one tabq_eval_kernel / tabq_eval_hbm_kernel launch next to the training rollout's."""
import os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-grid-agents_amd")):
    sys.path.insert(0, p)
import safe_grid_agents_amd as S

name, n, kernel = sys.argv[1], int(sys.argv[2]), sys.argv[3]
env = S.BatchedGridworldEnv(name, n, seed=0x5AFE)
agent = S.BatchedTabularQAgent(env, types.SimpleNamespace(lr=0.5, discount=0.99, epsilon=0.01, epsilon_anneal=100000))
agent.rollout(3000)
bm = agent.evaluate(2000, kernel=kernel)
print(name, n, kernel, "episodes", bm.episodes, "steps", bm.steps, flush=True)
agent.close(); env.close()
