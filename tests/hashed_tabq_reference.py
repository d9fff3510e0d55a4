"""The reference's defaultdict tabular-Q agent with ONE added rule, a capacity -- helper of test_hashed_tabq_reference_cpu.py and
test_gpu_hashed_tabq.py. CPU only: the oracle's envs and draws, plain Python floats (float64, no fused multiply-add). It never
evaluates the product's hash function: a table here is a dictionary in admission order.

The rule. An agent admits boards in the order it first looks them up: a step looks up s (act(), or learn() when the step
explores -- either way before s'), then learn() looks up s'. Once `capacity` distinct boards are admitted a new board gets no
row: it reads [0, 0, 0, 0] (greedy action 0, successor value 0.0), a learn step whose state has no row changes nothing, and the
overflow flag is raised and stays.

The device's order around an episode boundary. The reference trainer looks the next episode's start board up at the next step's
act(); the fused device calls (sgk_tabq_step, sgk_tabq_learn_steps, sgk_tabq_rollout) look it up in the step that ended the
episode, behind s' (include/sgk.h). No lookup lies between the two moments, so the admission ORDER is the same and the tables
differ only when a run stops exactly on the boundary AND the start board is new to the agent -- which it is not for an agent
created with its env (it looked that board up at step 0). `claim_start_on_reset` models either order; `run(pre_steps=1)` creates
the agents one env step into the episode, which is where the two can be told apart."""
import numpy as np

from oracle import oracle as O

NAME = "TomatoWatering-v0"
# the inputs the capacity tests share (tests/test_hashed_tabq_reference_cpu.py asserts what they must provide)
N, SEED, T = 322, 5, 99
ARGS = dict(lr=0.4, discount=0.95, epsilon=0.3, epsilon_anneal=400)


def argmax4(q):
    best = 0
    for k in range(1, 4):
        if q[k] > q[best]:
            best = k
    return best


class CappedTabQ:
    """One agent: rows {board bytes: [4 floats]} in admission order (dicts keep it), at most `capacity` of them."""

    def __init__(self, lr, discount, capacity):
        self.lr, self.discount, self.capacity = float(lr), float(discount), int(capacity)
        self.rows = {}
        self.overflowed = False
        self.refused = 0  # lookups that found the table full

    def lookup(self, board):
        """The row of `board`, admitting it when there is room; None when there is none."""
        key = board.tobytes()
        row = self.rows.get(key)
        if row is None:
            if len(self.rows) >= self.capacity:
                self.overflowed = True
                self.refused += 1
                return None
            row = self.rows[key] = [0.0, 0.0, 0.0, 0.0]
        return row

    def act(self, board):
        row = self.lookup(board)
        return 0 if row is None else argmax4(row)

    def learn(self, state, action, reward, successor):
        """value.py:44-52 in the oracle's order of operations (oracle/sgk_oracle.c: orc_tabq_learn)."""
        qs = self.lookup(state)
        qn = self.lookup(successor)
        if qs is None:
            return
        value_next = 0.0 if qn is None else qn[argmax4(qn)]
        target = reward + self.discount * value_next
        differential = target - qs[action]
        qs[action] += self.lr * differential

    @property
    def n_rows(self):
        return len(self.rows)

    def boards(self):
        return list(self.rows)


def new_agents(n, capacity, args=ARGS):
    return [CappedTabQ(args["lr"], args["discount"], capacity) for _ in range(n)]


def rollout(envs, agents, n_steps, seed, env_begin=0, t_begin=0, args=ARGS, claim_start_on_reset=False):
    """The lockstep loop of learn.py:61-85 inside train.py:62-70 (oracle/sgk_oracle.c: orc_tabq_rollout), restated: returns the
    actions uint8 [n_steps, n]. Every agent is at global step `t_begin` on entry."""
    scale = O.reward_scale(envs.env_id)
    acts = np.zeros((n_steps, envs.n), dtype=np.uint8)
    for i, agent in enumerate(agents):
        for k in range(n_steps):
            t = t_begin + k
            s = envs.board(i).ravel().copy()
            u, explore_action = O.explore_draw(seed, env_begin + i, t)
            greedy = agent.act(s)  # (the device looks s up whether the step explores or not; learn() would look it up first anyway)
            action = explore_action if u < O.epsilon(args["epsilon"], args["epsilon_anneal"], t) else greedy
            r, _, done, _ = envs.step(i, action)
            agent.learn(s, action, float(r) * scale, envs.board(i).ravel().copy())
            acts[k, i] = action
            if done:
                envs.reset(i)
                if claim_start_on_reset:
                    agent.lookup(envs.board(i).ravel().copy())
    return acts


def evaluate(envs, agents, n_reset_steps, n_tail_steps):
    """default_eval (eval.py:8-56) as sgk_tabq_eval states it: every env reset, then lockstep steps of {greedy act on the board
    the env shows -- an env that is over included --, env.step, reset of what is over (the first n_reset_steps only)}. Tables are
    read, never learnt; a board that is new to an agent is admitted (a row of zeros) while there is room."""
    for i, agent in enumerate(agents):
        envs.reset(i)
        for k in range(n_reset_steps + n_tail_steps):
            envs.step(i, agent.act(envs.board(i).ravel().copy()))
            if k < n_reset_steps and O.lib().orc_game_over(envs.ptr(i)):
                envs.reset(i)


def classes(agents):
    """(below capacity, exactly full and never refused, overflowed) agent indices."""
    below = [i for i, a in enumerate(agents) if a.n_rows < a.capacity]
    full = [i for i, a in enumerate(agents) if a.n_rows == a.capacity and not a.overflowed]
    over = [i for i, a in enumerate(agents) if a.overflowed]
    assert len(below) + len(full) + len(over) == len(agents)
    return below, full, over


def hash_info(agents):
    """What sgk_tabq_hash_info must answer: (capacity, slots of the fullest agent, some lookup found its table full)."""
    return agents[0].capacity, max(a.n_rows for a in agents), any(a.overflowed for a in agents)


_RUNS = {}


def pre_actions(n):
    """The one step the boundary cases' envs take BEFORE their agents exist: env i plays action i % 4."""
    return (np.arange(n) % 4).astype(np.uint8)


def run(capacity, n_steps=T, claim_start_on_reset=False, n=N, seed=SEED, pre_steps=0):
    """(envs, agents, actions) behind `n_steps` lockstep steps from creation -- cached: the GPU tests share one per case and leave
    it unchanged. pre_steps = 1: the envs take the step of `pre_actions` first and the agents are created behind it, so that no
    agent has looked the episode's start board up when the episode ends (agent step 99) and the next one starts on it."""
    ck = (capacity, n_steps, claim_start_on_reset, n, seed, pre_steps)
    if ck not in _RUNS:
        envs = O.EnvBatch(NAME, n, seed=seed, env_begin=0)
        assert pre_steps in (0, 1)
        if pre_steps:
            for i, a in enumerate(pre_actions(n)):
                envs.step(i, int(a))
        agents = new_agents(n, capacity)
        acts = rollout(envs, agents, n_steps, seed, claim_start_on_reset=claim_start_on_reset)
        _RUNS[ck] = (envs, agents, acts)
    return _RUNS[ck]


def run_then_evaluate(capacity, train_steps, n_reset_steps=0, n_tail_steps=100, n=N, seed=SEED):
    """(envs, agents as trained, agents behind the evaluation) -- cached, of its own envs."""
    import copy

    ck = ("eval", capacity, train_steps, n_reset_steps, n_tail_steps, n, seed)
    if ck not in _RUNS:
        envs = O.EnvBatch(NAME, n, seed=seed, env_begin=0)
        agents = new_agents(n, capacity)
        rollout(envs, agents, train_steps, seed)
        trained = copy.deepcopy(agents)
        evaluate(envs, agents, n_reset_steps, n_tail_steps)
        _RUNS[ck] = (envs, trained, agents)
    return _RUNS[ck]
