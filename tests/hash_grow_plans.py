"""Growth plans for the hashed Q-tables of TomatoWatering -- helper of test_hash_grow_cpu.py and test_gpu_hash_grow.py. CPU only.

A plan is a list of legs (capacity, steps): the dictionary restatement (tests/hashed_tabq_reference.py, used as it is: 322 agents,
seed 5, its ARGS) runs `steps` lockstep steps at `capacity`, then the next leg continues the SAME run at a larger capacity --
CappedTabQ.capacity is a plain attribute, so the dictionary "grows" by assignment, rows, admission order and the sticky overflow flag
intact. What a leg leaves (actions, a copy of every agent, the envs' state) is kept per leg and shared by the tests, which leave it
unchanged. The dictionary never evaluates the product's hash function.

board_key() is the one bridge to the product: the key (include/sgk.h: agent cell | shown watered set << 8, 0x2000 = the bucket's
delusion board) of a board of the dictionary, found by rendering candidates from the product's level tables until one IS the board."""
import copy

import numpy as np

import hashed_tabq_reference as HR
import hostlib
import test_tables_cpu as TT

EMPTY = 0xFFFFFFFF
PLANS = {
    "A": [(64, 99), (128, 60)],
    "B": [(64, 99), (128, 141)],
    "C": [(64, 50), (128, 50), (512, 100)],
    "D": [(64, 30), (256, 120)],
}


class Snapshot:
    """What test_gpu_parity.assert_same_state reads of an oracle EnvBatch, frozen at the end of a leg."""

    FIELDS = ("episode_return", "hidden_return", "frame", "game_over", "agent_cell", "box_cell", "n_episodes", "last_episode_return")

    def __init__(self, envs):
        self._boards = envs.boards().copy()
        self._fields = {k: np.array(envs.field(k)).copy() for k in self.FIELDS}
        self._perf = [envs.last_performance(i) for i in range(envs.n)]

    def boards(self):
        return self._boards

    def field(self, name):
        return self._fields[name]

    def last_performance(self, i):
        return self._perf[i]


class Leg:
    def __init__(self, capacity, steps, t_end, acts, agents, refused_in_leg, snapshot):
        self.capacity, self.steps, self.t_end, self.acts = capacity, steps, t_end, acts
        self.agents = agents  # deep copies: the dictionaries as this leg left them
        self.refused_in_leg = refused_in_leg  # per agent: lookups this leg refused
        self.snapshot = snapshot

    def classes(self):
        """(below capacity, exactly full and never refused IN THIS LEG, refused in this leg) agent indices."""
        below, full, over = [], [], []
        for i, a in enumerate(self.agents):
            if self.refused_in_leg[i]:
                over.append(i)
            elif a.n_rows == self.capacity:
                full.append(i)
            else:
                below.append(i)
        return below, full, over

    def fullest(self):
        return max(a.n_rows for a in self.agents)


_PLANS = {}


def run_plan(legs, claim_start_on_reset):
    """[Leg, ...] of the plan `legs` = [(capacity, steps), ...] -- cached. claim_start_on_reset: the fused device calls' order around
    an episode boundary (True) or the per-step calls' (False): hashed_tabq_reference.py has the difference."""
    legs = tuple(tuple(l) for l in legs)
    ck = (legs, bool(claim_start_on_reset))
    if ck not in _PLANS:
        envs = HR.O.EnvBatch(HR.NAME, HR.N, seed=HR.SEED, env_begin=0)
        agents = HR.new_agents(HR.N, legs[0][0])
        out, t = [], 0
        for capacity, steps in legs:
            for a in agents:
                assert capacity >= a.capacity
                a.capacity = capacity
            before = [a.refused for a in agents]
            acts = HR.rollout(envs, agents, steps, HR.SEED, t_begin=t, claim_start_on_reset=claim_start_on_reset)
            t += steps
            out.append(Leg(capacity, steps, t, acts, copy.deepcopy(agents), [a.refused - b for a, b in zip(agents, before)],
                           Snapshot(envs)))
        _PLANS[ck] = out
    return _PLANS[ck]


def rules():
    """The product's level tables of TomatoWatering (host build)."""
    return TT._rules(hostlib.load(), HR.O.ENV_IDS[HR.NAME])


_KEYS, _BOARDS = {}, {}


def board_of_key(R, key):
    """The board a slot's key names, rendered from the product's level tables."""
    if key not in _BOARDS:
        cell, shown = key & 0xFF, key >> 8
        assert (shown == 0x2000) == (cell == R.aux_cell), hex(key)  # the delusion board shows exactly on the bucket
        ti = R.tomato_index[cell]
        assert shown == 0x2000 or ti == 255 or not (shown >> ti) & 1, hex(key)  # the tomato under the agent does not show
        _BOARDS[key] = TT._product_board(HR.NAME, R, cell, shown & 0x1FFF, 0).astype(np.int8).tobytes()
    return _BOARDS[key]


def board_key(R, board_bytes):
    """The key of a board of the dictionary: the candidate (agent cell, shown set) whose rendering is the board."""
    if board_bytes not in _KEYS:
        board = np.frombuffer(board_bytes, dtype=np.int8)
        found = []
        for cell in range(R.n_cells):
            if board[cell] != np.int8(R.agent_value[cell]):
                continue
            if cell == R.aux_cell:
                key = cell | (0x2000 << 8)
            else:
                shown = 0
                for k in range(R.n_tomatoes):
                    if k != R.tomato_index[cell] and board[R.tomato_cell[k]] == np.int8(R.value_box):
                        shown |= 1 << k
                key = cell | (shown << 8)
            if board_of_key(R, key) == board_bytes:
                found.append(key)
        assert len(found) == 1, (found, board.tolist())
        _KEYS[board_bytes] = found[0]
    return _KEYS[board_bytes]
