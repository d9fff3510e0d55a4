"""What N private tabular-Q agents recommend TOGETHER: a plurality vote per state, on the device.

BatchedTabularQAgent trains up to a quarter of a million seeds of the reference's `tabular-q` in one launch; each of them can be
evaluated alone, in its own env. Here the runs are asked as one (include/sgk.h, csrc/sgk_tabq_consensus.hip):

  sgk_tabq_consensus    one streaming read of the tables [n_states][N][4]: agent e votes in state s iff it may (the mask) and its
                        row of s holds anything but zeros (a row it never learnt is the reference's fresh defaultdict row: its argmax
                        of 0 is no opinion); its vote is its greedy action (the first maximum, np.argmax's rule). votes int64 [S, 4],
                        voters int64 [S] -- integers, so the result is exact whatever the grid and the order of the atomics
  sgk_tabq_load_shared  the mirror: every agent's table := one [S, 4] table, one streaming write

ConsensusMixin gives BatchedTabularQAgent consensus() (the counts, the plurality policy, the agreement), load_shared_table(),
consensus_agent() (a fresh env + agent of the same level whose every table is the vote counts as float64: the argmax of the counts
under the first-max rule IS the plurality vote with np.argmax's tie rule, and a state without voters reads as a zero row) and
evaluate_consensus() (the consensus agent through the existing fused evaluation, sgk_tabq_eval). The source agent is only read: its
tables, step counter and epsilon stay as they were, and the consensus agent acts on an env handle of its own.

On TomatoWatering every agent keeps a HASH table of its own, so the rows do not line up by slot; they line up by board key
(csrc/sgk_tabq_hash_consensus.hip):

  sgk_tabq_hash_consensus    the same vote per board key: a 2^22-bit presence bitmap + prefix popcount rank the voted keys, the output
                             is the U voted keys ascending with their counts and U itself on the device
  sgk_tabq_hash_load_shared  the mirror: the selected agents' tables := the one table a sequential insertion of (key, row) pairs leaves

hash_consensus() / load_shared_hash_table() / hash_consensus_agent() / evaluate_hash_consensus() are the four methods again under new
names; the old ones keep refusing the level.

This module also holds the command line's side: --consensus-eval and --hash-consensus-eval (check_consensus_eval,
check_hash_consensus_eval: SystemExit with a plain message).
"""
import ctypes

from . import _lib


class TabularConsensus:
    """The vote of one consensus() call. votes: int64 [S, 4] on the device, votes[s, a] = voting agents whose greedy action in state
    s is a; voters: int64 [S], the voting agents per state (the row sums of votes). Both are the buffers the kernel wrote: views of
    votes_out / voters_out where the caller gave them."""

    def __init__(self, votes, voters):
        self.votes = votes
        self.voters = voters

    @property
    def policy(self):
        """uint8 [S]: the first action with the most votes (np.argmax's tie rule), 0 where nobody voted."""
        import torch

        votes = self.votes
        top = votes.max(dim=1, keepdim=True).values
        index = torch.arange(4, device=votes.device, dtype=torch.int64).expand_as(votes)
        return torch.where(votes == top, index, torch.full_like(index, 4)).min(dim=1).values.to(torch.uint8)

    def agreement(self):
        """sum over states of the winning action's votes / sum over states of the voters, a Python float from the two exact integers
        (synchronises); 0.0 when nobody voted anywhere."""
        won, cast = int(self.votes.max(dim=1).values.sum().item()), int(self.voters.sum().item())
        return won / cast if cast else 0.0


class ConsensusMixin:
    """consensus() / load_shared_table() / consensus_agent() / evaluate_consensus() for BatchedTabularQAgent (`env`, `lib`, `_h`,
    `n_states`, `args`)."""

    _consensus_cache = None  # n_envs -> {"agent", "votes", "voters", "table"}: evaluate_consensus()'s agent and buffers, made once

    def _consensus_level(self):
        if self.env.info.env_id == _lib.TOMATO_WATERING:
            raise ValueError("%s keeps a private hash table per agent: an agent's slots are its own, so the agents' rows do not line up "
                             "by state and there is nothing to vote on" % self.env.name)

    def consensus(self, mask=None, votes_out=None, voters_out=None):
        """The agents' vote on every state (sgk_tabq_consensus: one launch, or three where several workgroups share a state; no host
        synchronisation) -> TabularConsensus. mask: uint8 or bool [N] on the env's device, agent e may vote iff mask[e] != 0 (default:
        everyone); votes_out int64 [S, 4], voters_out int64 [S]: buffers to write (overwritten, not accumulated), made here when None.
        ValueError for a tensor of the wrong device, dtype or shape and for a level with hashed tables."""
        import torch

        self._consensus_level()
        env, S = self.env, self.n_states
        if mask is not None:
            mask = env._check(mask, "mask", shape=(env.n_envs,), dtypes=("uint8", "bool"))
        dev = "cuda:%d" % env.device
        votes = torch.empty((S, 4), dtype=torch.int64, device=dev) if votes_out is None else \
            env._check(votes_out, "votes_out", shape=(S, 4), dtypes=("int64",))
        voters = torch.empty(S, dtype=torch.int64, device=dev) if voters_out is None else \
            env._check(voters_out, "voters_out", shape=(S,), dtypes=("int64",))
        env._sync_torch_to_lib()
        _lib.check(self.lib.sgk_tabq_consensus(self._h, None if mask is None else ctypes.c_void_p(mask.data_ptr()),
                                               ctypes.c_void_p(votes.data_ptr()), ctypes.c_void_p(voters.data_ptr())))
        env._sync_lib_to_torch()
        return TabularConsensus(votes, voters)

    def load_shared_table(self, table):
        """Every agent's table := `table`, float64 [S, 4] on the env's device (sgk_tabq_load_shared: one launch, no host
        synchronisation); the rows the per-step kernels keep are forgotten. The step counter and epsilon stay."""
        self._consensus_level()
        env = self.env
        table = env._check(table, "table", shape=(self.n_states, 4), dtypes=("float64",))
        env._sync_torch_to_lib()
        _lib.check(self.lib.sgk_tabq_load_shared(self._h, ctypes.c_void_p(table.data_ptr())))
        env._sync_lib_to_torch()

    def _fresh_twin(self, n_envs, seed=None):
        """A fresh env of the same level (n_envs envs, the default layout, the source env's device, env_index_base and -- unless given --
        seed) and a fresh agent with the same args on it."""
        from .envs import BatchedGridworldEnv

        src = self.env
        n = min(src.n_envs, 1024) if n_envs is None else int(n_envs)
        if n < 1:
            raise ValueError("n_envs must be >= 1, not %d" % n)
        env = BatchedGridworldEnv(src.name, n, device=src.device, seed=int(src.info.seed) if seed is None else int(seed),
                                  env_index_base=int(src.info.env_index_base))
        try:
            return type(self)(env, self.args)
        except Exception:
            env.close()
            raise

    def consensus_agent(self, n_envs=None, mask=None, seed=None):
        """A fresh BatchedTabularQAgent (same args) on a fresh env of the same level -- n_envs envs (default min(N, 1024)), the default
        layout, the source env's device, env_index_base and (unless `seed` is given) seed -- whose every table is this agent's vote
        counts as float64: its greedy action in a state is the plurality vote there. The caller closes it and its env. This agent
        is only read."""
        import torch

        self._consensus_level()
        votes = self.consensus(mask=mask).votes
        agent = self._fresh_twin(n_envs, seed)
        agent.load_shared_table(votes.to(torch.float64))
        return agent

    def evaluate_consensus(self, eval_timesteps, n_envs=None, mask=None):
        """The consensus agent through evaluate() (default_eval in one launch, sgk_tabq_eval) -> (BatchMetrics, {"agreement": the
        vote's agreement(), "voted_states": states with at least one voter, "voters": votes cast, summed over the states}). The
        consensus agent and the buffers are made once per n_envs (default min(N, 1024)) and kept until close(); later calls only vote
        again and load again."""
        import torch

        self._consensus_level()
        n = min(self.env.n_envs, 1024) if n_envs is None else int(n_envs)
        if self._consensus_cache is None:
            self._consensus_cache = {}
        st = self._consensus_cache.get(n)
        if st is None:
            dev = "cuda:%d" % self.env.device
            st = self._consensus_cache[n] = {"votes": torch.empty((self.n_states, 4), dtype=torch.int64, device=dev),
                                             "voters": torch.empty(self.n_states, dtype=torch.int64, device=dev),
                                             "table": torch.empty((self.n_states, 4), dtype=torch.float64, device=dev),
                                             "agent": self._fresh_twin(n)}
        cons = self.consensus(mask=mask, votes_out=st["votes"], voters_out=st["voters"])
        st["table"].copy_(st["votes"])  # int64 -> float64, exact for any count a table can hold
        st["agent"].load_shared_table(st["table"])
        bm = st["agent"].evaluate(eval_timesteps)
        stats = {"agreement": cons.agreement(), "voted_states": int((st["voters"] > 0).sum().item()), "voters": int(st["voters"].sum().item())}
        return bm, stats

    def _close_consensus(self):
        cache, self._consensus_cache = self._consensus_cache, None
        hashed, self._hash_consensus_cache = self._hash_consensus_cache, None
        self._hash_consensus_buffers = None
        for st in list((cache or {}).values()) + list((hashed or {}).values()):
            agent = st.get("agent")
            if agent is not None:
                env = agent.env
                agent.close()
                env.close()

    # -- the hashed levels (TomatoWatering): the vote by board key ---------------------------------------------------------------------
    _hash_consensus_cache = None    # n_envs -> {"agent", "rows"}: evaluate_hash_consensus()'s twin, made once
    _hash_consensus_buffers = None  # the default outputs and the workspace of hash_consensus(), made once per capacity

    HASH_CONSENSUS_MAX_KEYS = 1 << 18

    def _hash_consensus_level(self):
        if self.env.info.env_id != _lib.TOMATO_WATERING:
            raise ValueError("%s has a perfect hash of its boards: its agents' rows line up by state and consensus() is the vote; "
                             "hash_consensus() is for the levels with a hash table per agent" % self.env.name)

    def _hash_workspace(self):
        """(uint8 workspace of the size the library asks for at the current capacity, its size): made once, again after a growth."""
        import torch

        need = int(self.lib.sgk_tabq_hash_consensus_workspace_bytes(self._h))
        if need < 0:
            _lib.check(need)
        st = self._hash_consensus_buffers
        if st is None:
            st = self._hash_consensus_buffers = {}
        ws = st.get("workspace")
        if ws is None or ws.numel() < need:
            ws = st["workspace"] = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % self.env.device)
        return ws, need

    def hash_consensus(self, mask=None, max_keys=None, out=None):
        """The agents' vote on every board some agent has an opinion on (sgk_tabq_hash_consensus: memsets and three launches, no host
        synchronisation) -> HashedConsensus: the voted keys ascending, their counts, and their number on the device. mask: uint8 or bool
        [N], agent e may vote iff mask[e] != 0 (default: everyone). max_keys: rows of the outputs (default min(N * capacity, 2^18));
        with fewer rows than voted keys the first max_keys keys are written and count still tells the true number. out: a
        HashedConsensus whose tensors are written again (its max_keys holds). The default outputs and the workspace are made once per
        agent and reused: a later call overwrites the result of an earlier one. ValueError on a level with a perfect hash and for a
        tensor of the wrong device, dtype or shape."""
        import torch

        self._hash_consensus_level()
        env = self.env
        if mask is not None:
            mask = env._check(mask, "mask", shape=(env.n_envs,), dtypes=("uint8", "bool"))
        dev = "cuda:%d" % env.device
        if out is not None:
            if max_keys is not None and int(max_keys) != out.max_keys:
                raise ValueError("max_keys is %d but out has %d rows" % (int(max_keys), out.max_keys))
            K = out.max_keys
            keys = env._check(out.keys, "out.keys", shape=(K,), dtypes=("int32",))
            votes = env._check(out.votes, "out.votes", shape=(K, 4), dtypes=("int64",))
            voters = env._check(out.voters, "out.voters", shape=(K,), dtypes=("int64",))
            count = env._check(out.count, "out.count", shape=(1,), dtypes=("int64",))
        else:
            K = min(env.n_envs * self.n_states, self.HASH_CONSENSUS_MAX_KEYS) if max_keys is None else int(max_keys)
            if K < 1:
                raise ValueError("max_keys must be >= 1, not %d" % K)
            ws, _ = self._hash_workspace()
            st = self._hash_consensus_buffers
            if st.get("max_keys") != K:
                st.update(max_keys=K, keys=torch.empty(K, dtype=torch.int32, device=dev), votes=torch.empty((K, 4), dtype=torch.int64, device=dev),
                          voters=torch.empty(K, dtype=torch.int64, device=dev), count=torch.empty(1, dtype=torch.int64, device=dev))
            keys, votes, voters, count = st["keys"], st["votes"], st["voters"], st["count"]
        ws, need = self._hash_workspace()
        desc = _lib.SgkTabqHashVotes(keys.data_ptr(), votes.data_ptr(), voters.data_ptr(), count.data_ptr(), K, ws.data_ptr(), need)
        env._sync_torch_to_lib()
        _lib.check(self.lib.sgk_tabq_hash_consensus(self._h, None if mask is None else ctypes.c_void_p(mask.data_ptr()), ctypes.byref(desc)))
        env._sync_lib_to_torch()
        return HashedConsensus(keys, votes, voters, count)

    def load_shared_hash_table(self, keys, rows, count=None, mask=None):
        """The selected agents' tables := the table a sequential insertion of keys[0 .. count) with the rows rows[j] leaves
        (sgk_tabq_hash_load_shared: three launches, no host synchronisation). keys: int32 [K] bit patterns as HashedConsensus.keys
        holds them; rows: float64 [K, 4]; count: int64 [1] ON THE DEVICE (default: K); mask: uint8 or bool [N] (default: everyone).
        A later duplicate key overwrites the earlier row, a key that finds the table full is dropped and raises the overflow flag, the
        selected agents forget a pending act(); the others keep every byte."""
        import torch

        self._hash_consensus_level()
        env = self.env
        if getattr(keys, "dim", lambda: 0)() != 1 or keys.shape[0] < 1:
            raise ValueError("keys must be a tensor [K] with K >= 1")
        K = int(keys.shape[0])
        keys = env._check(keys, "keys", shape=(K,), dtypes=("int32",))
        rows = env._check(rows, "rows", shape=(K, 4), dtypes=("float64",))
        if count is None:
            count = torch.full((1,), K, dtype=torch.int64, device="cuda:%d" % env.device)
        count = env._check(count, "count", shape=(1,), dtypes=("int64",))
        if mask is not None:
            mask = env._check(mask, "mask", shape=(env.n_envs,), dtypes=("uint8", "bool"))
        ws, need = self._hash_workspace()
        desc = _lib.SgkTabqHashVotes(None, None, None, None, 0, ws.data_ptr(), need)
        env._sync_torch_to_lib()
        _lib.check(self.lib.sgk_tabq_hash_load_shared(self._h, None if mask is None else ctypes.c_void_p(mask.data_ptr()),
                                                      ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(rows.data_ptr()),
                                                      ctypes.c_void_p(count.data_ptr()), K, ctypes.byref(desc)))
        env._sync_lib_to_torch()

    @staticmethod
    def _hash_capacity_for(n_keys, reserve_steps):
        """The next power of two >= n_keys + 2 * reserve_steps + 1 (reserve_hash's bound: a step claims at most two slots), >= 64."""
        return max(64, 1 << (int(n_keys) + 2 * int(reserve_steps)).bit_length())

    def _grow_twin(self, twin, n_keys, reserve_steps):
        need = self._hash_capacity_for(n_keys, reserve_steps)
        if need > twin.HASH_CAPACITY_MAX:
            raise RuntimeError("%d voted boards and %d steps need %d slots per agent, above the largest hash table of 2^24 slots"
                               % (n_keys, reserve_steps, need))
        if twin.n_states < need:
            twin.grow_hash(need)

    def hash_consensus_agent(self, n_envs=None, mask=None, seed=None, reserve_steps=0):
        """consensus_agent() for the hashed levels: a fresh agent (same args) on a fresh env of the same level, created at or grown to
        the next power of two >= U + 2 * reserve_steps + 1 slots (U voted boards; room for reserve_steps lockstep steps, in which
        greedy acting claims slots too), every table the vote counts as float64 by board key: its greedy action on a board is the
        plurality vote there, and a board nobody voted on reads as zeros. Reads U back once. The caller closes it and its env; this
        agent is only read."""
        import torch

        self._hash_consensus_level()
        cons = self.hash_consensus(mask=mask)
        n_keys = cons.n_keys()
        agent = self._fresh_twin(n_envs, seed)
        try:
            self._grow_twin(agent, n_keys, reserve_steps)
            agent.load_shared_hash_table(cons.keys, cons.votes.to(torch.float64), cons.count)
        except Exception:
            env = agent.env
            agent.close()
            env.close()
            raise
        return agent

    def evaluate_hash_consensus(self, eval_timesteps, n_envs=None, mask=None):
        """evaluate_consensus() for the hashed levels -> (BatchMetrics, {"agreement", "voted_states", "voters"}): the vote, one
        read-back of the number of voted boards, growth of the cached twin where it needs room (the boards plus two slots per step of
        the evaluation: eval_timesteps - 1 + max_iterations steps), the load, then evaluate(). Greedy acting claims slots on this
        level, so every call loads again: what an earlier evaluation claimed is gone. The twin is made once per n_envs (default
        min(N, 1024)) and kept until close()."""
        import torch

        self._hash_consensus_level()
        n = min(self.env.n_envs, 1024) if n_envs is None else int(n_envs)
        if self._hash_consensus_cache is None:
            self._hash_consensus_cache = {}
        st = self._hash_consensus_cache.get(n)
        if st is None:
            st = self._hash_consensus_cache[n] = {"agent": self._fresh_twin(n), "rows": None}
        cons = self.hash_consensus(mask=mask)
        n_keys = cons.n_keys()
        twin = st["agent"]
        self._grow_twin(twin, n_keys, max(int(eval_timesteps) - 1, 0) + int(twin.env.info.max_iterations))
        if st["rows"] is None or st["rows"].shape != cons.votes.shape:
            st["rows"] = torch.empty(cons.votes.shape, dtype=torch.float64, device=cons.votes.device)
        st["rows"].copy_(cons.votes)  # int64 -> float64, exact for any count a table can hold
        twin.load_shared_hash_table(cons.keys, st["rows"], cons.count)
        bm = twin.evaluate(eval_timesteps)
        stats = {"agreement": cons.agreement(), "voted_states": n_keys, "voters": int(cons.voters.sum().item())}
        return bm, stats


class HashedConsensus:
    """The vote of one hash_consensus() call, on the device: keys int32 [K] -- the voted boards' keys ascending, as bit patterns (-1 =
    unused: behind the last key); votes int64 [K, 4], votes[j, a] = voting agents whose greedy action on board keys[j] is a; voters
    int64 [K], the row sums; count int64 [1], the number U of voted boards -- the true number, also where it exceeds K. The tensors are
    the buffers the kernels wrote."""

    def __init__(self, keys, votes, voters, count):
        self.keys, self.votes, self.voters, self.count = keys, votes, voters, count
        self.max_keys = int(keys.shape[0])

    def n_keys(self):
        """U, read back (synchronises). RuntimeError when the outputs hold fewer rows than that."""
        n = int(self.count.item())
        if n > self.max_keys:
            raise RuntimeError("%d boards were voted on but max_keys is %d: the outputs hold the first %d keys only; vote again with "
                               "max_keys >= %d" % (n, self.max_keys, self.max_keys, n))
        return n

    policy = TabularConsensus.policy  # uint8 [K]: the first action with the most votes, 0 behind the last key

    agreement = TabularConsensus.agreement

    def as_dict(self):
        """{key: [4 counts]} on the host (synchronises)."""
        n = self.n_keys()
        keys = (self.keys[:n].cpu().numpy().astype("int64") & 0xFFFFFFFF).tolist()
        return dict(zip(keys, self.votes[:n].cpu().tolist()))


# -- the command line ---------------------------------------------------------------------------------------------------------------
def check_consensus_eval(args):
    """--consensus-eval of `args` -> True / False. SystemExit with a plain message for an agent other than tabular-q, for tomato (hashed
    tables), without a batch of more than one agent, and for more than one device (summing the votes over ranks is not built)."""
    if not getattr(args, "consensus_eval", False):
        return False
    if args.agent_alias != "tabular-q":
        raise SystemExit("--consensus-eval runs on a batch of private tabular-q agents, not %r" % (args.agent_alias,))
    if args.env_alias == "tomato":
        raise SystemExit("--consensus-eval cannot run on tomato: every agent keeps a hash table of its own, the agents' rows do not line up "
                         "by state (--hash-consensus-eval votes by board key there)")
    if int(getattr(args, "n_envs", 0) or 0) < 2:
        raise SystemExit("--consensus-eval needs -N > 1: the consensus is the vote of the batch's private agents")
    if int(getattr(args, "devices", 1) or 1) > 1:
        raise SystemExit("--consensus-eval runs on one device: summing the votes over the ranks of --devices %d is not built" % args.devices)
    return True


def check_hash_consensus_eval(args):
    """--hash-consensus-eval of `args` -> True / False. SystemExit with a plain message for an agent other than tabular-q, for a level
    other than tomato (--consensus-eval is the flag there), without a batch of more than one agent, for more than one device, and next
    to --consensus-eval."""
    if not getattr(args, "hash_consensus_eval", False):
        return False
    if args.agent_alias != "tabular-q":
        raise SystemExit("--hash-consensus-eval runs on a batch of private tabular-q agents, not %r" % (args.agent_alias,))
    if args.env_alias != "tomato":
        raise SystemExit("--hash-consensus-eval votes by board key, for tomato's hash tables: on %s the agents' rows line up by state, "
                         "use --consensus-eval" % (args.env_alias,))
    if int(getattr(args, "n_envs", 0) or 0) < 2:
        raise SystemExit("--hash-consensus-eval needs -N > 1: the consensus is the vote of the batch's private agents")
    if int(getattr(args, "devices", 1) or 1) > 1:
        raise SystemExit("--hash-consensus-eval runs on one device: summing the votes over the ranks of --devices %d is not built" % args.devices)
    return True


def write_consensus_eval(writer, bm, stats, period):
    """The three scalars of one consensus evaluation."""
    writer.add_scalar("Eval/consensus_return", bm.meter("returns")["avg"], period)
    writer.add_scalar("Eval/consensus_safety", bm.meter("safeties")["avg"], period)
    writer.add_scalar("Eval/consensus_agreement", stats["agreement"], period)
