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

This module also holds the command line's side: --consensus-eval (check_consensus_eval: SystemExit with a plain message).
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
        for st in (cache or {}).values():
            agent = st.get("agent")
            if agent is not None:
                env = agent.env
                agent.close()
                env.close()


# -- the command line ---------------------------------------------------------------------------------------------------------------
def check_consensus_eval(args):
    """--consensus-eval of `args` -> True / False. SystemExit with a plain message for an agent other than tabular-q, for tomato (hashed
    tables), without a batch of more than one agent, and for more than one device (summing the votes over ranks is not built)."""
    if not getattr(args, "consensus_eval", False):
        return False
    if args.agent_alias != "tabular-q":
        raise SystemExit("--consensus-eval runs on a batch of private tabular-q agents, not %r" % (args.agent_alias,))
    if args.env_alias == "tomato":
        raise SystemExit("--consensus-eval cannot run on tomato: every agent keeps a hash table of its own, the agents' rows do not line up")
    if int(getattr(args, "n_envs", 0) or 0) < 2:
        raise SystemExit("--consensus-eval needs -N > 1: the consensus is the vote of the batch's private agents")
    if int(getattr(args, "devices", 1) or 1) > 1:
        raise SystemExit("--consensus-eval runs on one device: summing the votes over the ranks of --devices %d is not built" % args.devices)
    return True


def write_consensus_eval(writer, bm, stats, period):
    """The three scalars of one consensus evaluation."""
    writer.add_scalar("Eval/consensus_return", bm.meter("returns")["avg"], period)
    writer.add_scalar("Eval/consensus_safety", bm.meter("safeties")["avg"], period)
    writer.add_scalar("Eval/consensus_agreement", stats["agreement"], period)
