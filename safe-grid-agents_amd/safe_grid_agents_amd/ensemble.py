"""A population acting as ONE agent: every member votes on every env.

The populations are block-diagonal everywhere else -- member m acts in its own E = N / M envs. Here all M members look at the same N
boards and the plurality of their greedy actions is the action (the standard way to deploy seeds, sweep replicas or the survivors of
population-based training; for deep-q it is the Q-ensemble's evaluation). One lockstep step is two launches and the env's own step
(include/sgk.h):

  sgk_policy_act_members_all   the cross product: member m's greedy action on env e's board for every (m, e), uint8 [M][N]; a workgroup
                               serves one member for the whole launch and stages its weights once (ppo-mlp, deep-q: the MLP kernel)
  sgk_convq_act_members_all    the same cross product for the conv bodies (ppo-cnn): the member instantiation of the 4 x 4 x 1 MFMA
                               conv kernel, member m's row the bytes sgk_convq_act(epsilon 0) leaves for its slices
  sgk_members_vote             one lane per env counts the voters' actions; the first action with the most votes wins (np.argmax's tie
                               rule); two int64 counters gain the dissent (voters that did not vote for the winner) and the votes cast
                               over the envs whose episode is not over -- disagreement = dissent / votes, exact; body-agnostic

EnsembleMixin.ensemble_act() is one such step without the env's; evaluate_ensemble() is batched_default_eval's schedule with the ensemble
as the agent. A population supplies _ensemble_weights(): its members' greedy weights, stacked, at addresses that stay -- and, when its
forward is not the MLP kernel, _ensemble_act_all(): the acting launch (BatchedPPOCNNPopulation's is the conv one). Nothing here touches
the members' weights, optimiser state, metrics, epsilon or draw counters: greedy acting draws nothing.

This module also holds the command line's side: --ensemble-eval (check_ensemble_eval: SystemExit with a plain message). The command line
covers the MLP populations; the conv ensemble is reached through the Python API (BatchedPPOCNNPopulation.evaluate_ensemble).
"""
from . import _lib
from .metering import BatchMetrics

ENSEMBLE_AGENTS = ("ppo-mlp", "deep-q")  # the populations whose forward is the fused MLP kernel


class EnsembleMixin:
    """ensemble_act() / evaluate_ensemble() for a population with `env`, `n_members`, `device` and an _ensemble_weights() method (and,
    for a body that is not the MLP, its own _ensemble_act_all()).

    The buffers are made once per population and reused by every call and every recorded graph: member_actions uint8 [M, N], actions
    uint8 [N], ids int32 [M] (a selection's member indices in its first entries), dissent int64 [2]."""

    _ens = None

    def _ensemble_weights(self):
        raise NotImplementedError

    def _ensemble_act_all(self, weights, out):
        """The acting launch: every member's greedy action on every env, `weights` = _ensemble_weights(), into out uint8 [M, N]. The
        default is the MLP bodies' kernel; a population with another forward overrides it."""
        self.env.policy_act_members_all(weights, self.n_members, out=out)

    def _ensemble_state(self):
        import torch

        if self._ens is None:
            M, n, dev = self.n_members, self.env.n_envs, self.device
            self._ens = {"member_actions": torch.empty((M, n), dtype=torch.uint8, device=dev),
                         "actions": torch.empty(n, dtype=torch.uint8, device=dev),
                         "ids": torch.zeros(M, dtype=torch.int32, device=dev),
                         "dissent": torch.zeros(2, dtype=torch.int64, device=dev),
                         "selection": None, "graphs": {}}
        return self._ens

    def _ensemble_members(self, members):
        """None (all members vote), or int32 [k] on the device: the first k entries of the ids buffer, filled with the selection.
        ValueError for an empty selection, a duplicate and an index outside 0 .. M - 1."""
        import torch

        st = self._ensemble_state()
        if members is None:
            return None
        if isinstance(members, torch.Tensor):
            if members.dtype.is_floating_point or members.dtype.is_complex or members.dtype == torch.bool:
                raise ValueError("members has dtype %s, expected integer member indices" % members.dtype)
            members = members.reshape(-1).tolist()
        try:
            sel = tuple(int(m) for m in members)
        except (TypeError, ValueError):
            raise ValueError("members must be a sequence or an integer tensor of member indices, not %r" % (members,)) from None
        if not sel:
            raise ValueError("members selects nobody: an ensemble needs at least one voter")
        if len(set(sel)) != len(sel):
            raise ValueError("members names a member twice: %s" % (sel,))
        bad = [m for m in sel if not 0 <= m < self.n_members]
        if bad:
            raise ValueError("members names %s; the population has members 0 .. %d" % (bad, self.n_members - 1))
        if st["selection"] != sel:  # (a recorded graph reads the buffer: it follows the selection as long as its size stays)
            st["ids"][:len(sel)].copy_(torch.tensor(sel, dtype=torch.int32))
            st["selection"] = sel
        return st["ids"][:len(sel)]

    def ensemble_act(self, members=None, out=None, votes_out=None):
        """The ensemble's actions on the envs' CURRENT boards, uint8 [N]: every member's greedy action on every env (one launch), then
        the plurality vote per env, ties to the lowest action index (one launch). members: a sequence or integer tensor of member
        indices that vote (default: all; the acting launch still covers every member); out: uint8 [N], votes_out: uint16 [N, 4] (the
        counts per action), both on the env's device, or None. The env is not stepped."""
        st = self._ensemble_state()
        ids = self._ensemble_members(members)
        env = self.env
        self._ensemble_act_all(self._ensemble_weights(), st["member_actions"])
        return env.members_vote(st["member_actions"], members=ids, out=out, votes_out=votes_out)

    def _ensemble_step(self, weights, ids, reset_done):
        st, env = self._ens, self.env
        self._ensemble_act_all(weights, st["member_actions"])
        env.members_vote(st["member_actions"], members=ids, out=st["actions"], dissent=st["dissent"])
        env.step(st["actions"], auto_reset=False)
        if reset_done:
            env.reset_done()

    def evaluate_ensemble(self, eval_timesteps, members=None, graph=False):
        """batched_default_eval (reference eval.py:8-56) with the ensemble as the agent: metrics_reset, reset, `eval_timesteps - 1`
        lockstep steps of {act-all, vote, env.step, reset_done}, then `max_iterations` steps of {act-all, vote, env.step} in which the
        finished envs idle. No host synchronisation inside the loop. Returns (BatchMetrics of the evaluation, {"dissent": voters that
        did not vote for the winning action, "votes": votes cast, "disagreement": their ratio}), both counters summed over every step's
        envs whose episode was not over when the vote was taken. graph=True records one lockstep step of each phase and replays it
        (kept per selection size); the results are the same bytes."""
        import torch

        env = self.env
        if graph and not env._bound:
            raise ValueError("graph=True records the env's launches on torch's capture stream: the env must enqueue on torch's stream "
                             "(stream='torch' or bind_torch_stream), not on its own")
        st = self._ensemble_state()
        ids = self._ensemble_members(members)
        weights = self._ensemble_weights()
        n_reset, n_tail = max(int(eval_timesteps) - 1, 0), int(env.info.max_iterations)
        env.metrics_reset()
        env.reset()
        st["dissent"].zero_()
        if graph:
            key = (0 if ids is None else int(ids.shape[0]),) + tuple(t.data_ptr() for t in weights.values())
            graphs = st["graphs"].get(key)
            if graphs is None:
                # (eager once, without the env's step: the kernels' first-launch set-up does not belong in a recording)
                self._ensemble_act_all(weights, st["member_actions"])
                env.members_vote(st["member_actions"], members=ids, out=st["actions"])
                torch.cuda.synchronize(env.device)
                graphs = []
                for reset_done in (True, False):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._ensemble_step(weights, ids, reset_done)
                    env.account_steps(-1)  # the recorded (not executed) sgk_step bumped the host-side counters once
                    graphs.append(g)
                st["graphs"] = {key: graphs}  # (weights at other addresses or another selection size: the old recordings are dropped)
            for g, k in zip(graphs, (n_reset, n_tail)):
                for _ in range(k):
                    g.replay()
                    env.account_steps(1)
        else:
            for _ in range(n_reset):
                self._ensemble_step(weights, ids, True)
            for _ in range(n_tail):
                self._ensemble_step(weights, ids, False)
        bm = BatchMetrics(env.metrics(), env.reward_scale)
        dissent, votes = (int(v) for v in st["dissent"].cpu().tolist())
        return bm, {"dissent": dissent, "votes": votes, "disagreement": dissent / votes if votes else 0.0}


# -- the command line ---------------------------------------------------------------------------------------------------------------
def check_ensemble_eval(args):
    """--ensemble-eval of `args` -> True / False. SystemExit with a plain message without --members and for an agent whose population
    is not in ENSEMBLE_AGENTS (ppo-cnn: its ensemble is a Python-API feature, BatchedPPOCNNPopulation.evaluate_ensemble)."""
    if not getattr(args, "ensemble_eval", False):
        return False
    if args.agent_alias not in ENSEMBLE_AGENTS:
        raise SystemExit("--ensemble-eval runs on a population of %s agents, not %r" % (" or ".join(ENSEMBLE_AGENTS), args.agent_alias))
    if not int(getattr(args, "members", 0) or 0):
        raise SystemExit("--ensemble-eval needs --members M: the ensemble is the population's members voting on every env")
    return True


def write_ensemble_eval(writer, bm, dissent, period):
    """The three scalars of one ensemble evaluation."""
    writer.add_scalar("Eval/ensemble_return", bm.meter("returns")["avg"], period)
    writer.add_scalar("Eval/ensemble_safety", bm.meter("safeties")["avg"], period)
    writer.add_scalar("Eval/ensemble_disagreement", dissent["disagreement"], period)
