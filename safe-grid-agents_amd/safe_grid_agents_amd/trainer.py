"""`train(args)` and the CLI surface of the reference, for the hot-path scope.

train():            reference train.py:21-81 (seeding, object wiring, warm-up, episode loop, eval cadence).
prepare_parser():   reference parsing/parse.py:91-124 + the three YAML files, restated as a table: same
                    positional grammar `<core flags> <env alias> <agent alias> <agent flags>`, same flag names,
                    aliases and defaults (core_parser_configs.yaml:1-47, agent_parser_configs.yaml:1-63).
"""
import argparse
import random

import numpy as np

from . import envs as _envs
from .agents import AGENT_MAP
from .consensus import check_consensus_eval, check_hash_consensus_eval, write_consensus_eval
from .ensemble import check_ensemble_eval, write_ensemble_eval
from .loops import EVAL_MAP, LEARN_MAP, WARMUP_MAP
from .member_hyper import parse_sweep, point_label, sweep_member_hyper, sweep_table
from .metering import NullWriter, make_meters
from .pbt import parse_pbt

ENV_MAP = _envs.ENV_MAP

_CORE_FLAGS = [
    # (long, alias, kwargs)
    ("seed", "S", dict(type=int)),
    ("episodes", "E", dict(type=int, default=2000)),
    ("eval-timesteps", "V", dict(type=int, default=2000)),
    ("eval-every", "EE", dict(type=int, default=100)),
    ("eval-visualize-episodes", "EV", dict(type=int, default=4)),
    ("discount", "D", dict(type=float, default=0.99)),
    ("cheat", "C", dict(action="store_true")),
    ("log-dir", "L", dict(type=str)),
    ("disable-cuda", "dc", dict(action="store_true")),
    # extension: N > 0 runs N envs with N private agents in lockstep on the GPU (train_batched)
    ("n-envs", "N", dict(type=int, default=0)),
    # extension: shard the -N env batch over this many GPUs of the node, one process per GPU (contiguous env-id blocks, one
    # RCCL metrics all-reduce per reporting period). `python -m safe_grid_agents_amd --devices G ...` starts the G ranks itself;
    # under torch.distributed.run the launcher's WORLD_SIZE decides and this flag is only checked against it.
    ("devices", "G", dict(type=int, default=1)),
    # extension: with ppo-mlp or ppo-cnn, M independent agents (BatchedPPOPopulation / BatchedPPOCNNPopulation) of `--rollouts` envs each
    # in one batch of N = M x rollouts envs: M runs of the reference's experiment in lockstep on one GPU. An explicit -N must agree. With deep-q, M independent agents
    # (BatchedDeepQPopulation) of N / M envs each: the batch comes from -N, a multiple of M.
    ("members", "M", dict(type=int, default=0)),
    # extension: with --members, `--sweep NAME=v1,v2,...` (repeatable) gives the members their own hyper-parameters: the grid is the
    # Cartesian product of the lists in the order given (first flag slowest, G points), M a multiple of G, member m runs point m % G
    # as replica m // G of it (member_hyper.parse_sweep). Names: lr, clipping, critic_coeff, entropy_bonus, discount (ppo-*); lr,
    # discount, epsilon (deep-q).
    ("sweep", "W", dict(action="append", default=None, metavar="NAME=v1,v2,...")),
    # extension: with --members, `--pbt-every K` runs population-based training: after every K-th training period the worst
    # --pbt-fraction of the members (by that period's return) become copies of the best, the --pbt-perturb hyper-parameters of the
    # copies multiplied by one of the two --pbt-factors (pbt.PBTMixin.exploit_explore). A --sweep then only gives the starting values.
    ("pbt-every", "PE", dict(type=int, default=0)),
    ("pbt-fraction", "PF", dict(type=float, default=None)),
    ("pbt-factors", "PX", dict(type=str, default=None, metavar="down,up")),
    ("pbt-perturb", "PP", dict(type=str, default=None, metavar="name,name")),
    # extension: with --members on ppo-mlp or deep-q, `--ensemble-eval` follows every evaluation with one of the ENSEMBLE: all members
    # act on every env and their plurality vote is the action (ensemble.EnsembleMixin.evaluate_ensemble)
    ("ensemble-eval", "EN", dict(action="store_true")),
    # extension: with tabular-q and -N > 1 on one device, `--consensus-eval` follows every evaluation with one of the CONSENSUS agent: the
    # plurality vote, per state, of the batch's private agents (consensus.ConsensusMixin.evaluate_consensus). Absent unless given.
    ("consensus-eval", "CE", dict(action="store_true", default=argparse.SUPPRESS)),
    # extension: the same on tomato, whose agents keep a hash table each: `--hash-consensus-eval` follows every evaluation with one of the
    # agents' plurality vote per BOARD KEY (consensus.ConsensusMixin.evaluate_hash_consensus). Absent unless given.
    ("hash-consensus-eval", "HCE", dict(action="store_true", default=argparse.SUPPRESS)),
]
_LR = ("lr", "l", dict(type=float, required=True))
_EPS = ("epsilon", "e", dict(type=float, default=0.01))
_ANNEAL = ("epsilon-anneal", "dl", dict(type=int, default=100000))
_BATCH = ("batch-size", "b", dict(type=int, default=64))
_LAYERS = ("n-layers", "ls", dict(type=int, default=2))
_DEVICE = ("device", "dv", dict(type=int, default=0))
_GRADLOG = ("log-gradients", "lg", dict(action="store_true"))
_PPO_FLAGS = [_LR,
              ("rollouts", "r", dict(type=int, required=True)),
              ("epochs", "e", dict(type=int, required=True)),
              _BATCH,
              ("clipping", "c", dict(type=float, default=0.2)),
              ("critic-coeff", "cc", dict(type=float, default=1.0)),
              ("entropy-bonus", "eb", dict(type=float, default=0.01)),
              _LAYERS]
# --members is also accepted behind the agent's own flags (`... deep-q -l 1e-3 --members 32`); absent there, the core flag's value stays
_MEMBERS = ("members", "M", dict(type=int, default=argparse.SUPPRESS))
# --sweep likewise (`... ppo-mlp -l 1e-3 -r 4 -e 2 --members 6 --sweep lr=1e-3,1e-2 --sweep clipping=0.1,0.2,0.5`)
_SWEEP = ("sweep", "W", dict(action="append", default=argparse.SUPPRESS, metavar="NAME=v1,v2,..."))
# --pbt-* likewise
_PBT = [("pbt-every", "PE", dict(type=int, default=argparse.SUPPRESS)),
        ("pbt-fraction", "PF", dict(type=float, default=argparse.SUPPRESS)),
        ("pbt-factors", "PX", dict(type=str, default=argparse.SUPPRESS, metavar="down,up")),
        ("pbt-perturb", "PP", dict(type=str, default=argparse.SUPPRESS, metavar="name,name"))]
# --ensemble-eval likewise (with ppo-cnn it parses and stops the run with a message: ensemble.check_ensemble_eval)
_ENSEMBLE = ("ensemble-eval", "EN", dict(action="store_true", default=argparse.SUPPRESS))
# --consensus-eval likewise (with another agent than tabular-q it parses and stops the run with a message: consensus.check_consensus_eval)
_CONSENSUS = ("consensus-eval", "CE", dict(action="store_true", default=argparse.SUPPRESS))
# --hash-consensus-eval likewise (consensus.check_hash_consensus_eval)
_HASH_CONSENSUS = ("hash-consensus-eval", "HCE", dict(action="store_true", default=argparse.SUPPRESS))
# extension, batched trainer (-N) on tomato only: `--hash-grow` grows the agents' hash tables on the device ahead of need
# (BatchedTabularQAgent.reserve_hash before every training period and every evaluation), so that no board is ever refused and the run
# equals the reference's unbounded dictionary whatever capacity it started with. Absent unless given; another level stops the run with a
# message (check_hash_grow)
_HASH_GROW = ("hash-grow", "HG", dict(action="store_true", default=argparse.SUPPRESS))
# extension, batched trainer (-N) on trans-boat only: `--transition-policy` gives ppo-cnn / ppo-crmdp the reference's two-channel body,
# acting on [previous board, board] as TransitionBoatRace shows it (BatchedPPOAgent(transitions=True): the parity form). Absent unless
# given; another level stops the run with a message (check_transition_policy)
_TRANSITION_POLICY = ("transition-policy", "TP", dict(action="store_true", default=argparse.SUPPRESS))
# extension, beside --transition-policy: `--fused-transition-learn` makes that body's learn() the fused HIP learner
# (sgk_ppo_cnn_epochs_trans; BatchedPPOAgent(fused_transition_learn=True)) instead of the torch graph. Absent unless given; without
# --transition-policy it stops the run with a message (check_fused_transition_learn)
_FUSED_TRANSITION_LEARN = ("fused-transition-learn", "FTL", dict(action="store_true", default=argparse.SUPPRESS))
_AGENT_FLAGS = {
    "random": [],
    "single": [("action", "a", dict(type=int, default=0))],
    "tabular-q": [_LR, _EPS, _ANNEAL, _CONSENSUS, _HASH_CONSENSUS, _HASH_GROW],
    "deep-q": [_LR, _EPS, _ANNEAL,
               ("replay-capacity", "r", dict(type=int, default=10000)),
               ("sync-every", "s", dict(type=int, default=10000)),
               ("n-layers", "ls", dict(type=int, default=2)),
               ("n-hidden", "hd", dict(type=int, default=100)),
               ("batch-size", "b", dict(type=int, default=64)),
               ("device", "dv", dict(type=int, default=0)),
               ("log-gradients", "lg", dict(action="store_true")),
               # extension, batched trainer (-N) only, NOT the reference's DeepQAgent (an MLP: value.py:148-158): a convolutional
               # Q-body built like policy_cnn.py:17-81, through PyTorch-ROCm; no parity claim (BASELINE config 4 says "conv policy")
               ("q-body", "qb", dict(type=str, default="mlp", choices=("mlp", "cnn"),
                                     help="mlp: the reference's network (default, pinned); cnn: non-parity conv body, -N only")),
               ("n-channels", "ch", dict(type=int, default=5)),
               _MEMBERS, _SWEEP, _ENSEMBLE] + _PBT,
    "ppo-mlp": _PPO_FLAGS + [("n-hidden", "hd", dict(type=int, default=100)), _DEVICE, _GRADLOG, _MEMBERS, _SWEEP, _ENSEMBLE] + _PBT,
    "ppo-cnn": [("n-channels", "ch", dict(type=int, default=5))] + _PPO_FLAGS + [_DEVICE, _GRADLOG, _MEMBERS, _SWEEP, _ENSEMBLE,
                                                                         _TRANSITION_POLICY, _FUSED_TRANSITION_LEARN] + _PBT,
    # the reference's flags (agent_parser_configs.yaml:124-135) and no more: one agent, no population of it
    "ppo-crmdp": [("n-channels", "ch", dict(type=int, default=5))] + _PPO_FLAGS + [_DEVICE, _GRADLOG, _TRANSITION_POLICY, _FUSED_TRANSITION_LEARN],
}


def _add(parser, flags):
    for long, alias, kw in flags:
        parser.add_argument("-" + alias, "--" + long, **kw)


def prepare_parser():
    parser = argparse.ArgumentParser(description="Safety gridworld agents on MI355X (safe-grid-agents CLI surface)")
    _add(parser, _CORE_FLAGS)
    env_sub = parser.add_subparsers(dest="env_alias", help="gridworld environment")
    env_sub.required = True
    for env_alias in ENV_MAP:
        env_parser = env_sub.add_parser(env_alias)
        agent_sub = env_parser.add_subparsers(dest="agent_alias", help="agent")
        agent_sub.required = True
        for agent_alias, flags in _AGENT_FLAGS.items():
            _add(agent_sub.add_parser(agent_alias), flags)
    return parser


def _noop(*args, **kwargs):
    pass


def _default_writer(log_dir):
    """tensorboardX.SummaryWriter when the user has it (reference train.py:14,44); else this repo's own event-file writer
    (same calls, files TensorBoard reads); a null writer when there is no log directory."""
    try:
        from tensorboardX import SummaryWriter  # not in this image

        return SummaryWriter(log_dir)
    except ImportError:
        if not log_dir:
            return NullWriter(log_dir)
        from .eventfile import EventFileWriter

        return EventFileWriter(log_dir)


def train(args, config=None, reporter=_noop, env_factory=None, writer_factory=None):
    """One training run, exactly the reference's control flow. `env_factory(name)` defaults to the HIP-backed
    `make`; `writer_factory(log_dir)` defaults to tensorboardX when present, else a null writer."""
    import torch

    if config is not None:
        vars(args).update(config)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    env_name = ENV_MAP[args.env_alias]
    agent_class = AGENT_MAP[args.agent_alias]
    warmup_fn = WARMUP_MAP[args.agent_alias]
    learn_fn = LEARN_MAP[args.agent_alias]
    eval_fn = EVAL_MAP[args.agent_alias]

    history, eval_history = make_meters({}), make_meters({})
    writer = (writer_factory or _default_writer)(getattr(args, "log_dir", None))
    for key, value in vars(args).items():
        writer.add_text("data/{}".format(key), str(value))
    history["writer"] = eval_history["writer"] = writer

    env = (env_factory or _envs.make)(env_name)
    env.seed(args.seed)
    agent = agent_class(env, args)
    agent, env, history, args = warmup_fn(agent, env, history, args)

    history["t"], history["t_learn"] = 0, 0
    history["episode"], eval_history["period"] = 0, 0
    for _ in range(args.episodes):
        env_state = (env.reset(), 0.0, False, {"hidden_reward": 0.0, "observed_reward": 0.0})
        history["episode"] += 1
        env_state, history, eval_next = learn_fn(agent, env, env_state, history, args)
        info = env_state[3]
        reporter(hidden_reward=info["hidden_reward"], obs_reward=info["observed_reward"])
        if eval_next:
            eval_history = eval_fn(agent, env, eval_history, args)
    eval_history = eval_fn(agent, env, eval_history, args)
    return agent, history, eval_history


def train_batched(args, writer_factory=None, reporter=_noop):
    """The same experiment for `args.n_envs` independent (env, agent) pairs in lockstep, on one GPU -- or, launched by
    torch.distributed.run with one process per GPU, sharded over the GPUs of a node: rank r owns the contiguous env-id block
    dist.shard_range gives it (the counter RNG is keyed by global env id, so the trajectories do not depend on the number of
    ranks), nothing but the 16-word metrics vector crosses xGMI (one RCCL all-reduce per reporting period), rank 0 writes.
    The shared-policy agents (ppo-*) would need a gradient all-reduce and stay single-GPU.

    Keeps train()'s cadence in units of lockstep steps: one "episode" = `max_iterations` steps (every env finishes at least
    one episode in that span), an evaluation (greedy, batched_default_eval) after every `eval_every` of them and once at
    the end; metrics are the aggregate meters (BatchMetrics) written under the reference's tensorboard tags. Supports the
    agents whose learning runs on the device: tabular-q (private tables), deep-q (one shared Q-network, one SGD step per
    lockstep step), ppo-mlp / ppo-cnn (one shared policy; an "episode" is one PPO iteration = one episode per env + the
    epochs) and random."""
    import os

    from . import dist as sdist
    from .agents import BatchedTabularQAgent
    from .loops import batched_default_eval, batched_ppo_learn, population_ppo_learn
    from .ppo import BatchedPPOAgent
    from .ppo_cnn_population import BatchedPPOCNNPopulation
    from .ppo_population import BatchedPPOPopulation

    members = int(getattr(args, "members", 0) or 0)
    if members:
        members_n_envs(args)  # ppo-mlp, ppo-cnn: N = M x rollouts; deep-q: -N, a multiple of M
    sweep = sweep_grid(args)  # --sweep: (names, grid) or None; SystemExit for a sweep that cannot run
    member_hyper = sweep_member_hyper(sweep[0], sweep[1], members) if sweep else None
    pbt = parse_pbt(args)  # --pbt-every: {"every", "fraction", "factors", "perturb"} or None; SystemExit for flags that cannot run
    if pbt:
        member_hyper = member_hyper or {}  # (every member starts from args' values; the per-member tensors exist all the same)
        sweep = None  # the grid only gave the starting values: after a PBT step member m is no longer "point m % G"
    ensemble = {} if check_ensemble_eval(args) else None  # --ensemble-eval: the last ensemble evaluation's figures; SystemExit if it cannot run
    consensus = {} if check_consensus_eval(args) else None  # --consensus-eval likewise
    if check_hash_consensus_eval(args):  # --hash-consensus-eval: the same scalars and closing line, voted by board key (tomato)
        consensus = {"hashed": True}
    hash_grow = check_hash_grow(args)  # --hash-grow: True / False; SystemExit on a level whose tables are not hashed
    transitions = check_transition_policy(args)  # --transition-policy: True / False; SystemExit off trans-boat or with --members
    trans_kw = {"transitions": True} if transitions else {}
    if check_fused_transition_learn(args):  # --fused-transition-learn: SystemExit without --transition-policy
        trans_kw["fused_transition_learn"] = True

    rank, local_rank, world = sdist.env_from_torchrun()
    if consensus is not None and world > 1:
        raise SystemExit("--%sconsensus-eval runs on one device: summing the votes over %d ranks is not built"
                         % ("hash-" if consensus.get("hashed") else "", world))
    if getattr(args, "devices", 1) > 1 and world != args.devices:
        raise SystemExit("--devices %d needs %d ranks (WORLD_SIZE is %d): run `python -m safe_grid_agents_amd --devices %d ...`, "
                         "which starts them, or torch.distributed.run --nproc-per-node %d" % (
                             args.devices, args.devices, world, args.devices, args.devices))
    if world > 1:
        if members:
            raise KeyError("--members runs on one GPU (sharding a population over GPUs is not built)")
        if args.agent_alias in ("ppo-mlp", "ppo-cnn", "ppo-crmdp"):
            raise KeyError("train_batched shards independent agents (tabular-q, random) over GPUs; %r shares one policy"
                           % (args.agent_alias,))
        sdist.init_process_group(os.environ.get("SGK_DIST_BACKEND"))  # nccl (= RCCL) unless the test knob says gloo
    if os.environ.get("SGK_BENCH_ONE_DEVICE") == "1":
        local_rank = 0  # test knob: every rank on the one GPU of the box
    begin, end = sdist.shard_range(args.n_envs, rank, world)
    env_name = ENV_MAP[args.env_alias]
    writer = (writer_factory or _default_writer)(getattr(args, "log_dir", None)) if rank == 0 else NullWriter(None)
    for key, value in vars(args).items():
        writer.add_text("data/{}".format(key), str(value))
    env = _envs.make(env_name, n_envs=end - begin, seed=args.seed or 0, device=local_rank, env_index_base=begin)
    horizon = int(env.info.max_iterations)
    sdist.library_comm(env)  # (several ranks under nccl) the metrics all-reduce's RCCL communicator, before the first flush
    if args.agent_alias == "tabular-q":
        agent = BatchedTabularQAgent(env, args)
    elif members and args.agent_alias == "deep-q":
        from .deepq_population import BatchedDeepQPopulation

        # the replay holds whole lockstep slices: as many as cover the reference's capacity per member, at least 2
        slices = max(2, -(-int(args.replay_capacity) // (env.n_envs // members)))
        agent = BatchedDeepQPopulation(env, args, members, replay_slices=slices, member_hyper=member_hyper)
        agent.warmup(slices)  # dqn_warmup (warmup.py:8-23) of every member: random-action transitions fill the replay
        env.reset()
    elif members:
        agent = (BatchedPPOCNNPopulation if args.agent_alias == "ppo-cnn" else BatchedPPOPopulation)(env, args, members,
                                                                                                     member_hyper=member_hyper)
    elif args.agent_alias in ("ppo-mlp", "ppo-cnn"):
        import torch

        torch.manual_seed(args.seed or 0)
        agent = BatchedPPOAgent(env, args, body=args.agent_alias[4:], **trans_kw)
    elif args.agent_alias == "ppo-crmdp":  # ppo-cnn with the corrupt-reward filter between the gather and the returns (crmdp.py)
        import torch

        from .crmdp import BatchedPPOCRMDPAgent

        torch.manual_seed(args.seed or 0)
        agent = BatchedPPOCRMDPAgent(env, args, **trans_kw)
    elif args.agent_alias == "deep-q":
        import torch

        from .deepq_batched import BatchedDeepQAgent

        if world > 1:
            raise KeyError("train_batched shards independent agents over GPUs; deep-q shares one network")
        torch.manual_seed(args.seed or 0)
        # the replay holds whole lockstep slices: as many as cover the reference's capacity, at least 2
        slices = max(2, -(-int(args.replay_capacity) // env.n_envs))
        agent = BatchedDeepQAgent(env, args, sgd_steps=1, replay_slices=slices)
        agent.warmup(slices)  # dqn_warmup (warmup.py:8-23): random-action transitions fill the replay
        env.reset()
    elif args.agent_alias == "random":
        agent = None
    else:
        raise KeyError("train_batched supports tabular-q, deep-q, ppo-mlp, ppo-cnn, ppo-crmdp and random, not %r" % (args.agent_alias,))
    ppo = isinstance(agent, (BatchedPPOAgent, BatchedPPOPopulation, BatchedPPOCNNPopulation))
    deepq = args.agent_alias == "deep-q"
    history = {"writer": writer, "t": 0, "t_learn": 0}
    period = 0
    per_member = None
    for episode in range(1, args.episodes + 1):
        if members and ppo:  # every member's rollout + epochs: two launches; the aggregate meters and the spread over the members
            per_member, bm = population_ppo_learn(agent, env, history, cheat=args.cheat)
            history["t"] += horizon
            for tag, name in (("Train/member_return", "returns"), ("Train/member_safety", "safeties")):
                writer.add_histogram(tag, np.array([m.meter(name)["avg"] for m in per_member], dtype=np.float64), episode)
        elif ppo:
            bm = batched_ppo_learn(agent, env, history, cheat=args.cheat)
            history["t"] += horizon
            if args.agent_alias == "ppo-crmdp":  # one read of three integers; RuntimeError for a corrupt state without a bound
                stats = agent.stats()
                writer.add_scalar("Train/crmdp_corrupt_states", stats["corrupt_states"], episode)
                writer.add_scalar("Train/crmdp_replaced_rewards", stats["replaced_rewards"], episode)
        else:
            env.metrics_reset()
            if agent is None:
                env.step_random(horizon, auto_reset=True)
            elif deepq:
                if members:
                    agent.reset_member_metrics()
                for _ in range(horizon):  # dqn_learn for every env: act_explore, step, replay add, one SGD step, epsilon, sync
                    agent.step(learn=True, cheat=args.cheat)
            else:
                if hash_grow:  # room for this period's boards before they are looked up (each rank on its own fullest table)
                    agent.reserve_hash(horizon)
                agent.rollout(horizon, cheat=args.cheat)
                if hasattr(agent, "check_hash_overflow"):
                    agent.check_hash_overflow()  # hashed tables (tomato watering): a full table stops the run at THIS period
            bm = sdist.global_metrics(env)  # this shard's metrics, all-reduced over the ranks when there are several
        bm.write(writer, episode, prefix="Train/")
        if members and deepq:  # the spread over the members, as the PPO population writes it
            per_member = agent.member_batch_metrics()
            for tag, name in (("Train/member_return", "returns"), ("Train/member_safety", "safeties")):
                writer.add_histogram(tag, np.array([m.meter(name)["avg"] for m in per_member], dtype=np.float64), episode)
        if sweep and per_member is not None:  # each grid point's return and safety, the mean over its replicas (members g, g + G, ...)
            G = len(sweep[1])
            for tag, name in (("Train/sweep_return", "returns"), ("Train/sweep_safety", "safeties")):
                avgs = np.array([m.meter(name)["avg"] for m in per_member], dtype=np.float64)
                for g, point in enumerate(sweep[1]):
                    writer.add_scalar("%s/%s" % (tag, point_label(sweep[0], point)), float(avgs[g::G].mean()), episode)
        if agent is not None and not ppo:
            eps = agent.epsilon  # (a swept population: one value per member on the device; the scalar is their mean)
            writer.add_scalar("Train/epsilon", float(eps.mean()) if hasattr(eps, "mean") else eps, agent.t)
        if deepq and agent.last_loss is not None:
            loss = agent.last_loss.mean() if members else agent.last_loss.reshape(-1)[0]  # (a population: the members' mean)
            writer.add_scalar("Train/value_loss", float(loss), agent.t)
        if pbt and episode % pbt["every"] == 0:  # the score: this period's per-member return (member_metrics, reset every period)
            agent.exploit_explore(fraction=pbt["fraction"], perturb=pbt["perturb"], factors=pbt["factors"])
            writer.add_scalar("Train/pbt/replaced", int((agent.pbt_src.cpu().numpy() != np.arange(members)).sum()), episode)
            for name in agent.PBT_COLUMNS:
                values = np.array([agent.member_hyper_of(m)[name] for m in range(members)], dtype=np.float64)
                writer.add_histogram("Train/pbt/%s" % name, values, episode)
        reporter(hidden_reward=bm.meter("safeties")["avg"], obs_reward=bm.meter("returns")["avg"])
        # evaluation cadence exactly as the reference's loops decide it: whiler (tabular-q / deep-q, learn.py:21-22) evaluates
        # after the episodes with episode % eval_every == eval_every - 1; ppo_learn (learn.py:100) after those with
        # episode % eval_every == 0 (episode > 0)
        if ppo:
            eval_next = episode > 0 and episode % args.eval_every == 0
        else:
            eval_next = episode % args.eval_every == args.eval_every - 1
        if agent is not None and eval_next:
            period = _batched_eval(agent, env, args, writer, period, rank, sdist, ensemble, consensus)
    if agent is not None:  # train.py:81: one more evaluation after the loop, unconditionally (also when the last episode had one)
        period = _batched_eval(agent, env, args, writer, period, rank, sdist, ensemble, consensus)
    if sweep and per_member is not None and rank == 0:  # the table, once: the last training period's episodes
        print("#### SWEEP: %d grid points x %d replicas, return and safety of the last training period, mean +- std over replicas ####"
              % (len(sweep[1]), members // len(sweep[1])))
        for line in sweep_table(sweep[0], sweep[1], [m.meter("returns")["avg"] for m in per_member],
                                [m.meter("safeties")["avg"] for m in per_member]):
            print(line)
    if pbt and per_member is not None and rank == 0:  # one line per member: where its hyper-parameters ended, and its last return
        print("#### PBT: %d members, every %d periods the worst %d became the best; values and return of the last training period ####"
              % (members, pbt["every"], int(pbt["fraction"] * members)))
        for m in range(members):
            print("member %-4d %-60s return %10.4f" % (m, " ".join("%s=%g" % kv for kv in agent.member_hyper_of(m).items()),
                                                       per_member[m].meter("returns")["avg"]))
    if ensemble and rank == 0:  # one line: the last evaluation of the members voting on every env
        print("#### ENSEMBLE: %d members vote on every env; last evaluation: return %.4f safety %.4f disagreement %.4f (%d of %d votes) ####"
              % (members, ensemble["return"], ensemble["safety"], ensemble["disagreement"], ensemble["dissent"], ensemble["votes"]))
    if consensus and "return" in consensus:  # one line: the last evaluation of the agents' plurality vote per state (tomato: per board)
        print("#### CONSENSUS: %d agents vote on every %s; last evaluation: return %.4f safety %.4f agreement %.4f (%d votes over %d %ss) ####"
              % (env.n_envs, "board" if consensus.get("hashed") else "state", consensus["return"], consensus["safety"], consensus["agreement"],
                 consensus["voters"], consensus["voted_states"], "board" if consensus.get("hashed") else "state"))
    return agent, env


def check_hash_grow(args):
    """--hash-grow of `args` -> True / False. SystemExit with a plain message for an agent other than tabular-q and for a level other
    than tomato: only its agents keep hash tables."""
    if not getattr(args, "hash_grow", False):
        return False
    if args.agent_alias != "tabular-q":
        raise SystemExit("--hash-grow grows the hash tables of tabular-q agents, not %r" % (args.agent_alias,))
    if args.env_alias != "tomato":
        raise SystemExit("--hash-grow runs on tomato only: %s has a perfect hash of its boards, its tables have no capacity to grow"
                         % (args.env_alias,))
    return True


def check_transition_policy(args):
    """--transition-policy of `args` -> True / False. SystemExit with a plain message for an agent without the conv body, for a level
    other than trans-boat (no other level observes transitions) and together with --members (the populations have no such form)."""
    if not getattr(args, "transition_policy", False):
        return False
    if args.agent_alias not in ("ppo-cnn", "ppo-crmdp"):
        raise SystemExit("--transition-policy is the two-channel conv body of ppo-cnn and ppo-crmdp, not %r" % (args.agent_alias,))
    if args.env_alias != "trans-boat":
        raise SystemExit("--transition-policy runs on trans-boat only: %s observes one board, not a transition" % (args.env_alias,))
    if int(getattr(args, "members", 0) or 0):
        raise SystemExit("--transition-policy has no population form: drop --members")
    return True


def check_fused_transition_learn(args):
    """--fused-transition-learn of `args` -> True / False. SystemExit with a plain message without --transition-policy: the flag
    chooses the learner of that body (check_transition_policy has the body's own conditions)."""
    if not getattr(args, "fused_transition_learn", False):
        return False
    if not getattr(args, "transition_policy", False):
        raise SystemExit("--fused-transition-learn is the fused learner of the two-channel body: give --transition-policy as well")
    return True


def sweep_grid(args):
    """--sweep NAME=v1,v2,... flags of `args` -> (names, grid) (member_hyper.parse_sweep; SystemExit with the valid names for a sweep
    that cannot run), or None without the flag."""
    specs = getattr(args, "sweep", None)
    if not specs:
        return None
    return parse_sweep(specs, args.agent_alias, int(getattr(args, "members", 0) or 0))


def members_n_envs(args):
    """--members M. ppo-mlp, ppo-cnn: the batch is N = M x rollouts envs (sets args.n_envs; an explicit -N that disagrees stops the run). deep-q:
    the batch is -N envs, N / M per member (N must be a multiple of M). Another agent stops the run with a message."""
    members = int(args.members)
    if members < 1:
        raise SystemExit("--members must be >= 1")
    if args.agent_alias == "deep-q":
        n = int(getattr(args, "n_envs", 0) or 0)
        if n < 1 or n % members:
            raise SystemExit("--members %d with deep-q splits the -N envs evenly: -N %d is %d x %d + %d (give -N a multiple of %d)"
                             % (members, n, members, n // members, n % members, members))
        if getattr(args, "q_body", "mlp") != "mlp":
            raise SystemExit("--members runs a population of the reference's MLP deep-q agents, not --q-body %s" % args.q_body)
        return n
    if args.agent_alias not in ("ppo-mlp", "ppo-cnn"):
        raise SystemExit("--members runs a population of ppo-mlp, ppo-cnn or deep-q agents, not %r" % (args.agent_alias,))
    n = members * int(args.rollouts)
    if int(getattr(args, "n_envs", 0) or 0) not in (0, n):
        raise SystemExit("--members %d with --rollouts %d is a batch of %d envs; -N %d disagrees (leave -N out)"
                         % (members, int(args.rollouts), n, args.n_envs))
    args.n_envs = n
    return n


def _batched_eval(agent, env, args, writer, period, rank, sdist, ensemble=None, consensus=None):
    from .loops import batched_default_eval

    if rank == 0:
        print("#### EVAL ####")
    if hasattr(agent, "check_hash_tables"):
        agent.check_hash_tables()  # levels without a perfect hash of their boards: a full table is an error, not a silent state
    if getattr(args, "hash_grow", False) and args.agent_alias == "tabular-q":  # greedy act() claims slots too
        agent.reserve_hash(max(int(args.eval_timesteps) - 1, 0) + int(env.info.max_iterations))
    if hasattr(agent, "member_metrics"):  # a population: the two greedy phases through the members rollout
        agent.evaluate(args.eval_timesteps)
    else:
        batched_default_eval(agent, env, args.eval_timesteps)
    sdist.global_metrics(env).write(writer, period, prefix="Evaluation/")
    if ensemble is not None:
        # --ensemble-eval: the same schedule once more with the members' vote as the agent. Training does not notice it: greedy acting
        # draws nothing and leaves the members' weights, optimiser state, metrics and draw counters alone; the env's metrics vector is
        # reset by the next training period before it is read, and the env.reset() below -- which follows every evaluation -- puts the
        # envs back to their initial states. (Levels whose own draws are keyed by the env's reset count see more resets, as they do
        # after any evaluation.)
        bm, dissent = agent.evaluate_ensemble(args.eval_timesteps)
        write_ensemble_eval(writer, bm, dissent, period)
        ensemble.update(dissent, **{"return": bm.meter("returns")["avg"], "safety": bm.meter("safeties")["avg"]})
    if consensus is not None:
        # --consensus-eval: the same schedule once more with the agents' plurality vote per state as the agent. Training does not notice
        # it: the vote only reads the tables, and the consensus agent acts on an env handle of its own -- this env's metrics, reset
        # counters and state words are not touched.
        hashed = consensus.get("hashed")  # (tomato: the vote by board key, on a twin whose greedy acting claims its own slots)
        bm, stats = (agent.evaluate_hash_consensus if hashed else agent.evaluate_consensus)(args.eval_timesteps)
        write_consensus_eval(writer, bm, stats, period)
        consensus.update(stats, **{"return": bm.meter("returns")["avg"], "safety": bm.meter("safeties")["avg"]})
    env.reset()
    return period + 1
