"""Independent-seed replica training, one process per GPU.

The reference trains ONE learner per ``main.py`` run (reference main.py:43-48
-> sac/agent.py:329-418).  The SAC step does not shard, so N GPUs train N
independent learners: rank r uses seed ``train.seed + r`` for its networks,
device RNG and envs, trains on ``cuda:LOCAL_RANK`` through
``SAC.run_vectorized_training_loop``, and every ``--aggregate-every``
gradient steps the replica metric vector (``sac.replicas.METRICS``: steps,
wall_s, the four losses, alpha, mean return of the last 100 episodes) is
all-reduced over RCCL (``torch.distributed`` backend "nccl" on ROCm) on the
device, with no host synchronisation in the loop.  Rank 0 prints the final
aggregate as one JSON line.

    python -m torch.distributed.run --nnodes 1 --nproc-per-node 8 \\
        --master-addr 127.0.0.1 --master-port 29500 \\
        soft-actor-critic_amd/sac/train_replicas.py --config cfg.yaml \\
        --env point_mass --num-envs 16 --env-steps 200000

Without torchrun it runs one replica in-process.  ``--env`` names one of the
probe envs of ``sac.envs``, ``pendulum``, ``reacher`` or ``cartpole`` (the control tasks of
``sac.control_envs``) or, when gymnasium is importable, any registered
gymnasium id (the reference's own envs).  The policy's output range is the
config's ``policy_net.action_scale``, not the environment's: for ``pendulum``
set it to 2.0 (its torque bound); at 1.0 the policy can use only half the
torque.  ``reacher`` and ``cartpole`` take 1.0.

``--device-envs`` (the built-in envs only) keeps the environments on the device
(``sac.device_envs.DeviceVectorEnv``) and trains through
``SAC.run_device_training_loop``: act -> step -> store is one launch per
vector step, with no per-step host<->device traffic.  A config with
``logger.log_q_values: true`` runs there unchanged: the per-env-step Q values
are evaluated and logged on the device (``device_q_values=True``).
``--graph-steps K`` (even, >= 2; with ``--device-envs``) replays blocks of K
vector steps from one hipGraph with the loop cursor on the device
(``run_device_training_loop(graph_steps=K)``); the aggregation callback then
runs once per block.

``--n-step K`` (1..8) sets ``train.n_step``: n-step returns in either loop
(``sac.nstep``).  The loop graph does not hold them, so ``--n-step`` above 1
with ``--graph-steps`` exits, and with ``--device-envs`` the per-env-step Q
values are not logged (``logger.log_q_values`` must be off).

``--bootstrap-truncated`` sets ``train.bootstrap_truncated: true``: time-limit
bootstrapping in either loop, with or without ``--graph-steps`` and ``--n-step``
(a stored row's done is ``terminated`` alone).

``--random-steps K`` sets ``train.random_steps``: the first K env steps of either
loop act uniformly at random over the policy's range, with or without
``--device-envs``, ``--graph-steps``, ``--n-step`` and ``--bootstrap-truncated``
(DESIGN.md §3.13).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
from typing import Callable, Optional

import torch

if __package__ in (None, ""):  # run as a script: make `sac` importable
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sac.replicas import ReplicaAggregator, replica_seed  # noqa: E402

# name -> (module of the sac package, class, constructor arguments): the environments with a device form
PROBE_ENVS = {
    "point_mass": ("envs", "OneDPointMassReachEnv", {}),
    "constant_reward": ("envs", "ConstantRewardEnv", {}),
    "quadratic_action": ("envs", "QuadraticActionRewardEnv", {}),
    "random_obs_binary": ("envs", "RandomObsBinaryRewardEnv", {}),
    "pendulum": ("control_envs", "PendulumEnv", {}),
    "reacher": ("control_envs", "ReacherEnv", {}),
    "cartpole": ("control_envs", "CartPoleEnv", {}),
}


def env_factory(name: str) -> Callable[[], object]:
    """A zero-argument env constructor for ``name``: a probe env of sac.envs or
    a control task of sac.control_envs, else a gymnasium id (gymnasium must be
    importable)."""
    if name in PROBE_ENVS:
        import importlib

        mod, cls, kw = PROBE_ENVS[name]
        return lambda: getattr(importlib.import_module("sac." + mod), cls)(**kw)
    try:
        import gymnasium as gym
    except ImportError as e:  # the probe envs need nothing
        raise SystemExit(f"--env {name!r}: not a probe env ({sorted(PROBE_ENVS)}) and gymnasium is not installed") from e
    return lambda: gym.make(name)


def rank_env() -> tuple:
    """(rank, world, local_rank) from the torchrun environment (0, 1, 0 without it)."""
    return (int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)),
            int(os.environ.get("LOCAL_RANK", 0)))


def train_replica(config: dict, make_env: Callable[[], object], num_envs: int, env_steps: int, every: int,
                  rank: int, device: Optional[str] = None, agent_cls=None, vec_env_cls=None,
                  device_envs: bool = False, graph_steps: int = 0) -> dict:
    """Train this rank's replica and return {"metrics": its loop metrics,
    "aggregate": the all-reduced METRICS summary}.  ``agent_cls`` /
    ``vec_env_cls`` default to sac.agent.SAC / sac.vector_env.SyncVectorEnv
    (tests pass host stubs).  ``device_envs``: ``make_env`` must build a probe
    env of sac.envs or a control task of sac.control_envs; num_envs device copies of it (DeviceVectorEnv.from_env)
    train through ``run_device_training_loop`` (``graph_steps``: its argument)."""
    if agent_cls is None:
        from sac.agent import SAC as agent_cls  # noqa: N813
    if vec_env_cls is None:
        from sac.vector_env import SyncVectorEnv as vec_env_cls  # noqa: N813
    cfg = copy.deepcopy(config)
    cfg["train"]["seed"] = replica_seed(cfg["train"]["seed"], rank)
    if device is not None:
        cfg["train"]["device"] = device
    lg = cfg.get("logger", {})
    if lg.get("agent_name"):
        lg["agent_name"] = f"{lg['agent_name']}_rank{rank}"  # per-replica run directories
    if device_envs:
        from sac.device_envs import DeviceVectorEnv

        vec = DeviceVectorEnv.from_env(make_env(), num_envs, device=cfg["train"].get("device"))
    else:
        vec = vec_env_cls([make_env] * num_envs)
    agent = agent_cls(vec, cfg)
    if getattr(agent, "engine", None) is None:
        # no HIP engine (no MI355X visible, or train.engine_device: cpu): the
        # learner cannot step and there is no CPU fallback -- say so here,
        # before the loop, instead of failing inside it
        from sac import _engine as E

        raise E.EngineUnavailable(f"replica {rank}: replica training needs the HIP engine on an MI355X "
                                  f"(train.device={cfg['train'].get('device')!r}); there is no CPU fallback")
    agg = ReplicaAggregator(agent.engine, every)
    if device_envs:
        # a config with logger.log_q_values (every probe config of the reference) logs them on the device
        extra = {"graph_steps": graph_steps} if graph_steps else {}
        # n-step returns (train.n_step > 1) have no device Q-value log
        metrics = agent.run_device_training_loop(env_steps, callback=agg, seed=cfg["train"]["seed"],
                                                 device_q_values=int(cfg["train"].get("n_step", 1)) == 1, **extra)
    else:
        metrics = agent.run_vectorized_training_loop(env_steps, callback=agg, seed=cfg["train"]["seed"])
    return {"metrics": metrics, "aggregate": agg.finish()}


def parse_args(argv=None) -> argparse.Namespace:
    """The command line, with the combinations the device loop cannot run refused (SystemExit)."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="YAML config in the reference's format")
    ap.add_argument("--env", default="point_mass")
    ap.add_argument("--num-envs", type=int, default=16)
    ap.add_argument("--env-steps", type=int, default=100_000)
    ap.add_argument("--aggregate-every", type=int, default=1000, help="gradient steps between all-reduces")
    ap.add_argument("--device-envs", action="store_true",
                    help="keep the (built-in) environments on the device: one fused act/step/store launch per vector "
                         "step")
    ap.add_argument("--graph-steps", type=int, default=0,
                    help="with --device-envs: vector steps per hipGraph replay of the loop (even, >= 2; 0 = stepwise)")
    ap.add_argument("--n-step", type=int, default=None,
                    help="n-step returns: sets train.n_step (1..8; default: the config's, else 1)")
    ap.add_argument("--bootstrap-truncated", action="store_true",
                    help="time-limit bootstrapping: sets train.bootstrap_truncated (rows the time limit ended "
                         "bootstrap from their next state)")
    ap.add_argument("--random-steps", type=int, default=None,
                    help="uniform-random warm-up actions: sets train.random_steps (env steps, >= 0; default: the "
                         "config's, else 0)")
    a = ap.parse_args(argv)
    if a.random_steps is not None and a.random_steps < 0:
        raise SystemExit(f"--random-steps must be an integer >= 0, got {a.random_steps}")
    if a.device_envs and a.env not in PROBE_ENVS:
        raise SystemExit(f"--device-envs: {a.env!r} is not a probe env ({sorted(PROBE_ENVS)})")
    if a.graph_steps and not a.device_envs:
        raise SystemExit("--graph-steps needs --device-envs (the loop graph holds the device-resident loop)")
    if a.n_step is not None:
        from sac.nstep import check_n_step, n_step_refusal

        try:
            check_n_step(a.n_step, "--n-step")
        except ValueError as e:
            raise SystemExit(str(e)) from e
        if a.n_step > 1 and a.graph_steps:
            raise SystemExit(n_step_refusal(a.n_step, "graph_steps"))
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    import yaml

    with open(a.config) as f:
        config = yaml.safe_load(f)
    if a.n_step is not None:
        config["train"]["n_step"] = a.n_step
    if a.bootstrap_truncated:
        config["train"]["bootstrap_truncated"] = True
    if a.random_steps is not None:
        config["train"]["random_steps"] = a.random_steps
    rank, world, local = rank_env()
    if not torch.cuda.is_available():
        raise SystemExit("train_replicas: no HIP device visible; replica training runs the HIP engine, one "
                         "process per MI355X (there is no CPU fallback)")
    device = f"cuda:{local}"
    if world > 1:
        import torch.distributed as dist

        torch.cuda.set_device(local)
        dist.init_process_group("nccl")  # RCCL on ROCm: the metric all-reduce only
    try:
        out = train_replica(config, env_factory(a.env), a.num_envs, a.env_steps, a.aggregate_every, rank, device,
                            device_envs=a.device_envs, graph_steps=a.graph_steps)
    finally:
        if world > 1:
            import torch.distributed as dist

            dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"replicas": world, "rank0": out["metrics"], "aggregate": out["aggregate"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
