"""The probe environments of ``sac.envs`` and the control tasks of
``sac.control_envs`` (the pendulum swing-up, the two-link reacher, the balancing
cart-pole) resident on the device.

``DeviceVectorEnv`` holds N copies of one environment as device state
(``include/sac_engine.h`` ``sac_envs``) and steps them in HIP kernels with the
semantics ``sac.vector_env.SyncVectorEnv`` gives the host classes: same-step
autoreset, ``infos["final_obs"]`` holding the true next state of every env.
Observations, rewards and flags are the host classes' (bit for bit; what
``sac/envs.py`` keeps as Python floats is float64 on the device).

Two ways to step:

* ``step(actions)``: the gym-shaped path for a caller with its own policy.
  Takes and returns device tensors, never copies to the host;
* ``SacEngine.rollout_step(envs, replay)``: act -> step -> store fused into ONE
  launch (the policy forward, the squashed-Gaussian sample, the env step and
  the write into the replay ring), the step of ``SAC.run_device_training_loop``.

The only randomness is ``RandomObsBinaryRewardEnv``'s observations and the
reset states of the control tasks: Philox draws keyed by the seed given to
``reset`` with counter (vector step, env row), so a run is reproducible
whatever order the workgroups run in (the host classes draw from numpy's
generator instead: same distribution, other numbers).  ``obs_dim`` and
``act_dim`` are the host class's spaces', per kind (``include/sac_engine.h``
has the table).  A control task's float64 arithmetic is the host class's in the
same order; its ``sin`` / ``cos`` are the device library's, so its fp32
observations and rewards may differ from the host's in the last bit.  Per task:

* ``PendulumEnv``: one torque, never terminated;
* ``ReacherEnv``: two torques; its state never takes a sine or cosine in, so
  its (angles, speeds, target) are the host class's bit for bit;
* ``CartPoleEnv``: one force; episodes end by failure, at different steps in
  different rows; ``sin`` / ``cos`` feed back into its state, which therefore
  follows the host class's to a few float64 ulps, not to the bit.

Episode statistics: every step writes each env's running (return, length,
ended) into a dense ring ``[ring_steps][N]`` indexed by ``t % ring_steps``;
``episode_cells`` queues an asynchronous copy of the cells of a range of steps
and ``EpisodeDrain`` consumes them in ``(t, i)`` order, the order in which the
host loop sees episodes end.

There is no host fallback: without the engine ``DeviceVectorEnv(...)`` raises
``EngineUnavailable``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _engine as E
from . import control_envs
from . import envs as host_envs
from .copy_behind import PendingCopies, copy_ring_cells

# kind name -> (sac_env_kind, host class); the names of sac/train_replicas.py
KINDS = {
    "constant_reward": (0, host_envs.ConstantRewardEnv),
    "quadratic_action": (1, host_envs.QuadraticActionRewardEnv),
    "random_obs_binary": (2, host_envs.RandomObsBinaryRewardEnv),
    "point_mass": (3, host_envs.OneDPointMassReachEnv),
    "pendulum": (8, control_envs.PendulumEnv),
    "reacher": (16, control_envs.ReacherEnv),
    "cartpole": (32, control_envs.CartPoleEnv),
}
# rows of the float64 state tensor of a control task: its position block, the episode return, its velocity block
# (include/sac_engine.h: SAC_ENV_POS_ROWS + 1 + SAC_ENV_VEL_ROWS, which has each block's components)
_DSTATE_ROWS = {"pendulum": 3, "reacher": 7, "cartpole": 5}
_BY_CLASS = {cls.__name__: name for name, (_, cls) in KINDS.items()}
_BY_CODE = {code: name for name, (code, _) in KINDS.items()}
# Kinds that ``kind_name`` (and so ``DeviceVectorEnv(name, N)``) does not resolve from the bare table key:
# tests/test_device_envs_cpu.py has used "cartpole" as its example of an unknown name since before the kind
# existed, and that test stands.  The cart-pole is reached by its class, its class name, its code 32, or
# ``DeviceVectorEnv.from_env(CartPoleEnv(...), N)``; KINDS, _PARAM_ATTRS and train_replicas --env use the key.
_CLASS_OR_CODE_ONLY = frozenset({"cartpole"})

# sac_env_config double <- attribute of the host instance, per kind
_PARAM_ATTRS = {
    "constant_reward": {"reward": "constant_reward"},
    "quadratic_action": {"target": "target"},
    "random_obs_binary": {"threshold": "threshold"},
    "point_mass": {"start_pos": "start_pos", "goal_pos": "goal_pos", "dt": "dt", "step_penalty": "step_penalty",
                   "goal_reward": "goal_reward", "goal_tolerance": "goal_tolerance"},
    "pendulum": {"dt": "dt"},  # the torque bound is the action space's, as for every kind
    "reacher": {"dt": "dt"},
    "cartpole": {"dt": "dt"},
}


def kind_name(kind_or_name) -> str:
    """Canonical kind name of a name, a ``sac.envs`` / ``sac.control_envs`` class (or its name) or a
    sac_env_kind code.  The cart-pole's key is not accepted as a name (``_CLASS_OR_CODE_ONLY``)."""
    if isinstance(kind_or_name, str):
        name = _BY_CLASS.get(kind_or_name, None if kind_or_name in _CLASS_OR_CODE_ONLY else kind_or_name)
    elif isinstance(kind_or_name, type):
        name = _BY_CLASS.get(kind_or_name.__name__)
    else:
        name = _BY_CODE.get(int(kind_or_name))
    if name not in KINDS:
        raise ValueError(f"unknown device environment {kind_or_name!r} (one of "
                         f"{sorted(set(KINDS) - _CLASS_OR_CODE_ONLY)}, a host class, its name or a kind code)")
    return name


def dstate_rows(kind: str) -> int:
    """Rows of the float64 state tensor of a kind; a probe has its position and the episode return."""
    return _DSTATE_ROWS.get(kind, 2)


class DeviceVectorEnv:
    #: vector steps the episode ring holds; a loop must copy a step's cells out
    #: before ``ring_steps`` further steps overwrite them
    RING_STEPS = 256

    def __init__(self, kind_or_name, num_envs: int, device=None, ring_steps: Optional[int] = None, **env_kwargs):
        self._setup(KINDS[kind_name(kind_or_name)][1](**env_kwargs), num_envs, device, ring_steps)

    @classmethod
    def from_env(cls, host_env, num_envs: int, device=None, ring_steps: Optional[int] = None) -> "DeviceVectorEnv":
        """N device copies of ``host_env`` (an instance of a ``sac.envs`` class or of a
        ``sac.control_envs`` one), with its parameters."""
        kind_name(type(host_env))
        self = cls.__new__(cls)
        self._setup(host_env, num_envs, device, ring_steps)
        return self

    def _setup(self, host, num_envs: int, device, ring_steps: Optional[int]) -> None:
        self.kind = kind_name(type(host))
        self.kind_code = KINDS[self.kind][0]
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("DeviceVectorEnv needs at least one environment")
        # the host instance supplies the spaces (the same Box as sac/envs.py) and the parameters
        self.single_observation_space = self.observation_space = host.observation_space
        self.single_action_space = self.action_space = host.action_space
        self.spec = getattr(host, "spec", None)
        self.obs_dim = int(np.prod(host.observation_space.shape))
        self.act_dim = int(np.prod(host.action_space.shape))
        self.max_steps = int(host.max_steps)
        params = dict.fromkeys(E.ENV_PARAMS, 0.0)
        params["action_low"] = float(host.action_space.low[0])
        params["action_high"] = float(host.action_space.high[0])
        for field, attr in _PARAM_ATTRS[self.kind].items():
            params[field] = float(getattr(host, attr))
        self.params = params
        self._params = [params[k] for k in E.ENV_PARAMS]
        self._icfg = [self.kind_code, self.num_envs, self.obs_dim, self.max_steps]
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        E.require_gpu(self.device)
        self.ops = E.ops()
        N, dev = self.num_envs, self.device
        self.ring_steps = int(ring_steps or self.RING_STEPS)
        if self.ring_steps < 1:
            raise ValueError("ring_steps must be >= 1")
        self.obs = torch.zeros(N, self.obs_dim, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, N, dtype=torch.int32, device=dev)   # step in episode, episode length
        self.dstate = torch.zeros(dstate_rows(self.kind), N, dtype=torch.float64, device=dev)
        self.ring = torch.zeros(self.ring_steps, N, 2, dtype=torch.float64, device=dev)
        self.seed = 0
        self.t = 0  # vector steps taken since the last reset; step k (0-based) is RNG step t = k + 1
        self._reset_done = False

    # ------------------------------------------------------------------ gym-shaped API
    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """Reset every env (``seed`` keys the observation draws from here on;
        None keeps the current one).  Returns (obs device tensor, {})."""
        if seed is not None:
            self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self.t = 0
        with torch.cuda.device(self.device):
            self.ops.envs_reset(self.obs, self.counters, self.dstate, self._icfg, self._params, self.seed)
        self._reset_done = True
        return self.obs.clone(), {}

    def step(self, actions):
        """Step with device actions [N][act_dim] -> device tensors (obs, rewards,
        terminated, truncated, {"final_obs": ...}); no host copy, no sync."""
        if not self._reset_done:
            self.reset()
        if not (isinstance(actions, torch.Tensor) and actions.is_cuda):
            raise TypeError("DeviceVectorEnv.step takes a device tensor of actions (it never copies from the host)")
        actions = actions.to(torch.float32).reshape(self.num_envs, self.act_dim).contiguous()
        with torch.cuda.device(self.device):
            obs, final_obs, rew, term, trunc = self.ops.envs_step(
                self.obs, self.counters, self.dstate, self.ring, self._icfg, self._params, self.seed, actions,
                self.t + 1)
        self.t += 1
        return obs, rew, term, trunc, {"final_obs": final_obs}

    def seed_action_spaces(self, seed: int) -> None:
        self.action_space.seed(seed)

    def close(self) -> None:
        pass

    # ------------------------------------------------------------------ episode records
    def episode_cells(self, t_first: int, t_last: int):
        """Queue an asynchronous copy of the ring cells of steps t_first..t_last
        (RNG step numbers, inclusive; at most ring_steps of them) to pinned host
        memory: (host tensor [n][N][2] float64, event).  No synchronisation."""
        n = t_last - t_first + 1
        if n < 1 or n > self.ring_steps:
            raise ValueError(f"episode_cells: {n} steps do not fit the ring of {self.ring_steps}")
        return copy_ring_cells(self.ring, t_first, n)

    @staticmethod
    def decode_cells(host) -> Tuple[List[float], List[int]]:
        """(returns, lengths) of the episodes that ended in copied cells [n][N][2], in (t, i) order."""
        ints = host[..., 1].contiguous().view(torch.int32).reshape(host.shape[0], host.shape[1], 2)
        ended = ints[..., 1] != 0  # boolean-mask indexing is row-major: (t, i) order
        return host[..., 0][ended].tolist(), ints[..., 0][ended].tolist()

    @staticmethod
    def decode_cell_positions(host) -> Tuple[List[int], List[int]]:
        """(step offsets into the copy, env rows) of the same episodes, in the same order: a cell's
        position in the ring is where its episode ended."""
        ints = host[..., 1].contiguous().view(torch.int32).reshape(host.shape[0], host.shape[1], 2)
        where = torch.nonzero(ints[..., 1] != 0)  # row-major, as the boolean mask of decode_cells
        return where[:, 0].tolist(), where[:, 1].tolist()


def first_episodes_per_row(episodes, num_envs: int, k: int) -> List[float]:
    """The returns of each env row's first ``k`` episodes out of ``episodes``, an
    iterable of (vector step, env row, return) in (step, row) order, listed in
    (episode index, row) order: every row's first episode, then every row's
    second, ...  Taking the first ``k * num_envs`` episodes that finish instead
    over-counts short episodes once lengths vary (a row that fails early
    restarts and contributes again while a row that survives is still on its
    first); with equal lengths both rules pick the same episodes in the same
    order.  ValueError if a row has fewer than ``k``."""
    if num_envs < 1 or k < 1:
        raise ValueError("first_episodes_per_row needs num_envs >= 1 and k >= 1")
    per_row: List[List[float]] = [[] for _ in range(num_envs)]
    for _, row, ret in episodes:
        if len(per_row[row]) < k:
            per_row[row].append(ret)
    short = [i for i, r in enumerate(per_row) if len(r) < k]
    if short:
        raise ValueError(f"rows {short[:8]} ended fewer than {k} episodes")
    return [per_row[i][e] for e in range(k) for i in range(num_envs)]


class EpisodeDrain:
    """Finished episodes of a ``DeviceVectorEnv`` in ``(t, i)`` order without
    per-step host traffic (the copies of ``sac.copy_behind``): every
    ``every`` vector steps ``after_step`` queues one pinned copy of the new ring
    cells behind the launches and hands finished copies to ``on_episode(ret,
    length)``; ``finish`` waits for the rest.  ``on_episode_at(t, row, ret,
    length)``, if given, is called as well, with the vector step (RNG step
    number) and env row the episode ended at."""

    def __init__(self, envs: DeviceVectorEnv, on_episode, every: int = 64, on_episode_at=None):
        self.envs, self.on_episode, self.on_episode_at = envs, on_episode, on_episode_at
        self.every = max(1, min(int(every), envs.ring_steps))
        self.copied_to = envs.t  # last RNG step whose cells were queued
        self.pending = PendingCopies()

    def _queue(self) -> None:
        t = self.envs.t
        if t > self.copied_to:
            self.pending.push(*self.envs.episode_cells(self.copied_to + 1, t), self.copied_to + 1)
            self.copied_to = t

    def _deliver(self, host, t_first: int) -> None:
        rets, lengths = DeviceVectorEnv.decode_cells(host)
        if self.on_episode is not None:
            for ret, length in zip(rets, lengths):
                self.on_episode(ret, length)
        if self.on_episode_at is not None:
            for dt, row, ret, length in zip(*DeviceVectorEnv.decode_cell_positions(host), rets, lengths):
                self.on_episode_at(t_first + dt, row, ret, length)

    def after_step(self) -> None:
        if self.envs.t - self.copied_to >= self.every:
            self._queue()
        if self.pending:
            self.pending.consume(False, self._deliver)

    def finish(self) -> None:
        """Blocking: every episode that ended up to now."""
        self._queue()
        self.pending.consume(True, self._deliver)


class DeviceQValueLog:
    """``QValues/Q1`` and ``QValues/Q2`` per env step of the device-resident
    loop: the device counterpart of ``sac.agent.QValueLog``, built like
    ``EpisodeDrain``.

    ``after_step(first_slot, first_step)`` queues ONE launch of the
    critic-evaluation kernel (``SacEngine.q_values_replay``) that reads the N
    transitions the rollout step just wrote from the replay ring in place and
    writes Q1 / Q2 of (final_obs_i, a_i) under the critics of that moment into
    cell ``t % S`` of a device ring ``[S][N][2]`` -- the quantity
    ``run_vectorized_training_loop`` logs per env step.  Every ``every`` vector
    steps the new cells are copied to pinned memory behind the launches;
    once a copy's event has completed its values go to
    ``logger.log_q_values(q1, q2, step)``, steps ``first_step + i`` in order.
    ``finish`` consumes the rest, blocking.  Nothing else synchronises.

    ``first_cell`` shifts the cells: the k-th cell written is ``(first_cell +
    k) % S``.  A loop graph (``SacEngine.loop_graph(..., q_ring=log.ring)``)
    writes its vector steps' cells itself, at ``RNG step % S``; a log created
    with ``first_cell`` = the RNG step of the next vector step then only has to
    be told about them (``after_graph``) and drains them with the rest."""

    RING_STEPS = 256

    def __init__(self, engine, replay, num_envs: int, logger, every: int = 64, ring_steps: Optional[int] = None,
                 first_cell: int = 0):
        self.engine, self.replay, self.logger = engine, replay, logger
        self.first_cell = int(first_cell)
        self.num_envs = int(num_envs)
        self.ring_steps = int(ring_steps or self.RING_STEPS)
        if self.ring_steps < 1:
            raise ValueError("ring_steps must be >= 1")
        self.every = max(1, min(int(every), self.ring_steps))
        self.ring = torch.zeros(self.ring_steps, self.num_envs, 2, dtype=torch.float32, device=engine.device)
        self.t = 0          # cells written
        self.copied_to = 0  # cells queued for copy
        self.first_steps: List[int] = []  # first env step of the cells not yet queued
        self.pending = PendingCopies()

    def after_step(self, first_slot: int, first_step: int) -> None:
        """The rollout step wrote its N rows at ring slots ``first_slot + i``
        (wrapping); row i is logged at env step ``first_step + i``."""
        self.engine.q_values_replay(self.replay, first_slot, self.num_envs, next_obs=True,
                                    out=self.ring[(self.first_cell + self.t) % self.ring_steps])
        self.t += 1
        self.first_steps.append(int(first_step))
        self._poll()

    def after_graph(self, k_steps: int, first_step: int) -> None:
        """A loop graph just queued ``k_steps`` vector steps that write the
        next ``k_steps`` cells; the rows of the first are logged from env step
        ``first_step``.  Launches nothing."""
        for j in range(int(k_steps)):
            self.first_steps.append(int(first_step) + j * self.num_envs)
        self.t += int(k_steps)
        self._poll()

    def _poll(self) -> None:
        if self.t - self.copied_to >= self.every:
            self._queue()
        if self.pending:
            self.pending.consume(False, self._deliver)

    def _queue(self) -> None:
        n = self.t - self.copied_to
        if n < 1:
            return
        # later launches into these cells queue behind this copy on the stream
        self.pending.push(*copy_ring_cells(self.ring, self.first_cell + self.copied_to, n), self.first_steps)
        self.first_steps = []
        self.copied_to = self.t

    def _deliver(self, host, firsts: List[int]) -> None:
        for cell, first in zip(host.tolist(), firsts):
            for i, (q1, q2) in enumerate(cell):
                self.logger.log_q_values(q1, q2, first + i)

    def finish(self) -> None:
        """Blocking: every value recorded up to now."""
        self._queue()
        self.pending.consume(True, self._deliver)


__all__ = ["DeviceVectorEnv", "DeviceQValueLog", "EpisodeDrain", "KINDS", "first_episodes_per_row", "kind_name"]
