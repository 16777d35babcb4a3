"""Soft Actor-Critic agent (API of reference ``sac/agent.py``) on the MI355X engine.

``SAC(env, config)`` accepts the reference's YAML config unchanged and exposes
the same attributes and methods.  What changes is underneath:

* ``training_step`` (agent.py:302-327) is ONE call into ``libsac_engine.so``:
  four HIP kernels (sample+target+critic-backward, critic update, actor, actor
  update) on the current stream, no host synchronisation and no ``.item()``;
* the replay buffer lives in HBM (``sac.replay_buffer``);
* ``select_action`` (agent.py:149-156) runs the policy head in a HIP kernel.

Extra (optional) config keys, all under ``train``:
    precision: 'fp32' (default; exact-fp32 MFMA products, the reference's arithmetic) |
               'bf16' (opt-in: bf16 MFMA products, fp32 accumulate and master weights;
               loss deviation from the fp32 reference up to ~2e-3 rel)
    rng:       'device' (default; Philox/Feistel on the GPU, graph-replayable) |
               'reference' (Python ``random.sample`` indices + torch eps draws,
               the reference's RNG consumption)
    graph_chunk: steps per captured hipGraph for ``train_steps`` (default 32)
    engine_device: 'auto' (default) | 'cpu'.  The reference's ``device: cpu``
               configs (e.g. hparam_search/configs/inverted_pendulum.yaml:38)
               run unchanged: with 'auto' and a HIP device visible, the agent
               trains on the engine (``cuda:<current device>``) and warns once;
               'cpu' keeps the networks on the host, where the hot path raises
               ``EngineUnavailable`` (there is no CPU fallback).

    n_step:    n-step returns, 1 (default) .. 8, in ``run_vectorized_training_loop`` and
               ``run_device_training_loop`` (``sac.nstep``): the loops stage the last n
               vector steps' rows and store n-step rows, and the engine trains with the
               discount gamma^n.  Everything that stores one-step rows or replays the
               loop graph refuses n_step > 1 (ValueError): ``run_training_loop``,
               ``store_transition``, ``warmup_replay_buffer``, ``graph_steps`` > 0 and
               ``device_q_values=True``.

    bootstrap_truncated: false (default) | true.  Time-limit bootstrapping in all four
               loops: a stored row's ``done`` is ``terminated`` alone, so a
               row the time limit ended bootstraps from its true next state.  With n_step > 1
               a window the limit closes after k < n steps stores ``1 - gamma^k / gamma^n``
               (<= 0), which the gradient step's ``gamma^n (1 - done)`` turns into gamma^k.

    random_steps: K >= 0 (default 0: nothing changes).  The first K env steps of a
               ``run_vectorized_training_loop`` or ``run_device_training_loop`` run act
               uniformly at random over the policy's range [-action_scale, action_scale)
               instead of sampling the untrained policy: vector step v of
               N envs is uniform iff v * N < K (``uniform_vector_step``).  On the device the
               step is a launch with no policy forward; the vectorised loop takes the same
               draws from the host (``SacEngine.uniform_actions``).  ``run_training_loop``
               keeps the reference's ``warmup_replay_buffer``.

After ``load_agent`` with auto-tuning, alpha stays frozen as in the reference
(it rebinds ``log_alpha`` but not its optimizer, agent.py:550-554); the
optional ``train.alpha_after_load: tune`` keeps tuning it instead.

Per-env-step ``QValues/*`` logging (``logger.log_q_values``) runs without the
reference's ``.item()`` syncs (``QValueLog``), in both training loops.
"""
from __future__ import annotations

import os
import pprint
import random
import time
import warnings
from collections import deque
from copy import deepcopy
from typing import Callable, Any, Dict, List, Optional

import numpy as np
import torch
import torch.optim as optim

from . import _engine as E
from .copy_behind import PendingCopies, copy_ring_cells
from .engine import SacEngine
from .models import PolicyNetwork, QNetwork
from .nstep import NStepStage, check_n_step, discount_powers, end_codes, refuse_n_step
from .replay_buffer import ReplayBuffer, Transition

try:  # progress bars are optional
    from tqdm import tqdm as _tqdm
except Exception:  # pragma: no cover
    def _tqdm(it, disable=False):
        return it


def _make_logger(cfg, env_name, agent_name):
    from .utils.experiment_logger import ExperimentLogger

    return ExperimentLogger(cfg, env_name=env_name, agent_name=agent_name)


def resolve_device(train_cfg: dict) -> torch.device:
    """Device the agent trains on.  ``train.device`` as written, except that a
    reference config asking for ``cpu`` moves to the HIP device when one is
    visible (``train.engine_device: auto``, the default): the step only exists
    as the engine, and the reference's CPU configs should drop in unchanged."""
    dev = torch.device(train_cfg["device"])
    mode = train_cfg.get("engine_device", "auto")
    if mode not in ("auto", "cpu"):
        raise ValueError(f"train.engine_device must be 'auto' or 'cpu', got {mode!r}")
    if dev.type == "cpu" and mode == "auto" and torch.cuda.is_available():
        gpu = torch.device("cuda", torch.cuda.current_device())
        warnings.warn(f"train.device is 'cpu': the SAC step runs on the MI355X engine, training on {gpu} "
                      "(train.engine_device: cpu keeps the host device)", stacklevel=3)
        return gpu
    return dev


def due_updates(old_steps: int, new_steps: int, update_frequency: int, gradient_steps: int) -> int:
    """Gradient steps the reference loop runs while its env-step counter goes
    from old_steps to new_steps: ``gradient_steps`` at every step t with
    t % update_frequency == 0 (agent.py:361-364)."""
    return (new_steps // update_frequency - old_steps // update_frequency) * gradient_steps


def due_updates_gated(old_steps: int, new_steps: int, len_before: int, capacity: int, warming_steps: int,
                      update_frequency: int, gradient_steps: int) -> int:
    """``due_updates`` restricted to the env steps at which the reference's
    ``can_update()`` already holds (agent.py:159-164, 361-362): env step t
    (old_steps < t <= new_steps) pushes the (t - old_steps)-th of this vector
    step's transitions, after which the buffer holds min(capacity, len_before +
    t - old_steps) rows; it updates only if that is >= warming_steps."""
    if warming_steps > capacity or new_steps <= old_steps:
        return 0
    first = old_steps + max(1, warming_steps - len_before)  # first env step with can_update() true
    if first > new_steps:
        return 0
    return due_updates(first - 1, new_steps, update_frequency, gradient_steps)


def due_updates_staged(old_steps: int, new_steps: int, emitted: int, len_before: int, capacity: int,
                       warming_steps: int, update_frequency: int, gradient_steps: int) -> int:
    """The gate of a vector step of an n-step loop (``train.n_step``), which
    stores its rows n - 1 vector steps late.  A step that ``emitted`` its rows is
    gated exactly as ``due_updates_gated``; a step that emitted none leaves the
    buffer at ``len_before`` rows, so ``can_update()`` holds at every one of its
    env steps or at none: ``due_updates`` if ``warming_steps <= capacity`` and
    ``len_before >= warming_steps``, else 0."""
    if emitted:
        return due_updates_gated(old_steps, new_steps, len_before, capacity, warming_steps, update_frequency,
                                 gradient_steps)
    if warming_steps > capacity or len_before < warming_steps or new_steps <= old_steps:
        return 0
    return due_updates(old_steps, new_steps, update_frequency, gradient_steps)


def check_random_steps(k, key: str = "train.random_steps") -> int:
    """``k`` as an int >= 0, or ValueError naming ``key``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 0:
        raise ValueError(f"{key} must be an integer >= 0, got {k!r}")
    return int(k)


def uniform_vector_step(v: int, num_envs: int, random_steps: int) -> bool:
    """Whether vector step ``v`` (0-based in the run) of ``num_envs`` envs acts
    uniformly at random under ``train.random_steps``: iff its first env step,
    ``v * num_envs``, is one of the first ``random_steps``.  So the uniform
    steps are the first ceil(random_steps / num_envs) of a run."""
    return v * num_envs < random_steps


def graph_block_policy_only(first: int, num_envs: int, random_steps: int) -> bool:
    """Whether the block of vector steps that starts at ``first`` may run from
    the loop graph as far as ``train.random_steps`` goes: none of its steps is
    uniform.  The uniform steps are a prefix of the run, so that is its first."""
    return not uniform_vector_step(first, num_envs, random_steps)


#: times ``run_device_training_loop(graph_steps=K)`` captures its loop graph again because the block's
#: gradient-step pattern changed; after that a block with another pattern runs stepwise
MAX_RECAPTURES = 4


def plan_graph_block(total_steps: int, len_replay: int, capacity: int, warming_steps: int, update_frequency: int,
                     gradient_steps: int, num_envs: int, k_steps: int) -> List[int]:
    """Gradient steps the device-resident loop runs after each of its next
    ``k_steps`` vector steps, from its bookkeeping before the first of them
    (env steps taken, rows in the replay buffer): vector step j moves the env
    step counter by ``num_envs`` and runs ``due_updates_gated`` of that move if
    ``can_update()`` holds after it, exactly as the stepwise loop does."""
    counts = []
    for _ in range(k_steps):
        due = due_updates_gated(total_steps, total_steps + num_envs, len_replay, capacity, warming_steps,
                                update_frequency, gradient_steps)
        total_steps += num_envs
        len_replay = min(capacity, len_replay + num_envs)
        counts.append(due if len_replay >= warming_steps else 0)
    return counts


def graph_block_ready(counts: List[int], len_replay: int, capacity: int, warming_steps: int, batch: int,
                      num_envs: int) -> bool:
    """Whether a block with these per-vector-step gradient counts may run from
    the loop graph: the warm-up is over by its first vector step
    (``can_update()`` holds after it) and every gradient step finds at least
    ``batch`` rows.  A block that fails runs stepwise, which raises what the
    stepwise loop raises."""
    if min(capacity, len_replay + num_envs) < warming_steps:
        return False
    return all(min(capacity, len_replay + (j + 1) * num_envs) >= batch for j, g in enumerate(counts) if g)


class GraphBlockPolicy:
    """Which blocks replay the captured loop graph: the first ready block
    captures; a ready block with the captured pattern replays; one with
    another pattern captures again, ``max_recaptures`` times in all, and runs
    stepwise after that."""

    def __init__(self, max_recaptures: int = MAX_RECAPTURES):
        self.captured: Optional[List[int]] = None
        self.left = int(max_recaptures)

    def admit(self, counts: List[int]) -> bool:
        if counts == self.captured:
            return True
        if self.captured is not None:
            if self.left <= 0:
                return False
            self.left -= 1
        self.captured = list(counts)
        return True


class LossLog:
    """Loss and throughput scalars for the logger without per-step host syncs
    (the reference logs none: agent.py:324 drops the alpha
    dict and the losses are never read).  Every ``every`` gradient steps it
    queues an async device->pinned copy of the last step's [L_Q1, L_Q2, L_pi,
    L_alpha, alpha] behind the training launches and logs the previous
    snapshot once its event has completed; ``finish`` waits for the last one.
    Tags: Loss/Q1, Loss/Q2, Loss/Policy, Loss/Alpha (auto-tuning only), Alpha,
    Perf/GradientStepsPerSec, Perf/EnvStepsPerSec (host wall clock between
    snapshots), all at the gradient-step count of the snapshot."""

    TAGS = ("Loss/Q1", "Loss/Q2", "Loss/Policy", "Loss/Alpha", "Alpha")

    def __init__(self, engine: SacEngine, logger, every: int):
        self.engine, self.logger, self.every = engine, logger, max(1, int(every))
        self.buf = torch.zeros(5, dtype=torch.float64, pin_memory=torch.cuda.is_available())
        self.ev: Optional[torch.cuda.Event] = None
        self.pending_step = 0
        self.next_at = self.every
        self.t0 = time.perf_counter()
        self.grad0 = engine.steps_done
        self.env0 = 0

    def _emit(self) -> None:
        vals = self.buf.tolist()
        for tag, v in zip(self.TAGS, vals):
            if not (tag == "Loss/Alpha" and v != v):  # NaN L_alpha: fixed temperature
                self.logger.log_scalar(tag, v, self.pending_step)
        self.ev = None

    def after_updates(self, env_steps: int) -> None:
        eng = self.engine
        if eng.steps_done < self.next_at:
            return
        if self.ev is not None:
            if not self.ev.query():
                return  # the previous snapshot has not landed: skip this one, never block
            self._emit()
        now = time.perf_counter()
        dt = max(now - self.t0, 1e-9)
        self.logger.log_scalar("Perf/GradientStepsPerSec", (eng.steps_done - self.grad0) / dt, eng.steps_done)
        self.logger.log_scalar("Perf/EnvStepsPerSec", (env_steps - self.env0) / dt, eng.steps_done)
        self.t0, self.grad0, self.env0 = now, eng.steps_done, env_steps
        with torch.cuda.device(eng.device):
            snap = torch.cat([eng.stats[:4].double(), eng.alpha_state[1:2]])
            self.buf.copy_(snap, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()
        self.pending_step = eng.steps_done
        self.next_at = (eng.steps_done // self.every + 1) * self.every

    def finish(self) -> None:
        if self.ev is not None:
            self.ev.synchronize()
            self._emit()


class QValueLog:
    """``QValues/Q1`` and ``QValues/Q2`` per env step (agent.py:370-376,
    493-500) without the reference's two ``.item()`` host syncs per env step.

    ``record`` evaluates Q1 and Q2 of the env steps' (next state, action)
    pairs under the critics of that moment -- an eager forward on the
    engine-owned parameters, queued behind that env step's gradient steps --
    into a device buffer of [n][2]; the host inputs go up through pinned
    memory (non-blocking), so nothing waits.  Every ``every`` env steps (and
    at ``finish``) the filled rows are copied to pinned host memory behind the
    training launches, and ``logger.log_q_values(q1, q2, step)`` runs for each
    of them once that copy's event has completed (polled, never waited for,
    except by ``finish``).  Values are the reference's: the mean over a batch
    of one row is that row's value, as float32."""

    def __init__(self, agent: "SAC", logger, every: int = 256):
        self.agent, self.logger, self.every = agent, logger, max(1, int(every))
        self.cap = 2 * self.every
        self.dev = torch.empty(self.cap, 2, dtype=torch.float32, device=agent.device)
        self.fill = 0
        self.steps = []
        self.pending = PendingCopies()

    def record(self, states: Any, actions: Any, first_step: int) -> None:
        """Q of rows (states[i], actions[i]) logged at step first_step + i."""
        a = self.agent
        host = np.concatenate([np.asarray(states, np.float32).reshape(-1, a.obs_size),
                               np.asarray(actions, np.float32).reshape(-1, a.action_size)], axis=1)
        n = host.shape[0]
        if self.fill + n > self.cap:
            self._flush()
        if n > self.cap:  # one call larger than the ring (num_envs > 2 * every): grow it
            self.cap = n
            self.dev = torch.empty(self.cap, 2, dtype=torch.float32, device=a.device)
        x = torch.from_numpy(np.ascontiguousarray(host))
        if a.device.type == "cuda":
            x = x.pin_memory().to(a.device, non_blocking=True)
        s, act = x[:, :a.obs_size], x[:, a.obs_size:]
        with torch.no_grad():
            self.dev[self.fill:self.fill + n, 0] = a.q_net1(s, act).reshape(-1)
            self.dev[self.fill:self.fill + n, 1] = a.q_net2(s, act).reshape(-1)
        self.steps.extend(range(first_step, first_step + n))
        self.fill += n
        if self.fill >= self.every:
            self._flush()
        if self.pending:
            self.pending.consume(False, self._deliver)

    def _flush(self) -> None:
        if not self.fill:
            return
        # later record() writes to self.dev queue behind this copy on the stream
        self.pending.push(*copy_ring_cells(self.dev, 0, self.fill), self.steps)
        self.steps, self.fill = [], 0

    def _deliver(self, host, steps) -> None:
        for (q1, q2), st in zip(host.tolist(), steps):
            self.logger.log_q_values(q1, q2, st)

    def finish(self) -> None:
        self._flush()
        self.pending.consume(True, self._deliver)


class EpisodeStats:
    """What a training loop keeps about finished episodes (agent.py:331-336,
    391-404): ``count`` of them, ``avg`` return over the last 100 (nan before
    the first) and the ``best`` such average.  ``episode(ret, length)`` is
    called once per finished episode, in the order the loop sees them end:
    it appends to the window, updates ``avg`` then ``best``, logs the episode
    to ``logger`` (None: not logged) under index ``count``, prints the
    reference's line if ``print_rewards``, and only then counts it."""

    def __init__(self, logger=None, print_rewards: bool = False):
        self.logger, self.print_rewards = logger, print_rewards
        self.window = deque(maxlen=100)
        self.avg, self.best, self.count = float("nan"), -float("inf"), 0

    def episode(self, ret: float, length: int) -> None:
        self.window.append(ret)
        self.avg = float(np.mean(self.window))
        self.best = max(self.best, self.avg)
        if self.logger is not None:
            self.logger.log_episode_metrics(episode_idx=self.count, reward=ret, length=length)
        if self.print_rewards:
            print(f"Episode {self.count}, Return: {ret:.2f}, Average Return(last 100 episodes): {self.avg:.2f}")
        self.count += 1

    def counters(self, env_steps: int, gradient_steps: int) -> Dict[str, float]:
        """The host counters a loop's ``callback`` is given."""
        return {"env_steps": env_steps, "gradient_steps": gradient_steps, "episodes": self.count,
                "avg_return": self.avg}


class SAC:
    n_step = 1  # train.n_step; __init__ reads it
    bootstrap_truncated = False  # train.bootstrap_truncated; __init__ reads it
    random_steps = 0  # train.random_steps; __init__ reads it

    def __init__(self, env, config: dict):
        self.env = env
        self.config = config
        # n-step returns (sac.nstep): the discount powers gpow[0..n]; the engine trains with gpow[n]
        self.n_step = check_n_step(config["train"].get("n_step", 1))
        self.gpow = discount_powers(config["sac"]["gamma"], self.n_step)
        # time-limit bootstrapping: the stored done is `terminated` alone
        self.bootstrap_truncated = config["train"].get("bootstrap_truncated", False)
        if not isinstance(self.bootstrap_truncated, (bool, np.bool_)):
            raise ValueError(f"train.bootstrap_truncated must be a bool, got {self.bootstrap_truncated!r}")
        self.bootstrap_truncated = bool(self.bootstrap_truncated)
        # uniform-random warm-up actions of the vectorised and device loops
        self.random_steps = check_random_steps(config["train"].get("random_steps", 0))
        self.device = resolve_device(config["train"])
        self.replay_buffer = ReplayBuffer(config["buffer"]["capacity"], device=self.device)
        self.obs_size = env.observation_space.shape[0]
        self.action_size = env.action_space.shape[0]
        # same construction order (and therefore torch RNG use) as the reference
        self._init_policy_network()
        self._init_q_networks()
        self._init_optimizers()
        self._set_seed(config["train"]["seed"])

        self.target_entropy = -float(self.action_size)
        sac_cfg = config["sac"]
        self._auto = bool(sac_cfg["auto_entropy_tuning"])
        tr = config["train"]
        self.precision = tr.get("precision", "fp32")
        self.rng_mode = tr.get("rng", "device")
        self.graph_chunk = int(tr.get("graph_chunk", 32))
        self.engine: Optional[SacEngine] = None
        self._fixed_alpha = torch.tensor(sac_cfg["alpha"]).to(self.device)
        self.alpha_optimizer = None
        if self.device.type == "cuda":
            self._build_engine()

        self.env_name = config["logger"]["env_name"] or self._infer_env_name(env)
        self.agent_name = config["logger"]["agent_name"] or self.__class__.__name__
        self.logger = (_make_logger(config["logger"], self.env_name, self.agent_name)
                       if config["logger"]["enabled"] else None)

    # ------------------------------------------------------------------ construction
    def _init_q_networks(self) -> None:
        qc, seed = self.config["q_net"], self.config["train"]["seed"]
        kw = dict(obs_size=self.obs_size, action_size=self.action_size, hidden_sizes=qc["hidden_sizes"],
                  hidden_activations=qc["hidden_layers_act"], output_activation=qc["output_activation"])
        self.q_net1 = QNetwork(seed=seed, **kw).to(self.device)
        self.q_net2 = QNetwork(seed=seed + 1, **kw).to(self.device)
        self.q_net1_target = deepcopy(self.q_net1).to(self.device)
        self.q_net2_target = deepcopy(self.q_net2).to(self.device)

    def _init_policy_network(self) -> None:
        pc = self.config["policy_net"]
        self.policy_net = PolicyNetwork(
            obs_size=self.obs_size, action_size=self.action_size, hidden_sizes=pc["hidden_sizes"],
            log_std_min=pc["log_std_min"], log_std_max=pc["log_std_max"], action_scale=pc["action_scale"],
            hidden_activations=pc["hidden_layers_act"], output_activation=pc["output_activation"],
            seed=self.config["train"]["seed"]).to(self.device)

    def _init_optimizers(self) -> None:
        s = self.config["sac"]
        self.policy_optimizer = optim.Adam(self.policy_net.parameters(), lr=s["actor_lr"])
        self.q1_optimizer = optim.Adam(self.q_net1.parameters(), lr=s["critic_lr"])
        self.q2_optimizer = optim.Adam(self.q_net2.parameters(), lr=s["critic_lr"])

    def _set_seed(self, seed: int) -> None:
        np.random.seed(seed)
        torch.manual_seed(seed)
        random.seed(seed)
        self.env.reset(seed=seed)
        self.env.action_space.seed(seed)
        self.env.observation_space.seed(seed)

    def _build_engine(self) -> None:
        s, tr = self.config["sac"], self.config["train"]
        self.engine = SacEngine(
            self.policy_net, self.q_net1, self.q_net2, self.q_net1_target, self.q_net2_target,
            batch_size=tr["batch_size"], gamma=self._discount(), tau=s["tau"], actor_lr=s["actor_lr"],
            critic_lr=s["critic_lr"], alpha_lr=s["alpha_lr"], alpha=s["alpha"],
            auto_entropy_tuning=self._auto, device=self.device, precision=self.precision,
            seed=int(tr.get("engine_seed", tr["seed"])))
        eng = self.engine
        if self.bootstrap_truncated:  # at n > 1 the rollout kernel's rows go to the staging table, as end codes
            eng.set_done_mode(E.DONE_TERMINATED if self.n_step == 1 else E.DONE_END_CODE)
        # torch.optim.Adam objects whose state IS the engine's device state
        for opt, key in ((self.policy_optimizer, "pi"), (self.q1_optimizer, "q1"), (self.q2_optimizer, "q2")):
            ms, vs = eng.adam_views(key)
            for p, m, v in zip(eng.param_views(key), ms, vs):
                opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m, "exp_avg_sq": v}
        if self._auto:
            self.log_alpha = eng.alpha_state[0]
            self.alpha_optimizer = optim.Adam([self.log_alpha], lr=s["alpha_lr"])
            self.alpha_optimizer.state[self.log_alpha] = {
                "step": torch.tensor(0.0), "exp_avg": eng.alpha_state[2], "exp_avg_sq": eng.alpha_state[3]}

    def _discount(self) -> float:
        """The discount of the stored rows: sac.gamma, or gamma^n (``gpow[n]``) with train.n_step = n > 1."""
        return self.config["sac"]["gamma"] if self.n_step == 1 else self.gpow[self.n_step]

    def _new_stage(self, num_envs: int) -> Optional[NStepStage]:
        """The staging table of one loop run (None at n_step = 1: the loops store their rows directly)."""
        if self.n_step == 1:
            return None
        return NStepStage(self.n_step, num_envs, self.replay_buffer, self.config["sac"]["gamma"],
                          bootstrap_truncated=self.bootstrap_truncated)

    def _stored_done(self, terminated, truncated):
        """The ``done`` of a one-step row: ``terminated | truncated``, or ``terminated`` alone with
        train.bootstrap_truncated (scalars or arrays)."""
        return terminated if self.bootstrap_truncated else np.logical_or(terminated, truncated)

    def _engine(self) -> SacEngine:
        if self.engine is None:
            E.require_gpu(self.device)
        return self.engine

    @property
    def alpha(self) -> torch.Tensor:
        """Current temperature: float64 0-dim when auto-tuned (agent.py:50), fp32 otherwise."""
        if self._auto and self.engine is not None:
            return self.engine.alpha_state[1]
        return self._fixed_alpha

    # ------------------------------------------------------------------ data
    def store_transition(self, state: Any, action: Any, reward: float, next_state: Any, done: bool) -> None:
        refuse_n_step(self.n_step, "store_transition")
        self.replay_buffer.push(state, action, reward, next_state, done)

    def warmup_replay_buffer(self, env: Any, steps: int) -> None:
        refuse_n_step(self.n_step, "warmup_replay_buffer")
        state, _ = env.reset()
        for _ in range(steps):
            action = env.action_space.sample()
            next_state, reward, terminated, truncated, _ = env.step(action)
            done = terminated or truncated
            self.store_transition(state, action, reward, next_state, bool(self._stored_done(terminated, truncated)))
            state = next_state
            if done:
                state, _ = env.reset()

    def select_action(self, state: Any, deterministic: bool = False) -> Any:
        """Policy action for one observation (HIP policy kernel; agent.py:149-156)."""
        eng = self._engine()
        obs = torch.as_tensor(np.asarray(state, dtype=np.float32)).reshape(1, -1).to(self.device)
        if deterministic:
            act = eng.policy_act(obs)
        else:
            eps = torch.distributions.utils._standard_normal((1, self.action_size), torch.float32, self.device)
            act = eng.policy_act(obs, eps)
        return act.cpu().numpy()[0]

    def select_actions(self, states: Any, deterministic: bool = False) -> np.ndarray:
        """Policy actions for N observations [N, obs]: one H2D copy, ONE policy
        kernel, one D2H copy (the batched form of ``select_action``; row i draws
        its noise from the same torch generator stream as N single calls would
        for N = 1)."""
        eng = self._engine()
        host = np.ascontiguousarray(np.asarray(states, dtype=np.float32).reshape(-1, self.obs_size))
        obs = torch.from_numpy(host)
        if self.device.type == "cuda":
            obs = obs.pin_memory().to(self.device, non_blocking=True)
        if deterministic:
            act = eng.policy_act(obs)
        else:
            eps = torch.distributions.utils._standard_normal((host.shape[0], self.action_size), torch.float32,
                                                             self.device)
            act = eng.policy_act(obs, eps)
        return act.cpu().numpy()

    def q_values(self, states: Any, actions: Any, target: bool = False):
        """(q1, q2) of n (state, action) pairs as float32 arrays of length n:
        ONE launch of the critic-evaluation kernel on the weights the engine
        trains with (``target``: the target critics).  Host arrays go up
        through pinned memory; device tensors are read in place."""
        eng = self._engine()

        def rows(x, width):
            if isinstance(x, torch.Tensor):
                return x.detach().to(torch.float32).reshape(-1, width).to(self.device)
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, width)))
            return t.pin_memory().to(self.device, non_blocking=True) if self.device.type == "cuda" else t

        q = eng.q_values(rows(states, self.obs_size), rows(actions, self.action_size), target=target).cpu().numpy()
        return q[:, 0].copy(), q[:, 1].copy()

    def store_transitions(self, states: Any, actions: Any, rewards: Any, next_states: Any, dones: Any) -> None:
        """N transitions in env order: one pinned H2D copy + one push kernel."""
        self.replay_buffer.push_batch(states, actions, rewards, next_states, dones)

    def _run_updates(self, n: int) -> None:
        """n consecutive gradient steps (agent.py:361-364): one engine call, no
        host sync (device RNG); per-step calls in reference-RNG mode."""
        if n <= 0:
            return
        if self.rng_mode == "reference":
            for _ in range(n):
                self.training_step()
            return
        self.replay_buffer._check(self.config["train"]["batch_size"])
        if n >= self.graph_chunk:
            self._engine().train_graph(self.replay_buffer, n, self.graph_chunk)
        else:
            self._engine().train(self.replay_buffer, n)

    def can_update(self) -> bool:
        if self.config["train"]["warming_steps"] > self.config["buffer"]["capacity"]:
            print("Warning: warming_steps is greater than replay buffer capacity.")
        return len(self.replay_buffer) >= self.config["train"]["warming_steps"]

    def sample_batch(self) -> Transition:
        """Minibatch as device tensors (agent.py:166-193), reference RNG order."""
        return self.replay_buffer.sample_tensors(self.config["train"]["batch_size"])

    # ------------------------------------------------------------------ the hot path
    def _reference_rng_inputs(self):
        B, A = self.config["train"]["batch_size"], self.action_size
        idx = torch.tensor(self.replay_buffer.sample_indices(B), dtype=torch.int32)
        sn = torch.distributions.utils._standard_normal
        eps_t = sn((B, A), torch.float32, self.device)  # target rsample (agent.py:204)
        eps_a = sn((B, A), torch.float32, self.device)  # actor rsample (agent.py:241)
        return idx.reshape(1, B), torch.stack([eps_t, eps_a]).reshape(1, 2, B, A)

    def training_step(self):
        """One SAC gradient step on the engine (agent.py:302-327)."""
        eng = self._engine()
        if self.rng_mode == "reference":
            idx, eps = self._reference_rng_inputs()
            eng.train(self.replay_buffer, 1, indices=idx, eps=eps)
        else:
            self.replay_buffer._check(self.config["train"]["batch_size"])
            eng.train(self.replay_buffer, 1)

    def train_steps(self, n: int) -> None:
        """n consecutive gradient steps (device RNG) replayed from a hipGraph."""
        eng = self._engine()
        if self.rng_mode == "reference":
            for _ in range(n):
                self.training_step()
        else:
            self.replay_buffer._check(self.config["train"]["batch_size"])
            eng.train_graph(self.replay_buffer, n, self.graph_chunk)

    def _loss_log(self, active_logger) -> Optional[LossLog]:
        """logger.log_losses_every (default 1000 gradient steps; 0 = off)."""
        every = int(self.config["logger"].get("log_losses_every", 1000))
        if active_logger is None or self.engine is None or every <= 0 or not hasattr(active_logger, "log_scalar"):
            return None
        return LossLog(self.engine, active_logger, every)

    def _q_log(self, active_logger) -> Optional[QValueLog]:
        """logger.log_q_values: per-env-step Q values, flushed every
        logger.q_values_flush_every env steps (default 256) without host syncs."""
        if active_logger is None or not self.config["logger"]["log_q_values"]:
            return None
        return QValueLog(self, active_logger, int(self.config["logger"].get("q_values_flush_every", 256)))

    def last_losses(self) -> Dict[str, float]:
        """Losses of the last step (reads device memory: synchronises)."""
        l = self._engine().losses()
        return {"q1_loss": l[0], "q2_loss": l[1], "policy_loss": l[2], "alpha_loss": l[3],
                "alpha": float(self.alpha.item())}

    # Reference sub-steps (agent.py:195-300), unfused.  training_step() runs
    # them fused on the HIP engine; called one by one they keep the reference's
    # semantics on the engine's own state: the modules' parameters, the Adam
    # moments and log alpha ARE the engine's buffers, so these run as PyTorch
    # eager ops on the GPU (the reference's own code, not the hot path), with
    # the optimizer step counts taken from and returned to the engine and the
    # packed MFMA copies re-derived after each update (sync_params).
    # tests/test_gpu_substeps.py: the five composed == one fused step.
    def _opt_step(self, opt, idx: int) -> None:
        eng = self._engine()
        t = float(eng.opt_steps[idx].item())
        for st in opt.state.values():
            st["step"] = torch.tensor(t)
        opt.step()
        eng.opt_steps[idx] = t + 1.0

    def compute_target_q_values(self, rewards: Any, dones: Any, next_states: Any) -> Any:
        """y = r + gamma (1 - d)(min Q_t(s', a') - alpha log pi(a'|s')) (agent.py:195-211).
        ``d`` enters as the float it is, so the fractional ``done`` of train.bootstrap_truncated with
        n_step > 1 needs nothing else here."""
        self._engine()
        with torch.no_grad():
            alpha = self.alpha.detach()
            next_actions, next_log_pi = self.policy_net.sample_action(next_states)
            q1 = self.q_net1_target(next_states, next_actions)
            q2 = self.q_net2_target(next_states, next_actions)
            return rewards + self._discount() * (1 - dones) * (torch.min(q1, q2) - alpha * next_log_pi)

    def update_q_networks(self, states: Any, actions: Any, target_q_values: Any) -> None:
        """MSE critic losses, one Adam step per critic (agent.py:213-236)."""
        eng = self._engine()
        for net, opt, idx in ((self.q_net1, self.q1_optimizer, 1), (self.q_net2, self.q2_optimizer, 2)):
            loss = torch.nn.functional.mse_loss(net(states, actions), target_q_values)
            opt.zero_grad()
            loss.backward()
            self._opt_step(opt, idx)
        eng.sync_params()

    def update_policy_network(self, states: Any):
        """L_pi = mean(alpha log pi - min Q) through the current critics; returns log pi (agent.py:238-260)."""
        eng = self._engine()
        actions, log_pi = self.policy_net.sample_action(states)
        min_q = torch.min(self.q_net1(states, actions), self.q_net2(states, actions))
        policy_loss = (self.alpha.detach() * log_pi - min_q).mean()
        self.policy_optimizer.zero_grad()
        policy_loss.backward()
        self._opt_step(self.policy_optimizer, 0)
        for net in (self.q_net1, self.q_net2):  # the reference leaves critic grads behind; drop them
            net.zero_grad(set_to_none=True)
        eng.sync_params()
        return log_pi

    def update_entropy_temperature(self, log_pi: Any) -> Dict[str, float]:
        """Adam step on float64 log alpha (agent.py:263-280); {} when alpha is fixed."""
        eng = self._engine()
        if not self._auto:
            return {}
        term = (log_pi + self.target_entropy).detach()
        alpha_loss = -(self.log_alpha.to(term.dtype) * term).mean()
        if eng.alpha_updates:  # off after a reference-style load_agent (agent.py:550-554)
            self.log_alpha.grad = (-term.mean()).to(self.log_alpha.dtype).reshape(self.log_alpha.shape)
            self._opt_step(self.alpha_optimizer, 3)
            self.log_alpha.grad = None
            eng.alpha_state[1] = eng.alpha_state[0].exp()
        return {"alpha_loss": alpha_loss.item(), "alpha": self.alpha.item()}

    def soft_update_target_networks(self) -> None:
        """Polyak t <- tau p + (1 - tau) t (agent.py:282-300)."""
        eng = self._engine()
        tau = self.config["sac"]["tau"]
        with torch.no_grad():
            for tgt, src in ((self.q_net1_target, self.q_net1), (self.q_net2_target, self.q_net2)):
                for tp, sp in zip(tgt.parameters(), src.parameters()):
                    tp.data.copy_(tau * sp.data + (1.0 - tau) * tp.data)
        eng.sync_params()

    # ------------------------------------------------------------------ loops
    def _episode_stats(self, active_logger, print_rewards: bool) -> EpisodeStats:
        """logger.log_episode_stats: whether finished episodes go to the logger."""
        log = active_logger is not None and self.config["logger"]["log_episode_stats"]
        return EpisodeStats(active_logger if log else None, print_rewards)

    def _run_due(self, due: int, loss_log: Optional[LossLog], env_steps: int) -> int:
        """Run the ``due`` gradient steps of a vector step that ended at env
        step ``env_steps``, if ``can_update()`` holds, and let the loss log look
        at them.  Returns the number of gradient steps run (``due`` or 0)."""
        if not (self.can_update() and due):
            return 0
        self._run_updates(due)
        if loss_log is not None:
            loss_log.after_updates(env_steps)
        return due

    def _finish_loop(self, active_logger, stats: EpisodeStats, pending: tuple, **counters) -> Dict[str, float]:
        """The end of every training loop, in this order: raise if a hand-off
        timed out (an invalid run is not reported); ``finish`` each of
        ``pending`` (drains and logs, None skipped), which blocks and may still
        add episodes to ``stats``; build the metrics, ``counters`` after the
        episode statistics; ``log_hparams``.  Returns the metrics."""
        if self.engine is not None:
            self.engine.check()
        for log in pending:
            if log is not None:
                log.finish()
        metrics = {"total_episodes": stats.count, "best_avg_return": stats.best, "final_avg_return": stats.avg,
                   **counters}
        if active_logger is not None:
            active_logger.log_hparams(self.config, metrics)
        return metrics

    def run_training_loop(self, num_episodes: int, logger=None, tqdm_disable: bool = False,
                          print_rewards: bool = False) -> Dict[str, float]:
        refuse_n_step(self.n_step, "run_training_loop")
        active_logger = logger or self.logger
        total_steps = 0
        stats = self._episode_stats(active_logger, print_rewards)
        tr = self.config["train"]
        update_every = tr.get("update_frequency", 1)
        n_grad = tr.get("gradient_steps_per_update", 1)
        loss_log = self._loss_log(active_logger)
        q_log = self._q_log(active_logger)
        for _ in _tqdm(range(num_episodes), disable=tqdm_disable):
            state, _ = self.env.reset()
            done = False
            episode_return = 0.0
            episode_steps = 0
            while not done:
                action = self.select_action(state)
                next_state, reward, terminated, truncated, _ = self.env.step(action)
                done = terminated or truncated
                self.store_transition(state, action, reward, next_state,
                                      bool(self._stored_done(terminated, truncated)))
                state = next_state
                episode_return += reward
                episode_steps += 1
                total_steps += 1
                if self.can_update() and total_steps % update_every == 0:
                    self._run_updates(n_grad)
                    if loss_log is not None:
                        loss_log.after_updates(total_steps)
                if q_log is not None:  # Q(s', a) of this env step (agent.py:370-376), no host sync
                    q_log.record(state, action, total_steps)
            stats.episode(episode_return, episode_steps)
        metrics = self._finish_loop(active_logger, stats, (loss_log, q_log))
        if self.config["logger"]["save_model"]["enabled"]:
            save_path = self.config["logger"]["save_model"]["path"]
            if save_path is None:
                save_path = active_logger.run_dir
            else:
                os.makedirs(save_path, exist_ok=True)
            model_path = os.path.join(save_path, "sac_agent.pth")
            self.save_agent(model_path)
            print(f"Agent saved to {model_path}")
        if active_logger is not None and self.config["logger"]["log_episode_stats"]:
            from .utils.logger_utils import save_lengths, save_rewards

            save_rewards(active_logger.run_dir, active_logger.episode_rewards)
            save_lengths(active_logger.run_dir, active_logger.episode_lengths)
        return metrics

    def run_vectorized_training_loop(self, total_env_steps: int, vec_env: Any = None, logger=None,
                                     tqdm_disable: bool = True, print_rewards: bool = False,
                                     seed: Optional[int] = None,
                                     callback: Optional[Callable[[Dict[str, float]], None]] = None) -> Dict[str, float]:
        """Batched form of ``run_training_loop`` (agent.py:329-418) over a
        ``SyncVectorEnv`` of N envs.

        Per vector step: ONE policy kernel for the N actions, the N env steps on
        the host, ONE push of the N transitions, then every gradient step that
        fell due in those N env steps (``update_frequency`` /
        ``gradient_steps_per_update``, counted per env step exactly as the
        reference counts them) as ONE engine call: K steps per launch sequence,
        hipGraph replay when K >= graph_chunk, no host synchronisation.  With
        N = 1 it performs the reference loop's exact sequence of pushes,
        updates and RNG draws (tests/test_gpu_rollout.py).

        ``vec_env`` defaults to ``self.env`` (pass a ``SyncVectorEnv`` as the
        agent's env so ``_set_seed`` seeds env i with seed + i).  Stops after the
        first vector step that reaches ``total_env_steps``.

        ``callback`` (optional) is called after every vector step with the
        loop's host counters (``env_steps``, ``gradient_steps``, ``episodes``,
        ``avg_return`` over the last 100 episodes): the hook of
        ``sac.replicas.ReplicaAggregator`` (independent-seed replicas, one per
        GPU, sac/train_replicas.py).  It must not synchronise the device.

        ``train.n_step`` = n > 1: the N rows of a vector step go to a staging
        table (``sac.nstep.NStepStage``) and, from the n-th vector step on, one
        launch stores the N n-step rows of the window that just closed; the
        gradient steps are gated by ``due_updates_staged``.

        ``train.random_steps`` = K > 0: vector step v with v * N < K
        (``uniform_vector_step``) takes ``SacEngine.uniform_actions(N, v + 1)``
        instead of the policy's actions -- the draws the device loop takes with
        the same engine seed, bit for bit; nothing after the actions changes."""
        env = vec_env if vec_env is not None else self.env
        if not hasattr(env, "num_envs"):
            raise TypeError("run_vectorized_training_loop needs a vectorised env (sac.vector_env.SyncVectorEnv)")
        active_logger = logger or self.logger
        tr = self.config["train"]
        update_every = tr.get("update_frequency", 1)
        n_grad = tr.get("gradient_steps_per_update", 1)
        N = env.num_envs
        stage = self._new_stage(N)
        obs, _ = env.reset(seed=seed)
        if stage is not None:
            stage.clear()
        ep_ret = np.zeros(N, np.float64)
        ep_len = np.zeros(N, np.int64)
        stats = self._episode_stats(active_logger, print_rewards)
        total_steps = grad_steps = 0
        loss_log = self._loss_log(active_logger)
        q_log = self._q_log(active_logger)
        pbar = _tqdm(range((int(total_env_steps) + N - 1) // N), disable=tqdm_disable)
        for v in pbar:
            if uniform_vector_step(v, N, self.random_steps):
                actions = self._engine().uniform_actions(N, v + 1)
            else:
                actions = self.select_actions(obs)
            next_obs, rewards, terminated, truncated, info = env.step(actions)
            dones = np.logical_or(terminated, truncated)
            len_before = len(self.replay_buffer)
            emitted = N
            if stage is None:
                self.store_transitions(obs, actions, rewards, info["final_obs"],
                                       self._stored_done(terminated, truncated))
            else:  # the stage holds flags, or with train.bootstrap_truncated end codes
                stage.push(obs, actions, rewards, info["final_obs"],
                           end_codes(terminated, truncated) if self.bootstrap_truncated else dones)
                emitted = stage.emit()
            old = total_steps
            total_steps += N
            grad_steps += self._run_due(due_updates_staged(old, total_steps, emitted, len_before,
                                                           self.replay_buffer.capacity, tr["warming_steps"],
                                                           update_every, n_grad),
                                        loss_log, total_steps)
            if q_log is not None:  # env step old + 1 + i logs Q(s'_i, a_i) under the critics after this vector step
                q_log.record(info["final_obs"], actions, old + 1)
            ep_ret += rewards
            ep_len += 1
            for i in np.nonzero(dones)[0]:
                stats.episode(float(ep_ret[i]), int(ep_len[i]))
                ep_ret[i] = 0.0
                ep_len[i] = 0
            obs = next_obs
            if callback is not None:
                callback(stats.counters(total_steps, grad_steps))
        return self._finish_loop(active_logger, stats, (loss_log, q_log), total_env_steps=total_steps,
                                 gradient_steps=grad_steps)

    def _device_env(self, vec_env: Any, what: str):
        from .device_envs import DeviceVectorEnv

        env = vec_env if vec_env is not None else self.env
        if not isinstance(env, DeviceVectorEnv):
            raise TypeError(f"{what} needs a sac.device_envs.DeviceVectorEnv (a probe environment of sac.envs or "
                            "a control task of sac.control_envs resident on the device); other environments run "
                            "through run_vectorized_training_loop")
        return env

    def run_device_training_loop(self, total_env_steps: int, vec_env: Any = None, logger=None,
                                 print_rewards: bool = False, seed: Optional[int] = None,
                                 callback: Optional[Callable[[Dict[str, float]], None]] = None,
                                 drain_every: int = 64, device_q_values: bool = False,
                                 graph_steps: int = 0) -> Dict[str, float]:
        """``run_vectorized_training_loop`` over a ``DeviceVectorEnv``: the envs
        live on the device and act -> step -> store is ONE launch
        (``SacEngine.rollout_step``), so a vector step is that launch plus the
        gradient steps that fell due -- gated and counted exactly as in the
        vectorised loop (``due_updates_gated``, ``can_update``, ``_run_updates``,
        the loss log, the callback) -- with no host<->device copy, no ``.cpu()``,
        no ``.item()`` and no synchronisation per step.

        Episode returns and lengths are accumulated on the device and written
        to the envs' episode ring; every ``drain_every`` vector steps the new
        cells are copied to pinned memory behind the launches and consumed once
        the copy has landed (``sac.device_envs.EpisodeDrain``, on the copies
        of ``sac.copy_behind``), and after the last step the rest is consumed blocking.  So
        the returned metrics and the logged episodes are exact and in the
        order the host loop sees them, (vector step, env row); but the
        ``episodes`` and ``avg_return`` a ``callback`` sees inside the loop may
        lag the device by up to ``drain_every`` vector steps (plus the copy in
        flight).  ``drain_every`` is capped at the ring's length.

        Actions are sampled with the engine's device RNG (Philox, ``which`` =
        2), not torch's generator, so a seeded run differs from the vectorised
        loop's in its noise draws, not in distribution.

        ``logger.log_q_values``: the host ``QValueLog`` evaluates the critics
        per env step on host inputs, which this loop does not have, so by
        default a config with it on is refused (ValueError).  With
        ``device_q_values=True`` the values are logged on the device instead
        (``sac.device_envs.DeviceQValueLog``): after each vector step's
        gradient steps ONE launch of the critic-evaluation kernel reads the N
        transitions just written from the replay ring and writes Q1 / Q2 of
        (final_obs_i, a_i) into a device ring, drained every ``drain_every``
        vector steps like the episodes -- the quantity the vectorised loop
        logs, from the packed weights the engine trains with (in bf16 mode
        those are the bf16 copies, not the fp32 eager forward).  With the
        config key off, ``device_q_values`` logs and launches nothing.

        ``graph_steps = K`` (even, >= 2; 0 = off, the loop above unchanged):
        whole blocks of K vector steps -- rollout, the gradient steps due after
        each (``plan_graph_block``), the Q-value launch -- are ONE hipGraph
        replay (``SacEngine.loop_graph``) with the loop cursor (replay size,
        write slot, step number) kept on the device, so a block costs the host
        one call.  A block goes through the graph when K whole vector steps
        remain, the warm-up is over and every gradient step finds a full batch
        (``graph_block_ready``), and its gradient-step pattern is the captured
        one; a new pattern captures again, at most ``MAX_RECAPTURES`` times.
        Every other block (warm-up, another pattern after that, the tail) runs
        stepwise as above, and the device cursor is re-seeded from the host
        mirrors before the next graph block (one asynchronous copy).  The
        results are those of ``graph_steps = 0`` bit for bit.  The loss log,
        the episode drain, the Q-value drain, the status poll and ``callback``
        run once per block: a callback sees ``env_steps`` advance by K * N.
        Needs ``K + drain_every <= `` the episode ring's (and the Q ring's)
        steps, and the device RNG (``rng_mode`` "reference" feeds the gradient
        step from the host): otherwise ValueError before any launch.

        ``train.n_step`` = n > 1: the step is ``SacEngine.rollout_step_nstep``
        -- the same fused launch into a staging table plus one launch that
        stores the n-step rows -- gated by ``due_updates_staged``.
        ``graph_steps`` > 0 and ``device_q_values=True`` are refused (the loop
        graph needs a second cursor for the staging table).

        ``train.random_steps`` = K > 0: the engine's action source is
        ``E.ACTIONS_UNIFORM`` for the vector steps v with v * N < K
        (``uniform_vector_step``) and ``E.ACTIONS_POLICY`` afterwards, set at
        the boundary only and back to the policy when the loop leaves, however
        it leaves.  Gating, the n-step stage, the done mode, the Q-value log
        and the drains are as without it.  With ``graph_steps`` a block goes
        through the graph only if none of its steps is uniform
        (``graph_block_policy_only``); earlier blocks run stepwise."""
        from .device_envs import DeviceQValueLog, EpisodeDrain

        if graph_steps:
            refuse_n_step(self.n_step, "graph_steps")
        if device_q_values:
            refuse_n_step(self.n_step, "device_q_values")
        if self.config["logger"]["log_q_values"]:
            refuse_n_step(self.n_step, "logger.log_q_values in run_device_training_loop")
        env = self._device_env(vec_env, "run_device_training_loop")
        K = int(graph_steps)
        if K:
            if K < 2 or K % 2:
                raise ValueError(f"graph_steps must be 0 or an even number >= 2 (the device cursor alternates between "
                                 f"two slots); got {graph_steps}")
            if self.rng_mode == "reference":
                raise ValueError("graph_steps needs the device RNG: rng_mode 'reference' draws every gradient step's "
                                 "indices and noise on the host")
            if K + max(1, int(drain_every)) > env.ring_steps:
                raise ValueError(f"graph_steps ({K}) + drain_every ({max(1, int(drain_every))}) exceeds the episode "
                                 f"ring's {env.ring_steps} steps: a block would overwrite cells not yet copied")
            if device_q_values and (logger or self.logger) is not None and self.config["logger"]["log_q_values"] \
                    and K + max(1, int(drain_every)) > DeviceQValueLog.RING_STEPS:
                raise ValueError(f"graph_steps ({K}) + drain_every ({max(1, int(drain_every))}) exceeds the Q-value "
                                 f"ring's {DeviceQValueLog.RING_STEPS} steps")
        if self.config["logger"]["log_q_values"] and not device_q_values:
            raise ValueError("run_device_training_loop does not support logger.log_q_values through the host path "
                             "(per-env-step Q values need the transitions on the host); pass device_q_values=True "
                             "to log them on the device, use run_vectorized_training_loop, or turn it off")
        eng = self._engine()
        active_logger = logger or self.logger
        tr = self.config["train"]
        update_every = tr.get("update_frequency", 1)
        n_grad = tr.get("gradient_steps_per_update", 1)
        N = env.num_envs
        stage = self._new_stage(N)
        env.reset(seed=seed)
        if stage is not None:
            stage.clear()
        stats = self._episode_stats(active_logger, print_rewards)
        total_steps = grad_steps = 0
        loss_log = self._loss_log(active_logger)
        drain = EpisodeDrain(env, stats.episode, drain_every)
        q_log = None
        if device_q_values and active_logger is not None and self.config["logger"]["log_q_values"]:
            # with the graph, cell = RNG step % S on both paths: the graph's kernel indexes its cell that way
            q_log = DeviceQValueLog(eng, self.replay_buffer, N, active_logger, drain_every,
                                    first_cell=env.t + 1 if K else 0)
        vec_steps = (int(total_env_steps) + N - 1) // N
        rb, cap, warming = self.replay_buffer, self.replay_buffer.capacity, tr["warming_steps"]

        def source(v: int) -> None:
            """The engine's action source for vector step ``v``: a call into the engine at the boundary only."""
            want = E.ACTIONS_UNIFORM if uniform_vector_step(v, N, self.random_steps) else E.ACTIONS_POLICY
            if eng.action_source != want:
                eng.set_action_source(want)

        def step(due: int) -> None:
            """One vector step issued from the host, with ``due`` gradient steps after it."""
            nonlocal total_steps, grad_steps
            if q_log is not None:
                rb.flush()  # rows pushed from the host go in first: they move the write slot
            first_slot = rb._pos  # the step's N rows go to ring slots first_slot + i
            source(total_steps // N)
            eng.rollout_step(env, rb)
            total_steps += N
            grad_steps += self._run_due(due, loss_log, total_steps)
            if q_log is not None:  # env step first + i logs Q(s'_i, a_i) under the critics after this vector step
                q_log.after_step(first_slot, total_steps - N + 1)

        def report() -> None:
            drain.after_step()
            if callback is not None:
                callback(stats.counters(total_steps, grad_steps))

        try:
            if K:
                cursor, policy, seeded, done = eng.loop_cursor(), GraphBlockPolicy(), False, 0
                batch = tr["batch_size"]
                while done < vec_steps:
                    counts = plan_graph_block(total_steps, len(rb), cap, warming, update_every, n_grad, N, K)
                    if vec_steps - done >= K and graph_block_policy_only(done, N, self.random_steps) \
                            and graph_block_ready(counts, len(rb), cap, warming, batch, N) and policy.admit(counts):
                        if not seeded:  # the last block moved the host mirrors only
                            eng.seed_cursor(cursor, env, rb)
                            seeded = True
                        source(done)
                        eng.loop_graph(env, rb, cursor, counts, 1, None if q_log is None else q_log.ring)
                        if q_log is not None:
                            q_log.after_graph(K, total_steps + 1)
                        total_steps += K * N
                        grad_steps += sum(counts)
                        if loss_log is not None and sum(counts):
                            loss_log.after_updates(total_steps)
                        done += K
                    else:
                        seeded = False
                        for due in counts[:vec_steps - done]:
                            step(due)
                            done += 1
                    report()
            elif stage is not None:  # train.n_step > 1: the rows of a vector step are stored n - 1 steps late
                for v in range(vec_steps):
                    len_before = len(rb)
                    source(v)
                    emitted = eng.rollout_step_nstep(env, stage)
                    total_steps += N
                    grad_steps += self._run_due(due_updates_staged(total_steps - N, total_steps, emitted, len_before,
                                                                   cap, warming, update_every, n_grad), loss_log,
                                                total_steps)
                    report()
            else:
                for _ in range(vec_steps):
                    step(due_updates_gated(total_steps, total_steps + N, len(rb), cap, warming, update_every, n_grad))
                    report()
        finally:  # the source is the loop's, not the engine's: evaluation and later runs start from the policy
            if eng.action_source != E.ACTIONS_POLICY:
                eng.set_action_source(E.ACTIONS_POLICY)
        return self._finish_loop(active_logger, stats, (drain, loss_log, q_log), total_env_steps=total_steps,
                                 gradient_steps=grad_steps)

    def evaluate_device(self, num_episodes: Optional[int] = None, vec_env: Any = None,
                        episodes_per_env: Optional[int] = None) -> float:
        """Mean return of the deterministic policy (tanh(mu) * scale) on a
        ``DeviceVectorEnv``.  Exactly one count is given.  ``num_episodes``: the
        first ``num_episodes`` episodes that finish, counted in (vector step, env
        row) order -- exact where every episode has the same length, biased
        toward short episodes where lengths vary.  ``episodes_per_env = k``:
        each env row's first ``k`` episodes (``first_episodes_per_row``), the
        rule for tasks that end by failure; at most ``k * max_steps`` vector
        steps.  Nothing is stored: the replay buffer and its device state are
        untouched.  The envs are reset first; one blocking read of the episode
        ring per ring length."""
        from .device_envs import EpisodeDrain, first_episodes_per_row

        if (num_episodes is None) == (episodes_per_env is None):
            raise ValueError("evaluate_device takes exactly one of num_episodes and episodes_per_env")
        env = self._device_env(vec_env, "evaluate_device")
        per_row = episodes_per_env is not None
        if per_row:
            k = int(episodes_per_env)
            if k < 1:
                raise ValueError("episodes_per_env must be >= 1")
        elif num_episodes < 1:
            raise ValueError("num_episodes must be >= 1")
        eng = self._engine()
        env.reset()
        episodes: list = []  # (vector step, env row, return) in the order they ended
        ended = [0] * env.num_envs

        def at(t, row, ret, length):
            episodes.append((t, row, ret))
            ended[row] += 1

        drain = EpisodeDrain(env, None, env.ring_steps, on_episode_at=at)
        # every row ends an episode at least once per max_steps vector steps
        rounds = 1 if per_row else (num_episodes + env.num_envs - 1) // env.num_envs
        chunk = max(1, min(env.ring_steps, env.max_steps * rounds))
        while (min(ended) < k) if per_row else (len(episodes) < num_episodes):
            for _ in range(chunk):
                eng.rollout_step(env, self.replay_buffer, deterministic=True, store=False)
            drain.finish()
        if per_row:
            return float(np.mean(first_episodes_per_row(episodes, env.num_envs, k)))
        return float(np.mean([ret for _, _, ret in episodes[:num_episodes]]))

    def eval_agent(self, num_episodes: int, render_mode: Optional[str] = None, tqdm_disable: bool = False,
                   print_returns: bool = False, writer=None) -> float:
        eval_env = self._get_render_environment(render_mode)
        total_return = 0.0
        for episode in _tqdm(range(num_episodes), disable=tqdm_disable):
            state, _ = eval_env.reset()
            done = False
            episode_return = 0.0
            length = 0
            while not done:
                action = self.select_action(state, deterministic=True)
                next_state, reward, terminated, truncated, _ = eval_env.step(action)
                done = terminated or truncated
                state = next_state
                episode_return += reward
                length += 1
            total_return += episode_return
            if print_returns:
                print(f"Evaluation Episode {episode}, Return: {episode_return:.2f}")
            if writer is not None:
                writer.add_scalar("Eval/Episode/Return", episode_return, episode)
                writer.add_scalar("Eval/Episode/Length", length, episode)
        avg_return = total_return / num_episodes
        if print_returns:
            print(f"Average Return over {num_episodes} episodes: {avg_return:.2f}")
        if eval_env is not self.env:
            eval_env.close()
        return avg_return

    def _get_render_environment(self, render_mode: Optional[str]):
        if render_mode is None or getattr(self.env, "render_mode", None) == render_mode:
            return self.env
        spec = getattr(self.env, "spec", None)
        if spec is not None and getattr(spec, "id", None):
            try:
                import gymnasium as gym

                print(f"Creating new environment for evaluation with render_mode='{render_mode}'")
                eval_env = gym.make(spec.id, render_mode=render_mode)
                seed = self.config["train"].get("seed")
                if seed is not None:
                    eval_env.reset(seed=seed)
                    eval_env.action_space.seed(seed)
                return eval_env
            except Exception as e:  # noqa: BLE001 - same behaviour as the reference
                print(f"Warning: Failed to create new env for rendering: {e}. Using original env.")
                return self.env
        print("Warning: Cannot create new env for rendering as env.spec.id is not available. Using original env.")
        return self.env

    def _log_q_values(self, states: Any, actions: Any, logger, step: int) -> None:
        with torch.no_grad():
            q1 = self.q_net1(states, actions)
            q2 = self.q_net2(states, actions)
            logger.log_q_values(q1.mean().item(), q2.mean().item(), step)

    def _infer_env_name(self, env) -> str:
        spec = getattr(env, "spec", None)
        if spec is not None and getattr(spec, "id", None):
            return spec.id
        return env.__class__.__name__

    def show_config(self, indent: int = 4) -> None:
        pprint.PrettyPrinter(indent=indent).pprint(self.config)

    def print_net_architectures(self) -> None:
        print("Policy Network Architecture:")
        print(self.policy_net)
        print("\nQ-Network 1 Architecture:")
        print(self.q_net1)
        print("\nQ-Network 2 Architecture:")
        print(self.q_net2)

    # ------------------------------------------------------------------ checkpoints
    def _export_steps(self) -> None:
        if self.engine is None:
            return
        steps = self.engine.opt_steps.cpu().tolist()
        for opt, i in ((self.policy_optimizer, 0), (self.q1_optimizer, 1), (self.q2_optimizer, 2),
                       (self.alpha_optimizer, 3)):
            if opt is None:
                continue
            for st in opt.state.values():
                st["step"] = torch.tensor(float(steps[i]))

    def save_agent(self, filepath: str) -> None:
        """Same checkpoint dict as the reference (agent.py:521-536).  Raises
        HandoffTimeout instead of saving a state an invalid step produced."""
        if self.engine is not None:
            self.engine.check()
        self._export_steps()
        ckpt = {
            "policy_net_state_dict": self.policy_net.state_dict(),
            "q_net1_state_dict": self.q_net1.state_dict(),
            "q_net2_state_dict": self.q_net2.state_dict(),
            "q_net1_target_state_dict": self.q_net1_target.state_dict(),
            "q_net2_target_state_dict": self.q_net2_target.state_dict(),
            "policy_optimizer_state_dict": self.policy_optimizer.state_dict(),
            "q1_optimizer_state_dict": self.q1_optimizer.state_dict(),
            "q2_optimizer_state_dict": self.q2_optimizer.state_dict(),
        }
        if self._auto:
            ckpt["log_alpha"] = self.log_alpha.detach().clone()
            ckpt["alpha_optimizer_state_dict"] = self.alpha_optimizer.state_dict()
        torch.save(ckpt, filepath)

    def _import_opt(self, opt, sd, key: Optional[str], step_idx: int) -> None:
        """Load a torch Adam state_dict into the engine-owned moment buffers."""
        eng = self.engine
        params = list(opt.param_groups[0]["params"])
        for g, gsd in zip(opt.param_groups, sd["param_groups"]):
            for k, v in gsd.items():
                if k != "params":
                    g[k] = v
        steps = []
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            cur = opt.state[p]
            if st is None:
                cur["exp_avg"].zero_()
                cur["exp_avg_sq"].zero_()
                steps.append(0.0)
                continue
            cur["exp_avg"].copy_(st["exp_avg"].reshape(cur["exp_avg"].shape))
            cur["exp_avg_sq"].copy_(st["exp_avg_sq"].reshape(cur["exp_avg_sq"].shape))
            steps.append(float(st["step"]))
        if eng is not None and steps:
            eng.opt_steps[step_idx] = max(steps)

    def load_agent(self, filepath: str) -> None:
        """Load a reference-format checkpoint (agent.py:538-554).

        Loaded with ``weights_only=True``: checkpoints are plain tensors/dicts."""
        ckpt = torch.load(filepath, map_location=self.device, weights_only=True)
        self.policy_net.load_state_dict(ckpt["policy_net_state_dict"])
        self.q_net1.load_state_dict(ckpt["q_net1_state_dict"])
        self.q_net2.load_state_dict(ckpt["q_net2_state_dict"])
        self.q_net1_target.load_state_dict(ckpt["q_net1_target_state_dict"])
        self.q_net2_target.load_state_dict(ckpt["q_net2_target_state_dict"])
        if self.engine is None:
            self.policy_optimizer.load_state_dict(ckpt["policy_optimizer_state_dict"])
            self.q1_optimizer.load_state_dict(ckpt["q1_optimizer_state_dict"])
            self.q2_optimizer.load_state_dict(ckpt["q2_optimizer_state_dict"])
            return
        self._import_opt(self.policy_optimizer, ckpt["policy_optimizer_state_dict"], "pi", 0)
        self._import_opt(self.q1_optimizer, ckpt["q1_optimizer_state_dict"], "q1", 1)
        self._import_opt(self.q2_optimizer, ckpt["q2_optimizer_state_dict"], "q2", 2)
        if self._auto and "log_alpha" in ckpt:
            la = ckpt["log_alpha"].detach().to(torch.float64).reshape(())
            self.engine.alpha_state[0] = la
            self.engine.alpha_state[1] = la.exp()
            if "alpha_optimizer_state_dict" in ckpt:
                self._import_opt(self.alpha_optimizer, ckpt["alpha_optimizer_state_dict"], None, 3)
            # The reference rebinds self.log_alpha to the checkpoint's tensor but
            # leaves alpha_optimizer bound to the old one (agent.py:550-554): from
            # here on its steps still compute L_alpha, but log_alpha, alpha and the
            # alpha optimizer state stay as loaded.  Reproduced by default
            # (pinned by tests/golden/ref_ckpt_*.npz); train.alpha_after_load:
            # "tune" keeps tuning the loaded log_alpha instead.
            mode = self.config["train"].get("alpha_after_load", "reference")
            if mode not in ("reference", "tune"):
                raise ValueError("train.alpha_after_load must be 'reference' or 'tune'")
            self.engine.set_alpha_update(mode == "tune")
        self.engine.sync_params()
