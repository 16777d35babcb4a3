"""n-step returns for the vectorised and device-resident loops (``train.n_step``).

By default the stored ``done`` is ``terminated | truncated``, so a window that
an episode end closes never bootstraps and one that stays open spans n steps:
an n-step row is an ordinary replay row trained with the constant discount
gamma^n.  With ``x_s = (o_s, a_s, r_s, o'_s, d_s)`` the
one-step rows of one environment for consecutive vector steps, the n-step row
opened at s is ``(o_s, a_s, R, o'_{s+k-1}, d_{s+k-1})``: k is the smallest j + 1
(0 <= j < n) with ``d_{s+j} = 1``, or n; ``R = gpow[0] r_s + ... + gpow[k-1]
r_{s+k-1}`` in float64, accumulated in that order from the first product and
rounded to fp32 once.

With ``train.bootstrap_truncated`` the staged ``done`` is the
END CODE ``c = terminated + 2 * truncated`` in {0, 1, 2, 3}.  Any non-zero code
closes the window as above (k, R and ``next_obs`` do not change); the stored
``done`` is ``+0.0`` if no row of the window ended, ``1.0`` if the closing step
terminated (code 1 or 3), and ``fp32(1.0 - gpow[k] / gpow[n])`` -- float64, one
rounding, ``+0.0`` at k = n and negative below -- if the time limit alone closed
it (code 2).  The gradient step computes ``y = r + (gamma^n (1 - d)) (...)``, so
such a row bootstraps with gamma^k from its true next state.

* ``discount_powers`` / ``nstep_rows`` (``codes=True``: from end codes): the
  definition in plain Python and numpy.
* ``NStepStage``: the last n vector steps' one-step rows in a staging
  ``ReplayBuffer`` of n * N rows, and ONE launch per vector step
  (``torch.ops.sac_hip.replay_emit_nstep``) that writes the N n-step rows of the
  window that just closed into the training replay buffer.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from ._engine import NSTEP_MAX, ops
from .replay_buffer import ReplayBuffer


def check_n_step(n, key: str = "train.n_step") -> int:
    """``n`` as an int in 1..NSTEP_MAX, or ValueError naming ``key``."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= NSTEP_MAX:
        raise ValueError(f"{key} must be an integer in 1..{NSTEP_MAX}, got {n!r}")
    return int(n)


def n_step_refusal(n: int, what: str) -> str:
    return (f"train.n_step = {n}: {what} stores one-step rows or replays the loop graph, which n-step returns "
            "(train.n_step > 1) do not support; they run through run_vectorized_training_loop and "
            "run_device_training_loop(graph_steps=0)")


def refuse_n_step(n: int, what: str) -> None:
    """ValueError naming train.n_step if ``what`` is asked for with n > 1."""
    if n > 1:
        raise ValueError(n_step_refusal(n, what))


def discount_powers(gamma: float, n: int) -> List[float]:
    """``[1.0, g, g*g, ...]`` of length n + 1 by repeated multiplication in
    Python floats (float64), not ``g ** j``: ``gpow[1] == gamma`` exactly and
    ``gpow[n]`` is the discount the engine trains n-step rows with."""
    g = float(gamma)
    gpow = [1.0]
    for _ in range(int(n)):
        gpow.append(gpow[-1] * g)
    return gpow


def end_codes(terminated, truncated) -> np.ndarray:
    """``terminated + 2 * truncated`` as fp32: the end codes of a staging table."""
    return (np.asarray(terminated, bool).astype(np.float32)
            + np.float32(2.0) * np.asarray(truncated, bool).astype(np.float32))


def nstep_rows(obs, act, rew, next_obs, done, gpow, codes: bool = False):
    """The n-step rows (n = len(gpow) - 1) of one-step rows ``[T][N][...]``
    (``rew`` and ``done`` ``[T][N]``): ``(obs, act, rew, next_obs, done)`` of
    shape ``[T - n + 1][N][...]``, fp32, window s built from steps s .. s + n - 1.
    T < n gives no rows.  ``codes``: ``done`` holds end codes (``end_codes``) and
    the rows' done is 0, 1 or ``fp32(1 - gpow[k] / gpow[n])`` (module docstring)."""
    n = len(gpow) - 1
    obs, act, next_obs = (np.asarray(x, np.float32) for x in (obs, act, next_obs))
    rew = np.asarray(rew, np.float32)
    done = np.asarray(done, np.float32)
    T, N = rew.shape
    W = max(0, T - n + 1)
    acc = float(gpow[0]) * rew[:W].astype(np.float64)
    last = np.zeros((W, N), np.int64)  # k - 1: the window step whose next_obs and done the row takes
    opened = done[:W] == 0
    for j in range(1, n):
        acc = np.where(opened, acc + float(gpow[j]) * rew[j:j + W].astype(np.float64), acc)
        last = np.where(opened, j, last)
        opened = opened & (done[j:j + W] == 0)
    step = np.arange(W)[:, None] + last
    row = np.broadcast_to(np.arange(N)[None, :], (W, N))
    dlast = done[step, row]
    if codes:
        share = 1.0 - np.asarray(gpow, np.float64)[last + 1] / float(gpow[n])  # k = last + 1
        dlast = np.where(dlast == 0, np.float32(0.0),
                         np.where(dlast == 2, share.astype(np.float32), np.float32(1.0))).astype(np.float32)
    return (obs[:W].copy(), act[:W].copy(), acc.astype(np.float32), next_obs[step, row], dlast)


class NStepStage:
    """The staging table of one loop run: ``push`` (host rows) or
    ``after_rollout`` (rows the fused rollout kernel wrote into ``buffer``)
    count a vector step, ``emit`` then writes the N n-step rows of the window
    that closed with it into ``replay`` -- nothing for the first n - 1 vector
    steps after ``clear()``.  ``staged`` counts the vector steps since then."""

    def __init__(self, n: int, num_envs: int, replay: ReplayBuffer, gamma: float, bootstrap_truncated: bool = False):
        self.n = check_n_step(n, "n")
        # the table's done column holds end codes (``end_codes``; the rollout kernel in DONE_END_CODE mode)
        self.bootstrap_truncated = bool(bootstrap_truncated)
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.replay = replay
        self.gpow = discount_powers(gamma, self.n)
        # allocated on first use, with the environments' dims
        self.buffer = ReplayBuffer(self.n * self.num_envs, device=replay.device, layout=replay.layout)
        self.clear()

    def clear(self) -> None:
        """Forget the staged steps: the environments were reset, so the next n
        - 1 vector steps emit nothing."""
        self.staged = 0
        self._emitted_at = 0
        self._base = 0
        self._last_t: Optional[int] = None

    @property
    def newest(self) -> int:
        """Staging slot of environment 0's row of the newest vector step."""
        return (self.buffer._pos - self.num_envs) % self.buffer.capacity

    def _count(self, t: Optional[int]) -> None:
        buf, N = self.buffer, self.num_envs
        if self.staged == 0:
            self._base = self.newest
        elif t is not None and self._last_t is not None and t != self._last_t + 1:
            raise ValueError(f"NStepStage: vector step {t} does not follow step {self._last_t}: the environments "
                             "were reset without clear()")
        self.staged += 1
        self._last_t = t
        if self._base % N or buf._pos != (self._base + self.staged * N) % buf.capacity \
                or buf._size < min(buf.capacity, self.staged * N):
            raise ValueError(f"NStepStage: the staging buffer (size {buf._size}, write slot {buf._pos}) does not hold "
                             f"{self.staged} consecutive vector steps of {N} rows: something else wrote to it")

    def push(self, states, actions, rewards, next_states, dones, t: Optional[int] = None) -> None:
        """Stage one host vector step (the arguments of ``SAC.store_transitions``;
        N rows in environment order; with ``bootstrap_truncated`` ``dones`` are
        the step's ``end_codes``).  ``t``: the environments' step counter after
        it, if they keep one."""
        if np.asarray(rewards).reshape(-1).shape[0] != self.num_envs:
            raise ValueError(f"NStepStage.push takes one vector step of {self.num_envs} rows")
        if self.bootstrap_truncated:  # the codes as the floats they are, not as flags
            self.buffer.push_batch(states, actions, rewards, next_states, dones, done_values=True)
        else:
            self.buffer.push_batch(states, actions, rewards, next_states, dones)
        self._count(t)

    def after_rollout(self, t: Optional[int] = None) -> None:
        """Count a device vector step the rollout kernel wrote into ``buffer``
        (``t``: the environments' ``t`` after it)."""
        self._count(t)

    def _launch(self, newest: int) -> None:
        rb, buf = self.replay, self.buffer
        with torch.cuda.device(rb.device):
            if self.bootstrap_truncated:
                ops().replay_emit_nstep_codes(rb.storage, rb.state, rb.layout_spec, buf.storage, buf.state,
                                              buf.layout_spec, self.n, self.num_envs, newest, self.gpow[:self.n + 1],
                                              rb._size, rb._pos)
            else:
                ops().replay_emit_nstep(rb.storage, rb.state, rb.layout_spec, buf.storage, buf.state, buf.layout_spec,
                                        self.n, self.num_envs, newest, self.gpow[:self.n], rb._size, rb._pos)

    def emit(self) -> int:
        """Write the n-step rows of the window the newest staged step closed:
        one launch, and ``replay``'s host (size, pos) advance as a push of N rows
        does.  Returns the rows emitted: N, or 0 while fewer than n steps are
        staged (or the newest step's window has been emitted already)."""
        if self.staged < self.n or self._emitted_at == self.staged:
            return 0
        rb, buf, N = self.replay, self.buffer, self.num_envs
        if not rb._alloc_done:
            rb._alloc(buf.obs_dim, buf.act_dim)
        rb.flush()
        if N > rb.capacity:
            raise ValueError(f"NStepStage: num_envs ({N}) exceeds the replay capacity ({rb.capacity})")
        self._launch(self.newest)
        rb._size = min(rb.capacity, rb._size + N)
        rb._pos = (rb._pos + N) % rb.capacity
        self._emitted_at = self.staged
        return N
