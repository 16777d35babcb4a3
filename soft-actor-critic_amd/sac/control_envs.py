"""Control tasks: environments that need a bootstrapping critic and a policy of
a multi-dimensional state, unlike the closed-form probes of ``sac/envs.py``
(which stays the mirror of the reference's file).

``PendulumEnv`` is the classic pendulum swing-up, restated here from its
equations (gymnasium is not needed): a rod of mass ``m`` and length ``l``
hanging from a pivot, angle ``th`` measured from upright, one torque ``u``:

    u      = clip(a, -max_torque, max_torque)
    an     = ((th + pi) % (2 pi)) - pi
    reward = -(an^2 + 0.1 thdot^2 + 0.001 u^2)            (the pre-step state)
    thdot' = clip(thdot + (3 g / (2 l) sin th + 3 / (m l^2) u) dt, -8, 8)
    th'    = th + thdot' dt
    obs    = float32 [cos th', sin th', thdot']

It never terminates and is truncated after ``max_steps`` steps; ``reset`` draws
``th ~ U(-pi, pi)``, ``thdot ~ U(-1, 1)``.  The per-step cost is at most
pi^2 + 0.1 * 64 + 0.001 * max_torque^2 (16.27 at the default torque), so a
200-step return lies in [-3255, 0]; a policy that swings up and balances
reaches about -150.

The device-resident form (``sac.device_envs.DeviceVectorEnv("pendulum", N)``,
``SAC_ENV_PENDULUM`` of include/sac_engine.h) computes the same float64
arithmetic in the same order; only its ``sin`` / ``cos`` (the device library's,
not the host libm's) and its reset draws (Philox instead of numpy's generator)
differ.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .envs import Box, _Env


class PendulumEnv(_Env):
    """Pendulum swing-up; ``state`` = [th, thdot] as Python floats (settable)."""

    g = 10.0
    m = 1.0
    l = 1.0  # noqa: E741
    max_speed = 8.0

    def __init__(self, max_steps: int = 200, dt: float = 0.05, max_torque: float = 2.0):
        super().__init__()
        self.max_steps = int(max_steps)
        self.dt = float(dt)
        self.max_torque = float(max_torque)
        self.action_space = Box(low=-self.max_torque, high=self.max_torque, shape=(1,), dtype=np.float32)
        high = np.array([1.0, 1.0, self.max_speed], dtype=np.float32)
        self.observation_space = Box(low=-high, high=high, shape=(3,), dtype=np.float32)
        self.current_step = 0
        self.state = [0.0, 0.0]
        self.episode_reward = 0.0

    @staticmethod
    def angle_normalize(th: float) -> float:
        return ((th + math.pi) % (2 * math.pi)) - math.pi

    def _obs(self) -> np.ndarray:
        th, thdot = self.state
        return np.array([math.cos(th), math.sin(th), thdot], dtype=np.float32)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        super().reset(seed=seed)
        self.current_step, self.episode_reward = 0, 0.0
        th = float(self.np_random.uniform(low=-math.pi, high=math.pi))
        thdot = float(self.np_random.uniform(low=-1.0, high=1.0))
        self.state = [th, thdot]
        return self._obs(), {}

    def step(self, action):
        self.current_step += 1
        th, thdot = float(self.state[0]), float(self.state[1])
        g, m, l, dt = self.g, self.m, self.l, self.dt  # noqa: E741
        u = float(np.clip(np.float32(action[0]), self.action_space.low[0], self.action_space.high[0]))
        an = self.angle_normalize(th)
        reward = -(an * an + 0.1 * thdot * thdot + 0.001 * u * u)
        thdot = thdot + (3 * g / (2 * l) * math.sin(th) + 3 / (m * l * l) * u) * dt
        thdot = min(max(thdot, -self.max_speed), self.max_speed)
        th = th + thdot * dt
        self.state = [th, thdot]
        self.episode_reward += reward
        truncated = self.current_step >= self.max_steps
        info = {"action": u}
        if truncated:
            info["episode"] = {"r": self.episode_reward, "l": self.current_step}
        return self._obs(), reward, False, truncated, info


__all__ = ["PendulumEnv"]
