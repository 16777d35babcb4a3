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

``ReacherEnv`` is a planar two-link arm reaching for a target, the one task
with TWO action components.  The joints are decoupled first-order rotors driven
by a torque each (no mass matrix): what the policy has to learn is the
kinematics that couple them.  With links ``L1 = L2 = 0.1``, ``GAIN = 10``,
``DAMP = 2``, ``CTRL_COST = 0.1`` and the target (tx, ty) fixed for the episode:

    u_j    = clip(a_j, -max_torque, max_torque)                        j = 0, 1
    dx     = (L1 cos th1 + L2 cos(th1 + th2)) - tx
    dy     = (L1 sin th1 + L2 sin(th1 + th2)) - ty
    reward = -sqrt(dx^2 + dy^2) - CTRL_COST (u0^2 + u1^2)              (the pre-step state)
    w_j'   = w_j + (GAIN u_j - DAMP w_j) dt
    th_j'  = th_j + w_j' dt
    obs    = float32 [cos th1', cos th2', sin th1', sin th2', tx, ty, w1', w2', dx', dy']

It never terminates and is truncated after ``max_steps`` steps; ``reset`` draws
``tx, ty ~ U(-0.14, 0.14)`` (a square inside the reach circle of radius 0.2),
``th1, th2 ~ U(-pi, pi)`` and starts at rest.  |w| stays below GAIN / DAMP *
max_torque = 5, so no speed clip is needed.  Standing still costs about -16 per
100-step episode, a joint-space PD controller toward the inverse-kinematics
solution about -3.6 (profiles/reacher_baselines.txt).  Train it with
``policy_net.action_scale: 1.0``.

Its device form (``DeviceVectorEnv("reacher", N)``, ``SAC_ENV_REACHER``) never
feeds a sine or cosine back into the state, so the state trajectory is this
class's bit for bit; observations and rewards differ by the device library's
``sin`` / ``cos`` only.

``CartPoleEnv`` is the classic balancing cart-pole, the one task that ENDS BY
FAILURE: a pole hinged on a cart that a horizontal force pushes along a track.
The reward is +1 for every step survived, so the ``done`` column of a
transition is the only learning signal: a target that ignored it would make
every state worth 1 / (1 - gamma).  With ``G = 9.8``, ``M_CART = 1``, ``M_POLE =
0.1``, ``HALF_LEN = 0.5``, ``FORCE_MAG = 10`` and ``M = M_CART + M_POLE``:

    u      = clip(a, -max_action, max_action)
    F      = FORCE_MAG u;  c = cos th;  s = sin th
    temp   = (F + M_POLE HALF_LEN thdot^2 s) / M
    thacc  = (G s - c temp) / (HALF_LEN (4/3 - M_POLE c^2 / M))
    xacc   = temp - M_POLE HALF_LEN thacc c / M
    x' = x + dt xdot;  xdot' = xdot + dt xacc;  th' = th + dt thdot;  thdot' = thdot + dt thacc
    reward = 1                                            (every step, the failing one included)
    terminated = |x'| > X_LIMIT (2.4) or |th'| > TH_LIMIT (12 degrees)
    truncated  = current_step >= max_steps                (independent of terminated)
    obs    = float32 [x', xdot', th', thdot']

``reset`` draws all four components from U(-0.05, 0.05).  Episodes end at
different steps in different rows of a vector env.  Left alone the pole falls in
about 40 steps; a linear feedback on the state balances for the whole 500
(profiles/cartpole_baselines.txt).  Train it with ``policy_net.action_scale:
1.0``.

Its device form (``DeviceVectorEnv(CartPoleEnv, N)``, ``SAC_ENV_CARTPOLE``) takes
``sin th`` and ``cos th`` back into the state, so its trajectory follows this
class's to a few float64 ulps of the device library's functions, not to the bit.
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


class ReacherEnv(_Env):
    """Planar two-link reacher; ``state`` = [th1, th2, w1, w2, tx, ty] as Python floats (settable)."""

    L1 = 0.1
    L2 = 0.1
    GAIN = 10.0
    DAMP = 2.0
    CTRL_COST = 0.1
    TARGET_HALF_SIDE = 0.14

    def __init__(self, max_steps: int = 100, dt: float = 0.05, max_torque: float = 1.0):
        super().__init__()
        self.max_steps = int(max_steps)
        self.dt = float(dt)
        self.max_torque = float(max_torque)
        self.action_space = Box(low=-self.max_torque, high=self.max_torque, shape=(2,), dtype=np.float32)
        w_max = self.GAIN / self.DAMP * self.max_torque
        reach = self.L1 + self.L2 + self.TARGET_HALF_SIDE
        high = np.array([1.0, 1.0, 1.0, 1.0, self.TARGET_HALF_SIDE, self.TARGET_HALF_SIDE, w_max, w_max, reach, reach],
                        dtype=np.float32)
        self.observation_space = Box(low=-high, high=high, shape=(10,), dtype=np.float32)
        self.current_step = 0
        self.state = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        self.episode_reward = 0.0

    def _tip_to_target(self):
        th1, th2, _, _, tx, ty = self.state
        dx = (self.L1 * math.cos(th1) + self.L2 * math.cos(th1 + th2)) - tx
        dy = (self.L1 * math.sin(th1) + self.L2 * math.sin(th1 + th2)) - ty
        return dx, dy

    def _obs(self) -> np.ndarray:
        th1, th2, w1, w2, tx, ty = self.state
        dx, dy = self._tip_to_target()
        return np.array([math.cos(th1), math.cos(th2), math.sin(th1), math.sin(th2), tx, ty, w1, w2, dx, dy],
                        dtype=np.float32)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        super().reset(seed=seed)
        self.current_step, self.episode_reward = 0, 0.0
        h = self.TARGET_HALF_SIDE
        tx = float(self.np_random.uniform(low=-h, high=h))
        ty = float(self.np_random.uniform(low=-h, high=h))
        th1 = float(self.np_random.uniform(low=-math.pi, high=math.pi))
        th2 = float(self.np_random.uniform(low=-math.pi, high=math.pi))
        self.state = [th1, th2, 0.0, 0.0, tx, ty]
        return self._obs(), {}

    def step(self, action):
        self.current_step += 1
        th1, th2, w1, w2, tx, ty = (float(x) for x in self.state)
        self.state = [th1, th2, w1, w2, tx, ty]
        dt = self.dt
        lo, hi = self.action_space.low, self.action_space.high
        u0 = float(np.clip(np.float32(action[0]), lo[0], hi[0]))
        u1 = float(np.clip(np.float32(action[1]), lo[1], hi[1]))
        dx, dy = self._tip_to_target()
        reward = -math.sqrt(dx * dx + dy * dy) - self.CTRL_COST * (u0 * u0 + u1 * u1)
        w1 = w1 + (self.GAIN * u0 - self.DAMP * w1) * dt
        w2 = w2 + (self.GAIN * u1 - self.DAMP * w2) * dt
        th1 = th1 + w1 * dt
        th2 = th2 + w2 * dt
        self.state = [th1, th2, w1, w2, tx, ty]
        self.episode_reward += reward
        truncated = self.current_step >= self.max_steps
        info = {"action": (u0, u1)}
        if truncated:
            info["episode"] = {"r": self.episode_reward, "l": self.current_step}
        return self._obs(), reward, False, truncated, info


class CartPoleEnv(_Env):
    """Balancing cart-pole; ``state`` = [x, xdot, th, thdot] as Python floats (settable)."""

    G = 9.8
    M_CART = 1.0
    M_POLE = 0.1
    HALF_LEN = 0.5
    FORCE_MAG = 10.0
    X_LIMIT = 2.4
    TH_LIMIT = 12 * 2 * math.pi / 360
    RESET_HALF_SIDE = 0.05

    def __init__(self, max_steps: int = 500, dt: float = 0.02, max_action: float = 1.0):
        super().__init__()
        self.max_steps = int(max_steps)
        self.dt = float(dt)
        self.max_action = float(max_action)
        self.action_space = Box(low=-self.max_action, high=self.max_action, shape=(1,), dtype=np.float32)
        high = np.array([self.X_LIMIT, np.inf, self.TH_LIMIT, np.inf], dtype=np.float32)
        self.observation_space = Box(low=-high, high=high, shape=(4,), dtype=np.float32)
        self.current_step = 0
        self.state = [0.0, 0.0, 0.0, 0.0]
        self.episode_reward = 0.0

    def _obs(self) -> np.ndarray:
        return np.array(self.state, dtype=np.float32)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        super().reset(seed=seed)
        self.current_step, self.episode_reward = 0, 0.0
        h = self.RESET_HALF_SIDE
        self.state = [float(self.np_random.uniform(low=-h, high=h)) for _ in range(4)]
        return self._obs(), {}

    def step(self, action):
        self.current_step += 1
        x, xdot, th, thdot = (float(v) for v in self.state)
        dt = self.dt
        u = float(np.clip(np.float32(action[0]), self.action_space.low[0], self.action_space.high[0]))
        F = self.FORCE_MAG * u  # noqa: N806
        c, s = math.cos(th), math.sin(th)
        M = self.M_CART + self.M_POLE  # noqa: N806
        temp = (F + self.M_POLE * self.HALF_LEN * thdot * thdot * s) / M
        thacc = (self.G * s - c * temp) / (self.HALF_LEN * (4.0 / 3.0 - self.M_POLE * c * c / M))
        xacc = temp - self.M_POLE * self.HALF_LEN * thacc * c / M
        x = x + dt * xdot
        xdot = xdot + dt * xacc
        th = th + dt * thdot
        thdot = thdot + dt * thacc
        self.state = [x, xdot, th, thdot]
        reward = 1.0
        self.episode_reward += reward
        terminated = abs(x) > self.X_LIMIT or abs(th) > self.TH_LIMIT
        truncated = self.current_step >= self.max_steps
        info = {"action": u}
        if terminated or truncated:
            info["episode"] = {"r": self.episode_reward, "l": self.current_step}
        return self._obs(), reward, terminated, truncated, info


__all__ = ["PendulumEnv", "ReacherEnv", "CartPoleEnv"]
