"""The pendulum swing-up without a GPU: the host export of the device dynamics
(sac_debug_env_step_host: the inline function the kernels call, compiled for
the host) against sac.control_envs.PendulumEnv bit for bit, the angle
normalisation, the reset draws, the C ABI's validation and struct layout, and
the host class under SyncVectorEnv."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

INCLUDE = os.path.join(ROOT, "include")
INVALID = -1
PENDULUM = 8
u64, i32, vp = ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
f32p, f64p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_env_step_host.argtypes = [ctypes.POINTER(E.EnvConfig), f64p, i32, ctypes.c_float, f32p, f64p, i32p]
    lb.sac_debug_env_step_host.restype = ctypes.c_int
    lb.sac_debug_env_reset_host.argtypes = [u64, u64, i32, f64p]
    lb.sac_debug_env_reset_host.restype = ctypes.c_int
    lb.sac_debug_env_obs_host.argtypes = [u64, u64, i32, i32, i32, vp]
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


def _cfg(E, max_steps=200, dt=0.05, max_torque=2.0):
    c = E.EnvConfig()
    c.kind, c.num_envs, c.obs_dim, c.max_steps = PENDULUM, 1, 3, max_steps
    c.action_low, c.action_high, c.dt = -max_torque, max_torque, dt
    return c


def _step_host(lib, cfg, state, step, action):
    st = (ctypes.c_double * 2)(*state)
    obs = (ctypes.c_float * 3)()
    rew, trunc = ctypes.c_double(), ctypes.c_int32()
    assert lib.sac_debug_env_step_host(ctypes.byref(cfg), st, step, float(np.float32(action)), obs,
                                       ctypes.byref(rew), ctypes.byref(trunc)) == 0, _err(lib)
    return [st[0], st[1]], np.array(obs[:], np.float32), rew.value, bool(trunc.value)


def _f64bits(x):
    return np.float64(x).view(np.uint64)


# ---------------------------------------------------------------- 1. host export against the host class
@pytest.mark.parametrize("steps,max_steps,dt,torque", [(300, 200, 0.05, 2.0), (40, 5, 0.05, 2.0), (40, 7, 0.1, 1.25)])
def test_step_host_is_the_host_class_bit_for_bit(lib, steps, max_steps, dt, torque):
    from sac import _engine as E
    from sac.control_envs import PendulumEnv

    env = PendulumEnv(max_steps=max_steps, dt=dt, max_torque=torque)
    env.reset(seed=steps)
    cfg = _cfg(E, max_steps, dt, torque)
    rng = np.random.default_rng(steps + max_steps)
    actions = rng.uniform(-1.6 * torque, 1.6 * torque, size=steps).astype(np.float32)
    lo, hi = np.float32(-torque), np.float32(torque)
    edge = [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(9)), np.float32(0.0), np.float32(-0.0)]
    actions[::7] = [edge[k % len(edge)] for k in range(len(actions[::7]))]
    assert (np.abs(actions) > torque).any() and (np.abs(actions) < torque).any()
    state, step, n_trunc = list(env.state), 0, 0
    for a in actions:
        assert state == list(env.state)  # both start every step from the same float64 state
        obs, rew, term, trunc, _ = env.step(np.array([a], np.float32))
        state, got_obs, got_rew, got_trunc = _step_host(lib, cfg, state, step, a)
        assert obs.dtype == np.float32 and np.array_equal(obs.view(np.uint32), got_obs.view(np.uint32)), (step, obs, got_obs)
        assert _f64bits(rew) == _f64bits(got_rew), (step, rew, got_rew)
        assert _f64bits(env.state[0]) == _f64bits(state[0]) and _f64bits(env.state[1]) == _f64bits(state[1])
        assert term is False and trunc == got_trunc
        step += 1
        if trunc:
            n_trunc += 1
            env.reset()
            state, step = list(env.state), 0
    assert n_trunc == steps // max_steps >= 1
    assert -(math.pi ** 2 + 6.4 + 0.001 * torque ** 2) <= got_rew <= 0.0


def test_step_host_rejects_bad_arguments(lib):
    from sac import _engine as E

    cfg = _cfg(E)
    st, obs = (ctypes.c_double * 2)(), (ctypes.c_float * 3)()
    rew, trunc = ctypes.c_double(), ctypes.c_int32()
    assert lib.sac_debug_env_step_host(None, st, 0, 0.0, obs, ctypes.byref(rew), ctypes.byref(trunc)) == INVALID
    assert lib.sac_debug_env_step_host(ctypes.byref(cfg), None, 0, 0.0, obs, ctypes.byref(rew),
                                       ctypes.byref(trunc)) == INVALID
    cfg.kind = 3
    assert lib.sac_debug_env_step_host(ctypes.byref(cfg), st, 0, 0.0, obs, ctypes.byref(rew),
                                       ctypes.byref(trunc)) == INVALID
    assert "SAC_ENV_PENDULUM" in _err(lib)
    assert lib.sac_debug_env_reset_host(0, 0, 0, None) == INVALID
    assert lib.sac_debug_env_reset_host(0, 0, -1, st) == INVALID


# ---------------------------------------------------------------- 2. angle normalisation
@pytest.mark.parametrize("th", [0.0, math.pi, -math.pi, 1.5 * math.pi, -1.5 * math.pi, 7.5, -7.5, 100.0])
def test_angle_normalisation_is_pythons_modulo(lib, th):
    from sac import _engine as E
    from sac.control_envs import PendulumEnv

    an = ((th + math.pi) % (2 * math.pi)) - math.pi
    assert -math.pi <= an < math.pi and PendulumEnv.angle_normalize(th) == an
    # thdot = 0 and a = 0 leave reward = -(an * an): the export's angle, squared
    _, _, rew, _ = _step_host(lib, _cfg(E), [th, 0.0], 0, 0.0)
    assert _f64bits(rew) == _f64bits(-(an * an + 0.1 * 0.0 * 0.0 + 0.001 * 0.0 * 0.0)), (th, an, rew)


# ---------------------------------------------------------------- 3. reset draws
def _reset_host(lib, seed, t, row):
    st = (ctypes.c_double * 2)()
    assert lib.sac_debug_env_reset_host(seed, t, row, st) == 0
    return st[0], st[1]


@pytest.mark.parametrize("seed,t", [(0, 0), (11, 61), (2**40 + 5, 2**33 + 1)])
def test_reset_draws_are_the_reset_blocks_first_two_uniforms(lib, seed, t):
    n = 33
    obs = np.zeros((n, 2), np.float32)  # which = 4, block 0: obs = 2u - 1 exactly, so u = (obs + 1) / 2 exactly
    assert lib.sac_debug_env_obs_host(seed, t, 4, n, 2, obs.ctypes.data) == 0
    u = (obs.astype(np.float64) + 1.0) / 2.0
    assert np.all((u * 2.0 ** 24) % 1.0 == 0.0) and np.all(u >= 0.0) and np.all(u < 1.0)
    for row in range(n):
        th, thdot = _reset_host(lib, seed, t, row)
        assert _f64bits(th) == _f64bits(math.pi * (2.0 * u[row, 0] - 1.0)), row
        assert _f64bits(thdot) == _f64bits(2.0 * u[row, 1] - 1.0), row


def test_reset_draws_lie_in_range(lib):
    draws = np.array([_reset_host(lib, 1, 2, row) for row in range(4096)])
    th, thdot = draws[:, 0], draws[:, 1]
    assert th.min() >= -math.pi and th.max() < math.pi and thdot.min() >= -1.0 and thdot.max() < 1.0
    assert abs(th.mean()) < 0.15 and abs(thdot.mean()) < 0.05 and len(np.unique(th)) > 4000
    assert th.min() < -3.0 and th.max() > 3.0 and thdot.min() < -0.95 and thdot.max() > 0.95
    assert _reset_host(lib, 1, 3, 0) != _reset_host(lib, 1, 2, 0) != _reset_host(lib, 2, 2, 0)


# ---------------------------------------------------------------- 4. validation, layout, codes
def _envs(E, kind=PENDULUM, n=4, obs=3, max_steps=5, vel=True):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, max_steps
    d.obs = d.step = d.ep_length = d.pos = d.ep_return = 0x1000  # never dereferenced: rejected before a launch
    d.episodes, d.ring_steps = 0x1000, 8
    if vel:
        d.vel = 0x1000
    return d


@pytest.mark.parametrize("kw,msg", [
    (dict(obs=1), "obs_dim"),
    (dict(obs=4), "obs_dim"),
    (dict(vel=False), "null environment state"),
    (dict(kind=4), "unknown environment kind"),
    (dict(kind=7), "unknown environment kind"),
    (dict(kind=9), "unknown environment kind"),
    (dict(max_steps=0), "max_steps"),
])
def test_entry_points_reject_bad_pendulum_envs(lib, kw, msg):
    from sac import _engine as E

    d = _envs(E, **kw)
    rb = E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, 3, 1, 0x1000, 0)
    assert lib.sac_envs_step(ctypes.byref(d), 0x1000, 1, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_envs_reset(ctypes.byref(d), 0, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
    assert msg in _err(lib)


def test_valid_pendulum_envs_pass_validation_and_probes_need_no_vel(lib):
    from sac import _engine as E

    rb = E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, 3, 1, 0x1000, 0)
    d = _envs(E)  # everything about the environments is accepted: the next check (the engine) is what fails
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
    assert "null engine" in _err(lib)
    rb1 = E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, 1, 1, 0x1000, 0)
    p = _envs(E, kind=3, obs=1, vel=False)
    assert lib.sac_rollout_step(None, ctypes.byref(p), ctypes.byref(rb1), 0, 0, 1, 0, 1, None) == INVALID
    assert "null engine" in _err(lib)


def test_envs_struct_layout_matches_c(tmp_path):
    from sac import _engine as E

    assert E.EnvsDesc._fields_[-1][0] == "vel"  # appended: every earlier field keeps its offset
    structs = {"sac_env_config": E.EnvConfig, "sac_envs": E.EnvsDesc}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "sac_engine.h"', "int main(void) {"]
    for st, cls in structs.items():
        src.append(f'printf("{st} size %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            src.append(f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    src.append('printf("kind pendulum %d\\n", (int)SAC_ENV_PENDULUM);')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    lay = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, v = line.split()
        lay[(st, f)] = int(v)
    for st, cls in structs.items():
        assert ctypes.sizeof(cls) == lay[(st, "size")], st
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == lay[(st, name)], (st, name)
    assert lay[("kind", "pendulum")] == PENDULUM


def test_kind_code_matches_header_and_python_tables():
    from sac import _engine as E
    from sac.control_envs import PendulumEnv
    from sac.device_envs import KINDS, kind_name

    text = open(os.path.join(INCLUDE, "sac_engine.h")).read()
    code = int(re.search(r"SAC_ENV_PENDULUM\s*=\s*(\d+)", text).group(1))
    assert code == PENDULUM == E.ENV_KINDS["pendulum"] == KINDS["pendulum"][0]
    assert KINDS["pendulum"][1] is PendulumEnv
    assert kind_name(PendulumEnv) == kind_name("PendulumEnv") == kind_name(8) == "pendulum"
    # the probes keep their codes, 4 stays unassigned
    assert [E.ENV_KINDS[k] for k in ("constant_reward", "quadratic_action", "random_obs_binary", "point_mass")] == \
        [0, 1, 2, 3]
    with pytest.raises(ValueError):
        kind_name(4)


# ---------------------------------------------------------------- 5. the host class
def test_spaces_and_constructor():
    from sac.control_envs import PendulumEnv

    env = PendulumEnv()
    assert (env.max_steps, env.dt, env.max_torque) == (200, 0.05, 2.0)
    assert env.observation_space.shape == (3,) and env.observation_space.dtype == np.float32
    assert env.observation_space.low.tolist() == [-1.0, -1.0, -8.0]
    assert env.observation_space.high.tolist() == [1.0, 1.0, 8.0]
    assert env.action_space.shape == (1,) and env.action_space.low.tolist() == [-2.0]
    assert env.action_space.high.tolist() == [2.0]
    env = PendulumEnv(max_steps=9, dt=0.1, max_torque=1.5)
    assert (env.max_steps, env.dt) == (9, 0.1) and env.action_space.high.tolist() == [1.5]
    draws = []
    for seed in range(200):
        obs, info = env.reset(seed=seed)
        th, thdot = env.state
        assert -math.pi <= th < math.pi and -1.0 <= thdot < 1.0 and info == {}
        assert np.array_equal(obs, np.array([math.cos(th), math.sin(th), thdot], np.float32))
        draws.append((th, thdot))
    assert len(set(draws)) == 200
    obs_a, _ = env.reset(seed=5)
    obs_b, _ = env.reset(seed=5)
    assert np.array_equal(obs_a, obs_b)


def test_speed_limit_and_settable_state():
    from sac.control_envs import PendulumEnv

    env = PendulumEnv()
    env.reset(seed=0)
    env.state = [math.pi / 2, 7.9]  # sin = 1: thdot + (15 + 6) * 0.05 passes the limit
    obs, rew, term, trunc, _ = env.step(np.array([5.0], np.float32))
    assert env.state[1] == 8.0 and obs[2] == 8.0 and env.state[0] == math.pi / 2 + 8.0 * 0.05
    an = math.pi / 2
    assert rew == -(an * an + 0.1 * 7.9 * 7.9 + 0.001 * 2.0 * 2.0) and not term and not trunc
    env.state = [-math.pi / 2, -7.9]
    env.step(np.array([-5.0], np.float32))
    assert env.state[1] == -8.0


def test_sync_vector_env_truncates_and_resets_in_the_same_step():
    from sac.control_envs import PendulumEnv
    from sac.vector_env import SyncVectorEnv

    N, M = 3, 5
    vec = SyncVectorEnv([lambda: PendulumEnv(max_steps=M)] * N)
    obs, _ = vec.reset(seed=7)
    assert obs.shape == (N, 3) and obs.dtype == np.float32 and vec.obs_dim == 3 and vec.act_dim == 1
    rng = np.random.default_rng(0)
    for t in range(1, 2 * M + 1):
        before = [list(e.state) for e in vec.envs]
        nxt, rew, term, trunc, info = vec.step(rng.uniform(-3, 3, size=(N, 1)).astype(np.float32))
        assert not term.any() and rew.dtype == np.float64 and np.all(rew <= 0.0)
        assert trunc.all() if t % M == 0 else not trunc.any()
        fin = info["final_obs"]
        assert np.allclose(fin[:, 0] ** 2 + fin[:, 1] ** 2, 1.0, atol=1e-6)
        if t % M == 0:
            # final_obs is the state stepped to; the returned observation is a fresh reset draw
            assert not np.array_equal(fin, nxt)
            for i, e in enumerate(vec.envs):
                assert e.current_step == 0 and -1.0 <= e.state[1] < 1.0
                assert np.array_equal(nxt[i], np.array([math.cos(e.state[0]), math.sin(e.state[0]), e.state[1]],
                                                       np.float32))
                assert fin[i, 2] != nxt[i, 2] and before[i] != e.state
        else:
            assert np.array_equal(fin, nxt)


def test_train_replicas_accepts_pendulum():
    from sac.control_envs import PendulumEnv
    from sac.train_replicas import PROBE_ENVS, env_factory, parse_args

    assert "pendulum" in PROBE_ENVS and isinstance(env_factory("pendulum")(), PendulumEnv)
    for extra in ([], ["--device-envs"], ["--device-envs", "--graph-steps", "4"]):
        a = parse_args(["--config", "unused.yaml", "--env", "pendulum"] + extra)
        assert a.env == "pendulum" and a.device_envs == bool(extra)
    with pytest.raises(SystemExit, match="pendulum"):  # the refusal lists it among the names it would take
        parse_args(["--config", "unused.yaml", "--env", "Pendulum-v1", "--device-envs"])
    # the probes still come from sac.envs
    from sac import envs

    assert isinstance(env_factory("point_mass")(), envs.OneDPointMassReachEnv)
