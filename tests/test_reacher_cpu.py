"""The two-link reacher without a GPU: the host export of the device dynamics
(sac_debug_reacher_step_host: the inline function the kernels call, compiled
for the host) against sac.control_envs.ReacherEnv bit for bit, the reset draws
against a numpy restatement of the Philox block, the C ABI's validation and
struct layout, the host class under SyncVectorEnv, and what the task is worth:
the returns of two scripted policies (profiles/reacher_baselines.txt)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_device_envs_cpu import env_obs_numpy

INCLUDE = os.path.join(ROOT, "include")
INVALID = -1
REACHER = 16
u64, i32 = ctypes.c_uint64, ctypes.c_int32
f32p, f64p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_reacher_step_host.argtypes = [ctypes.POINTER(E.EnvConfig), f64p, i32, f32p, f32p, f64p, i32p]
    lb.sac_debug_reacher_step_host.restype = ctypes.c_int
    lb.sac_debug_reacher_reset_host.argtypes = [u64, u64, i32, f64p]
    lb.sac_debug_reacher_reset_host.restype = ctypes.c_int
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


def _cfg(E, max_steps=100, dt=0.05, max_torque=1.0):
    c = E.EnvConfig()
    c.kind, c.num_envs, c.obs_dim, c.max_steps = REACHER, 1, 10, max_steps
    c.action_low, c.action_high, c.dt = -max_torque, max_torque, dt
    return c


def _step_host(lib, cfg, state, step, action):
    st = (ctypes.c_double * 6)(*state)
    act = (ctypes.c_float * 2)(*[float(np.float32(a)) for a in action])
    obs = (ctypes.c_float * 10)()
    rew, trunc = ctypes.c_double(), ctypes.c_int32()
    assert lib.sac_debug_reacher_step_host(ctypes.byref(cfg), st, step, act, obs, ctypes.byref(rew),
                                           ctypes.byref(trunc)) == 0, _err(lib)
    return list(st), np.array(obs[:], np.float32), rew.value, bool(trunc.value)


def _f64bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. host export against the host class
def test_step_host_is_the_host_class_bit_for_bit(lib):
    """Full 100-step episodes from 20 seeded states, actions uniform in +-1.5 (a third beyond the torque bound)."""
    from sac import _engine as E
    from sac.control_envs import ReacherEnv

    cfg = _cfg(E)
    n_clipped = 0
    for seed in range(20):
        env = ReacherEnv()
        env.reset(seed=seed)
        rng = np.random.default_rng(1000 + seed)
        actions = rng.uniform(-1.5, 1.5, size=(100, 2)).astype(np.float32)
        n_clipped += int(np.sum(np.abs(actions) > 1.0))
        state = list(env.state)
        for step, a in enumerate(actions):
            assert state == list(env.state)  # both start every step from the same float64 state
            obs, rew, term, trunc, _ = env.step(a)
            state, got_obs, got_rew, got_trunc = _step_host(lib, cfg, state, step, a)
            assert obs.dtype == np.float32 and obs.shape == (10,)
            assert np.array_equal(obs.view(np.uint32), got_obs.view(np.uint32)), (seed, step, obs, got_obs)
            assert _f64bits(rew) == _f64bits(got_rew), (seed, step, rew, got_rew)
            assert np.array_equal(_f64bits(env.state), _f64bits(state)), (seed, step)
            assert term is False and trunc == got_trunc == (step == 99)
            assert abs(state[2]) <= 5.0 and abs(state[3]) <= 5.0 and rew <= 0.0
    assert n_clipped > 1000


@pytest.mark.parametrize("max_steps,dt,torque", [(5, 0.05, 1.0), (7, 0.1, 0.75)])
def test_step_host_takes_the_constructor_arguments(lib, max_steps, dt, torque):
    from sac import _engine as E
    from sac.control_envs import ReacherEnv

    env = ReacherEnv(max_steps=max_steps, dt=dt, max_torque=torque)
    env.reset(seed=3)
    cfg = _cfg(E, max_steps, dt, torque)
    rng = np.random.default_rng(max_steps)
    state = list(env.state)
    for step in range(max_steps):
        a = rng.uniform(-1.5, 1.5, size=2).astype(np.float32)
        obs, rew, _, trunc, info = env.step(a)
        state, got_obs, got_rew, got_trunc = _step_host(lib, cfg, state, step, a)
        assert np.array_equal(obs.view(np.uint32), got_obs.view(np.uint32)) and _f64bits(rew) == _f64bits(got_rew)
        assert np.array_equal(_f64bits(env.state), _f64bits(state)) and trunc == got_trunc == (step == max_steps - 1)
        assert all(abs(u) <= torque for u in info["action"])


def test_the_two_action_components_drive_their_own_joints(lib):
    from sac import _engine as E

    cfg = _cfg(E)
    s0 = [0.3, -0.7, 0.0, 0.0, 0.05, -0.02]
    sa, _, ra, _ = _step_host(lib, cfg, s0, 0, (0.5, -0.25))
    sb, _, rb, _ = _step_host(lib, cfg, s0, 0, (-0.25, 0.5))
    assert sa[2] == 10.0 * 0.5 * 0.05 and sa[3] == 10.0 * -0.25 * 0.05  # w' = w + (GAIN u - DAMP w) dt from rest
    assert sb[2] == sa[3] and sb[3] == sa[2] and sa[0] != sb[0] and ra == rb  # the cost is symmetric, the motion not


def test_step_host_rejects_bad_arguments(lib):
    from sac import _engine as E

    cfg = _cfg(E)
    st, act, obs = (ctypes.c_double * 6)(), (ctypes.c_float * 2)(), (ctypes.c_float * 10)()
    rew, trunc = ctypes.c_double(), ctypes.c_int32()
    call = lib.sac_debug_reacher_step_host
    assert call(None, st, 0, act, obs, ctypes.byref(rew), ctypes.byref(trunc)) == INVALID
    assert call(ctypes.byref(cfg), None, 0, act, obs, ctypes.byref(rew), ctypes.byref(trunc)) == INVALID
    assert call(ctypes.byref(cfg), st, 0, None, obs, ctypes.byref(rew), ctypes.byref(trunc)) == INVALID
    cfg.kind = 8
    assert call(ctypes.byref(cfg), st, 0, act, obs, ctypes.byref(rew), ctypes.byref(trunc)) == INVALID
    assert "SAC_ENV_REACHER" in _err(lib)
    assert lib.sac_debug_reacher_reset_host(0, 0, 0, None) == INVALID
    assert lib.sac_debug_reacher_reset_host(0, 0, -1, st) == INVALID


# ---------------------------------------------------------------- 2. reset draws
def _reset_host(lib, seed, t, row):
    st = (ctypes.c_double * 6)()
    assert lib.sac_debug_reacher_reset_host(seed, t, row, st) == 0
    return tuple(st)


@pytest.mark.parametrize("seed,t", [(0, 0), (11, 61), (2**40 + 5, 2**33 + 1)])
def test_reset_draws_are_the_reset_blocks_four_uniforms(lib, seed, t):
    n = 33
    obs = env_obs_numpy(seed, t, 4, n, 4)  # which = 4, block 0: obs = 2u - 1 exactly, so u = (obs + 1) / 2 exactly
    u = (obs.astype(np.float64) + 1.0) / 2.0
    assert np.all((u * 2.0 ** 24) % 1.0 == 0.0) and np.all(u >= 0.0) and np.all(u < 1.0)
    for row in range(n):
        th1, th2, w1, w2, tx, ty = _reset_host(lib, seed, t, row)
        assert _f64bits(tx) == _f64bits(0.14 * (2.0 * u[row, 0] - 1.0)), row
        assert _f64bits(ty) == _f64bits(0.14 * (2.0 * u[row, 1] - 1.0)), row
        assert _f64bits(th1) == _f64bits(math.pi * (2.0 * u[row, 2] - 1.0)), row
        assert _f64bits(th2) == _f64bits(math.pi * (2.0 * u[row, 3] - 1.0)), row
        assert w1 == 0.0 and w2 == 0.0


def test_reset_draws_lie_in_range(lib):
    draws = np.array([_reset_host(lib, 1, 2, row) for row in range(5000)])
    th, w, tg = draws[:, :2], draws[:, 2:4], draws[:, 4:]
    assert tg.min() >= -0.14 and tg.max() <= 0.14 and th.min() >= -math.pi and th.max() < math.pi
    assert np.all(w == 0.0)
    assert np.hypot(tg[:, 0], tg[:, 1]).max() < 0.2  # the target square lies inside the reach circle
    assert tg.min() < -0.135 and tg.max() > 0.135 and th.min() < -3.1 and th.max() > 3.1
    assert np.abs(tg.mean(axis=0)).max() < 0.005 and np.abs(th.mean(axis=0)).max() < 0.1
    assert len(np.unique(draws, axis=0)) == 5000 and len(np.unique(draws[:, [0, 1, 4, 5]].reshape(-1))) > 19900
    base = _reset_host(lib, 1, 2, 0)
    assert base != _reset_host(lib, 1, 3, 0) and base != _reset_host(lib, 2, 2, 0) and base != _reset_host(lib, 1, 2, 1)


# ---------------------------------------------------------------- 3. validation, layout, codes
def _envs(E, kind=REACHER, n=4, obs=10, max_steps=5, vel=True):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, max_steps
    d.obs = d.step = d.ep_length = d.pos = d.ep_return = 0x1000  # never dereferenced: rejected before a launch
    d.episodes, d.ring_steps = 0x1000, 8
    if vel:
        d.vel = 0x1000
    return d


def _replay(E, obs=10, act=2):
    return E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, obs, act, 0x1000, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(obs=3), "obs_dim"),
    (dict(obs=9), "obs_dim"),
    (dict(vel=False), "null environment state"),
    (dict(kind=9), "unknown environment kind"),
    (dict(kind=15), "unknown environment kind"),
    (dict(kind=17), "unknown environment kind"),
])
def test_entry_points_reject_bad_reacher_envs(lib, kw, msg):
    from sac import _engine as E

    d = _envs(E, **kw)
    rb = _replay(E)
    assert lib.sac_envs_step(ctypes.byref(d), 0x1000, 1, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_envs_reset(ctypes.byref(d), 0, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
    assert msg in _err(lib)


def test_rollout_needs_a_replay_of_two_action_columns(lib):
    from sac import _engine as E

    d = _envs(E)
    for rb in (_replay(E, act=1), _replay(E, act=3), _replay(E, obs=3)):
        assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
        assert "replay dims" in _err(lib) and "act_dim 2" in _err(lib)
    cursor = (ctypes.c_int64 * 8)()
    rb1 = _replay(E, act=1)
    assert lib.sac_rollout_step_dev(None, ctypes.byref(d), ctypes.byref(rb1), cursor, 0, 0, 1, None) == INVALID
    assert "replay dims" in _err(lib)
    grad = (ctypes.c_int32 * 2)(1, 1)
    assert lib.sac_engine_loop_graph(None, ctypes.byref(d), ctypes.byref(rb1), cursor, 2, grad, None, 0, 0,
                                     None) == INVALID
    assert "replay dims" in _err(lib)
    # the one-action kinds still refuse a replay of two columns
    p = _envs(E, kind=8, obs=3)
    assert lib.sac_rollout_step(None, ctypes.byref(p), ctypes.byref(_replay(E, obs=3, act=2)), 0, 0, 1, 0, 1,
                                None) == INVALID
    assert "replay dims" in _err(lib) and "act_dim 1" in _err(lib)


def test_valid_reacher_envs_pass_validation(lib):
    from sac import _engine as E

    d = _envs(E)  # everything about the environments is accepted: the next check (the engine) is what fails
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(_replay(E)), 0, 0, 1, 0, 1, None) == INVALID
    assert "null engine" in _err(lib)


def test_host_engine_of_another_width_is_refused(lib):
    from sac import _engine as E

    lib.sac_debug_engine_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.POINTER(ctypes.c_void_p)]

    def engine(act):
        c = E.EngineConfig()
        c.obs_dim, c.act_dim, c.batch = 10, act, 16
        c.q_layers = c.pi_layers = 3
        for k, v in enumerate((10 + act, 32, 32, 1)):
            c.q_dims[k] = v
        for k, v in enumerate((10, 32, 32, 2 * act)):
            c.pi_dims[k] = v
        c.q_hidden_act = c.pi_hidden_act = 1
        c.gamma, c.tau, c.log_std_min, c.log_std_max, c.action_scale = 0.99, 0.005, -20.0, 2.0, 1.0
        c.actor_lr = c.critic_lr = c.alpha_lr = 3e-4
        c.beta1, c.beta2, c.adam_eps, c.target_entropy = 0.9, 0.999, 1e-8, -float(act)
        h = ctypes.c_void_p()
        assert lib.sac_debug_engine_host(ctypes.byref(c), ctypes.byref(h)) == 0, _err(lib)
        return h

    d, rb = _envs(E), _replay(E)
    e1, e2 = engine(1), engine(2)
    try:
        assert lib.sac_rollout_step(e1, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
        assert "engine dims" in _err(lib) and "act_dim 2" in _err(lib)
        # a matching engine passes every argument check: a host-only engine has nothing to launch on
        assert lib.sac_rollout_step(e2, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
        assert "no device state" in _err(lib)
    finally:
        lib.sac_engine_destroy(e1)
        lib.sac_engine_destroy(e2)


def test_envs_struct_layout_is_unchanged(tmp_path):
    from sac import _engine as E

    assert E.EnvsDesc._fields_[-1][0] == "vel"  # no field added for the reacher
    assert [n for n, t in E.EnvConfig._fields_ if t is ctypes.c_double] == list(E.ENV_PARAMS) and len(E.ENV_PARAMS) == 11
    structs = {"sac_env_config": E.EnvConfig, "sac_envs": E.EnvsDesc}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "sac_engine.h"', "int main(void) {"]
    for st, cls in structs.items():
        src.append(f'printf("{st} size %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            src.append(f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    src.append('printf("kind reacher %d\\n", (int)SAC_ENV_REACHER);')
    for k in (0, 3, 8, 16):
        src.append(f'printf("act {k} %d\\n", (int)SAC_ENV_ACT_DIM({k}));')
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
    assert (ctypes.sizeof(E.EnvConfig), ctypes.sizeof(E.EnvsDesc)) == (112, 176)  # as before the reacher
    assert lay[("kind", "reacher")] == REACHER
    assert [lay[("act", str(k))] for k in (0, 3, 8, 16)] == [1, 1, 1, 2]


def test_kind_code_matches_header_and_python_tables():
    from sac import _engine as E
    from sac.control_envs import ReacherEnv
    from sac.device_envs import _PARAM_ATTRS, KINDS, kind_name

    text = open(os.path.join(INCLUDE, "sac_engine.h")).read()
    code = int(re.search(r"SAC_ENV_REACHER\s*=\s*(\d+)", text).group(1))
    assert code == REACHER == E.ENV_KINDS["reacher"] == KINDS["reacher"][0]
    assert KINDS["reacher"][1] is ReacherEnv and _PARAM_ATTRS["reacher"] == {"dt": "dt"}
    assert kind_name(ReacherEnv) == kind_name("ReacherEnv") == kind_name(16) == "reacher"
    for unassigned in (9, 15, 17):
        with pytest.raises(ValueError):
            kind_name(unassigned)


def test_width_macros_match_the_python_tables_and_the_host_spaces(tmp_path):
    """include/sac_engine.h's width table, compiled as C, against what DeviceVectorEnv allocates and the host
    classes' spaces, for every kind.  SAC_ENV_OBS_DIM is 0 where the obs_dim is the caller's."""
    from sac.device_envs import KINDS, dstate_rows

    src = ['#include <stdio.h>', '#include "sac_engine.h"', "int main(void) {"]
    for code, _ in KINDS.values():
        src.append(f'printf("%d %d %d %d\\n", (int)SAC_ENV_OBS_DIM({code}), (int)SAC_ENV_ACT_DIM({code}), '
                   f'(int)SAC_ENV_POS_ROWS({code}), (int)SAC_ENV_VEL_ROWS({code}));')
    src.append("return 0; }")
    c = tmp_path / "widths.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "widths"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(KINDS) == 7
    for (name, (code, cls)), line in zip(KINDS.items(), lines):
        obs, act, pos_rows, vel_rows = (int(v) for v in line.split())
        host = cls()
        assert pos_rows + 1 + vel_rows == dstate_rows(name), name
        assert act == int(np.prod(host.action_space.shape)), name
        assert obs == (0 if name == "random_obs_binary" else int(np.prod(host.observation_space.shape))), name


# ---------------------------------------------------------------- 4. the host class
def test_spaces_and_constructor():
    from sac.control_envs import ReacherEnv

    env = ReacherEnv()
    assert (env.max_steps, env.dt, env.max_torque) == (100, 0.05, 1.0)
    assert (env.L1, env.L2, env.GAIN, env.DAMP, env.CTRL_COST, env.TARGET_HALF_SIDE) == (0.1, 0.1, 10.0, 2.0, 0.1, 0.14)
    want = np.array([1, 1, 1, 1, 0.14, 0.14, 5, 5, 0.34, 0.34], np.float32)
    assert env.observation_space.shape == (10,) and env.observation_space.dtype == np.float32
    assert np.allclose(env.observation_space.high, want, rtol=1e-6) and np.allclose(env.observation_space.low, -want, rtol=1e-6)
    assert env.action_space.shape == (2,) and env.action_space.low.tolist() == [-1.0, -1.0]
    assert env.action_space.high.tolist() == [1.0, 1.0]
    assert ReacherEnv(max_torque=0.5).observation_space.high[6] == 2.5
    draws = []
    for seed in range(200):
        obs, info = env.reset(seed=seed)
        th1, th2, w1, w2, tx, ty = env.state
        assert -math.pi <= th1 < math.pi and -math.pi <= th2 < math.pi and (w1, w2) == (0.0, 0.0) and info == {}
        assert abs(tx) <= 0.14 and abs(ty) <= 0.14 and all(isinstance(x, float) for x in env.state)
        dx = (0.1 * math.cos(th1) + 0.1 * math.cos(th1 + th2)) - tx
        dy = (0.1 * math.sin(th1) + 0.1 * math.sin(th1 + th2)) - ty
        assert np.array_equal(obs, np.array([math.cos(th1), math.cos(th2), math.sin(th1), math.sin(th2), tx, ty, 0.0,
                                             0.0, dx, dy], np.float32))
        assert np.all(np.abs(obs) <= env.observation_space.high)
        draws.append(tuple(env.state))
    assert len(set(draws)) == 200
    assert np.array_equal(env.reset(seed=5)[0], env.reset(seed=5)[0])


def test_speed_stays_inside_gain_over_damp():
    from sac.control_envs import ReacherEnv

    env = ReacherEnv(max_steps=400)
    env.reset(seed=0)
    for _ in range(400):  # full torque for ever: w -> GAIN / DAMP from below
        obs, *_ = env.step(np.array([3.0, -3.0], np.float32))
        assert np.all(np.abs(obs) <= env.observation_space.high)
    assert 4.99 < env.state[2] <= 5.0 and -5.0 <= env.state[3] < -4.99


def test_sync_vector_env_truncates_and_resets_in_the_same_step():
    from sac.control_envs import ReacherEnv
    from sac.vector_env import SyncVectorEnv

    N, M = 3, 5
    vec = SyncVectorEnv([lambda: ReacherEnv(max_steps=M)] * N)
    obs, _ = vec.reset(seed=7)
    assert obs.shape == (N, 10) and obs.dtype == np.float32 and vec.obs_dim == 10 and vec.act_dim == 2
    rng = np.random.default_rng(0)
    for t in range(1, 2 * M + 1):
        before = [list(e.state) for e in vec.envs]
        nxt, rew, term, trunc, info = vec.step(rng.uniform(-1.5, 1.5, size=(N, 2)).astype(np.float32))
        assert not term.any() and rew.dtype == np.float64 and np.all(rew <= 0.0)
        assert trunc.all() if t % M == 0 else not trunc.any()
        fin = info["final_obs"]
        assert np.allclose(fin[:, 0] ** 2 + fin[:, 2] ** 2, 1.0, atol=1e-6)
        if t % M == 0:
            # final_obs is the state stepped to; the returned observation is a fresh reset draw, at rest
            assert not np.array_equal(fin, nxt) and np.all(nxt[:, 6:8] == 0.0) and np.all(fin[:, 6:8] != 0.0)
            for i, e in enumerate(vec.envs):
                assert e.current_step == 0 and before[i] != e.state and np.array_equal(nxt[i], e._obs())
        else:
            assert np.array_equal(fin, nxt)


def test_train_replicas_accepts_reacher():
    from sac.control_envs import ReacherEnv
    from sac.train_replicas import PROBE_ENVS, env_factory, parse_args

    assert "reacher" in PROBE_ENVS and isinstance(env_factory("reacher")(), ReacherEnv)
    for extra in ([], ["--device-envs"], ["--device-envs", "--graph-steps", "4"]):
        a = parse_args(["--config", "unused.yaml", "--env", "reacher"] + extra)
        assert a.env == "reacher" and a.device_envs == bool(extra)


# ---------------------------------------------------------------- 5. the task is what it claims
def zero_torque(env):
    return np.zeros(2, np.float32)


def ik_solutions(tx, ty, l1=0.1, l2=0.1):
    """Both joint configurations whose fingertip is at (tx, ty) (the nearest point of the annulus if out of reach)."""
    c2 = min(1.0, max(-1.0, (tx * tx + ty * ty - l1 * l1 - l2 * l2) / (2.0 * l1 * l2)))
    out = []
    for q2 in (math.acos(c2), -math.acos(c2)):
        out.append((math.atan2(ty, tx) - math.atan2(l2 * math.sin(q2), l1 + l2 * math.cos(q2)), q2))
    return out


def _wrap(a):
    return ((a + math.pi) % (2 * math.pi)) - math.pi


def pd_controller(env):
    """Joint-space PD toward the inverse-kinematics solution nearer in joint space:
    u = clip(2 wrap(q* - th) - 0.4 w, +-1)."""
    th1, th2, w1, w2, tx, ty = env.state
    q = min(ik_solutions(tx, ty), key=lambda q: abs(_wrap(q[0] - th1)) + abs(_wrap(q[1] - th2)))
    u = [2.0 * _wrap(q[0] - th1) - 0.4 * w1, 2.0 * _wrap(q[1] - th2) - 0.4 * w2]
    return np.clip(np.array(u, np.float32), -1.0, 1.0)


def scripted_returns(policy, seeds):
    """(returns, final fingertip distances) of one default episode per seed under ``policy(env) -> action``."""
    from sac.control_envs import ReacherEnv

    rets, dists = [], []
    for seed in seeds:
        env = ReacherEnv()
        env.reset(seed=seed)
        ret, trunc = 0.0, False
        while not trunc:
            _, r, _, trunc, _ = env.step(policy(env))
            ret += r
        rets.append(ret)
        dists.append(math.hypot(*env._tip_to_target()))
    return np.array(rets), np.array(dists)


# profiles/reacher_baselines.txt, the committed class over seeds 0..99
BASELINE_SEEDS = range(100)


def test_standing_still_is_poor_and_a_pd_controller_reaches():
    zero, _ = scripted_returns(zero_torque, BASELINE_SEEDS)
    pd, dist = scripted_returns(pd_controller, BASELINE_SEEDS)
    print(f"zero torque: mean {zero.mean():.3f} min {zero.min():.3f} max {zero.max():.3f}; "
          f"PD: mean {pd.mean():.3f} worst {pd.min():.3f} final distance max {dist.max():.2e}")
    assert zero.mean() <= -12.0
    assert pd.mean() >= -6.0
    assert dist.max() < 1e-3 and pd.min() > zero.mean()  # every episode ends on the target, the worst beats standing still
