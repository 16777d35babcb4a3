"""The balancing cart-pole without a GPU: the host export of the device dynamics
(sac_debug_cartpole_step_host: the inline function the kernels call, compiled
for the host) against sac.control_envs.CartPoleEnv bit for bit, the margin by
which terminating states break their limit (the precondition of the GPU
comparison), the flags at chosen states, the reset draws against a numpy
restatement of the Philox block, the C ABI's validation and struct layout, the
host class under SyncVectorEnv, what the task is worth (two scripted policies,
profiles/cartpole_baselines.txt) and the per-row episode selection of
SAC.evaluate_device(episodes_per_env=k)."""
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
CARTPOLE = 32
X_LIMIT, TH_LIMIT = 2.4, 12 * 2 * math.pi / 360
u64, i32 = ctypes.c_uint64, ctypes.c_int32
f32p, f64p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_cartpole_step_host.argtypes = [ctypes.POINTER(E.EnvConfig), f64p, i32, f32p, f32p, f64p, i32p, i32p]
    lb.sac_debug_cartpole_step_host.restype = ctypes.c_int
    lb.sac_debug_cartpole_reset_host.argtypes = [u64, u64, i32, f64p]
    lb.sac_debug_cartpole_reset_host.restype = ctypes.c_int
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


def _cfg(E, max_steps=500, dt=0.02, max_action=1.0):
    c = E.EnvConfig()
    c.kind, c.num_envs, c.obs_dim, c.max_steps = CARTPOLE, 1, 4, max_steps
    c.action_low, c.action_high, c.dt = -max_action, max_action, dt
    return c


def _step_host(lib, cfg, state, step, action):
    st = (ctypes.c_double * 4)(*state)
    act = (ctypes.c_float * 1)(float(np.float32(action)))
    obs = (ctypes.c_float * 4)()
    rew, term, trunc = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.sac_debug_cartpole_step_host(ctypes.byref(cfg), st, step, act, obs, ctypes.byref(rew),
                                            ctypes.byref(term), ctypes.byref(trunc)) == 0, _err(lib)
    return list(st), np.array(obs[:], np.float32), rew.value, bool(term.value), bool(trunc.value)


def _f64bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def limit_margin(state):
    """By how much a state exceeds the limit it broke (the larger excess if it broke both; <= 0: inside both)."""
    return max(abs(state[0]) - X_LIMIT, abs(state[2]) - TH_LIMIT)


# ---------------------------------------------------------------- 1. host export against the host class
def test_step_host_is_the_host_class_bit_for_bit(lib):
    """20 seeded episodes of at most 60 steps under uniform random actions (a third of them beyond the force
    bound): state, fp32 observation, reward and both flags exact at every step; terminations and truncations
    both occur, and every terminating state is more than 1e-9 outside the limit it broke -- the precondition
    for comparing the device's flags (its state is within 1e-12 of the host's) with the host's exactly."""
    from sac import _engine as E
    from sac.control_envs import CartPoleEnv

    max_steps = 60
    cfg = _cfg(E, max_steps=max_steps)
    n_term = n_trunc = n_clipped = n_steps = 0
    margins = []
    for seed in range(20):
        env = CartPoleEnv(max_steps=max_steps)
        env.reset(seed=seed)
        # few random-action episodes last 60 steps: with these action seeds two of the twenty do
        rng = np.random.default_rng(3000 + seed)
        state = list(env.state)
        for step in range(max_steps):
            a = rng.uniform(-1.5, 1.5, size=1).astype(np.float32)
            n_clipped += int(abs(a[0]) > 1.0)
            assert state == list(env.state)  # both start every step from the same float64 state
            obs, rew, term, trunc, info = env.step(a)
            state, got_obs, got_rew, got_term, got_trunc = _step_host(lib, cfg, state, step, a[0])
            n_steps += 1
            assert obs.dtype == np.float32 and obs.shape == (4,)
            assert np.array_equal(obs.view(np.uint32), got_obs.view(np.uint32)), (seed, step, obs, got_obs)
            assert np.array_equal(_f64bits(env.state), _f64bits(state)), (seed, step)
            assert rew == got_rew == 1.0 and isinstance(rew, float)
            assert term is got_term and trunc is got_trunc and trunc == (step == max_steps - 1), (seed, step)
            assert abs(info["action"]) <= 1.0 and ("episode" in info) == (term or trunc)
            if term:
                margins.append(limit_margin(state))
            if term or trunc:
                assert info["episode"] == {"r": float(step + 1), "l": step + 1}
                n_term, n_trunc = n_term + term, n_trunc + trunc
                break
            assert limit_margin(state) <= 0.0
    print(f"{n_steps} steps, {n_term} terminated, {n_trunc} truncated, {n_clipped} clipped actions, "
          f"smallest margin of a terminating state {min(margins):.3e}")
    assert n_term >= 5 and n_trunc >= 2 and n_clipped > 100
    assert min(margins) > 1e-9


@pytest.mark.parametrize("max_steps,dt,force", [(5, 0.02, 1.0), (7, 0.05, 0.5)])
def test_step_host_takes_the_constructor_arguments(lib, max_steps, dt, force):
    from sac import _engine as E
    from sac.control_envs import CartPoleEnv

    env = CartPoleEnv(max_steps=max_steps, dt=dt, max_action=force)
    env.reset(seed=3)
    cfg = _cfg(E, max_steps, dt, force)
    rng = np.random.default_rng(max_steps)
    state = list(env.state)
    for step in range(max_steps):
        a = rng.uniform(-1.5, 1.5, size=1).astype(np.float32)
        obs, rew, term, trunc, info = env.step(a)
        state, got_obs, got_rew, got_term, got_trunc = _step_host(lib, cfg, state, step, a[0])
        assert np.array_equal(obs.view(np.uint32), got_obs.view(np.uint32)) and rew == got_rew == 1.0
        assert np.array_equal(_f64bits(env.state), _f64bits(state)) and not term and not got_term
        assert trunc == got_trunc == (step == max_steps - 1) and abs(info["action"]) <= force


def test_one_step_from_rest_is_the_equations(lib):
    from sac import _engine as E

    # th = thdot = 0: s = 0, c = 1, temp = F / M, thacc = -temp / (0.5 (4/3 - 0.1 / 1.1)), xacc = temp - 0.05 thacc / 1.1
    st, obs, rew, term, trunc = _step_host(lib, _cfg(E), [0.0, 0.0, 0.0, 0.0], 0, 0.5)
    M = 1.0 + 0.1
    temp = (10.0 * 0.5 + 0.1 * 0.5 * 0.0 * 0.0 * 0.0) / M
    thacc = (9.8 * 0.0 - 1.0 * temp) / (0.5 * (4.0 / 3.0 - 0.1 * 1.0 * 1.0 / M))
    xacc = temp - 0.1 * 0.5 * thacc * 1.0 / M
    assert st == [0.0, 0.02 * xacc, 0.0, 0.02 * thacc] and xacc > 0.0 > thacc  # a push to the right tips the pole left
    assert np.array_equal(obs, np.array(st, np.float32)) and (rew, term, trunc) == (1.0, False, False)


# ---------------------------------------------------------------- 2. flags at chosen states
@pytest.mark.parametrize("state,step,max_steps,want", [
    ([2.39, 1.0, 0.0, 0.0], 0, 500, (True, False)),     # x' = 2.41: over the track's end
    ([-2.39, -1.0, 0.0, 0.0], 0, 500, (True, False)),
    ([0.0, 0.0, 0.2, 1.0], 0, 500, (True, False)),      # th' = 0.22 > 0.2094: the pole is down
    ([0.0, 0.0, -0.2, -1.0], 0, 500, (True, False)),
    ([0.0, 0.0, 0.0, 0.0], 499, 500, (False, True)),    # centred on the last step: truncated only
    ([0.0, 0.0, 0.0, 0.0], 498, 500, (False, False)),
    ([2.39, 1.0, 0.0, 0.0], 499, 500, (True, True)),    # fails on the last step: both
    ([0.0, 0.0, 0.2, 1.0], 4, 5, (True, True)),
])
def test_flags_at_chosen_states(lib, state, step, max_steps, want):
    from sac import _engine as E
    from sac.control_envs import CartPoleEnv

    env = CartPoleEnv(max_steps=max_steps)
    env.reset(seed=0)
    env.state, env.current_step = list(state), step
    _, rew, term, trunc, info = env.step(np.zeros(1, np.float32))
    new, _, got_rew, got_term, got_trunc = _step_host(lib, _cfg(E, max_steps=max_steps), state, step, 0.0)
    assert (term, trunc) == (got_term, got_trunc) == want and rew == got_rew == 1.0  # the failing step is paid too
    assert new == env.state and ("episode" in info) == (term or trunc)
    if want[0]:
        assert limit_margin(new) > 1e-3


# ---------------------------------------------------------------- 3. reset draws
def _reset_host(lib, seed, t, row):
    st = (ctypes.c_double * 4)()
    assert lib.sac_debug_cartpole_reset_host(seed, t, row, st) == 0
    return tuple(st)


@pytest.mark.parametrize("seed,t", [(0, 0), (11, 61), (2**40 + 5, 2**33 + 1)])
def test_reset_draws_are_the_reset_blocks_four_uniforms(lib, seed, t):
    n = 33
    obs = env_obs_numpy(seed, t, 4, n, 4)  # which = 4, block 0: obs = 2u - 1 exactly, so u = (obs + 1) / 2 exactly
    u = (obs.astype(np.float64) + 1.0) / 2.0
    assert np.all((u * 2.0 ** 24) % 1.0 == 0.0) and np.all(u >= 0.0) and np.all(u < 1.0)
    for row in range(n):
        got = _reset_host(lib, seed, t, row)
        for k in range(4):  # x, xdot, th, thdot
            assert _f64bits(got[k]) == _f64bits(0.05 * (2.0 * u[row, k] - 1.0)), (row, k)


def test_reset_draws_lie_in_range(lib):
    draws = np.array([_reset_host(lib, 1, 2, row) for row in range(5000)])
    assert draws.min() >= -0.05 and draws.max() < 0.05
    assert np.all(draws.min(axis=0) < -0.049) and np.all(draws.max(axis=0) > 0.049)
    assert np.abs(draws.mean(axis=0)).max() < 0.002
    assert len(np.unique(draws, axis=0)) == 5000 and len(np.unique(draws.reshape(-1))) > 19900
    base = _reset_host(lib, 1, 2, 0)
    assert base != _reset_host(lib, 1, 3, 0) and base != _reset_host(lib, 2, 2, 0) and base != _reset_host(lib, 1, 2, 1)


def test_host_exports_reject_bad_arguments(lib):
    from sac import _engine as E

    cfg = _cfg(E)
    st, act, obs = (ctypes.c_double * 4)(), (ctypes.c_float * 1)(), (ctypes.c_float * 4)()
    rew, term, trunc = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
    r, te, tr = ctypes.byref(rew), ctypes.byref(term), ctypes.byref(trunc)
    call = lib.sac_debug_cartpole_step_host
    assert call(None, st, 0, act, obs, r, te, tr) == INVALID
    assert call(ctypes.byref(cfg), None, 0, act, obs, r, te, tr) == INVALID
    assert call(ctypes.byref(cfg), st, 0, None, obs, r, te, tr) == INVALID
    assert call(ctypes.byref(cfg), st, 0, act, obs, r, None, tr) == INVALID
    assert call(ctypes.byref(cfg), st, -1, act, obs, r, te, tr) == INVALID
    cfg.kind = 16
    assert call(ctypes.byref(cfg), st, 0, act, obs, r, te, tr) == INVALID
    assert "SAC_ENV_CARTPOLE" in _err(lib)
    assert lib.sac_debug_cartpole_reset_host(0, 0, 0, None) == INVALID
    assert lib.sac_debug_cartpole_reset_host(0, 0, -1, st) == INVALID


# ---------------------------------------------------------------- 4. validation, layout, codes
def _envs(E, kind=CARTPOLE, n=4, obs=4, max_steps=5, vel=True):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, max_steps
    d.obs = d.step = d.ep_length = d.pos = d.ep_return = 0x1000  # never dereferenced: rejected before a launch
    d.episodes, d.ring_steps = 0x1000, 8
    if vel:
        d.vel = 0x1000
    return d


def _replay(E, obs=4, act=1):
    return E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, obs, act, 0x1000, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(obs=3), "obs_dim must be 4 for SAC_ENV_CARTPOLE"),
    (dict(obs=5), "obs_dim must be 4 for SAC_ENV_CARTPOLE"),
    (dict(vel=False), "null environment state"),
    (dict(kind=17), "unknown environment kind"),
    (dict(kind=31), "unknown environment kind"),
    (dict(kind=33), "unknown environment kind"),
])
def test_entry_points_reject_bad_cartpole_envs(lib, kw, msg):
    from sac import _engine as E

    d = _envs(E, **kw)
    rb = _replay(E)
    assert lib.sac_envs_step(ctypes.byref(d), 0x1000, 1, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_envs_reset(ctypes.byref(d), 0, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
    assert msg in _err(lib)


def test_rollout_needs_a_replay_of_one_action_column(lib):
    from sac import _engine as E

    d = _envs(E)
    for rb in (_replay(E, act=2), _replay(E, obs=3)):
        assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(rb), 0, 0, 1, 0, 1, None) == INVALID
        assert "replay dims" in _err(lib) and "act_dim 1" in _err(lib)
    cursor = (ctypes.c_int64 * 8)()
    rb2 = _replay(E, act=2)
    assert lib.sac_rollout_step_dev(None, ctypes.byref(d), ctypes.byref(rb2), cursor, 0, 0, 1, None) == INVALID
    assert "replay dims" in _err(lib)
    grad = (ctypes.c_int32 * 2)(1, 1)
    assert lib.sac_engine_loop_graph(None, ctypes.byref(d), ctypes.byref(rb2), cursor, 2, grad, None, 0, 0,
                                     None) == INVALID
    assert "replay dims" in _err(lib)
    # everything about valid environments is accepted: the next check (the engine) is what fails
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(_replay(E)), 0, 0, 1, 0, 1, None) == INVALID
    assert "null engine" in _err(lib)


def test_host_engine_of_two_action_components_is_refused(lib):
    from sac import _engine as E

    lib.sac_debug_engine_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.POINTER(ctypes.c_void_p)]

    def engine(act):
        c = E.EngineConfig()
        c.obs_dim, c.act_dim, c.batch = 4, act, 16
        c.q_layers = c.pi_layers = 3
        for k, v in enumerate((4 + act, 32, 32, 1)):
            c.q_dims[k] = v
        for k, v in enumerate((4, 32, 32, 2 * act)):
            c.pi_dims[k] = v
        c.q_hidden_act = c.pi_hidden_act = 1
        c.gamma, c.tau, c.log_std_min, c.log_std_max, c.action_scale = 0.99, 0.005, -20.0, 2.0, 1.0
        c.actor_lr = c.critic_lr = c.alpha_lr = 3e-4
        c.beta1, c.beta2, c.adam_eps, c.target_entropy = 0.9, 0.999, 1e-8, -float(act)
        h = ctypes.c_void_p()
        assert lib.sac_debug_engine_host(ctypes.byref(c), ctypes.byref(h)) == 0, _err(lib)
        return h

    d = _envs(E)
    e1, e2 = engine(1), engine(2)
    try:
        assert lib.sac_rollout_step(e2, ctypes.byref(d), ctypes.byref(_replay(E)), 0, 0, 1, 0, 1, None) == INVALID
        assert "engine dims" in _err(lib) and "act_dim 1" in _err(lib)
        # a matching engine passes every argument check: a host-only engine has nothing to launch on
        assert lib.sac_rollout_step(e1, ctypes.byref(d), ctypes.byref(_replay(E)), 0, 0, 1, 0, 1, None) == INVALID
        assert "no device state" in _err(lib)
    finally:
        lib.sac_engine_destroy(e1)
        lib.sac_engine_destroy(e2)


def test_envs_struct_layout_is_unchanged(tmp_path):
    from sac import _engine as E

    assert E.EnvsDesc._fields_[-1][0] == "vel"  # no field added for the cart-pole
    assert [n for n, t in E.EnvConfig._fields_ if t is ctypes.c_double] == list(E.ENV_PARAMS) and len(E.ENV_PARAMS) == 11
    src = ['#include <stdio.h>', '#include "sac_engine.h"', "int main(void) {",
           'printf("%zu %zu %d %d\\n", sizeof(sac_env_config), sizeof(sac_envs), (int)SAC_ENV_CARTPOLE, '
           '(int)SAC_ENV_ACT_DIM(SAC_ENV_CARTPOLE));', "return 0; }"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [112, 176, CARTPOLE, 1]
    assert (ctypes.sizeof(E.EnvConfig), ctypes.sizeof(E.EnvsDesc)) == (112, 176)


def test_kind_code_matches_header_and_python_tables():
    from sac import _engine as E
    from sac.control_envs import CartPoleEnv
    from sac.device_envs import _DSTATE_ROWS, _PARAM_ATTRS, KINDS, kind_name

    text = open(os.path.join(INCLUDE, "sac_engine.h")).read()
    code = int(re.search(r"SAC_ENV_CARTPOLE\s*=\s*(\d+)", text).group(1))
    assert code == CARTPOLE == E.ENV_KINDS["cartpole"] == KINDS["cartpole"][0]
    assert KINDS["cartpole"][1] is CartPoleEnv and _PARAM_ATTRS["cartpole"] == {"dt": "dt"}
    assert _DSTATE_ROWS["cartpole"] == 5  # x, th, episode return, xdot, thdot
    assert kind_name(CartPoleEnv) == kind_name("CartPoleEnv") == kind_name(32) == "cartpole"
    with pytest.raises(ValueError):  # the bare key stays the unknown name tests/test_device_envs_cpu.py uses it as
        kind_name("cartpole")
    for unassigned in (17, 31, 33):
        with pytest.raises(ValueError):
            kind_name(unassigned)


# ---------------------------------------------------------------- 5. the host class
def test_spaces_and_constructor():
    from sac.control_envs import CartPoleEnv

    env = CartPoleEnv()
    assert (env.max_steps, env.dt, env.max_action) == (500, 0.02, 1.0)
    assert (env.G, env.M_CART, env.M_POLE, env.HALF_LEN, env.FORCE_MAG, env.X_LIMIT) == (9.8, 1.0, 0.1, 0.5, 10.0, 2.4)
    assert env.TH_LIMIT == TH_LIMIT and abs(TH_LIMIT - math.radians(12)) < 1e-15
    hi = env.observation_space.high
    assert env.observation_space.shape == (4,) and env.observation_space.dtype == np.float32
    assert hi[0] == np.float32(2.4) and hi[2] == np.float32(TH_LIMIT) and np.isinf(hi[1]) and np.isinf(hi[3])
    assert np.array_equal(env.observation_space.low, -hi)
    assert env.action_space.shape == (1,) and env.action_space.low.tolist() == [-1.0]
    assert CartPoleEnv(max_action=0.5).action_space.high.tolist() == [0.5]
    draws = []
    for seed in range(200):
        obs, info = env.reset(seed=seed)
        assert info == {} and all(isinstance(v, float) and -0.05 <= v <= 0.05 for v in env.state)
        assert np.array_equal(obs, np.array(env.state, np.float32)) and env.current_step == 0
        draws.append(tuple(env.state))
    assert len(set(draws)) == 200
    assert np.array_equal(env.reset(seed=5)[0], env.reset(seed=5)[0])


def test_sync_vector_env_resets_failed_rows_in_the_same_step():
    from sac.control_envs import CartPoleEnv
    from sac.vector_env import SyncVectorEnv

    N, M = 4, 12
    vec = SyncVectorEnv([lambda: CartPoleEnv(max_steps=M)] * N)
    obs, _ = vec.reset(seed=7)
    assert obs.shape == (N, 4) and obs.dtype == np.float32 and vec.obs_dim == 4 and vec.act_dim == 1
    vec.envs[1].state = [0.0, 0.0, 0.2, 1.0]    # falls on the first step
    vec.envs[2].state = [2.39, 0.4, 0.0, 0.0]   # leaves the track on the second
    ended_at = {i: [] for i in range(N)}
    for t in range(1, M + 1):
        nxt, rew, term, trunc, info = vec.step(np.zeros((N, 1), np.float32))
        assert rew.dtype == np.float64 and np.all(rew == 1.0)
        fin = info["final_obs"]
        for i, e in enumerate(vec.envs):
            if term[i] or trunc[i]:
                ended_at[i].append(t)
                # final_obs is the failed state; the returned observation is a fresh draw near the centre
                assert e.current_step == 0 and np.all(np.abs(nxt[i]) <= 0.05) and np.array_equal(nxt[i], e._obs())
                if term[i]:
                    assert abs(fin[i, 0]) > 2.4 or abs(fin[i, 2]) > TH_LIMIT
            else:
                assert np.array_equal(fin[i], nxt[i])
        if t == 1:
            assert term.tolist() == [False, True, False, False] and not trunc.any()
        if t == 2:
            assert term.tolist() == [False, False, True, False] and not trunc.any()
    assert ended_at[1][0] == 1 and ended_at[2][0] == 2 and ended_at[0] == ended_at[3] == [M]  # rows not in lockstep


def test_train_replicas_accepts_cartpole():
    from sac.control_envs import CartPoleEnv
    from sac.train_replicas import PROBE_ENVS, env_factory, parse_args

    assert "cartpole" in PROBE_ENVS and isinstance(env_factory("cartpole")(), CartPoleEnv)
    for extra in ([], ["--device-envs"], ["--device-envs", "--graph-steps", "4"]):
        a = parse_args(["--config", "unused.yaml", "--env", "cartpole"] + extra)
        assert a.env == "cartpole" and a.device_envs == bool(extra)


# ---------------------------------------------------------------- 6. the task is what it claims
def zero_force(env):
    return np.zeros(1, np.float32)


def linear_feedback(env):
    """u = clip(0.1 x + 0.3 xdot + 4 th + 0.6 thdot, +-1): push the cart under the falling pole."""
    x, xdot, th, thdot = env.state
    return np.clip(np.array([0.1 * x + 0.3 * xdot + 4.0 * th + 0.6 * thdot], np.float32), -1.0, 1.0)


def scripted_lengths(policy, seeds, max_steps=500):
    """(episode lengths = returns, terminated flags) of one episode per seed under ``policy(env) -> action``."""
    from sac.control_envs import CartPoleEnv

    lengths, terms = [], []
    for seed in seeds:
        env = CartPoleEnv(max_steps=max_steps)
        env.reset(seed=seed)
        ret, term, trunc = 0.0, False, False
        while not (term or trunc):
            _, r, term, trunc, _ = env.step(policy(env))
            ret += r
        assert ret == env.current_step
        lengths.append(env.current_step)
        terms.append(term)
    return np.array(lengths), np.array(terms)


# profiles/cartpole_baselines.txt: the committed class over seeds 0..99; the test takes the first 20
BASELINE_SEEDS = range(100)


def test_left_alone_the_pole_falls_and_a_linear_feedback_balances():
    seeds = list(BASELINE_SEEDS)[:20]
    zero, zero_term = scripted_lengths(zero_force, seeds)
    fb, fb_term = scripted_lengths(linear_feedback, seeds)
    print(f"zero force: mean {zero.mean():.1f} min {zero.min()} max {zero.max()}; feedback: mean {fb.mean():.1f} "
          f"min {fb.min()}")
    assert zero_term.all() and zero.max() < 200 and zero.min() >= 1
    assert np.all(fb == 500) and not fb_term.any()


# ---------------------------------------------------------------- 7. per-row episode selection
def test_first_episodes_per_row_on_unequal_lengths():
    from sac.device_envs import first_episodes_per_row

    # (vector step, row, return) in (step, row) order: row 1 fails early and often, row 0 survives, row 2 in between
    eps = [(3, 1, 3.0), (5, 1, 2.0), (7, 2, 7.0), (9, 1, 4.0), (10, 0, 10.0), (10, 1, 1.0), (15, 2, 8.0), (20, 0, 10.0),
           (21, 1, 11.0), (24, 2, 9.0)]
    assert first_episodes_per_row(eps, 3, 1) == [10.0, 3.0, 7.0]
    assert first_episodes_per_row(eps, 3, 2) == [10.0, 3.0, 7.0, 10.0, 2.0, 8.0]
    # the first 6 to finish hold four of row 1's failures and none of row 0's second episode: mean 4.5 against 6.67
    first_finished = [r for _, _, r in eps[:6]]
    assert np.mean(first_finished) == 4.5 and np.mean(first_episodes_per_row(eps, 3, 2)) == 40.0 / 6.0
    with pytest.raises(ValueError, match=r"rows \[0\]"):
        first_episodes_per_row(eps, 3, 3)  # row 0 ended two
    with pytest.raises(ValueError):
        first_episodes_per_row(eps, 4, 1)  # row 3 ended none
    with pytest.raises(ValueError):
        first_episodes_per_row(eps, 3, 0)


def test_first_episodes_per_row_on_equal_lengths_is_first_finished():
    from sac.device_envs import first_episodes_per_row

    N, L, k = 5, 4, 3
    rng = np.random.default_rng(0)
    eps = [(L * e, i, float(rng.normal())) for e in range(1, k + 2) for i in range(N)]  # k + 1 episodes per row
    assert first_episodes_per_row(eps, N, k) == [r for _, _, r in eps[:k * N]]
    assert first_episodes_per_row(iter(eps), N, 1) == [r for _, _, r in eps[:N]]
