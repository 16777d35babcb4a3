"""train.random_steps without a device: the host export of the uniform draws against a
restatement on oracle/sampler_oracle.py's Philox, their distribution, the engine's action-source switch, the
key, the helpers that say which vector steps are uniform, the command line, and the vectorised loop's actions."""
import copy
import ctypes
import itertools
import math

import numpy as np
import pytest

import _control
from _gpu import FakeEnv
from oracle import sampler_oracle as S

F32 = np.float32
INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    lb = E.load_library()
    lb.sac_debug_engine_host.restype = ctypes.c_int
    lb.sac_debug_engine_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.POINTER(ctypes.c_void_p)]
    return lb


def export(lib, seed, t, n, act_dim, scale):
    out = np.full((n, act_dim), np.nan, np.float32)
    rc = lib.sac_uniform_actions_host(seed, t, n, act_dim, scale, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == 0, lib.sac_last_error().decode()
    return out


# ---------------------------------------------------------------- 1. the definition
def restated(seed, t, n, act_dim, scale):
    """The issue's definition, word for word: key = seed, counter (t lo, t hi, i, 5 << 16 | j / 4), word j % 4,
    u = (float)(w >> 8) * 2^-24, a = scale * (2.0f * u - 1.0f) with every operation rounded to fp32."""
    out = np.empty((n, act_dim), np.float32)
    for i in range(n):
        for j in range(act_dim):
            c = S.philox4x32_10([t & S.M32, (t >> 32) & S.M32, i, (5 << 16) | (j // 4)], seed & S.M32,
                                (seed >> 32) & S.M32)
            u = F32(c[j % 4] >> 8) * F32(2.0 ** -24)
            out[i, j] = F32(scale) * (F32(2.0) * u - F32(1.0))
    return out


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("act_dim", [1, 2, 4, 5, 8, 32])
def test_export_matches_the_definition(lib, act_dim, scale):
    for seed, t, n in itertools.product((0, 2 ** 63 + 5), (1, 2 ** 32 + 3), (1, 40)):
        got, want = export(lib, seed, t, n, act_dim, scale), restated(seed, t, n, act_dim, scale)
        assert np.array_equal(bits(got), bits(want)), (seed, t, n)
        assert (got >= -scale).all() and (got < scale).all()
    # the draws depend on every argument of the counter and on the key
    base = export(lib, 7, 3, 40, act_dim, scale)
    assert not np.array_equal(base, export(lib, 8, 3, 40, act_dim, scale))
    assert not np.array_equal(base, export(lib, 7, 4, 40, act_dim, scale))
    assert not np.array_equal(base, export(lib, 7, 3 + 2 ** 32, 40, act_dim, scale))
    assert not np.array_equal(base, export(lib, 7 + 2 ** 32, 3, 40, act_dim, scale))
    assert len(np.unique(base)) >= base.size - 1  # rows and components draw their own words


def test_export_refuses_bad_arguments_before_writing(lib):
    out = np.full((4, 4), 77.0, np.float32)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    bad = {
        "null out": (0, 1, 4, 4, 1.0, None),
        "n = 0": (0, 1, 0, 4, 1.0, ptr),
        "n < 0": (0, 1, -3, 4, 1.0, ptr),
        "act_dim = 0": (0, 1, 4, 0, 1.0, ptr),
        "act_dim = 33": (0, 1, 4, 33, 1.0, ptr),
        "scale = 0": (0, 1, 4, 4, 0.0, ptr),
        "scale < 0": (0, 1, 4, 4, -1.0, ptr),
        "scale = inf": (0, 1, 4, 4, math.inf, ptr),
        "scale = nan": (0, 1, 4, 4, math.nan, ptr),
    }
    for what, args in bad.items():
        assert lib.sac_uniform_actions_host(*args) == INVALID, what
        assert lib.sac_last_error().decode().startswith("uniform_actions:"), what
        assert (out == 77.0).all(), what


def test_distribution_of_the_draws(lib):
    """M = 65536 draws of U[-1, 1): the mean of M draws has standard deviation sqrt(1/3) / sqrt(M), and the count
    of one of 8 equal bins is binomial(M, 1/8); both held to 5 sigma."""
    M = 65536
    a = export(lib, 12345, 9, M // 4, 4, 1.0).ravel().astype(np.float64)
    assert a.size == M
    mean = a.mean()
    counts = np.histogram(a, bins=8, range=(-1.0, 1.0))[0]
    sigma = math.sqrt(M * (1 / 8) * (7 / 8))
    print(f"mean {mean:+.5f} (bound {5 / math.sqrt(3 * M):.5f}); bins {counts.tolist()} (M/8 = {M // 8}, "
          f"5 sigma = {5 * sigma:.1f})")
    assert abs(mean) <= 5 / math.sqrt(3 * M)
    assert counts.sum() == M and (np.abs(counts - M / 8) <= 5 * sigma).all()


# ---------------------------------------------------------------- 2. the switch
def host_engine(lib, E, act=1, obs=1):
    c = E.EngineConfig()
    c.obs_dim, c.act_dim, c.batch = obs, act, 16
    c.q_layers = c.pi_layers = 3
    for k, v in enumerate((obs + act, 32, 32, 1)):
        c.q_dims[k] = v
    for k, v in enumerate((obs, 32, 32, 2 * act)):
        c.pi_dims[k] = v
    c.q_hidden_act = c.pi_hidden_act = 1
    c.gamma, c.tau, c.log_std_min, c.log_std_max, c.action_scale = 0.99, 0.005, -20.0, 2.0, 1.0
    c.actor_lr = c.critic_lr = c.alpha_lr = 3e-4
    c.beta1, c.beta2, c.adam_eps, c.target_entropy = 0.9, 0.999, 1e-8, -float(act)
    h = ctypes.c_void_p()
    assert lib.sac_debug_engine_host(ctypes.byref(c), ctypes.byref(h)) == 0, lib.sac_last_error().decode()
    return h


PTR = 0x10000


def rollout_errors(lib, E, h):
    """(return code, message) of rollout calls with bad arguments and of one whose arguments are all good, on a
    host-only engine: nothing is ever launched or read through the made-up addresses."""
    def envs(**fields):
        d = E.EnvsDesc()
        d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = 3, 4, 1, 5
        d.obs = d.step = d.ep_length = d.pos = d.ep_return = d.episodes = PTR
        d.ring_steps = 8
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def replay(**fields):
        r = E.ReplayDesc(PTR, PTR, PTR, PTR, PTR, 12, 1, 1, PTR, 0)
        for k, v in fields.items():
            setattr(r, k, v)
        return r

    cursor = ctypes.cast(PTR, ctypes.POINTER(ctypes.c_int64))
    calls = {
        "null replay": lambda: lib.sac_rollout_step(h, ctypes.byref(envs()), None, 0, 0, 1, 0, 1, None),
        "no episode ring": lambda: lib.sac_rollout_step(h, ctypes.byref(envs(episodes=None)), ctypes.byref(replay()),
                                                        0, 0, 1, 0, 1, None),
        "pos = capacity": lambda: lib.sac_rollout_step(h, ctypes.byref(envs()), ctypes.byref(replay()), 0, 12, 1, 0,
                                                       1, None),
        "replay dims": lambda: lib.sac_rollout_step(h, ctypes.byref(envs()), ctypes.byref(replay(act_dim=2)), 0, 0, 1,
                                                    0, 1, None),
        "capacity < num_envs": lambda: lib.sac_rollout_step(h, ctypes.byref(envs()), ctypes.byref(replay(capacity=3)),
                                                            0, 0, 1, 0, 1, None),
        "good, host-only engine": lambda: lib.sac_rollout_step(h, ctypes.byref(envs()), ctypes.byref(replay()), 0, 0,
                                                               1, 0, 1, None),
        "dev: null cursor": lambda: lib.sac_rollout_step_dev(h, ctypes.byref(envs()), ctypes.byref(replay()), None, 0,
                                                             0, 1, None),
        "dev: parity 2": lambda: lib.sac_rollout_step_dev(h, ctypes.byref(envs()), ctypes.byref(replay()), cursor, 2,
                                                          0, 1, None),
        "dev: good, host-only engine": lambda: lib.sac_rollout_step_dev(h, ctypes.byref(envs()),
                                                                        ctypes.byref(replay()), cursor, 0, 0, 1, None),
    }
    out = {}
    for what, call in calls.items():
        out[what] = (call(), lib.sac_last_error().decode())
    return out


def test_set_action_source_checks_the_source_and_changes_no_argument_error(lib):
    from sac import _engine as E

    assert (E.ACTIONS_POLICY, E.ACTIONS_UNIFORM) == (0, 1)
    for bad in (-1, 2, 100):
        assert lib.sac_engine_set_action_source(None, bad) == INVALID
        msg = lib.sac_last_error().decode()
        assert msg.startswith("set_action_source: source") and "0..1" in msg, msg
    for ok in (0, 1):  # a valid source gets as far as the null engine
        assert lib.sac_engine_set_action_source(None, ok) == INVALID
        assert "null engine" in lib.sac_last_error().decode()
    h = host_engine(lib, E)
    try:
        for bad in (-1, 2):
            assert lib.sac_engine_set_action_source(h, bad) == INVALID
        assert lib.sac_engine_set_action_source(h, E.ACTIONS_POLICY) == 0
        under_policy = rollout_errors(lib, E, h)
        assert lib.sac_engine_set_action_source(h, E.ACTIONS_UNIFORM) == 0
        under_uniform = rollout_errors(lib, E, h)
        assert lib.sac_engine_set_action_source(h, E.ACTIONS_POLICY) == 0
    finally:
        lib.sac_engine_destroy(h)
    assert under_policy == under_uniform
    assert all(rc == INVALID for rc, _ in under_policy.values()), under_policy
    assert "no device state" in under_policy["good, host-only engine"][1]
    assert "no device state" in under_policy["dev: good, host-only engine"][1]
    assert len({msg for _, msg in under_policy.values()}) >= 6  # the cases fail for their own reasons


# ---------------------------------------------------------------- 3. host logic
def cpu_cfg(**train):
    cfg = copy.deepcopy(_control.cfg("point_mass", hidden=(16, 16), warming=10 ** 9))
    cfg["train"].update(device="cpu", engine_device="cpu", **train)
    return cfg


def test_key_defaults_to_zero_and_takes_a_non_negative_int_only():
    from sac.agent import SAC

    assert SAC.random_steps == 0
    assert SAC(FakeEnv(1, 1), cpu_cfg()).random_steps == 0
    assert SAC(FakeEnv(1, 1), cpu_cfg(random_steps=0)).random_steps == 0
    assert SAC(FakeEnv(1, 1), cpu_cfg(random_steps=1000)).random_steps == 1000
    got = SAC(FakeEnv(1, 1), cpu_cfg(random_steps=np.int64(7), n_step=3, bootstrap_truncated=True)).random_steps
    assert got == 7 and type(got) is int
    for bad in (True, False, 1.0, 10.5, -1, "10", None, [3]):
        with pytest.raises(ValueError, match=r"train\.random_steps"):
            SAC(FakeEnv(1, 1), cpu_cfg(random_steps=bad))


def test_which_vector_steps_are_uniform():
    from sac.agent import graph_block_policy_only, uniform_vector_step

    def uniform(N, K, steps=12):
        return [v for v in range(steps) if uniform_vector_step(v, N, K)]

    assert uniform(4, 10) == [0, 1, 2]  # K no multiple of N: the step that holds env step K - 1 is uniform, whole
    assert uniform(4, 8) == [0, 1] and uniform(4, 9) == [0, 1, 2] and uniform(4, 1) == [0]
    assert uniform(4, 0) == [] and uniform(1, 0) == []
    assert uniform(4, 10 ** 6) == list(range(12))  # K beyond the run
    assert uniform(1, 5) == [0, 1, 2, 3, 4]
    for N, K in ((4, 10), (7, 7), (3, 0), (40, 100)):
        assert len(uniform(N, K, 1000)) == -(-K // N)
        # a block may replay the loop graph iff none of its steps is uniform, whatever its length
        for first in range(0, 12):
            for k in (2, 4, 8):
                want = not any(uniform_vector_step(v, N, K) for v in range(first, first + k))
                assert graph_block_policy_only(first, N, K) == want, (N, K, first, k)


def test_train_replicas_flag():
    from sac.train_replicas import parse_args

    assert parse_args(["--config", "c.yaml"]).random_steps is None
    assert parse_args(["--config", "c.yaml", "--random-steps", "0"]).random_steps == 0
    a = parse_args(["--config", "c.yaml", "--random-steps", "1000", "--device-envs", "--graph-steps", "4",
                    "--bootstrap-truncated"])
    assert a.random_steps == 1000 and a.graph_steps == 4 and a.bootstrap_truncated
    a = parse_args(["--config", "c.yaml", "--random-steps", "64", "--n-step", "3"])
    assert a.random_steps == 64 and a.n_step == 3 and not a.device_envs
    for bad in ("-1", "1.5", "many"):
        with pytest.raises(SystemExit):
            parse_args(["--config", "c.yaml", "--random-steps", bad])


class HostEngine:
    """What the vectorised loop asks of the engine for a uniform step, over the export (no device)."""

    def __init__(self, lib, seed, scale, act_dim):
        self.lib, self.seed, self.scale, self.act_dim = lib, seed, scale, act_dim

    def uniform_actions(self, n, t):
        return export(self.lib, self.seed, t, n, self.act_dim, self.scale)


@pytest.mark.parametrize("K", [0, 10, 8])
def test_vectorised_loop_takes_the_uniform_actions_first(lib, K):
    from sac.agent import SAC
    from sac.envs import OneDPointMassReachEnv
    from sac.vector_env import SyncVectorEnv

    N, steps = 4, 6
    taken = []

    class Env(SyncVectorEnv):
        def step(self, actions):
            taken.append(np.array(actions, np.float32))
            return super().step(actions)

    vec = Env([lambda: OneDPointMassReachEnv(max_steps=5)] * N)
    agent = SAC(vec, cpu_cfg(random_steps=K))
    eng = HostEngine(lib, seed=2 ** 40 + 17, scale=1.0, act_dim=1)
    agent._engine = lambda: eng
    policy = np.full((N, 1), 0.125, np.float32)  # no uniform draw of 24 bits is all this
    agent.select_actions = lambda obs, deterministic=False: policy.copy()
    stored = []
    agent.store_transitions = lambda s, a, r, s2, d: stored.append(np.array(a, np.float32))
    m = agent.run_vectorized_training_loop(steps * N, vec_env=vec)
    assert m["total_env_steps"] == steps * N and len(taken) == len(stored) == steps
    n_uniform = -(-K // N)
    for v in range(steps):
        want = eng.uniform_actions(N, v + 1) if v < n_uniform else policy
        assert np.array_equal(bits(taken[v]), bits(want)), v
        assert np.array_equal(bits(stored[v]), bits(want)), v
        assert np.array_equal(taken[v], eng.uniform_actions(N, v + 1)) == (v < n_uniform), v
