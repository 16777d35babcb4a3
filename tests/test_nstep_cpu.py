"""n-step returns (train.n_step, sac/nstep.py) without a GPU: the numpy statement of the definition against a
brute-force one written here, the discount powers, the gate of a loop that stores its rows n - 1 vector steps
late, the stage's bookkeeping with the launch stubbed, the agent's refusals, and the host checks of
sac_replay_emit_nstep.  Every comparison of rows is bit for bit."""
import copy
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _control
from _gpu import FakeEnv


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. nstep_rows against the definition
def brute_force(obs, act, rew, nxt, done, gamma, n):
    """The definition, window by window: (rows, k of every window)."""
    gpow = [1.0]
    for _ in range(n):
        gpow.append(gpow[-1] * gamma)
    T, N = rew.shape
    W = T - n + 1
    out = [np.zeros((W, N) + x.shape[2:], np.float32) for x in (obs, act, rew, nxt, done)]
    ks = np.zeros((W, N), np.int64)
    for s in range(W):
        for i in range(N):
            k = n
            for j in range(n):
                if done[s + j, i] == 1:
                    k = j + 1
                    break
            acc = gpow[0] * float(rew[s, i])
            for j in range(1, k):
                acc = acc + gpow[j] * float(rew[s + j, i])
            out[0][s, i], out[1][s, i] = obs[s, i], act[s, i]
            out[2][s, i] = np.float32(acc)
            out[3][s, i], out[4][s, i] = nxt[s + k - 1, i], done[s + k - 1, i]
            ks[s, i] = k
    return out, ks


def trajectories(episode_lengths, O=3, A=2, seed=0):
    """One-step rows [T][N][...] of N environments whose consecutive episodes have the given lengths (one list
    per environment, all of the same total T): done = 1 on the last step of every episode."""
    rng = np.random.default_rng(seed)
    N, T = len(episode_lengths), sum(episode_lengths[0])
    assert all(sum(l) == T for l in episode_lengths)
    done = np.zeros((T, N), np.float32)
    for i, lengths in enumerate(episode_lengths):
        done[np.cumsum(lengths) - 1, i] = 1.0
    obs = rng.standard_normal((T, N, O)).astype(np.float32)
    act = rng.standard_normal((T, N, A)).astype(np.float32)
    nxt = rng.standard_normal((T, N, O)).astype(np.float32)
    rew = (rng.standard_normal((T, N)) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(np.float32)
    return obs, act, rew, nxt, done


def episode_sets(n):
    """Episodes shorter than n, equal to n and longer than n, and two ends inside one window."""
    sets = [[1, 1, n, 2 * n + 1, n + 1, 1, 1, 2, n],  # 1, 1: two ends inside one window (n >= 2)
            [3 * n, 2, 1, n, n + 4]]
    if n > 1:
        sets.append([n - 1, n - 1, 2 * n + 3, 1, n])
    T = max(sum(s) for s in sets)
    return [s + [1] * (T - sum(s)) for s in sets] + [[T]]  # and one environment that never ends before T


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_nstep_rows_match_the_definition(n):
    from sac.nstep import discount_powers, nstep_rows

    gamma = 0.99
    obs, act, rew, nxt, done = trajectories(episode_sets(n), seed=n)
    want, ks = brute_force(obs, act, rew, nxt, done, gamma, n)
    got = nstep_rows(obs, act, rew, nxt, done, discount_powers(gamma, n))
    T = rew.shape[0]
    for g, w, name in zip(got, want, ("obs", "act", "rew", "next_obs", "done")):
        assert g.shape == w.shape and g.shape[0] == T - n + 1 and g.dtype == np.float32, name
        assert np.array_equal(bits(g), bits(w)), name
    assert sorted(set(ks.reshape(-1).tolist())) == list(range(1, n + 1))  # every k occurs
    if n >= 3:
        # two episode ends inside one window: the first wins (environment 0 starts with two one-step episodes)
        assert done[0, 0] == 1 and done[1, 0] == 1 and ks[0, 0] == 1
        assert np.array_equal(bits(got[3][0, 0]), bits(nxt[0, 0])) and bits(got[2][0, 0]) == bits(rew[0, 0])
    # a window that stays open bootstraps from step s + n - 1 and is not done
    open_w = ks == n
    assert open_w.any() and (got[4][open_w & (done[n - 1:] == 0)] == 0).all()
    assert (got[4][ks < n] == 1).all()


def test_nstep_rows_at_n_1_keep_every_reward_bit():
    from sac.nstep import discount_powers, nstep_rows

    obs, act, rew, nxt, done = trajectories([[2, 3, 1], [6]], seed=7)
    rew[0, 0], rew[1, 1], rew[2, 0] = -0.0, np.float32(1e-45), np.float32(-3.4e38)  # -0.0, a denormal, near the max
    got = nstep_rows(obs, act, rew, nxt, done, discount_powers(0.99, 1))
    for g, w in zip(got, (obs, act, rew, nxt, done)):
        assert np.array_equal(bits(g), bits(w))
    assert bits(got[2][0, 0]) == 0x80000000


def test_nstep_rows_shorter_than_a_window_give_nothing():
    from sac.nstep import discount_powers, nstep_rows

    obs, act, rew, nxt, done = trajectories([[2], [2]])
    got = nstep_rows(obs, act, rew, nxt, done, discount_powers(0.99, 3))
    assert [g.shape for g in got] == [(0, 2, 3), (0, 2, 2), (0, 2), (0, 2, 3), (0, 2)]


def test_discount_powers():
    from sac.nstep import discount_powers

    for gamma in (0.99, 0.995, 0.9, 1.0, 0.3):
        gpow = discount_powers(gamma, 8)
        assert len(gpow) == 9 and gpow[0] == 1.0 and gpow[1] == gamma
        acc = 1.0
        for j in range(1, 9):
            acc = acc * gamma
            assert gpow[j] == acc
    # repeated multiplication, not gamma ** j: they differ in the last bit for some j
    assert any(discount_powers(0.99, 8)[j] != 0.99 ** j for j in range(9))
    assert discount_powers(0.99, 1) == [1.0, 0.99]


# ---------------------------------------------------------------- 2. the gate
def reference_gate(T, N, n, cap, warming, uf, gs):
    """Gradient steps per vector step by the reference's rule, env step by env step: the rows of vector step v
    are stored, one per env step, only if v >= n - 1; an env step updates if can_update() holds after it and
    its index is a multiple of update_frequency."""
    total = length = 0
    out = []
    for v in range(T):
        emitted, count = v >= n - 1, 0
        for _ in range(N):
            total += 1
            if emitted:
                length = min(cap, length + 1)
            if length >= warming and total % uf == 0:
                count += gs
        out.append(count)
    return out


@pytest.mark.parametrize("n", [1, 3])
def test_staged_gate_matches_the_reference_gate(n):
    from sac.agent import due_updates_gated, due_updates_staged

    T = 12
    for N, cap, warming, uf, gs in itertools.product((1, 4, 7), (10, 40, 1000), (1, 5, 16, 30, 2000), (1, 3, 8),
                                                     (1, 2)):
        want = reference_gate(T, N, n, cap, warming, uf, gs)
        total = length = 0
        for v in range(T):
            emitted = N if v >= n - 1 else 0
            got = due_updates_staged(total, total + N, emitted, length, cap, warming, uf, gs)
            assert got == want[v], (n, N, cap, warming, uf, gs, v)
            if n == 1:
                assert got == due_updates_gated(total, total + N, length, cap, warming, uf, gs)
            total += N
            length = min(cap, length + emitted)
    # the simulation does gate: a warm-up that ends inside the run, and one that never ends
    assert 0 < sum(reference_gate(T, 4, n, 40, 16, 1, 1)) < T * 4 and sum(reference_gate(T, 4, n, 10, 16, 1, 1)) == 0


# ---------------------------------------------------------------- 3. the stage's bookkeeping
class FakeBuffer:
    """The host mirrors of a ReplayBuffer whose pushes move nothing."""

    def __init__(self, capacity):
        self.capacity, self._size, self._pos = capacity, 0, 0
        self.obs_dim, self.act_dim, self._alloc_done = 3, 1, True
        self.pushed = 0

    def push_batch(self, s, a, r, s2, d):
        n = len(r)
        self._size = min(self.capacity, self._size + n)
        self._pos = (self._pos + n) % self.capacity
        self.pushed += n

    def flush(self):
        pass


def make_stage(n, N, cap=23):
    from sac.nstep import NStepStage

    replay = FakeBuffer(cap)
    replay.device, replay.layout = torch.device("cpu"), "records"
    stage = NStepStage(n, N, replay, 0.99)
    assert stage.buffer.capacity == n * N and stage.buffer.layout == "records" and not stage.buffer._alloc_done
    stage.buffer = FakeBuffer(n * N)
    launches = []
    stage._launch = lambda newest: launches.append((newest, replay._size, replay._pos))
    return stage, replay, launches


def vector_step(N):
    return np.zeros((N, 3)), np.zeros((N, 1)), np.zeros(N), np.zeros((N, 3)), np.zeros(N, bool)


@pytest.mark.parametrize("n,N", [(1, 5), (3, 4), (8, 1)])
def test_stage_emits_from_the_nth_step_and_mirrors_a_push(n, N):
    from sac.nstep import discount_powers

    T, cap = 2 * n + 5, 23
    stage, replay, launches = make_stage(n, N, cap)
    assert stage.gpow == discount_powers(0.99, n)
    emitted = []
    for v in range(T):
        stage.push(*vector_step(N))
        assert stage.staged == v + 1
        assert stage.newest == (v % n) * N  # the slot the step's first row went to
        emitted.append(stage.emit())
        assert stage.emit() == 0  # the window of a step is emitted once
    assert emitted == [0] * (n - 1) + [N] * (T - n + 1)
    assert [l[0] for l in launches] == [(v % n) * N for v in range(n - 1, T)]
    # the launch is given the mirrors before the rows, which then advance as a push of N rows does
    assert [l[1:] for l in launches] == [(min(cap, j * N), (j * N) % cap) for j in range(T - n + 1)]
    assert (replay._size, replay._pos) == (min(cap, (T - n + 1) * N), ((T - n + 1) * N) % cap)
    # clear(): the next n - 1 steps emit nothing, wherever the staging ring stands
    stage.clear()
    assert stage.staged == 0
    again = []
    for _ in range(n + 1):
        stage.push(*vector_step(N))
        again.append(stage.emit())
    assert again == [0] * (n - 1) + [N, N]


def test_stage_counts_device_steps_and_detects_a_reset_without_clear():
    n, N = 3, 4
    stage, replay, launches = make_stage(n, N)
    buf = stage.buffer
    for t in (1, 2, 3, 4):  # the rollout kernel wrote the rows: the buffer's mirrors moved, then the stage counts
        buf.push_batch(*vector_step(N))
        stage.after_rollout(t)
        assert stage.emit() == (N if t >= n else 0)
    buf.push_batch(*vector_step(N))
    with pytest.raises(ValueError, match="reset without clear"):
        stage.after_rollout(1)  # the environments' t went back to 0: a reset nobody announced
    stage.clear()
    buf.push_batch(*vector_step(N))
    stage.after_rollout(1)
    assert stage.staged == 1 and stage.emit() == 0
    # rows that did not come through the stage
    buf.push_batch(*vector_step(N))
    buf.push_batch(*vector_step(N))
    with pytest.raises(ValueError, match="consecutive vector steps"):
        stage.after_rollout(2)
    stage, _, _ = make_stage(n, N)
    with pytest.raises(ValueError, match="one vector step"):
        stage.push(*vector_step(N + 1))
    with pytest.raises(ValueError, match="consecutive vector steps"):
        stage.after_rollout(1)  # nothing was written


def test_stage_refuses_a_bad_n():
    from sac.nstep import NStepStage

    replay = SimpleNamespace(device=torch.device("cpu"), layout="soa")
    for n in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError):
            NStepStage(n, 4, replay, 0.99)
    with pytest.raises(ValueError):
        NStepStage(2, 0, replay, 0.99)
    assert NStepStage(8, 4, replay, 0.99).buffer.layout == "soa"


# ---------------------------------------------------------------- 4. SAC
def cpu_agent(n_step=None):
    from sac.agent import SAC

    cfg = copy.deepcopy(_control.cfg("pendulum", hidden=(16, 16)))
    cfg["train"].update(device="cpu", engine_device="cpu")
    if n_step is not None:
        cfg["train"]["n_step"] = n_step
    return SAC(FakeEnv(3, 1), cfg)


@pytest.mark.parametrize("bad", [0, 9, -2, 2.5, "3", True, None])
def test_agent_refuses_n_step_out_of_range(bad):
    from sac.agent import SAC

    cfg = copy.deepcopy(_control.cfg("pendulum", hidden=(16, 16)))
    cfg["train"].update(device="cpu", engine_device="cpu", n_step=bad)
    with pytest.raises(ValueError, match="train.n_step"):
        SAC(FakeEnv(3, 1), cfg)


def test_agent_discount_is_gamma_to_the_n():
    a = cpu_agent()
    assert a.n_step == 1 and a._discount() == 0.99 and a._new_stage(4) is None
    a = cpu_agent(1)
    assert a._discount() == 0.99
    a = cpu_agent(3)
    assert a.n_step == 3 and a.gpow == [1.0, 0.99, 0.99 * 0.99, 0.99 * 0.99 * 0.99]
    assert a._discount() == 0.99 * 0.99 * 0.99
    stage = a._new_stage(4)
    assert stage.n == 3 and stage.num_envs == 4 and stage.replay is a.replay_buffer and stage.gpow == a.gpow
    assert cpu_agent(8).n_step == 8


def test_agent_refuses_what_stores_one_step_rows():
    from sac import _engine as E

    a = cpu_agent(3)
    z = np.zeros(3, np.float32)
    calls = {
        "run_training_loop": lambda ag: ag.run_training_loop(1),
        "store_transition": lambda ag: ag.store_transition(z, np.zeros(1), 0.0, z, False),
        "warmup_replay_buffer": lambda ag: ag.warmup_replay_buffer(ag.env, 1),
        "graph_steps": lambda ag: ag.run_device_training_loop(10, graph_steps=2),
        "device_q_values": lambda ag: ag.run_device_training_loop(10, device_q_values=True),
    }
    for key, call in calls.items():
        with pytest.raises(ValueError, match=r"train\.n_step = 3: " + key):
            call(a)
    # at n_step = 1 none of them is refused for that reason
    one = cpu_agent(1)
    with pytest.raises(E.EngineUnavailable):
        calls["store_transition"](one)
    with pytest.raises(TypeError, match="DeviceVectorEnv"):
        calls["graph_steps"](one)


def test_train_replicas_n_step_argument():
    from sac.nstep import n_step_refusal
    from sac.train_replicas import parse_args

    a = parse_args(["--config", "c.yaml", "--n-step", "3", "--device-envs"])
    assert a.n_step == 3
    assert parse_args(["--config", "c.yaml"]).n_step is None
    assert parse_args(["--config", "c.yaml", "--n-step", "1", "--device-envs", "--graph-steps", "4"]).graph_steps == 4
    with pytest.raises(SystemExit) as e:
        parse_args(["--config", "c.yaml", "--n-step", "3", "--device-envs", "--graph-steps", "4"])
    assert str(e.value) == n_step_refusal(3, "graph_steps")
    with pytest.raises(ValueError) as v:
        cpu_agent(3).run_device_training_loop(10, graph_steps=4)
    assert str(v.value) == str(e.value)  # the same message
    with pytest.raises(SystemExit, match="--n-step"):
        parse_args(["--config", "c.yaml", "--n-step", "9"])


# ---------------------------------------------------------------- 5. host checks of the entry point
@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    return E.load_library()


def tables(E, n=3, N=4, cap=50, O=3, A=1):
    """Descriptors with made-up non-null addresses: every call below fails its host checks before any HIP call,
    so nothing is ever read through them."""
    def desc(base, capacity):
        return E.ReplayDesc(base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000, capacity, O, A,
                            base + 0x5000, 0)

    return desc(0x10000, n * N), desc(0x80000, cap)


def test_emit_nstep_checks_every_argument(lib):
    from sac import _engine as E
    from sac.nstep import discount_powers

    n, N, cap = 3, 4, 50
    gp = (ctypes.c_double * 8)(*discount_powers(0.99, 7))

    def call(stage, rb, n_=n, N_=N, newest=0, gpow=gp, size=0, pos=0):
        rc = lib.sac_replay_emit_nstep(None if stage is None else ctypes.byref(stage),
                                       None if rb is None else ctypes.byref(rb), n_, N_, newest, gpow, size, pos, None)
        return rc, lib.sac_last_error().decode()

    def edited(which, **fields):
        st, rb = tables(E, n, N, cap)
        for k, v in fields.items():
            setattr(st if which == "stage" else rb, k, v)
        return st, rb

    st, rb = tables(E, n, N, cap)
    bad = {
        "null stage": call(None, rb),
        "null rb": call(st, None),
        "null stage field": call(*edited("stage", rew=None)),
        "null stage obs": call(*edited("stage", obs=None)),
        "null rb field": call(*edited("rb", next_obs=None)),
        "null rb state": call(*edited("rb", state=None)),
        "null gpow": call(st, rb, gpow=None),
        "n = 0": call(st, rb, n_=0),
        "n = 9": call(st, rb, n_=9),
        "num_envs = 0": call(st, rb, N_=0),
        "stage capacity": call(*edited("stage", capacity=n * N + 1)),
        "stage capacity for another n": call(st, rb, n_=2),
        "obs_dim differs": call(*edited("stage", obs_dim=4)),
        "act_dim differs": call(*edited("rb", act_dim=2)),
        "num_envs > capacity": call(*edited("rb", capacity=N - 1)),
        "newest < 0": call(st, rb, newest=-1),
        "newest past the table": call(st, rb, newest=n * N),
        "size < 0": call(st, rb, size=-1),
        "size > capacity": call(st, rb, size=cap + 1),
        "pos < 0": call(st, rb, pos=-1),
        "pos = capacity": call(st, rb, pos=cap),
        "same table": call(st, st),
        "same storage": call(st, tables(E, n, N, cap)[0]),  # another descriptor of the same fields
    }
    for what, (rc, msg) in bad.items():
        assert rc == -1 and msg.startswith("emit_nstep: "), (what, rc, msg)
    assert "same table" in bad["same table"][1] and "same table" in bad["same storage"][1]
    assert "1..8" in bad["n = 9"][1] and "n * num_envs" in bad["stage capacity"][1]
    assert "newest" in bad["newest < 0"][1] and "(size, pos)" in bad["pos = capacity"][1]
    with pytest.raises(E.EngineError, match="emit_nstep"):
        E.check(bad["n = 0"][0])
