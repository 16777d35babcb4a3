"""Time-limit bootstrapping (train.bootstrap_truncated) without a GPU: the numpy statement of the
coded n-step definition against a plain Python loop, the bound on the discount a fractional done gives, the form
of the oracle's target that the fractional done relies on, the agent's handling of the key on the host loops, and
the host checks of the two new entry points.  Every comparison of rows is bit for bit."""
import copy
import ctypes

import numpy as np
import pytest

import _control
from _fixtures import batch, eps, oracle_state
from _gpu import FakeEnv

F32 = np.float32
GAMMAS = (0.5, 0.8, 0.9, 0.95, 0.99, 0.995, 0.999, 1.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. nstep_rows(codes=True) against the definition
def brute_force_codes(obs, act, rew, nxt, code, gamma, n):
    """§3.12 window by window: (rows, k of every window, closing code of every window)."""
    gpow = [1.0]
    for _ in range(n):
        gpow.append(gpow[-1] * gamma)
    T, N = rew.shape
    W = T - n + 1
    out = [np.zeros((W, N) + x.shape[2:], np.float32) for x in (obs, act, rew, nxt, code)]
    ks, closing = np.zeros((W, N), np.int64), np.zeros((W, N), np.int64)
    for s in range(W):
        for i in range(N):
            k = n
            for j in range(n):
                if code[s + j, i] != 0:
                    k = j + 1
                    break
            acc = gpow[0] * float(rew[s, i])
            for j in range(1, k):
                acc = acc + gpow[j] * float(rew[s + j, i])
            c = int(code[s + k - 1, i])
            if c == 0:
                done = np.float32(0.0)
            elif c == 2:
                done = np.float32(1.0 - gpow[k] / gpow[n])
            else:
                done = np.float32(1.0)
            out[0][s, i], out[1][s, i] = obs[s, i], act[s, i]
            out[2][s, i] = np.float32(acc)
            out[3][s, i], out[4][s, i] = nxt[s + k - 1, i], done
            ks[s, i], closing[s, i] = k, c
    return out, ks, closing


def random_steps(rng, T, N, codes, O=3, A=2):
    obs = rng.standard_normal((T, N, O)).astype(np.float32)
    act = rng.standard_normal((T, N, A)).astype(np.float32)
    nxt = rng.standard_normal((T, N, O)).astype(np.float32)
    rew = (rng.standard_normal((T, N)) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(np.float32)
    code = np.where(rng.random((T, N)) < 0.25, rng.choice(codes, (T, N)), 0).astype(np.float32)
    return obs, act, rew, nxt, code


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_coded_rows_match_the_definition(n):
    from sac.nstep import discount_powers, nstep_rows

    T, N, gamma = 12, 5, 0.99
    gpow = discount_powers(gamma, n)
    seen_k, seen_c = set(), set()
    for seed in range(40):  # T * N = 60 rows a draw: enough draws that every k and every closing code occurs
        steps = random_steps(np.random.default_rng(100 * n + seed), T, N, (1, 2, 3))
        want, ks, closing = brute_force_codes(*steps, gamma, n)
        got = nstep_rows(*steps, gpow, codes=True)
        for g, w, name in zip(got, want, ("obs", "act", "rew", "next_obs", "done")):
            assert g.shape == w.shape and g.shape[0] == T - n + 1 and g.dtype == np.float32, name
            assert np.array_equal(bits(g), bits(w)), (name, seed)
        ended = closing != 0
        seen_k |= set(ks[ended].tolist())
        seen_c |= set(closing.reshape(-1).tolist())
        d = got[4]
        assert (bits(d[closing == 0]) == 0).all()  # +0.0, sign bit included
        assert (d[(closing == 1) | (closing == 3)] == 1).all()
        trunc = closing == 2
        assert (bits(d[trunc & (ks == n)]) == 0).all() and (d[trunc & (ks < n)] < 0).all()
    assert seen_k == set(range(1, n + 1)) and seen_c == {0, 1, 2, 3}, (seen_k, seen_c)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_codes_0_and_1_give_the_flag_rows(n):
    from sac.nstep import discount_powers, nstep_rows

    gpow = discount_powers(0.99, n)
    steps = random_steps(np.random.default_rng(n), 12, 5, (1,))
    assert set(np.unique(steps[4]).tolist()) == {0.0, 1.0}
    for g, w in zip(nstep_rows(*steps, gpow, codes=True), nstep_rows(*steps, gpow)):
        assert np.array_equal(bits(g), bits(w))


def test_end_codes():
    from sac.nstep import end_codes

    te = np.array([False, True, False, True])
    tr = np.array([False, False, True, True])
    c = end_codes(te, tr)
    assert c.dtype == np.float32 and c.tolist() == [0.0, 1.0, 2.0, 3.0]


# ---------------------------------------------------------------- 2. the discount a fractional done gives
def test_fractional_done_gives_gamma_to_the_k_within_4_ulps():
    """fl(fp32(gpow[n]) * fl(1 - d')) against gpow[k]: four fp32 roundings (d', 1 - d', gamma_eff, the product) of
    at most 2^-24 relative error each, so at most 4 fp32 ulps of gamma^k."""
    from sac.nstep import discount_powers

    worst = 0.0
    for gamma in GAMMAS:
        for n in range(1, 9):
            gpow = discount_powers(gamma, n)
            g_eff = F32(gpow[n])
            for k in range(1, n + 1):
                d = F32(1.0 - gpow[k] / gpow[n])
                if k == n:
                    assert bits(d) == 0, (gamma, n)  # +0.0
                else:
                    assert d < 0 or gamma == 1.0, (gamma, n, k)
                disc = F32(g_eff * F32(F32(1.0) - d))
                ulp = float(np.spacing(F32(gpow[k])))
                err = abs(float(disc) - gpow[k]) / ulp
                worst = max(worst, err)
                assert err <= 4.0, (gamma, n, k, err)
    print(f"largest error {worst:.2f} fp32 ulps of gamma^k")
    assert worst > 0.0


# ---------------------------------------------------------------- 3. the oracle's target reads d as a float
def test_oracle_target_has_the_one_minus_d_form():
    """oracle/sac_oracle.py computes y = r + (gamma (1 - d)) (min Q' - alpha log pi') with d as the float it is:
    on a batch whose done holds 0, 1 and the negative fractions of §3.12, y equals that expression in float64."""
    from oracle import sac_oracle as O
    from sac.nstep import discount_powers

    st, hp, fx, _ = oracle_state("c1_auto")
    b = batch(fx, 1)
    et, ea = eps(fx, 1)
    B = np.asarray(b.r).shape[0]
    gpow = discount_powers(0.99, 8)
    fractions = [F32(1.0 - gpow[k] / gpow[8]) for k in range(1, 8)]
    d = np.zeros(B, np.float32)
    d[1::3] = 1.0
    d[2::3] = [fractions[i % len(fractions)] for i in range(len(d[2::3]))]
    assert (d == 0).sum() >= 4 and (d == 1).sum() >= 4 and (d < 0).sum() >= 4
    a2, lp2, _ = O.policy_sample(st.pi, np.asarray(b.s2, F32), et, hp.policy)
    q1, _ = O.q_forward(st.q1t, np.asarray(b.s2, F32), a2)
    q2, _ = O.q_forward(st.q2t, np.asarray(b.s2, F32), a2)
    soft = np.minimum(q1, q2).astype(np.float64) - float(F32(st.alpha)) * lp2.astype(np.float64)
    want = np.asarray(b.r, np.float64) + float(F32(hp.gamma)) * (1.0 - d.astype(np.float64)) * soft
    ref = O.training_step(st, hp, O.Batch(b.s, b.a, b.r, b.s2, d), et, ea)
    err = np.abs(ref["y"].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-6, err.max()
    # the rows differ by kind: a fractional row bootstraps with more than gamma, a terminal one not at all
    assert np.array_equal(ref["y"][d == 1], np.asarray(b.r, F32)[d == 1])
    frac = d < 0
    plain = np.asarray(b.r, np.float64) + float(F32(hp.gamma)) * soft
    assert (np.abs(ref["y"][frac] - plain[frac]) > 1e-5 * np.abs(soft[frac])).all()


# ---------------------------------------------------------------- 4. the key on the host loops
def cpu_cfg(**train):
    cfg = copy.deepcopy(_control.cfg("point_mass", hidden=(16, 16), warming=10 ** 9))
    cfg["train"].update(device="cpu", engine_device="cpu", **train)
    return cfg


def test_key_defaults_to_off_and_takes_a_bool_only():
    from sac.agent import SAC

    assert SAC.bootstrap_truncated is False
    assert SAC(FakeEnv(1, 1), cpu_cfg()).bootstrap_truncated is False
    assert SAC(FakeEnv(1, 1), cpu_cfg(bootstrap_truncated=False)).bootstrap_truncated is False
    on = SAC(FakeEnv(1, 1), cpu_cfg(bootstrap_truncated=True, n_step=3))
    assert on.bootstrap_truncated is True
    assert on._new_stage(4).bootstrap_truncated is True
    assert SAC(FakeEnv(1, 1), cpu_cfg(n_step=3))._new_stage(4).bootstrap_truncated is False
    for bad in (1, 0, "true", "false", None, 1.0, [True]):
        with pytest.raises(ValueError, match=r"train\.bootstrap_truncated"):
            SAC(FakeEnv(1, 1), cpu_cfg(bootstrap_truncated=bad))


class Rows:
    """A replay buffer that keeps what it is given."""

    def __init__(self):
        self.rows = []

    def push(self, s, a, r, s2, d):
        assert isinstance(d, bool)
        self.rows.append((np.array(s, np.float32), np.array(a, np.float32), float(r), np.array(s2, np.float32), d))

    def __len__(self):
        return len(self.rows)


def host_run(option, what):
    """The rows a host loop stores on a point mass whose episodes end by reaching the goal, by the time limit of 4
    steps, or by both at the fourth step; and the (terminated, truncated) of every step."""
    from sac.agent import SAC
    from sac.envs import OneDPointMassReachEnv

    flags = []

    class Env(OneDPointMassReachEnv):
        def step(self, action):
            out = super().step(action)
            flags.append((bool(out[2]), bool(out[3])))
            return out

    env = Env(goal_pos=0.2, max_steps=4, goal_tolerance=0.05)
    agent = SAC(env, cpu_cfg(bootstrap_truncated=option) if option is not None else cpu_cfg())
    agent.replay_buffer = Rows()
    rng = np.random.default_rng(11)
    agent.select_action = lambda state, deterministic=False: rng.uniform(-0.02, 0.1, 1).astype(np.float32)
    env.action_space.seed(5)
    if what == "loop":
        agent.run_training_loop(60, tqdm_disable=True)
    else:
        agent.warmup_replay_buffer(env, 240)
    return agent.replay_buffer.rows, flags


@pytest.mark.parametrize("what", ["loop", "warmup"])
def test_host_loops_store_terminated_alone(what):
    off, flags = host_run(None, what)
    on, flags_on = host_run(True, what)
    also_off, _ = host_run(False, what)
    assert flags == flags_on and len(off) == len(on) == len(flags) >= 100
    kinds = set(flags)
    assert {(False, False), (True, False), (False, True)} <= kinds, kinds  # both kinds of end occur
    print(what, {k: flags.count(k) for k in sorted(kinds)})
    for row_off, row_on, row_f, (te, tr) in zip(off, on, also_off, flags):
        assert row_off[4] == (te or tr) and row_on[4] == te and row_f[4] == (te or tr)
        for x, y, z in zip(row_off[:4], row_on[:4], row_f[:4]):  # nothing else in the row changes
            assert np.array_equal(x, y) and np.array_equal(x, z)


def test_train_replicas_flag():
    from sac.train_replicas import parse_args

    assert parse_args(["--config", "c.yaml"]).bootstrap_truncated is False
    a = parse_args(["--config", "c.yaml", "--bootstrap-truncated", "--device-envs", "--graph-steps", "4"])
    assert a.bootstrap_truncated is True and a.graph_steps == 4
    assert parse_args(["--config", "c.yaml", "--bootstrap-truncated", "--n-step", "3"]).n_step == 3


def test_push_batch_keeps_flags_unless_told():
    """ReplayBuffer.push_batch(done_values=True) is what lets a host stage hold end codes; the default still turns
    dones into 0 / 1 (checked on the packing, which needs no device)."""
    import inspect

    from sac.replay_buffer import ReplayBuffer

    sig = inspect.signature(ReplayBuffer.push_batch)
    assert sig.parameters["done_values"].default is False


# ---------------------------------------------------------------- 5. host checks of the entry points
@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    return E.load_library()


def test_set_done_mode_checks_the_mode(lib):
    from sac import _engine as E

    assert (E.DONE_ANY_END, E.DONE_TERMINATED, E.DONE_END_CODE) == (0, 1, 2)
    for bad in (3, -1, 100):
        assert lib.sac_engine_set_done_mode(None, bad) == -1
        msg = lib.sac_last_error().decode()
        assert msg.startswith("set_done_mode: mode") and "0..2" in msg, msg
    for mode in (0, 1, 2):  # a valid mode gets as far as the null engine
        assert lib.sac_engine_set_done_mode(None, mode) == -1
        assert "null engine" in lib.sac_last_error().decode()


def tables(E, n=3, N=4, cap=50, O=3, A=1):
    """Descriptors with made-up non-null addresses: every call below fails its host checks before any HIP call,
    so nothing is ever read through them."""
    def desc(base, capacity):
        return E.ReplayDesc(base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000, capacity, O, A,
                            base + 0x5000, 0)

    return desc(0x10000, n * N), desc(0x80000, cap)


def test_emit_nstep_codes_checks_every_argument(lib):
    from sac import _engine as E
    from sac.nstep import discount_powers

    n, N, cap = 3, 4, 50
    gp = (ctypes.c_double * 9)(*discount_powers(0.99, 8))

    def call(stage, rb, n_=n, N_=N, newest=0, gpow=gp, size=0, pos=0):
        rc = lib.sac_replay_emit_nstep_codes(None if stage is None else ctypes.byref(stage),
                                             None if rb is None else ctypes.byref(rb), n_, N_, newest, gpow, size,
                                             pos, None)
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
        "null stage field": call(*edited("stage", done=None)),
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
        "stride below a field": call(*edited("rb", row_stride=2)),
        "num_envs > capacity": call(*edited("rb", capacity=N - 1)),
        "newest < 0": call(st, rb, newest=-1),
        "newest past the table": call(st, rb, newest=n * N),
        "size < 0": call(st, rb, size=-1),
        "size > capacity": call(st, rb, size=cap + 1),
        "pos < 0": call(st, rb, pos=-1),
        "pos = capacity": call(st, rb, pos=cap),
        "same table": call(st, st),
        "same storage": call(st, tables(E, n, N, cap)[0]),
    }
    for what, (rc, msg) in bad.items():
        assert rc == -1 and msg.startswith("emit_nstep: "), (what, rc, msg)
    assert "same table" in bad["same table"][1] and "same table" in bad["same storage"][1]
    assert "1..8" in bad["n = 9"][1] and "n * num_envs" in bad["stage capacity"][1]
    assert "newest" in bad["newest < 0"][1] and "(size, pos)" in bad["pos = capacity"][1]
