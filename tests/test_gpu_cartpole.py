"""The device-resident balancing cart-pole on the MI355X, the one environment
whose episodes end by failure, at different steps in different rows: the step
kernel against sac.control_envs.CartPoleEnv, the fused rollout step against the
step kernel and sac_policy_act, the loop graph against the stepwise loop, the
per-row evaluation SAC.evaluate_device(episodes_per_env=k), and a training run
whose evaluation return has to pass a bar set by scripted policies on the host
class alone.

Equality rules.  sin th and cos th feed back into the cart-pole's state, so
device against host is NOT bit for bit: the device library's values differ from
the host libm's by a few float64 ulps, and over at most 60 steps of an unstable
pole (growth rate about 4 / s, so at most x ~100 over 1.2 s) the difference
stays far below fp32 resolution.  Every fp32 observation is within ONE fp32 ulp
of the host's; the float64 state is within 1e-12 absolute (states are of
magnitude <= 10: four orders above the propagated libm difference, many orders
below any wrong term).  Rewards, flags, counters, lengths, ended marks and
returns (sums of 1.0) are exact: every terminating state of the host is more
than 1e-9 outside the limit it broke (asserted here and in
tests/test_cartpole_cpu.py), so a state within 1e-12 of it breaks the same
limit.  Device against device (fused step against step kernel and policy_act,
graph against stepwise, the two evaluation rules) is bit for bit."""
import ctypes
import math
from functools import partial

import numpy as np
import pytest
import torch

import _control
from _control import DEV, bits, raw, twin_of, within_one_ulp

pytestmark = pytest.mark.gpu

u64, i32, vp = ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
f64p = ctypes.POINTER(ctypes.c_double)
X_LIMIT, TH_LIMIT = 2.4, 12 * 2 * math.pi / 360


_cfg = partial(_control.cfg, "cartpole")
make_agent = partial(_control.make_agent, _cfg, "CartPoleEnv")


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    lb = E.load_library()
    lb.sac_debug_rollout_eps_device.argtypes = [u64, u64, i32, i32, vp, vp]
    lb.sac_debug_rollout_eps_device.restype = ctypes.c_int
    lb.sac_debug_cartpole_reset_host.argtypes = [u64, u64, i32, f64p]
    lb.sac_debug_cartpole_reset_host.restype = ctypes.c_int
    return lb


def host_states(dstate):
    """CartPoleEnv.state of every row, [N][4], from the device's float64 rows (x, th, episode return, xdot, thdot)."""
    return np.stack([dstate[0], dstate[3], dstate[1], dstate[4]], axis=1)


def feedback(state):
    """The linear feedback of tests/test_cartpole_cpu.py: it balances, so its rows reach max_steps."""
    x, xdot, th, thdot = state
    return float(np.clip(np.float32(0.1 * x + 0.3 * xdot + 4.0 * th + 0.6 * thdot), -1.0, 1.0))


# ---------------------------------------------------------------- 1. step kernel against the host class
def test_step_matches_host_class(lib):
    from sac.control_envs import CartPoleEnv
    from sac.device_envs import DeviceVectorEnv

    N, max_steps, T, seed = 37, 60, 120, 11  # three workgroups of SAC_ROWS = 16 rows, the last partial
    pinned = (5, 30)  # rows that take the feedback law's action: they balance, so truncations are certain
    dv = DeviceVectorEnv.from_env(CartPoleEnv(max_steps=max_steps), N, device=DEV)
    assert dv.obs_dim == 4 and dv.act_dim == 1 and tuple(dv.dstate.shape) == (5, N) and dv.kind_code == 32
    hosts = [CartPoleEnv(max_steps=max_steps) for _ in range(N)]
    obs0, info = dv.reset(seed=seed)
    assert info == {} and obs0.is_cuda and tuple(obs0.shape) == (N, 4)

    def adopt(rows, t):  # the host instances take the reset draws of step t (their own generator's differ by design)
        for i in rows:
            st = (ctypes.c_double * 4)()
            assert lib.sac_debug_cartpole_reset_host(seed, t, i, st) == 0
            hosts[i].reset()
            hosts[i].state = list(st)

    worst = {"state": 0.0}

    def assert_state_is_the_hosts(what, exact_rows=()):
        got = host_states(dv.dstate.cpu().numpy())
        want = np.array([h.state for h in hosts], np.float64)
        err = np.abs(got - want)
        worst["state"] = max(worst["state"], float(err.max()))
        assert err.max() <= 1e-12, (what, float(err.max()), np.argwhere(err > 1e-12)[:4])
        for i in exact_rows:  # a reset draw holds no sine or cosine: bit for bit
            assert np.array_equal(got[i].view(np.uint64), want[i].view(np.uint64)), (what, i)
        return got

    adopt(range(N), 0)
    st = assert_state_is_the_hosts("reset", range(N))
    assert np.all(np.abs(st) <= 0.05) and len(np.unique(st)) == 4 * N
    assert np.array_equal(bits(obs0.cpu().numpy()), bits(st.astype(np.float32)))
    rng = np.random.default_rng(100 + N)
    actions = rng.uniform(-1.5, 1.5, size=(T, N, 1)).astype(np.float32)  # a third of them beyond the force bound
    ep_len, cells, margins = np.zeros(N, np.int64), [], []
    n_diff = n_all = 0
    for t in range(T):
        for i in pinned:
            actions[t, i, 0] = feedback(hosts[i].state)
        o, r, te, tr, inf = dv.step(torch.from_numpy(actions[t]).to(DEV))
        assert all(x.is_cuda for x in (o, r, te, tr, inf["final_obs"])) and te.dtype == torch.bool
        o, r, te, tr, fin = (x.cpu().numpy() for x in (o, r, te, tr, inf["final_obs"]))
        want = [h.step(actions[t, i]) for i, h in enumerate(hosts)]
        w_fin = np.stack([w[0] for w in want])
        w_term = np.array([w[2] for w in want], bool)
        w_trunc = np.array([w[3] for w in want], bool)
        margins += [max(abs(h.state[0]) - X_LIMIT, abs(h.state[2]) - TH_LIMIT) for h, e in zip(hosts, w_term) if e]
        assert np.array_equal(te, w_term) and np.array_equal(tr, w_trunc), t
        assert np.all(r == 1.0) and r.dtype == np.float32
        n_diff += within_one_ulp(fin, w_fin, f"step {t + 1} final_obs")
        n_all += fin.size
        ep_len += 1
        w_done = w_term | w_trunc
        cells.append((ep_len.copy(), w_done.copy(), w_term.copy(), w_trunc.copy()))
        ep_len[w_done] = 0
        # the failed state is what final_obs holds; a row that ended starts again from this step's draw
        assert np.all((np.abs(fin[w_term, 0]) > X_LIMIT) | (np.abs(fin[w_term, 2]) > TH_LIMIT))
        adopt(np.nonzero(w_done)[0], t + 1)
        w_cur = np.stack([h._obs() for h in hosts])
        assert_state_is_the_hosts(f"step {t + 1}", np.nonzero(w_done)[0])
        n_diff += within_one_ulp(o, w_cur, f"step {t + 1} obs after autoreset")
        n_all += o.size
        assert np.all(np.abs(o[w_done]) <= 0.05)
        counters = dv.counters.cpu().numpy()
        assert np.array_equal(counters[0], [h.current_step for h in hosts]), t
        assert np.array_equal(counters[1], ep_len), t
    print(f"{n_diff} of {n_all} fp32 elements not identical to the host's; float64 state max |device - host| "
          f"{worst['state']:.3e}; smallest margin of a terminating host state {min(margins):.3e}")
    assert min(margins) > 1e-9  # the precondition of the exact flags (module docstring)
    # the episode ring: returns (sums of 1.0), lengths and ended marks exact
    ring = dv.ring.cpu()
    ints = ring[..., 1].contiguous().view(torch.int32).reshape(ring.shape[0], N, 2).numpy()
    rets = ring[..., 0].numpy()
    for t, (w_len, w_end, _, _) in enumerate(cells, start=1):
        c = t % dv.ring_steps
        assert np.array_equal(ints[c, :, 0], w_len) and np.array_equal(ints[c, :, 1], w_end.astype(np.int32)), t
        assert np.array_equal(rets[c], w_len.astype(np.float64)), t
    end_steps = [t for t, c in enumerate(cells, start=1) if c[1].any()]
    n_term, n_trunc = sum(int(c[2].sum()) for c in cells), sum(int(c[3].sum()) for c in cells)
    print(f"rows ended at {len(end_steps)} distinct vector steps; {n_term} terminated, {n_trunc} truncated")
    assert len(end_steps) >= 10 and n_term >= 10 and n_trunc >= 2  # rows do not move in lockstep
    assert all(cells[max_steps - 1][3][i] and not cells[max_steps - 1][2][i] for i in pinned)


# ---------------------------------------------------------------- 2. the fused rollout step
# rows that fail within one to three steps whatever the (bounded) force: (row, [x, xdot, th, thdot])
DOOMED = [(0, [0.0, 0.0, 0.2, 1.0]), (1, [0.0, 0.0, -0.2, -1.0]), (2, [2.39, 1.0, 0.0, 0.0]),
          (3, [-2.39, -1.0, 0.0, 0.0]), (17, [0.0, 0.0, 0.18, 1.0]), (18, [0.0, 0.0, -0.18, -1.0]),
          (35, [2.33, 1.5, 0.0, 0.0]), (36, [-2.33, -1.5, 0.0, 0.0])]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["records", "soa"])
def test_fused_rollout_matches_step_kernel_and_policy_act(lib, layout, precision):
    N, T, cap = 37, 7, 100  # the ring wraps on the third step, at a capacity that is no multiple of N
    agent, dv = make_agent(N, max_steps=5, precision=precision, layout=layout, capacity=cap, batch=16)
    eng, rb = agent.engine, agent.replay_buffer
    assert float(eng.cfg.action_scale) == 1.0 and int(eng.cfg.act_dim) == 1 and int(eng.cfg.obs_dim) == 4
    rb._alloc(dv.obs_dim, dv.act_dim)
    assert rb.layout == layout and tuple(rb.act.shape) == (cap, 1)
    for i, s in DOOMED:  # dstate rows: x, th, episode return, xdot, thdot; the observation is the state in fp32
        dv.dstate[:, i] = torch.tensor([s[0], s[2], 0.0, s[1], s[3]], dtype=torch.float64, device=DEV)
        dv.obs[i] = torch.tensor(s, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    gen0 = int(rb.state.cpu()[2])
    seed = int(eng.cfg.seed)
    dones, terms, truncs = [], [], []
    for t in range(1, T + 1):
        tw = twin_of(dv)
        before = dv.obs.clone()
        slots = (torch.arange(N, device=DEV) + rb._pos) % cap
        eng.rollout_step(dv, rb)
        got = {k: getattr(rb, k)[slots].clone() for k in ("obs", "act", "rew", "next_obs", "done")}
        # the stored action: policy_act on the observations the step saw with the step's Philox noise
        eps = torch.full((N, 1), float("nan"), device=DEV)
        assert lib.sac_debug_rollout_eps_device(seed, t, N, 1, eps.data_ptr(), None) == 0
        want_act = eng.policy_act(before, eps)
        assert tuple(want_act.shape) == (N, 1) and torch.equal(raw(got["act"]), raw(want_act)), t
        # the stored transition: the step kernel's from the same state with those actions, bit for bit
        o, r, te, tr, inf = tw.step(got["act"])
        assert torch.equal(raw(got["obs"]), raw(before)), t
        assert torch.equal(raw(got["next_obs"]), raw(inf["final_obs"])), t
        assert torch.equal(raw(got["rew"]), raw(r)) and bool((got["rew"] == 1.0).all()), t
        assert torch.equal(got["done"].reshape(-1), (te | tr).to(torch.float32)), t  # 1.0 on both kinds of ending
        for name in ("obs", "counters", "dstate", "ring"):
            assert torch.equal(raw(getattr(dv, name)), raw(getattr(tw, name))), (t, name)
        assert torch.equal(raw(o), raw(dv.obs))
        te, tr = te.cpu().numpy(), tr.cpu().numpy()
        nxt, cur = got["next_obs"].cpu().numpy(), dv.obs.cpu().numpy()
        # next_obs of a failed row is the failed state; its current observation is the fresh draw
        assert np.all((np.abs(nxt[te, 0]) > X_LIMIT) | (np.abs(nxt[te, 2]) > TH_LIMIT))
        assert np.all((np.abs(nxt[~te, 0]) <= X_LIMIT) & (np.abs(nxt[~te, 2]) <= TH_LIMIT))
        assert np.all(np.abs(cur[te | tr]) <= 0.05) and np.array_equal(bits(cur[~(te | tr)]), bits(nxt[~(te | tr)]))
        dones.append(got["done"].cpu().numpy().reshape(-1))
        terms.append(te)
        truncs.append(tr)
    dones, terms, truncs = np.stack(dones), np.stack(terms), np.stack(truncs)
    doomed = [i for i, _ in DOOMED]
    others = [i for i in range(N) if i not in doomed]
    first_end = np.argmax(dones[:, doomed] > 0, axis=0) + 1
    print(f"doomed rows {doomed} failed at steps {first_end.tolist()}")
    assert np.all(terms[first_end - 1, doomed]) and set(first_end.tolist()) == {1, 2, 3}
    assert not terms[:, others].any() and np.array_equal(np.nonzero(truncs[:, others].all(axis=1))[0], [4])
    assert not truncs[:4].any()  # a doomed row, restarted at step k, is truncated at step k + 5 (or fails again)
    assert np.array_equal(dones, (terms | truncs).astype(np.float32))
    cells = DeviceCells(dv, 1, T)
    assert np.array_equal(cells.ended, terms | truncs)
    assert np.array_equal(cells.length[4, others], np.full(len(others), 5)) and np.array_equal(cells.ret, cells.length)
    assert np.array_equal(cells.length[first_end - 1, doomed], first_end)
    assert rb.state.cpu().tolist() == [cap, (T * N) % cap, gen0 + T] and (rb._size, rb._pos) == (cap, (T * N) % cap)

    # store = 0 (evaluation): the environments step, the replay and its generation stay
    storage0, state0 = raw(rb.storage), rb.state.cpu().tolist()
    tw = twin_of(dv)
    before = dv.obs.clone()
    eng.rollout_step(dv, rb, deterministic=True, store=False)
    torch.cuda.synchronize()
    assert torch.equal(storage0, raw(rb.storage)) and rb.state.cpu().tolist() == state0
    assert (rb._size, rb._pos) == (cap, (T * N) % cap)
    tw.step(eng.policy_act(before))
    for name in ("obs", "counters", "dstate"):
        assert torch.equal(raw(getattr(dv, name)), raw(getattr(tw, name))), name
    assert dv.t == T + 1


class DeviceCells:
    """The episode ring's cells of RNG steps t_first..t_last as numpy arrays [steps][N]: ret, length, ended."""

    def __init__(self, dv, t_first, t_last):
        host, ev = dv.episode_cells(t_first, t_last)
        ev.synchronize()
        ints = host[..., 1].contiguous().view(torch.int32).reshape(host.shape[0], host.shape[1], 2).numpy()
        self.ret, self.length, self.ended = host[..., 0].numpy().copy(), ints[..., 0].copy(), ints[..., 1] != 0


# ---------------------------------------------------------------- 3. device cursor and graph
class Logger:
    def __init__(self):
        self.episodes, self.q, self.hparams = [], [], []

    def log_episode_metrics(self, episode_idx, reward, length):
        self.episodes.append((episode_idx, reward, length))

    def log_q_values(self, q1, q2, step):
        self.q.append((step, q1, q2))

    def log_hparams(self, cfg, metrics):
        self.hparams.append(dict(metrics))


def test_training_loop_with_graph_steps_matches_stepwise():
    N, warming, V = 8, 64, 105
    total = (V - 1) * N + 5  # the warm-up ends with the eighth vector step; 96 whole steps and a ragged one follow
    runs = []
    for graph_steps in (0, 8):
        agent, dv = make_agent(N, max_steps=60, capacity=300, batch=32, warming=warming, log_episodes=True, log_q=True)
        logger = Logger()
        calls = []
        orig = agent.engine.loop_graph
        agent.engine.loop_graph = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        m = agent.run_device_training_loop(total, logger=logger, graph_steps=graph_steps, drain_every=8,
                                           device_q_values=True)
        torch.cuda.synchronize()
        agent.engine.check()
        state = dict(agent.engine.state_tensors(), storage=agent.replay_buffer.storage,
                     replay_state=agent.replay_buffer.state, env_obs=dv.obs, env_counters=dv.counters,
                     env_dstate=dv.dstate, env_ring=dv.ring)
        assert dv.t == V <= dv.ring_steps
        runs.append(dict(metrics=m, episodes=logger.episodes, q=logger.q, state={k: raw(v) for k, v in state.items()},
                         graphs=len(calls), cells=DeviceCells(dv, 1, V)))
    a, b = runs
    assert a["graphs"] == 0 and b["graphs"] >= 4
    assert a["metrics"] == b["metrics"] and a["metrics"]["total_env_steps"] == V * N
    assert a["metrics"]["gradient_steps"] == V * N - (warming - 1)
    assert a["episodes"] == b["episodes"] and len(a["episodes"]) == a["metrics"]["total_episodes"] >= N
    lengths = [length for _, _, length in a["episodes"]]
    assert all(1 <= length <= 60 and ret == float(length) for _, ret, length in a["episodes"])
    # episodes ended by failure, row by row, inside the blocks the graph replays (vector steps 9 .. 104)
    ended = b["cells"].ended
    assert int(ended.sum()) == len(lengths) and np.array_equal(ended, a["cells"].ended)
    steps, rows = np.nonzero(ended[8:V - 1])
    print(f"{len(lengths)} episodes, lengths {min(lengths)}..{max(lengths)}; inside graph blocks: {len(steps)} ends at "
          f"{len(set(steps.tolist()))} distinct steps in {len(set(rows.tolist()))} rows")
    assert len(set(steps.tolist())) >= 6 and len(set(rows.tolist())) >= 6 and len(set(lengths)) >= 4
    assert len(set((steps % 8).tolist())) >= 3  # not on the blocks' boundaries only
    assert [s for s, _, _ in a["q"]] == [s for s, _, _ in b["q"]] == list(range(1, V * N + 1))
    qa = np.array([(q1, q2) for _, q1, q2 in a["q"]], np.float32).view(np.uint32)
    qb = np.array([(q1, q2) for _, q1, q2 in b["q"]], np.float32).view(np.uint32)
    assert np.array_equal(qa, qb) and len(np.unique(qa)) > 100
    bad = [k for k in a["state"] if not torch.equal(a["state"][k], b["state"][k])]
    assert not bad, f"graph_steps = 8 against stepwise: {bad} differ"
    assert a["state"].keys() >= {"param/pi", "param/q1", "storage", "env_dstate"}


# ---------------------------------------------------------------- 4. evaluation that variable lengths do not bias
def test_evaluate_device_per_env_takes_each_rows_first_episodes():
    N, k = 16, 3
    agent, dv = make_agent(N, max_steps=60, hidden=(32, 32), batch=16, ring_steps=256)  # 3 * 60 steps fit the ring
    rb = agent.replay_buffer
    rb._alloc(dv.obs_dim, dv.act_dim)
    torch.cuda.synchronize()
    storage0, state0 = raw(rb.storage), rb.state.cpu().tolist()
    got = agent.evaluate_device(episodes_per_env=k, vec_env=dv)
    assert torch.equal(storage0, raw(rb.storage)) and rb.state.cpu().tolist() == state0  # nothing stored
    assert 1 <= dv.t <= k * 60
    cells = DeviceCells(dv, 1, dv.t)
    picked, first_finished = [[] for _ in range(N)], []
    for t in range(cells.ended.shape[0]):
        for i in range(N):
            if cells.ended[t, i]:
                first_finished.append(cells.ret[t, i])
                if len(picked[i]) < k:
                    picked[i].append(cells.ret[t, i])
    assert all(len(p) == k for p in picked)
    want = float(np.mean([picked[i][e] for e in range(k) for i in range(N)]))
    lengths = sorted({int(x) for p in picked for x in p})
    print(f"per-row mean {got:.4f} over {N * k} episodes of lengths {lengths[0]}..{lengths[-1]} in {dv.t} steps; "
          f"first {N * k} finished: {np.mean(first_finished[:N * k]):.4f}")
    assert got == want and isinstance(got, float) and 1.0 <= got <= 60.0
    assert len(lengths) > 1  # the rows' episodes are of unequal length: the case the rule exists for
    assert got == agent.evaluate_device(None, dv, k) == agent.evaluate_device(vec_env=dv, episodes_per_env=k)
    with pytest.raises(ValueError):
        agent.evaluate_device()
    with pytest.raises(ValueError):
        agent.evaluate_device(3, episodes_per_env=3)
    with pytest.raises(ValueError):
        agent.evaluate_device(vec_env=dv, episodes_per_env=0)


def test_evaluate_device_per_env_equals_first_finished_on_equal_lengths():
    from sac.control_envs import PendulumEnv

    N = 16
    agent, dv = make_agent(N, max_steps=5, hidden=(32, 32), batch=16, host_cls=PendulumEnv, action_scale=2.0)
    per_env = agent.evaluate_device(episodes_per_env=2)
    assert per_env == agent.evaluate_device(2 * N) == agent.evaluate_device(2 * N, dv) and per_env < 0.0
    assert dv.t == 10


# ---------------------------------------------------------------- 5. learning
# 16 environments, one gradient step per environment step after a warm-up of 1,000 transitions, blocks of 8 vector
# steps from the loop graph; evaluation: each row's first 4 deterministic episodes of at most 500 steps.
LEARNING = dict(num_envs=16, hidden=[256, 256], precision="fp32", batch=256, capacity=100_000, warming=1000,
                gradient_steps=50_000, graph_steps=8, episodes_per_env=4, alpha=0.2, alpha_lr=3e-4)
# profiles/cartpole_baselines.txt, the host class alone: zero force lasts 40.67 steps, the linear feedback 500.00
# (means of 100 seeded episodes).  The bar is their midpoint, 270.33.
ZERO_FORCE, LINEAR_FEEDBACK = 40.67, 500.00
LEARNING_BAR = (ZERO_FORCE + LINEAR_FEEDBACK) / 2
# The step count is the smallest multiple of 10,000 at which the worst of seeds 1, 2, 3 cleared the bar by a tenth of
# the zero-to-feedback gap (45.93, so 316.27), measured once (profiles/cartpole_learning.txt), with the reacher
# test's hyper-parameters (alpha_0 0.2, every learning rate 3e-4): worst seed 119.53 at 10,000, 120.08 at 20,000,
# 166.45 at 30,000, 265.62 at 40,000, 344.20 at 50,000 (seeds 1, 2, 3: 500.00, 500.00, 344.20).


def learning_run(seed, gradient_steps=None, **hparams):
    import time

    from sac.agent import SAC
    from sac.control_envs import CartPoleEnv
    from sac.device_envs import DeviceVectorEnv

    c = dict(LEARNING, gradient_steps=gradient_steps or LEARNING["gradient_steps"], **hparams)
    t0 = time.perf_counter()
    dv = DeviceVectorEnv(CartPoleEnv, c["num_envs"], device=DEV)
    agent = SAC(dv, _cfg(hidden=c["hidden"], precision=c["precision"], capacity=c["capacity"], batch=c["batch"],
                         warming=c["warming"], seed=seed, alpha=c["alpha"], alpha_lr=c["alpha_lr"]))
    untrained = agent.evaluate_device(episodes_per_env=c["episodes_per_env"], vec_env=dv)
    t1 = time.perf_counter()
    # whole vector steps; the first update is at the warming-th transition: at most c["gradient_steps"] of them
    vec_steps = (c["gradient_steps"] + c["warming"] - 1) // c["num_envs"]
    m = agent.run_device_training_loop(vec_steps * c["num_envs"], seed=seed, graph_steps=c["graph_steps"])
    assert 0.99 * c["gradient_steps"] <= m["gradient_steps"] <= c["gradient_steps"]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    trained = agent.evaluate_device(episodes_per_env=c["episodes_per_env"], vec_env=dv)
    agent.engine.close()
    return dict(untrained=untrained, trained=trained, gradient_steps=m["gradient_steps"],
                env_steps=m["total_env_steps"], episodes=m["total_episodes"], train_s=t2 - t1,
                total_s=time.perf_counter() - t0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_training_passes_the_bar_of_the_scripted_policies(seed):
    """The done column carries a task: with +1 per step and failure as the only signal, the device loop lifts the
    deterministic policy's mean episode length (each row's first 4 episodes) from the zero-force side of the bar
    to the feedback law's side.  A target that ignored done would value every state at 1 / (1 - gamma) and learn
    nothing; rows fail and restart at their own steps inside the graph's blocks throughout.
    profiles/cartpole_learning.txt holds the measured returns per seed and step count."""
    r = learning_run(seed)
    print(f"seed {seed}: untrained {r['untrained']:.2f} trained {r['trained']:.2f} bar {LEARNING_BAR:.2f} "
          f"gradient_steps {r['gradient_steps']} train_wall_s {r['train_s']:.2f} total_s {r['total_s']:.2f}")
    assert 1.0 <= r["untrained"] < LEARNING_BAR < r["trained"] <= 500.0, r


# ---------------------------------------------------------------- 6. replica training
@pytest.mark.parametrize("device_envs,graph_steps", [(True, 0), (True, 4), (False, 0)])
def test_train_replica_on_cartpole(device_envs, graph_steps):
    """sac/train_replicas.py --env cartpole, with and without --device-envs: one rank over RCCL."""
    import socket

    import torch.distributed as dist

    from sac.train_replicas import env_factory, train_replica

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cfg = _cfg(hidden=(32, 32), batch=16, warming=24, capacity=4096, seed=5)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        out = train_replica(cfg, env_factory("cartpole"), num_envs=4, env_steps=1000, every=64, rank=0,
                            device="cuda:0", device_envs=device_envs, graph_steps=graph_steps)
    finally:
        dist.destroy_process_group()
    m, agg = out["metrics"], out["aggregate"]
    # 250 vector steps of 4 environments; the number of episodes depends on how soon the poles fall
    assert m["total_env_steps"] == 1000 and m["gradient_steps"] == 1000 - 23
    assert m["total_episodes"] >= 4 and 1.0 <= m["final_avg_return"] <= 500.0
    assert agg["world"] == 1 and agg["aggregations"] >= 1
