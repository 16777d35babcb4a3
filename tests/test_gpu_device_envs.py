"""Device-resident probe environments and the fused rollout step on the MI355X.

The yardsticks all predate the device code: the host classes of sac/envs.py
stepped by sac.vector_env.SyncVectorEnv (dynamics, stored transitions, episode
bookkeeping), the sac_policy_act kernel (the fused step's actions) and the
host-tracked ring arithmetic of ReplayBuffer.  Equality rules: observations,
final observations and flags bit for bit; rewards within 1 fp32 ulp of
np.float32(host reward) (numpy 1.x and 2.x promote ``np.float32 - float``
differently; with numpy 2 they are identical except where numpy's scalar
``np.float32 ** 2``, a powf call, misses the correctly rounded square that the
device's fp32 product gives: about 0.07 % of QuadraticActionRewardEnv's
rewards, one ulp each, counted in the assertion message)."""
import collections
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
u64, i32, vp = ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    lb = E.load_library()
    lb.sac_debug_rollout_eps_host.argtypes = [u64, u64, i32, i32, vp]
    lb.sac_debug_env_obs_host.argtypes = [u64, u64, i32, i32, i32, vp]
    return lb


def _cfg(precision="fp32", capacity=4096, warming=24, update_frequency=1, log_episodes=False, seed=3, nets=None):
    """nets: {"q_net": {...}, "policy_net": {...}} entries laid over the ReLU defaults."""
    cfg = {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.2, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [32, 32], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [32, 32], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": 1.0},
        "buffer": {"capacity": capacity},
        "train": {"gradient_steps_per_update": 1, "update_frequency": update_frequency, "seed": seed,
                  "batch_size": 16, "warming_steps": warming, "device": "cuda", "precision": precision,
                  "graph_chunk": 4},
        "logger": {"enabled": False, "env_name": "probe", "agent_name": "SAC", "log_episode_stats": log_episodes,
                   "log_q_values": False, "save_model": {"enabled": False, "path": None}},
    }
    for k, v in (nets or {}).items():
        cfg[k].update(v)
    return cfg


# name -> (sac.envs class name, constructor arguments)
CASES = {
    "constant": ("ConstantRewardEnv", dict(reward=0.3, max_steps=3)),
    "quadratic": ("QuadraticActionRewardEnv", dict(target=0.37, max_steps=2)),
    "random_obs": ("RandomObsBinaryRewardEnv", dict(obs_dim=5, threshold=0.2, max_steps=4)),
    "point_short": ("OneDPointMassReachEnv", dict(max_steps=7, dt=0.5)),
    "point_default": ("OneDPointMassReachEnv", dict()),
    # the fused-step tests choose their own point mass: policy actions in (-1, 1) reach this goal often
    "point_reach": ("OneDPointMassReachEnv", dict(max_steps=7, dt=0.5, action_low=-1.0, action_high=1.0, goal_pos=0.5,
                                                  goal_tolerance=0.2)),
    "point_six": ("OneDPointMassReachEnv", dict(max_steps=6)),
    # random_obs with the nets of NON_RELU_NETS (the fused step's action path off the ReLU branch)
    "random_obs_out_smooth": ("RandomObsBinaryRewardEnv", dict(obs_dim=5, threshold=0.2, max_steps=4)),
    # random_obs with SCALED_NETS' action_scale (the fused step's own tanh(z) * scale)
    "random_obs_scale": ("RandomObsBinaryRewardEnv", dict(obs_dim=5, threshold=0.2, max_steps=4)),
}
# the out_smooth fixture's activations: ELU policy with a tanh output under a log sigma clamp at +-0.5
NON_RELU_NETS = {"random_obs_out_smooth": {
    "q_net": {"hidden_layers_act": "tanh", "output_activation": "elu"},
    "policy_net": {"hidden_layers_act": "elu", "output_activation": "tanh", "log_std_min": -0.5, "log_std_max": 0.5}}}
SCALED_NETS = {"random_obs_scale": {"policy_net": {"action_scale": 2.5}}}


def host_vec(lib, case, N, seed):
    """SyncVectorEnv of the host classes; RandomObsBinaryRewardEnv is subclassed
    so that _obs() returns the device draws' host export (env row i, the vector
    step the SyncVectorEnv is at; which = 3 stepping, 4 resetting)."""
    from sac import envs
    from sac.vector_env import SyncVectorEnv

    cls_name, kw = CASES[case]
    cls = getattr(envs, cls_name)
    if cls_name != "RandomObsBinaryRewardEnv":
        return SyncVectorEnv([lambda: cls(**kw)] * N)

    class HostRandomObs(cls):
        def __init__(self, row):
            super().__init__(**kw)
            self.row, self.t, self.which = row, 0, 4

        def _obs(self):
            out = np.zeros((self.row + 1, self.obs_dim), np.float32)
            assert lib.sac_debug_env_obs_host(seed, self.t, self.which, self.row + 1, self.obs_dim,
                                              out.ctypes.data) == 0
            return out[self.row].copy()

        def step(self, action):
            self.t += 1
            self.which = 3
            return super().step(action)

        def reset(self, seed=None, options=None):
            self.which = 4
            return super().reset(seed=seed)

    return SyncVectorEnv([(lambda i=i: HostRandomObs(i)) for i in range(N)])


def host_rollout(lib, case, N, seed, actions):
    """Step the host envs with actions [T][N][1]; what the vectorised loop would
    store and book: obs (before each step), rewards (float64), final_obs, flags,
    and the finished episodes (return, length) in (t, i) order."""
    vec = host_vec(lib, case, N, seed)
    obs, _ = vec.reset()
    T = actions.shape[0]
    out = dict(obs=[], rew=[], final=[], next=[], term=[], trunc=[], episodes=[])
    ep_ret, ep_len = np.zeros(N, np.float64), np.zeros(N, np.int64)
    for t in range(T):
        nxt, rew, term, trunc, info = vec.step(actions[t])
        out["obs"].append(obs)
        out["rew"].append(rew)
        out["final"].append(info["final_obs"])
        out["next"].append(nxt)
        out["term"].append(term)
        out["trunc"].append(trunc)
        ep_ret += rew
        ep_len += 1
        for i in np.nonzero(term | trunc)[0]:
            out["episodes"].append((float(ep_ret[i]), int(ep_len[i])))
            ep_ret[i], ep_len[i] = 0.0, 0
        obs = nxt
    return {k: (np.stack(v) if k != "episodes" else v) for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_rewards(dev, host64, what):
    """dev fp32 within 1 ulp of np.float32(host reward); the message counts the non-identical ones."""
    want = np.asarray(host64).astype(np.float32)
    dev = np.asarray(dev, np.float32)
    n_diff = int(np.sum(bits(dev) != bits(want)))
    ok = np.abs(dev.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(ok), f"{what}: {int(np.sum(~ok))} rewards beyond 1 ulp, {n_diff} of {dev.size} not identical"
    return n_diff


def scripted_actions(case, N, T, rng):
    """Uniform [-1.5, 1.5] actions (clipping is hit), with rows pinned to the
    edges of each probe's decisions."""
    f32 = np.float32
    a = rng.uniform(-1.5, 1.5, size=(T, N, 1)).astype(np.float32)
    cls_name, kw = CASES[case]
    lo, hi = f32(kw.get("action_low", -1.0 if "Point" not in cls_name else -0.1)), \
        f32(kw.get("action_high", 1.0 if "Point" not in cls_name else 0.1))
    edge = [lo, hi, np.nextafter(lo, f32(0)), np.nextafter(hi, f32(0)), np.nextafter(lo, f32(-9)),
            np.nextafter(hi, f32(9)), f32(0.0), f32(-0.0)]
    if cls_name == "RandomObsBinaryRewardEnv":
        th = f32(kw["threshold"])  # float(th) > 0.2 but float(nextafter(th, 0)) < 0.2: both sides of <=
        edge += [th, -th, np.nextafter(th, f32(0)), -np.nextafter(th, f32(0)), np.nextafter(th, f32(1)),
                 f32(np.float64(kw["threshold"]))]
    for t in range(T):  # the first row walks the edge values; the last row walks them from another offset
        a[t, 0, 0] = edge[t % len(edge)] if t % 2 == 0 else a[t, 0, 0]
        a[t, N - 1, 0] = edge[(t + 3) % len(edge)] if t % 3 == 0 else a[t, N - 1, 0]
    if case == "point_default":
        # rows scripted so that pos lands on goal -/+ tolerance as exactly as fp32 actions allow, the goal is
        # reached (terminated), and it is reached exactly at max_steps (terminated and truncated together)
        step = float(hi)  # the clipped action widened, as the env adds it (dt = 1)
        pos9 = 0.0
        for _ in range(9):
            pos9 += step
        scripts = {
            0: [1.0] * 9 + [f32(0.95 - pos9)] + [1.0] * 50,                    # lands on goal - tol
            1: [1.0] * 9 + [f32((1.05 - step) - pos9)] + [1.0] * 50,           # ... then on goal + tol
            2: [0.0] * 40 + [1.0] * 20,                                        # reaches at step 50 == max_steps
            3: [1.0] * 60,                                                     # reaches at step 10, again and again
            4: [1.0] * 9 + [np.nextafter(f32(0.95 - pos9), f32(1))] + [1.0] * 50,
            5: [1.0] * 9 + [np.nextafter(f32((1.05 - step) - pos9), f32(1))] + [1.0] * 50,
        }
        for row, s in scripts.items():
            if row < N:
                a[:, row, 0] = np.asarray(s[:T], np.float32)
    return a


# ---------------------------------------------------------------- 1. dynamics against the host classes
@pytest.mark.parametrize("N", [1, 17, 33])
@pytest.mark.parametrize("case", ["constant", "quadratic", "random_obs", "point_short", "point_default"])
def test_step_matches_host_classes(lib, case, N):
    from sac import envs
    from sac.device_envs import DeviceVectorEnv

    T, seed = 60, 11
    cls_name, kw = CASES[case]
    actions = scripted_actions(case, N, T, np.random.default_rng(100 + N))
    want = host_rollout(lib, case, N, seed, actions)
    dv = DeviceVectorEnv.from_env(getattr(envs, cls_name)(**kw), N, device=DEV)
    obs0, info = dv.reset(seed=seed)
    assert info == {} and obs0.is_cuda
    acts = torch.from_numpy(actions).to(DEV)
    got = collections.defaultdict(list)
    got["obs"].append(obs0)
    for t in range(T):
        o, r, te, tr, inf = dv.step(acts[t])
        assert all(x.is_cuda for x in (o, r, te, tr, inf["final_obs"])) and te.dtype == torch.bool
        for k, v in (("obs", o), ("rew", r), ("term", te), ("trunc", tr), ("final", inf["final_obs"])):
            got[k].append(v)
    g = {k: torch.stack(v).cpu().numpy() for k, v in got.items()}
    assert np.array_equal(bits(g["obs"][:-1]), bits(want["obs"])), "observations before each step"
    assert np.array_equal(bits(g["obs"][1:]), bits(want["next"])), "observations after autoreset"
    assert np.array_equal(bits(g["final"]), bits(want["final"])), "final_obs"
    assert np.array_equal(g["term"], want["term"]) and np.array_equal(g["trunc"], want["trunc"])
    assert_rewards(g["rew"], want["rew"], case)
    done = want["term"] | want["trunc"]
    assert done.any() and not done.all()
    if case == "point_default" and N >= 17:  # reaching the goal, truncation, and both in one step all occur
        te, tr = want["term"], want["trunc"]
        assert (te & ~tr).any() and (tr & ~te).any() and (te & tr).any()
    if case == "point_short":
        assert want["trunc"].any()
    if case == "random_obs":
        assert len({float(x) for x in want["rew"].ravel()}) == 2  # both sides of the threshold


def test_step_takes_device_tensors_only():
    from sac.device_envs import DeviceVectorEnv

    dv = DeviceVectorEnv("point_mass", 3, device=DEV)
    dv.reset(seed=1)
    with pytest.raises(TypeError):
        dv.step(np.zeros((3, 1), np.float32))


# ---------------------------------------------------------------- agents on device envs
def make_agent(case, N, precision="fp32", layout="records", **cfg_kw):
    from sac import envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv
    from sac.replay_buffer import ReplayBuffer

    cls_name, kw = CASES[case]
    cfg = _cfg(precision=precision, **cfg_kw)
    dv = DeviceVectorEnv.from_env(getattr(envs, cls_name)(**kw), N, device=DEV)
    agent = SAC(dv, cfg)  # _set_seed resets the envs with train.seed
    if layout != "records":
        agent.replay_buffer = ReplayBuffer(cfg["buffer"]["capacity"], device=agent.device, layout=layout)
    return agent, dv


def rows_of(rb, n=None):
    n = len(rb) if n is None else n
    torch.cuda.synchronize()
    return {k: getattr(rb, k)[:n].cpu().numpy().copy() for k in ("obs", "act", "rew", "next_obs", "done")}


def check_stored(lib, case, N, seed, rows, T, what=""):
    """Rows t * N + i of a buffer written by T fused steps against the host envs
    replaying the stored actions; returns the host record."""
    O = rows["obs"].shape[1]
    actions = rows["act"][:T * N].reshape(T, N, 1)
    want = host_rollout(lib, case, N, seed, actions)
    assert np.array_equal(bits(rows["obs"][:T * N]).reshape(T, N, O), bits(want["obs"])), f"{what} obs"
    assert np.array_equal(bits(rows["next_obs"][:T * N]).reshape(T, N, O), bits(want["final"])), f"{what} next_obs"
    assert np.array_equal(rows["done"][:T * N].reshape(T, N), (want["term"] | want["trunc"]).astype(np.float32)), \
        f"{what} done"
    assert_rewards(rows["rew"][:T * N].reshape(T, N), want["rew"], what)
    return want


# ---------------------------------------------------------------- 2. the fused step's actions
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["random_obs", "point_reach", "random_obs_out_smooth", "random_obs_scale"])
def test_fused_actions_match_policy_act(lib, case, precision):
    N, T = 17, 3
    agent, dv = make_agent(case, N, precision, nets=NON_RELU_NETS.get(case) or SCALED_NETS.get(case))
    if case in NON_RELU_NETS:
        assert agent.policy_net.hidden_activations == "elu" and agent.policy_net.output_activation == "tanh"
    assert float(agent.engine.cfg.action_scale) == (2.5 if case in SCALED_NETS else 1.0)
    eng, rb = agent.engine, agent.replay_buffer
    for _ in range(T):
        eng.rollout_step(dv, rb)
    rows = rows_of(rb)
    assert len(rb) == T * N
    seed = int(eng.cfg.seed)
    for t in range(1, T + 1):
        eps = np.zeros((N, 1), np.float32)
        assert lib.sac_debug_rollout_eps_host(seed, t, N, 1, eps.ctypes.data) == 0
        sl = slice((t - 1) * N, t * N)
        want = eng.policy_act(torch.from_numpy(rows["obs"][sl]), torch.from_numpy(eps)).cpu().numpy()
        err = np.abs(rows["act"][sl] - want).max()
        assert err <= 1e-6, (t, err)
    assert len(np.unique(rows["act"])) > N  # not one constant action
    if case in SCALED_NETS:  # the scale shows: |tanh| alone stays below 1
        assert np.abs(rows["act"]).max() > 1.0
    # deterministic: tanh(mu) * scale of the observation the step saw
    before = dv.obs.clone()
    n0 = len(rb)
    eng.rollout_step(dv, rb, deterministic=True)
    got = rows_of(rb)["act"][n0:n0 + N]
    want = eng.policy_act(before).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6


# ---------------------------------------------------------------- 3. stored transitions
@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("case", ["quadratic", "random_obs", "point_reach"])
def test_stored_transitions_match_host_replay(lib, case, layout):
    N, T = 17, 40
    agent, dv = make_agent(case, N, layout=layout, capacity=1024)
    for _ in range(T):
        agent.engine.rollout_step(dv, agent.replay_buffer)
    assert len(agent.replay_buffer) == T * N and agent.replay_buffer.layout == layout
    rows = rows_of(agent.replay_buffer)
    want = check_stored(lib, case, N, dv.seed, rows, T, f"{case}/{layout}")
    done = want["term"] | want["trunc"]
    assert done.any() and not done.all()
    if case == "point_reach":
        assert want["term"].any() and want["trunc"].any()
    torch.cuda.synchronize()
    assert agent.replay_buffer.state.cpu().tolist()[:2] == [T * N, T * N]


# ---------------------------------------------------------------- 4. ring wrap and generation
def test_ring_wrap_and_generation(lib):
    case, N, T, cap = "point_reach", 16, 6, 40
    agent, dv = make_agent(case, N, capacity=cap)
    rb = agent.replay_buffer
    rb._alloc(dv.obs_dim, dv.act_dim)
    torch.cuda.synchronize()
    gen0 = int(rb.state.cpu()[2])
    acts = []
    for t in range(T):
        slots = (torch.arange(N, device=DEV) + rb._pos) % cap
        agent.engine.rollout_step(dv, rb)
        acts.append(rb.act[slots].clone())  # this step's actions, before a later step overwrites them
    torch.cuda.synchronize()
    actions = torch.stack(acts).cpu().numpy().reshape(T, N, 1)
    want = host_rollout(lib, case, N, dv.seed, actions)
    O = dv.obs_dim
    model = dict(obs=np.zeros((cap, O), np.float32), act=np.zeros((cap, 1), np.float32), rew=np.zeros(cap, np.float64),
                 next_obs=np.zeros((cap, O), np.float32), done=np.zeros(cap, np.float32))
    size = pos = 0
    for t in range(T):  # ReplayBuffer's host-tracked ring arithmetic
        for i in range(N):
            s = (pos + i) % cap
            model["obs"][s], model["act"][s], model["rew"][s] = want["obs"][t, i], actions[t, i], want["rew"][t, i]
            model["next_obs"][s] = want["final"][t, i]
            model["done"][s] = float(want["term"][t, i] or want["trunc"][t, i])
        size, pos = min(cap, size + N), (pos + N) % cap
    assert (size, pos) == (40, (6 * 16) % 40)
    rows = rows_of(rb, cap)
    for k in ("obs", "act", "next_obs", "done"):
        assert np.array_equal(bits(rows[k]), bits(model[k])), k
    assert_rewards(rows["rew"], model["rew"], "wrapped ring")
    assert rb.state.cpu().tolist() == [40, (6 * 16) % 40, gen0 + 6]
    assert len(rb) == 40 and (rb._size, rb._pos) == (40, 16)


def test_more_envs_than_capacity_raises():
    from sac import _engine as E

    agent, dv = make_agent("point_reach", 41, capacity=40)
    with pytest.raises(ValueError, match="exceeds the replay capacity"):
        agent.engine.rollout_step(dv, agent.replay_buffer)
    # the op itself refuses too (the C ABI's validation)
    rb = agent.replay_buffer
    rb._alloc(dv.obs_dim, dv.act_dim)
    with pytest.raises(RuntimeError, match="exceeds the replay capacity"):
        E.ops().rollout_step(agent.engine.handle.value, dv.obs, dv.counters, dv.dstate, dv.ring, dv._icfg, dv._params,
                             dv.seed, rb.storage, rb.state, rb.layout_spec, 0, 0, 1, False, True)
    assert len(rb) == 0


# ---------------------------------------------------------------- 5. training reads what the rollout wrote
def test_training_consumes_rollout_rows():
    from sac import envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    N = 32
    dv = DeviceVectorEnv.from_env(envs.ConstantRewardEnv(reward=1.0, max_steps=1), N, device=DEV)
    agent = SAC(dv, _cfg(warming=64, update_frequency=1))
    m = agent.run_device_training_loop(20 * N)
    torch.cuda.synchronize()
    assert m["total_env_steps"] == 20 * N and m["total_episodes"] == 20 * N
    assert agent.engine.steps_done > 0 and agent.engine.steps_done == m["gradient_steps"]
    y = agent.engine.last_targets().cpu().numpy()
    assert y.shape == (16,) and np.all(y == np.float32(1.0)), y  # every done flag set: y == r (sac/envs.py)
    assert m["final_avg_return"] == 1.0 and m["best_avg_return"] == 1.0


# ---------------------------------------------------------------- 6 / 7. loop bookkeeping, no host sync
class RecordingLogger:
    def __init__(self):
        self.episodes, self.hparams = [], []

    def log_episode_metrics(self, episode_idx, reward, length):
        self.episodes.append((episode_idx, reward, length))

    def log_hparams(self, cfg, metrics):
        self.hparams.append(dict(metrics))


@pytest.fixture(scope="module", params=["point_six", "point_reach"])
def loop_run(request):
    """The device loop of test 6 run once under the spies of test 7."""
    from sac.device_envs import EpisodeDrain
    from sac.engine import SacEngine

    case, N, T = request.param, 8, 50
    agent, dv = make_agent(case, N, log_episodes=True)
    logger = RecordingLogger()
    inside, calls = [], []  # names of the two wrapped blocking calls we are inside of; (spied name, inside-of)

    def spy(name, orig):
        def f(*a, **k):
            calls.append((name, inside[-1] if inside else None))
            return orig(*a, **k)
        return f

    def wrap(name, orig):
        def f(*a, **k):
            inside.append(name)
            try:
                return orig(*a, **k)
            finally:
                inside.pop()
        return f

    callbacks = []
    with pytest.MonkeyPatch.context() as mp:
        for name in ("item", "cpu", "numpy"):
            mp.setattr(torch.Tensor, name, spy(name, getattr(torch.Tensor, name)))
        mp.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
        mp.setattr(EpisodeDrain, "finish", wrap("EpisodeDrain.finish", EpisodeDrain.finish))
        mp.setattr(SacEngine, "check", wrap("SacEngine.check", SacEngine.check))
        metrics = agent.run_device_training_loop(N * T, logger=logger, drain_every=7, callback=callbacks.append)
    return dict(case=case, N=N, T=T, agent=agent, dv=dv, logger=logger, metrics=metrics, calls=calls,
                callbacks=callbacks)


def test_loop_bookkeeping_matches_host_loop(lib, loop_run):
    from sac.agent import due_updates_gated

    r = loop_run
    N, T, agent, m = r["N"], r["T"], r["agent"], r["metrics"]
    rows = rows_of(agent.replay_buffer)
    assert len(agent.replay_buffer) == N * T
    want = check_stored(lib, r["case"], N, r["dv"].seed, rows, T, "loop")
    eps = want["episodes"]
    logged = r["logger"].episodes
    assert [e[0] for e in logged] == list(range(len(eps)))          # episode_idx in order
    assert [e[2] for e in logged] == [l for _, l in eps]            # lengths exact, same order
    for (_, ret, _), (w, _) in zip(logged, eps):
        assert ret == pytest.approx(w, rel=1e-6, abs=0)
    assert m["total_episodes"] == len(eps) > 0
    tr = agent.config["train"]
    grad = sum(due_updates_gated(t * N, (t + 1) * N, min(4096, t * N), 4096, tr["warming_steps"],
                                 tr["update_frequency"], tr["gradient_steps_per_update"]) for t in range(T))
    assert m["gradient_steps"] == grad == agent.engine.steps_done > 0
    assert m["total_env_steps"] == N * T
    window, best, avg = collections.deque(maxlen=100), -float("inf"), float("nan")
    for ret, _ in eps:
        window.append(ret)
        avg = float(np.mean(window))
        best = max(best, avg)
    assert m["final_avg_return"] == pytest.approx(avg, rel=1e-6, abs=0)
    assert m["best_avg_return"] == pytest.approx(best, rel=1e-6, abs=0)
    assert r["logger"].hparams == [m]
    # the callback's counters: exact env / gradient steps every vector step, episodes never ahead of the device
    cb = r["callbacks"]
    assert [c["env_steps"] for c in cb] == [N * (t + 1) for t in range(T)]
    assert cb[-1]["gradient_steps"] == grad and all(c["episodes"] <= len(eps) for c in cb)
    if r["case"] == "point_reach":
        assert len({l for _, l in eps}) > 1  # episodes of several lengths: goals reached and truncations


def test_loop_runs_without_host_sync(loop_run):
    outside = [c for c in loop_run["calls"] if c[1] is None]
    assert outside == [], f"host syncs inside the loop: {collections.Counter(n for n, _ in outside)}"
    # whatever the two blocking calls at the end did is attributed to them by name
    assert all(w in ("EpisodeDrain.finish", "SacEngine.check") for _, w in loop_run["calls"])


def test_loop_rejects_q_value_logging_and_host_envs():
    from sac.vector_env import SyncVectorEnv
    from sac import envs

    agent, dv = make_agent("point_six", 4)
    agent.config["logger"]["log_q_values"] = True
    with pytest.raises(ValueError, match="log_q_values"):
        agent.run_device_training_loop(8)
    agent.config["logger"]["log_q_values"] = False
    with pytest.raises(TypeError, match="DeviceVectorEnv"):
        agent.run_device_training_loop(8, vec_env=SyncVectorEnv([envs.OneDPointMassReachEnv] * 2))


# ---------------------------------------------------------------- 8. evaluation
def test_evaluate_device_leaves_replay_untouched():
    from sac import envs

    N = 17
    agent, dv = make_agent("quadratic", N)
    rb = agent.replay_buffer
    for _ in range(3):
        agent.engine.rollout_step(dv, rb)
    torch.cuda.synchronize()
    state0, len0, rows0 = rb.state.cpu().tolist(), len(rb), rows_of(rb)
    got = agent.evaluate_device(20, dv)
    torch.cuda.synchronize()
    assert rb.state.cpu().tolist() == state0 and len(rb) == len0 == 3 * N
    rows1 = rows_of(rb)
    assert all(np.array_equal(bits(rows0[k]), bits(rows1[k])) for k in rows0)
    # host: the deterministic action of the (always zero) observation, through the host class
    a = agent.engine.policy_act(torch.zeros(1, 1, device=DEV)).cpu().numpy()[0]
    env = envs.QuadraticActionRewardEnv(**CASES["quadratic"][1])
    returns = []
    for _ in range(20):
        env.reset()
        ret, done = 0.0, False
        while not done:
            _, rwd, te, tr, _ = env.step(a)
            ret += float(rwd)
            done = te or tr
        returns.append(ret)
    assert got == pytest.approx(float(np.mean(returns)), rel=1e-6, abs=0)
    with pytest.raises(ValueError):
        agent.evaluate_device(0, dv)


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("case", ["random_obs", "point_reach"])
def test_same_seeds_same_buffers(case):
    out = []
    for _ in range(2):
        agent, dv = make_agent(case, 17)
        for _ in range(10):
            agent.engine.rollout_step(dv, agent.replay_buffer)
        out.append((rows_of(agent.replay_buffer), dv.ring.cpu().numpy().copy(), dv.obs.cpu().numpy().copy()))
    (ra, ring_a, obs_a), (rb, ring_b, obs_b) = out
    for k in ra:
        assert np.array_equal(bits(ra[k]), bits(rb[k])), k
    assert np.array_equal(ring_a.view(np.uint64), ring_b.view(np.uint64)) and np.array_equal(bits(obs_a), bits(obs_b))
    # and another env seed draws other observations
    if case == "random_obs":
        agent, dv = make_agent(case, 17, seed=4)
        agent.engine.rollout_step(dv, agent.replay_buffer)
        assert not np.array_equal(rows_of(agent.replay_buffer)["obs"], ra["obs"][:17])
