"""The device loop cursor and the loop graph on the MI355X.

Every comparison is bit for bit: both sides run the same kernels on the same
inputs in the same order (the cursor kernels share their bodies with the
host-argument ones, and eager == graph already holds for train_graph), so there
is no tolerance.  Shapes: N = 40 environments (three row tiles, the last one
ragged with 8 rows: several workgroups read the cursor), a replay ring of 100
(it wraps on the third stored step), batch 32, hidden [64, 64] on a rows-layout
engine; one case at [256, 256], B = 256 (the default hidden-split kernels) and
one in bf16."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N, CAP, BATCH, RING = 40, 100, 32, 16

# name -> (sac.envs class, constructor arguments): all four sac_env_kind values
ENVS = {
    "constant": ("ConstantRewardEnv", dict(reward=0.3, max_steps=3)),
    "quadratic": ("QuadraticActionRewardEnv", dict(target=0.37, max_steps=2)),
    "random_obs": ("RandomObsBinaryRewardEnv", dict(obs_dim=5, threshold=0.2, max_steps=4)),
    "point_reach": ("OneDPointMassReachEnv", dict(max_steps=7, dt=0.5, action_low=-1.0, action_high=1.0, goal_pos=0.5,
                                                  goal_tolerance=0.2)),
}
# name -> (hidden, batch, capacity, layout override, precision, kernel family, host-argument steps run first so
# that the first gradient step finds a full batch)
ENGINES = {
    "rows": ([64, 64], BATCH, CAP, {"layout": "rows"}, "fp32", "rows", 0),
    "split": ([256, 256], 256, 300, None, "fp32", "split", 7),
    "bf16": ([64, 64], BATCH, CAP, {"layout": "rows"}, "bf16", "rows", 0),
}


def raw(t):
    """The bytes of a tensor (NaNs, as in the never-written stats, compare equal to themselves)."""
    return t.detach().contiguous().view(torch.uint8).cpu()


def make_side(env="random_obs", engine="rows", rb_layout="records", n=N):
    """One of two identical twins: engine, device envs and an empty replay ring, all from fixed seeds."""
    from _gpu import assert_layout, build_engine
    from sac import envs
    from sac.device_envs import DeviceVectorEnv
    from sac.replay_buffer import ReplayBuffer

    hidden, batch, cap, layout, precision, family, _ = ENGINES[engine]
    cls, kw = ENVS[env]
    host = getattr(envs, cls)(**kw)
    obs_dim = int(np.prod(host.observation_space.shape))
    rb = ReplayBuffer(cap, device=DEV, obs_dim=obs_dim, act_dim=1, layout=rb_layout)
    eng, rb, _ = build_engine(dict(obs=obs_dim, act=1, hidden=hidden, batch=batch, capacity=cap), precision,
                              device=DEV, layout=layout, replay=rb)
    assert_layout(eng, family)
    dv = DeviceVectorEnv.from_env(host, n, device=DEV, ring_steps=RING)
    dv.reset(seed=5)
    return eng, dv, rb


def state_of(eng, dv, rb):
    """Every device tensor a vector step or a gradient step writes."""
    out = dict(eng.state_tensors(), stats=eng.stats, storage=rb.storage, replay_state=rb.state, env_obs=dv.obs,
               env_counters=dv.counters, env_dstate=dv.dstate, env_ring=dv.ring)
    return {k: raw(v) for k, v in out.items()}


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad} differ"


def mirrors(dv, rb):
    return [rb._size, rb._pos, dv.t, 0]


# ---------------------------------------------------------------- 1. rollout_step_dev == rollout_step
# (deterministic, store) of the 7 steps: sampled, deterministic, not stored (evaluation), and their mixtures
MODES = [(False, True), (False, True), (True, True), (False, False), (False, True), (True, False), (False, True)]


@pytest.mark.parametrize("rb_layout", ["records", "soa"])
@pytest.mark.parametrize("env", sorted(ENVS))
def test_rollout_step_dev_matches_rollout_step(env, rb_layout):
    ea, da, ra = make_side(env, rb_layout=rb_layout)
    eb, db, rb = make_side(env, rb_layout=rb_layout)
    assert ra.layout == rb_layout
    cursor = eb.new_cursor()
    eb.seed_cursor(cursor, db, rb)
    slots, want_slots = [], []
    for j, (deterministic, store) in enumerate(MODES):
        ea.rollout_step(da, ra, deterministic=deterministic, store=store)
        eb.rollout_step_dev(db, rb, cursor, j & 1, deterministic=deterministic, store=store)
        slots.append(cursor[(j & 1) ^ 1].clone())  # the slot this step wrote
        want_slots.append(mirrors(da, ra))
        assert mirrors(db, rb) == mirrors(da, ra)
    torch.cuda.synchronize()
    assert_same(state_of(ea, da, ra), state_of(eb, db, rb), f"{env}/{rb_layout}")
    assert [s.cpu().tolist() for s in slots] == want_slots
    assert want_slots[-1] == [CAP, (5 * N) % CAP, 7, 0]  # five stored steps: the ring wrapped, t counts all seven
    assert ra.state.cpu().tolist()[:2] == [CAP, (5 * N) % CAP]
    assert len(np.unique(ra.act.cpu().numpy())) > N  # not one constant action


def test_unseeded_cursor_is_a_no_op():
    """A slot whose (size, pos) lie outside the ring writes nothing: neither rows, nor state, nor the other slot."""
    eng, dv, rb = make_side()
    cursor = eng.new_cursor()
    cursor[0] = torch.tensor([CAP + 1, CAP, 0, 0], device=DEV)
    cursor[1] = -7
    before = state_of(eng, dv, rb)
    eng.ops.rollout_step_dev(eng.handle.value, dv.obs, dv.counters, dv.dstate, dv.ring, dv._icfg, dv._params, dv.seed,
                             rb.storage, rb.state, rb.layout_spec, cursor, 0, False, True)
    torch.cuda.synchronize()
    assert_same(before, state_of(eng, dv, rb), "no-op")
    assert cursor[1].cpu().tolist() == [-7] * 4


# ---------------------------------------------------------------- 2. graph == stepwise
PATTERN, REPLAYS = [1, 0, 2, 1], 3


def stepwise(eng, dv, rb, pattern, replays, q_ring=None):
    """The loop graph's sequence through the host-argument entry points."""
    for _ in range(replays):
        for g in pattern:
            first = rb._pos
            eng.rollout_step(dv, rb)
            if g:
                eng.train(rb, g)
            if q_ring is not None:
                eng.q_values_replay(rb, first, dv.num_envs, next_obs=True, out=q_ring[dv.t % q_ring.shape[0]])


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_loop_graph_matches_stepwise(engine):
    ea, da, ra = make_side(engine=engine)
    eb, db, rb = make_side(engine=engine)
    for _ in range(ENGINES[engine][6]):
        ea.rollout_step(da, ra)
        eb.rollout_step(db, rb)
    stepwise(ea, da, ra, PATTERN, REPLAYS)
    cursor = eb.new_cursor()
    eb.seed_cursor(cursor, db, rb)
    eb.loop_graph(db, rb, cursor, PATTERN, REPLAYS)
    torch.cuda.synchronize()
    ea.check()
    eb.check()
    assert mirrors(db, rb) == mirrors(da, ra) and eb.steps_done == ea.steps_done == sum(PATTERN) * REPLAYS
    a, b = state_of(ea, da, ra), state_of(eb, db, rb)
    assert {"param/pi", "param/q1", "param/q2", "param/q1t", "param/q2t", "m/pi", "v/q2", "alpha_state", "opt_steps",
            "rng_step", "stats"} <= a.keys()
    assert_same(a, b, engine)
    assert cursor[0].cpu().tolist() == mirrors(da, ra)  # an even K leaves slot 0 ready for the next replay
    assert rb.state.cpu().tolist()[0] == ENGINES[engine][2]  # the ring is full: it wrapped


# ---------------------------------------------------------------- 3. the Q ring
def test_loop_graph_q_ring_matches_stepwise_q_values_replay():
    ea, da, ra = make_side()
    eb, db, rb = make_side()
    qa = torch.zeros(RING, N, 2, device=DEV)
    qb = torch.zeros(RING, N, 2, device=DEV)
    stepwise(ea, da, ra, PATTERN, REPLAYS, q_ring=qa)
    cursor = eb.new_cursor()
    eb.seed_cursor(cursor, db, rb)
    eb.loop_graph(db, rb, cursor, PATTERN, REPLAYS, q_ring=qb)
    torch.cuda.synchronize()
    assert_same(state_of(ea, da, ra), state_of(eb, db, rb), "with the Q ring")
    cells = [t % RING for t in range(1, len(PATTERN) * REPLAYS + 1)]
    for t, c in enumerate(cells, start=1):
        assert torch.equal(raw(qa[c]), raw(qb[c])), f"vector step {t}"
    assert not qb[0].any() and not qb[13:].any()  # 12 steps wrote cells 1 .. 12 and nothing else
    assert len(torch.unique(qb[1:13])) > 12 * N  # values of their own
    # (the third step's rows wrap the ring: slots 80 .. 119 of 100.)  A cell holds the critics' value at its
    # moment: no update ran after the last step, so the final critics reproduce the last cell from the ring rows
    last = (len(cells) - 1) * N % CAP
    assert torch.equal(raw(eb.q_values_replay(rb, last, N)), raw(qb[cells[-1]]))
    # the single launch through its own op, on the slot the last step read
    one = torch.zeros(RING, N, 2, device=DEV)
    eb.ops.q_values_replay_dev(eb.handle.value, rb.storage, rb.state, rb.layout_spec, cursor, 1, N, True, False, one)
    torch.cuda.synchronize()
    assert torch.equal(raw(one[cells[-1]]), raw(qb[cells[-1]])) and int((one != 0).any(-1).any(-1).sum()) == 1


# ---------------------------------------------------------------- 4 / 5. the training loop
def loop_cfg(update_frequency, n_grad, warming, precision="fp32"):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.2, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [64, 64], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [64, 64], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": 1.0},
        "buffer": {"capacity": CAP},
        "train": {"gradient_steps_per_update": n_grad, "update_frequency": update_frequency, "seed": 3,
                  "batch_size": BATCH, "warming_steps": warming, "device": "cuda", "precision": precision,
                  "graph_chunk": 4},
        "logger": {"enabled": False, "env_name": "probe", "agent_name": "SAC", "log_episode_stats": True,
                   "log_q_values": True, "save_model": {"enabled": False, "path": None}},
    }


# name -> (envs, update_frequency, gradient steps per update, warming_steps, total env steps)
LOOPS = {
    # the warm-up ends inside the first block of 8 (100 rows >= 90 after the third step): that block is stepwise,
    # two blocks replay, and 3 * 40 + 7 env steps remain: four more vector steps, stepwise
    "warmup_mid_block": (N, 1, 1, 90, 3 * 8 * N + 3 * N + 7),
    # 24 env steps per block against an update every 5: the pattern changes from block to block, so the graph is
    # captured again MAX_RECAPTURES times and the blocks after that run stepwise unless they repeat a pattern
    "pattern_changes": (3, 5, 2, 37, 12 * 8 * 3 + 10),
}


def loop_agent(name):
    from sac import envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    n, uf, n_grad, warming, _ = LOOPS[name]
    host = getattr(envs, ENVS["point_reach"][0])(**ENVS["point_reach"][1])
    dv = DeviceVectorEnv.from_env(host, n, device=DEV, ring_steps=32)
    return SAC(dv, loop_cfg(uf, n_grad, warming)), dv


class Logger:
    def __init__(self):
        self.episodes, self.q, self.hparams = [], [], []

    def log_episode_metrics(self, episode_idx, reward, length):
        self.episodes.append((episode_idx, reward, length))

    def log_q_values(self, q1, q2, step):
        self.q.append((step, q1, q2))

    def log_hparams(self, cfg, metrics):
        self.hparams.append(dict(metrics))


def run_loop(name, graph_steps, spies=False):
    from sac.device_envs import DeviceQValueLog, EpisodeDrain
    from sac.engine import SacEngine

    agent, dv = loop_agent(name)
    logger, callbacks = Logger(), []
    inside, calls, engine_calls = [], [], collections.Counter()

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

    def count(name, orig):
        def f(*a, **k):
            engine_calls[name] += 1
            return orig(*a, **k)
        return f

    with pytest.MonkeyPatch.context() as mp:
        if spies:  # those of test_loop_runs_without_host_sync (tests/test_gpu_device_envs.py)
            for nm in ("item", "cpu", "numpy"):
                mp.setattr(torch.Tensor, nm, spy(nm, getattr(torch.Tensor, nm)))
            mp.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
            mp.setattr(EpisodeDrain, "finish", wrap("EpisodeDrain.finish", EpisodeDrain.finish))
            mp.setattr(DeviceQValueLog, "finish", wrap("DeviceQValueLog.finish", DeviceQValueLog.finish))
            mp.setattr(SacEngine, "check", wrap("SacEngine.check", SacEngine.check))
            for nm in ("rollout_step", "train", "train_graph", "q_values_replay", "loop_graph", "seed_cursor"):
                mp.setattr(SacEngine, nm, count(nm, getattr(SacEngine, nm)))
        metrics = agent.run_device_training_loop(LOOPS[name][4], logger=logger, drain_every=5,
                                                 callback=lambda c: callbacks.append(dict(c)), device_q_values=True,
                                                 graph_steps=graph_steps)
    torch.cuda.synchronize()
    return dict(agent=agent, dv=dv, logger=logger, metrics=metrics, callbacks=callbacks, calls=calls,
                engine_calls=engine_calls)


@pytest.fixture(scope="module")
def graph_run():
    """The warm-up config through graph_steps = 8, run once under the spies."""
    return run_loop("warmup_mid_block", 8, spies=True)


def assert_same_run(a, b):
    assert a["metrics"] == b["metrics"] and a["logger"].hparams == b["logger"].hparams == [a["metrics"]]
    assert a["logger"].episodes == b["logger"].episodes and len(a["logger"].episodes) > 0
    qa, qb = a["logger"].q, b["logger"].q
    assert [s for s, _, _ in qa] == [s for s, _, _ in qb] == list(range(1, a["metrics"]["total_env_steps"] + 1))
    fa = np.array([(q1, q2) for _, q1, q2 in qa], np.float32).view(np.uint32)
    fb = np.array([(q1, q2) for _, q1, q2 in qb], np.float32).view(np.uint32)
    assert np.array_equal(fa, fb) and len(np.unique(fa)) > 100
    ea, eb = a["agent"].engine, b["agent"].engine
    assert ea.steps_done == eb.steps_done == a["metrics"]["gradient_steps"] > 0
    assert_same(state_of(ea, a["dv"], a["agent"].replay_buffer), state_of(eb, b["dv"], b["agent"].replay_buffer))


def test_training_loop_with_graph_steps_matches_stepwise(graph_run):
    n, _, _, _, total = LOOPS["warmup_mid_block"]
    want = run_loop("warmup_mid_block", 0)
    assert want["metrics"]["total_env_steps"] == 28 * n >= total and total % (8 * n)
    assert_same_run(want, graph_run)
    # the callback runs once per block of 8 (the tail: 4), the stepwise loop's once per vector step
    assert [c["env_steps"] for c in graph_run["callbacks"]] == [8 * n, 16 * n, 24 * n, 28 * n]
    assert [c["gradient_steps"] for c in graph_run["callbacks"]] == \
        [want["callbacks"][i]["gradient_steps"] for i in (7, 15, 23, 27)]
    assert len(want["callbacks"]) == 28


def test_graph_blocks_are_host_free(graph_run):
    """Blocks 2 and 3 are one loop_graph call each: the 12 stepwise vector steps account for every rollout_step,
    q_values_replay and train / train_graph call, and nothing synchronises inside the loop."""
    c = graph_run["engine_calls"]
    assert c["loop_graph"] == 2 and c["seed_cursor"] == 1
    assert c["rollout_step"] == 12 and c["q_values_replay"] == 12
    assert c["train"] + c["train_graph"] == 6 + 4  # steps 3 .. 8 (the warm-up ends at the third) and the tail
    outside = [x for x in graph_run["calls"] if x[1] is None]
    assert outside == [], f"host syncs inside the loop: {collections.Counter(n for n, _ in outside)}"
    assert all(w in ("EpisodeDrain.finish", "DeviceQValueLog.finish", "SacEngine.check") for _, w in graph_run["calls"])


def test_training_loop_with_a_changing_pattern_matches_stepwise():
    from sac.agent import MAX_RECAPTURES

    want, got = run_loop("pattern_changes", 0), run_loop("pattern_changes", 8, spies=True)
    assert_same_run(want, got)
    c = got["engine_calls"]
    # 100 vector steps: 12 whole blocks and a tail of 4.  The first two blocks are the warm-up; the pattern then
    # repeats every 5 blocks, so 1 + MAX_RECAPTURES blocks capture and some later ones run stepwise
    assert 1 + MAX_RECAPTURES <= c["loop_graph"] < 10 and c["rollout_step"] == 100 - 8 * c["loop_graph"]


# ---------------------------------------------------------------- 6. the caches
def test_loop_graph_and_train_graph_keep_separate_caches():
    ea, da, ra = make_side()
    eb, db, rb = make_side()
    cursor = eb.new_cursor()
    eb.seed_cursor(cursor, db, rb)
    eb.loop_graph(db, rb, cursor, PATTERN, 1)
    eb.train_graph(rb, 4, chunk=2)          # captures and replays train_graph's own graph
    eb.loop_graph(db, rb, cursor, PATTERN, 1)  # the loop graph is still there, and slot 0 still holds the mirrors
    eb.train_graph(rb, 2, chunk=2)
    stepwise(ea, da, ra, PATTERN, 1)
    ea.train(ra, 4)
    stepwise(ea, da, ra, PATTERN, 1)
    ea.train(ra, 2)
    torch.cuda.synchronize()
    assert_same(state_of(ea, da, ra), state_of(eb, db, rb), "interleaved with train_graph")

    # another K: captured again
    eb.loop_graph(db, rb, cursor, [2, 0], 2)
    stepwise(ea, da, ra, [2, 0], 2)
    torch.cuda.synchronize()
    assert_same(state_of(ea, da, ra), state_of(eb, db, rb), "K = 2")

    # another replay buffer: captured again (a stale graph would fill the old one and leave this one empty)
    from sac.replay_buffer import ReplayBuffer

    ra2 = ReplayBuffer(CAP, device=DEV, obs_dim=ra.obs_dim, act_dim=1)
    rb2 = ReplayBuffer(CAP, device=DEV, obs_dim=rb.obs_dim, act_dim=1)
    old = raw(rb.storage)
    eb.seed_cursor(cursor, db, rb2)
    eb.loop_graph(db, rb2, cursor, [2, 0], 1)
    stepwise(ea, da, ra2, [2, 0], 1)
    torch.cuda.synchronize()
    assert_same(state_of(ea, da, ra2), state_of(eb, db, rb2), "new replay")
    assert torch.equal(old, raw(rb.storage)) and rb2.state.cpu().tolist()[:2] == [2 * N, 2 * N]


def test_loop_graph_repeats_from_a_snapshot():
    eng, dv, rb = make_side()
    cursor = eng.new_cursor()
    for _ in range(2):  # some history first
        eng.rollout_step(dv, rb)
    eng.train(rb, 3)
    torch.cuda.synchronize()
    snap = eng.snapshot()
    tensors = dict(storage=rb.storage, state=rb.state, obs=dv.obs, counters=dv.counters, dstate=dv.dstate,
                   ring=dv.ring, stats=eng.stats)
    saved = {k: v.clone() for k, v in tensors.items()}
    host = (rb._size, rb._pos, dv.t, eng.steps_done)
    runs = []
    for _ in range(2):
        eng.restore(snap)
        for k, v in tensors.items():
            v.copy_(saved[k])
        rb._size, rb._pos, dv.t, eng.steps_done = host
        eng.seed_cursor(cursor, dv, rb)
        eng.loop_graph(dv, rb, cursor, PATTERN, 2)
        torch.cuda.synchronize()
        runs.append(state_of(eng, dv, rb))
    assert_same(runs[0], runs[1], "repeated from a snapshot")
    assert not torch.equal(runs[0]["param/pi"], raw(snap["param/pi"]))  # it did train
