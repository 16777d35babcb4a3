"""Uniform-random warm-up actions (train.random_steps) on the MI355X: the uniform rollout
kernels against a twin that feeds SacEngine.uniform_actions to the step kernel, their independence of the policy,
the action source against `deterministic` and `store`, the cursor form, the loop graph's key, the device loop and
a learning run.  Every comparison of rows, storage and state is bit for bit."""
from functools import partial

import numpy as np
import pytest
import torch

import _control
from _control import DEV, bits, raw, twin_of

pytestmark = pytest.mark.gpu

ENV_STATE = ("obs", "counters", "dstate", "ring")
FIELDS = ("obs", "act", "rew", "next_obs", "done")
FILL = 7.25  # what a word no kernel wrote holds


def make(task, N, layout="records", capacity=700, max_steps=3, **cfg_kw):
    """(agent, its DeviceVectorEnv, a function that makes a twin environment in its state): one environment of
    every class the rollout kernels are compiled for."""
    if task == "point":
        from test_gpu_bootstrap_truncated import point_agent, point_twin

        agent, dv = point_agent(N, "fp32", layout, capacity)
        return agent, dv, point_twin
    name, cls, scale = {"pendulum": ("pendulum", "PendulumEnv", 2.0), "reacher": ("reacher", "ReacherEnv", 1.0),
                        "cartpole": ("cartpole", "CartPoleEnv", 1.0)}[task]
    agent, dv = _control.make_agent(partial(_control.cfg, name), cls, N, max_steps=max_steps, layout=layout,
                                    capacity=capacity, action_scale=scale, **cfg_kw)
    return agent, dv, twin_of


def fresh(rb, dv):
    """The replay allocated and filled with FILL, so that a word outside the rows a step wrote is seen."""
    rb._alloc(dv.obs_dim, dv.act_dim)
    rb.storage.fill_(FILL)
    torch.cuda.synchronize()
    return rb


def snapshot(rb, dv):
    torch.cuda.synchronize()
    out = {name: raw(getattr(dv, name)) for name in ENV_STATE}
    out.update(storage=raw(rb.storage), state=raw(rb.state))
    return out


def same(a, b, what=""):
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad} differ"


def done_word(te, tr, mode):
    te, tr = te.to(torch.float32), tr.to(torch.float32)
    return (torch.maximum(te, tr), te, te + 2 * tr)[mode]


# ---------------------------------------------------------------- 1. the uniform step against a twin
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("task", ["point", "pendulum", "reacher", "cartpole"])
def test_uniform_step_matches_a_twin(task, layout, mode):
    from sac import _engine as E
    from sac.replay_buffer import ReplayBuffer

    N, T, cap = 300, 7, 700  # two workgroups of 256 threads, the second ragged; the ring wraps on the third step
    agent, dv, twin = make(task, N, layout, cap)
    eng, rb = agent.engine, fresh(agent.replay_buffer, dv)
    assert rb.layout == layout and dv.act_dim == (2 if task == "reacher" else 1)
    scale = float(eng.cfg.action_scale)
    assert scale == (2.0 if task == "pendulum" else 1.0)
    eng.set_done_mode(mode)
    eng.set_action_source(E.ACTIONS_UNIFORM)
    assert eng.action_source == E.ACTIONS_UNIFORM
    want_rb = ReplayBuffer(cap, device=DEV, obs_dim=dv.obs_dim, act_dim=dv.act_dim, layout=layout)
    want_rb.storage.fill_(FILL)
    tw = twin(dv)
    gen0 = int(rb.state.cpu()[2])
    ended = np.zeros(2, np.int64)
    for t in range(1, T + 1):
        acts = eng.uniform_actions(N, t)
        assert acts.shape == (N, dv.act_dim) and acts.dtype == np.float32
        assert (acts >= -scale).all() and (acts < scale).all()
        slots = (torch.arange(N, device=DEV) + rb._pos) % cap
        before = tw.obs.clone()
        eng.rollout_step(dv, rb)
        a = torch.from_numpy(acts).to(DEV)
        _, r, te, tr, info = tw.step(a)
        ended += [int(te.sum()), int(tr.sum())]
        rows = dict(obs=before, act=a, rew=r, next_obs=info["final_obs"], done=done_word(te, tr, mode))
        for name in FIELDS:
            dst = getattr(want_rb, name)
            dst[slots] = rows[name].reshape(dst[slots].shape)
        got = rb.act[slots].cpu().numpy()
        assert np.array_equal(bits(got), bits(acts)), t  # the stored actions are the export's, before anything else
    torch.cuda.synchronize()
    assert torch.equal(raw(rb.storage), raw(want_rb.storage))
    assert rb.state.cpu().tolist() == [cap, (T * N) % cap, gen0 + T] and (rb._size, rb._pos) == (cap, (T * N) % cap)
    for name in ENV_STATE:  # the environments and the episode ring
        assert torch.equal(raw(getattr(dv, name)), raw(getattr(tw, name))), name
    assert dv.t == tw.t == T
    assert ended.sum() > 0 and (task == "point" or ended[1] > 0), ended  # episodes ended inside the steps
    if task == "pendulum":
        assert np.abs(rb.act.cpu().numpy()).max() > 1.0  # the policy's scale, 2.0
    if task == "reacher":  # both words of block 0
        act = rb.act.cpu().numpy()
        assert len(np.unique(act)) > N and not np.array_equal(act[:, 0], act[:, 1])
    eng.close()


# ---------------------------------------------------------------- 2. no dependence on the policy
@pytest.mark.parametrize("task", ["pendulum", "reacher"])
def test_uniform_step_reads_nothing_of_the_policy(task):
    from sac import _engine as E

    N, T = 40, 3
    runs, means = [], []
    for poison in (False, True):
        agent, dv, _ = make(task, N)
        eng, rb = agent.engine, fresh(agent.replay_buffer, dv)
        if poison:
            with torch.no_grad():
                for p in agent.policy_net.parameters():
                    p.fill_(float("nan"))
                eng.flat["pi"].fill_(float("nan"))
            eng.sync_params()
        means.append(eng.policy_act(dv.obs.clone()).cpu())
        if poison:  # the policy itself no longer answers what it did
            assert torch.isfinite(means[0]).all() and not torch.equal(means[0], means[1])
        eng.set_action_source(E.ACTIONS_UNIFORM)
        for _ in range(T):
            eng.rollout_step(dv, rb)
        runs.append(snapshot(rb, dv))
        rows = {name: getattr(rb, name)[:T * N].cpu().numpy() for name in FIELDS}
        assert all(np.isfinite(x).all() for x in rows.values())
        eng.close()
    same(runs[0], runs[1], "NaN policy parameters")


# ---------------------------------------------------------------- 3. source, deterministic and store
def test_source_leaves_the_mean_and_store_alone():
    from sac import _engine as E

    N = 40
    agent, dv, twin = make("reacher", N)
    other, dv2, _ = make("reacher", N)
    eng, rb = agent.engine, fresh(agent.replay_buffer, dv)
    eng2, rb2 = other.engine, fresh(other.replay_buffer, dv2)
    # the policy mean, whatever the source
    eng.set_action_source(E.ACTIONS_UNIFORM)
    eng.rollout_step(dv, rb, deterministic=True)
    eng2.rollout_step(dv2, rb2, deterministic=True)
    same(snapshot(rb, dv), snapshot(rb2, dv2), "deterministic under UNIFORM")
    assert not np.array_equal(rb.act[:N].cpu().numpy(), eng.uniform_actions(N, 1))
    # store = False: the environments take the uniform actions, the replay stays
    before = snapshot(rb, dv)
    tw = twin(dv)
    eng.rollout_step(dv, rb, store=False)
    tw.step(torch.from_numpy(eng.uniform_actions(N, 2)).to(DEV))
    after = snapshot(rb, dv)
    assert torch.equal(after["storage"], before["storage"]) and torch.equal(after["state"], before["state"])
    assert (rb._size, rb._pos) == (N, N) and dv.t == 2
    for name in ENV_STATE:
        assert torch.equal(after[name], raw(getattr(tw, name))), name
    assert not torch.equal(after["dstate"], before["dstate"])
    # UNIFORM -> POLICY -> step: a twin that never switched
    for name in ENV_STATE:  # the twin's environments follow the step it did not take
        getattr(dv2, name).copy_(getattr(dv, name))
    dv2.t = dv.t
    assert eng2.action_source == E.ACTIONS_POLICY
    eng.set_action_source(E.ACTIONS_POLICY)
    eng.rollout_step(dv, rb)
    eng2.rollout_step(dv2, rb2)
    same(snapshot(rb, dv), snapshot(rb2, dv2), "POLICY after UNIFORM")
    assert not np.array_equal(rb.act[N:2 * N].cpu().numpy(), eng.uniform_actions(N, 3))
    eng.close()
    eng2.close()


def test_engine_refuses_a_bad_source():
    from sac import _engine as E

    agent, dv, _ = make("pendulum", 5)
    eng = agent.engine
    assert eng.action_source == E.ACTIONS_POLICY
    for bad in (2, -1, True, 1.0, None, "uniform"):
        with pytest.raises(ValueError):
            eng.set_action_source(bad)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="0 .policy. or 1 .uniform."):
            E.ops().engine_set_action_source(eng.handle.value, bad)
    assert eng.action_source == E.ACTIONS_POLICY
    E.ops().engine_set_action_source(eng.handle.value, 0)
    eng.close()


# ---------------------------------------------------------------- 4. the cursor form
@pytest.mark.parametrize("task", ["point", "cartpole"])
def test_cursor_form_matches_the_host_form(task):
    from sac import _engine as E

    N, T, cap = 300, 4, 700
    agent, dv, _ = make(task, N, capacity=cap)
    other, dv2, _ = make(task, N, capacity=cap)
    eng, rb = agent.engine, fresh(agent.replay_buffer, dv)
    eng2, rb2 = other.engine, fresh(other.replay_buffer, dv2)
    eng.set_action_source(E.ACTIONS_UNIFORM)
    eng2.set_action_source(E.ACTIONS_UNIFORM)
    cursor = eng2.new_cursor()
    eng2.seed_cursor(cursor, dv2, rb2)
    for t in range(T):
        eng.rollout_step(dv, rb)
        eng2.rollout_step_dev(dv2, rb2, cursor, t & 1)
        same(snapshot(rb, dv), snapshot(rb2, dv2), f"cursor form, step {t}")
        assert cursor[(t & 1) ^ 1].cpu().tolist() == [min(cap, (t + 1) * N), ((t + 1) * N) % cap, t + 1, 0], t
        assert (rb2._size, rb2._pos, dv2.t) == (rb._size, rb._pos, dv.t)
    assert cursor.cpu().tolist() == [[cap, (T * N) % cap, T, 0], [cap, ((T - 1) * N) % cap, T - 1, 0]]
    # store = 0 advances t only
    eng.rollout_step(dv, rb, store=False)
    eng2.rollout_step_dev(dv2, rb2, cursor, 0, store=False)
    same(snapshot(rb, dv), snapshot(rb2, dv2), "cursor form, store = 0")
    assert cursor[1].cpu().tolist() == [cap, (T * N) % cap, T + 1, 0]
    # a cursor that was never seeded (a slot outside the ring): nothing moves, the other slot included
    unseeded = torch.full((2, 4), -1, dtype=torch.int64, device=DEV)
    before = snapshot(rb2, dv2)
    eng2.rollout_step_dev(dv2, rb2, unseeded, 1)
    same(before, snapshot(rb2, dv2), "unseeded cursor")
    assert unseeded.cpu().tolist() == [[-1] * 4] * 2
    eng.close()
    eng2.close()


# ---------------------------------------------------------------- 5. the graph key
def test_loop_graph_captures_again_for_another_source():
    from sac import _engine as E

    N = 40
    agent, dv, _ = make("pendulum", N, capacity=1000)
    other, dv2, _ = make("pendulum", N, capacity=1000)
    eng, rb = agent.engine, fresh(agent.replay_buffer, dv)
    eng2, rb2 = other.engine, fresh(other.replay_buffer, dv2)
    cursor = eng.loop_cursor()
    eng.seed_cursor(cursor, dv, rb)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)
    eng.set_action_source(E.ACTIONS_UNIFORM)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)  # the same call: another key, another capture
    eng.set_action_source(E.ACTIONS_POLICY)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)
    for source in (0, 0, 1, 1, 0, 0):
        if eng2.action_source != source:
            eng2.set_action_source(source)
        eng2.rollout_step(dv2, rb2)
    same(snapshot(rb, dv), snapshot(rb2, dv2), "loop graph against stepwise")
    act = rb.act[:6 * N].cpu().numpy().reshape(6, N, 1)
    for t in range(6):
        assert np.array_equal(bits(act[t]), bits(eng.uniform_actions(N, t + 1))) == (t in (2, 3)), t
    eng.close()
    eng2.close()


# ---------------------------------------------------------------- 6. the loop
def loop_agent(N, random_steps, n_step=1, bootstrap_truncated=False, **cfg_kw):
    from sac import control_envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    kw = dict(capacity=1000, batch=32, warming=64, action_scale=2.0)
    kw.update(cfg_kw)
    c = _control.cfg("pendulum", **kw)
    c["train"].update(n_step=n_step, bootstrap_truncated=bootstrap_truncated)
    if random_steps is not None:
        c["train"]["random_steps"] = random_steps
    dv = DeviceVectorEnv.from_env(control_envs.PendulumEnv(max_steps=5), N, device=DEV)
    return SAC(dv, c), dv


@pytest.mark.parametrize("n_step,bootstrap_truncated", [(1, False), (3, True)])
def test_device_loop_acts_uniformly_first(n_step, bootstrap_truncated):
    from sac import _engine as E

    N, V = 40, 8
    K = 5 * N // 2  # 2.5 N: the third vector step is uniform, whole
    agent, dv = loop_agent(N, K, n_step, bootstrap_truncated)
    eng = agent.engine
    assert agent.random_steps == K and eng.action_source == E.ACTIONS_POLICY
    switches = []
    orig = eng.set_action_source
    eng.set_action_source = lambda s: (switches.append((dv.t, s)), orig(s))[1]
    m = agent.run_device_training_loop(V * N)
    torch.cuda.synchronize()
    eng.check()
    assert switches == [(0, E.ACTIONS_UNIFORM), (3, E.ACTIONS_POLICY)]  # at the boundaries only
    assert eng.action_source == E.ACTIONS_POLICY
    # row m * N + i is the row (n_step = 1) or the window (n_step = 3) that vector step m opened: its action is
    # that step's draw
    rows = (V - n_step + 1) * N
    assert len(agent.replay_buffer) == rows
    act = agent.replay_buffer.act[:rows].cpu().numpy().reshape(-1, N, 1)
    for v in range(4):
        assert np.array_equal(bits(act[v]), bits(eng.uniform_actions(N, v + 1))) == (v < 3), v
    assert np.isfinite(eng.losses()).all()
    off, _ = loop_agent(N, None, n_step, bootstrap_truncated)
    m0 = off.run_device_training_loop(V * N)
    torch.cuda.synchronize()
    assert (m["total_env_steps"], m["gradient_steps"]) == (m0["total_env_steps"], m0["gradient_steps"])
    assert m["total_env_steps"] == V * N and m["gradient_steps"] > 0 and m["total_episodes"] == m0["total_episodes"]
    assert not np.array_equal(off.replay_buffer.act[:N].cpu().numpy(), act[0])
    off.engine.close()
    eng.close()


def test_device_loop_restores_the_source_after_an_exception():
    from sac import _engine as E

    N = 40
    agent, dv = loop_agent(N, 10 * N)

    class Stop(Exception):
        pass

    def callback(metrics):
        assert agent.engine.action_source == E.ACTIONS_UNIFORM
        if metrics["env_steps"] >= 2 * N:
            raise Stop

    with pytest.raises(Stop):
        agent.run_device_training_loop(8 * N, callback=callback)
    assert agent.engine.action_source == E.ACTIONS_POLICY and dv.t == 2
    # and the C side: the next sampled step is the policy's
    rb = agent.replay_buffer
    agent.engine.rollout_step(dv, rb)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rb.act[N:2 * N].cpu().numpy()), bits(agent.engine.uniform_actions(N, 2)))
    assert not np.array_equal(rb.act[2 * N:3 * N].cpu().numpy(), agent.engine.uniform_actions(N, 3))
    agent.engine.close()


def test_loop_graph_with_random_steps_matches_stepwise():
    """warming = N and batch < N: without random_steps the first block of four would replay the graph.  With K =
    2.5 N it holds uniform steps and runs stepwise; the blocks after it replay the graph."""
    N = 17
    K = 5 * N // 2
    total = 4 * N + 16 * N + 5
    runs = []
    for graph_steps in (0, 4):
        agent, dv = loop_agent(N, K, capacity=300, batch=16, warming=N)
        calls = []
        orig = agent.engine.loop_graph
        agent.engine.loop_graph = lambda *a, **k: (calls.append((dv.t, agent.engine.action_source)), orig(*a, **k))[1]
        m = agent.run_device_training_loop(total, graph_steps=graph_steps, drain_every=8)
        torch.cuda.synchronize()
        agent.engine.check()
        state = dict(agent.engine.state_tensors(), storage=agent.replay_buffer.storage,
                     replay_state=agent.replay_buffer.state, env_obs=dv.obs, env_counters=dv.counters,
                     env_dstate=dv.dstate, env_ring=dv.ring)
        runs.append(dict(metrics=m, state={k: raw(v) for k, v in state.items()}, calls=calls))
        agent.engine.close()
    a, b = runs
    assert a["calls"] == [] and b["calls"][0] == (4, 0) and len(b["calls"]) >= 2, b["calls"]
    assert all(source == 0 for _, source in b["calls"])
    assert a["metrics"] == b["metrics"] and a["metrics"]["gradient_steps"] > 0
    bad = [k for k in a["state"] if not torch.equal(a["state"][k], b["state"][k])]
    assert not bad, f"graph_steps = 4 against stepwise: {bad} differ"
    # the same configuration without random_steps does replay its first block: the rule above is what held it back
    agent, dv = loop_agent(N, None, capacity=300, batch=16, warming=N)
    first = []
    orig = agent.engine.loop_graph
    agent.engine.loop_graph = lambda *a, **k: (first.append(dv.t), orig(*a, **k))[1]
    agent.run_device_training_loop(8 * N, graph_steps=4, drain_every=8)
    torch.cuda.synchronize()
    assert first[0] == 0
    agent.engine.close()


# ---------------------------------------------------------------- 7. learning
def random_steps_learning_run(seed, random_steps, task="pendulum"):
    """tests/test_gpu_pendulum.py's learning run (tests/test_gpu_cartpole.py's for the cart-pole is measured by
    tools/random_steps_learning.py) with train.random_steps."""
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv
    from test_gpu_pendulum import LEARNING, _cfg

    c = LEARNING
    dv = DeviceVectorEnv("pendulum", c["num_envs"], device=DEV)
    cfg = _cfg(hidden=c["hidden"], precision=c["precision"], capacity=c["capacity"], batch=c["batch"],
               warming=c["warming"], seed=seed, action_scale=c["action_scale"])
    cfg["train"]["random_steps"] = random_steps
    agent = SAC(dv, cfg)
    untrained = agent.evaluate_device(c["eval_episodes"], dv)
    vec_steps = (c["gradient_steps"] + c["warming"] - 1) // c["num_envs"]
    m = agent.run_device_training_loop(vec_steps * c["num_envs"], seed=seed, graph_steps=c["graph_steps"])
    torch.cuda.synchronize()
    trained = agent.evaluate_device(c["eval_episodes"], dv)
    agent.engine.close()
    return dict(untrained=untrained, trained=trained, gradient_steps=m["gradient_steps"])


def test_training_with_random_steps_improves_the_evaluation_return():
    """profiles/random_steps_learning.txt has seeds 0..2 with and without the option; this is seed 0 with it."""
    from test_gpu_pendulum import LEARNING, LEARNING_BAR

    r = random_steps_learning_run(0, LEARNING["warming"])
    print(f"random_steps {LEARNING['warming']}: untrained {r['untrained']:.2f} trained {r['trained']:.2f} bar "
          f"{LEARNING_BAR} gradient_steps {r['gradient_steps']}")
    assert 0.99 * LEARNING["gradient_steps"] <= r["gradient_steps"] <= LEARNING["gradient_steps"]
    assert -3255.0 <= r["untrained"] < LEARNING_BAR, r
    assert LEARNING_BAR < r["trained"] <= 0.0, r
