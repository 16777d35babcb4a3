"""Time-limit bootstrapping (train.bootstrap_truncated) on the MI355X: the coded emit kernel
against sac.nstep.nstep_rows(codes=True) on synthetic staging tables, the three done modes of the fused rollout
kernel as twin runs, a stage fed by the rollout kernel's end codes, one gradient step on rows with a fractional
done on every kernel layout, the four training loops with the option on, a learning run on the pendulum, and
replica training.  Every comparison of rows, storage and state is bit for bit."""
import copy
from functools import partial

import numpy as np
import pytest
import torch

import _control
from _control import DEV, bits, raw, twin_of
from test_gpu_nstep import FIELDS, GAMMA, gate, staged_steps

pytestmark = pytest.mark.gpu


def closings(code, n):
    """(k, closing code) of every window of one-step end codes [T][N]."""
    T, N = code.shape
    ks = np.full((T - n + 1, N), n, np.int64)
    cs = np.zeros((T - n + 1, N), np.int64)
    for s in range(T - n + 1):
        for i in range(N):
            for j in range(n):
                if code[s + j, i] != 0:
                    ks[s, i], cs[s, i] = j + 1, int(code[s + j, i])
                    break
    return ks, cs


# ---------------------------------------------------------------- 1. the kernel on synthetic staging
def staged_codes(rng, n, N, O, A, pattern):
    """test_gpu_nstep.staged_steps with end codes in the done column."""
    obs, act, rew, nxt, _ = staged_steps(rng, n, N, O, A, 0)
    if pattern == "random":
        code = np.where(rng.random((n, N)) < 0.25, rng.integers(1, 4, (n, N)), 0).astype(np.float32)
    elif pattern == "flags":
        code = (rng.random((n, N)) < 0.25).astype(np.float32)
    elif pattern == "newest":
        code = np.zeros((n, N), np.float32)
        code[n - 1] = 2.0
    else:
        code = np.full((n, N), float(pattern), np.float32)
    return obs, act, rew, nxt, code


@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("O,A", [(1, 1), (3, 1), (10, 2), (33, 7)])
def test_coded_emit_kernel_matches_nstep_rows(layout, O, A):
    from sac._engine import ops
    from sac.nstep import discount_powers, nstep_rows
    from sac.replay_buffer import ReplayBuffer

    rng = np.random.default_rng(1000 * O + A)
    for N in (1, 37, 130):
        cap = 2 * N + 3  # no multiple of N: the written rows wrap
        rb = ReplayBuffer(cap, device=DEV, obs_dim=O, act_dim=A, layout=layout)
        want_rb = ReplayBuffer(cap, device=DEV, obs_dim=O, act_dim=A, layout=layout)
        for n in (1, 2, 3, 8):
            gpow = discount_powers(GAMMA, n)
            stage = ReplayBuffer(n * N, device=DEV, obs_dim=O, act_dim=A, layout=layout)
            # every rotation of the staging ring, and two positions that are no multiple of N
            cases = [("random", r * N) for r in range(n)] + [("random", n * N - 1), ("random", 5 % (n * N))]
            cases += [(0, 0), (2, (n - 1) * N), (3, 0), ("newest", (n // 2) * N), ("flags", 0)]
            seen_k, seen_c = set(), set()
            for c, (pattern, newest) in enumerate(cases):
                steps = staged_codes(rng, n, N, O, A, pattern)
                want = [x[0] for x in nstep_rows(*steps, gpow, codes=True)]
                if pattern == "random":
                    ks, cs = closings(steps[4], n)
                    seen_k |= set(ks[cs != 0].tolist())
                    seen_c |= set(cs.reshape(-1).tolist())
                elif pattern == 2:  # the oldest row closes every window: k = 1
                    assert (want[4] < 0).all() if n > 1 else (bits(want[4]) == 0).all()
                elif pattern == "newest":  # k = n: the window spans n steps, gamma^n is the right discount
                    assert (bits(want[4]) == 0).all()
                elif pattern == 3:
                    assert (want[4] == 1).all()
                # the row of environment i at window step j (age n - 1 - j) lives in this staging slot
                slot = (newest - (n - 1 - np.arange(n))[:, None] * N + np.arange(N)[None, :]) % (n * N)
                for name, x in zip(FIELDS, steps):
                    host = np.zeros((n * N,) + x.shape[2:], np.float32)
                    host[slot.reshape(-1)] = x.reshape((n * N,) + x.shape[2:])
                    getattr(stage, name).copy_(torch.from_numpy(host))
                size, pos, gen = (cap - 2, cap - max(1, N // 2), 40 + c) if c % 2 else (N // 3, (7 * c) % cap, c)
                dst = torch.from_numpy((pos + np.arange(N)) % cap).to(DEV)
                stage_before = raw(stage.storage)
                what = (layout, O, A, N, n, pattern, newest)

                def emit(op, powers):
                    rb.storage.fill_(7.25)
                    rb.state.copy_(torch.tensor([size, pos, gen]))
                    op(rb.storage, rb.state, rb.layout_spec, stage.storage, stage.state, stage.layout_spec, n, N,
                       newest, powers, size, pos)
                    return raw(rb.storage), rb.state.cpu().tolist()

                want_rb.storage.fill_(7.25)
                for name, x in zip(FIELDS, want):
                    getattr(want_rb, name)[dst] = torch.from_numpy(x).to(DEV)
                got, state = emit(ops().replay_emit_nstep_codes, gpow[:n + 1])
                # the N rows, and everything outside them (other slots, the records' padding) untouched
                assert torch.equal(got, raw(want_rb.storage)), what
                assert state == [min(cap, size + N), (pos + N) % cap, gen + 1], what
                assert torch.equal(raw(stage.storage), stage_before) and stage.state.cpu().tolist() == [0, 0, 0], what
                if pattern in ("flags", 0):  # a table of 0 and 1: exactly the flag kernel's rows
                    flag, flag_state = emit(ops().replay_emit_nstep, gpow[:n])
                    assert torch.equal(got, flag) and state == flag_state, what
                if n == 1:  # the identity on every field but done, -0.0 included
                    assert bits(rb.rew[dst].cpu().numpy())[0] == 0x80000000, what
            if N == 130:
                assert seen_k == set(range(1, n + 1)) and seen_c == {0, 1, 2, 3}, (n, seen_k, seen_c)


def test_coded_emit_op_needs_n_plus_1_powers():
    from sac._engine import ops
    from sac.nstep import discount_powers
    from sac.replay_buffer import ReplayBuffer

    rb = ReplayBuffer(20, device=DEV, obs_dim=3, act_dim=1)
    stage = ReplayBuffer(6, device=DEV, obs_dim=3, act_dim=1)
    with pytest.raises(RuntimeError, match="n \\+ 1"):
        ops().replay_emit_nstep_codes(rb.storage, rb.state, rb.layout_spec, stage.storage, stage.state,
                                      stage.layout_spec, 3, 2, 0, discount_powers(GAMMA, 3)[:3], 0, 0)


# ---------------------------------------------------------------- 2. the rollout kernel's three modes
def cartpole_agent(max_steps, N, precision, layout, capacity):
    return _control.make_agent(partial(_control.cfg, "cartpole"), "CartPoleEnv", N, max_steps=max_steps,
                               precision=precision, layout=layout, capacity=capacity)


def point_agent(N, precision, layout, capacity):
    from test_gpu_device_envs import make_agent

    return make_agent("point_reach", N, precision=precision, layout=layout, capacity=capacity)


def point_twin(dv):
    from sac import envs
    from sac.device_envs import DeviceVectorEnv
    from test_gpu_device_envs import CASES

    tw = DeviceVectorEnv.from_env(envs.OneDPointMassReachEnv(**CASES["point_reach"][1]), dv.num_envs, device=DEV)
    tw.seed, tw.t, tw._reset_done = dv.seed, dv.t, True
    for name in ("obs", "counters", "dstate", "ring"):
        getattr(tw, name).copy_(getattr(dv, name))
    return tw


def mode_runs(make, twin, N, T):
    """T fused steps in each done mode from equal seeds.  Returns the storage without its done column, the done
    column [T][N], the environments' state and the replay state per mode, and the (terminated, truncated) [T][N]
    the step kernel gives a twin environment for the actions mode 0 stored."""
    runs, flags = {}, None
    for mode in (0, 1, 2):
        agent, dv = make()
        eng, rb = agent.engine, agent.replay_buffer
        assert eng.done_mode == 0
        eng.set_done_mode(mode)
        tw = twin(dv) if mode == 0 else None
        te, tr = [], []
        for t in range(T):
            eng.rollout_step(dv, rb)
            if tw is not None:
                _, _, term, trunc, _ = tw.step(rb.act[t * N:(t + 1) * N].clone())
                te.append(term.cpu().numpy())
                tr.append(trunc.cpu().numpy())
        torch.cuda.synchronize()
        if tw is not None:
            flags = (np.stack(te), np.stack(tr))
            for name in ("obs", "counters", "dstate"):
                assert torch.equal(raw(getattr(tw, name)), raw(getattr(dv, name))), name
        # store = False touches nothing, whatever the mode
        before = (raw(rb.storage), rb.state.cpu().tolist(), rb._size, rb._pos)
        snap = {name: getattr(dv, name).clone() for name in ("obs", "counters", "dstate", "ring")}
        t_before = dv.t
        eng.rollout_step(dv, rb, store=False)
        torch.cuda.synchronize()
        assert torch.equal(raw(rb.storage), before[0]) and (rb.state.cpu().tolist(), rb._size, rb._pos) == before[1:]
        for name, x in snap.items():  # back to the state after T steps, which the modes are compared on
            getattr(dv, name).copy_(x)
        dv.t = t_before
        done = rb.done[:T * N].cpu().numpy().reshape(T, N).copy()
        rb.done.zero_()
        runs[mode] = dict(rest=raw(rb.storage), done=done, state=rb.state.cpu().tolist(),
                          envs={name: raw(getattr(dv, name)) for name in ("obs", "counters", "dstate", "ring")})
        eng.close()
    for mode in (1, 2):  # every other word of storage, the environments and the episode ring do not see the mode
        assert torch.equal(runs[mode]["rest"], runs[0]["rest"]), mode
        assert runs[mode]["state"] == runs[0]["state"] == [T * N, T * N, T], mode
        for name, x in runs[0]["envs"].items():
            assert torch.equal(runs[mode]["envs"][name], x), (mode, name)
    te, tr = flags
    assert np.array_equal(runs[0]["done"], (te | tr).astype(np.float32))
    assert np.array_equal(runs[1]["done"], te.astype(np.float32))
    assert np.array_equal(runs[2]["done"], te.astype(np.float32) + 2 * tr.astype(np.float32))
    return runs, te, tr


@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rollout_modes_on_a_cartpole_that_only_fails(precision, layout):
    N, T = 37, 60
    runs, te, tr = mode_runs(lambda: cartpole_agent(500, N, precision, layout, T * N + 7), twin_of, N, T)
    assert te.any() and not tr.any()
    assert np.array_equal(runs[1]["done"], runs[0]["done"])  # no time limit in reach: terminated alone is any end
    assert set(np.unique(runs[2]["done"]).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rollout_modes_on_a_cartpole_the_limit_ends(precision, layout):
    N, T = 37, 21
    runs, te, tr = mode_runs(lambda: cartpole_agent(7, N, precision, layout, T * N + 7), twin_of, N, T)
    limit = tr & ~te
    assert limit.any()
    assert (runs[0]["done"][limit] == 1).all() and (runs[1]["done"][limit] == 0).all()
    assert (runs[2]["done"][limit] == 2).all()


@pytest.mark.parametrize("layout", ["records", "soa"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rollout_modes_on_a_point_mass_that_reaches_its_goal(precision, layout):
    N, T = 37, 28
    runs, te, tr = mode_runs(lambda: point_agent(N, precision, layout, T * N + 7), point_twin, N, T)
    codes = set(np.unique(runs[2]["done"]).tolist())
    print(f"point mass {precision} {layout}: end codes {sorted(codes)}, terminated {int(te.sum())}, truncated "
          f"{int(tr.sum())}, both {int((te & tr).sum())}")
    assert {0.0, 1.0, 2.0} <= codes <= {0.0, 1.0, 2.0, 3.0}  # both flags occur
    assert (3.0 in codes) == bool((te & tr).any())
    both = te & tr
    assert (runs[1]["done"][both] == 1).all() and (runs[0]["done"][both] == 1).all()


def test_engine_refuses_a_bad_mode_and_a_stage_of_the_other_kind():
    from sac import _engine as E
    from sac.nstep import NStepStage

    agent, dv = cartpole_agent(7, 5, "fp32", "records", 100)
    eng = agent.engine
    for bad in (3, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            eng.set_done_mode(bad)
    for bad in (3, -1):
        with pytest.raises(ValueError, match="0 .any end., 1 .terminated. or 2"):
            E.ops().engine_set_done_mode(eng.handle.value, bad)
    assert eng.done_mode == E.DONE_ANY_END
    E.ops().engine_set_done_mode(eng.handle.value, 0)
    coded = NStepStage(3, 5, agent.replay_buffer, GAMMA, bootstrap_truncated=True)
    with pytest.raises(ValueError, match="reads end codes"):
        eng.rollout_step_nstep(dv, coded)
    eng.set_done_mode(E.DONE_END_CODE)
    with pytest.raises(ValueError, match="reads done flags"):
        eng.rollout_step_nstep(dv, NStepStage(3, 5, agent.replay_buffer, GAMMA))
    assert eng.rollout_step_nstep(dv, coded) == 0
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------- 3. a stage fed by the rollout kernel's end codes
def make(task, N, max_steps, n_step=1, option=True, capacity=1000, precision="fp32", seed=3, **cfg_kw):
    """(agent, its DeviceVectorEnv) of N copies of a control task with train.n_step and train.bootstrap_truncated."""
    from sac import control_envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    cls = {"reacher": "ReacherEnv", "cartpole": "CartPoleEnv", "pendulum": "PendulumEnv"}[task]
    c = _control.cfg(task, precision=precision, capacity=capacity, seed=seed, **cfg_kw)
    c["train"]["n_step"] = n_step
    if option is not None:
        c["train"]["bootstrap_truncated"] = option
    dv = DeviceVectorEnv.from_env(getattr(control_envs, cls)(max_steps=max_steps), N, device=DEV)
    return SAC(dv, c), dv


def test_agent_sets_the_engines_mode():
    from sac import _engine as E

    for n_step, option, want in ((1, None, E.DONE_ANY_END), (1, False, E.DONE_ANY_END), (3, False, E.DONE_ANY_END),
                                 (1, True, E.DONE_TERMINATED), (3, True, E.DONE_END_CODE)):
        agent, _ = make("pendulum", 3, 5, n_step=n_step, option=option, action_scale=2.0)
        assert agent.engine.done_mode == want, (n_step, option)
        stage = agent._new_stage(3)
        assert (stage is None) == (n_step == 1) and (stage is None or stage.bootstrap_truncated == bool(option))
        agent.engine.close()


def coded_twin_run(task, N, max_steps, T, n, cap_b=100):
    """Agent A (option off) stores T vector steps of one-step rows in a buffer that does not wrap, and a twin
    environment stepped by the step kernel with A's actions gives terminated and truncated; agent B, of the same
    seed and weights, runs them through a coded stage into a ring of cap_b rows.  Returns B's emitted done values
    and the end codes [T][N] after checking B against nstep_rows(codes=True)."""
    from sac.nstep import discount_powers, end_codes, nstep_rows

    a, dva = make(task, N, max_steps, option=False, capacity=T * N + 7)
    b, dvb = make(task, N, max_steps, n_step=n, option=True, capacity=cap_b)
    for k in ("param/pi", "param/q1"):
        assert torch.equal(raw(a.engine.state_tensors()[k]), raw(b.engine.state_tensors()[k])), k
    tw = twin_of(dva)
    stage = b._new_stage(N)
    assert stage.n == n and stage.bootstrap_truncated and stage.buffer.capacity == n * N
    emitted, te, tr = [], [], []
    for t in range(T):
        a.engine.rollout_step(dva, a.replay_buffer)
        _, _, term, trunc, _ = tw.step(a.replay_buffer.act[t * N:(t + 1) * N].clone())
        te.append(term.cpu().numpy())
        tr.append(trunc.cpu().numpy())
        emitted.append(b.engine.rollout_step_nstep(dvb, stage))
    torch.cuda.synchronize()
    assert emitted == [0] * (n - 1) + [N] * (T - n + 1)
    for name in ("obs", "counters", "dstate", "ring"):
        assert torch.equal(raw(getattr(dva, name)), raw(getattr(dvb, name))), name
    ra, rb = a.replay_buffer, b.replay_buffer
    steps = [getattr(ra, f)[:T * N].cpu().numpy().reshape((T, N) + tuple(getattr(ra, f).shape[1:])) for f in FIELDS]
    code = end_codes(np.stack(te), np.stack(tr))
    assert np.array_equal(steps[4], (code != 0).astype(np.float32))  # A's own rows: any end
    steps[4] = code
    want = [x.reshape((-1,) + x.shape[2:]) for x in nstep_rows(*steps, discount_powers(GAMMA, n), codes=True)]
    M = (T - n + 1) * N
    assert want[2].shape == (M,) and M > cap_b  # B's ring wrapped
    rows = np.arange(M - cap_b, M)  # the emitted rows the ring still holds, at slot r % cap_b
    for f, w in zip(FIELDS, want):
        got = getattr(rb, f).cpu().numpy()
        assert np.array_equal(bits(got[rows % cap_b]), bits(w[rows])), (f, n)
    assert rb.state.cpu().tolist() == [cap_b, M % cap_b, T - n + 1]
    a.engine.close()
    b.engine.close()
    return want[4], code


@pytest.mark.parametrize("n", [3, 5, 8])
def test_coded_stage_on_reacher(n):
    done, code = coded_twin_run("reacher", 37, 5, 20, n)
    assert set(np.unique(code).tolist()) == {0.0, 2.0}  # the reacher never terminates
    assert (done < 0).any() and not (done == 1).any()
    assert (done <= 0).all()
    if n == 8:  # episodes of 5 steps: the limit closes every window early
        assert (done < 0).all()


def test_coded_stage_on_cartpole():
    done, code = coded_twin_run("cartpole", 37, 7, 30, 3)
    assert 2.0 in set(np.unique(code).tolist())
    assert (done < 0).any() and (done == 0).any()


# ---------------------------------------------------------------- 4. one gradient step on fractional done
def mixed_done(cap, n=8):
    """0, 1 and the fractions 1 - gamma^k / gamma^n (k < n) in turn."""
    from sac.nstep import discount_powers

    gpow = discount_powers(GAMMA, n)
    frac = [np.float32(1.0 - gpow[k] / gpow[n]) for k in range(1, n)]
    d = np.zeros(cap, np.float32)
    d[1::3] = 1.0
    d[2::3] = [frac[i % len(frac)] for i in range(len(d[2::3]))]
    return d


@pytest.mark.parametrize("layout", ["pairs", "roles", "rows", "split", "stage"])
def test_gradient_step_reads_a_fractional_done(layout, monkeypatch):
    """y and the post-step parameters of one step against the oracle, with test_gpu_hyper.py's checks and
    tolerances (_check_config_against_oracle, traj_tol 2e-3), on a replay whose done column holds 0, 1 and the
    negative fractions a truncated n-step window stores; the engine trains with gamma^8.  A kernel that read
    done as a flag (d != 0, or a select) instead of computing gamma (1 - d) fails y on every fractional row."""
    import _gpu
    from sac.nstep import discount_powers
    from test_gpu_activations import LAYOUTS
    from test_gpu_parity import _check_config_against_oracle

    assert sorted(LAYOUTS) == ["pairs", "roles", "rows", "split", "stage"]
    shape, lay = LAYOUTS[layout]
    build = _gpu.build_engine

    def build_with_fractions(c, *args, **kw):
        eng, rb, cc = build(c, *args, **kw)
        rb.done.copy_(torch.from_numpy(mixed_done(rb.capacity)))
        torch.cuda.synchronize()
        return eng, rb, cc

    monkeypatch.setattr(_gpu, "build_engine", build_with_fractions)
    kinds = []

    def on_step(k, hp, bt, pi_pre, post_loc, eng):
        d = np.asarray(bt.d)
        kinds.append((int((d == 0).sum()), int((d == 1).sum()), int((d < 0).sum())))
        print(f"[bootstrap_truncated] {layout} step {k}: rows with done 0 / 1 / fractional {kinds[-1]}")
        assert min(kinds[-1]) >= 4 and sum(kinds[-1]) == d.size, kinds[-1]

    c = dict(shape, name=f"{layout}_fractional_done", gamma=discount_powers(GAMMA, 8)[8], done_p=0.3)
    _check_config_against_oracle(c, "fp32", 1, traj_tol=2e-3, layout=lay, expect=layout, on_step=on_step)
    assert len(kinds) == 1


# ---------------------------------------------------------------- 5. the loops
@pytest.mark.parametrize("n", [1, 3])
def test_device_loop_bootstraps_through_the_limit(n):
    N, V, warming = 17, 20, 64
    agent, dv = make("pendulum", N, 5, n_step=n, capacity=1000, batch=32, warming=warming, action_scale=2.0)
    m = agent.run_device_training_loop(V * N)
    torch.cuda.synchronize()
    agent.engine.check()
    assert m["total_env_steps"] == V * N and m["total_episodes"] == (V // 5) * N  # episodes ended
    assert m["gradient_steps"] == gate(V, N, n, 1000, warming)
    rb = agent.replay_buffer
    M = (V - n + 1) * N
    assert len(rb) == M
    done = rb.done[:M].cpu().numpy()
    assert not (done == 1).any()
    if n == 1:
        assert (bits(done) == 0).all()
    else:
        from sac.nstep import discount_powers

        gpow = discount_powers(GAMMA, n)
        fractions = [np.float32(1.0 - gpow[k] / gpow[n]) for k in range(1, n)]
        assert set(bits(done).tolist()) == {0} | set(bits(fractions).tolist())
    assert np.isfinite(agent.engine.losses()).all()
    agent.engine.close()
    # the same run with the option off stores the limit as an end
    off, _ = make("pendulum", N, 5, n_step=n, option=False, capacity=1000, batch=32, warming=warming, action_scale=2.0)
    off.run_device_training_loop(V * N)
    torch.cuda.synchronize()
    assert (off.replay_buffer.done[:M] == 1).any()
    off.engine.close()


def test_loop_graph_with_the_option_matches_stepwise():
    N, warming = 17, 64
    total = 4 * N + 16 * N + 5  # the warm-up ends with the fourth vector step; 16 whole steps and a ragged one follow
    runs = []
    for graph_steps in (0, 4):
        agent, dv = make("pendulum", N, 5, capacity=300, batch=32, warming=warming, action_scale=2.0)
        calls = []
        orig = agent.engine.loop_graph
        agent.engine.loop_graph = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        m = agent.run_device_training_loop(total, graph_steps=graph_steps, drain_every=8)
        torch.cuda.synchronize()
        agent.engine.check()
        state = dict(agent.engine.state_tensors(), storage=agent.replay_buffer.storage,
                     replay_state=agent.replay_buffer.state, env_obs=dv.obs, env_counters=dv.counters,
                     env_dstate=dv.dstate, env_ring=dv.ring)
        runs.append(dict(metrics=m, state={k: raw(v) for k, v in state.items()}, graphs=len(calls),
                         done=agent.replay_buffer.done.cpu().numpy()))
        agent.engine.close()
    a, b = runs
    assert a["graphs"] == 0 and b["graphs"] >= 2
    assert a["metrics"] == b["metrics"] and a["metrics"]["total_episodes"] == 4 * N
    bad = [k for k in a["state"] if not torch.equal(a["state"][k], b["state"][k])]
    assert not bad, f"graph_steps = 4 against stepwise: {bad} differ"
    assert (bits(b["done"]) == 0).all()  # the ring wrapped: every row it holds was stored with the option on


def test_loop_graph_captures_again_for_another_mode():
    """The done mode is part of the loop graph's key: the same call after set_done_mode stores the other word."""
    from sac import _engine as E

    N = 5
    agent, dv = make("pendulum", N, 2, option=False, capacity=100, action_scale=2.0)
    eng, rb = agent.engine, agent.replay_buffer
    cursor = eng.loop_cursor()
    eng.seed_cursor(cursor, dv, rb)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)
    eng.set_done_mode(E.DONE_TERMINATED)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)
    eng.set_done_mode(E.DONE_ANY_END)
    eng.loop_graph(dv, rb, cursor, [0, 0], 1)
    torch.cuda.synchronize()
    done = rb.done[:6 * N].cpu().numpy().reshape(6, N)
    # episodes of two steps: the second step of every block ends by the limit
    assert np.array_equal(done, np.repeat(np.array([0, 1, 0, 0, 0, 1], np.float32)[:, None], N, 1))
    eng.close()


class RecordingEnds:
    """A vector environment that keeps the one-step rows the loop is given to store, with both end flags."""

    def __init__(self, env):
        self.env, self.rows, self._cur = env, [], None

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kw):
        obs, info = self.env.reset(**kw)
        self._cur = obs.copy()
        return obs, info

    def step(self, actions):
        obs, rew, te, tr, info = self.env.step(actions)
        self.rows.append((self._cur, np.array(actions, np.float32), rew.astype(np.float32), info["final_obs"].copy(),
                          np.array(te, bool), np.array(tr, bool)))
        self._cur = obs.copy()
        return obs, rew, te, tr, info


@pytest.mark.parametrize("n", [1, 3])
def test_vectorised_loop_stores_the_coded_rows(n):
    from sac.agent import SAC
    from sac.control_envs import CartPoleEnv
    from sac.nstep import discount_powers, end_codes, nstep_rows
    from sac.vector_env import SyncVectorEnv

    N, V, warming = 4, 30, 24
    c = _control.cfg("cartpole", hidden=(32, 32), batch=16, warming=warming, capacity=4096, seed=5)
    c["train"].update(n_step=n, bootstrap_truncated=True)
    env = RecordingEnds(SyncVectorEnv([partial(CartPoleEnv, max_steps=7)] * N))
    agent = SAC(env, c)
    m = agent.run_vectorized_training_loop(V * N, seed=5)
    torch.cuda.synchronize()
    agent.engine.check()
    assert m["total_env_steps"] == V * N and len(env.rows) == V
    assert m["gradient_steps"] == gate(V, N, n, 4096, warming)
    steps = [np.stack([row[f] for row in env.rows]) for f in range(4)]
    te, tr = (np.stack([row[f] for row in env.rows]) for f in (4, 5))
    assert (tr & ~te).any()  # the limit ended episodes inside the run
    want = nstep_rows(*steps, end_codes(te, tr), discount_powers(GAMMA, n), codes=True)
    M = (V - n + 1) * N
    rb = agent.replay_buffer
    assert len(rb) == M and rb.state.cpu().tolist() == [M, M, V - n + 1]
    for f, w in zip(FIELDS, want):
        got = getattr(rb, f)[:M].cpu().numpy()
        assert np.array_equal(bits(got), bits(w.reshape(got.shape))), f
    done = rb.done[:M].cpu().numpy()
    if n == 1:
        assert np.array_equal(done.reshape(-1, N), te.astype(np.float32))
    else:
        assert (done < 0).any()
    agent.engine.close()


# ---------------------------------------------------------------- 6. learning
# tests/test_gpu_pendulum.py's LEARNING configuration and its own bar (-702.76, measured with the option off:
# profiles/pendulum_learning.txt), stepwise, n_step = 1, option on.  profiles/bootstrap_truncated_learning.txt: seeds
# 0, 1, 2 measured once at 20,000 and 40,000 gradient steps with the option off and on; BT_GRADIENT_STEPS is the
# smallest multiple of 20,000 at which the worst of the three "on" seeds clears the bar.
BT_GRADIENT_STEPS = 20_000


def bt_learning_run(seed, gradient_steps, option=True):
    import time

    from test_gpu_pendulum import LEARNING, _cfg

    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    c = LEARNING
    dv = DeviceVectorEnv("pendulum", c["num_envs"], device=DEV)
    cfg = _cfg(hidden=c["hidden"], precision=c["precision"], capacity=c["capacity"], batch=c["batch"],
               warming=c["warming"], seed=seed, action_scale=c["action_scale"])
    if option:
        cfg["train"]["bootstrap_truncated"] = True
    agent = SAC(dv, cfg)
    untrained = agent.evaluate_device(c["eval_episodes"], dv)
    vec_steps = (gradient_steps + c["warming"] - 1) // c["num_envs"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = agent.run_device_training_loop(vec_steps * c["num_envs"], seed=seed)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    trained = agent.evaluate_device(c["eval_episodes"], dv)
    rb = agent.replay_buffer
    ends = int((rb.done[:len(rb)] == 1).sum().item())
    agent.engine.close()
    return dict(untrained=untrained, trained=trained, gradient_steps=m["gradient_steps"], vec_steps=vec_steps,
                episodes=m["total_episodes"], rows_with_done_1=ends, train_s=train_s)


def test_training_with_the_option_improves_the_evaluation_return():
    """Rows that bootstrap through the time limit train: the stepwise device loop with the option on lifts the
    pendulum's deterministic return over the bar the build without the option set.  Every done the pendulum
    stores comes from the limit, so with the option on no row of the replay says "ended"."""
    from test_gpu_pendulum import LEARNING_BAR

    r = bt_learning_run(0, BT_GRADIENT_STEPS)
    print(f"untrained {r['untrained']:.2f} trained {r['trained']:.2f} bar {LEARNING_BAR} "
          f"gradient_steps {r['gradient_steps']} episodes {r['episodes']} train_wall_s {r['train_s']:.2f}")
    assert 0.99 * BT_GRADIENT_STEPS <= r["gradient_steps"] <= BT_GRADIENT_STEPS
    assert r["episodes"] > 0 and r["rows_with_done_1"] == 0
    assert -3255.0 <= r["untrained"] < LEARNING_BAR, r
    assert LEARNING_BAR < r["trained"] <= 0.0, r


# ---------------------------------------------------------------- 7. replica training
@pytest.mark.parametrize("device_envs", [True, False])
def test_train_replica_with_the_flag(device_envs):
    """sac/train_replicas.py --env pendulum --bootstrap-truncated, with and without --device-envs: one rank."""
    import socket

    import torch.distributed as dist

    from sac.agent import SAC
    from sac.train_replicas import env_factory, train_replica

    made = []

    class Kept(SAC):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cfg = _control.cfg("pendulum", hidden=(32, 32), batch=16, warming=24, capacity=4096, seed=5, action_scale=2.0)
    cfg["train"]["bootstrap_truncated"] = True
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        out = train_replica(copy.deepcopy(cfg), env_factory("pendulum"), num_envs=4, env_steps=1000, every=64, rank=0,
                            device="cuda:0", device_envs=device_envs, agent_cls=Kept)
    finally:
        dist.destroy_process_group()
    m = out["metrics"]
    # 250 vector steps of 4 environments with episodes of 200 steps: one finished per environment, by the limit
    assert m["total_env_steps"] == 1000 and m["total_episodes"] == 4
    assert m["gradient_steps"] == 1000 - 23 and -3255.0 <= m["final_avg_return"] < 0.0
    agent, = made
    assert agent.bootstrap_truncated and len(agent.replay_buffer) == 1000
    assert (bits(agent.replay_buffer.done[:1000].cpu().numpy()) == 0).all()
