"""The device loop cursor and the loop graph without a GPU: the three symbols
are exported with the header's signatures, the ops are registered with Meta
kernels, every argument check of sac_rollout_step_dev / sac_q_values_replay_dev
/ sac_engine_loop_graph returns SAC_E_INVALID with its message before any HIP
call (the dims-dependent ones on a host-only engine, sac_debug_engine_host), the
block planner of run_device_training_loop(graph_steps=K) reproduces the stepwise
loop's own gating, and the loop's precondition errors are raised.

Not reachable without a device: the rowtile_fits refusal (a host-only engine
has no layer table; "no device state" is checked first and is what these tests
reach with otherwise valid arguments)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

INCLUDE = os.path.join(ROOT, "include")
INVALID = -1
PTR = 0x1000  # never dereferenced: every call below is rejected before a launch
SYMBOLS = ("sac_rollout_step_dev", "sac_q_values_replay_dev", "sac_engine_loop_graph")


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_engine_host.restype = ctypes.c_int
    lb.sac_debug_engine_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.POINTER(ctypes.c_void_p)]
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


def _config(E, obs=5, act=1, hidden=(64, 64), batch=16):
    c = E.EngineConfig()
    c.obs_dim, c.act_dim, c.batch = obs, act, batch
    qd, pd = [obs + act, *hidden, 1], [obs, *hidden, 2 * act]
    c.q_layers, c.pi_layers = len(qd) - 1, len(pd) - 1
    for i, d in enumerate(qd):
        c.q_dims[i] = d
    for i, d in enumerate(pd):
        c.pi_dims[i] = d
    c.q_hidden_act = c.pi_hidden_act = 1
    c.gamma, c.tau, c.log_std_min, c.log_std_max, c.action_scale = 0.99, 0.005, -20.0, 2.0, 1.0
    c.actor_lr = c.critic_lr = c.alpha_lr = 3e-4
    c.beta1, c.beta2, c.adam_eps = 0.9, 0.999, 1e-8
    c.auto_entropy, c.target_entropy, c.precision = 1, -float(act), 0
    return c


def _host_engine(lib, **kw):
    from sac import _engine as E

    h = ctypes.c_void_p()
    cfg = _config(E, **kw)
    assert lib.sac_debug_engine_host(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    return h


@pytest.fixture()
def eng(lib):
    """A host-only engine of obs 5 / act 1 / batch 16, the fused rollout step's action width."""
    h = _host_engine(lib)
    yield h
    lib.sac_engine_destroy(h)


@pytest.fixture()
def eng_act3(lib):
    h = _host_engine(lib, act=3)
    yield h
    lib.sac_engine_destroy(h)


def _replay(E, cap=64, obs=5, act=1, stride=8, null=()):
    d = E.ReplayDesc(PTR, PTR, PTR, PTR, PTR, cap, obs, act, PTR, stride)
    for field in null:
        setattr(d, field, None)
    return d


def _envs(E, kind=2, n=17, obs=5, null=()):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, 4
    for field in ("obs", "step", "ep_length", "pos", "ep_return", "episodes"):
        setattr(d, field, None if field in null else PTR)
    d.ring_steps = 8
    return d


def _counts(*g):
    return (ctypes.c_int32 * len(g))(*g)


# ---------------------------------------------------------------- ABI
def test_symbols_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name


C_TYPES = {"sac_engine *": ctypes.c_void_p, "float *": ctypes.c_void_p, "void *": ctypes.c_void_p,
           "int64_t *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p, "int32_t": ctypes.c_int32,
           "const int32_t *": ctypes.POINTER(ctypes.c_int32)}


def test_ctypes_signatures_match_header():
    """Every parameter of the three declarations, in order, against sac._engine.SIGNATURES."""
    from sac import _engine as E

    structs = {"const sac_replay *": ctypes.POINTER(E.ReplayDesc), "const sac_envs *": ctypes.POINTER(E.EnvsDesc)}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "sac_engine.h")).read(), flags=re.S)
    names = {}
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        want, names[name] = [], []
        for p in m.group(1).split(","):
            names[name].append(re.search(r"(\w+)\s*$", p.strip()).group(1))
            ctype = re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", p.strip())).strip()  # drop the parameter name
            want.append(structs.get(ctype) or C_TYPES[ctype])
        res, args = E.SIGNATURES[name]
        assert res is ctypes.c_int and args == want, (name, args, want)
    # the documented parameter lists
    assert names["sac_rollout_step_dev"] == ["e", "envs", "rb", "cursor", "parity", "deterministic", "store", "stream"]
    assert names["sac_q_values_replay_dev"] == ["e", "rb", "cursor", "parity", "n", "use_next_obs", "target", "q_ring",
                                               "q_ring_steps", "stream"]
    assert names["sac_engine_loop_graph"] == ["e", "envs", "rb", "cursor", "k_steps", "grad_steps_host", "q_ring",
                                             "q_ring_steps", "n_replays", "stream"]


def test_ops_registered_with_meta_kernels(lib):
    import torch

    from sac import _engine as E

    ops = E.ops()
    schema = {n: str(getattr(ops, n).default._schema) for n in ("rollout_step_dev", "q_values_replay_dev",
                                                                "loop_graph")}
    for n, s in schema.items():
        assert s.endswith("-> ()"), s
    assert "Tensor(g!) cursor, int parity, bool deterministic=False, bool store=True" in schema["rollout_step_dev"]
    assert "Tensor(e!) storage" in schema["rollout_step_dev"]
    assert "Tensor cursor, int parity, int n" in schema["q_values_replay_dev"]  # the cursor is only read
    assert "Tensor(a!) q_ring" in schema["q_values_replay_dev"]
    assert "Tensor(a!)[] state" in schema["loop_graph"] and "Tensor(h!) cursor, int[] grad_steps, int n_replays" in \
        schema["loop_graph"] and "q_ring=None" in schema["loop_graph"]
    m = dict(device="meta")
    N, O, cap, stride = 40, 5, 100, 16
    obs, counters = torch.empty(N, O, **m), torch.empty(2, N, dtype=torch.int32, **m)
    dstate, ring = torch.empty(2, N, dtype=torch.float64, **m), torch.empty(8, N, 2, dtype=torch.float64, **m)
    storage, rstate = torch.empty(cap * stride, **m), torch.empty(3, dtype=torch.int64, **m)
    layout = [cap, O, 1, stride, 0, 2 * O, 2 * O + 1, O, 2 * O + 2]
    cursor, q_ring = torch.empty(2, 4, dtype=torch.int64, **m), torch.empty(16, N, 2, **m)
    env = (obs, counters, dstate, ring, [2, N, O, 4], [0.0] * 11, 7)
    assert ops.rollout_step_dev(1, *env, storage, rstate, layout, cursor, 1, False, True) is None
    assert ops.q_values_replay_dev(1, storage, rstate, layout, cursor, 0, N, True, False, q_ring) is None
    state = [torch.empty(4, **m) for _ in range(16)]
    assert ops.loop_graph(1, state, *env, storage, rstate, layout, cursor, [1, 0], 3, q_ring) is None
    assert ops.loop_graph(1, state, *env, storage, rstate, layout, cursor, [1, 0], 0) is None
    with pytest.raises(NotImplementedError, match="CPU"):  # CUDA and Meta kernels only: no CPU fallback
        ops.q_values_replay_dev(1, torch.zeros(cap * stride), torch.zeros(3, dtype=torch.int64), layout,
                                torch.zeros(2, 4, dtype=torch.int64), 0, N, True, False, torch.zeros(16, N, 2))


def test_python_entry_points_exist():
    from sac.agent import SAC, GraphBlockPolicy, MAX_RECAPTURES, graph_block_ready, plan_graph_block  # noqa: F401
    from sac.device_envs import DeviceQValueLog
    from sac.engine import SacEngine

    assert list(inspect.signature(SacEngine.rollout_step_dev).parameters) == [
        "self", "envs", "replay", "cursor", "parity", "deterministic", "store"]
    assert list(inspect.signature(SacEngine.loop_graph).parameters) == [
        "self", "envs", "replay", "cursor", "grad_steps", "n_replays", "q_ring"]
    assert list(inspect.signature(plan_graph_block).parameters) == [
        "total_steps", "len_replay", "capacity", "warming_steps", "update_frequency", "gradient_steps", "num_envs",
        "k_steps"]
    assert inspect.signature(SAC.run_device_training_loop).parameters["graph_steps"].default == 0
    assert 1 <= MAX_RECAPTURES <= 16 and hasattr(DeviceQValueLog, "after_graph")


# ---------------------------------------------------------------- sac_rollout_step_dev
def _rollout_dev(lib, e, ev, rb, cursor=PTR, parity=0, deterministic=0, store=1):
    return lib.sac_rollout_step_dev(e, ctypes.byref(ev) if ev is not None else None,
                                    ctypes.byref(rb) if rb is not None else None, cursor, parity, deterministic, store,
                                    None)


def test_rollout_step_dev_rejects_bad_arguments(lib, eng, eng_act3):
    from sac import _engine as E

    ev, rb = _envs(E), _replay(E)
    assert _rollout_dev(lib, eng, None, rb) == INVALID and "null environments" in _err(lib)
    assert _rollout_dev(lib, eng, _envs(E, null=("episodes",)), rb) == INVALID and "episode ring" in _err(lib)
    assert _rollout_dev(lib, eng, ev, None) == INVALID and "null replay" in _err(lib)
    assert _rollout_dev(lib, eng, ev, _replay(E, null=("state",))) == INVALID and "null replay" in _err(lib)
    assert _rollout_dev(lib, eng, ev, _replay(E, cap=16)) == INVALID and "exceeds the replay capacity" in _err(lib)
    assert _rollout_dev(lib, eng, ev, rb, cursor=None) == INVALID and "null cursor" in _err(lib)
    for parity in (-1, 2, 7):
        assert _rollout_dev(lib, eng, ev, rb, parity=parity) == INVALID and "must be 0 or 1" in _err(lib)
    assert _rollout_dev(lib, eng, ev, _replay(E, obs=4)) == INVALID and "replay dims do not match" in _err(lib)
    assert _rollout_dev(lib, eng, _envs(E, obs=4), _replay(E, obs=4)) == INVALID and \
        "engine dims do not match" in _err(lib)
    assert _rollout_dev(lib, None, ev, rb) == INVALID and "null engine" in _err(lib)
    assert _rollout_dev(lib, eng_act3, ev, rb) == INVALID and "engine dims do not match" in _err(lib)


@pytest.mark.parametrize("parity,deterministic,store", [(0, 0, 1), (1, 1, 1), (1, 0, 0)])
def test_rollout_step_dev_valid_arguments_reach_the_launch(lib, eng, parity, deterministic, store):
    from sac import _engine as E

    assert _rollout_dev(lib, eng, _envs(E), _replay(E), PTR, parity, deterministic, store) == INVALID
    assert "rollout_step_dev" in _err(lib) and "no device state" in _err(lib)


# ---------------------------------------------------------------- sac_q_values_replay_dev
def _q_dev(lib, e, rb, cursor=PTR, parity=0, n=17, q_ring=PTR, steps=8, use_next=1, target=0):
    return lib.sac_q_values_replay_dev(e, ctypes.byref(rb) if rb is not None else None, cursor, parity, n, use_next,
                                       target, q_ring, steps, None)


def test_q_values_replay_dev_rejects_bad_arguments(lib, eng, eng_act3):
    from sac import _engine as E

    rb = _replay(E)
    assert _q_dev(lib, eng, None) == INVALID and "null replay" in _err(lib)
    for field in ("obs", "act", "next_obs"):
        assert _q_dev(lib, eng, _replay(E, null=(field,))) == INVALID and "null replay" in _err(lib)
    assert _q_dev(lib, eng, rb, q_ring=None) == INVALID and "null output ring" in _err(lib)
    assert _q_dev(lib, eng, rb, cursor=None) == INVALID and "null cursor" in _err(lib)
    for parity in (-1, 2):
        assert _q_dev(lib, eng, rb, parity=parity) == INVALID and "must be 0 or 1" in _err(lib)
    assert _q_dev(lib, eng, rb, n=0) == INVALID and "n >= 1" in _err(lib)
    for steps in (0, -4):
        assert _q_dev(lib, eng, rb, steps=steps) == INVALID and "q_ring_steps >= 1" in _err(lib)
    assert _q_dev(lib, eng, _replay(E, cap=0)) == INVALID and "capacity >= 1" in _err(lib)
    assert _q_dev(lib, eng, rb, n=65) == INVALID and "exceeds the replay capacity" in _err(lib)
    assert _q_dev(lib, None, rb) == INVALID and "null engine" in _err(lib)
    assert _q_dev(lib, eng_act3, rb) == INVALID and "replay dims do not match the engine" in _err(lib)
    assert _q_dev(lib, eng, _replay(E, stride=4)) == INVALID and "stride below the field width" in _err(lib)


@pytest.mark.parametrize("stride,parity,n,use_next,target", [(8, 0, 17, 1, 0), (0, 1, 64, 0, 1)])
def test_q_values_replay_dev_valid_arguments_reach_the_launch(lib, eng, stride, parity, n, use_next, target):
    from sac import _engine as E

    assert _q_dev(lib, eng, _replay(E, stride=stride), PTR, parity, n, PTR, 8, use_next, target) == INVALID
    assert "no device state" in _err(lib)


# ---------------------------------------------------------------- sac_engine_loop_graph
def _graph(lib, e, ev, rb, cursor=PTR, counts=(1, 0), k=None, q_ring=None, steps=0, n_replays=1, null_counts=False):
    g = _counts(*counts)
    return lib.sac_engine_loop_graph(e, ctypes.byref(ev) if ev is not None else None,
                                     ctypes.byref(rb) if rb is not None else None, cursor,
                                     len(counts) if k is None else k, None if null_counts else g, q_ring, steps,
                                     n_replays, None)


def test_loop_graph_rejects_bad_arguments(lib, eng, eng_act3):
    from sac import _engine as E

    ev, rb = _envs(E), _replay(E)
    assert _graph(lib, eng, None, rb) == INVALID and "null environments" in _err(lib)
    assert _graph(lib, eng, _envs(E, null=("obs",)), rb) == INVALID and "null environment state" in _err(lib)
    assert _graph(lib, eng, _envs(E, null=("episodes",)), rb) == INVALID and "episode ring" in _err(lib)
    assert _graph(lib, eng, ev, None) == INVALID and "null replay" in _err(lib)
    assert _graph(lib, eng, ev, _replay(E, null=("rew",))) == INVALID and "null replay" in _err(lib)
    assert _graph(lib, eng, ev, _replay(E, cap=16)) == INVALID and "exceeds the replay capacity" in _err(lib)
    assert _graph(lib, eng, ev, rb, cursor=None) == INVALID and "null cursor" in _err(lib)
    for counts in ((), (1,), (1, 0, 1), (1,) * 7):
        assert _graph(lib, eng, ev, rb, counts=counts or (0,), k=len(counts)) == INVALID
        assert "must be even and >= 2" in _err(lib), counts
    assert _graph(lib, eng, ev, rb, k=-2) == INVALID and "must be even and >= 2" in _err(lib)
    assert _graph(lib, eng, ev, rb, null_counts=True) == INVALID and "null gradient-step counts" in _err(lib)
    assert _graph(lib, eng, ev, rb, counts=(1, 0, -1, 2)) == INVALID
    assert "negative gradient-step count at vector step 2" in _err(lib)
    assert _graph(lib, eng, ev, rb, n_replays=-1) == INVALID and "n_replays >= 0" in _err(lib)
    for steps in (0, -1):
        assert _graph(lib, eng, ev, rb, q_ring=PTR, steps=steps) == INVALID and "q_ring_steps >= 1" in _err(lib)
    assert _graph(lib, eng, ev, _replay(E, obs=4)) == INVALID and "replay dims do not match" in _err(lib)
    assert _graph(lib, eng, ev, _replay(E, act=3)) == INVALID and "replay dims do not match" in _err(lib)
    assert _graph(lib, eng, _envs(E, obs=4), _replay(E, obs=4)) == INVALID and "engine dims do not match" in _err(lib)
    assert _graph(lib, None, ev, rb) == INVALID and "null engine" in _err(lib)
    assert _graph(lib, eng_act3, ev, rb) == INVALID and "engine dims do not match" in _err(lib)


@pytest.mark.parametrize("counts,q_ring,steps,n_replays", [((1, 0), None, 0, 1), ((0, 0, 0, 0), PTR, 8, 0),
                                                           ((1, 0, 2, 1), PTR, 1, 3)])
def test_loop_graph_valid_arguments_reach_the_launch(lib, eng, counts, q_ring, steps, n_replays):
    """A host-only engine is refused where the first launch would be, capture-only calls included."""
    from sac import _engine as E

    rc = _graph(lib, eng, _envs(E), _replay(E), counts=counts, q_ring=q_ring, steps=steps, n_replays=n_replays)
    assert rc == INVALID and "loop_graph" in _err(lib) and "no device state" in _err(lib)


# ---------------------------------------------------------------- the block planner
CAPACITY, BATCH = 100, 32


def stepwise_counts(total_env_steps, N, capacity, warming, update_frequency, n_grad):
    """run_device_training_loop(graph_steps=0)'s bookkeeping, vector step by vector
    step: (gradient steps run, rows in the buffer before the step) per step."""
    from sac.agent import due_updates_gated

    out, total, length = [], 0, 0
    for _ in range((total_env_steps + N - 1) // N):
        len_before = length
        length = min(capacity, length + N)       # the rollout step stores N rows
        old, total = total, total + N
        due = due_updates_gated(old, total, len_before, capacity, warming, update_frequency, n_grad)
        can_update = length >= warming           # SAC.can_update after the step
        out.append((due if can_update and due else 0, len_before))
    return out


def planned_blocks(total_env_steps, N, K, capacity, warming, update_frequency, n_grad, batch):
    """The loop's graph_steps = K control flow on host integers alone:
    [(kind, first vector step, counts)]."""
    from sac.agent import GraphBlockPolicy, graph_block_ready, plan_graph_block

    vec_steps = (total_env_steps + N - 1) // N
    policy, blocks, done, total, length = GraphBlockPolicy(), [], 0, 0, 0
    while done < vec_steps:
        counts = plan_graph_block(total, length, capacity, warming, update_frequency, n_grad, N, K)
        assert len(counts) == K
        if vec_steps - done >= K and graph_block_ready(counts, length, capacity, warming, batch, N) \
                and policy.admit(counts):
            kind, n = "graph", K
        else:
            kind, n = "stepwise", min(K, vec_steps - done)
        blocks.append((kind, done, counts[:n]))
        done, total, length = done + n, total + n * N, min(capacity, length + n * N)
    return blocks


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("warming", [0, 37, 1000, CAPACITY + 1])
@pytest.mark.parametrize("n_grad", [1, 2])
@pytest.mark.parametrize("update_frequency", [1, 3, 50])
@pytest.mark.parametrize("N", [1, 3, 40])
def test_planner_matches_the_stepwise_gating(N, update_frequency, n_grad, warming, K):
    from sac.agent import MAX_RECAPTURES

    seen_graph = False
    for total_env_steps in (5 * K * N, 5 * K * N + 3 * N + 1, 333):  # the last two are no multiple of K * N
        want = stepwise_counts(total_env_steps, N, CAPACITY, warming, update_frequency, n_grad)
        blocks = planned_blocks(total_env_steps, N, K, CAPACITY, warming, update_frequency, n_grad, BATCH)
        got = [g for _, _, counts in blocks for g in counts]
        assert got == [g for g, _ in want]                       # per vector step
        assert sum(got) == sum(g for g, _ in want)               # the loop's gradient_steps
        if warming > CAPACITY:
            assert sum(got) == 0
        # the blocks tile the run, and a graph block is K whole steps past the warm-up on full batches
        assert [b[1] for b in blocks] == [sum(len(c) for _, _, c in blocks[:i]) for i in range(len(blocks))]
        patterns = []
        for kind, first, counts in blocks:
            if kind != "graph":
                continue
            seen_graph = True
            assert len(counts) == K and first + K <= len(want)
            assert min(CAPACITY, want[first][1] + N) >= warming
            for j, g in enumerate(counts):
                assert not g or min(CAPACITY, want[first + j][1] + N) >= BATCH
            if not patterns or patterns[-1] != counts:
                patterns.append(counts)
        assert len(patterns) <= 1 + MAX_RECAPTURES
        # the tail, the warm-up and the blocks that miss a full batch are stepwise
        for kind, first, counts in blocks:
            if len(counts) < K or min(CAPACITY, want[first][1] + N) < warming:
                assert kind == "stepwise"
    if warming <= 37:
        assert seen_graph  # the grid does exercise the graph path


def test_policy_stops_recapturing():
    from sac.agent import GraphBlockPolicy

    p = GraphBlockPolicy(max_recaptures=2)
    assert p.admit([1, 0]) and p.admit([1, 0])          # capture, replay
    assert p.admit([0, 1]) and p.admit([1, 1])          # two re-captures
    assert not p.admit([1, 0]) and not p.admit([0, 0])  # another pattern: stepwise from now on
    assert p.admit([1, 1])                              # the captured one still replays


# ---------------------------------------------------------------- precondition errors
def _loop_stub(rng_mode="device", ring_steps=16, log_q=False):
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    # what run_device_training_loop reads before its first launch
    env = DeviceVectorEnv.__new__(DeviceVectorEnv)
    env.ring_steps, env.num_envs = ring_steps, 4
    agent = SAC.__new__(SAC)
    agent.env, agent.rng_mode, agent.logger = env, rng_mode, None
    agent.config = {"logger": {"log_q_values": log_q, "log_episode_stats": False}, "train": {}}
    return agent


@pytest.mark.parametrize("K", [1, 3, 7, -2])
def test_loop_rejects_odd_graph_steps(K):
    with pytest.raises(ValueError, match="even number >= 2"):
        _loop_stub().run_device_training_loop(64, graph_steps=K)


def test_loop_rejects_reference_rng_with_graph_steps():
    with pytest.raises(ValueError, match="rng_mode 'reference'"):
        _loop_stub(rng_mode="reference").run_device_training_loop(64, graph_steps=8)


@pytest.mark.parametrize("K,drain_every", [(8, 9), (16, 1), (2, 15)])
def test_loop_rejects_blocks_the_episode_ring_cannot_hold(K, drain_every):
    with pytest.raises(ValueError, match="exceeds the episode ring's 16 steps"):
        _loop_stub(ring_steps=16).run_device_training_loop(64, graph_steps=K, drain_every=drain_every)


def test_loop_rejects_blocks_the_q_ring_cannot_hold():
    from sac.device_envs import DeviceQValueLog

    agent, S = _loop_stub(ring_steps=4 * DeviceQValueLog.RING_STEPS, log_q=True), DeviceQValueLog.RING_STEPS
    with pytest.raises(ValueError, match=f"exceeds the Q-value ring's {S} steps"):
        agent.run_device_training_loop(64, logger=object(), device_q_values=True, graph_steps=30, drain_every=S - 20)
