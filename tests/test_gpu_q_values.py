"""The critic-evaluation kernel (sac_q_values / sac_q_values_replay) and the
device-side Q-value log on the MI355X.

Yardsticks: the critics' torch modules over the engine-owned parameters,
evaluated in float64 on the CPU (metric |q - ref| / max(1, |ref|), bounds those
of test_policy_act_matches_torch: 2e-5 in fp32 mode, 3e-2 in bf16 mode -- the
same forward on the same packed copies; where bf16 arithmetic itself misses
3e-2 on the rows, at 306 inputs, 4 x that arithmetic's error: see bound()); and,
for everything about addressing,
row placement, capture and the device loop, the kernel's own output on the same
rows placed differently: bit for bit."""
import collections

import numpy as np
import pytest
import torch

import _depth
import _widths

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = {"fp32": 2e-5, "bf16": 3e-2}
NETS = ("q1", "q2", "q1t", "q2t")

# name -> (config dict of _gpu.build_engine, layout override, the kernel family phases A / C then run)
SHAPES = {
    # widths that pad (72 -> 96, 40 -> 64), on the role kernels and on a forced stage path
    "pad_roles": (dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                  {"layout": "roles"}, "roles"),
    "pad_stage": (dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                  {"stage_path": 1}, "stage"),
    # obs + act = 34: the concatenation crosses the 32-column pad chunk
    "cross32": (dict(obs=30, act=4, hidden=[64, 64], batch=32, capacity=64), None, None),
    # C2 dims (the hidden-split role kernels)
    "c2": (dict(obs=24, act=4, hidden=[256, 256], batch=256, capacity=512), None, None),
    # a 4-layer critic
    "deep": (dict(obs=11, act=2, q_hidden=[64, 64, 64], pi_hidden=[64, 64], batch=32, capacity=64), None, None),
    # the row-tile LDS layout as plan() builds it for the row tiles and for the pair tiles (2R-row buffers,
    # two different sets of them), at the padded widths and at a 4-layer critic
    "rows_pad": (dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                 {"layout": "rows"}, "rows"),
    "pairs_pad": (dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                  {"layout": "pairs"}, "pairs"),
    "pairs_deep": (dict(obs=11, act=3, hidden=[128, 96, 64], batch=80, capacity=128), {"layout": "pairs"}, "pairs"),
    # the stage path because the shape does not fit the phase kernels (R rows, no pre-activation buffers)
    "stage_obs300": (dict(obs=300, act=6, hidden=[256, 256], batch=64, capacity=128), None, "stage"),
    "stage_512": (dict(obs=24, act=4, hidden=[512, 512], batch=64, capacity=128), None, "stage"),
    "stage_400_300": (dict(obs=17, act=6, hidden=[400, 300], batch=64, capacity=128), None, "stage"),
    # wide actions (the action columns of the critics' input: 17, 32 and 8 of obs + act = 22, 37 and 13), on
    # the engines of test_gpu_forward_layouts.py
    "act17_rows": (dict(obs=5, act=17, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                   {"layout": "rows"}, "rows"),
    "act17_pairs": (dict(obs=5, act=17, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                    {"layout": "pairs"}, "pairs"),
    "act32_roles": (dict(obs=5, act=32, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                    {"layout": "roles"}, "roles"),
    "act8_stage": (dict(obs=5, act=8, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64),
                   {"stage_path": 1}, "stage"),
}
# critics of depth 1 and 5 (tests/_depth.py), with a policy as deep and with one of another depth (q1_pi3,
# q5_pi1: the kernel's LDS layout is sized over all five nets), each on every layout the shape can take
DEPTH_SHAPES = ("h1_roles", "h1_rows", "h1_pairs", "h5_roles", "h5_rows", "h5_pairs", "h5_stage",
                "q1_pi3_roles", "q1_pi3_rows", "q1_pi3_pairs", "q5_pi1_roles", "q5_pi1_rows", "q5_pi1_pairs")
SHAPES.update({k: (dict(_depth.CASES[k][0], capacity=64),) + _depth.CASES[k][1:] for k in DEPTH_SHAPES})
# critics at layer widths off the 8-column grid (tests/_widths.py): [33, 50] on every family, [7, 1] (a hidden layer
# of one unit, a K = 1 output layer), [257, 31] and [401, 299] on the stage path
WIDTH_SHAPES = ("odd_roles", "odd_rows", "odd_pairs", "odd_stage", "tiny_roles", "w257_roles", "w401_stage")
SHAPES.update({k: (dict(_widths.CASES[k][0], capacity=64),) + _widths.CASES[k][1:] for k in WIDTH_SHAPES})
ACTS = {"relu": dict(), "gelu_tanh": dict(q_act="gelu", q_out_act="tanh")}
ROWS = (1, 16, 17, 33)  # one row, a full tile, a ragged tile, three tiles


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def randomise_critics(eng, seed=11, scale=0.1):
    """Independent noise on every critic parameter: target != online, Q1 != Q2."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for k in NETS:
            eng.flat[k].add_((scale * torch.randn(eng.flat[k].numel(), generator=g)).to(eng.device))
    eng.sync_params()


def make_engine(shape, acts, precision, **over):
    from _gpu import assert_layout, build_engine

    c, layout, family = SHAPES[shape]
    eng, rb, c = build_engine(dict(c, **ACTS[acts], **over), precision, device=DEV, layout=layout)
    if family is not None:
        assert_layout(eng, family)
    randomise_critics(eng)
    return eng, rb, c


_engines = {}


def shared_engine(shape, acts, precision):
    """Engines of the read-only tests, built once (no test that takes one trains or edits it)."""
    key = (shape, acts, precision)
    if key not in _engines:
        _engines[key] = make_engine(*key)
    return _engines[key]


def rows_for(c, n, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, c["obs"], generator=g).to(DEV), (2 * torch.rand(n, c["act"], generator=g) - 1).to(DEV)


def ref64(eng, key, s, a, bf16=False):
    """The critic `key` over the engine's current parameters, in float64 on the CPU
    (bf16: with the weights and every layer's inputs rounded to bf16 first)."""
    from sac.models import QNetwork

    net = eng.nets[key]
    hidden = [lin.out_features for lin in net.linears()[:-1]]
    ref = QNetwork(net.obs_size, net.action_size, hidden, net.hidden_activations, net.output_activation).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    s, a = s.detach().cpu().double(), a.detach().cpu().double()
    with torch.no_grad():
        if not bf16:
            return ref(s, a).numpy()
        rnd = lambda t: t.float().bfloat16().double()  # noqa: E731
        x = torch.cat((s, a), dim=-1)
        for m in ref.net:
            x = torch.nn.functional.linear(rnd(x), rnd(m.weight), m.bias) if isinstance(m, torch.nn.Linear) else m(x)
        return x.squeeze(-1).numpy()


def rel_err(q, eng, s, a, target):
    """max over rows and both critics of |q - ref| / max(1, |ref|); also the references."""
    q = q.detach().cpu().numpy().astype(np.float64)
    refs = np.stack([ref64(eng, ("q1t", "q2t")[i] if target else ("q1", "q2")[i], s, a) for i in range(2)], axis=1)
    return float(np.max(np.abs(q - refs) / np.maximum(1.0, np.abs(refs)))), refs


def bound(eng, s, a, target, refs, precision):
    """The project's bound wherever the arithmetic of the precision can meet it.  In bf16 mode
    at 306 inputs the float64 forward with bf16-rounded weights and layer inputs is itself up to
    4.2e-2 from float64 on these rows (the kernel's error agrees with it to three digits): where
    that arithmetic misses the bound, the bound is 4 x the arithmetic's error.  Nothing of the
    kernel's output enters; every shape below 300 inputs keeps 3e-2 (their arithmetic: <= 2e-2)."""
    tol = TOL[precision]
    if precision != "bf16":
        return tol
    rounded = np.stack([ref64(eng, ("q1t", "q2t")[i] if target else ("q1", "q2")[i], s, a, bf16=True)
                        for i in range(2)], axis=1)
    arith = float(np.max(np.abs(rounded - refs) / np.maximum(1.0, np.abs(refs))))
    if arith > tol:
        print(f"  bf16 arithmetic on these rows: {arith:.3e} from float64 -> bound {4 * arith:.3e}")
    return tol if arith <= tol else 4.0 * arith


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("acts", sorted(ACTS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_q_values_match_float64(shape, acts, precision):
    eng, _, c = shared_engine(shape, acts, precision)
    worst = 0.0
    for target in (False, True):
        for n in ROWS:
            s, a = rows_for(c, n, seed=n)
            q = eng.q_values(s, a, target=target)
            assert tuple(q.shape) == (n, 2) and q.dtype == torch.float32
            err, refs = rel_err(q, eng, s, a, target)
            worst = max(worst, err)
            print(f"q_values {shape} {acts} {precision} target={int(target)} n={n}: err {err:.3e}")
            assert err <= bound(eng, s, a, target, refs, precision), (target, n, err)
            if acts == "gelu_tanh":
                assert np.all(np.abs(refs) < 1.0)  # the output activation is applied
    # the four critics are four different functions: a wrong net index would not pass the bound above
    s, a = rows_for(c, 33, seed=5)
    r = [ref64(eng, k, s, a) for k in NETS]
    gap = min(float(np.max(np.abs(r[i] - r[j]))) for i in range(4) for j in range(i))
    assert gap > 2 * TOL[precision], gap
    print(f"q_values {shape} {acts} {precision}: worst {worst:.3e}, smallest gap between critics {gap:.3e}")


# ---------------------------------------------------------------- 2. row independence
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,acts", [("pad_roles", "gelu_tanh"), ("c2", "relu"), ("deep", "relu"),
                                        ("rows_pad", "relu"), ("pairs_deep", "relu"), ("stage_512", "relu"),
                                        ("h1_pairs", "relu"), ("h5_stage", "gelu_tanh"), ("q5_pi1_rows", "relu"),
                                        ("q1_pi3_roles", "gelu_tanh")])
def test_rows_do_not_depend_on_their_tile(shape, acts, precision):
    eng, _, c = shared_engine(shape, acts, precision)
    n = 33
    s, a = rows_for(c, n, seed=2)
    for target in (False, True):
        full = bits(eng.q_values(s, a, target=target))
        fs, fa = rows_for(c, 16, seed=9)  # other rows around the one under test
        for i in (0, 1, 15, 16, 17, 31, 32):
            alone = bits(eng.q_values(s[i:i + 1], a[i:i + 1], target=target))
            assert np.array_equal(alone[0], full[i]), (target, i)
            fs[15], fa[15] = s[i], a[i]
            last = bits(eng.q_values(fs, fa, target=target))
            assert np.array_equal(last[15], full[i]), (target, i)
        # and a prefix of the rows gives a prefix of the values (ragged last tile)
        assert np.array_equal(bits(eng.q_values(s[:17], a[:17], target=target)), full[:17])


# ---------------------------------------------------------------- 3. freshness
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["pad_roles", "pad_stage", "c2", "rows_pad", "pairs_pad", "stage_512",
                                   "h1_roles", "h1_rows", "h1_pairs"])
def test_q_values_read_the_updated_copies(shape, precision):
    """Large steps (critic_lr 3e-2, tau 0.5) so that two gradient steps move
    online and target values by more than the bound."""
    eng, rb, c = make_engine(shape, "relu", precision, critic_lr=3e-2, tau=0.5)
    s, a = rows_for(c, 33, seed=4)
    tol = TOL[precision]
    before = {t: eng.q_values(s, a, target=t).clone() for t in (False, True)}
    eng.train(rb, 2)
    for t in (False, True):
        q = eng.q_values(s, a, target=t)
        err, _ = rel_err(q, eng, s, a, t)
        stale, _ = rel_err(before[t], eng, s, a, t)
        print(f"freshness {shape} {precision} target={int(t)}: err {err:.3e}, pre-step values {stale:.3e}")
        assert err <= tol, (t, err)
        assert not np.array_equal(bits(q), bits(before[t]))
        assert stale > 2 * tol, (t, stale)  # the pre-step values would not pass
    eng.check()
    # a host-side edit of the parameters, then sync_params
    with torch.no_grad():
        eng.flat["q1"].mul_(1.5)
        eng.flat["q2"].mul_(0.5)
        eng.flat["q1t"].mul_(-1.0)
        eng.flat["q2t"].mul_(2.0)
    mid = {t: eng.q_values(s, a, target=t).clone() for t in (False, True)}
    eng.sync_params()
    for t in (False, True):
        q = eng.q_values(s, a, target=t)
        err, _ = rel_err(q, eng, s, a, t)
        stale, _ = rel_err(mid[t], eng, s, a, t)
        assert err <= tol, (t, err)
        assert stale > 2 * tol, (t, stale)  # before sync_params the kernel still read the old packed weights


# ---------------------------------------------------------------- 4. addressing
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replay_addressing_matches_dense_rows(precision):
    from sac.replay_buffer import ReplayBuffer

    eng, _, c = shared_engine("pad_roles", "gelu_tanh", precision)
    O, A, cap, n, first = c["obs"], c["act"], 12, 5, 10
    rng = np.random.default_rng(1)
    cols = (rng.standard_normal((cap, O), dtype=np.float32), rng.uniform(-1, 1, (cap, A)).astype(np.float32),
            rng.standard_normal(cap, dtype=np.float32), rng.standard_normal((cap, O), dtype=np.float32),
            np.zeros(cap, np.float32))
    bufs = {}
    for layout in ("records", "soa"):
        rb = ReplayBuffer(cap, device=DEV, obs_dim=O, act_dim=A, layout=layout)
        rb.push_batch(*cols)
        bufs[layout] = rb
    assert bufs["records"].row_stride > 0 and bufs["soa"].row_stride == 0
    slots = torch.tensor([(first + i) % cap for i in range(n)], device=DEV)
    assert slots.tolist() == [10, 11, 0, 1, 2]  # the slots wrap
    for next_obs in (True, False):
        for target in (False, True):
            got = {k: bits(eng.q_values_replay(rb, first, n, next_obs=next_obs, target=target))
                   for k, rb in bufs.items()}
            rb = bufs["records"]
            dense = bits(eng.q_values((rb.next_obs if next_obs else rb.obs)[slots], rb.act[slots], target=target))
            assert np.array_equal(got["records"], got["soa"]), (next_obs, target)
            assert np.array_equal(got["records"], dense), (next_obs, target)
    # s' and s are different rows: the flag is honoured
    assert not np.array_equal(bits(eng.q_values_replay(bufs["soa"], first, n, next_obs=True)),
                              bits(eng.q_values_replay(bufs["soa"], first, n, next_obs=False)))
    # the whole ring from its last slot, and out= (the C ABI through ctypes) against the op
    rb = bufs["records"]
    order = torch.tensor([(cap - 1 + i) % cap for i in range(cap)], device=DEV)
    out = torch.full((cap, 2), float("nan"), device=DEV)
    assert eng.q_values_replay(rb, cap - 1, cap, out=out) is out
    assert np.array_equal(bits(out), bits(eng.q_values(rb.next_obs[order], rb.act[order])))
    assert np.array_equal(bits(out), bits(eng.q_values_replay(rb, cap - 1, cap)))
    with pytest.raises(ValueError):
        eng.q_values_replay(rb, cap, 1)
    with pytest.raises(ValueError):
        eng.q_values_replay(rb, 0, cap + 1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_strided_column_views_are_read_in_place(precision):
    from sac.replay_buffer import ReplayBuffer

    eng, _, c = shared_engine("pad_roles", "gelu_tanh", precision)
    O, A, n = c["obs"], c["act"], 33
    rb = ReplayBuffer(64, device=DEV, obs_dim=O, act_dim=A)
    rng = np.random.default_rng(2)
    rb.push_batch(rng.standard_normal((n, O), dtype=np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
                  np.zeros(n, np.float32), rng.standard_normal((n, O), dtype=np.float32), np.zeros(n, np.float32))
    s, a = rb.next_obs[:n], rb.act[:n]  # column views of the records table
    assert s.stride(0) == rb.row_stride > O and not s.is_contiguous() and not a.is_contiguous()
    want = bits(eng.ops.q_values(eng.handle.value, s.contiguous(), a.contiguous(), False))
    assert np.array_equal(bits(eng.ops.q_values(eng.handle.value, s, a, False)), want)
    assert np.array_equal(bits(eng.q_values(s, a)), want)
    out = torch.empty(n, 2, device=DEV)
    eng.q_values(s, a, out=out)
    assert np.array_equal(bits(out), want)
    # the op refuses what it cannot address
    with pytest.raises(RuntimeError, match="unit inner stride"):
        eng.ops.q_values(eng.handle.value, rb.records[:n, 0:2 * O:2], a, False)
    with pytest.raises(RuntimeError, match="float32"):
        eng.ops.q_values(eng.handle.value, s.double(), a, False)
    with pytest.raises(RuntimeError, match="same number of rows"):
        eng.ops.q_values(eng.handle.value, s, a[:5], False)
    with pytest.raises(ValueError):
        eng.q_values(s[:, :O - 1], a)


def test_agent_q_values_takes_host_arrays():
    agent, _ = loop_agent(warming=10 ** 6)
    eng = agent.engine
    rng = np.random.default_rng(3)
    s, a = rng.standard_normal((17, 1)).astype(np.float32), rng.uniform(-1, 1, (17, 1)).astype(np.float32)
    for target in (False, True):
        q1, q2 = agent.q_values(s, a, target=target)
        assert q1.dtype == q2.dtype == np.float32 and q1.shape == q2.shape == (17,)
        want = bits(eng.q_values(torch.from_numpy(s).to(DEV), torch.from_numpy(a).to(DEV), target=target))
        assert np.array_equal(bits(q1), want[:, 0]) and np.array_equal(bits(q2), want[:, 1])
        t1, t2 = agent.q_values(torch.from_numpy(s).to(DEV), torch.from_numpy(a), target=target)
        assert np.array_equal(bits(t1), want[:, 0]) and np.array_equal(bits(t2), want[:, 1])


# ---------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_q_values_capture_under_torch_cuda_graph(precision):
    """One stream, one kernel node per op: no parallel branches."""
    from sac.replay_buffer import ReplayBuffer

    eng, _, c = shared_engine("pad_roles", "gelu_tanh", precision)
    O, A, n = c["obs"], c["act"], 17
    s, a = rows_for(c, n, seed=6)
    rb = ReplayBuffer(12, device=DEV, obs_dim=O, act_dim=A, layout="soa")
    rng = np.random.default_rng(4)
    rb.push_batch(rng.standard_normal((12, O), dtype=np.float32), rng.uniform(-1, 1, (12, A)).astype(np.float32),
                  np.zeros(12, np.float32), rng.standard_normal((12, O), dtype=np.float32), np.zeros(12, np.float32))
    torch.cuda.synchronize()
    h = eng.handle.value
    eng.ops.q_values(h, s, a, True)  # both kernels loaded before the capture
    eng.ops.q_values_replay(h, rb.storage, rb.state, rb.layout_spec, 10, 5, True, False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q = eng.ops.q_values(h, s, a, True)
        qr = eng.ops.q_values_replay(h, rb.storage, rb.state, rb.layout_spec, 10, 5, True, False)
    for k in range(2):  # each replay on new inputs in the captured buffers
        s2, a2 = rows_for(c, n, seed=20 + k)
        s.copy_(s2)
        a.copy_(a2)
        rb.next_obs.mul_(-0.5)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(q), bits(eng.q_values(s2, a2, target=True))), k
        assert np.array_equal(bits(qr), bits(eng.q_values_replay(rb, 10, 5))), k


# ---------------------------------------------------------------- 6 - 9. the device loop
N_ENVS, T_STEPS, CAPACITY = 5, 12, 24  # 60 transitions through a ring of 24


def loop_cfg(warming, log_q=True, precision="fp32"):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.2, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [32, 32], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [32, 32], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": 1.0},
        "buffer": {"capacity": CAPACITY},
        "train": {"gradient_steps_per_update": 1, "update_frequency": 1, "seed": 3, "batch_size": 16,
                  "warming_steps": warming, "device": "cuda", "precision": precision, "graph_chunk": 4},
        "logger": {"enabled": False, "env_name": "probe", "agent_name": "SAC", "log_episode_stats": False,
                   "log_q_values": log_q, "save_model": {"enabled": False, "path": None}},
    }


def loop_agent(warming, log_q=True, precision="fp32"):
    from sac import envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    host = envs.OneDPointMassReachEnv(max_steps=7, dt=0.5, action_low=-1.0, action_high=1.0, goal_pos=0.5,
                                      goal_tolerance=0.2)
    dv = DeviceVectorEnv.from_env(host, N_ENVS, device=DEV)
    return SAC(dv, loop_cfg(warming, log_q, precision)), dv


class QLogger:
    def __init__(self):
        self.q, self.hparams = [], []

    def log_q_values(self, q1, q2, step):
        self.q.append((step, q1, q2))

    def log_hparams(self, cfg, metrics):
        self.hparams.append(dict(metrics))


def logged_bits(logger):
    return bits(np.array([(q1, q2) for _, q1, q2 in logger.q], np.float32)).reshape(-1, N_ENVS, 2)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_device_loop_logs_q_of_every_transition_critics_frozen(precision):
    agent, dv = loop_agent(warming=10 ** 6, precision=precision)  # no update ever falls due
    rb, eng, logger = agent.replay_buffer, agent.engine, QLogger()
    seen = []

    def keep_rows(c):  # the N transitions of this vector step, before the ring overwrites them
        slots = torch.tensor([(c["env_steps"] - N_ENVS + i) % CAPACITY for i in range(N_ENVS)], device=DEV)
        seen.append((rb.next_obs[slots].clone(), rb.act[slots].clone()))

    m = agent.run_device_training_loop(N_ENVS * T_STEPS, logger=logger, drain_every=5, callback=keep_rows,
                                       device_q_values=True)
    assert m["gradient_steps"] == 0 and eng.steps_done == 0 and m["total_env_steps"] == N_ENVS * T_STEPS
    assert [st for st, _, _ in logger.q] == list(range(1, N_ENVS * T_STEPS + 1))
    got = logged_bits(logger)
    assert len(seen) == T_STEPS and rb._pos == (N_ENVS * T_STEPS) % CAPACITY  # the ring wrapped
    for t, (s2, a) in enumerate(seen):
        assert np.array_equal(got[t], bits(eng.q_values(s2, a))), t
    assert len({tuple(r) for r in got.reshape(-1, 2).tolist()}) > T_STEPS  # not one constant


@pytest.fixture(scope="module")
def moving_run():
    """The loop with updates on and Q logging on the device, run once under the
    spies of test_loop_runs_without_host_sync (tests/test_gpu_device_envs.py)."""
    from sac.device_envs import DeviceQValueLog, EpisodeDrain
    from sac.engine import SacEngine

    agent, dv = loop_agent(warming=16)
    logger = QLogger()
    inside, calls, launches = [], [], []

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

    def count(orig):
        def f(self, replay, first_slot, n, **k):
            launches.append((first_slot, n))
            return orig(self, replay, first_slot, n, **k)
        return f

    consumed_inside = []
    with pytest.MonkeyPatch.context() as mp:
        for name in ("item", "cpu", "numpy"):
            mp.setattr(torch.Tensor, name, spy(name, getattr(torch.Tensor, name)))
        mp.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
        mp.setattr(EpisodeDrain, "finish", wrap("EpisodeDrain.finish", EpisodeDrain.finish))
        mp.setattr(DeviceQValueLog, "finish", wrap("DeviceQValueLog.finish", DeviceQValueLog.finish))
        mp.setattr(SacEngine, "check", wrap("SacEngine.check", SacEngine.check))
        mp.setattr(SacEngine, "q_values_replay", count(SacEngine.q_values_replay))
        metrics = agent.run_device_training_loop(N_ENVS * T_STEPS, logger=logger, drain_every=5,
                                                 callback=lambda c: consumed_inside.append(len(logger.q)),
                                                 device_q_values=True)
    return dict(agent=agent, logger=logger, metrics=metrics, calls=calls, launches=launches,
                consumed_inside=consumed_inside)


def test_device_loop_logs_match_lockstep_agent_critics_moving(moving_run):
    from sac.agent import due_updates_gated

    r = moving_run
    other, dv = loop_agent(warming=16)  # same seed, driven by hand
    rb, eng, tr = other.replay_buffer, other.engine, other.config["train"]
    dv.reset(seed=None)
    want, total, grad = [], 0, 0
    for _ in range(T_STEPS):
        len_before, first = len(rb), rb._pos
        eng.rollout_step(dv, rb)
        old, total = total, total + N_ENVS
        due = due_updates_gated(old, total, len_before, rb.capacity, tr["warming_steps"], tr["update_frequency"],
                                tr["gradient_steps_per_update"])
        if other.can_update() and due:
            other._run_updates(due)
            grad += due
        want.append(eng.q_values_replay(rb, first, N_ENVS))
    torch.cuda.synchronize()
    eng.check()
    assert r["metrics"]["gradient_steps"] == grad > 0 and r["agent"].engine.steps_done == grad
    assert [st for st, _, _ in r["logger"].q] == list(range(1, N_ENVS * T_STEPS + 1))
    got = logged_bits(r["logger"])
    for t in range(T_STEPS):
        assert np.array_equal(got[t], bits(want[t])), t
    # one launch per vector step, on the slots the rollout step wrote
    assert r["launches"] == [((t * N_ENVS) % CAPACITY, N_ENVS) for t in range(T_STEPS)]
    # the values are those of the moment: no update ran after the last vector step, one ran after the one before
    slot = lambda t: (t * N_ENVS) % CAPACITY  # noqa: E731
    assert np.array_equal(bits(eng.q_values_replay(rb, slot(T_STEPS - 1), N_ENVS)), bits(want[-1]))
    assert not np.array_equal(bits(eng.q_values_replay(rb, slot(T_STEPS - 2), N_ENVS)), bits(want[-2]))
    # copies queued inside the loop (every 5 < 12 vector steps) are handed over whole and in order, whenever
    # they land; the last 2 cells can only come from the final blocking drain
    seen = r["consumed_inside"]
    print("values consumed by the end of each vector step:", seen)
    assert seen == sorted(seen) and all(k % (5 * N_ENVS) == 0 for k in seen) and seen[-1] <= 10 * N_ENVS


def test_device_loop_with_q_logging_runs_without_host_sync(moving_run):
    calls = moving_run["calls"]
    outside = [c for c in calls if c[1] is None]
    assert outside == [], f"host syncs inside the loop: {collections.Counter(n for n, _ in outside)}"
    assert all(w in ("EpisodeDrain.finish", "DeviceQValueLog.finish", "SacEngine.check") for _, w in calls)


def test_gates():
    from sac.engine import SacEngine

    launches = []
    with pytest.MonkeyPatch.context() as mp:
        for name in ("q_values", "q_values_replay"):
            orig = getattr(SacEngine, name)
            mp.setattr(SacEngine, name, lambda self, *a, _o=orig, **k: (launches.append(1), _o(self, *a, **k))[1])
        agent, _ = loop_agent(warming=16, log_q=False)
        logger = QLogger()
        m = agent.run_device_training_loop(N_ENVS * T_STEPS, logger=logger, device_q_values=True)
        assert m["gradient_steps"] > 0 and logger.q == [] and launches == []
        # the default still refuses the config key, and names the way out
        agent, _ = loop_agent(warming=16, log_q=True)
        with pytest.raises(ValueError, match="log_q_values") as e:
            agent.run_device_training_loop(N_ENVS * T_STEPS, logger=QLogger())
        assert "device_q_values" in str(e.value) and launches == []
        # no logger, nothing to log to: nothing launched either
        agent.logger = None
        agent.run_device_training_loop(N_ENVS * 2, device_q_values=True)
        assert launches == []
