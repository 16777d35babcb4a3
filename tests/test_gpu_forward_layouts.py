"""The forward-only kernels -- the policy kernel behind sac_policy_act and the
fused rollout step behind sac_rollout_step -- on every engine layout.

Both run on the engine's row-tile LDS layout and on the packed weight copies,
whichever kernels the training phases use.  plan() builds that LDS layout three
ways (2R-row buffers for the row tiles, another set of buffers for the pair
tiles, R rows and no pre-activation buffers on the stage path) and four families
of update code rewrite the packed copies, so every check here runs on split,
roles, rows, pairs and stage engines, forced and unforced (the critic kernel's
share of this is in test_gpu_q_values.py).

Yardstick: a ``.double()`` copy of the policy module over the engine's current
parameters, with the head of sac/models.py (clamp, exp, z = mu + eps sigma,
a = tanh(z) scale) in float64 on the CPU and

    log pi = sum_j [-eps^2 / 2 - log sigma - 1/2 log 2 pi] - sum_j 2 (log 2 - z - softplus(-2 z)).

Metrics: actions |a - ref| / scale, log pi |lp - ref| / max(1, |ref|).  Bounds:
the project's 2e-5 (fp32 mode) and 3e-2 (bf16 mode), those of
test_policy_act_matches_torch and test_gpu_q_values.py.  Next to every kernel
error the tests print the error of the reference arithmetic on the same rows
against float64 (fp32: the torch module in float32 on the CPU; bf16: the float64
forward with the weights and every layer's inputs rounded to bf16):
profiles/forward_layouts_gputest.txt.  Placement (tile, slot, ragged tiles) is
compared with the kernel's own output on the same rows, bit for bit.

act17: create accepts act 17 (the header's limit is act <= 32), so the 34 output
columns cross the 32-column pad as asked; no smaller stand-in is used.  It runs
the role kernels only: act17_rows and act17_pairs put the same 34 columns on the
row and pair tiles' 2R-row buffers, act32_roles is the widest head (64 columns)
and act8_stage the stage path's (2 act = 16).

Head saturation: the issue's bias cycles have five entries and the engines it
names have at most three action dimensions, so at a fixed start the +-20 means
and the upper clamp edge would never be reached.  The cycles are therefore
started at each of their five entries in turn (start 0 is the cycle as stated),
and act17, which holds the whole cycle at once, is run as well.  The tanh-output
variant bounds |mu| by 1, so |z| > 15 is asserted on the identity-output engines
only; both clamp edges are asserted on every engine."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _depth
import _widths

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = {"fp32": 2e-5, "bf16": 3e-2}
NETS = ("pi", "q1", "q2", "q1t", "q2t")
ROWS = (1, 16, 17, 33)  # one row, a full tile, a ragged tile, three tiles

PAD = dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=64)
DEEP = dict(obs=11, act=3, hidden=[128, 96, 64], batch=80, capacity=128)
# name -> (config dict of _gpu.build_engine, layout override, the kernel family phases A / C then run)
ENGINES = {
    "split_c2": (dict(obs=24, act=4, hidden=[256, 256], batch=256, capacity=512), None, "split"),
    "roles_pad": (PAD, {"layout": "roles"}, "roles"),
    "rows_pad": (PAD, {"layout": "rows"}, "rows"),
    "pairs_pad": (PAD, {"layout": "pairs"}, "pairs"),
    "pairs_deep": (DEEP, {"layout": "pairs"}, "pairs"),
    "roles_deep": (DEEP, None, "roles"),
    "stage_pad": (PAD, {"stage_path": 1}, "stage"),
    # the stage path because the shape does not fit the phase kernels' LDS layout
    "stage_obs300": (dict(obs=300, act=6, hidden=[256, 256], batch=64, capacity=128), None, "stage"),
    "stage_512": (dict(obs=24, act=4, hidden=[512, 512], batch=64, capacity=128), None, "stage"),
    "stage_400_300": (dict(obs=17, act=6, hidden=[400, 300], batch=64, capacity=128), None, "stage"),
    # the rollout kernel's action width; 2 act = 34 output columns across the 32-column pad
    "act1": (dict(obs=5, act=1, hidden=[64, 64], batch=17, capacity=64), None, "roles"),
    "act17": (dict(obs=3, act=17, hidden=[64, 64], batch=32, capacity=64), None, "roles"),
    # wide actions on the other LDS layouts: the row and pair tiles' 2R-row buffers at 34 output columns, 64
    # output columns (the API's maximum) and the stage path's widest head (2 act = 16)
    "act17_rows": (dict(PAD, act=17), {"layout": "rows"}, "rows"),
    "act17_pairs": (dict(PAD, act=17), {"layout": "pairs"}, "pairs"),
    "act32_roles": (dict(PAD, act=32), {"layout": "roles"}, "roles"),
    "act8_stage": (dict(PAD, act=8), {"stage_path": 1}, "stage"),
}
# network depths 1 and 5 (tests/_depth.py): the kernels' own layer loops with one hidden layer (the output layer is
# layer 1) and with all SAC_DEV_LAYERS slots in use; q5_pi1: a one-layer policy on an LDS layout the five-layer
# critics size; h1_256: one hidden layer of 256 (the hidden split refused by depth)
DEPTH_ENGINES = ("h1_roles", "h1_rows", "h1_pairs", "h5_roles", "h5_pairs", "h5_stage", "q5_pi1_roles", "q5_pi1_rows",
                 "h1_256_roles")
ENGINES.update({k: (dict(_depth.CASES[k][0], capacity=64),) + _depth.CASES[k][1:] for k in DEPTH_ENGINES})
# layer widths off the 8-column grid (tests/_widths.py): [50, 33] on every family, a hidden layer of one unit, one
# past 256 (a 17th column tile) and [299, 401] on the stage path: the forward epilogues' n < N at a ragged last tile
# and the packed copies at odd K and N
WIDTH_ENGINES = ("odd_roles", "odd_rows", "odd_pairs", "odd_stage", "tiny_roles", "w257_roles", "w401_stage")
ENGINES.update({k: (dict(_widths.CASES[k][0], capacity=64),) + _widths.CASES[k][1:] for k in WIDTH_ENGINES})
ACTS = {"relu": dict(),
        "tanh": dict(pi_act="tanh", pi_out_act="tanh", log_std_min=-0.5, log_std_max=0.5, action_scale=2.5)}
CASES = [(name, "relu") for name in ENGINES] + [(name, "tanh") for name in ("roles_pad", "pairs_pad", "stage_pad")]


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def randomise(eng, seed=11, scale=0.1):
    """Independent N(0, scale^2) noise on every parameter of all five nets: the
    policy's output depends on every weight and bias, target != online, Q1 != Q2."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for k in NETS:
            eng.flat[k].add_((scale * torch.randn(eng.flat[k].numel(), generator=g)).to(eng.device))
    eng.sync_params()


def make_engine(name, acts, precision, **over):
    from _gpu import assert_layout, build_engine

    c, layout, family = ENGINES[name]
    eng, rb, c = build_engine(dict(c, **ACTS[acts], **over), precision, device=DEV, layout=layout)
    assert_layout(eng, family)
    randomise(eng)
    return eng, rb, c


_engines = {}


def shared_engine(name, acts, precision):
    """Engines of the read-only tests, built once (no test that takes one trains or edits it)."""
    key = (name, acts, precision)
    if key not in _engines:
        _engines[key] = make_engine(*key)
    return _engines[key]


def rows_for(c, n, seed=0):
    """n observation rows and their noise, on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, c["obs"], generator=g), torch.randn(n, c["act"], generator=g)


# ---------------------------------------------------------------- the float64 reference
def policy64(eng):
    """A float64 copy of the policy module over the engine's current parameters, on the CPU."""
    from sac.models import PolicyNetwork

    net = eng.nets["pi"]
    hidden = [lin.out_features for lin in net.linears()[:-1]]
    ref = PolicyNetwork(net.obs_size, net.action_size, hidden, log_std_min=net.log_std_min,
                        log_std_max=net.log_std_max, action_scale=net.action_scale,
                        hidden_activations=net.hidden_activations, output_activation=net.output_activation).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref


def net_out64(ref, s, bf16=False):
    """ref.net(s) in float64; bf16: the weights and every layer's inputs rounded to bf16 first."""
    x = s.double()
    with torch.no_grad():
        if not bf16:
            return ref.net(x).numpy()
        rnd = lambda t: t.float().bfloat16().double()  # noqa: E731
        for m in ref.net:
            x = torch.nn.functional.linear(rnd(x), rnd(m.weight), m.bias) if isinstance(m, torch.nn.Linear) else m(x)
        return x.numpy()


def head64(ref, out, eps):
    """The head of sac/models.py on the net's float64 output [n][2A] ->
    dict(det, act, lp, z, ls, raw): tanh(mu) scale, tanh(z) scale, log pi, and
    z, the clamped and the raw log sigma."""
    A = ref.action_size
    mu, raw = out[:, :A], out[:, A:]
    ls = np.clip(raw, ref.log_std_min, ref.log_std_max)
    e = eps.double().numpy()
    z = mu + e * np.exp(ls)
    lp = np.sum(-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi), axis=1) \
        - np.sum(2.0 * (math.log(2.0) - z - np.logaddexp(0.0, -2.0 * z)), axis=1)
    return dict(det=np.tanh(mu) * ref.action_scale, act=np.tanh(z) * ref.action_scale, lp=lp, z=z, ls=ls, raw=raw)


def ref_outputs(ref, s, eps, bf16=False):
    return head64(ref, net_out64(ref, s, bf16), eps)


def torch32_outputs(ref, s, eps):
    """The torch module in float32 on the CPU and head64's formulas in float32 (not
    torch.distributions' log_prob: its (z - mu)^2 / (2 sigma^2) cancels for a small sigma, so
    it is no yardstick for an error)."""
    from sac.models import PolicyNetwork

    hidden = [lin.out_features for lin in ref.linears()[:-1]]
    m = PolicyNetwork(ref.obs_size, ref.action_size, hidden, log_std_min=ref.log_std_min, log_std_max=ref.log_std_max,
                      action_scale=ref.action_scale, hidden_activations=ref.hidden_activations,
                      output_activation=ref.output_activation)
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    with torch.no_grad():
        mu, log_std = m(s.float())
        e = eps.float()
        z = mu + e * log_std.exp()
        lp = (-0.5 * e * e - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        lp = lp - (2.0 * (math.log(2.0) - z - torch.nn.functional.softplus(-2.0 * z))).sum(-1)
        return dict(det=(torch.tanh(mu) * m.action_scale).numpy(), act=(torch.tanh(z) * m.action_scale).numpy(),
                    lp=lp.numpy())


def errors(got, want, scale):
    """(deterministic action, sampled action, log pi) errors in the metrics of the module docstring."""
    e = [float(np.max(np.abs(np.asarray(got[k], np.float64) - want[k]))) / scale for k in ("det", "act")]
    lp = np.asarray(got["lp"], np.float64)
    return e + [float(np.max(np.abs(lp - want["lp"]) / np.maximum(1.0, np.abs(want["lp"]))))]


def arithmetic_errors(ref, s, eps, want, precision):
    """The reference arithmetic of `precision` on the same rows, against float64."""
    got = torch32_outputs(ref, s, eps) if precision == "fp32" else ref_outputs(ref, s, eps, bf16=True)
    return errors(got, want, ref.action_scale)


def bounds(arith, tol):
    """The bound of each metric: the project's tolerance wherever the reference arithmetic of
    that precision meets it on these rows; where that arithmetic itself misses it (bf16 at the
    wide and deep shapes, and where log pi passes near 0), 4 x the arithmetic's error.
    Nothing of the kernel's output enters."""
    return [tol if a <= tol else 4.0 * a for a in arith]


def kernel_outputs(eng, s, eps):
    """policy_act in both modes -> dict(det, act, lp) of numpy arrays; shapes, dtypes and the
    deterministic call's missing log pi are asserted on the way."""
    n, A = s.shape[0], eng.cfg.act_dim
    det, none = eng.policy_act(s.to(DEV), None, want_log_pi=True)
    assert none is None  # no noise, no log pi
    act, lp = eng.policy_act(s.to(DEV), eps.to(DEV), want_log_pi=True)
    assert tuple(det.shape) == tuple(act.shape) == (n, A) and tuple(lp.shape) == (n,)
    assert det.dtype == act.dtype == lp.dtype == torch.float32
    only_act = eng.policy_act(s.to(DEV), eps.to(DEV))
    assert np.array_equal(bits(only_act), bits(act))  # the action does not depend on whether log pi is asked for
    return dict(det=det.cpu().numpy(), act=act.cpu().numpy(), lp=lp.cpu().numpy())


def fmt(e):
    return "/".join(f"{x:.2e}" for x in e)


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,acts", CASES)
def test_policy_act_matches_float64(name, acts, precision):
    eng, _, c = shared_engine(name, acts, precision)
    ref, tol, tag = policy64(eng), TOL[precision], f"policy_act {name} {acts} {precision}"
    scale = float(ref.action_scale)
    assert float(eng.cfg.action_scale) == scale == (2.5 if acts == "tanh" else 1.0)
    worst, worst_arith = [0.0] * 3, [0.0] * 3
    for n in ROWS:
        s, eps = rows_for(c, n, seed=n)
        want = ref_outputs(ref, s, eps)
        err = errors(kernel_outputs(eng, s, eps), want, scale)
        arith = arithmetic_errors(ref, s, eps, want, precision)
        worst = [max(a, b) for a, b in zip(worst, err)]
        worst_arith = [max(a, b) for a, b in zip(worst_arith, arith)]
        print(f"{tag} n={n}: det/act/log_pi err {fmt(err)}, the reference arithmetic {fmt(arith)}")
        assert all(e <= b for e, b in zip(err, bounds(arith, tol))), (n, err, arith)
    print(f"{tag}: worst {fmt(worst)} (bound {tol:g}), the reference arithmetic {fmt(worst_arith)}")
    # what these rows can tell apart, on the references alone
    s, eps = rows_for(c, 33, seed=33)
    want = ref_outputs(ref, s, eps)
    assert np.max(np.abs(want["act"] - want["det"])) / scale > 2 * tol  # the noise is applied
    if acts == "tanh":
        assert np.any(want["raw"] < ref.log_std_min) and np.any(want["raw"] > ref.log_std_max)  # both clamp edges
        assert np.max(np.abs(want["act"])) > 1.0  # |tanh| alone stays below 1: the scale shows
    # every layer counts: zeroing one layer's weights moves the float64 output past the bound
    for li, lin in enumerate(ref.linears()):
        kept = lin.weight.detach().clone()
        with torch.no_grad():
            lin.weight.zero_()
            moved = errors(ref_outputs(ref, s, eps), want, scale)
            lin.weight.copy_(kept)
        assert max(moved) > 2 * tol, (li, moved)


# ---------------------------------------------------------------- 2. head saturation
MU_BIAS = (0.0, 3.0, -9.0, 20.0, -20.0)
LS_BIAS = (-30.0, -5.0, 0.0, 1.0, 10.0)
SATURATION = [("roles_pad", "relu"), ("roles_pad", "tanh"), ("act1", "relu"), ("pairs_deep", "relu"),
              ("act17", "relu")]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,acts", SATURATION)
def test_policy_head_in_saturation(name, acts, precision):
    """Means of +-20, log sigma far past both clamp edges and noise of up to 4 sigma:
    tanhf, expf, logf, the softplus and the clamp where they saturate."""
    eng, _, c = make_engine(name, acts, precision)
    A, n, tol, scale = c["act"], 33, TOL[precision], float(eng.cfg.action_scale)
    s, _ = rows_for(c, n, seed=7)
    g = torch.Generator(device="cpu").manual_seed(8)
    eps = torch.tensor([0.0, 1.0, -1.0, 4.0, -4.0])[torch.randint(0, 5, (n, A), generator=g)]
    last = eng.nets["pi"].linears()[-1]
    big_z = low = high = False
    for start in range(5):
        with torch.no_grad():
            last.bias[:A] = torch.tensor([MU_BIAS[(start + j) % 5] for j in range(A)], device=DEV)
            last.bias[A:] = torch.tensor([LS_BIAS[(start + j) % 5] for j in range(A)], device=DEV)
        eng.sync_params()
        ref = policy64(eng)
        want = ref_outputs(ref, s, eps)
        got = kernel_outputs(eng, s, eps)
        for k in ("det", "act", "lp"):
            assert np.all(np.isfinite(got[k])), (start, k)
        assert np.all(np.abs(got["det"]) <= scale) and np.all(np.abs(got["act"]) <= scale), start
        err = errors(got, want, scale)
        arith = arithmetic_errors(ref, s, eps, want, precision)
        print(f"saturation {name} {acts} {precision} start={start}: det/act/log_pi err {fmt(err)}, "
              f"the reference arithmetic {fmt(arith)}, max |z| {np.max(np.abs(want['z'])):.1f}")
        # fp32: the bound as it is; bf16: mu's rounding moves z by up to |z| 2^-8, which a log pi near 0 does not absorb
        bnd = bounds(arith, tol) if precision == "bf16" else [tol] * 3
        assert all(e <= b for e, b in zip(err, bnd)), (start, err, arith)
        big_z |= bool(np.any(np.abs(want["z"]) > 15))
        low |= bool(np.any(want["raw"] < ref.log_std_min))
        high |= bool(np.any(want["raw"] > ref.log_std_max))
    assert low and high  # sigma at each clamp edge
    assert big_z or acts == "tanh"  # a tanh output keeps |mu| <= 1


# ---------------------------------------------------------------- 3. row independence
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["rows_pad", "pairs_pad", "pairs_deep", "stage_512", "split_c2", "act17",
                                  "h1_roles", "h1_pairs", "h5_roles", "h5_stage", "q5_pi1_rows"])
def test_rows_do_not_depend_on_their_tile(name, precision):
    eng, _, c = shared_engine(name, "relu", precision)
    n = 33
    s, eps = (t.to(DEV) for t in rows_for(c, n, seed=2))

    def run(s_, eps_, sampled):  # -> the call's outputs as bit patterns
        if not sampled:
            return [bits(eng.policy_act(s_))]
        a, lp = eng.policy_act(s_, eps_, want_log_pi=True)
        return [bits(a), bits(lp)]

    for sampled in (False, True):
        full = run(s, eps, sampled)
        fs, fe = (t.to(DEV) for t in rows_for(c, 16, seed=9))  # other rows around the one under test
        for i in (0, 1, 15, 16, 17, 31, 32):
            alone = run(s[i:i + 1], eps[i:i + 1], sampled)
            fs[15], fe[15] = s[i], eps[i]
            last = run(fs, fe, sampled)
            for f, a, l in zip(full, alone, last):
                assert np.array_equal(a[0], f[i]), (sampled, i)
                assert np.array_equal(l[15], f[i]), (sampled, i)
        # and a prefix of the rows gives a prefix of the outputs (ragged last tile)
        for f, p in zip(full, run(s[:17], eps[:17], sampled)):
            assert np.array_equal(p, f[:17]), sampled


# ---------------------------------------------------------------- 4. freshness
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["roles_pad", "rows_pad", "pairs_pad", "stage_pad", "stage_512", "split_c2",
                                  "h1_roles", "h1_rows", "h1_pairs", "h5_roles", "h5_pairs", "h5_stage"])
def test_policy_act_reads_the_updated_copies(name, precision):
    """A large actor step (actor_lr 3e-2) so that two gradient steps move the
    policy's outputs by more than the bound: after train, after train_graph and
    after a host-side edit with sync_params the kernel must compute the current
    parameters' policy, and its earlier outputs must no longer pass."""
    eng, rb, c = make_engine(name, "relu", precision, actor_lr=3e-2)
    tol, scale = TOL[precision], float(eng.cfg.action_scale)
    s, eps = rows_for(c, 33, seed=4)

    def check(before, what):
        ref = policy64(eng)
        want = ref_outputs(ref, s, eps)
        now = kernel_outputs(eng, s, eps)
        err, stale = errors(now, want, scale), errors(before, want, scale)
        arith = arithmetic_errors(ref, s, eps, want, precision)
        bnd = bounds(arith, tol)
        print(f"freshness {name} {precision} {what}: err {fmt(err)}, the reference arithmetic {fmt(arith)}, "
              f"earlier outputs {fmt(stale)}")
        assert all(e <= b for e, b in zip(err, bnd)), (what, err, arith)
        assert any(e > b + 2 * tol for e, b in zip(stale, bnd)), (what, stale)  # the earlier outputs miss by far
        return now

    out = kernel_outputs(eng, s, eps)
    eng.train(rb, 2)
    eng.check()
    out = check(out, "after train")
    eng.train_graph(rb, 2, chunk=2)
    eng.check()
    out = check(out, "after train_graph")
    with torch.no_grad():
        eng.flat["pi"].mul_(1.5)
    # before sync_params the kernel still reads the old packed weights (the biases it reads in place)
    mid = kernel_outputs(eng, s, eps)
    eng.sync_params()
    check(mid, "after sync_params")


# ---------------------------------------------------------------- 6. the fused rollout step
ENVS = {"random_obs": ("random_obs_binary", dict(obs_dim=5, threshold=0.2, max_steps=4)),
        "point_mass": ("point_mass", dict(max_steps=7, dt=0.5, action_low=-1.0, action_high=1.0, goal_pos=0.5,
                                          goal_tolerance=0.2))}
ROLLOUT_LAYOUTS = {"rows": {"layout": "rows"}, "pairs": {"layout": "pairs"}, "stage": {"stage_path": 1}, "roles": None,
                   # "<depth>_<family>": a one-layer and a five-layer policy under the fused step
                   "h1_roles": None, "h1_rows": {"layout": "rows"}, "h1_pairs": {"layout": "pairs"},
                   "h5_roles": None, "h5_pairs": {"layout": "pairs"}, "h5_stage": {"stage_path": 1}}
ROLLOUT_HIDDEN = {"": [64, 64], "h1": [64], "h5": [64, 40, 56, 24, 48]}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("family", sorted(ROLLOUT_LAYOUTS))
@pytest.mark.parametrize("env", sorted(ENVS))
def test_fused_actions_match_policy_act(env, family, precision):
    """test_gpu_device_envs.py::test_fused_actions_match_policy_act on each layout: the same
    arithmetic on the same packed copies, 1e-6 absolute."""
    from _gpu import assert_layout, build_engine
    from sac import _engine as E
    from sac.device_envs import DeviceVectorEnv
    from sac.replay_buffer import ReplayBuffer

    N, T = 17, 3
    kind, kw = ENVS[env]
    dv = DeviceVectorEnv(kind, N, device=DEV, **kw)
    O = dv.obs_dim
    assert (O, dv.act_dim) == (5 if env == "random_obs" else 1, 1)
    depth, _, kernels = family.rpartition("_")
    eng, _, c = build_engine(dict(obs=O, act=1, hidden=ROLLOUT_HIDDEN[depth], batch=17, capacity=64), precision,
                             device=DEV, layout=ROLLOUT_LAYOUTS[family])
    assert_layout(eng, kernels)
    assert len(eng.nets["pi"].linears()) == len(ROLLOUT_HIDDEN[depth]) + 1
    randomise(eng)
    lib = E.load_library()
    lib.sac_debug_rollout_eps_host.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_void_p]
    rb = ReplayBuffer(128, device=DEV, obs_dim=O, act_dim=1)
    dv.reset(seed=5)
    for _ in range(T):
        eng.rollout_step(dv, rb)
    torch.cuda.synchronize()
    assert len(rb) == T * N
    obs, act = rb.obs[:T * N].clone(), rb.act[:T * N].cpu().numpy()
    for t in range(1, T + 1):
        eps = np.zeros((N, 1), np.float32)
        assert lib.sac_debug_rollout_eps_host(int(eng.cfg.seed), t, N, 1, eps.ctypes.data) == 0
        sl = slice((t - 1) * N, t * N)
        want = eng.policy_act(obs[sl], torch.from_numpy(eps)).cpu().numpy()
        err = np.abs(act[sl] - want).max()
        print(f"rollout {env} {family} {precision} t={t}: |stored action - policy_act| {err:.2e}")
        assert err <= 1e-6, (t, err)
    assert len(np.unique(act)) > N  # not one constant action
    # deterministic: tanh(mu) * scale of the observation the step saw
    before = dv.obs.clone()
    eng.rollout_step(dv, rb, deterministic=True)
    torch.cuda.synchronize()
    got = rb.act[T * N:(T + 1) * N].cpu().numpy()
    want = eng.policy_act(before).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6
