"""GPU-side helpers: build an agent on the fixture's config and feed the
fixture's batches/eps through the C ABI with injected indices."""
import copy

import numpy as np
import torch

from _fixtures import batch, eps, init_state_dicts, load


class FakeSpace:
    def __init__(self, n):
        self.shape = (n,)

    def seed(self, s):
        return [s]

    def sample(self):
        return np.zeros(self.shape, np.float32)


class FakeEnv:
    spec = None

    def __init__(self, obs, act):
        self.observation_space = FakeSpace(obs)
        self.action_space = FakeSpace(act)

    def reset(self, seed=None, options=None):
        return np.zeros(self.observation_space.shape, np.float32), {}


def make_agent(name, precision="fp32", capacity=None):
    from sac.agent import SAC

    fx, meta = load(name)
    cfg = copy.deepcopy(meta["cfg"])
    cfg["train"]["device"] = "cuda"
    cfg["train"]["precision"] = precision
    B = meta["batch"]
    cfg["buffer"]["capacity"] = capacity or B * meta["steps"]
    agent = SAC(FakeEnv(meta["obs"], meta["act"]), cfg)
    sds = init_state_dicts(name)
    nets = {"policy": agent.policy_net, "q1": agent.q_net1, "q2": agent.q_net2, "q1t": agent.q_net1_target,
            "q2t": agent.q_net2_target}
    with torch.no_grad():
        for k, net in nets.items():
            for pk, p in net.state_dict().items():
                p.copy_(torch.from_numpy(np.asarray(sds[k][pk])))
    agent.engine.sync_params()
    for k in range(1, meta["steps"] + 1):
        b = batch(fx, k)
        agent.replay_buffer.push_batch(b.s, b.a, b.r, b.s2, b.d)
    return agent, fx, meta, nets


def _net_cfg(c):
    """The activation and shape fields of an engine config dict, with the
    defaults of bench.build_engine (ReLU nets, identity outputs, auto alpha,
    log sigma clamped to [-20, 2])."""
    return dict(q_hidden=c.get("q_hidden", c.get("hidden")), pi_hidden=c.get("pi_hidden", c.get("hidden")),
                q_act=c.get("q_act", "relu"), pi_act=c.get("pi_act", "relu"),
                q_out_act=c.get("q_out_act", "identity"), pi_out_act=c.get("pi_out_act", "identity"),
                auto=bool(c.get("auto", True)), log_std_min=c.get("log_std_min", -20), log_std_max=c.get("log_std_max", 2))


# build_engine's hyper-parameters where the config dict names none: those of bench.build_engine
HYPER_DEFAULTS = dict(gamma=0.99, tau=0.005, alpha=0.1, actor_lr=3e-4, critic_lr=3e-4, alpha_lr=3e-4,
                      action_scale=1.0, betas=(0.9, 0.999), adam_eps=1e-8, target_entropy=None)


def _hyper(c):
    return {k: c.get(k, d) for k, d in HYPER_DEFAULTS.items()}


def synthetic_rows(cap, obs, act, seed, done_p):
    """bench.synthetic_replay's rows (s ~ N(0, 1), a ~ U(-1, 1), r ~ N(0, 1),
    s' = the next row's s, the same draws in the same order) with terminal
    probability done_p instead of its 1 %, as a dict of the replay's columns
    (no GPU needed)."""
    rng = np.random.default_rng(seed)
    s_all = rng.standard_normal((cap + 1, obs), dtype=np.float32)
    a = rng.uniform(-1, 1, (cap, act)).astype(np.float32)
    r = rng.standard_normal(cap, dtype=np.float32)
    d = (rng.random(cap) < done_p).astype(np.float32)
    return dict(obs=s_all[:cap], act=a, rew=r, next_obs=s_all[1:cap + 1], done=d)


def config_rows(c, seed=3):
    """The replay rows build_engine fills for a config dict that names done_p."""
    return synthetic_rows(c["capacity"], c["obs"], c["act"], c.get("replay_seed", seed), c["done_p"])


def torch_nets(c, seed=3):
    """(pi, q1, q2) torch modules of a config dict on the CPU, as build_engine creates them."""
    from sac.models import PolicyNetwork, QNetwork

    n, h = _net_cfg(c), _hyper(c)
    pi = PolicyNetwork(c["obs"], c["act"], n["pi_hidden"], log_std_min=n["log_std_min"], log_std_max=n["log_std_max"],
                       seed=seed, action_scale=h["action_scale"], hidden_activations=n["pi_act"],
                       output_activation=n["pi_out_act"])
    q1 = QNetwork(c["obs"], c["act"], n["q_hidden"], n["q_act"], n["q_out_act"], seed=seed)
    q2 = QNetwork(c["obs"], c["act"], n["q_hidden"], n["q_act"], n["q_out_act"], seed=seed + 1)
    return pi, q1, q2


def oracle_fresh_state(c, seed=3):
    """The oracle's state of a config dict before its first step, from the same
    initial parameters build_engine gives the engine, and its hyper-parameters
    (no GPU needed).  Returns (SacState, SacHyper)."""
    from oracle import sac_oracle as O

    hp = oracle_hyper(c)
    mlps = [O.MLP.from_state_dict({k: v.detach().numpy().copy() for k, v in net.state_dict().items()},
                                  net.hidden_activations, net.output_activation) for net in torch_nets(c, seed)]
    return O.SacState.fresh(*mlps, hp, c["act"]), hp


def build_engine(c, precision, seed=3, device=None, layout=None, replay=None):
    """Engine + synthetic replay of a config dict, as bench.build_engine builds
    them (same seeding, hyper-parameters and replay rows), with the fields that
    one leaves at its defaults:
      obs, act, batch, capacity;
      hidden, or q_hidden and pi_hidden (they may differ);
      q_act, pi_act, q_out_act, pi_out_act (sac.models activation names);
      auto (entropy tuning; False: alpha stays at its initial value), log_std_min, log_std_max;
      gamma, tau, alpha (the initial one), actor_lr, critic_lr, alpha_lr, action_scale;
      betas, adam_eps (Adam, of all four optimizers), target_entropy (None: -act);
      done_p (terminal probability of the replay rows; given, the rows come
      from synthetic_rows instead of bench.synthetic_replay, which has 1 %;
      replay_seed: their seed, default the engine's);
      layout (kernel layout overrides of sac.engine.SacEngine; the `layout`
      argument is merged over it).
    replay: a caller's ReplayBuffer, returned as it is in place of the
    synthetic one (a ring state of tests/_ring.py, say; c's capacity is then
    not used).
    The engine gains `.split` (sac_engine_uses_split, include/
    sac_engine_testing.h) next to .roles / .pairs / .wide.  Returns (engine,
    replay, c)."""
    import ctypes

    import bench
    from sac.engine import SacEngine
    from sac.replay_buffer import ReplayBuffer

    device = device or torch.device("cuda", 0)
    n, h = _net_cfg(c), _hyper(c)
    pi, q1, q2 = (net.to(device) for net in torch_nets(c, seed))
    q1t, q2t = copy.deepcopy(q1), copy.deepcopy(q2)
    lay = dict(c.get("layout") or {}, **(layout or {}))
    eng = SacEngine(pi, q1, q2, q1t, q2t, batch_size=c["batch"], gamma=h["gamma"], tau=h["tau"],
                    actor_lr=h["actor_lr"], critic_lr=h["critic_lr"], alpha_lr=h["alpha_lr"], alpha=h["alpha"],
                    auto_entropy_tuning=n["auto"], device=device, precision=precision, seed=seed,
                    betas=tuple(h["betas"]), eps=h["adam_eps"], target_entropy=h["target_entropy"], layout=lay or None)
    eng.lib.sac_engine_uses_split.argtypes = [ctypes.c_void_p]
    eng.split = bool(eng.lib.sac_engine_uses_split(eng.handle))
    if replay is not None:
        assert (replay.obs_dim, replay.act_dim) == (c["obs"], c["act"])
        return eng, replay, c
    rb = ReplayBuffer(c["capacity"], device=device, obs_dim=c["obs"], act_dim=c["act"])
    if c.get("done_p") is None:
        bench.synthetic_replay(rb, c["capacity"], c["obs"], c["act"], seed)
    else:
        r = config_rows(c, seed)
        rb.push_batch(r["obs"], r["act"], r["rew"], r["next_obs"], r["done"])
        torch.cuda.synchronize()
    return eng, rb, c


def layout_of(eng):
    """The kernel family phases A and C of a build_engine engine run, by assert_layout's names."""
    return "stage" if eng.wide else "split" if eng.split else "roles" if eng.roles else "pairs" if eng.pairs else "rows"


def assert_layout(eng, want):
    """The kernel family phases A and C run: "split" (hidden-split role
    kernels), "roles" (per-network role kernels without the split), "rows"
    (one workgroup per row tile), "pairs" (pair tiles) or "stage" (the
    layer-synchronous stage path)."""
    got = layout_of(eng)
    flags = dict(split=eng.split, roles=eng.roles, pairs=eng.pairs, wide=eng.wide)
    assert got == want, (want, flags)
    # the flags exclude one another, except that the hidden split is a form of the role kernels
    assert not (eng.wide and (eng.roles or eng.pairs)) and not (eng.pairs and eng.roles), flags
    assert eng.roles or not eng.split, flags


def oracle_hyper(c):
    """oracle.sac_oracle.SacHyper of build_engine(c)."""
    from oracle import sac_oracle as O

    n, h = _net_cfg(c), _hyper(c)
    return O.SacHyper(gamma=h["gamma"], tau=h["tau"], alpha=h["alpha"], auto_entropy_tuning=n["auto"],
                      actor_lr=h["actor_lr"], critic_lr=h["critic_lr"], alpha_lr=h["alpha_lr"],
                      policy=O.PolicyCfg(n["log_std_min"], n["log_std_max"], h["action_scale"]),
                      beta1=h["betas"][0], beta2=h["betas"][1], adam_eps=h["adam_eps"],
                      target_entropy=h["target_entropy"])


def engine_mlp(eng, key):
    """Oracle MLP holding the engine's current parameters of one network, with
    that network's hidden and output activations."""
    from oracle import sac_oracle as O

    net = eng.nets[key]
    return O.MLP.from_state_dict({kk: v.detach().cpu().numpy().copy() for kk, v in net.state_dict().items()},
                                 net.hidden_activations, net.output_activation)


def run_step(agent, fx, meta, k):
    B, A = meta["batch"], meta["act"]
    idx = torch.arange((k - 1) * B, k * B, dtype=torch.int32).reshape(1, B)
    et, ea = eps(fx, k)
    e = torch.from_numpy(np.stack([et, ea])).reshape(1, 2, B, A)
    agent.engine.train(agent.replay_buffer, 1, indices=idx, eps=e)
    torch.cuda.synchronize()
    st = agent.engine.stats.cpu().numpy()
    return st[:4].astype(np.float64), st[4:4 + B], st[4 + B:4 + 2 * B]
