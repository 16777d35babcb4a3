"""Helpers shared by the tests: load golden fixtures, build oracle states."""
import json
import os

import numpy as np

from oracle import sac_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ["c1_fixed", "c1_auto", "elu3_clamp", "mix_act", "gelu_tanh", "const_reward", "c2", "donkey_new",
           "out_smooth", "out_kink"]
FULL_INIT = ["c1_fixed", "c1_auto", "elu3_clamp", "mix_act", "gelu_tanh", "const_reward", "out_smooth", "out_kink"]


class NpzParts:
    """Read-only view of a fixture stored as several archives (<stem>.part0.npz,
    <stem>.part1.npz, ...: make_golden.save_npz keeps every committed file under
    1 MiB), with the ``.files`` / ``fx[key]`` / ``key in fx`` interface of
    numpy's NpzFile.  Every key lives in exactly one part."""

    def __init__(self, paths):
        self._where = {}
        for p in paths:
            z = np.load(p)
            for k in z.files:
                assert k not in self._where, (k, p)
                self._where[k] = z
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)


def load_npz(stem):
    """tests/golden/<stem>.npz, or its parts <stem>.part<k>.npz as one archive."""
    whole = os.path.join(GOLDEN, f"{stem}.npz")
    if os.path.exists(whole):
        return np.load(whole)
    parts, k = [], 0
    while os.path.exists(os.path.join(GOLDEN, f"{stem}.part{k}.npz")):
        parts.append(os.path.join(GOLDEN, f"{stem}.part{k}.npz"))
        k += 1
    if not parts:
        raise FileNotFoundError(whole)
    return NpzParts(parts)


def load(name):
    fx = load_npz(name)
    meta = json.loads(str(fx["config"]))
    return fx, meta


def summary(t):
    f = np.asarray(t, np.float64).ravel()
    idx = np.linspace(0, f.size - 1, num=min(64, f.size)).astype(np.int64)
    s = np.zeros(64)
    s[: idx.size] = f[idx]
    return np.concatenate([[f.sum(), (f * f).sum()], s])


def batch(fx, k):
    return O.Batch(*(fx[f"step{k}/in/{x}"] for x in ("s", "a", "r", "s2", "d")))


def eps(fx, k):
    return fx[f"step{k}/in/eps_t"], fx[f"step{k}/in/eps_a"]


def init_state_dicts(name):
    """Initial weights of the 5 nets for a fixture: from the fixture when it holds
    them in full, else re-created with the reference seeding via sac.models."""
    fx, meta = load(name)
    cfg = meta["cfg"]
    out = {}
    if name in FULL_INIT:
        for net in ("policy", "q1", "q2", "q1t", "q2t"):
            out[net] = {k.split("/", 2)[2]: fx[k] for k in fx.files if k.startswith(f"init/{net}/") and "#" not in k}
        return out
    from sac.models import PolicyNetwork, QNetwork

    seed = cfg["train"]["seed"]
    pc, qc = cfg["policy_net"], cfg["q_net"]
    pi = PolicyNetwork(meta["obs"], meta["act"], pc["hidden_sizes"], seed=seed,
                       hidden_activations=pc["hidden_layers_act"])
    q1 = QNetwork(meta["obs"], meta["act"], qc["hidden_sizes"], qc["hidden_layers_act"], seed=seed)
    q2 = QNetwork(meta["obs"], meta["act"], qc["hidden_sizes"], qc["hidden_layers_act"], seed=seed + 1)
    for net, m in (("policy", pi), ("q1", q1), ("q2", q2), ("q1t", q1), ("q2t", q2)):
        out[net] = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    return out


def oracle_state(name):
    fx, meta = load(name)
    cfg = meta["cfg"]
    hp = O.SacHyper.from_config(cfg)
    sds = init_state_dicts(name)
    qa, pa = cfg["q_net"]["hidden_layers_act"], cfg["policy_net"]["hidden_layers_act"]
    qo, po = cfg["q_net"]["output_activation"], cfg["policy_net"]["output_activation"]
    pi = O.MLP.from_state_dict(sds["policy"], pa, po)
    q1 = O.MLP.from_state_dict(sds["q1"], qa, qo)
    q2 = O.MLP.from_state_dict(sds["q2"], qa, qo)
    st = O.SacState.fresh(pi, q1, q2, hp, meta["act"])
    st.q1t = O.MLP.from_state_dict(sds["q1t"], qa, qo)
    st.q2t = O.MLP.from_state_dict(sds["q2t"], qa, qo)
    return st, hp, fx, meta
