"""Dead hidden units for the ReLU masks of the dX epilogues (test
infrastructure; csrc/sac_split.h, gemm_hf's masked form).

A unit n of hidden layer l is dead when row n of W_l and b_l[n] are exactly
zero: its pre-activation is +0.0 in every row of every pass, relu'(+0) = 0
masks its dY, so the row and the bias get a zero gradient, their Adam moments
stay zero and the update adds 0: the unit is dead for good.  Its column of the
NEXT layer's W is left as initialised, so dX at the unit (dY W[:, n]) is not
zero before the mask: a mask that is read wrong shows as a bias that moved.

A spec names, for pi, q1 and q2 alike, the dead units of layers 0 and 1 and
optionally a constant for layer 1's biases and for each critic's output bias
(used where a whole layer is dead: see CASES).  The target critics are copies
of the critics, so they inherit all of it.
"""
import contextlib

import numpy as np

H = 256
# every 16-column tile has one dead unit (tile t: column (5 t + 3) % 16), plus
# the first and last column of a tile (0, 15, 16, 255) and one whole tile (6)
DEAD = sorted({0, 15, 16, 255} | set(range(96, 112)) | {16 * t + (5 * t + 3) % 16 for t in range(H // 16)})
ALL = list(range(H))
# distinct output biases of the critics: with a whole hidden layer dead both
# critics would otherwise be the same constant and every row a min-Q tie
Q_OUT_BIAS = {"q1": 0.25, "q2": -0.5}


def _shape(obs, act, batch, **extra):
    return dict(obs=obs, act=act, hidden=[H, H], batch=batch, capacity=1024, **extra)


def spec(l0=(), l1=(), b1=None, q_out_bias=None):
    return dict(l0=sorted(l0), l1=sorted(l1), b1=b1, q_out_bias=q_out_bias)


# name -> (config dict, spec).  Batch 20: one full row tile and one with 4 valid rows.
CASES = {
    # dead units in every tile of both hidden layers of pi, q1 and q2
    "dead_units": (_shape(24, 4, 20), spec(DEAD, DEAD)),
    # all of layer 0 dead.  Layer 1 then sees h0 = 0, so its biases are set to 0.1: its units are live
    # and dY1 W1 is not zero where layer 0's mask has to zero it
    "dead_layer0": (_shape(24, 4, 20), spec(ALL, (), b1=0.1, q_out_bias=Q_OUT_BIAS)),
    # all of layer 1 dead (layer 0: the set): pi's layer-2 dX masks every column
    "dead_layer1": (_shape(24, 4, 20), spec(DEAD, ALL, q_out_bias=Q_OUT_BIAS)),
    # Kp0 = 64 and 2A = 16: one full fp32 chunk of dOut
    "dead_units_kp64_act8": (_shape(40, 8, 20), spec(DEAD, DEAD)),
    # 2A = 24: pi's layer-2 dX over two fp32 chunks of dOut; the set plus all of columns [16, 32)
    "dead_units_act12": (_shape(11, 12, 20), spec(DEAD, set(DEAD) | set(range(16, 32)))),
}


def kill(nets, sp):
    """Apply a spec to (pi, q1, q2) torch modules in place."""
    import torch

    with torch.no_grad():
        for name, net in zip(("pi", "q1", "q2"), nets):
            lin = net.linears()
            for layer, units in ((0, sp["l0"]), (1, sp["l1"])):
                if units:
                    lin[layer].weight[units] = 0.0
                    lin[layer].bias[units] = 0.0
            if sp["b1"] is not None:
                lin[1].bias.fill_(sp["b1"])
            if sp["q_out_bias"] and name in sp["q_out_bias"]:
                lin[2].bias.fill_(sp["q_out_bias"][name])
    return nets


def kink_ties_skip_exact_zeros(mlp, x, rel=None):
    """tests/_ties.py::kink_ties, except that a pre-activation whose error
    bound rel (|W| |x| + |b|) is itself 0 is no tie: every term of its sum is
    exactly 0, so it is +0.0 in any summation order (a dead unit, or any unit
    behind a dead layer with a zero bias)."""
    import _ties

    rel = _ties.REL if rel is None else rel
    h = np.asarray(x, np.float64)
    rows = np.zeros(h.shape[0], bool)
    n = len(mlp.W)
    if mlp.hidden_act not in _ties.KINKED and mlp.out_act not in _ties.KINKED:
        return rows
    for i in range(n):
        act = mlp.hidden_act if i < n - 1 else mlp.out_act
        if i == n - 1 and act not in _ties.KINKED:
            break
        W, b = mlp.W[i].astype(np.float64), mlp.b[i].astype(np.float64)
        p = h @ W.T + b
        if act in _ties.KINKED:
            bound = np.abs(h) @ np.abs(W).T + np.abs(b)
            rows |= np.any((np.abs(p) <= rel * bound) & (bound > 0), axis=1)
        h = _ties._act64(act, p)
    return rows


@contextlib.contextmanager
def dead_nets(sp):
    """While active, tests/_gpu.py::torch_nets (what build_engine and
    oracle_fresh_state start from) returns nets with the spec applied, and the
    tie-free draws do not count a dead unit's exact zero as a tie."""
    import _gpu
    import _ties

    orig_nets, orig_ties = _gpu.torch_nets, _ties.relu_ties

    def torch_nets(c, seed=3):
        return kill(orig_nets(c, seed), sp)

    _gpu.torch_nets, _ties.relu_ties = torch_nets, kink_ties_skip_exact_zeros
    try:
        yield
    finally:
        _gpu.torch_nets, _ties.relu_ties = orig_nets, orig_ties


def dead_rows(sp):
    """[(layer, units)] with any dead unit."""
    return [(layer, units) for layer, units in ((0, sp["l0"]), (1, sp["l1"])) if units]


def assert_oracle_rows_zero(st, sp, where):
    """The dead rows of W and b, and of Adam's m and v, of the oracle state's pi, q1, q2 (and the
    targets' W and b) are exactly zero."""
    for name, net, opt in (("pi", st.pi, st.opt_pi), ("q1", st.q1, st.opt_q1), ("q2", st.q2, st.opt_q2),
                           ("q1t", st.q1t, None), ("q2t", st.q2t, None)):
        for layer, units in dead_rows(sp):
            arrays = [("W", net.W[layer]), ("b", net.b[layer])]
            if opt is not None:
                arrays += [("m_W", opt.m[2 * layer]), ("m_b", opt.m[2 * layer + 1]),
                           ("v_W", opt.v[2 * layer]), ("v_b", opt.v[2 * layer + 1])]
            for an, a in arrays:
                assert not np.any(a[units]), (where, name, layer, an, np.flatnonzero(np.any(a[units].reshape(len(units), -1), 1)))


def assert_engine_rows_zero(eng, sp, where):
    """The same of the engine: the networks' parameters and the flat Adam moments viewed layer by layer."""
    from sac.engine import _views

    for name, net in eng.nets.items():
        like = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
        groups = [("", like)]
        if name in eng.m:
            groups += [("m_", _views(eng.m[name], like)), ("v_", _views(eng.v[name], like))]
        for layer, units in dead_rows(sp):
            for prefix, ts in groups:
                for an, t in (("W", ts[2 * layer]), ("b", ts[2 * layer + 1])):
                    a = t.detach().cpu().numpy()[units].reshape(len(units), -1)
                    assert not np.any(a), (where, name, layer, prefix + an, np.flatnonzero(np.any(a, 1)))
