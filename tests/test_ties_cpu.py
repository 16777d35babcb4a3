"""tests/_ties.py on the CPU: a constructed tie of a kinked activation (ReLU,
leaky ReLU, SELU; hidden or output layer) is found on the row that holds it,
a smooth activation at 0 is not one, and a tie-free draw leaves no tie on any
pass (the GPU parity tests rely on these to keep the per-element parameter
check on every network)."""
import numpy as np
import pytest

import _ties
from oracle import sac_oracle as O


def _state(obs, act, hidden, seed):
    g = np.random.default_rng(seed)

    def mlp(dims):
        W = [(g.standard_normal((o, i)) * np.sqrt(2.0 / (i + o))).astype(np.float32) for i, o in zip(dims, dims[1:])]
        return O.MLP(W, [np.zeros(o, np.float32) for o in dims[1:]])

    hp = O.SacHyper(alpha=0.1, auto_entropy_tuning=True)
    st = O.SacState.fresh(mlp([obs, *hidden, 2 * act]), mlp([obs + act, *hidden, 1]), mlp([obs + act, *hidden, 1]),
                          hp, act)
    return st, hp


def test_relu_tie_is_found_on_its_row():
    st, _ = _state(5, 2, [16, 16], 0)
    x = np.random.default_rng(1).standard_normal((8, 5)).astype(np.float32)
    assert not _ties.relu_ties(st.pi, x).any()
    # move row 3's first hidden pre-activation of unit 0 to exactly 0
    w = st.pi.W[0][0].astype(np.float64)
    x[3] -= (x[3].astype(np.float64) @ w) / (w @ w) * w
    m = _ties.relu_ties(st.pi, x, rel=1e-6)
    assert m[3] and m.sum() == 1


def _row3_on_the_kink(mlp, x, layer):
    """x with row 3 moved so that unit 0's pre-activation of `layer` (0: first
    hidden layer, -1: the output layer of a net whose layers below it are the
    identity) is 0 up to float64 rounding."""
    w = mlp.W[0][0].astype(np.float64)
    if layer == -1:  # the composite linear map of the whole stack, biases 0
        M = np.eye(x.shape[1])
        for W in mlp.W:
            M = W.astype(np.float64) @ M
        w = M[0]
    x = x.copy()
    x[3] -= (x[3].astype(np.float64) @ w) / (w @ w) * w
    return x


@pytest.mark.parametrize("act", ["leaky_relu", "selu"])
def test_kinked_hidden_activation_tie_is_found_on_its_row(act):
    st, _ = _state(5, 2, [16, 16], 0)
    st.pi.hidden_act = act
    x = np.random.default_rng(1).standard_normal((8, 5)).astype(np.float32)
    assert not _ties.kink_ties(st.pi, x).any()
    m = _ties.kink_ties(st.pi, _row3_on_the_kink(st.pi, x, 0), rel=1e-6)
    assert m[3] and m.sum() == 1


@pytest.mark.parametrize("act", ["elu", "tanh", "gelu", "identity"])
def test_smooth_activation_at_zero_is_no_tie(act):
    """A pre-activation at 0 decides nothing for a smooth activation: not
    flagged, as a hidden or as an output activation."""
    st, _ = _state(5, 2, [16, 16], 0)
    x = np.random.default_rng(1).standard_normal((8, 5)).astype(np.float32)
    st.pi.hidden_act = act
    assert not _ties.kink_ties(st.pi, _row3_on_the_kink(st.pi, x, 0), rel=1e-6).any()
    st.pi.hidden_act, st.pi.out_act = "identity", act
    assert not _ties.kink_ties(st.pi, _row3_on_the_kink(st.pi, x, -1), rel=1e-6).any()


@pytest.mark.parametrize("act", ["relu", "leaky_relu", "selu"])
def test_kinked_output_activation_tie_is_found_on_its_row(act):
    st, _ = _state(5, 2, [16, 16], 0)
    st.pi.hidden_act, st.pi.out_act = "identity", act
    x = np.random.default_rng(1).standard_normal((8, 5)).astype(np.float32)
    assert not _ties.kink_ties(st.pi, x).any()
    m = _ties.kink_ties(st.pi, _row3_on_the_kink(st.pi, x, -1), rel=1e-6)
    assert m[3] and m.sum() == 1
    # behind a smooth hidden activation the output layer is still checked
    st.pi.hidden_act = "tanh"
    assert not _ties.kink_ties(st.pi, x).any()
    st.pi.b[-1][0] = -(st.pi.forward(x)[1][-1][1][3, 0])  # row 3's output pre-activation of unit 0 to ~0 (fp32)
    m = _ties.kink_ties(st.pi, x, rel=1e-6)
    assert m[3] and m.sum() == 1


def test_step_ties_names_the_pass_of_an_output_kink():
    """step_ties flags a kinked critic output activation on the critic pass."""
    st, hp = _state(5, 2, [16, 16], 0)
    for q in (st.q1, st.q2, st.q1t, st.q2t):
        q.out_act = "leaky_relu"
    g = np.random.default_rng(4)
    B = 8
    bt = O.Batch(g.standard_normal((B, 5)).astype(np.float32), g.uniform(-1, 1, (B, 2)).astype(np.float32),
                 g.standard_normal(B).astype(np.float32), g.standard_normal((B, 5)).astype(np.float32),
                 np.zeros(B, np.float32))
    et, ea = g.standard_normal((2, B, 2)).astype(np.float32)
    assert not _ties.step_ties(st, hp, bt, et, ea)[0]
    p = st.q1.forward(np.concatenate([bt.s, bt.a], 1))[1][-1][1]
    st.q1.b[-1][0] = -p[5, 0]
    ties = _ties.step_ties(st, hp, bt, et, ea, rel=1e-6)[0]
    assert set(ties) == {"q1(s,a)"} and ties["q1(s,a)"][5] and ties["q1(s,a)"].sum() == 1


@pytest.mark.parametrize("edge", ["lo", "hi"])
def test_log_sigma_on_a_clamp_edge_is_found_on_its_row(edge):
    """A raw log sigma moved onto an edge of a narrow clamp is flagged on its
    row, by clamp_ties and as step_ties' "clamp(s)"; at a distance of 1e-3
    from the edge it is not."""
    st, hp = _state(5, 2, [16, 16], 0)
    lo, hi = -0.1, 0.1
    hp.policy = O.PolicyCfg(lo, hi, 1.0)
    g = np.random.default_rng(4)
    B = 8
    bt = O.Batch(g.standard_normal((B, 5)).astype(np.float32), g.uniform(-1, 1, (B, 2)).astype(np.float32),
                 g.standard_normal(B).astype(np.float32), g.standard_normal((B, 5)).astype(np.float32),
                 np.zeros(B, np.float32))
    et, ea = g.standard_normal((2, B, 2)).astype(np.float32)
    assert not _ties.clamp_ties(st.pi, bt.s, lo, hi).any()
    assert "clamp(s)" not in _ties.step_ties(st, hp, bt, et, ea)[0]
    e = lo if edge == "lo" else hi
    raw = st.pi.forward(bt.s)[0][:, 2:]  # log sigma of unit 0 is output 2 (act = 2)
    b0 = st.pi.b[-1][2]
    st.pi.b[-1][2] = b0 + np.float32(e) - raw[5, 0]  # row 5's log sigma of unit 0 onto the edge (fp32 rounding)
    m = _ties.clamp_ties(st.pi, bt.s, lo, hi, rel=1e-6)
    assert m[5] and m.sum() == 1
    ties = _ties.step_ties(st, hp, bt, et, ea, rel=1e-6)[0]
    assert ties["clamp(s)"][5] and ties["clamp(s)"].sum() == 1
    for off in (1e-3, -1e-3):
        st.pi.b[-1][2] = b0 + np.float32(e + off) - raw[5, 0]
        assert not _ties.clamp_ties(st.pi, bt.s, lo, hi, rel=1e-6).any()
        assert "clamp(s)" not in _ties.step_ties(st, hp, bt, et, ea, rel=1e-6)[0]


def test_tie_free_draw_redraws_a_clamp_edge_row():
    """tie_free_draw replaces a row whose log sigma sits on a clamp edge."""
    obs, act, B, n = 5, 2, 8, 64
    st, hp = _state(obs, act, [16, 16], 0)
    hp.policy = O.PolicyCfg(-0.1, 0.1, 1.0)
    g = np.random.default_rng(3)
    s = g.standard_normal((n + 1, obs)).astype(np.float32)
    rows = dict(obs=s[:n], next_obs=s[1:], act=g.uniform(-1, 1, (n, act)).astype(np.float32),
                rew=g.standard_normal(n).astype(np.float32), done=(g.random(n) < 0.3).astype(np.float32))
    idx0 = np.random.default_rng(5).choice(n, size=B, replace=False)  # the draw tie_free_draw makes first
    raw = st.pi.forward(rows["obs"][idx0])[0][:, act:]
    st.pi.b[-1][act] += np.float32(0.1) - raw[2, 0]
    idx, et, ea, bt, outs, redrawn, seen = _ties.tie_free_draw(np.random.default_rng(5), rows, n, B, act, hp, [st],
                                                               rel=1e-6)
    assert seen.get("clamp(s)") == 1 and redrawn >= 1 and idx[2] != idx0[2]
    assert not _ties.step_ties(st, hp, bt, et, ea, rel=1e-6)[0]


def test_tie_free_draw_leaves_no_tie():
    obs, act, B, n = 6, 2, 512, 2048
    st, hp = _state(obs, act, [64, 64], 2)
    g = np.random.default_rng(3)
    s = g.standard_normal((n + 1, obs)).astype(np.float32)
    rows = dict(obs=s[:n], next_obs=s[1:], act=g.uniform(-1, 1, (n, act)).astype(np.float32),
                rew=g.standard_normal(n).astype(np.float32), done=(g.random(n) < 0.01).astype(np.float32))
    # a loose threshold so that ties do occur at this size
    rel = 1e-4
    idx, et, ea, bt, outs, redrawn, seen = _ties.tie_free_draw(g, rows, n, B, act, hp, [st], rel=rel)
    assert redrawn > 0 and seen
    assert len(set(idx.tolist())) == B
    ties, ref, _ = _ties.step_ties(st, hp, bt, et, ea, rel=rel)
    assert not ties
    np.testing.assert_array_equal(ref["y"], outs[0][0]["y"])
