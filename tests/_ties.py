"""Summation-order ties of one SAC step, and tie-free batch draws for the
fp32 parity checks (test infrastructure; the oracle is the checker).

A "tie" is a decision of the step that fp32 summation order can flip between
two correct implementations (the numpy oracle and the MFMA kernels):

* a pre-activation p of a kinked activation (ReLU, leaky ReLU, SELU; hidden
  layers and a kinked output activation) with |p| <= rel * (|W| |x| + |b|) on a pass
  whose backward runs (pi on s, the critics on (s, a) and, with the UPDATED
  critics, on (s, a~)): the unit's mask for that row, and so a rank-one term
  of every lower layer's dW, follows the sign the sum happened to take
  (profiles/r04_debug_wide512_relu_tie.txt);
* the same on the forward-only passes (pi on s', the targets on (s', a')),
  where the flipped unit moves y by ~|p| only, checked all the same;
* a min-Q near-tie of the actor pass, |q1 - q2| <= rel * (|q1| + |q2|): the
  min's backward routes the row's gradient to the other critic;
* a raw log sigma of pi(s), the pass whose backward runs, within
  rel * (|W| |x| + |b|) of an edge of the clamp: the clamp's backward keeps or
  zeroes that entry's gradient (a narrow clamp puts many entries near an edge;
  at the default [-20, 2] none is).

Reference: /root/reference/sac/agent.py:195-260 (the passes), sac/models.py:
104-149 (the activation stacks).  The parity tests draw each step's indices and eps
until no tie is found, so the per-element parameter check (>= 99.5% within
1e-6) runs on every network at every shape instead of being voided."""
import copy

import numpy as np

from oracle import sac_oracle as O

REL = 1e-7


KINKED = ("relu", "leaky_relu", "selu")  # derivative jump at 0: 1 | 0, 1 | 0.01, 1.0507 | 1.7581


def _act64(name, p):
    """The activation in float64 (oracle.sac_oracle.act_fwd rounds to fp32)."""
    if name == "identity":
        return p
    if name == "relu":
        return np.maximum(p, 0.0)
    if name == "tanh":
        return np.tanh(p)
    if name == "elu":
        return np.where(p > 0, p, np.expm1(np.minimum(p, 0.0)))
    if name == "leaky_relu":
        return np.where(p > 0, p, 0.01 * p)
    if name == "gelu":
        from scipy.special import erf

        return p * 0.5 * (1.0 + erf(p / np.sqrt(2.0)))
    if name == "selu":
        return float(O._SELU_SCALE) * np.where(p > 0, p, float(O._SELU_ALPHA) * np.expm1(np.minimum(p, 0.0)))
    raise KeyError(name)


def kink_ties(mlp, x, rel=REL):
    """Rows of this forward with a pre-activation of a kinked activation (ReLU,
    leaky ReLU, SELU: hidden layers, and the output layer when the net's output
    activation is one of them) within fp32 summation-order noise of 0 (float64
    evaluation, each layer propagated with its own activation), as a boolean
    mask.  The smooth activations (ELU, tanh, GELU, identity) have no such
    decision: a pre-activation at 0 moves their derivative by ~|p| only."""
    h = np.asarray(x, np.float64)
    rows = np.zeros(h.shape[0], bool)
    n = len(mlp.W)
    if mlp.hidden_act not in KINKED and mlp.out_act not in KINKED:
        return rows
    for i in range(n):
        act = mlp.hidden_act if i < n - 1 else mlp.out_act
        if i == n - 1 and act not in KINKED:
            break
        W, b = mlp.W[i].astype(np.float64), mlp.b[i].astype(np.float64)
        p = h @ W.T + b
        if act in KINKED:
            rows |= np.any(np.abs(p) <= rel * (np.abs(h) @ np.abs(W).T + np.abs(b)), axis=1)
        h = _act64(act, p)
    return rows


def clamp_ties(mlp, x, lo, hi, rel=REL):
    """Rows of the policy's forward with a raw log sigma output (the second
    half of the net's output, before the clamp) within fp32 summation-order
    noise of a clamp edge, as a boolean mask: the clamp's backward passes the
    entry's gradient inside [lo, hi] and zeroes it outside, so the side the sum
    happened to take decides a whole row of the last layer's dW.  float64
    evaluation; the noise of the last layer's sum is rel * (|W| |x| + |b|), and
    an output activation passes it on with a slope of at most 1.76 (SELU),
    taken as 2."""
    h = np.asarray(x, np.float64)
    n = len(mlp.W)
    for i in range(n):
        W, b = mlp.W[i].astype(np.float64), mlp.b[i].astype(np.float64)
        p = h @ W.T + b
        if i == n - 1:
            noise = rel * (np.abs(h) @ np.abs(W).T + np.abs(b))
            if mlp.out_act != "identity":
                noise = 2.0 * noise
            A = p.shape[1] // 2
            ls, noise = _act64(mlp.out_act, p)[:, A:], noise[:, A:]
            return np.any((np.abs(ls - float(lo)) <= noise) | (np.abs(ls - float(hi)) <= noise), axis=1)
        h = _act64(mlp.hidden_act, p)


relu_ties = kink_ties  # the name from when ReLU was the only kinked activation modelled


def step_ties(st, hp, bt, et, ea, rel=REL):
    """Ties of one oracle training step from state `st` (not mutated) on batch
    `bt` with eps (et, ea).  Returns (ties: dict pass -> boolean row mask, for
    the passes with a tie; the oracle's step result; the post-step state).  The
    post-step state is the oracle reference for a one-step parameter comparison
    from `st`."""
    ties = {}
    s = np.asarray(bt.s, np.float32)
    s2 = np.asarray(bt.s2, np.float32)
    a = np.asarray(bt.a, np.float32)
    pc = hp.policy
    ties["pi(s')"] = relu_ties(st.pi, s2, rel)
    ties["pi(s)"] = relu_ties(st.pi, s, rel)
    ties["clamp(s)"] = clamp_ties(st.pi, s, pc.log_std_min, pc.log_std_max, rel)
    a2, _, _ = O.policy_sample(st.pi, s2, et, pc)
    at, _, _ = O.policy_sample(st.pi, s, ea, pc)
    sa2 = np.concatenate([s2, a2], 1)
    ties["q1t(s',a')"] = relu_ties(st.q1t, sa2, rel)
    ties["q2t(s',a')"] = relu_ties(st.q2t, sa2, rel)
    sa = np.concatenate([s, a], 1)
    ties["q1(s,a)"] = relu_ties(st.q1, sa, rel)
    ties["q2(s,a)"] = relu_ties(st.q2, sa, rel)
    post = copy.deepcopy(st)
    ref = O.training_step(post, hp, bt, et, ea)
    # the actor pass runs the UPDATED critics on (s, a~); post.q1 / q2 are
    # those (the actor, alpha and Polyak updates leave the critics as they are)
    sat = np.concatenate([s, at], 1)
    ties["q1(s,a~)"] = relu_ties(post.q1, sat, rel)
    ties["q2(s,a~)"] = relu_ties(post.q2, sat, rel)
    q1v = O.q_forward(post.q1, s, at)[0].astype(np.float64)
    q2v = O.q_forward(post.q2, s, at)[0].astype(np.float64)
    ties["minQ(s,a~)"] = np.abs(q1v - q2v) <= 20 * rel * (np.abs(q1v) + np.abs(q2v)) + 1e-9
    return {k: v for k, v in ties.items() if v.any()}, ref, post


# passes whose ties depend on the row's eps_a alone (a~ = pi(s) sampled with it)
# and on the critics' update, which does not read eps_a: such a row is fixed by
# a fresh eps_a, which leaves every other row's ties as they were
ACTOR_PASSES = ("q1(s,a~)", "q2(s,a~)", "minQ(s,a~)")


def tie_free_draw(g, rows, n_rows, B, A, hp, states, max_rounds=64, rel=REL):
    """Draw B distinct indices and eps (et, ea) from rng `g`, then redraw the
    rows of any tie until the step has no tie from any state in `states`
    (oracle trajectories and/or the engine's own state).  A tie is a (row,
    unit) event (~1 per pass per step at B = 4096), so whole-batch redraws
    would never end.  A row tied on a pass before the actor's gets a fresh
    unused index and fresh eps (this moves the critics' update, so a later
    round can show a new actor-pass tie elsewhere); a row tied on the actor
    pass only (the updated critics on (s, a~), the min-Q) gets a fresh eps_a,
    which the critics' update does not read.  Returns (idx, et, ea, batch,
    [(ref, post) per state], rows redrawn, ties seen: pass -> count)."""
    idx = g.choice(n_rows, size=B, replace=False).astype(np.int32)
    et = g.standard_normal((B, A)).astype(np.float32)
    ea = g.standard_normal((B, A)).astype(np.float32)
    seen, redrawn = {}, 0
    for _ in range(max_rounds):
        bt = O.Batch(rows["obs"][idx], rows["act"][idx], rows["rew"][idx], rows["next_obs"][idx], rows["done"][idx])
        outs, row_tied, actor_tied = [], np.zeros(B, bool), np.zeros(B, bool)
        for st in states:
            ties, ref, post = step_ties(st, hp, bt, et, ea, rel)
            for k, m in ties.items():
                seen[k] = seen.get(k, 0) + int(m.sum())
                if k in ACTOR_PASSES:
                    actor_tied |= m
                else:
                    row_tied |= m
            outs.append((ref, post))
        if not (row_tied.any() or actor_tied.any()):
            return idx, et, ea, bt, outs, redrawn, seen
        r = np.flatnonzero(row_tied)
        if r.size:
            free = np.setdiff1d(np.arange(n_rows, dtype=np.int32), idx)
            idx = idx.copy()
            idx[r] = g.choice(free, size=r.size, replace=False).astype(np.int32)
            et[r] = g.standard_normal((r.size, A)).astype(np.float32)
        ra = np.flatnonzero(row_tied | actor_tied)
        ea[ra] = g.standard_normal((ra.size, A)).astype(np.float32)
        redrawn += int(ra.size)
    raise AssertionError(f"ties remain after {max_rounds} rounds of row redraws (ties seen: {seen})")
