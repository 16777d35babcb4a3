"""The inputs of tests/test_gpu_widths.py on the CPU oracle alone (no GPU).

Every layer must be visible (tests/test_depth_cpu.py's condition and share):
for every case and each of its hyper-parameter sets, step 1 drawn as the GPU
test draws it (rng 11, tie-free from the fresh state), at least half of the
elements of each weight matrix of pi, Q1 and Q2 must move by more than 1e-6.

Every hidden edge must be visible: for each hidden layer l of width N, the
last unit's row W_l[N - 1, :], its bias b_l[N - 1] and the column that reads
it, W_{l+1}[:, N - 1] (tests/_widths.py::edge_slices, which adds layer 0's
last input column), must each move in at least half of their elements, and a
hidden layer of one unit in all of them.  A dropped or misplaced last unit
then shows in the post-step parameters that the GPU test's edge hook bounds
element by element.

The conditions are on the inputs: on a miss change the shape's activation or
seed, never the share.

The device-RNG cases cannot redraw a tie, so the oracle's six steps on the
device RNG's draws must be tie-free from the fresh state at the engine seed
the GPU test uses."""
import numpy as np
import pytest

import _ties
import _widths
from _gpu import config_rows, oracle_fresh_state, synthetic_rows

MOVE, SHARE = 1e-6, 0.5
PAIRS = [(case, hset) for case in sorted(_widths.CASES) for hset in _widths.hsets(case)]


def _rows(c, seed=3):
    if c.get("done_p") is None:  # bench.synthetic_replay's rows: 1 % terminals
        return synthetic_rows(c["capacity"], c["obs"], c["act"], seed, 0.01)
    return config_rows(c, seed)


_first = {}


def _first_step(shape, hset):
    """(the fresh state, the oracle's state after step 1, rows redrawn) of a
    shape and set; the cases of one shape share their inputs."""
    if (shape, hset) not in _first:
        case = next(k for k in sorted(_widths.CASES) if _widths.SHAPE_OF[k] == shape)
        c = _widths.config(case, hset)
        st, hp = oracle_fresh_state(c)
        g = np.random.default_rng(11)
        # the engine's pre-step state is the fresh state on step 1: the trajectory and the local oracle coincide
        _, _, _, _, outs, redrawn, _ = _ties.tie_free_draw(g, _rows(c), c["capacity"], c["batch"], c["act"], hp,
                                                           [st, st])
        _first[shape, hset] = (dict(c, name=shape + ("" if hset == "default" else "_" + hset)), st, outs[0][1], redrawn)
    return _first[shape, hset]


def _moved(a0, a1):
    return np.abs(np.asarray(a1, np.float64) - np.asarray(a0, np.float64)) > MOVE


def test_the_matrix_is_the_issues():
    assert len(_widths.CASES) == 32 and set(_widths.SHAPE_OF.values()) == set(_widths.SHAPES)
    assert [c for c in sorted(_widths.CASES) if _widths.hsets(c) != _widths.HSETS] == ["obs1_pairs", "obs1_roles"]
    # no hidden width of the matrix is a multiple of 8: the widths are what the suite lacked
    widths = {w for s in _widths.SHAPES.values() for k in ("hidden", "q_hidden", "pi_hidden") for w in s.get(k, [])}
    assert widths == {1, 7, 17, 31, 33, 50, 65, 100, 257, 299, 401}


@pytest.mark.parametrize("case,hset", PAIRS)
def test_every_layer_moves_on_the_oracles_first_step(case, hset):
    c, st, post, redrawn = _first_step(_widths.SHAPE_OF[case], hset)
    shares = {}
    for name in ("pi", "q1", "q2"):
        before, after = getattr(st, name), getattr(post, name)
        assert len(before.W) == len(c.get(f"{'pi' if name == 'pi' else 'q'}_hidden", c.get("hidden"))) + 1
        for l, (w0, w1) in enumerate(zip(before.W, after.W)):
            shares[name, l] = float(np.mean(_moved(w0, w1)))
    print(f"[visible] {c['name']}: {redrawn} rows redrawn, lowest share {min(shares.values()):.3f} at "
          f"{min(shares, key=shares.get)}")
    low = {k: v for k, v in shares.items() if v < SHARE}
    assert not low, (c["name"], low)


@pytest.mark.parametrize("case,hset", PAIRS)
def test_every_hidden_edge_moves_on_the_oracles_first_step(case, hset):
    c, st, post, _ = _first_step(_widths.SHAPE_OF[case], hset)
    shares, low = {}, {}
    for name in ("pi", "q1", "q2"):
        before, after = getattr(st, name), getattr(post, name)
        for label, kind, l, ix, width in _widths.edge_slices(before.W, before.b)[1:]:  # the hidden layers' slices
            m = _moved(getattr(before, kind)[l][ix], getattr(after, kind)[l][ix])
            assert m.size >= 1
            shares[name, label] = float(np.mean(m))
            need = 1.0 if width == 1 else SHARE  # a layer of one unit: its row, bias and column move whole
            if shares[name, label] < need:
                low[name, label] = (shares[name, label], need)
    print(f"[edge-visible] {c['name']}: lowest share of an edge slice {min(shares.values()):.3f} at "
          f"{min(shares, key=shares.get)}")
    assert not low, (c["name"], low)


@pytest.mark.parametrize("shape", sorted(s for s in _widths.SHAPES if s not in _widths.DEFAULT_ONLY))
def test_the_rl_adam_steps_meet_the_conditions_on_their_inputs(shape):
    """test_gpu_hyper.py::_conditions on the oracle's own trajectory, the steps
    drawn as the GPU test draws them: every step's batch holds >= 4 terminal
    and >= 4 non-terminal rows, and >= 5 % of the raw log sigma entries lie
    below the narrow clamp, above it and inside it.  The cases of one shape
    share their inputs, so one walk per shape."""
    from test_gpu_hyper import _conditions

    case = next(k for k in sorted(_widths.CASES) if _widths.SHAPE_OF[k] == shape)
    c = _widths.config(case, "rl+adam")
    st, hp = oracle_fresh_state(c)
    B, A = c["batch"], c["act"]
    g = np.random.default_rng(11)
    check = _conditions(f"{shape}_rl+adam/oracle", True)
    for k in range(1, _widths.steps(c) + 1):
        _, _, _, bt, outs, _, _ = _ties.tie_free_draw(g, _rows(c), c["capacity"], B, A, hp, [st, st])
        check(k, hp, bt, st.pi, None, None)
        st = outs[0][1]


def _eps_bound_tensors(c):
    """The default-set steps of config c on the oracle's own trajectory, drawn
    as the GPU test draws them: [(step, net, tensor index, elements, sqrt(v^) /
    eps of the flagged ones)] for every tensor in which more than 0.1 % of the
    elements have 0 < sqrt(v^) < 10 adam_eps."""
    st, hp = oracle_fresh_state(c)
    g = np.random.default_rng(11)
    out = []
    for k in range(1, _widths.steps(c) + 1):
        _, _, _, _, outs, _, _ = _ties.tie_free_draw(g, _rows(c), c["capacity"], c["batch"], c["act"], hp, [st, st])
        st = outs[0][1]
        for n, opt in (("pi", st.opt_pi), ("q1", st.opt_q1), ("q2", st.opt_q2)):
            assert opt.step == k
            for i, v in enumerate(opt.v):
                r = np.sqrt(v.astype(np.float64) / (1.0 - hp.beta2 ** k)) / hp.adam_eps
                f = (r > 0) & (r < 10.0)
                if f.mean() > 1e-3:
                    out.append((k, n, i, v.size, np.round(np.sort(r[f]), 2).tolist()))
    return out


@pytest.mark.parametrize("shape", sorted(_widths.SHAPES))
def test_no_tensor_is_voided_by_gradients_within_adam_eps_of_zero(shape):
    """The default set has adam_eps = 1e-8.  An element with 0 < sqrt(v^) <
    10 eps takes an update that the summation order of its gradient decides
    (the update's slope in g is lr eps / (|g| + eps)^2 >= 2.5e2 there, so
    noise of 4e-9 in g moves it by 1e-6), on any correct fp32 implementation.
    _check_config_against_oracle allows 0.1 % of a tensor's elements to miss
    1e-6 against the local oracle, so no tensor of the oracle's own steps may
    hold more than 0.1 % of such elements: below 1000 elements, none.  On a
    miss the shape's default set gets another replay seed
    (tests/_widths.py::REPLAY_SEED), the smallest of 4.. that meets this."""
    case = next(k for k in sorted(_widths.CASES) if _widths.SHAPE_OF[k] == shape)
    c = _widths.config(case, "default")
    assert not _eps_bound_tensors(c), (shape, c.get("replay_seed", 3))
    if (shape, "default") in _widths.REPLAY_SEED:  # a reseeded shape misses it at build_engine's 3 and up to its own
        assert c["done_p"] == 0.01
        for seed in range(3, c["replay_seed"]):
            assert _eps_bound_tensors(dict(c, replay_seed=seed)), (shape, seed)
    else:
        assert "done_p" not in c and "replay_seed" not in c


@pytest.mark.parametrize("shape", ["odd", "tiny", "w257"])
def test_device_rng_draws_are_tie_free_at_the_gpu_tests_seed(shape):
    """The role, row-tile, pair-tile and stage cases of one shape share their
    seed and rows: one walk per shape."""
    from test_gpu_action_width import oracle_walk

    assert {_widths.SHAPE_OF[k] for k in _widths.RNG_CASES} == {"odd", "tiny", "w257"}
    c = dict(_widths.RNG_SHAPES[shape], done_p=0.01)
    st, hp = oracle_fresh_state(c, _widths.RNG_SEED)
    rows = _rows(c, _widths.RNG_SEED)
    walk = oracle_walk(st, hp, rows, c["capacity"], c["batch"], c["act"], _widths.RNG_SEED, 0, 6)
    ties = [t for t, _, _ in walk]
    assert not any(ties), (shape, _widths.RNG_SEED, ties)
    if shape == "tiny":  # why ELU here: with ReLU the zero biases behind the one-unit layer tie step 0 at any seed
        assert c["pi_act"] == c["q_act"] == "elu" and "pi_act" not in _widths.SHAPES["tiny"]
        for seed in range(4):
            relu = dict(_widths.SHAPES["tiny"], done_p=0.01)
            st, hp = oracle_fresh_state(relu, seed)
            cap, B, A = relu["capacity"], relu["batch"], relu["act"]
            tied = oracle_walk(st, hp, _rows(relu, seed), cap, B, A, seed, 0, 1)[0][0]
            assert tied.get("pi(s)", 0) >= 10 and tied.get("pi(s')", 0) >= 10, (seed, tied)



def _bf16_emulation_misses(c, steps=3):
    """Three steps with bf16 products (tests/_bf16_emulation.py) on the
    emulation's own trajectory from the fresh state, on the rows
    test_gpu_parity.py::_bf16_one_step_from_the_engine_state draws (rng 13),
    each measured against the fp32 oracle's step from the same state exactly
    as that function measures the engine.  Returns the standing bounds the
    emulation misses: [(step, what, the figures)]."""
    import copy

    import _bf16_emulation as EM
    from oracle import sac_oracle as O

    st, hp = oracle_fresh_state(c)
    rows, B, A = _rows(c), c["batch"], c["act"]
    f = max(1.0, (256 / B) ** 0.5)
    g = np.random.default_rng(13)
    lrs = {"pi": hp.actor_lr, "q1": hp.critic_lr, "q2": hp.critic_lr, "q1t": hp.critic_lr * hp.tau,
           "q2t": hp.critic_lr * hp.tau}
    missed = []
    for k in range(1, steps + 1):
        idx = g.choice(c["capacity"], size=B, replace=False).astype(np.int32)
        et = g.standard_normal((B, A)).astype(np.float32)
        ea = g.standard_normal((B, A)).astype(np.float32)
        bt = O.Batch(rows["obs"][idx], rows["act"][idx], rows["rew"][idx], rows["next_obs"][idx], rows["done"][idx])
        emu, post = EM.step(st, hp, bt, et, ea)
        assert O.MLP.forward.__module__ == O.__name__ and O.MLP.backward.__module__ == O.__name__
        ref_post = copy.deepcopy(st)
        ref = O.training_step(ref_post, hp, bt, et, ea)
        for nm, (p99, mx) in (("y", (8e-3 * f, 1.5e-2 * f)), ("log_pi", (3e-2 * f, 6e-2 * f))):
            r = np.abs(emu[nm] - ref[nm]) / (np.abs(ref[nm]) + 1.0)
            if not (np.quantile(r, 0.99) <= p99 and r.max() <= mx):
                missed.append((k, nm, float(np.quantile(r, 0.99)), float(r.max())))
        for n, lr in lrs.items():
            d = np.concatenate([np.abs(a - b).ravel() for a, b in zip(getattr(post, n).params(),
                                                                      getattr(ref_post, n).params())]) / lr
            assert d.max() <= 2.02, (k, n, d.max())
            if k == 1:
                ok = np.mean(d <= 0.01 * f) >= 1.0 - 0.015 * f
            else:
                ok = np.mean(d <= 0.05 * f) >= 0.92 and np.mean(d <= 0.25 * f) >= 0.985 and np.median(d) <= 0.02 * f
            if not ok:
                missed.append((k, n, round(float(np.mean(d <= 0.01 * f)), 4), round(float(np.mean(d <= 0.05 * f)), 4),
                               round(float(np.mean(d <= 0.25 * f)), 4), float(np.median(d))))
        st = post
    return missed


@pytest.mark.parametrize("shape", sorted(_widths.SHAPES))
def test_bf16_products_alone_miss_a_standing_bound_at_odd3_only(shape):
    """Why tests/test_gpu_widths.py::BF16_EMULATED names the odd3 cases and no
    other: no engine involved, the emulation misses a standing bound of
    _bf16_one_step_from_the_engine_state at that shape alone (step 2: Q2 and
    its target 0.8931 within 0.05 f lr, 0.92 asked; 0.9840 within 0.25 f lr,
    0.985 asked).  tiny, at 68 .. 79 parameters per network, meets them all."""
    from test_gpu_widths import BF16_EMULATED

    missed = _bf16_emulation_misses(dict(_widths.SHAPES[shape]))
    print(f"[bf16-emu] {shape}: standing bounds the emulation misses on steps 1..3: {missed}")
    assert BF16_EMULATED == {k for k in _widths.CASES if _widths.SHAPE_OF[k] == "odd3"}
    assert bool(missed) == (shape == "odd3"), (shape, missed)
    if shape == "odd3":
        assert {(k, n) for k, n, *_ in missed} == {(2, "q2"), (2, "q2t")}, missed
