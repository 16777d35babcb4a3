"""The inputs of tests/test_gpu_depth.py on the CPU oracle alone (no GPU).

Every layer must be visible: the GPU tests bound post-step parameters element
by element at 1e-6, so a layer whose dW the kernels dropped, or left from the
step before, shows only where the oracle's own step moves that layer's
elements by more than 1e-6.  For every case and both hyper-parameter sets,
step 1 drawn as the GPU test draws it (rng 11, tie-free from the fresh
state), at least half of the elements of each weight matrix of pi, Q1 and Q2
must move by more than 1e-6.  Measured: 0.73 (pi's fifth layer at h5 with
rl+adam) to 1.0; layer 0 is 1.0 everywhere.  The condition is on the inputs:
on a miss change the shape's widths or seed, never the share.

The device-RNG cases cannot redraw a tie, so the oracle's six steps on the
device RNG's draws must be tie-free from the fresh state at the engine seed
the GPU test uses."""
import numpy as np
import pytest

import _depth
import _ties
from _gpu import config_rows, oracle_fresh_state, synthetic_rows

MOVE, SHARE = 1e-6, 0.5


def _rows(c, seed=3):
    if c.get("done_p") is None:  # bench.synthetic_replay's rows: 1 % terminals
        return synthetic_rows(c["capacity"], c["obs"], c["act"], seed, 0.01)
    return config_rows(c, seed)


@pytest.mark.parametrize("hset", _depth.HSETS)
@pytest.mark.parametrize("case", sorted(_depth.CASES))
def test_every_layer_moves_on_the_oracles_first_step(case, hset):
    c = _depth.config(case, hset)
    st, hp = oracle_fresh_state(c)
    B, A = c["batch"], c["act"]
    g = np.random.default_rng(11)
    # the engine's pre-step state is the fresh state on step 1: the trajectory and the local oracle coincide
    _, _, _, _, outs, redrawn, _ = _ties.tie_free_draw(g, _rows(c), c["capacity"], B, A, hp, [st, st])
    post = outs[0][1]
    shares = {}
    for name in ("pi", "q1", "q2"):
        before, after = getattr(st, name), getattr(post, name)
        assert len(before.W) == len(c.get(f"{'pi' if name == 'pi' else 'q'}_hidden", c.get("hidden"))) + 1
        for l, (w0, w1) in enumerate(zip(before.W, after.W)):
            shares[name, l] = float(np.mean(np.abs(w1.astype(np.float64) - w0.astype(np.float64)) > MOVE))
    print(f"[visible] {c['name']}: {redrawn} rows redrawn, lowest share {min(shares.values()):.3f} at "
          f"{min(shares, key=shares.get)}")
    low = {k: v for k, v in shares.items() if v < SHARE}
    assert not low, (c["name"], low)


@pytest.mark.parametrize("shape", sorted(_depth.SHAPES))
def test_the_rl_adam_steps_meet_the_conditions_on_their_inputs(shape):
    """test_gpu_hyper.py::_conditions on the oracle's own trajectory, the steps
    drawn as the GPU test draws them: every step's batch holds >= 4 terminal
    and >= 4 non-terminal rows, and >= 5 % of the raw log sigma entries lie
    below the narrow clamp, above it and inside it.  The cases of one shape
    share their inputs, so one walk per shape."""
    from test_gpu_hyper import _conditions

    case = next(k for k in sorted(_depth.CASES) if _depth.SHAPE_OF[k] == shape)
    c = _depth.config(case, "rl+adam")
    st, hp = oracle_fresh_state(c)
    B, A = c["batch"], c["act"]
    g = np.random.default_rng(11)
    check = _conditions(f"{shape}_rl+adam/oracle", True)
    for k in range(1, (2 if B > 1024 else 3) + 1):
        _, _, _, bt, outs, _, _ = _ties.tie_free_draw(g, _rows(c), c["capacity"], B, A, hp, [st, st])
        check(k, hp, bt, st.pi, None, None)
        st = outs[0][1]


def test_bf16_products_alone_miss_the_step_one_bound_at_depth_5_b1100():
    """Why tests/test_gpu_depth.py::BF16_EMULATED exists: the step with bf16
    products (tests/_bf16_emulation.py), no engine involved, leaves fewer than
    98.5 % of pi's elements within 0.01 lr of the fp32 oracle on step 1 of
    h5_b1100 (measured 0.9767; the rest are +-lr sign flips of ~0 gradients),
    while the two-layer nets of the same widths and batch keep that bound.
    The patch of the oracle's MLP ends with the block."""
    import copy

    import _bf16_emulation as EM
    from oracle import sac_oracle as O

    shares = {}
    for name, c in (("h5", _depth.SHAPES["h5_b1100"]),
                    ("h2", dict(_depth.SHAPES["h5_b1100"], q_hidden=_depth.Q5[:2], pi_hidden=_depth.P5[:2]))):
        st, hp = oracle_fresh_state(c)
        rows, B, A = _rows(c), c["batch"], c["act"]
        g = np.random.default_rng(13)  # test_gpu_parity.py::_bf16_one_step_from_the_engine_state's draws
        idx = g.choice(c["capacity"], size=B, replace=False).astype(np.int32)
        et = g.standard_normal((B, A)).astype(np.float32)
        ea = g.standard_normal((B, A)).astype(np.float32)
        bt = O.Batch(rows["obs"][idx], rows["act"][idx], rows["rew"][idx], rows["next_obs"][idx], rows["done"][idx])
        _, emu = EM.step(st, hp, bt, et, ea)
        assert O.MLP.forward.__module__ == O.__name__ and O.MLP.backward.__module__ == O.__name__
        ref = copy.deepcopy(st)
        O.training_step(ref, hp, bt, et, ea)
        d = np.concatenate([np.abs(a - b).ravel() for a, b in zip(emu.pi.params(), ref.pi.params())]) / hp.actor_lr
        assert d.max() <= 2.02
        shares[name] = float(np.mean(d <= 0.01))
    print(f"[bf16-emu] step 1, pi within 0.01 lr: {shares}")
    assert 0.95 < shares["h5"] < 0.985 <= shares["h2"], shares


@pytest.mark.parametrize("case", ["h1_roles", "h5_roles"])
def test_device_rng_draws_are_tie_free_at_the_gpu_tests_seed(case):
    """The role, row-tile, pair-tile and stage cases of one depth share their
    shape, seed and rows: one walk per depth."""
    from test_gpu_action_width import oracle_walk
    from test_gpu_depth import RNG_CASES, RNG_SEED

    assert case in RNG_CASES
    c = dict(_depth.CASES[case][0], done_p=0.01)
    st, hp = oracle_fresh_state(c, RNG_SEED)
    rows = _rows(c, RNG_SEED)
    walk = oracle_walk(st, hp, rows, c["capacity"], c["batch"], c["act"], RNG_SEED, 0, 6)
    ties = [t for t, _, _ in walk]
    assert not any(ties), (case, RNG_SEED, ties)
