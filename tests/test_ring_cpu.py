"""The host model of the replay ring (tests/_ring.py) and the inputs of
tests/test_gpu_ring.py, checked without a GPU: the model is the reference's
deque, and on every ring state the GPU tests use, a gather with a wrong slot
rule would read other rows with other rewards and move the oracle's y and log
pi by 100 times the parity tolerance -- so the GPU tests cannot pass without
looking at how the step addresses the ring."""
import collections

import numpy as np
import pytest

import _ring as R

CASES = sorted(R.cases())
ENGINE_SEED = 3  # tests/_gpu.py::build_engine's default, the seed of the in-step sampler


@pytest.mark.parametrize("capacity", [1, 7, 37, 203])
def test_model_is_the_reference_deque(capacity):
    """Random sequences of push_batch, single pushes and clear(): the model's
    logical rows are those of collections.deque(maxlen=capacity), its (size,
    pos) those of a ring written in push order, and every logical row sits in
    the slot the model names."""
    g = np.random.default_rng(capacity)
    ring = R.Ring(capacity, 3, 2, R.mixed_rows(3, 2, 1))
    dq, pushed = collections.deque(maxlen=capacity), 0
    for it in range(40):
        op = g.random()
        if op < 0.08:
            ring.clear()
            dq.clear()
            pushed = 0
            assert ring.model.size == 0 and ring.model.pos == 0
            continue
        n = int(g.integers(1, 2 * capacity + 3)) if op < 0.6 else int(g.integers(1, 4))
        first = ring.count
        (ring.push_batch if op < 0.6 else ring.push_rows)(n)
        rows = ring.rows_fn(n, first)
        for i in range(n):
            dq.append(tuple(rows[k][i] for k in R.COLUMNS))
        pushed += n
        m = ring.model
        assert (m.size, m.pos) == (len(dq), pushed % capacity)
        log = m.logical()
        for j, k in enumerate(R.COLUMNS):
            assert np.array_equal(log[k], np.stack([r[j] for r in dq])), (it, k)
            assert np.array_equal(m.phys[k][m.slot(np.arange(m.size))], log[k]), (it, k)


def test_twin_is_full_with_slot_zero():
    geo = R.geometry("rows")
    for state in R.STATES:
        ring = R.fill(R.Ring(geo["capacity"], 5, 3, R.id_rows(5, 3, 0)), state, geo)
        t = R.twin(ring)
        assert (t.model.capacity, t.model.size, t.model.pos) == (ring.model.size, ring.model.size, 0)
        for k in R.COLUMNS:
            assert np.array_equal(t.model.logical()[k], ring.model.logical()[k])
            assert np.array_equal(t.model.phys[k], ring.model.logical()[k])
        assert np.array_equal(t.model.slot(np.arange(t.model.size)), np.arange(t.model.size))


@pytest.mark.parametrize("case", CASES)
def test_ring_states_tell_the_slot_rules_apart(case):
    """Every ring state of the identity test: the geometry is the one the
    issue of the test asks for, and each injected or device-sampled logical
    index maps to a slot other than the slot under the wrong rule (the index
    alone on the wrapped ring, (pos + li) % capacity on the partly filled
    ones), where another reward stands: 0 in a slot never written."""
    shape, lay, expect = R.cases()[case]
    geo = R.geometry(case)
    cap, B = geo["capacity"], shape["batch"]
    assert B == R.BATCH and 100 <= cap <= 300 and cap & (cap - 1) and geo["w"] % 16
    assert B <= geo["refill"] < cap / 2 < geo["partial"] < cap
    g = np.random.default_rng(0)
    for state in R.STATES:
        ring = R.fill(R.Ring(cap, shape["obs"], shape["act"], R.id_rows(shape["obs"], shape["act"], 0)), state, geo)
        m = ring.model
        if state == "wrapped":
            assert (m.size, m.pos) == (cap, geo["w"]) and ring.calls["push_batch"] >= 2 and ring.calls["push"] >= 3
        else:
            assert m.size == m.pos < cap
        rew = m.logical()["rew"]
        assert np.array_equal(rew, np.sort(rew)) and np.unique(rew).size == m.size and rew.min() >= 1
        inj = R.edge_indices(m, B, g)
        edges = {0, m.size - 1} | {e for e in (cap - m.pos - 1, cap - m.pos) if e < m.size}
        if state != "cleared":  # both neighbours of the physical wrap are rows of the ring
            assert len(edges) == 4
        assert edges <= set(inj[:R.ROWS].tolist()) and edges <= set(inj[(B - 1) // R.ROWS * R.ROWS:].tolist())
        assert int(inj[B - 1]) in edges
        # the injected batch, the sampler's batches of the first steps, and every logical index there is
        draws = [inj] + [R.sampled_indices(m.size, B, ENGINE_SEED, step) for step in range(12)] + [np.arange(m.size)]
        for li in draws:
            assert li.min() >= 0 and li.max() < m.size
            good, bad = m.slot(li), R.wrong_slots(m, li)
            assert np.all(good != bad)
            assert np.array_equal(m.phys["rew"][good], rew[li])
            assert np.all(m.phys["rew"][bad] != rew[li])
            if state == "partial":
                never = bad >= m.size
                assert np.all(m.phys["rew"][bad[never]] == 0)
        if state == "partial":  # some index of the batch lands in a slot never written, some wraps onto a written one
            bad = R.wrong_slots(m, inj)
            assert np.any(bad >= m.size) and np.any(bad < m.size)


@pytest.mark.parametrize("case", CASES)
def test_anchor_inputs_move_the_oracle_by_100_tolerances(case):
    """The oracle anchor's inputs: on the rows in physical order (the index
    taken for the slot) the oracle's y and log pi differ from the right ones by
    more than 1e-2, 100 times the anchor's 1e-4, in at least 90 % of the rows."""
    from _gpu import oracle_fresh_state
    from oracle import sac_oracle as O

    c, ring, idx, et, ea = R.anchor_inputs(case)
    m = ring.model
    assert (m.size, m.pos) == (m.capacity, R.geometry(case)["w"])
    assert 0.1 < m.logical()["done"].mean() < 0.5
    out = {}
    for name, rows in (("right", m.logical()), ("wrong", m.phys)):
        st, hp = oracle_fresh_state(c)
        out[name] = O.training_step(st, hp, R.batch_of(rows, idx), et, ea)
    for k in ("y", "log_pi"):
        d = np.abs(out["right"][k] - out["wrong"][k])
        assert np.mean(d > 1e-2) >= 0.9, (case, k, np.mean(d > 1e-2), np.sort(d)[:8])
