"""The gradient step's replay addressing on partly filled, wrapped and cleared
rings, on every kernel layout.

The step never calls the replay-gather kernel: every kernel family samples and
gathers its own batch, and the logical-to-slot rule `size < capacity ? li :
(pos + li) % capacity` stands twice in the sources -- tile_slots with
gather_rows behind it (csrc/sac_phases.h: the split, role, row-tile and pair
kernels' phase A and stage_next_batch, phase C's stager) and wide_gather_rows
(csrc/sac_wide.h: the stage path's gather launch and the gather inside its
last phase-C stage).  Every other oracle test of the step fills its replay
with exactly `capacity` rows: full, write slot 0, logical index = slot.  Here
the ring states of tests/_ring.py (tests/test_ring_cpu.py shows that they tell
the slot rules apart):

1. identity: every row terminal with rew = 1 + its push counter, so y == r bit
   for bit and the step's targets name the rows it gathered, with injected
   indices, the device sampler (phase A's gather, then phase C's staged
   records) and graph replay across a push that wraps the ring;
2. rotation invariance: an engine on the ring and one on its twin (the same
   logical rows in a full ring at slot 0) stay equal bit for bit in every
   tensor -- all five columns, and the parity the twin's state has against the
   oracle carried over to every rotation;
3. one independent anchor per layout: a step on the wrapped ring against the
   CPU oracle run on the host rows that were pushed.

Sections 1 and 2 are exact; section 3 uses the step-1 tolerances of
tests/test_gpu_parity.py.  Every case asserts the layout it ran."""
import ctypes

import numpy as np
import pytest
import torch

import _ring as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = R.cases()


def _make_buffer(c, storage="records"):
    from sac.replay_buffer import ReplayBuffer

    return lambda cap: ReplayBuffer(cap, device=DEV, obs_dim=c["obs"], act_dim=c["act"], layout=storage)


def _engine(case, precision, rb):
    from _gpu import assert_layout, build_engine

    shape, lay, expect = CASES[case]
    eng, _, c = build_engine(dict(shape, capacity=rb.capacity), precision, device=DEV, layout=lay, replay=rb)
    assert_layout(eng, expect)
    return eng, c


def _staged_step(eng):
    """The last step whose phase A used the record phase C staged for it."""
    from sac import _engine as E

    f = eng.lib.sac_engine_debug_staged_step
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    got = ctypes.c_uint64(0)
    E.check(f(eng.handle, ctypes.byref(got), eng._stream()))
    return got.value


def _host_sampler(eng, size, step):
    """sac_debug_sample_indices_host for the engine's seed."""
    f = eng.lib.sac_debug_sample_indices_host
    f.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    out = np.zeros(eng.batch, np.int32)
    assert f(size, eng.batch, int(eng.cfg.seed), step, out.ctypes.data) == 0
    return out.astype(np.int64)


def _y(eng):
    eng.check()
    return eng.last_targets().cpu().numpy()


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("storage", ["records", "soa"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_gathers_the_models_rows(case, storage, precision):
    shape = CASES[case][0]
    geo = R.geometry(case)
    B, cap = shape["batch"], geo["capacity"]
    mk = _make_buffer(shape, storage)
    rows_fn = R.id_rows(shape["obs"], shape["act"], 1)
    g = np.random.default_rng(2)
    eng = None
    keep = []  # buffers stay allocated: a staged record is keyed on its buffer's address
    for state in R.STATES:
        ring = R.Ring(cap, shape["obs"], shape["act"], rows_fn, mk(cap))
        keep.append(ring)
        if eng is None:
            eng, c = _engine(case, precision, ring.rb)
        # cleared: two device-sampled steps on the full ring leave a staged batch of its rows pending
        R.fill(ring, state, geo, between=lambda r: eng.train(r.rb, 2))
        ring.check_buffer()
        m, rb = ring.model, ring.rb
        rew = m.logical()["rew"]
        assert rb.layout == storage and np.array_equal(rb.rew.cpu().numpy(), m.phys["rew"])
        # injected indices: one step, then one call of two steps (the stage
        # path gathers the second inside the first step's last launch)
        idx = np.stack([R.edge_indices(m, B, g) for _ in range(3)])
        eng.train(rb, 1, indices=torch.from_numpy(idx[:1]))
        assert np.array_equal(_y(eng), rew[idx[0]]), (state, "injected")
        eng.train(rb, 2, indices=torch.from_numpy(idx[1:]))
        assert np.array_equal(_y(eng), rew[idx[2]]), (state, "injected, second step of a call")
        # device sampler: three calls of one step; the second and third read phase C's staged record
        steps = []
        for call in range(3):
            step = int(eng.rng_step.item())
            steps.append(step)
            eng.train(rb, 1)
            li = _host_sampler(eng, m.size, step)
            assert np.array_equal(li, R.sampled_indices(m.size, B, int(eng.cfg.seed), step))
            assert np.array_equal(_y(eng), rew[li]), (state, "sampled", call)
        if not eng.wide:
            assert _staged_step(eng) >= steps[1] > 0, (state, _staged_step(eng), steps)
        # one call of two steps: on the stage path the second step's batch is gathered one launch early
        step = int(eng.rng_step.item())
        eng.train(rb, 2)
        assert np.array_equal(_y(eng), rew[_host_sampler(eng, m.size, step + 1)]), (state, "sampled, two steps")

    # graph replay: captured on the partial ring, replayed after pushes that wrap it
    ring = R.Ring(cap, shape["obs"], shape["act"], rows_fn, mk(cap))
    keep.append(ring)
    R.fill(ring, "partial", geo)
    eng.train_graph(ring.rb, 0, 2)
    left = cap + geo["w"] - geo["partial"]
    ring.push_batch(left // 2)
    ring.push_batch(left - left // 2 - 2)
    ring.push_rows(2)
    ring.check_buffer()
    m = ring.model
    assert (m.size, m.pos) == (cap, geo["w"])
    rew = m.logical()["rew"]
    step = int(eng.rng_step.item())
    eng.train_graph(ring.rb, 3, 2)  # one replay of the graph and a remainder
    assert int(eng.rng_step.item()) == step + 3
    assert np.array_equal(_y(eng), rew[_host_sampler(eng, cap, step + 2)]), "graph, remainder"
    eng.train_graph(ring.rb, 2, 2)  # the replayed graph's own last step
    assert np.array_equal(_y(eng), rew[_host_sampler(eng, cap, step + 4)]), "graph"
    if not eng.wide:
        assert _staged_step(eng) >= step + 1


# ---------------------------------------------------------------- 2. rotation invariance
def _assert_equal_engines(a, b, what):
    a.check()
    b.check()
    assert torch.equal(a.stats, b.stats), (what, "stats")
    tb = b.state_tensors()
    for k, v in a.state_tensors().items():
        assert torch.equal(v, tb[k]), (what, k)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_training_does_not_depend_on_the_rings_rotation(case, precision):
    """Two engines built from the same arguments, one on the ring and one on
    its twin: the sampler, the eps and the logical rows depend on the size
    only, so every statistic and state tensor stays equal bit for bit, through
    injected steps, device-sampled steps and graph replay with a remainder."""
    shape = CASES[case][0]
    geo = R.geometry(case)
    B, A, cap = shape["batch"], shape["act"], geo["capacity"]
    mk = _make_buffer(shape)
    g = np.random.default_rng(4)
    keep = []
    for state in R.STATES:
        ring = R.Ring(cap, shape["obs"], shape["act"], R.mixed_rows(shape["obs"], shape["act"], 7), mk(cap))
        ea, c = _engine(case, precision, ring.rb)
        eb, _ = _engine(case, precision, ring.rb)
        keep += [ring, ea, eb]

        def between(r):
            # cleared: both engines take the same two steps on the full ring
            # (its own twin), which leave each a staged batch of the old rows
            t = R.twin(r, mk)
            keep.append(t)
            ea.train(r.rb, 2)
            eb.train(t.rb, 2)

        R.fill(ring, state, geo, between=between)
        ring.check_buffer()
        tw = R.twin(ring, mk)
        tw.check_buffer()
        keep.append(tw)
        m = ring.model
        assert 0.1 < m.logical()["done"].mean() < 0.5
        idx = torch.from_numpy(np.stack([R.edge_indices(m, B, g) for _ in range(2)]))
        eps = torch.from_numpy(g.standard_normal((2, 2, B, A)).astype(np.float32))
        for eng, rb in ((ea, ring.rb), (eb, tw.rb)):
            eng.train(rb, 2, indices=idx, eps=eps)
        _assert_equal_engines(ea, eb, (state, "injected"))
        for eng, rb in ((ea, ring.rb), (eb, tw.rb)):
            eng.train(rb, 1)
            eng.train(rb, 2)
        _assert_equal_engines(ea, eb, (state, "sampled"))
        if not ea.wide:
            assert _staged_step(ea) > 0 and _staged_step(eb) > 0
        for eng, rb in ((ea, ring.rb), (eb, tw.rb)):
            eng.train_graph(rb, 5, 2)  # two replays and a remainder
        _assert_equal_engines(ea, eb, (state, "graph"))
        assert int(ea.rng_step.item()) == (12 if state == "cleared" else 10)


@pytest.mark.parametrize("case", ["split", "stage"])
def test_graph_is_keyed_on_the_replay(case):
    """An engine that trained by graph on buffer A and is then put back to its
    first state trains by graph on buffer B like a fresh engine on B alone:
    the graph captured on A is not replayed on B."""
    shape = CASES[case][0]
    geo = R.geometry(case)
    cap = geo["capacity"]
    mk = _make_buffer(shape)
    a = R.fill(R.Ring(cap, shape["obs"], shape["act"], R.mixed_rows(shape["obs"], shape["act"], 8), mk(cap)),
               "wrapped", geo)
    b = R.fill(R.Ring(cap, shape["obs"], shape["act"], R.mixed_rows(shape["obs"], shape["act"], 9), mk(cap)),
               "partial", geo)
    used, _ = _engine(case, "fp32", a.rb)
    fresh, _ = _engine(case, "fp32", b.rb)
    snap = used.snapshot()
    used.train_graph(a.rb, 4, 2)
    used.check()
    assert int(used.rng_step.item()) == 4
    used.restore(snap)
    used.train_graph(b.rb, 5, 2)
    fresh.train_graph(b.rb, 5, 2)
    _assert_equal_engines(used, fresh, "graph on B after A")


# ---------------------------------------------------------------- 3. oracle anchor
@pytest.mark.parametrize("case", sorted(CASES))
def test_wrapped_ring_step_matches_oracle(case):
    """fp32, records, the wrapped ring, one step with injected indices and
    eps, against oracle.sac_oracle.training_step from the engine's initial
    state on the host rows that were pushed (never rb.gather), with the step-1
    tolerances of tests/test_gpu_parity.py: y and log pi per row 1e-4
    rtol / atol, losses 1e-4 rel (L_pi against the scale of its terms)."""
    from _gpu import oracle_fresh_state
    from oracle import sac_oracle as O
    from test_gpu_parity import _loss_ok

    shape = CASES[case][0]
    c, ring, idx, et, ea = R.anchor_inputs(case, _make_buffer(shape))
    ring.check_buffer()
    eng, _ = _engine(case, "fp32", ring.rb)
    B, A = c["batch"], c["act"]
    st, hp = oracle_fresh_state(c)
    ref = O.training_step(st, hp, R.batch_of(ring.model.logical(), idx), et, ea)
    eng.train(ring.rb, 1, indices=torch.from_numpy(idx).reshape(1, B),
              eps=torch.from_numpy(np.stack([et, ea])).reshape(1, 2, B, A))
    got = eng.losses()
    y, lp = eng.last_targets().cpu().numpy(), eng.last_log_pi().cpu().numpy()
    print(f"[ring] {case}: max |y - ref| {np.abs(y - ref['y']).max():.2e}, max |log pi - ref| "
          f"{np.abs(lp - ref['log_pi']).max():.2e}, losses {got} ref {ref['losses']}")
    np.testing.assert_allclose(y, ref["y"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lp, ref["log_pi"], rtol=1e-4, atol=1e-4)
    floor = float(np.mean(np.abs(st.alpha * ref["log_pi"])) + np.mean(np.abs(ref["y"]))) + 1e-6
    for i, (gv, w) in enumerate(zip(got, ref["losses"])):
        assert _loss_ok(gv, w, floor if i == 2 else 1e-3, 1e-4), (case, i, gv, w)
