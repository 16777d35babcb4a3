"""HIP engine vs the reference (golden vectors) and vs the pinned CPU oracle on
identical seeded batches + eps, through the C ABI (injected indices/eps).

Tolerances (written here, per north_star "within 1e-3 rel fp32"):
  fp32 mode (exact-fp32 MFMA products): losses 1e-4 rel; y/log_pi 1e-4;
  bf16 mode (bf16 MFMA products, fp32 accumulate): measured deviation of the
  losses 2e-5..1.4e-3 rel (tools/parity_report.py), asserted at 2e-3 rel with
  the abs floor (mean|alpha logpi| + mean|minQ|) for L_pi, which can be ~0
  (SURVEY §7.3).  fp32 mode is the parity mode for the 1e-3 north-star bar.
Post-step parameters: Adam turns a gradient into ~lr*sign(g), so elements whose
true gradient is ~0 may differ by up to 2*lr per step.  fp32: max error within
that bound and 99.5% of elements within 1e-6.  bf16: max within 2*lr*k and
mean |error| <= 0.05*lr*k (sign flips of near-zero gradients accumulate);
per element, one step from the engine's own state,
test_bf16_one_step_from_the_engine_state.
"""
import numpy as np
import pytest
import torch

import _ties
from _fixtures import CONFIGS, batch, eps, oracle_state
from oracle import sac_oracle as O

pytestmark = pytest.mark.gpu

NET_KEYS = ("policy", "q1", "q2", "q1t", "q2t")


def _oracle_net(st, k):
    return {"policy": st.pi, "q1": st.q1, "q2": st.q2, "q1t": st.q1t, "q2t": st.q2t}[k]


def _loss_ok(got, want, floor, rtol):
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= rtol * max(abs(want), floor)


# bf16 loss bounds of fixtures whose bf16 rounding alone exceeds 2e-3 rel, at
# 2x the error of the same step on the CPU with every forward matmul's operands
# rounded to bf16 (fp32 accumulate; tools/debug/bf16_loss_emulation.py) against
# the fp32 oracle.  out_smooth (B = 32, tanh critics under an ELU output), step
# 1: emulation L_Q1 2.36e-3, L_Q2 1.22e-3 rel; the engine 2.36e-3 on L_Q1 (the
# same arithmetic); steps 2, 3 of the emulation <= 9.6e-4.  The seven older
# fixtures in the same emulation: <= 1.4e-3 (mix_act step 2).
BF16_LOSS_RTOL = {"out_smooth": 2 * 2.36e-3}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CONFIGS)
def test_engine_matches_oracle(name, precision):
    from _gpu import make_agent, run_step

    agent, fx, meta, nets = make_agent(name, precision)
    st, hp, _, _ = oracle_state(name)
    rtol = 1e-4 if precision == "fp32" else BF16_LOSS_RTOL.get(name, 2e-3)
    lrs = {"policy": hp.actor_lr, "q1": hp.critic_lr, "q2": hp.critic_lr, "q1t": hp.critic_lr * hp.tau,
           "q2t": hp.critic_lr * hp.tau}  # per-step movement scale; targets accumulate tau * sum_i |dp_i|
    for k in range(1, meta["steps"] + 1):
        et, ea = eps(fx, k)
        ref = O.training_step(st, hp, batch(fx, k), et, ea)
        losses, y, lp = run_step(agent, fx, meta, k)
        floor = float(np.mean(np.abs(st.alpha * ref["log_pi"])) + np.mean(np.abs(ref["y"]))) + 1e-6
        for i, (g, w) in enumerate(zip(losses, ref["losses"])):
            assert _loss_ok(g, w, floor if i == 2 else 1e-3, rtol), (name, precision, k, i, g, w)
        if precision == "fp32":
            np.testing.assert_allclose(y, ref["y"], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(lp, ref["log_pi"], rtol=1e-4, atol=1e-4)
        else:  # bf16 products: mean error within 1% of the mean magnitude
            for got, want in ((y, ref["y"]), (lp, ref["log_pi"])):
                scale = np.abs(want).mean() + 1.0
                assert np.abs(got - want).mean() <= 1e-2 * scale, (name, k, np.abs(got - want).mean(), scale)
                assert np.abs(got - want).max() <= 0.1 * (np.abs(want).max() + 1.0)
        for key in NET_KEYS:
            mine = {kk: v.detach().cpu().numpy() for kk, v in nets[key].state_dict().items()}
            lr = lrs[key] * (k if key in ("policy", "q1", "q2") else k * (k + 1) / 2)
            ds = []
            for pk, want in _oracle_net(st, key).state_dict().items():
                d = np.abs(mine[pk] - want)
                assert d.max() <= 2 * lr + 1e-5, (name, precision, k, key, pk, d.max())
                if precision == "fp32":
                    assert np.mean(d <= 1e-6) >= 0.995, (name, k, key, pk, np.mean(d <= 1e-6))
                ds.append(d.ravel())
            if precision == "bf16":
                d = np.concatenate(ds)
                assert d.mean() <= 0.05 * lr + 1e-7, (name, k, key, d.mean())
        if st.log_alpha is not None:
            la = float(agent.engine.alpha_state[0].item())
            assert abs(la - st.log_alpha) <= (1e-7 if precision == "fp32" else 1e-5), (la, st.log_alpha)


@pytest.mark.parametrize("precision,parts", [("fp32", 4), ("bf16", 2)])
def test_c3_batch_part_counts_match_oracle(precision, parts):
    """C3's update tiles with a batch-part count other than the cost model's
    choice (3; config.upd_parts overrides it): 4 parts (the round-2 layout
    before the model) and 2, against the oracle like
    test_baseline_config_matches_oracle."""
    test_baseline_config_matches_oracle("c3", 12_288, 2, precision, layout={"upd_parts": parts})


@pytest.mark.parametrize("precision,parts", [("fp32", None), ("bf16", None), ("fp32", 4)])
def test_c3_update_block_sizes_match_oracle(precision, parts):
    """C3's phase B with the 1024-thread update tiles (config.upd_threads =
    1024; C3's default runs its 480 B blocks as 512-thread tiles, two per CU),
    default batch parts, and the 512-thread tiles at 4 parts (640 blocks, two
    rounds), against the oracle like test_baseline_config_matches_oracle."""
    lay = {"upd_threads": 512 if parts else 1024}
    if parts:
        lay["upd_parts"] = parts
    test_baseline_config_matches_oracle("c3", 12_288, 2, precision, layout=lay)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c3_stage_path_matches_oracle(precision):
    """C3 through the layer-synchronous stage path (stage_path=1; the row-tile
    kernels are C3's default), against the oracle like
    test_baseline_config_matches_oracle."""
    test_baseline_config_matches_oracle("c3", 12_288, 2, precision, layout={"stage_path": 1})


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c3_row_tiles_match_oracle(precision):
    """C3 through the one-workgroup-per-row-tile kernels (layout "rows"; C3's
    default is the pair-tile kernels, csrc/sac_pairs.h), against the oracle like
    test_baseline_config_matches_oracle."""
    test_baseline_config_matches_oracle("c3", 12_288, 2, precision, layout={"layout": "rows"})


# The layout the default does not take at these shapes: the pair-tile kernels at
# one row and with 4-layer nets (the role split's batches), the row-tile kernels
# at B = 4001 (251 row tiles; by default the pairs run it, the last pair with one
# row tile)
FORCED_EDGES = {"pairs_b1": ("b1", "pairs"), "pairs_deep4": ("deep4", "pairs"),
                "rows_b4001": ("rowtile_b4001", "rows")}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", sorted(FORCED_EDGES))
def test_forced_layout_edges_match_oracle(shape, precision):
    """Ragged and small shapes on the kernel layout the default does not pick
    there, against the oracle with the edge-shape tolerances."""
    base, lay = FORCED_EDGES[shape]
    c = dict(EDGE_SHAPES[base], name=shape)
    _check_config_against_oracle(c, precision, 2 if c["batch"] > 1024 else 3, traj_tol=2e-3,
                                 layout={"layout": lay})


@pytest.mark.parametrize("name", ["c1_auto", "c2", "out_smooth", "out_kink"])
def test_engine_matches_reference_golden_directly(name):
    """Step 1 against the reference's own captured outputs (no oracle in
    between); out_smooth / out_kink: nets with output activations."""
    from _gpu import make_agent, run_step

    agent, fx, meta, nets = make_agent(name, "fp32")
    losses, y, lp = run_step(agent, fx, meta, 1)
    want = fx["step1/out/losses"]
    for g, w in zip(losses, want):
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= 1e-4 * max(abs(w), 1e-2)
    np.testing.assert_allclose(y, fx["step1/out/y"], rtol=1e-4, atol=1e-4)
    key = "step1/post/policy/net.0.weight"
    if key in fx.files:
        got = nets["policy"].state_dict()["net.0.weight"].cpu().numpy()
        assert np.mean(np.abs(got - fx[key]) <= 1e-6) >= 0.995


def test_constant_reward_y_is_r_on_gpu():
    from _gpu import make_agent, run_step

    agent, fx, meta, _ = make_agent("const_reward", "bf16")
    _, y, _ = run_step(agent, fx, meta, 1)
    assert np.array_equal(y, np.ones_like(y))


BENCH_NETS = {"policy": "pi", "q1": "q1", "q2": "q2", "q1t": "q1t", "q2t": "q2t"}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg,capacity,steps", [("c4", 4096, 3), ("c4w", 2048, 3), ("c3", 12_288, 4)])
def test_baseline_config_matches_oracle(cfg, capacity, steps, precision, layout=None):
    """The BASELINE.json configs the fixtures do not cover, against the
    fixture-pinned oracle on seeded batches with injected indices and eps:
      c4  DonkeyVae as BASELINE.json states it: obs 32, act 2, [256,256], B 256;
      c4w the reference Donkey env's real observation width (32-D latent + 2x20
          command history, x3 frame stack = 216), act 2, B 256;
      c3  BipedalWalker at B = 4096 (256 row tiles: the non-role-split phase
          kernels and the 4-chunk update staging, a different code path), a
          4-step trajectory (the layout variants below run 2).
    No golden fixture exists at these shapes (parity unpinned by the reference
    itself; the oracle is pinned by the 8 reference fixtures).  Checks, per
    step: the four losses, y and log pi, every post-step parameter of the five
    networks and log alpha, with this file's tolerances."""
    import bench

    _check_config_against_oracle(dict(bench.CONFIGS[cfg], capacity=capacity), precision, steps,
                                 roles=cfg != "c3", layout=layout)


# Shapes at the edges of the kernels' tiling, none of them a BASELINE config:
# ragged last row tiles (B % 16 != 0) on each of the three phase-kernel layouts
# (hidden split, per-network roles, pair tiles: the row-tile kernels in FORCED_EDGES), a one-row batch,
# the widest input the [256, 256] nets take (obs 256 + act 6: Kp 288 > 256 for
# the critics) and four-layer nets.
EDGE_SHAPES = {
    "split_b250": dict(obs=24, act=4, hidden=[256, 256], batch=250, capacity=2048),
    "roles_b17": dict(obs=5, act=1, hidden=[64, 64], batch=17, capacity=512),
    "b1": dict(obs=3, act=2, hidden=[32, 32], batch=1, capacity=64),
    "rowtile_b4001": dict(obs=24, act=4, hidden=[256, 256], batch=4001, capacity=8192),
    "obs256": dict(obs=256, act=6, hidden=[256, 256], batch=64, capacity=1024),
    "deep4": dict(obs=11, act=3, hidden=[128, 96, 64], batch=80, capacity=1024),
    # past the phase kernels' LDS layout: the stage path (csrc/sac_wide.h) at small batches
    "obs300": dict(obs=300, act=6, hidden=[256, 256], batch=64, capacity=1024),
    "wide400_300": dict(obs=17, act=6, hidden=[400, 300], batch=256, capacity=2048),
    "wide512_b384": dict(obs=24, act=4, hidden=[512, 512], batch=384, capacity=2048),
    # the stage path at a large batch with ragged column blocks and three hidden layers
    "wide_deep_b1100": dict(obs=5, act=3, hidden=[96, 160, 64], batch=1100, capacity=4096),
}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", sorted(EDGE_SHAPES))
def test_edge_shapes_match_oracle(shape, precision):
    """Ragged and extreme shapes against the oracle, with the same checks and
    tolerances as the BASELINE configs (parity unpinned by the reference at
    these shapes; the oracle is pinned by the 8 reference fixtures).
    wide_deep_b1100 runs the stage path (forced: the row-tile kernels fit it)."""
    c = dict(EDGE_SHAPES[shape], name=shape)
    # y / log pi against the oracle's trajectory after step 1: 2e-3 at these
    # shapes (measured 6.1e-4 at obs 256, step 3: Adam sign flips of ~0 gradients)
    _check_config_against_oracle(c, precision, 2 if c["batch"] > 1024 else 3, traj_tol=2e-3,
                                 layout={"stage_path": 1} if shape == "wide_deep_b1100" else None)


# shapes the phase kernels fit: the stage path runs them only when forced (stage_path=1)
STAGE_FORCED = {"wide_deep_b1100", "rowtile_b4001"}


@pytest.mark.parametrize("shape", ["obs300", "wide400_300", "wide512_b384", "wide_deep_b1100", "rowtile_b4001"])
def test_stage_path_is_used_where_the_phase_kernels_do_not_fit(shape):
    """Shapes past the phase kernels' LDS layout run the layer-synchronous stage
    path (no fallback, no refusal); batches past the role split run it when
    stage_path=1 forces it."""
    import bench

    bench.CONFIGS["_stage"] = dict(EDGE_SHAPES[shape])
    try:
        eng, rb, cc = bench.build_engine("_stage", "fp32", 3, torch.device("cuda", 0),
                                         layout={"stage_path": 1} if shape in STAGE_FORCED else None)
    finally:
        del bench.CONFIGS["_stage"]
    assert eng.wide > 0 and not eng.roles
    eng.train(rb, 2)
    eng.check()
    assert all(np.isfinite(eng.losses()))


def _engine_mlp(eng, key):
    """Oracle MLP holding the engine's current parameters of one network (with
    its hidden and output activations)."""
    from _gpu import engine_mlp

    return engine_mlp(eng, key)


def _check_config_against_oracle(c, precision, steps, roles=None, traj_tol=1e-4, layout=None, expect=None,
                                 on_step=None):
    """`steps` engine steps of config c against two oracles, with injected
    indices and eps:
      the trajectory oracle, started from the engine's initial state and run
        on its own from there (losses, y, log pi, log alpha, parameter bounds,
        and in fp32 >= 99.5% of every network's elements within 1e-6);
      fp32 only, the local oracle, loaded with the engine's FULL state before
        each step (tests/test_gpu_parity.py::_oracle_state_from_engine): the
        losses to 1e-5 rel and >= 99.9% of every network's post-step elements
        within 1e-6, free of trajectory drift.
    fp32 steps are drawn tie-free from both states (tests/_ties.py: the rows of
    any summation-order tie -- a ReLU pre-activation within fp32 noise of 0 on
    any pass, a min-Q near-tie of the actor pass, a log sigma of pi(s) on an
    edge of the clamp -- get a fresh index and eps
    until none is left), so the element checks hold on all five networks at
    every shape; the test prints how many rows it redrew and the ties seen.
    c is a config dict of tests/_gpu.py::build_engine: besides the shape it may
    name activations, output activations, a fixed alpha (auto=False: L_alpha
    NaN on both sides, the alpha state untouched), the log sigma clamp, the
    hyper-parameters, Adam settings and the replay's terminal share; the
    oracle's nets and hyper-parameters are built from the same dict.  expect:
    the kernel layout the case must run (tests/_gpu.py::assert_layout).
    on_step: called after every step's checks with (k, hp, batch, the
    trajectory oracle's policy before the step, the local oracle's post-step
    state or None in bf16, the engine), for checks of the caller's own."""
    from _gpu import assert_layout, build_engine, oracle_hyper

    ckey = "_parity_" + c.get("name", "cfg")
    eng, rb, cc = build_engine(c, precision, 3, torch.device("cuda", 0), layout=layout)
    if roles is not None:
        assert eng.roles == roles
    if layout and layout.get("layout") == "pairs":
        assert eng.pairs and not eng.roles and not eng.wide
    if expect is not None:
        assert_layout(eng, expect)
    B, A = cc["batch"], cc["act"]
    hp = oracle_hyper(cc)  # bench.build_engine's hyper-parameters where c names none
    st = O.SacState.fresh(_engine_mlp(eng, "pi"), _engine_mlp(eng, "q1"), _engine_mlp(eng, "q2"), hp, A)
    alpha0 = eng.alpha_state[:2].cpu().numpy().copy()
    rows = {k: getattr(rb, k).cpu().numpy() for k in ("obs", "act", "rew", "next_obs", "done")}
    g = np.random.default_rng(11)
    # bf16: 2e-3 at B >= 256; a loss over fewer rows averages fewer independent
    # product roundings, so its relative error grows like 1 / sqrt(B)
    rtol = 1e-4 if precision == "fp32" else 2e-3 * max(1.0, (256 / B) ** 0.5)
    lrs = {"policy": hp.actor_lr, "q1": hp.critic_lr, "q2": hp.critic_lr, "q1t": hp.critic_lr * hp.tau,
           "q2t": hp.critic_lr * hp.tau}
    fp32 = precision == "fp32"
    for k in range(1, steps + 1):
        # the engine's own pre-step state: the local oracle (fp32), y / log pi one step from it
        loc = _oracle_state_from_engine(eng, A, hp.auto_entropy_tuning) if fp32 else None
        pre = {n: _engine_mlp(eng, n) for n in ("pi", "q1t", "q2t")}
        alpha_pre = np.float32(eng.alpha_state[1].item())
        pi_pre = st.pi.copy() if on_step else None
        idx, et, ea, bt, outs, redrawn, seen = _ties.tie_free_draw(g, rows, len(rb), B, A, hp,
                                                                    [st, loc] if fp32 else [])
        if fp32:
            print(f"[ties] {ckey} step {k}: {redrawn} rows redrawn, ties seen {seen}")
            (ref, st), (ref_loc, post_loc) = outs
        else:
            ref = O.training_step(st, hp, bt, et, ea)
        eng.train(rb, 1, indices=torch.from_numpy(idx).reshape(1, B),
                  eps=torch.from_numpy(np.stack([et, ea])).reshape(1, 2, B, A))
        torch.cuda.synchronize()
        got = eng.losses()
        floor = float(np.mean(np.abs(st.alpha * ref["log_pi"])) + np.mean(np.abs(ref["y"]))) + 1e-6
        # bf16 L_alpha = -log(alpha) mean(log pi + H): relative to the scale of its
        # terms, |log alpha| mean|log pi| (the mean cancels; measured 0.85% rel at obs 300)
        a_floor = abs(float(np.log(alpha_pre))) * float(np.mean(np.abs(ref["log_pi"]))) + 1e-6
        for i, (gv, w) in enumerate(zip(got, ref["losses"])):
            fl = floor if i == 2 else (a_floor if i == 3 and precision == "bf16" else 1e-3)
            assert _loss_ok(gv, w, fl, rtol), (ckey, precision, k, i, gv, w)
        y = eng.last_targets().cpu().numpy()
        lp = eng.last_log_pi().cpu().numpy()
        if fp32:
            _print_margins(ckey, k, eng, got, y, lp, ref, st, ref_loc, loc, post_loc, lrs, traj_tol, floor)
            # one step from the engine's own state: the kernels' arithmetic alone
            np.testing.assert_allclose(y, ref_loc["y"], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(lp, ref_loc["log_pi"], rtol=1e-4, atol=1e-4)
            fl_loc = float(np.mean(np.abs(loc.alpha * ref_loc["log_pi"])) + np.mean(np.abs(ref_loc["y"])))
            for i, (gv, w) in enumerate(zip(got, ref_loc["losses"])):
                assert _loss_ok(gv, w, fl_loc if i == 2 else 1e-3, 1e-5), (ckey, "local", k, i, gv, w)
            for n, net in (("pi", post_loc.pi), ("q1", post_loc.q1), ("q2", post_loc.q2), ("q1t", post_loc.q1t),
                           ("q2t", post_loc.q2t)):
                mine = {kk: v.detach().cpu().numpy() for kk, v in eng.nets[n].state_dict().items()}
                for pk, want in net.state_dict().items():
                    d = np.abs(mine[pk] - want)
                    assert np.mean(d <= 1e-6) >= 0.999, (ckey, "local", k, n, pk, np.mean(d <= 1e-6))
            # against the oracle's own trajectory: from step 2 on, an Adam update
            # whose gradient is ~0 may take the other sign under another
            # summation order (that element moves +-lr instead of -+lr, inside
            # the parameter bounds below): traj_tol (1e-4 for the BASELINE
            # configs; the edge shapes pass their measured bound)
            tol = 1e-4 if k == 1 else traj_tol
            np.testing.assert_allclose(y, ref["y"], rtol=tol, atol=tol)
            np.testing.assert_allclose(lp, ref["log_pi"], rtol=tol, atol=tol)
        else:
            for gv, want in ((y, ref["y"]), (lp, ref["log_pi"])):
                scale = np.abs(want).mean() + 1.0
                assert np.abs(gv - want).mean() <= 1e-2 * scale, (ckey, k, np.abs(gv - want).mean(), scale)
        for key, ek in BENCH_NETS.items():
            mine = {kk: v.detach().cpu().numpy() for kk, v in eng.nets[ek].state_dict().items()}
            lr = lrs[key] * (k if key in ("policy", "q1", "q2") else k * (k + 1) / 2)
            ds = []
            for pk, want in _oracle_net(st, key).state_dict().items():
                d = np.abs(mine[pk] - want)
                assert d.max() <= 2 * lr + 1e-5, (c.get('name'), precision, k, key, pk, d.max())
                if fp32:  # every network: the step was drawn tie-free
                    assert np.mean(d <= 1e-6) >= 0.995, (c.get('name'), k, key, pk, np.mean(d <= 1e-6))
                ds.append(d.ravel())
            if precision == "bf16":
                d = np.concatenate(ds)
                assert d.mean() <= 0.05 * lr + 1e-7, (c.get('name'), k, key, d.mean())
        if hp.auto_entropy_tuning:
            la = float(eng.alpha_state[0].item())
            assert abs(la - st.log_alpha) <= (1e-7 if precision == "fp32" else 1e-5), (la, st.log_alpha)
        else:  # fixed alpha: no L_alpha on either side, [log alpha, alpha] as created
            assert np.isnan(got[3]) and np.isnan(ref["losses"][3]), (ckey, k, got[3], ref["losses"][3])
            assert np.array_equal(eng.alpha_state[:2].cpu().numpy(), alpha0), (ckey, k)
        if on_step:
            on_step(k, hp, bt, pi_pre, post_loc if fp32 else None, eng)
    eng.check()


def _print_margins(ckey, k, eng, got, y, lp, ref, st, ref_loc, loc, post_loc, lrs, traj_tol, floor):
    """One line per fp32 step of _check_config_against_oracle, printed before its
    assertions (pytest -s): the kernel family that ran and every figure the
    step is bounded on, each as a fraction of its bound (<= 1 passes) or, for
    the element shares, as the lowest share over the tensors of all five
    networks next to the share asked."""
    from _gpu import layout_of

    def loss_frac(want, fl_pi, rtol):
        return max(abs(g - w) / (rtol * max(abs(w), fl_pi if i == 2 else 1e-3))
                   for i, (g, w) in enumerate(zip(got, want)) if not np.isnan(w))

    def close_frac(a, b, tol):  # numpy's assert_allclose: |a - b| <= atol + rtol |b|
        return float(np.max(np.abs(a - b) / (tol + tol * np.abs(b))))

    def nets(state):
        for key, ek in BENCH_NETS.items():
            mine = {kk: v.detach().cpu().numpy() for kk, v in eng.nets[ek].state_dict().items()}
            for pk, want in _oracle_net(state, key).state_dict().items():
                yield key, np.abs(mine[pk] - want)

    fl_loc = float(np.mean(np.abs(loc.alpha * ref_loc["log_pi"])) + np.mean(np.abs(ref_loc["y"])))
    tol = 1e-4 if k == 1 else traj_tol
    cap = max(float(d.max()) / (2 * lrs[key] * (k if key in ("policy", "q1", "q2") else k * (k + 1) / 2) + 1e-5)
              for key, d in nets(st))
    print(f"[margin] {ckey} step {k}: {layout_of(eng)} kernels; of its bound: losses {loss_frac(ref_loc['losses'], fl_loc, 1e-5):.3f} "
          f"local {loss_frac(ref['losses'], floor, 1e-4):.3f} trajectory, y {close_frac(y, ref_loc['y'], 1e-4):.3f} / "
          f"{close_frac(y, ref['y'], tol):.3f}, log pi {close_frac(lp, ref_loc['log_pi'], 1e-4):.3f} / "
          f"{close_frac(lp, ref['log_pi'], tol):.3f}, largest element error {cap:.3f} of 2 lr + 1e-5; lowest share of a "
          f"tensor within 1e-6: {min(float(np.mean(d <= 1e-6)) for _, d in nets(post_loc)):.5f} local (0.999 asked) "
          f"{min(float(np.mean(d <= 1e-6)) for _, d in nets(st)):.5f} trajectory (0.995 asked)")


def _oracle_state_from_engine(eng, act, auto=True):
    """The engine's full training state as an oracle SacState: parameters of the
    five networks, Adam moments and step counts, and the alpha state."""
    to_np = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    mlp = {k: _engine_mlp(eng, k) for k in ("pi", "q1", "q2", "q1t", "q2t")}
    steps = eng.opt_steps.cpu().numpy()
    opt = {}
    for i, k in enumerate(("pi", "q1", "q2")):
        m, v = eng.adam_views(k)
        opt[k] = O.AdamState([to_np(x) for x in m], [to_np(x) for x in v], float(steps[i]))
    al = eng.alpha_state.cpu().numpy()
    return O.SacState(mlp["pi"], mlp["q1"], mlp["q2"], mlp["q1t"], mlp["q2t"], opt["pi"], opt["q1"], opt["q2"], act,
                      log_alpha=float(al[0]) if auto else None, alpha=float(al[1]), opt_alpha_m=float(al[2]),
                      opt_alpha_v=float(al[3]), opt_alpha_step=float(steps[3]))


@pytest.mark.parametrize("shape", ["c2_split", "c4", "roles_b384", "rowtile_b2000", "pairs_b2000", "stage_b2000",
                                   "wide512_b384", "wide400_300"])
def test_one_step_from_the_engine_state(shape):
    """Per-step parity without trajectory drift (fp32): before every step the
    oracle is loaded with the engine's FULL state (parameters, Adam moments and
    step counts, alpha), runs the same step, and every post-step parameter of
    the five networks must match the engine's to 1e-6 for >= 99.9% of the
    elements (a handful may sit where Adam divides a ~0 gradient by ~eps) and
    to 2 lr everywhere; losses to 1e-5 rel (L_pi against the scale of its terms).  Four steps per shape, covering the
    hidden-split, role and row-tile kernel layouts and the stage path (B = 2000 with
    [128, 128], and [512, 512] / [400, 300] hidden layers at small batches)."""
    import bench

    c = {"c2_split": dict(obs=24, act=4, hidden=[256, 256], batch=256, capacity=2048),
         "c4": dict(obs=32, act=2, hidden=[256, 256], batch=256, capacity=2048),
         "roles_b384": dict(obs=24, act=4, hidden=[256, 256], batch=384, capacity=2048),
         "rowtile_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "pairs_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "stage_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "wide512_b384": dict(obs=24, act=4, hidden=[512, 512], batch=384, capacity=2048),
         "wide400_300": dict(obs=17, act=6, hidden=[400, 300], batch=256, capacity=2048),
         "split_b250": EDGE_SHAPES["split_b250"], "deep4": EDGE_SHAPES["deep4"], "deep4_pairs": EDGE_SHAPES["deep4"],
         "obs256": EDGE_SHAPES["obs256"],
         "c3_rows": dict(obs=24, act=4, hidden=[256, 256], batch=4096, capacity=8192),
         "c4w": dict(obs=216, act=2, hidden=[256, 256], batch=256, capacity=2048)}[shape]
    # roles_b384: the role kernels without the hidden split; stage_b2000: the
    # stage path (the row-tile kernels fit B = 2000)
    lay = {"roles_b384": {"layout": "roles"}, "stage_b2000": {"stage_path": 1},
           "rowtile_b2000": {"layout": "rows"}}.get(shape)
    bench.CONFIGS["_local"] = c
    try:
        eng, rb, cc = bench.build_engine("_local", "fp32", 3, torch.device("cuda", 0), layout=lay)
    finally:
        del bench.CONFIGS["_local"]
    B, A = cc["batch"], cc["act"]
    hp = O.SacHyper(alpha=0.1, auto_entropy_tuning=True)
    rows = {k: getattr(rb, k).cpu().numpy() for k in ("obs", "act", "rew", "next_obs", "done")}
    g = np.random.default_rng(11)
    lrs = {"pi": hp.actor_lr, "q1": hp.critic_lr, "q2": hp.critic_lr, "q1t": hp.critic_lr, "q2t": hp.critic_lr}
    for k in range(1, 5):
        st = _oracle_state_from_engine(eng, A)
        idx, et, ea, bt, outs, redrawn, seen = _ties.tie_free_draw(g, rows, len(rb), B, A, hp, [st])
        print(f"[ties] {shape} step {k}: {redrawn} rows redrawn, ties seen {seen}")
        (ref, post), = outs
        eng.train(rb, 1, indices=torch.from_numpy(idx).reshape(1, B),
                  eps=torch.from_numpy(np.stack([et, ea])).reshape(1, 2, B, A))
        torch.cuda.synchronize()
        # L_pi = mean(alpha log pi - min Q) cancels: its scale is that of its terms
        floor = float(np.mean(np.abs(st.alpha * ref["log_pi"])) + np.mean(np.abs(ref["y"])))
        for i, (gv, w) in enumerate(zip(eng.losses(), ref["losses"])):
            assert abs(gv - w) <= 1e-5 * max(abs(w), floor if i == 2 else 1e-3), (shape, k, i, gv, w)
        for n, net in (("pi", post.pi), ("q1", post.q1), ("q2", post.q2), ("q1t", post.q1t), ("q2t", post.q2t)):
            mine = {kk: v.detach().cpu().numpy() for kk, v in eng.nets[n].state_dict().items()}
            for pk, want in net.state_dict().items():
                d = np.abs(mine[pk] - want)
                assert d.max() <= 2 * lrs[n], (shape, k, n, pk, d.max())
                assert np.mean(d <= 1e-6) >= 0.999, (shape, k, n, pk, np.mean(d <= 1e-6))
        assert abs(float(eng.alpha_state[0].item()) - post.log_alpha) <= 1e-7
    eng.check()


@pytest.mark.parametrize("shape", ["c2_split", "c3_pairs", "roles_b384", "rowtile_b2000", "pairs_b2000", "stage_b2000",
                                   "wide400_300", "split_b250", "deep4", "deep4_pairs", "obs256", "c3_rows", "c4w"])
def test_bf16_one_step_from_the_engine_state(shape):
    """Per-element bound for the bf16 mode, free of trajectory drift: before
    every step the fp32 oracle is loaded with the engine's FULL state, both run
    the same step, and the bf16 engine's post-step parameters are compared
    element by element.  Adam's update is lr * m^/(sqrt(v^) + eps): a bf16
    gradient with a relative error d moves it by ~d * lr, so the bounds are in
    units of each network's lr (Polyak targets: tau * lr).  Bounds (measured,
    profiles/r06_bf16_local.txt, with margin; f = sqrt(256 / B) below B = 256,
    else 1): step 1 (Adam moments 0: every update is +-lr) >= 1 - 0.015 f of
    each network's elements within 0.01 f lr (the rest are sign flips of ~0
    gradients, 2 lr); later steps >= 92% within 0.05 f lr (measured >= 95.4%
    at B >= 250, 93.4% for the 4-layer nets at B = 80), >= 98.5% within
    0.25 f lr, median <= 0.02 f lr; every element within 2 lr (+ the Polyak
    update's own rounding); y and log pi per row within 8e-3 f / 3e-2 f of
    (|value| + 1) at the 99th percentile, 1.5e-2 f / 6e-2 f at most (measured
    <= 3.1e-3 / 1.1e-2 at obs <= 24, 5.2e-3 for y at the 216-wide C4w input).
    This check found the row-tile kernels' bf16 fault (fixed in round 6): the
    actor rows' log pi wrong in ~30% of rows at hidden widths other than 256."""
    c = {"c2_split": dict(obs=24, act=4, hidden=[256, 256], batch=256, capacity=2048),
         "c3_pairs": dict(obs=24, act=4, hidden=[256, 256], batch=4096, capacity=8192),
         "roles_b384": dict(obs=24, act=4, hidden=[256, 256], batch=384, capacity=2048),
         "rowtile_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "pairs_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "stage_b2000": dict(obs=17, act=6, hidden=[128, 128], batch=2000, capacity=4096),
         "wide400_300": dict(obs=17, act=6, hidden=[400, 300], batch=256, capacity=2048),
         "split_b250": EDGE_SHAPES["split_b250"], "deep4": EDGE_SHAPES["deep4"], "deep4_pairs": EDGE_SHAPES["deep4"],
         "obs256": EDGE_SHAPES["obs256"],
         "c3_rows": dict(obs=24, act=4, hidden=[256, 256], batch=4096, capacity=8192),
         "c4w": dict(obs=216, act=2, hidden=[256, 256], batch=256, capacity=2048)}[shape]
    lay = {"roles_b384": {"layout": "roles"}, "rowtile_b2000": {"layout": "rows"}, "pairs_b2000": {"layout": "pairs"},
           "c3_pairs": {"layout": "pairs"}, "stage_b2000": {"stage_path": 1}, "deep4_pairs": {"layout": "pairs"},
           "c3_rows": {"layout": "rows"}}.get(shape)
    _bf16_one_step_from_the_engine_state(shape, c, lay)


def _bf16_one_step_from_the_engine_state(shape, c, lay=None, expect=None, emulated=False):
    """The body of test_bf16_one_step_from_the_engine_state (its docstring
    states the bounds) for a config dict of tests/_gpu.py::build_engine; expect:
    the kernel layout the case must run.
    emulated: for a case whose bf16 rounding alone exceeds those bounds (the
    caller names the case and the figures).  Every step is also run on the CPU
    with bf16 products (tests/_bf16_emulation.py) from the same state on the
    same rows, and that emulation is measured against the fp32 oracle exactly
    as the engine is.  A bound the emulation meets stays as it is; one it
    misses becomes twice the emulation's deviation (for a share of elements:
    twice its missing share), the factor for the engine's other summation
    order.  Nothing of the engine's output enters a bound; the 2 lr cap on
    every element stays."""
    from _gpu import assert_layout, build_engine, oracle_hyper

    def lim(std, emu):  # the standing bound on a deviation, or twice the emulation's where it misses that
        return std if emu is None or emu <= std else 2.0 * emu

    def share_lim(std, emu):  # the same for a share of elements that must lie within a distance
        return std if emu is None or emu >= std else 1.0 - 2.0 * (1.0 - emu)

    eng, rb, cc = build_engine(c, "bf16", 3, torch.device("cuda", 0), layout=lay)
    if expect is not None:
        assert_layout(eng, expect)
    B, A = cc["batch"], cc["act"]
    hp = oracle_hyper(cc)
    rows = {k: getattr(rb, k).cpu().numpy() for k in ("obs", "act", "rew", "next_obs", "done")}
    g = np.random.default_rng(13)
    lrs = {"pi": hp.actor_lr, "q1": hp.critic_lr, "q2": hp.critic_lr, "q1t": hp.critic_lr * hp.tau,
           "q2t": hp.critic_lr * hp.tau}
    # fewer rows average fewer independent product roundings: bounds x sqrt(256 / B) below B = 256
    f = max(1.0, (256 / B) ** 0.5)
    bad = []
    for k in range(1, 4):
        st = _oracle_state_from_engine(eng, A, hp.auto_entropy_tuning)
        idx = g.choice(len(rb), size=B, replace=False).astype(np.int32)
        et = g.standard_normal((B, A)).astype(np.float32)
        ea = g.standard_normal((B, A)).astype(np.float32)
        bt = O.Batch(rows["obs"][idx], rows["act"][idx], rows["rew"][idx], rows["next_obs"][idx], rows["done"][idx])
        emu, emu_post = None, None
        if emulated:  # before the oracle's own step, which moves st
            import _bf16_emulation

            emu, emu_post = _bf16_emulation.step(st, hp, bt, et, ea)
        ref = O.training_step(st, hp, bt, et, ea)
        eng.train(rb, 1, indices=torch.from_numpy(idx).reshape(1, B),
                  eps=torch.from_numpy(np.stack([et, ea])).reshape(1, 2, B, A))
        torch.cuda.synchronize()
        for nm, got, want in (("y", eng.last_targets().cpu().numpy(), ref["y"]),
                              ("log_pi", eng.last_log_pi().cpu().numpy(), ref["log_pi"])):
            r = np.abs(got - want) / (np.abs(want) + 1.0)
            print(f"[bf16-local] {shape} step {k} {nm}: rel p50 {np.median(r):.2e} p99 {np.quantile(r, 0.99):.2e} "
                  f"max {r.max():.2e}")
            p99, mx = (8e-3 * f, 1.5e-2 * f) if nm == "y" else (3e-2 * f, 6e-2 * f)
            if emulated:
                re = np.abs(emu[nm] - want) / (np.abs(want) + 1.0)
                p99, mx = lim(p99, float(np.quantile(re, 0.99))), lim(mx, float(re.max()))
                print(f"[bf16-emu] {shape} step {k} {nm}: the emulation p99 {np.quantile(re, 0.99):.2e} max {re.max():.2e}"
                      f" -> bounds {p99:.2e} {mx:.2e}")
            if not (np.quantile(r, 0.99) <= p99 and r.max() <= mx):
                bad.append((k, nm, float(np.quantile(r, 0.99)), float(r.max())))
        for n, net in (("pi", st.pi), ("q1", st.q1), ("q2", st.q2), ("q1t", st.q1t), ("q2t", st.q2t)):
            mine = {kk: v.detach().cpu().numpy() for kk, v in eng.nets[n].state_dict().items()}
            d = np.concatenate([np.abs(mine[pk] - want).ravel() / lrs[n] for pk, want in net.state_dict().items()])
            print(f"[bf16-local] {shape} step {k} {n}: d/lr p50 {np.median(d):.2e} p99 {np.quantile(d, 0.99):.2e} "
                  f"p999 {np.quantile(d, 0.999):.2e} max {d.max():.2e} within 0.01 {np.mean(d <= 0.01):.4f} "
                  f"0.05 {np.mean(d <= 0.05):.4f}")
            ok = d.max() <= 2.02
            de = None
            if emulated:
                esd = getattr(emu_post, n).state_dict()
                de = np.concatenate([np.abs(esd[pk] - want).ravel() / lrs[n] for pk, want in net.state_dict().items()])
            within = (lambda x: None) if de is None else (lambda x: float(np.mean(de <= x)))  # the emulation's share
            if k == 1:
                need = [share_lim(1.0 - 0.015 * f, within(0.01 * f))]
                ok = ok and np.mean(d <= 0.01 * f) >= need[0]
            else:
                need = [share_lim(0.92, within(0.05 * f)), share_lim(0.985, within(0.25 * f)),
                        lim(0.02 * f, None if de is None else float(np.median(de)))]
                ok = ok and np.mean(d <= 0.05 * f) >= need[0] and np.mean(d <= 0.25 * f) >= need[1] and np.median(d) <= need[2]
            if emulated:
                print(f"[bf16-emu] {shape} step {k} {n}: the emulation within 0.01 f {within(0.01 * f):.4f} 0.05 f "
                      f"{within(0.05 * f):.4f} 0.25 f {within(0.25 * f):.4f} median {np.median(de):.2e} -> "
                      f"{'share asked' if k == 1 else 'shares asked, median allowed'} {' '.join(f'{m:.4f}' for m in need)}")
            if not ok:
                bad.append((k, n, float(np.mean(d <= 0.01 * f)), float(np.mean(d <= 0.05 * f)),
                            float(np.mean(d <= 0.25 * f)), float(np.median(d)), float(d.max())))
    assert not bad, (shape, bad)
    eng.check()
