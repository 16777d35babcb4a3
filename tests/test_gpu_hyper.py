"""Hyper-parameters, terminal rows, Adam settings and gradient magnitudes on
every kernel layout, against the CPU oracle.

Every other layout test runs tests/_gpu.py::HYPER_DEFAULTS (gamma 0.99, tau
0.005, lr 3e-4, alpha0 0.1, action_scale 1, clamp [-20, 2], Adam (0.9, 0.999,
1e-8), target entropy -act, 1 % terminals); the golden fixtures vary some of
them, on the plain role kernels only.  Each kernel family has its own copy of
the target y = r + gamma (1 - d)(min Q - alpha log pi'), of tanh(z) * scale and
its backward, of the clamp's mask and of Adam's bias-correction scalars
(csrc/sac_split.h, sac_pairs.h, sac_phases.h, sac_wide.h).

Three sets (HYPER): "rl" moves the RL side, "adam" the optimizer side,
"rl+adam" both.  adam_eps = 1e-3 is what makes the backward pass visible: at
1e-8 Adam's update lr m^ / sqrt(v^) does not change under a constant factor on
an element's gradient (a wrong 2/B, -1/B or alpha/B seed, a doubled bias
gradient: tests/test_oracle_hyper_cpu.py::test_adam_eps_decides_whether_a_
scaled_gradient_shows), while 1e-3 lies inside the gradient distribution
(median |g| 1.4e-3 .. 5.8e-3 on the first three steps of these shapes), so
the update reads the magnitude.  The float betas of the engine's config move
an update by ~1e-9 and log alpha by ~5e-9 (bound 1e-7).

Checks and tolerances are those of test_gpu_parity.py::
_check_config_against_oracle, unchanged (3 steps, traj_tol 2e-3 as for every
B = 40 shape), on the shapes of test_gpu_activations.py::LAYOUTS; every case
asserts its layout.  On top, per step (_conditions, _polyak):

* the batch holds >= 4 terminal and >= 4 non-terminal rows, and with the
  narrow clamp >= 5 % of the oracle's raw log sigma entries lie below it,
  >= 5 % above it and >= 5 % inside it, so that no case goes vacuous (on a
  miss: change the case's replay_seed, never the condition);
* fp32: Polyak in units of tau.  Against the local oracle (loaded with the
  engine's own pre-step state), every target element whose online element
  agrees within 1e-6 must agree within tau * 1e-6 + 2 ulp; at most 0.1 % of a
  tensor's elements may fail the precondition (the local oracle's own share).
  At the default tau and lr the targets move 1.5e-6 on step 1, which a 1e-6
  element tolerance barely sees."""
import numpy as np
import pytest

from test_gpu_activations import LAYOUTS, SMALL
from test_gpu_parity import _check_config_against_oracle

pytestmark = pytest.mark.gpu

RL = dict(gamma=0.9, tau=0.05, alpha=0.3, actor_lr=1e-3, critic_lr=2e-3, alpha_lr=5e-3, action_scale=2.5,
          log_std_min=-0.1, log_std_max=0.1, q_out_act="identity", pi_out_act="identity", done_p=0.3)


def _adam(act):
    return dict(betas=(0.8, 0.99), adam_eps=1e-3, target_entropy=-0.5 * act, done_p=0.3)


def hyper(name, act):
    """The config-dict fields of a hyper set for an action size."""
    return {"rl": dict(RL), "adam": _adam(act), "rl+adam": dict(RL, **_adam(act))}[name]


# multi-part update tiles (B > 1024: two batch parts) with non-default Adam scalars
LARGE = dict(SMALL, batch=1040, capacity=2048)


def _conditions(tag, narrow):
    def check(k, hp, bt, pi_pre, post_loc, eng):
        d = np.asarray(bt.d)
        n_term = int((d > 0).sum())
        msg = f"[hyper] {tag} step {k}: {n_term} terminal rows of {d.size}"
        assert n_term >= 4 and d.size - n_term >= 4, msg
        if narrow:
            A = np.asarray(bt.a).shape[1]
            raw = pi_pre.forward(np.asarray(bt.s, np.float32))[0][:, A:]
            lo, hi = np.float32(hp.policy.log_std_min), np.float32(hp.policy.log_std_max)
            below, above = float(np.mean(raw < lo)), float(np.mean(raw > hi))
            msg += f"; log sigma {below:.1%} below the clamp, {above:.1%} above, {1 - below - above:.1%} inside"
            assert min(below, above, 1 - below - above) >= 0.05, msg
        print(msg)
        if post_loc is not None:
            _polyak(tag, k, hp, post_loc, eng)
    return check


def _polyak(tag, k, hp, post_loc, eng):
    tau = float(hp.tau)
    worst = 0.0
    for on, tg in (("q1", "q1t"), ("q2", "q2t")):
        mine = {n: {kk: v.detach().cpu().numpy() for kk, v in eng.nets[n].state_dict().items()} for n in (on, tg)}
        want_t = getattr(post_loc, tg).state_dict()
        for pk, want in getattr(post_loc, on).state_dict().items():
            ok = np.abs(mine[on][pk] - want) <= 1e-6
            assert np.mean(~ok) <= 1e-3, (tag, k, on, pk, float(np.mean(~ok)))
            wt = want_t[pk]
            d = np.abs(mine[tg][pk].astype(np.float64) - wt.astype(np.float64))
            bound = tau * 1e-6 + 2.0 * np.spacing(np.abs(wt)).astype(np.float64)
            worst = max(worst, float((d / bound)[ok].max()))
            assert np.all(d[ok] <= bound[ok]), (tag, k, tg, pk, float((d / bound)[ok].max()))
    print(f"[hyper] {tag} step {k}: Polyak error at most {worst:.2f} of tau * 1e-6 + 2 ulp")


def _run(layout, hset, precision, steps=3, **extra):
    shape, lay = LAYOUTS[layout]
    h = hyper(hset, shape["act"])
    name = f"{layout}_{hset}" + ("_fixed_alpha" if extra.get("auto") is False else "")
    c = dict(shape, name=name, **h, **extra)
    _check_config_against_oracle(c, precision, steps, traj_tol=2e-3, layout=lay, expect=layout,
                                 on_step=_conditions(f"{name}/{precision}", "log_std_min" in h))


@pytest.mark.parametrize("hset", ["rl", "adam"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_hyper_sets_match_oracle(layout, hset):
    _run(layout, hset, "fp32")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_both_sets_with_fixed_alpha_match_oracle(layout):
    """rl+adam with entropy tuning off: alpha stays 0.3 (fp32 of it), which the
    target and the actor's alpha/B seed then read instead of 0.1."""
    _run(layout, "rl+adam", "fp32", auto=False)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bf16_both_sets_match_oracle(layout):
    """rl+adam with bf16 products, with _check_config_against_oracle's bf16 bounds."""
    _run(layout, "rl+adam", "bf16")


def test_large_batch_both_sets_match_oracle():
    """B = 1040 with two batch parts of the update tiles (upd_parts = 2), whose
    Adam scalars are their own copy: rl+adam, fp32, 2 steps.  At this batch
    the planner does not run the role kernels (asserted)."""
    c = dict(LARGE, name="large_rl+adam", **hyper("rl+adam", LARGE["act"]))
    _check_config_against_oracle(c, "fp32", 2, roles=False, traj_tol=2e-3, layout={"upd_parts": 2},
                                 on_step=_conditions("large_rl+adam/fp32", True))
