"""The acting head, target, seed and min-Q arithmetic without a GPU: csrc/sac_math.h
holds the functions that sac_policy_act_kernel, the rollout step and the stage
path call, and sac_debug_head_host is that header compiled for the host.

Exact checks (no tolerance): the tie rule and NaN propagation of the min-Q
weights, the clamp of log sigma at and beyond both bounds, the deterministic
action, and y == r where d == 1.

Value checks on a fixed grid.  The host's exp / tanh / log1p are libm's, not
numpy's, so equality is not expected; the bound comes from the float32 oracle's
own rounding error.  The same formulas (reference sac/models.py:79-87,
sac/agent.py:195-211 and 244-257) are evaluated in float64; for each output
quantity E32 = max |float32 oracle - float64| and the assertion is
max |host export - float64| <= 4 E32: one to two ulp per transcendental feeding
the same short chain.  Where E32 is 0 the assertion is equality.  z and the
action are oracle/sac_oracle.py's policy_sample through a single-layer identity
network; the target, seed and min-Q lines are its training_step's, restated
below because it returns none of them separately.  The acting log pi terms are
a form the oracle does not compute and have a bound of their own.  Measured
ratios: profiles/head_math_cpu.txt."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from oracle import sac_oracle as O

F32, F64 = np.float32, np.float64
LO, HI, SCALE, GAMMA, ALPHA, B = -20.0, 2.0, 2.0, 0.99, 0.2, 256
f32p, i32, f32 = ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_float


def _enums():
    text = open(os.path.join(ROOT, "include", "sac_engine_testing.h")).read()
    blocks = [re.findall(r"SAC_HEAD_\w+", b) for b in re.findall(r"enum \{([^}]*SAC_HEAD_[^}]*)\}", text)]
    assert len(blocks) == 2 and blocks[0][-1] == "SAC_HEAD_NIN" and blocks[1][-1] == "SAC_HEAD_NOUT"
    return ([n[len("SAC_HEAD_IN_"):].lower() for n in blocks[0][:-1]],
            [n[len("SAC_HEAD_"):].lower() for n in blocks[1][:-1]])


IN, OUT = _enums()


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_head_host.argtypes = [i32, f32p, f32, f32, f32, f32, f32, i32, f32p]
    lb.sac_debug_head_host.restype = ctypes.c_int
    return lb


def head_host(lib, lo=LO, hi=HI, scale=SCALE, gamma=GAMMA, alpha=ALPHA, batch=B, **cols):
    """The export on arrays; inputs not given are zero.  Returns {output name: float32 [n]}."""
    n = max(np.size(v) for v in cols.values())
    x = np.zeros((len(IN), n), F32)
    for k, v in cols.items():
        x[IN.index(k)] = v
    out = np.full((len(OUT), n), np.nan, F32)
    rc = lib.sac_debug_head_host(n, x.ctypes.data_as(f32p), lo, hi, scale, gamma, alpha, batch,
                                 out.ctypes.data_as(f32p))
    assert rc == 0, lib.sac_last_error().decode()
    return dict(zip(OUT, out))


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


# ----------------------------------------------------------------------------- exact checks
def test_minq_ties_order_and_nan(lib):
    gm = F32(-1.0) / F32(B)
    q1 = np.array([1.5, 0.0, -0.0, -3.25, 2.0, -1.0, 1e-30, np.nan, np.nan], F32)
    q2 = np.array([1.5, -0.0, 0.0, -3.25, 1.0, -0.5, 2e-30, 0.0, np.nan], F32)
    o = head_host(lib, q1=q1, q2=q2)
    tie, gt, lt = slice(0, 4), slice(4, 5), slice(5, 7)
    half = F32(gm * F32(0.5))
    assert (bits(o["w1"][tie]) == bits(half)).all() and (bits(o["w2"][tie]) == bits(half)).all()
    assert (bits(o["w1"][gt]) == bits(F32(0))).all() and (bits(o["w2"][gt]) == bits(gm)).all()
    assert (bits(o["w1"][lt]) == bits(gm)).all() and (bits(o["w2"][lt]) == bits(F32(0))).all()
    assert (o["minq"][:7] == np.minimum(q1, q2)[:7]).all()
    assert np.isnan(o["minq"][7:]).all()  # a NaN in q1 makes m NaN
    assert np.isnan(head_host(lib, q1=F32(0), q2=F32(np.nan))["minq"]).all()  # torch.min: in q2 as well


def test_clamp_at_and_beyond_the_bounds(lib):
    lo, hi = F32(LO), F32(HI)
    lsr = np.array([np.nextafter(lo, F32(-np.inf)), lo - 5, lo, np.nextafter(lo, F32(np.inf)), 0.0,
                    np.nextafter(hi, F32(-np.inf)), hi, np.nextafter(hi, F32(np.inf)), hi + 5], F32)
    o = head_host(lib, mu=F32(0.3), lsr=lsr, e=F32(0.5))
    assert (bits(o["ls"]) == bits(np.clip(lsr, lo, hi))).all()
    assert (o["ls"][:2] == lo).all() and (o["ls"][-2:] == hi).all()


# The grid of the value checks: z on both sides of the softplus threshold -2z = 20 (mu = -9.5 / -10.5), lsr below,
# at, inside and above the clamp, e = 0, and |mu| large against sd (mu = 50, -80 at every lsr level).
MU = np.array([0.0, 0.3, -1.7, 4.0, -9.5, -10.5, 50.0, -80.0], F32)
LSR = np.array([-25.0, -20.0, -3.0, 0.0, 1.0, 2.0, 3.5], F32)
EPS = np.array([0.0, 0.5, -1.3, 2.5], F32)
PER_LEVEL = MU.size * EPS.size


def grid():
    lsr, mu, e = (a.ravel() for a in np.meshgrid(LSR, MU, EPS, indexing="ij"))
    n = lsr.size
    cyc = lambda *v: np.resize(np.array(v, F32), n)
    return dict(mu=mu, lsr=lsr, e=e,
                q1=cyc(1.5, -2.0, 0.25, 0.25, 7.0, -1e-3, 40.0), q2=cyc(1.5, -1.0, 0.5, 0.25, -7.0, -2e-3, 40.0),
                r=cyc(0.0, 1.0, -0.5, 3.25), d=cyc(0.0, 1.0, 0.0), lp=cyc(-1.2, 0.4, 3.3, -7.5, 0.0, 11.0))


def test_grid_is_what_it_claims(lib):
    g = grid()
    o = head_host(lib, **g)
    assert np.isfinite(np.stack(list(o.values()))).all()
    assert (-2 * o["act_z"] > 20).any() and (-2 * o["act_z"] < 20).any() and (g["e"] == 0).any()
    assert (g["q1"] == g["q2"]).any() and (g["q1"] < g["q2"]).any() and (g["q1"] > g["q2"]).any()


def test_deterministic_action_ignores_lsr_and_e(lib):
    """Holds by head_act_mean's signature (mu and scale only) as long as the export calls it; what can fail
    here is the value: tanh(mu) * scale within the two roundings of the float32 chain."""
    g = grid()
    a = head_host(lib, **g)["act_mean"]
    b = head_host(lib, mu=g["mu"], lsr=g["lsr"][::-1].copy(), e=(g["e"] + F32(7)))["act_mean"]
    assert (bits(a) == bits(b)).all()
    assert (bits(a) == bits(head_host(lib, mu=g["mu"])["act_mean"])).all()
    want = np.tanh(g["mu"].astype(F64)) * SCALE  # |tanh| <= 1: libm's tanhf within 2 ulp of 1, the product half an ulp
    assert (np.abs(a.astype(F64) - want) <= 2.5 * 2.0 ** -24 * SCALE).all()


def test_done_rows_bootstrap_nothing(lib):
    g = grid()
    y = head_host(lib, **dict(g, d=np.ones_like(g["d"])))["y"]
    assert (bits(y) == bits(g["r"])).all()


# ----------------------------------------------------------------------------- value checks
def softplus64(x):  # torch softplus(beta=1, threshold=20)
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def reference64(g):
    """models.py:79-84, agent.py:195-211, 225 and 244-252 in float64 on float32 inputs."""
    mu, lsr, e = (g[k].astype(F64) for k in ("mu", "lsr", "e"))
    q1, q2, r, d, lpn = (g[k].astype(F64) for k in ("q1", "q2", "r", "d", "lp"))
    lo, hi, scale, alpha, gamma = (F64(F32(v)) for v in (LO, HI, SCALE, ALPHA, GAMMA))
    z = mu + e * np.exp(np.clip(lsr, lo, hi))
    m = np.minimum(q1, q2)
    y = r + gamma * (1 - d) * (m - alpha * lpn)
    gm = F64(F32(-1.0) / F32(B))
    return dict(act_z=z, act_act=np.tanh(z) * scale, y=y, seed_d=q1 - y, seed=F64(F32(2.0 / B)) * (q1 - y), minq=m,
                pi_term=alpha * lpn - m, w1=np.where(q1 == q2, gm / 2, np.where(q1 < q2, gm, 0.0)),
                w2=np.where(q1 == q2, gm / 2, np.where(q2 < q1, gm, 0.0)))


def oracle32(g):
    """The float32 oracle: policy_sample through pi(s) = s (rows of one action dim), and the target, seed and
    min-Q lines of training_step."""
    n = g["mu"].size
    pi = O.MLP([np.eye(2, dtype=F32)], [np.zeros(2, F32)])
    s = np.stack([g["mu"], g["lsr"]], axis=1)
    a, _, ctx = O.policy_sample(pi, s, g["e"].reshape(n, 1), O.PolicyCfg(LO, HI, SCALE))
    alpha32 = F32(ALPHA)
    q1, q2, r, d, lpn = (g[k] for k in ("q1", "q2", "r", "d", "lp"))
    minq = np.minimum(q1, q2)
    y = (r + (F32(GAMMA) * (F32(1) - d)) * (minq - alpha32 * lpn)).astype(F32)  # training_step: the target
    diff = q1 - y
    g_min = np.full(q1.size, F32(-1.0 / B), F32)  # training_step: the min-Q backward
    tie = q1 == q2
    return dict(act_z=ctx["z"][:, 0], act_act=a[:, 0], y=y, seed_d=diff, seed=(F32(2.0 / B) * diff).astype(F32),
                minq=minq, pi_term=(alpha32 * lpn - minq).astype(F32),
                w1=np.where(tie, g_min / F32(2), np.where(q1 < q2, g_min, F32(0))).astype(F32),
                w2=np.where(tie, g_min / F32(2), np.where(q2 < q1, g_min, F32(0))).astype(F32))


def check_within_oracle_error(tag, got, orc, ref, keys):
    worst = {}
    for k in keys:
        e32 = float(np.max(np.abs(orc[k].astype(F64) - ref[k])))
        err = float(np.max(np.abs(got[k].astype(F64) - ref[k])))
        worst[k] = err / e32 if e32 > 0 else (0.0 if err == 0 else math.inf)
        print(f"{tag} {k:8s} E32={e32:.3e} host={err:.3e} ratio={worst[k]:.3f}")
        if e32 == 0:
            assert (got[k].astype(F64) == ref[k]).all(), (tag, k)
        else:
            assert err <= 4 * e32, (tag, k, err, e32)
    return worst


def test_values_against_the_oracle_within_its_own_error(lib):
    g = grid()
    ref = reference64(g)
    check_within_oracle_error("grid", head_host(lib, **g), oracle32(g), ref, list(ref))


def test_head_values_inside_each_log_sigma_level(lib):
    """The same bound with both maxima taken inside each log-sigma level: z's error scales with sd."""
    g = grid()
    host = head_host(lib, **g)
    for lv in range(LSR.size):
        sl = slice(lv * PER_LEVEL, (lv + 1) * PER_LEVEL)
        gs = {k: v[sl] for k, v in g.items()}
        check_within_oracle_error(f"lsr={LSR[lv]:5.1f}", {k: v[sl] for k, v in host.items()}, oracle32(gs),
                                  reference64(gs), ("act_z", "act_act"))


def test_acting_log_pi_terms(lib):
    """The acting form takes (z - mu)^2 / (2 sd^2) + log sd as e^2 / 2 + ls, which the oracle does not compute, so
    its bound is the format's: three float32 operations and the rounded constant, each within half an ulp of a
    magnitude no larger than e^2 / 2 + |ls| + c, so 4 * 2^-24 of that sum in all.  Its tanh correction
    2 (log 2 - z - softplus(-2z)) is models.py:86's, within 4x the float32 oracle formula's own error against float64."""
    g = grid()
    o = head_host(lib, **g)
    z = o["act_z"]
    c64 = 2 * (math.log(2.0) - z.astype(F64) - softplus64(-2 * z.astype(F64)))
    c32 = (F32(2) * (O._LOG2 - z - O.softplus(F32(-2) * z))).astype(F32)  # policy_sample's line on the same z
    check_within_oracle_error("corr", dict(c=o["act_corr"]), dict(c=c32), dict(c=c64), ("c",))
    e, ls, c = g["e"].astype(F64), np.clip(g["lsr"], F32(LO), F32(HI)).astype(F64), math.log(math.sqrt(2 * math.pi))
    err = np.abs(o["act_lp"].astype(F64) - (-0.5 * e * e - ls - c))
    bound = 4 * 2.0 ** -24 * (0.5 * e * e + np.abs(ls) + c)
    print(f"acting lp: worst error / bound = {float(np.max(err / bound)):.3f}")
    assert (err <= bound).all()
