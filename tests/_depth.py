"""The network depths of the depth parity matrix (no GPU needed): shapes,
layout overrides and the kernel family each case must run, shared by
tests/test_gpu_depth.py, tests/test_depth_cpu.py, tests/test_plan_cpu.py, the
forward-only kernels' tests and tests/golden/make_plan_digests.py.

sac_engine_create takes one to five hidden layers per network, the critics'
depth independent of the policy's.  The small shapes use widths that pad
(72 -> 96, 40 -> 64, 56 -> 64, 24 -> 32, 88 -> 96, 48 -> 64) and differ
between the nets at every layer, so a layer read from the other net, or from
the slot next to its own, is a different matrix."""

S = dict(obs=5, act=3, batch=40, capacity=512)
Q5 = [72, 40, 56, 24, 88]
P5 = [40, 72, 24, 56, 48]
W256 = dict(obs=24, act=4, capacity=512)

SHAPES = {
    "h1": dict(S, q_hidden=Q5[:1], pi_hidden=P5[:1]),
    "h4": dict(S, q_hidden=Q5[:4], pi_hidden=P5[:4]),
    "h5": dict(S, q_hidden=Q5, pi_hidden=P5),
    "q1_pi3": dict(S, q_hidden=Q5[:1], pi_hidden=P5[:3]),
    "q5_pi1": dict(S, q_hidden=Q5, pi_hidden=P5[:1]),
    "q2_pi5": dict(S, q_hidden=Q5[:2], pi_hidden=P5),
    "q5_pi2": dict(S, q_hidden=Q5, pi_hidden=P5[:2]),
    # one hidden layer of 256: the hidden split refused by depth
    "h1_256": dict(W256, hidden=[256], batch=40),
    # five of 256: past the R-row LDS layout, the stage path by default
    "h5_256": dict(W256, hidden=[256] * 5, batch=72),
    # 69 row tiles, the last one ragged; Bp > 1024: the update tiles run in batch parts
    "h5_b1100": dict(S, q_hidden=Q5, pi_hidden=P5, batch=1100, capacity=4096),
    "h1_b1100": dict(S, q_hidden=Q5[:1], pi_hidden=P5[:1], batch=1100, capacity=4096),
}

ROLES, ROWS, PAIRS, STAGE = {"layout": "roles"}, {"layout": "rows"}, {"layout": "pairs"}, {"stage_path": 1}
FORCED = {"roles": ROLES, "rows": ROWS, "pairs": PAIRS, "stage": STAGE}

# shape -> [(family, forced?)]: every family at depth 1 and at depth 5, the
# unequal depths on the families whose code separates the two nets' depths
MATRIX = {
    "h1": [("roles", True), ("rows", True), ("pairs", True)],
    "q1_pi3": [("roles", True), ("rows", True), ("pairs", True)],
    "q5_pi1": [("roles", True), ("rows", True), ("pairs", True)],
    "h4": [("roles", True), ("stage", True)],
    "h5": [("roles", True), ("rows", True), ("pairs", True), ("stage", True)],
    "q2_pi5": [("pairs", True), ("stage", True)],
    "q5_pi2": [("rows", True), ("stage", True)],
    "h1_256": [("roles", False)],
    "h5_256": [("stage", False)],
    "h5_b1100": [("pairs", False), ("stage", True)],
    "h1_b1100": [("pairs", False), ("rows", True)],
}

# name -> (shape, layout override, the kernel family phases A and C must run)
CASES = {f"{shape}_{family}": (SHAPES[shape], FORCED[family] if forced else None, family)
         for shape, fams in MATRIX.items() for family, forced in fams}

SHAPE_OF = {f"{shape}_{family}": shape for shape, fams in MATRIX.items() for family, _ in fams}

HSETS = ("default", "rl+adam")
# Replay seeds other than build_engine's 3, where the rows of seed 3 miss a
# condition of test_gpu_hyper.py::_conditions (tests/test_depth_cpu.py checks
# them on the oracle).  h4 with rl+adam: the four-layer policy's raw log sigma
# is narrow against the [-0.1, 0.1] clamp, and at seed 3 only 3.3 % of step 3's
# entries lie above it (5 % asked); 14 is the smallest seed of 3..399 that
# clears 5 % with room on all three steps (6.7 %).
REPLAY_SEED = {("h4", "rl+adam"): 14}


def config(case, hset):
    """The config dict of tests/_gpu.py::build_engine for a case and a
    hyper-parameter set ("default" or test_gpu_hyper.py's "rl+adam")."""
    from test_gpu_hyper import hyper

    shape = CASES[case][0]
    if hset == "default":
        return dict(shape, name=case)
    c = dict(shape, name=f"{case}_{hset}", **hyper(hset, shape["act"]))
    if (SHAPE_OF[case], hset) in REPLAY_SEED:
        c["replay_seed"] = REPLAY_SEED[SHAPE_OF[case], hset]
    return c
