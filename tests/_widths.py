"""The layer widths of the width parity matrix (no GPU needed): shapes, layout
overrides and the kernel family each case must run, shared by
tests/test_gpu_widths.py, tests/test_widths_cpu.py, tests/test_plan_cpu.py, the
forward-only kernels' tests and tests/golden/make_plan_digests.py.

sac_engine_create takes any hidden width >= 1 and any obs_dim >= 1; the planner
pads every layer to 32 columns, and each kernel family handles the ragged last
tile on its own.  Every other test trains at hidden widths that are multiples
of 8 (300, a multiple of 4, on the stage path only).  The widths here are odd,
one past a pad, one short of it, or 1, and differ between the critics and the
policy at every layer, so a layer read from the other net is a different
matrix."""

S = dict(obs=5, act=3, batch=40, capacity=512)
ODD = dict(q_hidden=[33, 50], pi_hidden=[50, 33])

SHAPES = {
    # one past a pad (33 -> 64); even but no multiple of 4 (50)
    "odd": dict(S, **ODD),
    # one short of a pad (31); one past 64 (65 -> 96)
    "edge": dict(S, q_hidden=[31, 65], pi_hidden=[65, 31]),
    # the API's minimum width: a hidden layer of one unit, a K = 1 reduction behind it
    "tiny": dict(S, q_hidden=[7, 1], pi_hidden=[1, 7]),
    # the common user choice (100 -> 128)
    "h100": dict(S, hidden=[100, 100]),
    # one past 256 (-> 288: a 17th column tile, a second 8-wave pass)
    "w257": dict(S, q_hidden=[257, 31], pi_hidden=[31, 257]),
    # three hidden layers; ragged column blocks on the stage path
    "odd3": dict(S, q_hidden=[33, 50, 17], pi_hidden=[17, 33, 50], batch=72),
    # the update tiles' batch parts (Bp > 1024); the pair tiles by default
    "odd_b1100": dict(S, **ODD, batch=1100, capacity=4096),
    # the stage path by the planner's own choice, both widths odd
    "w401": dict(obs=17, act=6, q_hidden=[401, 299], pi_hidden=[299, 401], batch=40, capacity=512),
    # K = 1 for pi's layer 0, K = 2 for the critics'.  ELU hidden layers: with a one-dimensional input and ReLU,
    # 42 % of pi's layer-1 elements move on the oracle's first step and the last hidden unit's row does not move
    # at all (dead units), so the visibility conditions of tests/test_widths_cpu.py cannot hold
    "obs1": dict(S, obs=1, act=1, **ODD, q_act="elu", pi_act="elu"),
    # the critics' layer-0 K = 32 exactly, pi's 31
    "obs31": dict(S, obs=31, act=1, **ODD),
    # pi's layer-0 K one past the pad, the critics' 35
    "obs33": dict(S, obs=33, act=2, **ODD),
}

ROLES, ROWS, PAIRS, STAGE = {"layout": "roles"}, {"layout": "rows"}, {"layout": "pairs"}, {"stage_path": 1}
FORCED = {"roles": ROLES, "rows": ROWS, "pairs": PAIRS, "stage": STAGE}
ALL4 = [("roles", True), ("rows", True), ("pairs", True), ("stage", True)]

# shape -> [(family, forced?)]
MATRIX = {
    "odd": ALL4,
    "edge": ALL4,
    "tiny": ALL4,
    "h100": ALL4,
    # layout = pairs is refused at this shape (the pair-tile LDS layout does not fit): tests/test_plan_cpu.py
    "w257": [("roles", True), ("rows", True), ("stage", True)],
    "odd3": [("roles", True), ("pairs", True), ("stage", True)],
    "odd_b1100": [("pairs", False), ("rows", True), ("stage", True)],
    "w401": [("stage", False)],
    "obs1": [("roles", False), ("pairs", True)],
    "obs31": [("roles", False), ("pairs", True)],
    "obs33": [("roles", False), ("pairs", True)],
}

# name -> (shape, layout override, the kernel family phases A and C must run)
CASES = {f"{shape}_{family}": (SHAPES[shape], FORCED[family] if forced else None, family)
         for shape, fams in MATRIX.items() for family, forced in fams}

SHAPE_OF = {f"{shape}_{family}": shape for shape, fams in MATRIX.items() for family, _ in fams}

HSETS = ("default", "rl+adam")
# obs1 runs the default set only: with rl+adam (the narrow clamp [-0.1, 0.1]) at act 1 no replay seed of 4..59
# puts >= 5 % of the raw log sigma entries below the clamp, above it and inside it on every step
# (test_gpu_hyper.py::_conditions), and the condition is not the thing to change
DEFAULT_ONLY = ("obs1",)
# Replay seeds other than build_engine's 3, where the rows of seed 3 miss a condition of _conditions
# (tests/test_widths_cpu.py checks them on the oracle).  obs31 with rl+adam: at seed 3, step 1 has 92.5 % of the
# raw log sigma above the narrow clamp and 2.5 % inside (5 % asked); at seed 8 every condition holds on all
# three steps.
#
# The default set (adam_eps 1e-8) at h100 and odd3: Adam's update lr m^ / (sqrt(v^) + eps) of an element whose
# sqrt(v^) is within 10 eps of 0 without being 0 is decided by the summation order of its gradient (slope
# lr eps / (|g| + eps)^2 >= 2.5e2 in g), and _check_config_against_oracle lets 0.1 % of a tensor's elements miss
# 1e-6 against the local oracle: one such element voids a tensor of fewer than 1000.  At seed 3 the oracle's own
# step 1 at h100 has one in Q2's layer 0 (800 elements, |g| = 0.79 eps: its step is 0.44 lr on the oracle, and all
# four kernel families land 6e-6 .. 1.7e-5 from it), and odd3 has one in each critic's layer 2 (850 elements, 1.02
# and 3.65 eps).  tests/test_widths_cpu.py asserts the condition on every shape's default-set steps; the smallest
# replay seeds of 4.. that meet it are 4 (h100) and 9 (odd3).  The rows then come from tests/_gpu.py::synthetic_rows
# with the default replay's own 1 % terminals.
REPLAY_SEED = {("obs31", "rl+adam"): 8, ("h100", "default"): 4, ("odd3", "default"): 9}

# The device-RNG cases of tests/test_gpu_widths.py: odd, tiny and w257 on every family they run.  Device draws
# cannot be redrawn, so the oracle's six steps at this engine seed must be tie-free (tests/test_widths_cpu.py).
RNG_SEED = 0
# tiny runs the device RNG with ELU hidden layers.  Biases start at 0, so wherever pi's one-unit ReLU layer gives 0
# every pre-activation of the layer behind it is exactly 0, which tests/_ties.py counts as a tie (|p| <= 0): 35..80
# tied rows on step 0 at every engine seed of 0..59, and a unit behind a negative weight keeps its zero bias for
# good.  The injected draws redraw those rows (110 on step 1); device draws cannot, and no seed is tie-free.  ELU
# has no kinked decision, and the widths, the K = 1 reduction and the samplers are the same.
RNG_SHAPES = {"odd": SHAPES["odd"], "tiny": dict(SHAPES["tiny"], q_act="elu", pi_act="elu"), "w257": SHAPES["w257"]}
RNG_CASES =tuple(f"{shape}_{family}" for shape in ("odd", "tiny", "w257") for family, _ in MATRIX[shape])


def hsets(case):
    """The hyper-parameter sets a case runs."""
    return ("default",) if SHAPE_OF[case] in DEFAULT_ONLY else HSETS


def steps(shape):
    """fp32 steps of a shape dict: 2 at B > 1024, as the edge shapes do, else 3."""
    return 2 if shape["batch"] > 1024 else 3


def config(case, hset):
    """The config dict of tests/_gpu.py::build_engine for a case and a
    hyper-parameter set ("default" or test_gpu_hyper.py's "rl+adam")."""
    from test_gpu_hyper import hyper

    assert hset in hsets(case), (case, hset)
    shape = CASES[case][0]
    if hset == "default":
        if (SHAPE_OF[case], hset) in REPLAY_SEED:
            return dict(shape, name=case, done_p=0.01, replay_seed=REPLAY_SEED[SHAPE_OF[case], hset])
        return dict(shape, name=case)
    c = dict(shape, name=f"{case}_{hset}", **hyper(hset, shape["act"]))
    if (SHAPE_OF[case], hset) in REPLAY_SEED:
        c["replay_seed"] = REPLAY_SEED[SHAPE_OF[case], hset]
    return c


def edge_slices(W, b):
    """The edge elements of one network's parameters, W[l] of shape [N_l][K_l]:
    layer 0's last input column W[0][:, K - 1], and for every hidden layer l of
    width N the last unit's row W[l][N - 1, :], its bias b[l][N - 1] and the
    column that reads it, W[l + 1][:, N - 1].  Returns [(label, "W" | "b",
    layer, the index into that tensor, N or None for the input column)]."""
    out = [("W0[:, K-1]", "W", 0, (slice(None), W[0].shape[1] - 1), None)]
    for l in range(len(W) - 1):
        n = W[l].shape[0]
        assert b[l].shape == (n,) and W[l + 1].shape[1] == n
        out += [(f"W{l}[N-1, :]", "W", l, (n - 1, slice(None)), n), (f"b{l}[N-1]", "b", l, (slice(n - 1, n),), n),
                (f"W{l + 1}[:, N-1]", "W", l + 1, (slice(None), n - 1), n)]
    return out
