"""The engine's launch plan on the CPU (no GPU needed): sac_engine_create runs
the whole planner -- phase layouts, update tiles with their batch parts and
bias blocks, the stage path's job list -- before its first HIP call.  On a
machine without a GPU it must therefore stop at that first HIP call
(SAC_E_HIP), never at the planner's own consistency check ("internal: ...",
SAC_E_INVALID): a mismatch between the tiles the planner counts (the grids of
phases B and D) and the tiles it builds would make the update kernels read
descriptors that do not exist.  Every bench config, both precisions, and the
diagnostic layouts sac_engine_config's override fields select (the library
reads no environment: tested on its dynamic symbol table)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "soft-actor-critic_amd"))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sac import _engine as E  # noqa: E402

SAC_E_INVALID, SAC_E_HIP = -1, -2


def _cfg(name, precision):
    return _cfg_of(bench.CONFIGS[name], precision)


def _cfg_of(c, precision):
    """sac_engine_config of a config dict: hidden (or q_hidden / pi_hidden),
    and optionally q_act, pi_act, q_out_act, pi_out_act (sac.models names),
    auto, log_std_min / log_std_max: the fields of tests/_gpu.py::build_engine."""
    from sac.models import ACT_CODES

    cfg = E.EngineConfig()
    cfg.obs_dim, cfg.act_dim, cfg.batch = c["obs"], c["act"], c["batch"]
    qd = [c["obs"] + c["act"]] + c.get("q_hidden", c.get("hidden")) + [1]
    pd = [c["obs"]] + c.get("pi_hidden", c.get("hidden")) + [2 * c["act"]]
    cfg.q_layers, cfg.pi_layers = len(qd) - 1, len(pd) - 1
    for i, d in enumerate(qd):
        cfg.q_dims[i] = d
    for i, d in enumerate(pd):
        cfg.pi_dims[i] = d
    cfg.q_hidden_act, cfg.pi_hidden_act = ACT_CODES[c.get("q_act", "relu")], ACT_CODES[c.get("pi_act", "relu")]
    cfg.q_out_act, cfg.pi_out_act = ACT_CODES[c.get("q_out_act", "identity")], ACT_CODES[c.get("pi_out_act", "identity")]
    cfg.gamma, cfg.tau = 0.99, 0.005
    cfg.log_std_min, cfg.log_std_max, cfg.action_scale = c.get("log_std_min", -20.0), c.get("log_std_max", 2.0), 1.0
    cfg.actor_lr = cfg.critic_lr = cfg.alpha_lr = 3e-4
    cfg.beta1, cfg.beta2, cfg.adam_eps = 0.9, 0.999, 1e-8
    cfg.auto_entropy, cfg.target_entropy = int(c.get("auto", True)), -float(c["act"])
    cfg.precision = E.PREC_FP32 if precision == "fp32" else E.PREC_BF16
    cfg.seed = 0
    return cfg


@pytest.mark.parametrize("override", ["", "stage_batch=-1", "layout=1", "layout=2", "layout=3",
                                      "layout=3,upd_threads=512", "upd_parts=4", "upd_threads=1024",
                                      "stage_path=1", "stage_path=-1"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(bench.CONFIGS))
def test_plan_is_consistent(name, precision, override):
    lib = E.load_library()
    cfg = _cfg(name, precision)
    for kv in filter(None, override.split(",")):
        k, v = kv.split("=")
        setattr(cfg, k, int(v))
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    assert ws > 0, lib.sac_last_error()
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, ws)  # never dereferenced before the first HIP call
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    msg = lib.sac_last_error().decode()
    if rc == 0:  # a GPU is present: the engine exists; destroy it
        lib.sac_engine_destroy(out)
        pytest.skip("GPU present: the planner ran for real")
    assert "internal" not in msg, msg
    if cfg.layout and rc == SAC_E_INVALID:  # an explicit layout the shape cannot take fails, never falls back
        assert "layout override cannot be honoured" in msg, msg
        assert (name, cfg.layout) in HONOUR_REFUSED, (name, cfg.layout, msg)
        return
    assert (name, cfg.layout) not in HONOUR_REFUSED, (name, cfg.layout)
    assert rc == SAC_E_HIP, (rc, msg)


# (config, forced layout) pairs the planner cannot honour: the per-network role
# kernels need 6 workgroups per row tile co-resident (C3: 256 row tiles); the
# row and pair tiles hold 2R rows of every layer, which at obs 216 (C4') does
# not fit the CU's LDS (that config runs the role kernels by default)
HONOUR_REFUSED = {("c3", 1), ("c4w", 2), ("c4w", 3)}


def test_unhonourable_layout_override_fails():
    """layout=roles at C3 (1536 role workgroups > 256 CUs) used to
    fall back silently to other kernels; it now fails in create with
    SAC_E_INVALID, before any HIP call, like stage_path = -1 on a shape that
    needs the stage path."""
    lib = E.load_library()
    cfg = _cfg("c3", "fp32")
    cfg.layout = 1
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, ws)
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    if rc == 0:
        lib.sac_engine_destroy(out)
        pytest.fail("layout=roles honoured at C3")
    assert rc == SAC_E_INVALID and "cannot be honoured: roles" in lib.sac_last_error().decode()


def _activation_cases():
    """The shapes, layout overrides and activations of tests/test_gpu_activations.py."""
    import test_gpu_activations as GA

    shapes = dict(GA.LAYOUTS, **{"stage_" + k: v for k, v in GA.STAGE_SHAPES.items()})
    acts = {"elu_elu": dict(q_act="elu", pi_act="elu"), "relu_tanh": dict(q_act="relu", pi_act="tanh"),
            "elu_relu": dict(q_act="elu", pi_act="relu"), "selu_leaky": dict(q_act="selu", pi_act="leaky_relu"),
            "fixed_alpha": dict(q_act="elu", pi_act="elu", auto=False),
            "relu_out_smooth": dict(GA.OUT_ACTS["smooth"]), "relu_out_kink": dict(GA.OUT_ACTS["kink"]),
            "tanh_gelu_out_smooth": dict(GA.OUT_ACTS["smooth"], q_act="tanh", pi_act="gelu"),
            "elu_elu_q_out_only": dict(GA.OUT_ACTS["smooth"], q_act="elu", pi_act="elu", pi_out_act="identity")}
    return [(s, a, dict(shapes[s][0], **acts[a]), shapes[s][1]) for s in sorted(shapes) for a in sorted(acts)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,acts,c,lay", _activation_cases(), ids=[f"{s}-{a}" for s, a, _, _ in _activation_cases()])
def test_activation_matrix_plans(shape, acts, c, lay, precision):
    """The shapes of the GPU activation matrix with non-ReLU and output
    activation codes, their layout overrides, both precisions: the planner
    accepts each one (no "internal", no refused override) and creation stops at
    its first HIP call."""
    lib = E.load_library()
    cfg = _cfg_of(c, precision)
    for k, v in (lay or {}).items():
        setattr(cfg, k, E.LAYOUTS[v] if k == "layout" else int(v))
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    assert ws > 0, lib.sac_last_error()
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, ws)  # never dereferenced before the first HIP call
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    msg = lib.sac_last_error().decode()
    if rc == 0:  # a GPU is present: the engine exists; destroy it
        lib.sac_engine_destroy(out)
        pytest.skip("GPU present: the planner ran for real")
    assert "internal" not in msg, msg
    assert rc == SAC_E_HIP, (rc, msg)


@pytest.mark.parametrize("shape,needs", [("w288", False), ("w384", True)])
def test_stage_path_is_the_planners_choice_only_past_the_lds_layout(shape, needs):
    """With the stage path refused (stage_path = -1) creation fails in the
    planner exactly for the shape that needs it: [384, 384] critics do not fit
    the phase kernels' LDS layout, [288, 40] at B = 40 does (it runs the role
    kernels unless the stage path is forced)."""
    import test_gpu_activations as GA

    cfg = _cfg_of(dict(GA.STAGE_SHAPES[shape][0], q_act="elu", pi_act="elu"), "fp32")
    cfg.stage_path = -1
    lib = E.load_library()
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, max(ws, 1))
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    msg = lib.sac_last_error().decode()
    if rc == 0:
        lib.sac_engine_destroy(out)
        pytest.skip("GPU present: the planner ran for real")
    if needs:
        assert rc == SAC_E_INVALID and "B of LDS per workgroup (max 163840)" in msg, (rc, msg)
    else:
        assert rc == SAC_E_HIP and "internal" not in msg, (rc, msg)


def _create_rc(obs, act, hidden, batch=64):
    bench.CONFIGS["_wide"] = dict(obs=obs, act=act, hidden=hidden, batch=batch, capacity=256)
    try:
        cfg = _cfg("_wide", "fp32")
    finally:
        del bench.CONFIGS["_wide"]
    lib = E.load_library()
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, ws)
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    if rc == 0:
        lib.sac_engine_destroy(out)
        pytest.skip("GPU present: the planner ran for real")
    return rc, lib.sac_last_error().decode()


@pytest.mark.parametrize("obs,act,hidden", [(300, 6, [256, 256]), (24, 4, [512, 512]), (24, 4, [384, 384]),
                                            (17, 6, [400, 300]), (24, 4, [1024, 1024, 512])])
def test_shapes_past_the_lds_layout_take_the_stage_path(obs, act, hidden):
    """Widths whose phase-kernel workgroup would need more than the CU's 160 KiB
    of LDS (hidden layers past 256, inputs past 256 with [256, 256] nets) are
    planned on the layer-synchronous stage path (csrc/sac_wide.h), which takes
    any width: the planner succeeds and creation stops at its first HIP call."""
    rc, msg = _create_rc(obs, act, hidden)
    assert "internal" not in msg, msg
    assert rc == SAC_E_HIP, (rc, msg)


def test_one_wide_hidden_layer_is_refused():
    """A single hidden layer too wide for the phase kernels' LDS (the stage path
    needs two hidden layers) fails in sac_engine_create with SAC_E_INVALID and
    the byte count, before any HIP call."""
    rc, msg = _create_rc(24, 4, [1024])
    assert rc == SAC_E_INVALID and "B of LDS per workgroup (max 163840)" in msg, (rc, msg)


@pytest.mark.parametrize("field,value", [("layout", 4), ("stage_path", 2), ("stage_batch", 1), ("upd_parts", 5),
                                         ("upd_threads", 256)])
def test_bad_layout_override_is_refused(field, value):
    """Out-of-range override fields fail validation (SAC_E_INVALID) in both the
    workspace query and create, before any HIP call."""
    lib = E.load_library()
    cfg = _cfg("c2", "fp32")
    setattr(cfg, field, value)
    assert lib.sac_engine_workspace_bytes(ctypes.byref(cfg)) == 0
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, 1 << 30)
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    assert rc == SAC_E_INVALID and "layout override" in lib.sac_last_error().decode()


def _plan(c, precision, **overrides):
    """(rc, the plan's "path" or the error message) of a config dict through
    the host-only planner export (sac_debug_plan_host, include/
    sac_engine_testing.h: no HIP call, with or without a GPU)."""
    import json

    rc, text = _plan_text(c, precision, **overrides)
    return rc, json.loads(text)["path"] if rc == 0 else text


def _plan_text(c, precision, **overrides):
    """(rc, the export's whole JSON text or the error message)."""
    lib = E.load_library()
    lib.sac_debug_plan_host.restype = ctypes.c_int
    lib.sac_debug_plan_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.c_int32, ctypes.c_char_p,
                                        ctypes.c_size_t]
    cfg = _cfg_of(c, precision)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    buf = ctypes.create_string_buffer(1 << 16)
    rc = lib.sac_debug_plan_host(ctypes.byref(cfg), 256, buf, len(buf))
    return rc, (buf.value if rc == 0 else lib.sac_last_error()).decode()


PADH = dict(obs=5, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40)  # tests/test_gpu_action_width.py's small shape


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_hidden_split_takes_two_act_up_to_32(precision):
    """[256, 256] nets at obs 24: 2 act = 32 output columns still run the
    hidden-split kernels, 34 the role kernels without the split."""
    c = dict(obs=24, hidden=[256, 256], batch=64)
    assert _plan(dict(c, act=16), precision) == (0, "split")
    assert _plan(dict(c, act=17), precision) == (0, "roles")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage_path_override_is_ignored_past_act_8(precision):
    """stage_path = 1 forces the stage path up to 2 act = 16 (its head's
    column limit); at act 9 the same shape is created all the same and runs
    the role kernels: the override is ignored, not refused."""
    assert _plan(dict(PADH, act=8), precision, stage_path=1) == (0, "wide")
    assert _plan(dict(PADH, act=9), precision, stage_path=1) == (0, "roles")
    assert _plan(dict(PADH, act=9), precision) == (0, "roles")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layout,path", [(1, "roles"), (2, "rows"), (3, "pairs")])
def test_act_32_is_planned_on_every_forced_layout(layout, path, precision):
    assert _plan(dict(PADH, act=32), precision, layout=layout) == (0, path)


def test_act_33_is_refused():
    rc, msg = _plan(dict(PADH, act=33), "fp32")
    assert rc == SAC_E_INVALID and "act_dim <= 32" in msg, (rc, msg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [dict(obs=24, hidden=[512, 512], batch=64, act=9),
                                   dict(obs=376, hidden=[256, 256], batch=64, act=17)], ids=["w512_act9", "humanoid"])
def test_shapes_past_the_lds_layout_need_act_up_to_8(shape, precision):
    """Past the phase kernels' LDS layout only the stage path is left, and it
    takes 2 act <= 16: [512, 512] runs it at act 8 and is refused at act 9, as
    is obs 376 / act 17 with [256, 256] nets (Humanoid's shape), with
    SAC_E_INVALID and the LDS byte count."""
    if shape["hidden"] == [512, 512]:
        assert _plan(dict(shape, act=8), precision) == (0, "wide")
    rc, msg = _plan(shape, precision)
    assert rc == SAC_E_INVALID and "B of LDS per workgroup (max 163840)" in msg, (rc, msg)


# ---------------------------------------------------------------- network depths (tests/_depth.py)
PATH_OF = {"roles": "roles", "rows": "rows", "pairs": "pairs", "stage": "wide"}
DEPTH_SMALL = ("h1", "h4", "h5", "q1_pi3", "q5_pi1", "q2_pi5", "q5_pi2")  # obs 5, act 3, B = 40


def _depth_paths():
    """(id, shape name, overrides, the planner's path): the small shapes by
    default and on each forced layout; stage_path = 1, honoured where both
    nets have two hidden layers or more and ignored elsewhere; the 256-wide
    and the B = 1100 shapes; and every case of the GPU matrix."""
    import _depth

    t = []
    for s in DEPTH_SMALL:
        t += [(f"{s}/default", s, {}, "roles"), (f"{s}/layout=1", s, {"layout": 1}, "roles"),
              (f"{s}/layout=2", s, {"layout": 2}, "rows"), (f"{s}/layout=3", s, {"layout": 3}, "pairs")]
    t += [(f"{s}/stage_path=1", s, {"stage_path": 1}, "wide") for s in ("h4", "h5", "q2_pi5", "q5_pi2")]
    t += [(f"{s}/stage_path=1", s, {"stage_path": 1}, "roles") for s in ("h1", "q1_pi3", "q5_pi1")]
    t += [("h1_256/default", "h1_256", {}, "roles"),  # the hidden split refused by depth
          ("h5_256/default", "h5_256", {}, "wide"),  # the R-row layout does not fit
          ("h1_b1100/default", "h1_b1100", {}, "pairs"), ("h1_b1100/stage_path=1", "h1_b1100", {"stage_path": 1}, "pairs"),
          ("h5_b1100/default", "h5_b1100", {}, "pairs")]
    for case, (shape, lay, family) in sorted(_depth.CASES.items()):
        kv = {k: E.LAYOUTS[v] if k == "layout" else int(v) for k, v in (lay or {}).items()}
        t.append((f"case/{case}", _depth.SHAPE_OF[case], kv, PATH_OF[family]))
    return t


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,kv,path", [p[1:] for p in _depth_paths()], ids=[p[0] for p in _depth_paths()])
def test_depths_1_to_5_are_planned_on_the_expected_path(shape, kv, path, precision):
    import _depth

    assert _plan(_depth.SHAPES[shape], precision, **kv) == (0, path)


# ---------------------------------------------------------------- layer widths off the 8-column grid (tests/_widths.py)
def _width_paths():
    """(id, shape name, overrides, the planner's path): every shape of the
    width matrix as the engine plans it by default, and every case of the GPU
    matrix on its override."""
    import _widths

    default = {"odd": "roles", "edge": "roles", "tiny": "roles", "h100": "roles", "w257": "roles", "odd3": "roles",
               "odd_b1100": "pairs", "w401": "wide", "obs1": "roles", "obs31": "roles", "obs33": "roles"}
    assert sorted(default) == sorted(_widths.SHAPES)
    t = [(f"{s}/default", s, {}, p) for s, p in sorted(default.items())]
    for case, (shape, lay, family) in sorted(_widths.CASES.items()):
        kv = {k: E.LAYOUTS[v] if k == "layout" else int(v) for k, v in (lay or {}).items()}
        t.append((f"case/{case}", _widths.SHAPE_OF[case], kv, PATH_OF[family]))
    return t


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,kv,path", [p[1:] for p in _width_paths()], ids=[p[0] for p in _width_paths()])
def test_odd_widths_are_planned_on_the_expected_path(shape, kv, path, precision):
    import _widths

    assert _plan(_widths.SHAPES[shape], precision, **kv) == (0, path)
    rc, msg = _create(_cfg_of(_widths.SHAPES[shape], precision), **kv)
    assert rc == SAC_E_HIP and "internal" not in msg, (shape, kv, rc, msg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pair_tiles_are_refused_one_past_256(precision):
    """layout = pairs at [257, 31] | [31, 257]: 257 pads to 288 columns, and
    the pair tiles' LDS layout does not fit; the override fails in the planner
    and names the cause, it does not fall back."""
    import _widths

    rc, msg = _plan(_widths.SHAPES["w257"], precision, layout=3)
    assert rc == SAC_E_INVALID and "pairs (the pair-tile LDS layout or record does not fit)" in msg, (rc, msg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage_path_override_is_ignored_at_one_hidden_layer(precision):
    """stage_path = 1 where a net has one hidden layer: the same plan as
    without it, byte for byte, and no error; create accepts it too."""
    import _depth

    for shape in ("h1", "q1_pi3", "q5_pi1", "h1_b1100", "h1_256"):
        c = _depth.SHAPES[shape]
        plain, forced = _plan_text(c, precision), _plan_text(c, precision, stage_path=1)
        assert plain[0] == 0 and forced == plain, (shape, forced)
        rc, msg = _create(_cfg_of(c, precision), stage_path=1)
        assert rc == SAC_E_HIP and "internal" not in msg, (shape, rc, msg)


def _create(cfg, **overrides):
    """(rc, message) of sac_engine_create on fake buffers: the planner runs
    whole before the first HIP call, where a machine without a GPU stops."""
    for k, v in overrides.items():
        setattr(cfg, k, v)
    lib = E.load_library()
    ws = lib.sac_engine_workspace_bytes(ctypes.byref(cfg))
    bufs = E.EngineBuffers(*([0x1000] * 15), 0x100000, max(ws, 1))
    out = ctypes.c_void_p()
    rc = lib.sac_engine_create(ctypes.byref(cfg), ctypes.byref(bufs), None, ctypes.byref(out))
    if rc == 0:
        lib.sac_engine_destroy(out)
        pytest.skip("GPU present: the planner ran for real")
    return rc, lib.sac_last_error().decode()


@pytest.mark.parametrize("net", ["q", "pi"])
def test_six_hidden_layers_are_refused(net):
    """The library takes 2..6 Linear layers per network (SAC_DEV_LAYERS): a
    sixth hidden layer of either net fails validation in the workspace query
    and in create, before any HIP call."""
    c = dict(obs=5, act=3, batch=40, q_hidden=[72, 40], pi_hidden=[40, 72])
    c[f"{net}_hidden"] = [32] * 6
    cfg = _cfg_of(c, "fp32")
    assert max(cfg.q_layers, cfg.pi_layers) == 7
    lib = E.load_library()
    assert lib.sac_engine_workspace_bytes(ctypes.byref(cfg)) == 0
    assert "1..5 hidden layers" in lib.sac_last_error().decode()
    rc, msg = _create(cfg)
    assert rc == SAC_E_INVALID and "1..5 hidden layers" in msg, (rc, msg)
    rc, msg = _plan(c, "fp32")
    assert rc == SAC_E_INVALID and "1..5 hidden layers" in msg, (rc, msg)
    c[f"{net}_hidden"] = [32] * 5  # the limit itself is planned
    assert _plan(c, "fp32")[0] == 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("c", [dict(obs=24, act=4, hidden=[512] * 5, batch=64),
                               dict(obs=17, act=6, hidden=[400, 300, 400, 300, 400], batch=1100)],
                         ids=["512x5", "400_300x5_b1100"])
def test_five_wide_hidden_layers_take_the_stage_path(c, precision):
    """Five hidden layers past the phase kernels' LDS layout: the stage path's
    job list grows with the depth (WIDE_MAX_JOBS) and the update tiles' tables
    with it; the planner's own consistency check ("internal: ...") stays
    quiet, in the host-only export and in create."""
    assert _plan(c, precision) == (0, "wide")
    rc, msg = _create(_cfg_of(c, precision))
    assert "internal" not in msg, msg
    assert rc == SAC_E_HIP, (rc, msg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_refused_roles_override_names_the_cause_that_applies(precision):
    """layout = roles at [256] * 5, B = 40: three row tiles are 18 co-resident
    workgroups, well inside 256; what refuses the role kernels is their R-row
    LDS layout, and the message says so.  C3's 256 row tiles keep the
    workgroup count as their cause."""
    import _depth

    rc, msg = _plan(dict(_depth.SHAPES["h5_256"], batch=40), precision, layout=1)
    assert rc == SAC_E_INVALID and "cannot be honoured: roles (the R-row LDS layout does not fit" in msg, (rc, msg)
    rc, msg = _plan(bench.CONFIGS["c3"], precision, layout=1)
    assert rc == SAC_E_INVALID and "roles (needs 6 * row tiles <= 256 co-resident workgroups)" in msg, (rc, msg)


def test_engine_library_reads_no_environment():
    """the product library takes every layout choice from
    sac_engine_config; no getenv / secure_getenv import in its dynamic symbols
    (the SAC_STAMPS diagnostic build may read one)."""
    import subprocess

    syms = subprocess.run(["nm", "-D", "--undefined-only", E.library_path()], capture_output=True, text=True,
                          check=True).stdout
    assert "getenv" not in syms, [ln for ln in syms.splitlines() if "getenv" in ln]
