"""Generate tests/golden/plan_digests.json: the engine's launch plan for a matrix
of configs, as the host-only export sac_debug_plan_host reports it.

    python tests/golden/make_plan_digests.py

Needs the built library and no GPU (the export makes no HIP call).  Each case
is one line of the file, sorted by id: the export's JSON object (the kernel
path, the workspace / LDS sizes, the launch geometry of every phase and
FNV-1a hashes of the device descriptors, update tiles and stage-path jobs the
planner builds over fixed fake addresses), or {"rc", "message"} where the
planner refuses the config.  tests/test_plan_digests_cpu.py regenerates every
case and compares it with the file, so an edit of the planner that changes
any grid, LDS size, tile or descriptor byte fails there; regenerate the file
only with a change that means to alter the plan.

The matrix (cases()):
  * every bench.CONFIGS entry x {fp32, bf16} x the ten overrides of
    tests/test_plan_cpu.py::test_plan_is_consistent;
  * the shapes and layout overrides of the GPU activation matrix
    (test_plan_cpu._activation_cases) with ReLU and with ELU hidden layers;
  * the five shapes of test_shapes_past_the_lds_layout_take_the_stage_path;
  * edge shapes of the planner's own thresholds (EDGES below), the network
    depths 1..5 and unequal depths of tests/_depth.py and the odd layer widths
    of tests/_widths.py among them.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "soft-actor-critic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "plan_digests.json")
NCU = 256  # compute units of the MI355X
PRECISIONS = ("fp32", "bf16")
OVERRIDES = ["", "stage_batch=-1", "layout=1", "layout=2", "layout=3", "layout=3,upd_threads=512", "upd_parts=4",
             "upd_threads=1024", "stage_path=1", "stage_path=-1"]
PAST_LDS = [(300, 6, [256, 256]), (24, 4, [512, 512]), (24, 4, [384, 384]), (17, 6, [400, 300]),
            (24, 4, [1024, 1024, 512])]


def _edge(batch=256, obs=24, act=4, hidden=(256, 256), **kw):
    return dict(obs=obs, act=act, batch=batch, hidden=list(hidden), **kw)


# name -> (config dict, overrides, ncu): [256, 256] nets at obs 24, act 4, B = 256 unless stated
EDGES = {
    "b1": (_edge(batch=1), {}, NCU),
    "b17": (_edge(batch=17), {}, NCU),
    "b48_pairs": (_edge(batch=48), {"layout": 3}, NCU),  # an odd number of row tiles
    "b1025_parts0": (_edge(batch=1025), {"upd_parts": 0}, NCU),  # batch parts of the update tiles
    "b1025_parts3": (_edge(batch=1025), {"upd_parts": 3}, NCU),
    "b4096_parts0": (_edge(batch=4096), {"upd_parts": 0}, NCU),
    "b4096_parts3": (_edge(batch=4096), {"upd_parts": 3}, NCU),
    "act16": (_edge(act=16), {}, NCU),  # the hidden split's 2 * act <= 32
    "act17": (_edge(act=17), {}, NCU),
    # the API's widest action on each forced layout, and the stage path's 2 * act <= 16 (padded small nets, B = 40)
    "act32_roles": (_edge(batch=40, obs=5, act=32, q_hidden=[72, 40], pi_hidden=[40, 72]), {"layout": 1}, NCU),
    "act32_rows": (_edge(batch=40, obs=5, act=32, q_hidden=[72, 40], pi_hidden=[40, 72]), {"layout": 2}, NCU),
    "act32_pairs": (_edge(batch=40, obs=5, act=32, q_hidden=[72, 40], pi_hidden=[40, 72]), {"layout": 3}, NCU),
    "act8_stage": (_edge(batch=40, obs=5, act=8, q_hidden=[72, 40], pi_hidden=[40, 72]), {"stage_path": 1}, NCU),
    "obs216": (_edge(obs=216), {}, NCU),
    "pi_256_128": (_edge(pi_hidden=[256, 128]), {}, NCU),  # pi's own widths: the split refused by width
    "deep_64": (_edge(hidden=(64, 64, 64)), {}, NCU),  # 4-layer nets
    "ut512_b4096": (_edge(batch=4096), {"upd_threads": 512}, NCU),  # 256 < nB <= 512 (480, 336)
    "ut512_w384": (_edge(hidden=(384, 384)), {"upd_threads": 512}, NCU),
    "stage_b4096_ncu256": (_edge(batch=4096, hidden=(512, 512)), {}, 256),  # the stages' K buffers depend on ncu
    "stage_b4096_ncu128": (_edge(batch=4096, hidden=(512, 512)), {}, 128),
}


def _depth_edges():
    """Network depths 1..5 and unequal depths (tests/_depth.py): every case of
    the GPU depth matrix on its layout, each shape as the engine plans it by
    default, stage_path = 1 where a one-hidden-layer net makes it a no-op,
    layout = roles refused by the LDS layout, and five wide hidden layers."""
    import _depth

    lay = {"layout": {"roles": 1, "rows": 2, "pairs": 3}}
    out = {}
    for case, (shape, over, _) in _depth.CASES.items():
        out[f"depth_{case}"] = (shape, {k: lay.get(k, {}).get(v, v) for k, v in (over or {}).items()}, NCU)
    for name, shape in _depth.SHAPES.items():
        out[f"depth_{name}_default"] = (shape, {}, NCU)
    for name in ("h1", "q1_pi3", "q5_pi1"):
        out[f"depth_{name}_stage_ignored"] = (_depth.SHAPES[name], {"stage_path": 1}, NCU)
    out["depth_h5_256_b40_roles_refused"] = (dict(_depth.SHAPES["h5_256"], batch=40), {"layout": 1}, NCU)
    out["depth_512x5"] = (_edge(batch=64, hidden=(512,) * 5), {}, NCU)
    out["depth_400_300x5_b1100"] = (_edge(batch=1100, obs=17, act=6, hidden=(400, 300, 400, 300, 400)), {}, NCU)
    return out


EDGES.update(_depth_edges())


def _width_edges():
    """Layer widths off the 8-column grid (tests/_widths.py): every case of the
    GPU width matrix on its layout, each shape as the engine plans it by
    default, and layout = pairs refused one past 256."""
    import _widths

    lay = {"layout": {"roles": 1, "rows": 2, "pairs": 3}}
    out = {}
    for case, (shape, over, _) in _widths.CASES.items():
        out[f"width_{case}"] = (shape, {k: lay.get(k, {}).get(v, v) for k, v in (over or {}).items()}, NCU)
    for name, shape in _widths.SHAPES.items():
        out[f"width_{name}_default"] = (shape, {}, NCU)
    out["width_w257_pairs_refused"] = (_widths.SHAPES["w257"], {"layout": 3}, NCU)
    return out


EDGES.update(_width_edges())


def cases():
    """{id: (config dict, precision, {override field: int}, ncu)}"""
    import bench
    from sac import _engine as E
    from test_plan_cpu import _activation_cases

    out = {}
    for prec in PRECISIONS:
        for name in sorted(bench.CONFIGS):
            for ov in OVERRIDES:
                kv = {k: int(v) for k, v in (s.split("=") for s in filter(None, ov.split(",")))}
                out[f"bench/{name}/{prec}/{ov or 'default'}"] = (bench.CONFIGS[name], prec, kv, NCU)
        for shape, acts, c, lay in _activation_cases():
            if acts != "elu_elu":
                continue
            kv = {k: E.LAYOUTS[v] if k == "layout" else int(v) for k, v in (lay or {}).items()}
            out[f"act/{shape}/elu_elu/{prec}"] = (c, prec, kv, NCU)
            out[f"act/{shape}/relu_relu/{prec}"] = (dict(c, q_act="relu", pi_act="relu"), prec, kv, NCU)
        for obs, act, hidden in PAST_LDS:
            c = dict(obs=obs, act=act, hidden=hidden, batch=64)
            out[f"past_lds/obs{obs}_act{act}_{'x'.join(map(str, hidden))}/{prec}"] = (c, prec, {}, NCU)
        for name, (c, kv, ncu) in EDGES.items():
            out[f"edge/{name}/{prec}"] = (c, prec, kv, ncu)
    return out


def bind(lib):
    from sac import _engine as E

    lib.sac_debug_plan_host.restype = ctypes.c_int
    lib.sac_debug_plan_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.c_int32, ctypes.c_char_p,
                                        ctypes.c_size_t]
    return lib


def plan_text(lib, case, cap=1 << 16):
    """(rc, the export's text) of one case: its JSON, or sac_last_error()."""
    from test_plan_cpu import _cfg_of

    c, prec, kv, ncu = case
    cfg = _cfg_of(c, prec)
    for k, v in kv.items():
        setattr(cfg, k, v)
    buf = ctypes.create_string_buffer(cap)
    rc = lib.sac_debug_plan_host(ctypes.byref(cfg), ncu, buf, cap)
    return rc, (buf.value if rc == 0 else lib.sac_last_error()).decode()


def digest(lib, case):
    rc, text = plan_text(lib, case)
    return json.loads(text) if rc == 0 else {"rc": rc, "message": text}


def render(digests):
    lines = [f"{json.dumps(k)}: {json.dumps(digests[k], sort_keys=True)}" for k in sorted(digests)]
    return "{\n" + ",\n".join(lines) + "\n}\n"


def main():
    from sac import _engine as E

    lib = bind(E.load_library())
    digests = {k: digest(lib, c) for k, c in cases().items()}
    with open(OUT, "w") as f:
        f.write(render(digests))
    paths = {}
    for d in digests.values():
        paths[d.get("path", "refused")] = paths.get(d.get("path", "refused"), 0) + 1
    print(f"wrote {OUT}: {len(digests)} cases, {paths}")


if __name__ == "__main__":
    main()
