"""The critic-evaluation entry points without a GPU: both symbols are exported,
their ctypes signatures are the header's, and every argument check of
sac_q_values / sac_q_values_replay returns SAC_E_INVALID with its message before
any HIP call.  The checks that compare against the engine's dims run on a
host-only engine (include/sac_engine_testing.h sac_debug_engine_host: the
validated config, no device state).  sac_policy_act and sac_rollout_step, the
other two forward-only entry points, refuse that engine the same way."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

INCLUDE = os.path.join(ROOT, "include")
INVALID = -1
PTR = 0x1000  # never dereferenced: every call below is rejected before a launch


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_engine_host.restype = ctypes.c_int
    lb.sac_debug_engine_host.argtypes = [ctypes.POINTER(E.EngineConfig), ctypes.POINTER(ctypes.c_void_p)]
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


def _config(E, obs=5, act=3, hidden=(72, 40)):
    c = E.EngineConfig()
    c.obs_dim, c.act_dim, c.batch = obs, act, 16
    qd, pd = [obs + act, *hidden, 1], [obs, *hidden, 2 * act]
    c.q_layers, c.pi_layers = len(qd) - 1, len(pd) - 1
    for i, d in enumerate(qd):
        c.q_dims[i] = d
    for i, d in enumerate(pd):
        c.pi_dims[i] = d
    c.q_hidden_act = c.pi_hidden_act = 1
    c.gamma, c.tau, c.log_std_min, c.log_std_max, c.action_scale = 0.99, 0.005, -20.0, 2.0, 1.0
    c.actor_lr = c.critic_lr = c.alpha_lr = 3e-4
    c.beta1, c.beta2, c.adam_eps = 0.9, 0.999, 1e-8
    c.auto_entropy, c.target_entropy, c.precision = 1, -float(act), 0
    return c


@pytest.fixture()
def host_engine(lib):
    """A host-only engine of obs 5 / act 3."""
    from sac import _engine as E

    h = ctypes.c_void_p()
    cfg = _config(E)
    assert lib.sac_debug_engine_host(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    yield h
    lib.sac_engine_destroy(h)


def _replay(E, cap=12, obs=5, act=3, stride=16, null=()):
    d = E.ReplayDesc(PTR, PTR, PTR, PTR, PTR, cap, obs, act, PTR, stride)
    for field in null:
        setattr(d, field, None)
    return d


# ---------------------------------------------------------------- ABI
def test_symbols_exported(lib):
    for name in ("sac_q_values", "sac_q_values_replay", "sac_debug_engine_host"):
        assert hasattr(lib, name), name


C_TYPES = {"sac_engine *": ctypes.c_void_p, "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p,
           "void *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


def test_ctypes_signatures_match_header():
    """Every parameter of the two declarations, in order, against sac._engine.SIGNATURES."""
    from sac import _engine as E

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "sac_engine.h")).read(), flags=re.S)
    for name in ("sac_q_values", "sac_q_values_replay"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        want = []
        for p in m.group(1).split(","):
            ctype = re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", p.strip())).strip()  # drop the parameter name
            want.append(ctypes.POINTER(E.ReplayDesc) if ctype == "const sac_replay *" else C_TYPES[ctype])
        res, args = E.SIGNATURES[name]
        assert res is ctypes.c_int and args == want, (name, args, want)
    assert len(E.SIGNATURES["sac_q_values"][1]) == 9 and len(E.SIGNATURES["sac_q_values_replay"][1]) == 8


def test_host_engine_rejects_bad_config(lib):
    from sac import _engine as E

    h = ctypes.c_void_p()
    bad = _config(E)
    bad.q_dims[0] = 9
    assert lib.sac_debug_engine_host(ctypes.byref(bad), ctypes.byref(h)) == INVALID and not h.value
    assert lib.sac_debug_engine_host(None, ctypes.byref(h)) == INVALID
    assert lib.sac_debug_engine_host(ctypes.byref(_config(E)), None) == INVALID


# ---------------------------------------------------------------- sac_q_values
def test_q_values_rejects_nulls_and_empty(lib, host_engine):
    q = lambda e, obs, act, n, out: lib.sac_q_values(e, obs, 5, act, 3, n, 0, out, None)  # noqa: E731
    assert q(host_engine, None, PTR, 4, PTR) == INVALID and "null input" in _err(lib)
    assert q(host_engine, PTR, None, 4, PTR) == INVALID and "null input" in _err(lib)
    assert q(host_engine, PTR, PTR, 4, None) == INVALID and "null output" in _err(lib)
    assert q(host_engine, PTR, PTR, 0, PTR) == INVALID and "n >= 1" in _err(lib)
    assert q(host_engine, PTR, PTR, -3, PTR) == INVALID and "n >= 1" in _err(lib)
    assert q(None, PTR, PTR, 4, PTR) == INVALID and "null engine" in _err(lib)


@pytest.mark.parametrize("so,sa", [(4, 3), (5, 2), (0, 3), (5, -1)])
def test_q_values_rejects_narrow_strides(lib, host_engine, so, sa):
    assert lib.sac_q_values(host_engine, PTR, so, PTR, sa, 4, 0, PTR, None) == INVALID
    assert "stride below the field width" in _err(lib)


@pytest.mark.parametrize("so,sa,target", [(5, 3, 0), (16, 16, 1), (64, 7, 0)])
def test_q_values_valid_arguments_reach_the_launch(lib, host_engine, so, sa, target):
    """Valid arguments pass every check: the host-only engine is refused only where the launch would be."""
    assert lib.sac_q_values(host_engine, PTR, so, PTR, sa, 33, target, PTR, None) == INVALID
    assert "no device state" in _err(lib)


# ---------------------------------------------------------------- sac_q_values_replay
def test_q_values_replay_rejects_nulls_and_empty(lib, host_engine):
    from sac import _engine as E

    call = lambda e, rb, first=10, n=5, out=PTR: lib.sac_q_values_replay(e, rb, first, n, 1, 0, out, None)  # noqa: E731
    assert call(host_engine, None) == INVALID and "null replay" in _err(lib)
    for field in ("obs", "act", "next_obs"):
        assert call(host_engine, ctypes.byref(_replay(E, null=(field,)))) == INVALID and "null replay" in _err(lib)
    assert call(host_engine, ctypes.byref(_replay(E)), out=None) == INVALID and "null output" in _err(lib)
    assert call(host_engine, ctypes.byref(_replay(E)), n=0) == INVALID and "n >= 1" in _err(lib)
    assert call(None, ctypes.byref(_replay(E))) == INVALID and "null engine" in _err(lib)


@pytest.mark.parametrize("first", [-1, 12, 13, 2**40])
def test_q_values_replay_rejects_first_slot_outside_the_ring(lib, host_engine, first):
    from sac import _engine as E

    assert lib.sac_q_values_replay(host_engine, ctypes.byref(_replay(E)), first, 5, 1, 0, PTR, None) == INVALID
    assert "first_slot" in _err(lib) and "outside [0, capacity 12)" in _err(lib)


def test_q_values_replay_rejects_more_rows_than_slots(lib, host_engine):
    from sac import _engine as E

    assert lib.sac_q_values_replay(host_engine, ctypes.byref(_replay(E)), 0, 13, 1, 0, PTR, None) == INVALID
    assert "exceeds the replay capacity" in _err(lib)
    assert lib.sac_q_values_replay(host_engine, ctypes.byref(_replay(E, cap=0)), 0, 1, 1, 0, PTR, None) == INVALID


@pytest.mark.parametrize("kw", [dict(obs=4), dict(act=2), dict(obs=3, act=5)])
def test_q_values_replay_rejects_other_dims(lib, host_engine, kw):
    from sac import _engine as E

    assert lib.sac_q_values_replay(host_engine, ctypes.byref(_replay(E, **kw)), 10, 5, 1, 0, PTR, None) == INVALID
    assert "replay dims do not match the engine" in _err(lib)


def test_q_values_replay_rejects_narrow_records(lib, host_engine):
    from sac import _engine as E

    assert lib.sac_q_values_replay(host_engine, ctypes.byref(_replay(E, stride=4)), 10, 5, 1, 0, PTR, None) == INVALID
    assert "stride below the field width" in _err(lib)


@pytest.mark.parametrize("stride,first,n,use_next,target", [(16, 10, 5, 1, 0), (0, 0, 12, 0, 1), (16, 11, 12, 1, 1)])
def test_q_values_replay_valid_arguments_reach_the_launch(lib, host_engine, stride, first, n, use_next, target):
    from sac import _engine as E

    rb = _replay(E, stride=stride)
    assert lib.sac_q_values_replay(host_engine, ctypes.byref(rb), first, n, use_next, target, PTR, None) == INVALID
    assert "no device state" in _err(lib)


# ---------------------------------------------------------------- sac_policy_act / sac_rollout_step
@pytest.mark.parametrize("n,eps,log_pi", [(1, None, None), (33, PTR, None), (16, PTR, PTR)])
def test_policy_act_valid_arguments_reach_the_launch(lib, host_engine, n, eps, log_pi):
    """The policy kernel is guarded like the critic kernel: a host-only engine is refused before the launch."""
    assert lib.sac_policy_act(host_engine, PTR, n, eps, PTR, log_pi, None) == INVALID
    assert "policy_act" in _err(lib) and "no device state" in _err(lib)


def test_policy_act_still_rejects_bad_arguments_first(lib, host_engine):
    for args in ((None, PTR, 4, None, PTR), (host_engine, None, 4, None, PTR), (host_engine, PTR, 4, None, None),
                 (host_engine, PTR, 0, None, PTR)):
        assert lib.sac_policy_act(*args, None, None) == INVALID and "bad policy_act arguments" in _err(lib)


def _envs(E, kind=2, n=17, obs=5, null=()):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, 4
    for field in ("obs", "step", "ep_length", "pos", "ep_return", "episodes"):
        setattr(d, field, None if field in null else PTR)
    d.ring_steps = 8
    return d


@pytest.fixture()
def host_engine_act1(lib):
    """A host-only engine of obs 5 / act 1, the fused rollout step's action width."""
    from sac import _engine as E

    h = ctypes.c_void_p()
    cfg = _config(E, obs=5, act=1, hidden=(64, 64))
    assert lib.sac_debug_engine_host(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    yield h
    lib.sac_engine_destroy(h)


@pytest.mark.parametrize("size,pos,deterministic,store", [(0, 0, 0, 1), (64, 47, 1, 1), (17, 17, 0, 0)])
def test_rollout_step_valid_arguments_reach_the_launch(lib, host_engine_act1, size, pos, deterministic, store):
    from sac import _engine as E

    ev, rb = _envs(E), _replay(E, cap=64, obs=5, act=1, stride=8)
    rc = lib.sac_rollout_step(host_engine_act1, ctypes.byref(ev), ctypes.byref(rb), size, pos, 1, deterministic, store,
                              None)
    assert rc == INVALID and "rollout_step" in _err(lib) and "no device state" in _err(lib)


def test_rollout_step_still_rejects_bad_arguments_first(lib, host_engine, host_engine_act1):
    from sac import _engine as E

    ev, rb = _envs(E), _replay(E, cap=64, obs=5, act=1, stride=8)
    call = lambda e, ev, rb, size=0, pos=0: lib.sac_rollout_step(  # noqa: E731
        e, ctypes.byref(ev), ctypes.byref(rb), size, pos, 1, 0, 1, None)
    assert call(host_engine_act1, _envs(E, null=("episodes",)), rb) == INVALID and "episode ring" in _err(lib)
    assert call(host_engine_act1, ev, _replay(E, cap=16, obs=5, act=1)) == INVALID and "exceeds the replay" in _err(lib)
    assert call(host_engine_act1, ev, rb, pos=64) == INVALID and "out of range" in _err(lib)
    assert call(None, ev, rb) == INVALID and "null engine" in _err(lib)
    assert call(host_engine, ev, rb) == INVALID and "engine dims do not match" in _err(lib)  # act 3


# ---------------------------------------------------------------- torch ops
def test_ops_registered_read_only_with_meta_shapes(lib):
    import torch

    from sac import _engine as E

    ops = E.ops()
    for name in ("q_values", "q_values_replay"):
        schema = str(getattr(ops, name).default._schema)
        assert "!" not in schema and schema.endswith("-> Tensor"), schema  # no mutated argument, a fresh output
    obs, act = torch.empty(37, 5, device="meta"), torch.empty(37, 3, device="meta")
    assert tuple(ops.q_values(1, obs, act, True).shape) == (37, 2)
    storage, state = torch.empty(12 * 16, device="meta"), torch.empty(3, dtype=torch.int64, device="meta")
    q = ops.q_values_replay(1, storage, state, [12, 5, 3, 16, 0, 10, 13, 5, 14], 10, 5, True, False)
    assert tuple(q.shape) == (5, 2) and q.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="CPU"):  # CUDA and Meta kernels only: no CPU fallback
        ops.q_values(1, torch.zeros(4, 5), torch.zeros(4, 3), False)


# ---------------------------------------------------------------- no GPU
def test_python_entry_points_exist():
    import inspect

    from sac.agent import SAC
    from sac.device_envs import DeviceQValueLog
    from sac.engine import SacEngine

    assert list(inspect.signature(SacEngine.q_values).parameters) == ["self", "obs", "act", "target", "out"]
    assert list(inspect.signature(SacEngine.q_values_replay).parameters) == [
        "self", "replay", "first_slot", "n", "next_obs", "target", "out"]
    assert list(inspect.signature(SAC.q_values).parameters) == ["self", "states", "actions", "target"]
    p = inspect.signature(SAC.run_device_training_loop).parameters
    assert p["device_q_values"].default is False
    assert all(hasattr(DeviceQValueLog, m) for m in ("after_step", "finish"))
