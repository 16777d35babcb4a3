"""Device-resident probe environments without a GPU: the C-ABI additions
(symbols, struct layouts, host-side validation), the host exports of the new
Philox draws against restatements written here on oracle/sampler_oracle.py's
Philox, and the no-GPU behaviour of sac.device_envs."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

from oracle import sampler_oracle as S

INCLUDE = os.path.join(ROOT, "include")
INVALID = -1
u64, i32, i64, vp = ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from sac import _engine as E

    if not os.path.exists(E.library_path()):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    lb = E.load_library()
    lb.sac_debug_rollout_eps_host.argtypes = [u64, u64, i32, i32, vp]
    lb.sac_debug_env_obs_host.argtypes = [u64, u64, i32, i32, i32, vp]
    return lb


def _err(lib):
    return lib.sac_last_error().decode()


# ---------------------------------------------------------------- ABI
def test_new_symbols_exported(lib):
    for name in ("sac_envs_reset", "sac_envs_step", "sac_rollout_step", "sac_debug_rollout_eps_host",
                 "sac_debug_env_obs_host"):
        assert hasattr(lib, name), name


def test_env_struct_layouts_match_c(tmp_path):
    from sac import _engine as E

    structs = {"sac_env_config": E.EnvConfig, "sac_env_episode": E.EnvEpisode, "sac_envs": E.EnvsDesc}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "sac_engine.h"', "int main(void) {"]
    for st, cls in structs.items():
        src.append(f'printf("{st} size %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            src.append(f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    lay = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, v = line.split()
        lay[(st, f)] = int(v)
    for st, cls in structs.items():
        assert ctypes.sizeof(cls) == lay[(st, "size")], st
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == lay[(st, name)], (st, name)
    # the episode ring is exposed to PyTorch as float64 [S][N][2]: a cell is two doubles wide
    assert ctypes.sizeof(E.EnvEpisode) == 16 and E.EnvEpisode.length.offset == 8 and E.EnvEpisode.ended.offset == 12
    # the parameter order the torch ops take is the struct's
    assert [n for n, t in E.EnvConfig._fields_ if t is ctypes.c_double] == list(E.ENV_PARAMS)


def test_env_kind_codes_match_header():
    from sac import _engine as E
    from sac.device_envs import KINDS

    text = open(os.path.join(INCLUDE, "sac_engine.h")).read()
    for macro, name in (("SAC_ENV_CONSTANT_REWARD", "constant_reward"), ("SAC_ENV_QUADRATIC_ACTION", "quadratic_action"),
                        ("SAC_ENV_RANDOM_OBS", "random_obs_binary"), ("SAC_ENV_POINT_MASS", "point_mass")):
        import re

        code = int(re.search(macro + r"\s*=\s*(\d+)", text).group(1))
        assert E.ENV_KINDS[name] == code == KINDS[name][0]


# ---------------------------------------------------------------- validation (no device needed)
def _envs(E, kind=3, n=4, obs=1, max_steps=5, fake_ptrs=True, ring=True):
    d = E.EnvsDesc()
    d.cfg.kind, d.cfg.num_envs, d.cfg.obs_dim, d.cfg.max_steps = kind, n, obs, max_steps
    if fake_ptrs:  # never dereferenced: every case below is rejected before a launch
        d.obs = d.step = d.ep_length = d.pos = d.ep_return = 0x1000
        if ring:
            d.episodes, d.ring_steps = 0x1000, 8
    return d


def _replay(E, cap=64, obs=1, act=1):
    return E.ReplayDesc(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, cap, obs, act, 0x1000, 0)


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=4), "unknown environment kind"),
    (dict(kind=-1), "unknown environment kind"),
    (dict(n=0), "num_envs"),
    (dict(max_steps=0), "max_steps"),
    (dict(kind=3, obs=2), "obs_dim"),
    (dict(kind=2, obs=0), "obs_dim"),
    (dict(fake_ptrs=False), "null environment state"),
])
def test_envs_step_and_reset_reject_bad_envs(lib, kw, msg):
    from sac import _engine as E

    d = _envs(E, **kw)
    assert lib.sac_envs_step(ctypes.byref(d), 0x1000, 1, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_envs_reset(ctypes.byref(d), 0, None) == INVALID
    assert msg in _err(lib)
    assert lib.sac_rollout_step(None, ctypes.byref(d), ctypes.byref(_replay(E)), 0, 0, 1, 0, 1, None) == INVALID
    assert msg in _err(lib)


def test_envs_step_rejects_null_arguments(lib):
    from sac import _engine as E

    assert lib.sac_envs_step(None, 0x1000, 1, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None) == INVALID
    assert "null environments" in _err(lib)
    d = _envs(E)
    for hole in range(6):  # actions and each of the five outputs
        args = [0x1000] * 6
        args[hole] = None
        assert lib.sac_envs_step(ctypes.byref(d), args[0], 1, *args[1:], None) == INVALID
        assert "null actions or outputs" in _err(lib)


def test_rollout_step_rejects_bad_arguments(lib):
    from sac import _engine as E

    d = _envs(E, n=16)
    call = lambda e, ev, rb, size=0, pos=0: lib.sac_rollout_step(e, ev, rb, size, pos, 1, 0, 1, None)  # noqa: E731
    assert call(None, None, ctypes.byref(_replay(E))) == INVALID and "null environments" in _err(lib)
    assert call(None, ctypes.byref(d), None) == INVALID and "null replay" in _err(lib)
    assert call(None, ctypes.byref(_envs(E, n=16, ring=False)), ctypes.byref(_replay(E))) == INVALID
    assert "episode ring" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E, cap=15))) == INVALID
    assert "exceeds the replay capacity" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E)), size=65) == INVALID and "out of range" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E)), pos=64) == INVALID and "out of range" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E, obs=3))) == INVALID and "replay dims" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E, act=2))) == INVALID and "replay dims" in _err(lib)
    assert call(None, ctypes.byref(d), ctypes.byref(_replay(E))) == INVALID and "null engine" in _err(lib)


# ---------------------------------------------------------------- host RNG exports
def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.logf.restype = ctypes.c_float
    m.logf.argtypes = [ctypes.c_float]
    m.sincosf.restype = None
    m.sincosf.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    return m


def _normal2(libm, seed, t, row, which, pair):
    """sac_device.h philox_normal2 restated: the oracle's Philox words, then the
    fp32 Box-Muller with IEEE fp32 products and the C library's logf / sincosf."""
    f32 = np.float32
    c = S.philox4x32_10([t & S.M32, (t >> 32) & S.M32, row, (which << 16) | pair], seed & S.M32, (seed >> 32) & S.M32)
    u1 = (f32(c[0] >> 8) + f32(1.0)) * f32(5.9604644775390625e-8)
    u2 = f32(c[1] >> 8) * f32(5.9604644775390625e-8)
    r = np.sqrt(f32(-2.0) * f32(libm.logf(float(u1))))
    s, co = ctypes.c_float(), ctypes.c_float()
    libm.sincosf(float(f32(6.283185307179586) * u2), ctypes.byref(s), ctypes.byref(co))
    return r * f32(co.value), r * f32(s.value)


@pytest.mark.parametrize("seed,t,n,A", [(0, 1, 33, 1), (7, 12345, 17, 3), (2**40 + 5, 2**33 + 1, 8, 2)])
def test_rollout_eps_host_is_philox_normal2_which_2(lib, seed, t, n, A):
    out = np.full((n, A), np.nan, np.float32)
    assert lib.sac_debug_rollout_eps_host(seed, t, n, A, out.ctypes.data) == 0
    libm = _libm()
    want = np.zeros((n, A), np.float32)
    for i in range(n):
        for p in range((A + 1) // 2):
            n0, n1 = _normal2(libm, seed, t, i, 2, p)
            want[i, 2 * p] = n0
            if 2 * p + 1 < A:
                want[i, 2 * p + 1] = n1
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), int(np.sum(out != want))
    # another stream than the training draws (which 0 / 1) of the same (seed, step)
    assert not np.array_equal(out, S.eps_draws(seed, t, n, A)[0]) and not np.array_equal(out, S.eps_draws(seed, t, n, A)[1])
    assert lib.sac_debug_rollout_eps_host(seed, t, 0, A, out.ctypes.data) == INVALID
    assert lib.sac_debug_rollout_eps_host(seed, t, n, A, None) == INVALID


def env_obs_numpy(seed, t, which, n, obs_dim):
    """The counter layout of the observation draws, restated: block b of env row
    i at step t is Philox(counter (t lo, t hi, i, which << 16 | b), key seed);
    its word k gives obs[i][4 b + k] = 2 * ((word >> 8) * 2^-24) - 1 in fp32."""
    nb = (obs_dim + 3) // 4
    i, b = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(nb, dtype=np.uint64), indexing="ij")
    c = S._philox_np(np.full(i.shape, t & S.M32, np.uint64), np.full(i.shape, (t >> 32) & S.M32, np.uint64), i,
                     np.uint64(which << 16) | b, seed & S.M32, (seed >> 32) & S.M32)
    u = np.stack([(w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) for w in c], axis=-1)  # [n][nb][4]
    return (np.float32(2.0) * u - np.float32(1.0)).reshape(n, nb * 4)[:, :obs_dim].copy()


def _obs_host(lib, seed, t, which, n, O):
    out = np.full((n, O), np.nan, np.float32)
    assert lib.sac_debug_env_obs_host(seed, t, which, n, O, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("seed,t,n,O", [(0, 0, 33, 5), (3, 1, 17, 4), (2**40 + 5, 2**33 + 1, 9, 1), (11, 61, 5, 13)])
def test_env_obs_host_matches_counter_layout(lib, seed, t, n, O):
    for which in (3, 4):
        out = _obs_host(lib, seed, t, which, n, O)
        want = env_obs_numpy(seed, t, which, n, O)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), which
        assert np.all(out >= -1.0) and np.all(out < 1.0)


def test_env_obs_streams_differ(lib):
    seed, t, n, O = 5, 9, 17, 5
    base = _obs_host(lib, seed, t, 3, n, O)
    assert not np.any(base == _obs_host(lib, seed, t, 4, n, O))          # step vs reset draws
    assert not np.any(base == _obs_host(lib, seed, t + 1, 3, n, O))      # another vector step
    assert not np.any(base == _obs_host(lib, seed + 1, t, 3, n, O))      # another env seed
    assert len(np.unique(base, axis=0)) == n                              # every row its own draws
    assert len(np.unique(base.reshape(-1))) == n * O
    # a range check over many draws: [-1, 1) with the top 24 bits, both halves hit
    big = _obs_host(lib, 1, 2, 3, 4096, 8)
    assert big.min() >= -1.0 and big.max() < 1.0 and abs(float(big.mean())) < 0.02
    assert np.all(((big.astype(np.float64) + 1.0) * 2.0 ** 23) % 1.0 == 0.0)
    assert lib.sac_debug_env_obs_host(1, 2, 3, 0, 8, big.ctypes.data) == INVALID
    assert lib.sac_debug_env_obs_host(1, 2, 3, 8, 0, big.ctypes.data) == INVALID
    assert lib.sac_debug_env_obs_host(1, 2, 3, 8, 8, None) == INVALID


# ---------------------------------------------------------------- no GPU
def test_import_needs_no_gpu_and_construction_raises_without_one():
    from sac import _engine as E
    from sac import device_envs as D

    assert D.kind_name("OneDPointMassReachEnv") == D.kind_name(3) == "point_mass"
    with pytest.raises(ValueError):
        D.kind_name("cartpole")
    from sac.envs import ConstantRewardEnv

    # a host device is refused wherever this runs; with no HIP device visible the default is refused too
    with pytest.raises(E.EngineUnavailable):
        D.DeviceVectorEnv("random_obs_binary", 4, device="cpu", obs_dim=5)
    with pytest.raises(E.EngineUnavailable):
        D.DeviceVectorEnv.from_env(ConstantRewardEnv(reward=0.3, max_steps=3), 2, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(E.EngineUnavailable):
            D.DeviceVectorEnv("point_mass", 4)
        with pytest.raises(E.EngineUnavailable):
            D.DeviceVectorEnv.from_env(ConstantRewardEnv(reward=0.3, max_steps=3), 2)
