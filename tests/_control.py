"""What the GPU tests of the control tasks (tests/test_gpu_pendulum.py, test_gpu_reacher.py,
test_gpu_cartpole.py) share: the agent configuration, bit views, the one-ulp comparison, and agents and
twin environments on a task's host class.  Each file binds `cfg` and `make_agent` to its task with
functools.partial; its equality rules stay its own."""
import numpy as np
import torch

DEV = "cuda"


def cfg(env_name, hidden=(40, 72), precision="fp32", capacity=1000, batch=32, warming=64, seed=3, log_episodes=False,
        log_q=False, alpha=0.2, alpha_lr=3e-4, action_scale=1.0):
    hidden = list(hidden)
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": alpha, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": alpha_lr},
        "q_net": {"hidden_sizes": hidden, "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": hidden, "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": action_scale},
        "buffer": {"capacity": capacity},
        "train": {"gradient_steps_per_update": 1, "update_frequency": 1, "seed": seed, "batch_size": batch,
                  "warming_steps": warming, "device": "cuda", "precision": precision, "graph_chunk": 4},
        "logger": {"enabled": False, "env_name": env_name, "agent_name": "SAC", "log_episode_stats": log_episodes,
                   "log_q_values": log_q, "save_model": {"enabled": False, "path": None}},
    }


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw(t):
    return t.detach().contiguous().view(torch.uint8).cpu()


def within_one_ulp(dev, host, what):
    """dev fp32 within one fp32 ulp of host fp32, elementwise; returns the number of non-identical elements."""
    dev, host = np.asarray(dev, np.float32), np.asarray(host, np.float32)
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    ok = err <= np.spacing(np.abs(host)).astype(np.float64)
    n_diff = int(np.sum(bits(dev) != bits(host)))
    print(f"{what}: {n_diff} of {dev.size} not identical, max |err| {err.max():.3e}, beyond 1 ulp {int(np.sum(~ok))}")
    assert np.all(ok), f"{what}: {int(np.sum(~ok))} of {dev.size} beyond 1 ulp (max |err| {err.max():.3e})"
    return n_diff


def make_agent(task_cfg, task_cls, N, max_steps=5, precision="fp32", layout="records", host_cls=None, ring_steps=None,
               **cfg_kw):
    """(agent, its DeviceVectorEnv of N copies of the task): task_cfg is the task's `cfg`, task_cls the name of
    its class in sac.control_envs; host_cls, a class, takes its place."""
    from sac import control_envs
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv
    from sac.replay_buffer import ReplayBuffer

    c = task_cfg(precision=precision, **cfg_kw)
    host = (host_cls or getattr(control_envs, task_cls))(max_steps=max_steps)
    dv = DeviceVectorEnv.from_env(host, N, device=DEV, ring_steps=ring_steps)
    agent = SAC(dv, c)  # _set_seed resets the envs with train.seed
    if layout != "records":
        agent.replay_buffer = ReplayBuffer(c["buffer"]["capacity"], device=agent.device, layout=layout)
    return agent, dv


def twin_of(dv):
    """Another DeviceVectorEnv in dv's state: stepping it with the stored actions is the step kernel's answer."""
    from sac.device_envs import KINDS, DeviceVectorEnv

    tw = DeviceVectorEnv.from_env(KINDS[dv.kind][1](max_steps=dv.max_steps), dv.num_envs, device=DEV)
    tw.seed, tw.t, tw._reset_done = dv.seed, dv.t, True
    for name in ("obs", "counters", "dstate", "ring"):
        getattr(tw, name).copy_(getattr(dv, name))
    return tw
