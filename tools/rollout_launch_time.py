"""Device time of one fused rollout launch (act -> step -> store) per environment
kind, on one MI355X: `--launches` back-to-back SacEngine.rollout_step calls
between two events, queued behind large device copies so that the host is ahead
of the device and the interval is device time; median of `--repeats`, min .. max.
Nets 2x[256,256] fp32, B = 256, buffer 1e6 rows.

    python tools/rollout_launch_time.py [--envs point_mass,pendulum,reacher,cartpole] [--num-envs 4096]
                                        [--package DIR] [--label this] [--uniform] [--out FILE]
--package DIR imports the `sac` package (and the libraries beside it) from DIR
instead of this tree's soft-actor-critic_amd: another build of the project, for
an A/B in one session.  --uniform adds, after each fused measurement, the same
measurement with the engine's action source set to uniform (train.random_steps:
one thread per environment row, no policy forward), labelled `<label>-u`.
Prints one line per (env, N) and appends them to --out.
"""
import argparse
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# --env name -> (module of the sac package, host class, policy_net.action_scale)
ENVS = {"point_mass": ("envs", "OneDPointMassReachEnv", 1.0), "pendulum": ("control_envs", "PendulumEnv", 2.0),
        "reacher": ("control_envs", "ReacherEnv", 1.0), "cartpole": ("control_envs", "CartPoleEnv", 1.0)}


def cfg(env):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.1, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": ENVS[env][2]},
        "buffer": {"capacity": 1_000_000},
        "train": {"gradient_steps_per_update": 1, "update_frequency": 1, "seed": 0, "batch_size": 256,
                  "warming_steps": 256, "device": "cuda", "precision": "fp32", "graph_chunk": 32},
        "logger": {"enabled": False, "env_name": env, "agent_name": "SAC", "log_episode_stats": False,
                   "log_q_values": False, "save_model": {"enabled": False, "path": None}},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="point_mass,pendulum,reacher,cartpole")
    ap.add_argument("--num-envs", default="4096")
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--package", default=os.path.join(R, "soft-actor-critic_amd"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--uniform", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path[:0] = [R, os.path.abspath(args.package)]
    import importlib

    import torch

    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    if not torch.cuda.is_available():
        raise SystemExit("rollout_launch_time: no HIP device visible")
    big = torch.empty(2, 128 * 1024 * 1024, dtype=torch.float32, device="cuda")  # two 512 MiB halves
    lines = []
    for env in args.envs.split(","):
        host_cls = getattr(importlib.import_module("sac." + ENVS[env][0]), ENVS[env][1])
        for N in (int(x) for x in args.num_envs.split(",")):
            dv = DeviceVectorEnv.from_env(host_cls(), N, device="cuda")
            agent = SAC(dv, cfg(env))
            eng, rb = agent.engine, agent.replay_buffer
            for source, label in ((0, args.label), (1, args.label + "-u"))[:2 if args.uniform else 1]:
                if source:
                    eng.set_action_source(source)
                for _ in range(50):
                    eng.rollout_step(dv, rb)
                torch.cuda.synchronize()
                us = []
                for _ in range(args.repeats):
                    for _ in range(8):
                        big[1].copy_(big[0])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.launches):
                        eng.rollout_step(dv, rb)
                    b.record()
                    torch.cuda.synchronize()
                    us.append(a.elapsed_time(b) * 1000.0 / args.launches)
                eng.check()
                lines.append(f"{label:<7} {env:<11} N={N:>5}  {statistics.median(us):>8.3f}   "
                             f"{min(us):.3f} .. {max(us):.3f}")
                print(lines[-1], flush=True)
            eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
