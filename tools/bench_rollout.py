"""Environment steps per second of the training loop over the point-mass probe
env (or, with --env pendulum, the pendulum swing-up), host-stepped against
device-resident, on one MI355X.

  host    SAC.run_vectorized_training_loop over sac.vector_env.SyncVectorEnv:
          per vector step an H2D copy, one policy kernel, a blocking D2H copy,
          N Python env.step calls, a pinned H2D copy and one push kernel
  device  SAC.run_device_training_loop over sac.device_envs.DeviceVectorEnv:
          act -> step -> store in one launch, no per-step host<->device traffic

Networks 2x[256,256], batch 256, a 1e6-row buffer, fp32.  N in {64, 1024, 4096}
with one gradient step per vector step (update_frequency = N), N = 64 with one
gradient step per environment step, and a rollout-only leg (no updates) per N.

Method: each loop is warmed at its shape first (graph capture, allocator);
a sample is a window of at least --window seconds of back-to-back loop calls
ended by a device synchronise; host and device windows alternate inside this
one process; each is repeated --repeats times and reported as median with the
min..max spread.  Fails without a GPU.

    python tools/bench_rollout.py [--env point_mass|pendulum] [--num-envs 64,4096] [--legs device]
                                  [--window 2.0] [--repeats 3] [--out FILE]
--num-envs keeps the points with those N, --legs device skips the host loop
(a rollout-kernel comparison needs no host leg).  Prints one JSON line (and
writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "soft-actor-critic_amd")]
import torch  # noqa: E402


# --env name -> (module of the sac package, host class, policy_net.action_scale)
ENVS = {"point_mass": ("envs", "OneDPointMassReachEnv", 1.0), "pendulum": ("control_envs", "PendulumEnv", 2.0)}


def cfg(update_frequency, seed=0, env="point_mass"):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.1, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": ENVS[env][2]},
        "buffer": {"capacity": 1_000_000},
        "train": {"gradient_steps_per_update": 1, "update_frequency": update_frequency, "seed": seed,
                  "batch_size": 256, "warming_steps": 256, "device": "cuda", "precision": "fp32", "graph_chunk": 32},
        "logger": {"enabled": False, "env_name": env, "agent_name": "SAC", "log_episode_stats": False,
                   "log_q_values": False, "save_model": {"enabled": False, "path": None}},
    }


class Leg:
    """One loop at one shape: an agent and a call that runs `k` vector steps."""

    def __init__(self, kind, N, update_frequency, env="point_mass"):
        import importlib

        from sac.agent import SAC
        from sac.device_envs import DeviceVectorEnv
        from sac.vector_env import SyncVectorEnv

        self.N = N
        host_cls = getattr(importlib.import_module("sac." + ENVS[env][0]), ENVS[env][1])
        if kind == "device":
            self.agent = SAC(DeviceVectorEnv.from_env(host_cls(), N, device="cuda"), cfg(update_frequency, env=env))
            self.loop = self.agent.run_device_training_loop
        else:
            self.agent = SAC(SyncVectorEnv([host_cls] * N), cfg(update_frequency, env=env))
            self.loop = self.agent.run_vectorized_training_loop
        self.k = 4

    def call(self):
        m = self.loop(self.N * self.k)
        return m["total_env_steps"]

    def warm(self, target_s=0.4):
        """Warm the shape (first gradient steps, graph capture) and size a call to ~target_s."""
        self.call()
        torch.cuda.synchronize()
        for _ in range(3):
            t0 = time.perf_counter()
            self.call()
            torch.cuda.synchronize()
            dt = max(time.perf_counter() - t0, 1e-6)
            self.k = int(min(4096, max(2, self.k * target_s / dt)))

    def window(self, seconds):
        torch.cuda.synchronize()
        g0 = self.agent.engine.steps_done
        t0 = time.perf_counter()
        steps = 0
        while time.perf_counter() - t0 < seconds:
            steps += self.call()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return steps / el, (self.agent.engine.steps_done - g0) / el


def summarise(samples):
    env = [s[0] for s in samples]
    return {"env_steps_per_s": round(statistics.median(env), 1), "min": round(min(env), 1), "max": round(max(env), 1),
            "grad_steps_per_s": round(statistics.median(s[1] for s in samples), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--env", default="point_mass", choices=sorted(ENVS))
    ap.add_argument("--num-envs", default=None, help="comma-separated N: only the points with these")
    ap.add_argument("--legs", default="host,device", help="comma-separated: host, device")
    args = ap.parse_args()
    kinds = [k for k in ("host", "device") if k in args.legs.split(",")]
    if not kinds:
        raise SystemExit("bench_rollout: --legs names neither host nor device")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout: no HIP device visible")
    points = [(64, 64, "1 gradient step / vector step"), (1024, 1024, "1 gradient step / vector step"),
              (4096, 4096, "1 gradient step / vector step"), (64, 1, "1 gradient step / env step"),
              (64, 10 ** 12, "rollout only"), (1024, 10 ** 12, "rollout only"), (4096, 10 ** 12, "rollout only")]
    if args.num_envs:
        keep = {int(x) for x in args.num_envs.split(",")}
        points = [p for p in points if p[0] in keep]
    out = {"bench": "device_rollout", "env": f"{args.env} ({ENVS[args.env][1]} defaults)",
           "nets": "2x[256,256] fp32, B=256, buffer 1e6 rows", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "points": []}
    for N, uf, name in points:
        legs = {kind: Leg(kind, N, uf, args.env) for kind in kinds}
        for leg in legs.values():
            leg.warm()
        samples = {kind: [] for kind in kinds}
        for _ in range(args.repeats):  # host and device windows alternate
            for kind in kinds:
                samples[kind].append(legs[kind].window(args.window))
        p = {"num_envs": N, "schedule": name}
        p.update({kind: summarise(samples[kind]) for kind in kinds})
        if len(kinds) == 2:
            p["device_over_host"] = round(p["device"]["env_steps_per_s"] / p["host"]["env_steps_per_s"], 2)
        out["points"].append(p)
        for leg in legs.values():
            leg.agent.engine.close()
        del legs
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
