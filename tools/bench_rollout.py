"""Environment steps per second of the training loop over the point-mass probe
env, host-stepped against device-resident, on one MI355X.

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

    python tools/bench_rollout.py [--window 2.0] [--repeats 3] [--out FILE]
Prints one JSON line (and writes it to --out).
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


def cfg(update_frequency, seed=0):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.1, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": 1.0},
        "buffer": {"capacity": 1_000_000},
        "train": {"gradient_steps_per_update": 1, "update_frequency": update_frequency, "seed": seed,
                  "batch_size": 256, "warming_steps": 256, "device": "cuda", "precision": "fp32", "graph_chunk": 32},
        "logger": {"enabled": False, "env_name": "point_mass", "agent_name": "SAC", "log_episode_stats": False,
                   "log_q_values": False, "save_model": {"enabled": False, "path": None}},
    }


class Leg:
    """One loop at one shape: an agent and a call that runs `k` vector steps."""

    def __init__(self, kind, N, update_frequency):
        from sac.agent import SAC
        from sac.device_envs import DeviceVectorEnv
        from sac.envs import OneDPointMassReachEnv
        from sac.vector_env import SyncVectorEnv

        self.N = N
        if kind == "device":
            self.agent = SAC(DeviceVectorEnv("point_mass", N, device="cuda"), cfg(update_frequency))
            self.loop = self.agent.run_device_training_loop
        else:
            self.agent = SAC(SyncVectorEnv([OneDPointMassReachEnv] * N), cfg(update_frequency))
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout: no HIP device visible")
    points = [(64, 64, "1 gradient step / vector step"), (1024, 1024, "1 gradient step / vector step"),
              (4096, 4096, "1 gradient step / vector step"), (64, 1, "1 gradient step / env step"),
              (64, 10 ** 12, "rollout only"), (1024, 10 ** 12, "rollout only"), (4096, 10 ** 12, "rollout only")]
    out = {"bench": "device_rollout", "env": "point_mass (OneDPointMassReachEnv defaults)",
           "nets": "2x[256,256] fp32, B=256, buffer 1e6 rows", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "points": []}
    for N, uf, name in points:
        legs = {"host": Leg("host", N, uf), "device": Leg("device", N, uf)}
        for leg in legs.values():
            leg.warm()
        samples = {"host": [], "device": []}
        for _ in range(args.repeats):  # host and device windows alternate
            for kind in ("host", "device"):
                samples[kind].append(legs[kind].window(args.window))
        p = {"num_envs": N, "schedule": name, "host": summarise(samples["host"]),
             "device": summarise(samples["device"])}
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
