"""What replaying whole iterations of the device-resident training loop from one
hipGraph saves over issuing them from the host, on one MI355X.

  legs (SAC.run_device_training_loop over the point-mass probe env, 2x[256,256]
  nets, batch 256, a 1e6-row buffer, one gradient step per vector step, N = 64
  envs), each without Q-value logging and with device_q_values=True into a
  logger that only counts:
    stepwise   graph_steps = 0: one rollout launch, the gradient step's
               launches and (with Q logging) one q_values_replay launch per
               vector step, each issued by the host
    graph8     graph_steps = 8:  8 vector steps per hipGraph replay, the loop
    graph32    graph_steps = 32: 32 of them            cursor on the device

Method (that of tools/q_values_loop.py): every leg is warmed at its shape; a
sample is a window of at least --window seconds of back-to-back loop calls
ended by a device synchronise, the legs alternating inside this one process;
repeated --repeats times: median, min..max.  Every loop call starts with the
warm-up (4 vector steps at N = 64), which runs stepwise in every leg; a call is
sized to about 0.3 s, so that is well under 1 % of it.  --legs stepwise runs on
a tree without the feature too (nothing new is imported or passed), which is
how the parent commit's loop is measured.  Fails without a GPU.

    python tools/loop_graph_bench.py [--precision fp32] [--legs stepwise graph8 graph32] [--out FILE]
Prints one JSON line (and appends it to --out).
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

GRAPH_STEPS = {"stepwise": 0, "graph8": 8, "graph32": 32}


def cfg(update_frequency, precision, log_q):
    return {
        "sac": {"gamma": 0.99, "tau": 0.005, "alpha": 0.1, "auto_entropy_tuning": True, "actor_lr": 3e-4,
                "critic_lr": 3e-4, "alpha_lr": 3e-4},
        "q_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity"},
        "policy_net": {"hidden_sizes": [256, 256], "hidden_layers_act": "relu", "output_activation": "identity",
                       "log_std_min": -20, "log_std_max": 2, "action_scale": 1.0},
        "buffer": {"capacity": 1_000_000},
        "train": {"gradient_steps_per_update": 1, "update_frequency": update_frequency, "seed": 0,
                  "batch_size": 256, "warming_steps": 256, "device": "cuda", "precision": precision,
                  "graph_chunk": 32},
        "logger": {"enabled": False, "env_name": "point_mass", "agent_name": "SAC", "log_episode_stats": False,
                   "log_q_values": log_q, "save_model": {"enabled": False, "path": None}},
    }


class CountingLogger:
    def __init__(self):
        self.n = 0

    def log_q_values(self, q1, q2, step):
        self.n += 1

    def log_hparams(self, cfg, metrics):
        pass


class LoopLeg:
    def __init__(self, leg, q, N, precision):
        from sac.agent import SAC
        from sac.device_envs import DeviceVectorEnv

        self.N, self.k = N, 64
        self.agent = SAC(DeviceVectorEnv("point_mass", N, device="cuda"), cfg(N, precision, q))
        self.kw = {"logger": CountingLogger(), "device_q_values": True} if q else {}
        if GRAPH_STEPS[leg]:
            self.kw["graph_steps"] = GRAPH_STEPS[leg]

    def call(self):
        return self.agent.run_device_training_loop(self.N * self.k, **self.kw)["total_env_steps"]

    def warm(self, target_s=0.3):
        self.call()
        torch.cuda.synchronize()
        for _ in range(3):
            t0 = time.perf_counter()
            self.call()
            torch.cuda.synchronize()
            dt = max(time.perf_counter() - t0, 1e-6)
            # whole blocks of 32 after the 4 warm-up steps, so that no leg has a stepwise tail
            self.k = 4 + 32 * int(min(256, max(2, self.k * target_s / dt / 32)))

    def window(self, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        while time.perf_counter() - t0 < seconds:
            steps += self.call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (steps / self.N) * 1e6  # us per vector step


def spread(xs, digits=2):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--legs", nargs="+", default=list(GRAPH_STEPS), choices=list(GRAPH_STEPS))
    ap.add_argument("--q", nargs="+", default=["off", "device_q"], choices=["off", "device_q"])
    ap.add_argument("--window", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_graph_bench: no HIP device visible")
    out = {"bench": "loop_graph", "label": args.label, "precision": args.precision, "num_envs": args.envs,
           "nets": "2x[256,256], B=256, buffer 1e6 rows, 1 gradient step / vector step",
           "unit": "us per vector step", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "points": {}}
    for q in args.q:
        legs = {leg: LoopLeg(leg, q == "device_q", args.envs, args.precision) for leg in args.legs}
        for leg in legs.values():
            leg.warm()
        samples = {leg: [] for leg in legs}
        for _ in range(args.repeats):  # the legs alternate
            for name, leg in legs.items():
                samples[name].append(leg.window(args.window))
        p = {name: spread(xs) for name, xs in samples.items()}
        p["vector_steps_per_call"] = {name: leg.k for name, leg in legs.items()}
        for leg in legs.values():
            leg.agent.engine.close()
        out["points"][q] = p
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
