"""What per-env-step Q-value logging costs the device-resident training loop,
and the critic-evaluation kernel against the eager two-forward path, on one
MI355X.

  loop legs (SAC.run_device_training_loop over the point-mass probe env,
  2x[256,256] nets, batch 256, a 1e6-row buffer, one gradient step per vector
  step, N envs):
    off        logger.log_q_values off (the loop as it was before the feature)
    device_q   log_q_values on, device_q_values=True: one sac_q_values_replay
               launch per vector step into the device ring, drained every 64
               vector steps into a logger that only counts
  per-call legs (the N rows of one vector step, read from the replay ring):
    kernel     SacEngine.q_values_replay(replay, 0, N, out=cell): one launch
    eager      q_net1(s', a) and q_net2(s', a) on the same rows as device
               tensors, written into the same cell: what QValueLog.record runs
               once its rows are on the device (the fp32 modules)

Method: every leg is warmed at its shape; a loop sample is a window of at least
--window seconds of back-to-back loop calls ended by a device synchronise, the
legs alternating inside this one process; a per-call sample is --calls calls
ended by a synchronise.  Each is repeated --repeats times: median, min..max.
--legs off runs on a tree without the feature too (nothing new is imported),
which is how the parent commit's loop is measured.  Fails without a GPU.

    python tools/q_values_loop.py [--envs 64 1024] [--precision fp32] [--legs off device_q calls] [--out FILE]
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
    def __init__(self, kind, N, precision):
        from sac.agent import SAC
        from sac.device_envs import DeviceVectorEnv

        self.N, self.k = N, 4
        self.agent = SAC(DeviceVectorEnv("point_mass", N, device="cuda"), cfg(N, precision, kind == "device_q"))
        self.kw = {"logger": CountingLogger(), "device_q_values": True} if kind == "device_q" else {}

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
            self.k = int(min(4096, max(2, self.k * target_s / dt)))

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


def per_call(N, precision, calls, repeats):
    """us per call of the kernel and of the eager two-forward path on the same N replay rows."""
    leg = LoopLeg("off", N, precision)
    leg.call()  # fills the first rows of the ring
    agent, rb, eng = leg.agent, leg.agent.replay_buffer, leg.agent.engine
    cell = torch.empty(N, 2, device="cuda")
    s2, a = rb.next_obs[:N], rb.act[:N]

    def kernel():
        eng.q_values_replay(rb, 0, N, out=cell)

    def eager():
        with torch.no_grad():
            cell[:, 0] = agent.q_net1(s2, a).reshape(-1)
            cell[:, 1] = agent.q_net2(s2, a).reshape(-1)

    out = {}
    for name, f in (("kernel", kernel), ("eager", eager)):
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        out[name] = []
    for _ in range(repeats):  # the two alternate
        for name, f in (("kernel", kernel), ("eager", eager)):
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / calls * 1e6)
    eng.close()
    return {k: spread(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--legs", nargs="+", default=["off", "device_q", "calls"])
    ap.add_argument("--window", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("q_values_loop: no HIP device visible")
    out = {"bench": "q_values_loop", "label": args.label, "precision": args.precision,
           "nets": "2x[256,256], B=256, buffer 1e6 rows, 1 gradient step / vector step",
           "unit": "us per vector step (loop legs), us per call (per-call legs)", "window_s": args.window,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "points": []}
    for N in args.envs:
        p = {"num_envs": N}
        kinds = [k for k in ("off", "device_q") if k in args.legs]
        legs = {k: LoopLeg(k, N, args.precision) for k in kinds}
        for leg in legs.values():
            leg.warm()
        samples = {k: [] for k in kinds}
        for _ in range(args.repeats):  # the legs alternate
            for k in kinds:
                samples[k].append(legs[k].window(args.window))
        for k in kinds:
            p[k] = spread(samples[k])
            legs[k].agent.engine.close()
        if "off" in p and "device_q" in p:
            p["device_q_minus_off_us"] = round(p["device_q"]["median"] - p["off"]["median"], 2)
        if "calls" in args.legs:
            p["per_call"] = per_call(N, args.precision, args.calls, args.repeats)
        out["points"].append(p)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
