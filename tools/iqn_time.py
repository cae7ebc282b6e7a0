#!/usr/bin/env python3
"""What the distributional actor's act costs beside the dueling one's (DESIGN.md §14;
profiles/iqn).

128 frames (the reference's act batch), A = 15.  Per dtype (fp32, bf16): host wall time and device
event time per call over --steps calls after --warmup, for
  iqn_act at W = 8 and W = 32  (two forwards of 128 W rows each, library-drawn taus)
  dqn_act                      (two forwards of 128 rows)
in --runs alternating runs iqn8, iqn32, dqn, iqn8, ...  Prints one JSON line per dtype with each
run's figures, the means and the run-to-run spreads.  With --once NAME it runs that path alone,
--steps calls after the warm-up, for a kernel trace of its own.

usage: python tools/iqn_time.py [--steps 200] [--warmup 20] [--runs 4] [--dtypes fp32 bf16]
                                [--once iqn8|iqn32|dqn] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from impala_amd.dqn import AtariDQNModel, DqnEngine  # noqa: E402
from impala_amd.iqn import DistributionalAtariDQN, IqnEngine  # noqa: E402

N, A = 128, 15


def timed(step, steps, warmup):
    """-> (host wall ms per call, device event ms per call) of `steps` back-to-back calls."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return wall, e0.elapsed_time(e1) / steps


def paths(dev, dtype):
    obs = torch.randint(0, 256, (N, 3, 64, 64), dtype=torch.uint8, device=dev,
                        generator=torch.Generator(device=dev).manual_seed(3))
    counter = [0]
    out, keep = {}, []
    for W in (8, 32):
        m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
        e = IqnEngine(m, batch_size=N)
        keep.append((m, e))

        def step(e=e):
            counter[0] += 1
            e.act(obs, 0.4, seed=1, counter=counter[0])
        out[f"iqn{W}"] = step
    m = AtariDQNModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
    e = DqnEngine(m, batch_size=N, inference_only=True)
    keep.append((m, e))

    def step_d(e=e):
        counter[0] += 1
        e.act(obs, 0.4, seed=1, counter=counter[0])
    out["dqn"] = step_d
    return out, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--once", default=None, help="run this path alone (iqn8, iqn32 or dqn)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for dtype in args.dtypes:
        steps, keep = paths(dev, dtype)
        if args.once:
            wall, ev = timed(steps[args.once], args.steps, args.warmup)
            line = json.dumps({"dtype": dtype, "path": args.once, "frames": N, "calls": args.steps,
                               "wall_ms": round(wall, 5), "event_ms": round(ev, 5)})
        else:
            runs = {k: [] for k in steps}
            for _ in range(args.runs):
                for name, fn in steps.items():
                    runs[name].append(timed(fn, args.steps, args.warmup))
            out = {"dtype": dtype, "frames": N, "A": A, "steps": args.steps, "warmup": args.warmup}
            for kind, col in (("wall_ms", 0), ("event_ms", 1)):
                v = {k: [round(r[col], 5) for r in rs] for k, rs in runs.items()}
                out[kind] = {"runs": v, "mean": {k: round(float(np.mean(x)), 5) for k, x in v.items()},
                             "spread": {k: round(max(x) - min(x), 5) for k, x in v.items()}}
            line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        for _, e in keep:
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
