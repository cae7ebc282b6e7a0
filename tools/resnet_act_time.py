#!/usr/bin/env python3
"""What the ResNet actor's act costs, with the NatureCNN actor's beside it (DESIGN.md §15;
profiles/resnet).

128 frames already in HBM (the reference's act batch), A = 15, a quarter of the frames
deterministic, as bench.py's ``actor_act`` record (profiles/r06act).  Per dtype (fp32, bf16) and per
model (``resnet``: ImpalaResNetModel, ``nature``: AtariPPOModel):
  wall   ms per ``model.act`` call, results on the host: after --warmup calls and bench.py's
         settle (untimed calls for --settle-ms), the median, p90 and min of --steps calls
  event  device-event ms per call of --steps back-to-back engine-level act calls (no copies back)
in --runs alternating runs.  One JSON line per dtype.  With --once NAME that model's engine-level
act runs alone, --steps calls after the warm-up, for a kernel trace of its own.

usage: python tools/resnet_act_time.py [--steps 200] [--warmup 20] [--runs 3] [--settle-ms 250]
                                       [--dtypes fp32 bf16] [--once resnet|nature] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from impala_amd.model import AtariPPOModel  # noqa: E402
from impala_amd.resnet import ImpalaResNetModel  # noqa: E402

N, A = 128, 15


def settle(step, min_ms):
    t_end = time.perf_counter() + min_ms * 1e-3
    while True:
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            return


def wall(step, steps, warmup, settle_ms):
    for _ in range(warmup):
        step()
    settle(step, settle_ms)
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()  # (ends in a stream synchronize: the results are on the host)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(t)), 5), "p90": round(float(np.percentile(t, 90)), 5),
            "min": round(min(t), 5)}


def event(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / steps, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=250.0)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--once", default=None, choices=("resnet", "nature"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    obs = torch.randint(0, 256, (N, 3, 64, 64), dtype=torch.uint8, device=dev,
                        generator=torch.Generator(device=dev).manual_seed(3))
    det = torch.zeros(N, dtype=torch.bool)
    det[::4] = True
    det_dev = det.to(dev)
    lines = []
    for dtype in args.dtypes:
        models = {"resnet": ImpalaResNetModel((3, 64, 64), A, dev, dtype, seed=0),
                  "nature": AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)}
        full = {k: (lambda m=m: m.act(obs, det)) for k, m in models.items()}
        eng = {k: (lambda m=m: m._engine().act(obs, det_dev, seed=1, counter=1)) for k, m in models.items()}
        if args.once:
            out = {"dtype": dtype, "path": args.once, "frames": N, "calls": args.steps,
                   "event_ms": event(eng[args.once], args.steps, args.warmup)}
        else:
            out = {"dtype": dtype, "frames": N, "A": A, "steps": args.steps, "warmup": args.warmup,
                   "settle_ms": args.settle_ms, "wall_ms": {k: [] for k in models},
                   "event_ms": {k: [] for k in models}}
            for _ in range(args.runs):
                for k in models:
                    out["wall_ms"][k].append(wall(full[k], args.steps, args.warmup, args.settle_ms))
                    out["event_ms"][k].append(event(eng[k], args.steps, args.warmup))
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
