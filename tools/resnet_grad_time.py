#!/usr/bin/env python3
"""What the ResNet's forward_train + backward costs on the HIP path, with the same network in torch
float32 on the device beside it (profiles/resnet_backward, profiles/resnet_backward_bf16).

Per n (160: the IMPALA config's 8 x 20 frames; 1280: 64 x 20), observations already in HBM, A = 15,
standard-normal cotangents:
  hip    device-event ms per ``ResnetEngine.forward_train`` + ``backward`` of --steps back-to-back calls,
         one path per --dtype: ``hip`` the fp32 engine, ``hip_bf16`` the bf16 one
  torch  the yardstick: the network restated with tests/resnet_oracle.py's functions on float32
         device tensors, forward + ``torch.autograd.grad``, timed the same way
in --runs alternating runs; ``spread`` is (max - min) / min over a path's runs.  One JSON line per n.
With --once hip|hip_bf16|torch that path runs alone at --n, --steps calls after the warm-up, for a kernel
trace of its own.

usage: python tools/resnet_grad_time.py [--steps 20] [--warmup 5] [--runs 3] [--n 160 1280]
                                        [--dtype fp32 bf16] [--once hip|hip_bf16|torch] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import resnet_oracle as orc  # noqa: E402
from impala_amd.resnet import ImpalaResNetModel, ResnetEngine  # noqa: E402

A = 15


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


def torch_step(P, obs, dl, dv):
    keys = list(P)

    def step():
        x = obs.to(torch.float32) / 255
        for s in range(3):
            x = orc.pooled(x, P, 5 * s)
            for b in (1, 3):
                x = orc.res_x(x, orc.res_t(x, P, 5 * s + b), P, 5 * s + b + 1)
        lg, v = orc.heads(orc.fc(orc.layer_norm(orc.features(x), P), P), P)
        return torch.autograd.grad((lg * dl).sum() + (v * dv).sum(), [P[k] for k in keys])
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[160, 1280])
    ap.add_argument("--dtype", nargs="+", default=["fp32"], choices=("fp32", "bf16"))
    ap.add_argument("--once", default=None, choices=("hip", "hip_bf16", "torch"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = ImpalaResNetModel((3, 64, 64), A, dev, "fp32", seed=0)
    P = {k: v.to(dev, torch.float32).requires_grad_()
         for k, v in orc.params(model.flat.cpu().numpy(), A).items()}
    lines = []
    for n in args.n:
        gen = torch.Generator(device=dev).manual_seed(3)
        obs = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, device=dev, generator=gen)
        dl = torch.randn(n, A, device=dev, generator=gen)
        dv = torch.randn(n, device=dev, generator=gen)
        grad = torch.empty_like(model.flat)

        def hip(dtype):
            eng = ResnetEngine(model, n, dtype, train=True)

            def step():
                eng.forward_train(obs)
                eng.backward(dl, dv, out=grad)
            return step
        dtypes = args.dtype + (["bf16"] if args.once == "hip_bf16" and "bf16" not in args.dtype else [])
        paths = {"hip" if d == "fp32" else "hip_bf16": hip(d) for d in dtypes}
        paths["torch"] = torch_step(P, obs, dl, dv)
        if args.once:
            out = {"n": n, "path": args.once, "calls": args.steps,
                   "event_ms": event(paths[args.once], args.steps, args.warmup)}
        else:
            out = {"n": n, "A": A, "steps": args.steps, "warmup": args.warmup,
                   "event_ms": {k: [] for k in paths}}
            for _ in range(args.runs):
                for k in paths:
                    out["event_ms"][k].append(event(paths[k], args.steps, args.warmup))
            out["spread"] = {k: round((max(v) - min(v)) / min(v), 4) for k, v in out["event_ms"].items()}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del paths
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
