#!/usr/bin/env python3
"""What the IMPALA ResNet learner step costs on the HIP path (profiles/resnet_step).

At B = 64, T = 20, A = 15 (1280 frames), the batch already in HBM, per --dtype, device-event ms per call
of --steps back-to-back calls of
  step    ``ResnetEngine.train_step``: the one call (``resnet_train_step``)
  fwdbwd  ``forward_train`` + ``backward`` alone, on fixed cotangents
  parts   the composition without the one call: ``forward_train``, the V-trace loss in torch,
          ``backward`` through autograd, torch ``clip_grad_norm_`` + ``torch.optim.Adam``, the re-pack
in --runs alternating runs; ``spread`` is (max - min) / min over a path's runs.  One JSON line per dtype.
With --once step|fwdbwd|parts that path runs alone, for a kernel trace of its own.

usage: python tools/resnet_step_time.py [--steps 20] [--warmup 5] [--runs 3] [--dtype fp32 bf16]
                                        [--once step|fwdbwd|parts] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from impala_amd.resnet import ImpalaResNetModel  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.vtrace import mode_kwargs  # noqa: E402
from resnet_grad_time import event  # noqa: E402

B, T, A = 64, 20, 15


def paths(dtype, batch):
    dev, n = batch[0].device, B * T
    obs = batch[0].flatten(0, 1)

    def model():
        return ImpalaResNetModel((3, 64, 64), A, dev, "fp32", seed=0, train_batch=n, train_dtype=dtype)
    m = model()
    eng = m.train_engine()
    eng.step_init(B, T)
    m2 = model()
    eng2, grad = m2.train_engine(), torch.empty_like(m2.flat)
    gen = torch.Generator(device=dev).manual_seed(3)
    dl, dv = torch.randn(n, A, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)

    def fwdbwd():
        eng2.forward_train(obs)
        eng2.backward(dl, dv, out=grad)
    m3 = model()
    opt = torch.optim.Adam(m3.parameters(), lr=1e-4, eps=1e-5)

    def parts():
        opt.zero_grad(set_to_none=False)
        lg, v = m3.forward_train(obs)
        pi = torch.distributions.Categorical(logits=lg.reshape(B, T, A))
        pim = torch.distributions.Categorical(logits=batch[4])
        v = v.reshape(B, T)
        rho = torch.exp(pi.log_prob(batch[1]) - pim.log_prob(batch[1]))
        adv, err, _ = ref_cpu.batched_vtrace(v[:, :-1], v[:, 1:], batch[2][:, :-1], batch[3][:, :-1], rho[:, :-1],
                                             **mode_kwargs("sg_advantage"))
        (-(pi.log_prob(batch[1])[:, :-1] * adv).mean() + err.pow(2).mean() - 0.01 * pi.entropy().mean()).backward()
        torch.nn.utils.clip_grad_norm_(m3.parameters(), 0.5)
        opt.step()
        m3.params_changed()
        m3.train_engine()._fresh()
    return {"step": lambda: eng.train_step(*batch), "fwdbwd": fwdbwd, "parts": parts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["fp32", "bf16"], choices=("fp32", "bf16"))
    ap.add_argument("--once", default=None, choices=("step", "fwdbwd", "parts"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batch = [torch.from_numpy(x).to(dev) for x in ref_cpu.synthetic_batch(B, T, A, seed=7)]
    lines = []
    for dtype in args.dtype:
        p = paths(dtype, batch)
        if args.once:
            out = {"dtype": dtype, "path": args.once, "calls": args.steps,
                   "event_ms": event(p[args.once], args.steps, args.warmup)}
        else:
            out = {"dtype": dtype, "B": B, "T": T, "A": A, "steps": args.steps, "warmup": args.warmup,
                   "event_ms": {k: [] for k in p}}
            for _ in range(args.runs):
                for k in p:
                    out["event_ms"][k].append(event(p[k], args.steps, args.warmup))
            out["spread"] = {k: round((max(v) - min(v)) / min(v), 4) for k, v in out["event_ms"].items()}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
