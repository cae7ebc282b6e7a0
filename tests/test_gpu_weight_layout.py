"""The kernel-layout weight copies have two writers: the Adam kernel re-emits every weight it
updates, and pack_params derives all of them from the canonical parameters (bind time,
refresh_weights).  Both go through write_shadow and the index maps of net.h (w2t_index /
w3t_index for the fp32 dgrad copies, whose order is the order the waves load them in), and both
must leave every copy in the same state.

Handle A runs two learner steps; its second step reads what Adam emitted after the first.  Handle
B runs one step, re-derives the copies from the canonical parameters (params_changed +
refresh_weights) and runs the second step on those.  Parameters, gradient, Adam moments and
metrics after the second step must be equal bit for bit, at the shapes B x T = 1x2 and 2x3 under
the two run lengths of tests/test_gpu_frame_edges.py (default: the fused backward launch; run5:
the unfused lnc3_bwd / conv12_bwd_s2d, which share the loaders), in fp32 and bf16.

Both steps are also held to the float64 oracle (oracle/ref_cpu.py train_step_fp64, one and two
steps) with the bounds of tests/test_gpu_frame_edges.py: fp32 metrics 1e-5 relative, post-clip
gradient 1e-5 rel-L2, parameters 1e-6; bf16 metrics 5e-2 relative + 5e-3, gradient cosine > 0.99.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
A = 15
NAMES = ("loss", "entropy", "td", "pg", "kl", "ratio", "grad_norm")
RTOL = 1e-5
GRAD_RL2 = 1e-5
PARAM_ABS = 1e-6
SHAPES = [(1, 2), (2, 3)]
PLANS = {"default": {}, "run5": {"IMPALA_C12F_FPW": "5", "IMPALA_C1_FPW": "5"}}

_ORACLE = {}


def oracle(shape):
    """float64 reference of a shape, computed once: (parameters, post-clip gradient, metrics)
    after one step and after two."""
    if shape not in _ORACLE:
        B, T = shape
        batch = ref_cpu.synthetic_batch(B, T, A, seed=1234)
        flat0 = ref_cpu.flat_params(ref_cpu.make_model(0, A))
        steps = []
        for n in (1, 2):
            p, g, met = ref_cpu.train_step_fp64(flat0, batch, A, steps=n)
            steps.append((p, np.asarray(g, np.float64),
                          np.array([met["train/" + k] for k in NAMES], np.float64)))
        _ORACLE[shape] = {"batch": batch, "flat0": flat0, "steps": steps}
    return _ORACLE[shape]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _state(m, e):
    torch.cuda.synchronize()
    return {"params": m.flat.cpu().numpy().copy(), "grad": m.flat_grad.cpu().numpy().copy(),
            "exp_avg": e.exp_avg.cpu().numpy().copy(), "exp_avg_sq": e.exp_avg_sq.cpu().numpy().copy(),
            "metrics": e.metrics.cpu().numpy()[:7].copy()}


def _two_steps(shape, dtype, repack):
    """-> the state after step 1 and after step 2; `repack`: the kernel-layout weights are derived
    again from the canonical parameters between the steps."""
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    dev = torch.device("cuda:0")
    o = oracle(shape)
    m = AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype)
    m.load_flat(o["flat0"])
    e = Engine(m, batch_size=shape[0], rollout_length=shape[1])
    m._train_engine = e
    batch = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in o["batch"]]
    e.train_step(*batch)
    s1 = _state(m, e)
    if repack:
        m.params_changed()
        e.refresh_weights()
    e.train_step(*batch)
    s2 = _state(m, e)
    e.close()
    return s1, s2


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_T{s[1]}")
def test_adam_and_pack_emit_the_same_weights(shape, dtype, plan, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    a1, a2 = _two_steps(shape, dtype, repack=False)
    b1, b2 = _two_steps(shape, dtype, repack=True)
    for sa, sb, what in ((a1, b1, "step 1"), (a2, b2, "step 2")):
        for k in sa:
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), \
                f"{what}: {k} differs between Adam-emitted and re-packed kernel weights"
    for n, s in enumerate((a1, a2)):
        p64, g64, met64 = oracle(shape)["steps"][n]
        g, met, p = s["grad"], s["metrics"], s["params"]
        assert np.isfinite(g).all() and np.isfinite(met).all() and np.isfinite(p).all()
        rel = np.abs(met - met64) / np.maximum(np.abs(met64), 1e-30)
        rl2 = float(np.linalg.norm(g - g64) / max(np.linalg.norm(g64), 1e-30))
        cos = float(np.dot(g, g64) / (np.linalg.norm(g) * np.linalg.norm(g64)))
        dp = float(np.abs(p - p64).max())
        print(f"{dtype} {shape} {plan} step {n + 1}: metrics rel "
              + ", ".join(f"{k} {r:.1e}" for k, r in zip(NAMES, rel))
              + f"; grad rel-L2 {rl2:.2e}, cosine {cos:.5f}; params max |d| {dp:.2e}")
        if dtype == "fp32":
            for k, r in zip(NAMES, rel):
                assert r <= RTOL, (n + 1, k, r)
            assert rl2 <= GRAD_RL2, (n + 1, rl2)
            assert dp <= PARAM_ABS, (n + 1, dp)
        else:
            assert np.all(np.abs(met - met64) <= 5e-2 * np.abs(met64) + 5e-3), (n + 1, met, met64)
            assert cos > 0.99, (n + 1, cos)
