"""Edge frame counts of the per-frame kernels (conv1.h conv12_fwd_body with its conv3 tail,
conv12_bwd_body / conv12_bwd_body_f32; lnc3.h).

A workgroup of these kernels takes a contiguous run of frames.  Their frame loops compute the
lane offsets once and advance them, keep their padding as zeroed LDS rows or out-of-range buffer
offsets instead of tests, and branch on the wave index; what that can get wrong shows at the
ends of a run, not at the benchmark's 1280 frames: a run of one frame (no steady state, the
pipelines' prologue and epilogue only), a run shorter than the conv3 tail's five frame slots, a
full run, and a ragged last workgroup.

Shapes B x T: 1x1, 1x2, 1x5, 2x3, 1x11 -> N = 1, 2, 5, 6, 11 frames, under two run lengths:
  default  one frame per workgroup at these N (frames / CUs, rounded up): the fused backward
           launch (lnc3_conv12_bwd) and, for the replay-row path, the ObsRows instantiations;
  run5     IMPALA_C12F_FPW = IMPALA_C1_FPW = 5 (read in impala_create): 5-frame runs in the forward
           (all five tail slots; N = 1, 2 shorter, 5 equal, 6 and 11 longer with a ragged last
           workgroup of 1 frame) and in the conv2-dgrad / conv1-wgrad body (its two-group
           pipeline over 1..5 frames; launched on its own beside lnc3_bwd, the host fuses the
           two only at equal run lengths).
T = 1 has no V-trace step (the oracle's scan is empty and impala_create refuses T < 2), so N = 1
is a forward case only; the steps run at the other four shapes.

Reference: the float64 oracle step (oracle/ref_cpu.py train_step_fp64) on the same parameters
and synthetic batch.  fp32 holds the bounds of tests/test_gpu_parity_full.py for the same
quantities: metrics 1e-5 relative, post-clip gradient 1e-5 rel-L2, parameters after the step
1e-6, and the forward's logits / values normwise 1e-5 (|d| <= 1e-5 (|x| + rms x), that file's
bound for values that cross zero).  The native fp32 CPU oracle itself, run here without a GPU at
these shapes, is inside them except for one figure: metrics <= 7e-7 except grad_norm 1.7e-6 ..
6.3e-6 and the loss at 1x11, 1.2e-5 (a cancelling sum, -4.65 + 4.86 - 0.02 = 0.19, that
torch's CPU arithmetic misses by a hair); gradient rel-L2 1.9e-6 .. 6.6e-6; parameters 6e-8.  The
bounds stand as they are for every quantity, that loss included (the kernels' is 3.2e-6, their
worst loss over the shapes 3.6e-6: they round this sum as float64 does).  Those bounds are fp32 bounds (1e-5 = 2^-17 is below bf16's unit
roundoff 2^-9): bf16 holds the suite's one-step bf16 bounds instead (tests/test_gpu_parity.py, as
tests/test_gpu_wgrad_edges.py does): metrics 5e-2 relative + 5e-3, gradient cosine > 0.99,
forward rel-L2 3e-2 (logits) and 5e-2 (values).

Every case runs twice on fresh handles and must equal itself bit for bit; the replay-row step
(impala_train_step_rows, a permuted row map into a larger ring) must equal the direct step bit
for bit.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
A = 15
NAMES = ("loss", "entropy", "td", "pg", "kl", "ratio", "grad_norm")
RTOL = 1e-5      # test_gpu_parity_full.py: metrics, normwise forward values
GRAD_RL2 = 1e-5  # post-clip gradient, rel-L2
PARAM_ABS = 1e-6  # parameters after one step
SHAPES = [(1, 1), (1, 2), (1, 5), (2, 3), (1, 11)]
STEP_SHAPES = [s for s in SHAPES if s[1] >= 2]
PLANS = {"default": {}, "run5": {"IMPALA_C12F_FPW": "5", "IMPALA_C1_FPW": "5"}}
_ids = lambda s: f"B{s[0]}_T{s[1]}"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_ORACLE = {}


def oracle(shape):
    """float64 reference of a shape, computed once: forward logits / values of its N frames and,
    for T >= 2, the step's post-clip gradient, metrics and updated parameters."""
    if shape not in _ORACLE:
        B, T = shape
        batch = ref_cpu.synthetic_batch(B, T, A, seed=1234)
        flat0 = ref_cpu.flat_params(ref_cpu.make_model(0, A))
        ref = ref_cpu.RefModel(A).double()
        ref_cpu.load_flat(ref, flat0.astype(np.float64))
        with torch.no_grad():
            lg, v = ref(torch.from_numpy(batch[0].reshape(-1, 3, 64, 64)).double())
        out = {"batch": batch, "flat0": flat0, "logits": lg.numpy(), "values": v.numpy()}
        if T >= 2:
            p64, g64, met64 = ref_cpu.train_step_fp64(flat0, batch, A)
            out.update(p=p64, g=np.asarray(g64, np.float64),
                       met=np.array([met64["train/" + k] for k in NAMES], np.float64))
        _ORACLE[shape] = out
    return _ORACLE[shape]


def _handle(shape, dtype, plan, monkeypatch):
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    B, T = shape
    m = AtariPPOModel((3, 64, 64), A, device=_dev(), dtype=dtype)
    m.load_flat(oracle(shape)["flat0"])
    e = Engine(m, batch_size=B, rollout_length=max(T, 2))
    m._train_engine = e
    return m, e


def _forward(shape, dtype, plan, monkeypatch):
    m, e = _handle(shape, dtype, plan, monkeypatch)
    obs = torch.from_numpy(oracle(shape)["batch"][0].reshape(-1, 3, 64, 64)).to(_dev())
    lg, v = e.forward(obs)
    torch.cuda.synchronize()
    out = lg.cpu().numpy().copy(), v.cpu().numpy().copy()
    e.close()
    return out


def _step(shape, dtype, plan, monkeypatch, rows=False):
    """One learner step -> (post-clip gradient, metrics, parameters)."""
    dev = _dev()
    m, e = _handle(shape, dtype, plan, monkeypatch)
    batch = oracle(shape)["batch"]
    if rows:
        # the batch's trajectories scattered over a ring of B + 3 slots (the others hold other
        # data), read in place through the row map
        B = shape[0]
        C = B + 3
        perm = np.random.default_rng(5).permutation(C)[:B].astype(np.int64)
        other = ref_cpu.synthetic_batch(C, shape[1], A, seed=77)
        ring = []
        for f, o in zip(batch, other):
            r = np.ascontiguousarray(o).copy()
            r[perm] = f
            ring.append(torch.from_numpy(r).to(dev))
        e.train_step_rows(ring, perm)
    else:
        e.train_step(*[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in batch])
    torch.cuda.synchronize()
    out = (m.flat_grad.cpu().numpy().copy(), e.metrics.cpu().numpy()[:7].copy(),
           m.flat.cpu().numpy().copy())
    e.close()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_frame_edges(shape, dtype, plan, monkeypatch):
    lg, v = _forward(shape, dtype, plan, monkeypatch)
    lg2, v2 = _forward(shape, dtype, plan, monkeypatch)
    assert np.array_equal(_bits(lg), _bits(lg2)) and np.array_equal(_bits(v), _bits(v2))
    o = oracle(shape)
    assert np.isfinite(lg).all() and np.isfinite(v).all()
    for name, got, want in (("logits", lg, o["logits"]), ("values", v, o["values"])):
        want = want.reshape(got.shape)
        rms = float(np.sqrt(np.mean(want ** 2)))
        worst = float(np.max(np.abs(got - want) / (np.abs(want) + rms)))
        rl2 = _rel_l2(got, want)
        print(f"{dtype} {shape} {plan} forward {name}: normwise {worst:.2e}, rel-L2 {rl2:.2e}")
        if dtype == "fp32":
            assert worst <= RTOL, (name, worst)
        else:
            assert rl2 < (3e-2 if name == "logits" else 5e-2), (name, rl2)


@pytest.mark.parametrize("source", ["direct", "rows", "run5"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=_ids)
def test_step_frame_edges(shape, dtype, source, monkeypatch):
    plan = "run5" if source == "run5" else "default"
    g, met, p = _step(shape, dtype, plan, monkeypatch, rows=source == "rows")
    g2, met2, p2 = _step(shape, dtype, plan, monkeypatch, rows=source == "rows")
    for a, b in ((g, g2), (met, met2), (p, p2)):
        assert np.array_equal(_bits(a), _bits(b)), "the step is not bitwise reproducible"
    if source == "rows":  # the in-place read is the direct step, bit for bit
        gd, metd, pd = _step(shape, dtype, plan, monkeypatch)
        for a, b in ((g, gd), (met, metd), (p, pd)):
            assert np.array_equal(_bits(a), _bits(b)), "rows step differs from the direct step"
    o = oracle(shape)
    assert np.isfinite(g).all() and np.isfinite(met).all() and np.isfinite(p).all()
    rel = np.abs(met - o["met"]) / np.maximum(np.abs(o["met"]), 1e-30)
    rl2 = _rel_l2(g, o["g"])
    cos = float(np.dot(g, o["g"]) / (np.linalg.norm(g) * np.linalg.norm(o["g"])))
    dp = float(np.abs(p - o["p"]).max())
    print(f"{dtype} {shape} {source}: metrics rel " + ", ".join(f"{k} {r:.1e}" for k, r in zip(NAMES, rel))
          + f"; grad rel-L2 {rl2:.2e}, cosine {cos:.5f}; params max |d| {dp:.2e}")
    if dtype == "fp32":
        for k, r in zip(NAMES, rel):
            assert r <= RTOL, (k, r)
        assert rl2 <= GRAD_RL2, rl2
        assert dp <= PARAM_ABS, dp
    else:
        assert np.all(np.abs(met - o["met"]) <= 5e-2 * np.abs(o["met"]) + 5e-3), (met, o["met"])
        assert cos > 0.99, cos
