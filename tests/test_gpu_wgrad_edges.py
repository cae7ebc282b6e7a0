"""Edge shapes of the split weight-gradient GEMM (gemm.h gemm_wg_body: conv3, conv2 and FC
weight gradients, fp32 one 4-wave group per workgroup, bf16 two groups on interleaved chunks).

The staging loop leans on the buffer descriptors for its bounds (X rows past a split's end read
as zero), advances its row offsets by constants (X, FC, conv3) or by a per-lane cursor (conv2)
and skips the chunks that pad a split to the prefetch depth.  What that can get wrong shows at
small and ragged reductions, not at the benchmark's: a split's ragged last chunk, the zero-fill
boundary inside a chunk, splits shorter than the prefetch ring, the conv2 cursor across frame
boundaries, split starts, and the two-group bf16 interleave.

Shapes: N = B * T frames small and odd, so M is no multiple of the 32- (fp32) or 64-row (bf16)
chunk: (1, 3), (2, 5), (3, 7) -> conv3 M = 48 / 160 / 336, conv2 M = 108 / 360 / 756, FC
M = 3 / 10 / 21.  (8, 20) (conv3 M = 2560, conv2 5760, FC 160) runs under three split plans set
through IMPALA_WG3_TARGET / IMPALA_WG2_TARGET / IMPALA_FC_WG (read in impala_create; rows per
split are a multiple of 64):
  a: conv3 192 rows per split (fp32 6 chunks, bf16 3; last split 64), conv2 128 (4 / 2), FC 64
     (splits of 64, 64, 32 frames: 2, 2, 1 chunks / 1, 1, 1);
  b: conv3 128, conv2 192, FC 128 (128 + 32 frames: 4, 1 / 2, 1);
  c: conv3 64 and conv2 64 (fp32 2 chunks, bf16 1: shorter than the ring), FC one split of 160
     (5 / 3 chunks).

Check: the post-clip gradient of one step against the float64 oracle step on the same
parameters and synthetic batch (the harness of test_gpu_parity_full.py::_run): fp32 rel-L2
<= 1e-5 (GRAD_RL2); bf16 the one-step bounds of test_gpu_parity.py (metrics 5e-2 relative +
5e-3, gradient cosine > 0.99); and no NaN / Inf in any weight-gradient block.  fp32 also holds
each weight-gradient block on its own (BLOCK_RL2, reasoned where it is asserted).
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
GRAD_RL2 = 1e-5
BLOCK_RL2 = 1e-4
A = 15
NAMES = ("loss", "entropy", "td", "pg", "kl", "ratio", "grad_norm")
# canonical flat-parameter blocks (torch state_dict order, csrc/net.h canon())
_SIZES = (("w1", 32 * 192), ("b1", 32), ("w2", 64 * 512), ("b2", 64), ("w3", 64 * 576), ("b3", 64),
          ("lng", 1024), ("lnb", 1024), ("wfc", 256 * 1024), ("bfc", 256))
BLOCKS = {}
_o = 0
for _k, _n in _SIZES:
    BLOCKS[_k] = slice(_o, _o + _n)
    _o += _n

PLANS = {
    None: {},
    "a": {"IMPALA_WG3_TARGET": "126", "IMPALA_WG2_TARGET": "180", "IMPALA_FC_WG": "48"},
    "b": {"IMPALA_WG3_TARGET": "180", "IMPALA_WG2_TARGET": "120", "IMPALA_FC_WG": "32"},
    "c": {"IMPALA_WG3_TARGET": "360", "IMPALA_WG2_TARGET": "360", "IMPALA_FC_WG": "16"},
}
CASES = [pytest.param(1, 3, None, id="B1_T3"), pytest.param(2, 5, None, id="B2_T5"),
         pytest.param(3, 7, None, id="B3_T7"), pytest.param(8, 20, "a", id="B8_T20_a"),
         pytest.param(8, 20, "b", id="B8_T20_b"), pytest.param(8, 20, "c", id="B8_T20_c")]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_ORACLE = {}


def oracle(B, T):
    """(flat0, batch, float64 post-clip gradient, float64 metrics) of one step; computed once per
    shape and shared by the dtypes and split plans."""
    if (B, T) not in _ORACLE:
        batch = ref_cpu.synthetic_batch(B, T, A, seed=1234)
        flat0 = ref_cpu.flat_params(ref_cpu.make_model(0, A))
        _, g64, met64 = ref_cpu.train_step_fp64(flat0, batch, A)
        _ORACLE[(B, T)] = (flat0, batch, np.asarray(g64, np.float64), met64)
    return _ORACLE[(B, T)]


def _hip_step(B, T, dtype, plan, monkeypatch):
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    dev = _dev()
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    flat0, batch, _, _ = oracle(B, T)
    m = AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype)
    m.load_flat(flat0)
    e = Engine(m, batch_size=B, rollout_length=T)
    m._train_engine = e
    e.train_step(*[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in batch])
    torch.cuda.synchronize()
    g = m.flat_grad.cpu().numpy().astype(np.float64)
    met = e.metrics.cpu().numpy().astype(np.float64)
    e.close()
    return g, met


def _finite_blocks(g):
    for k in ("w2", "b2", "w3", "b3", "wfc", "bfc"):
        bad = int(np.sum(~np.isfinite(g[BLOCKS[k]])))
        assert bad == 0, (k, bad)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("B,T,plan", CASES)
def test_wgrad_edges_fp32(B, T, plan, monkeypatch):
    g, _ = _hip_step(B, T, "fp32", plan, monkeypatch)
    g64 = oracle(B, T)[2]
    _finite_blocks(g)
    per = {k: _rel_l2(g[BLOCKS[k]], g64[BLOCKS[k]]) for k in ("w2", "b2", "w3", "b3", "wfc", "bfc")}
    rl2 = _rel_l2(g, g64)
    print(f"fp32 B={B} T={T} plan={plan}: grad rel-L2 {rl2:.2e}; per block "
          + ", ".join(f"{k} {v:.1e}" for k, v in per.items()))
    assert rl2 <= GRAD_RL2, rl2
    # a 64-element bias block hides in the whole vector's norm, so each block is also held on
    # its own.  Bound 1e-4: an fp32 sum over M <= 5760 rows carries ~sqrt(M) * 2^-24 = 5e-6 of
    # its terms' magnitude, times the cancellation of a signed sum; a row or chunk dropped,
    # doubled or read from the wrong place moves a block by 1e-2 or more.
    for k, v in per.items():
        assert v <= BLOCK_RL2, (k, v)


@pytest.mark.parametrize("B,T,plan", CASES)
def test_wgrad_edges_bf16(B, T, plan, monkeypatch):
    g, met = _hip_step(B, T, "bf16", plan, monkeypatch)
    _, _, g64, met64 = oracle(B, T)
    _finite_blocks(g)
    exp = np.array([met64["train/" + k] for k in NAMES], np.float64)
    cos = float(np.dot(g, g64) / (np.linalg.norm(g) * np.linalg.norm(g64)))
    per = {}
    for k in ("w2", "w3", "wfc"):
        a, b = g[BLOCKS[k]], g64[BLOCKS[k]]
        per[k] = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    print(f"bf16 B={B} T={T} plan={plan}: grad cosine {cos:.5f}; per block "
          + ", ".join(f"{k} {v:.5f}" for k, v in per.items())
          + "; metrics max |d| / (5e-2 |x| + 5e-3) = "
          + f"{float(np.max(np.abs(met[:7] - exp) / (5e-2 * np.abs(exp) + 5e-3))):.2f}")
    assert np.all(np.abs(met[:7] - exp) <= 5e-2 * np.abs(exp) + 5e-3), (met[:7], exp)
    assert cos > 0.99, cos
