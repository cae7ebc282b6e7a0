"""The IMPALA ResNet actor path on the GPU (include/resnet_hip.h) against tests/resnet_oracle.py.

Shapes: n = 1 a lone frame; n = 3 fewer frames than workgroups, an odd count; n = 17 one full
16-row projection tile and a one-row tail; batch_size 17 throughout.  Stages are teacher-forced:
every exported tensor against the float64 stage on the kernel's own exported inputs, under
tests/stage_checks.py's bounds (fp32 |d| <= 1e-5 (|r| + rms r); bf16 |d| <= ulp(r) + the same;
the bf16 mode's fp32 heads under the fp32 bound).  End to end in fp32: 1e-4 rel + 1e-5 abs.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resnet_oracle as orc
from impala_amd import _lib
from oracle import ref_stages as rs

pytestmark = pytest.mark.gpu
BATCH = 17
CASES = [(d, n, A) for d in ("fp32", "bf16") for n, A in ((1, 15), (3, 2), (17, 6))]


@functools.lru_cache(maxsize=None)
def _inputs(A):
    """(model on the device, flat fp32 parameters, obs u8 [17,3,64,64]): the seed-0 init with every
    bias and the LayerNorm affine moved off 0 / 1, so that no stage can drop one and pass."""
    from impala_amd.resnet import ImpalaResNetModel, param_specs
    model = ImpalaResNetModel((3, 64, 64), A, "cuda", seed=0)
    flat = model.flat.cpu().numpy().copy()
    rng, off = np.random.default_rng(3), 0
    for _, s in param_specs(A):
        k = int(np.prod(s))
        if len(s) == 1:
            flat[off:off + k] += (0.05 * rng.standard_normal(k)).astype(np.float32)
        off += k
    model.flat.copy_(torch.from_numpy(flat))
    model.params_changed()
    obs = torch.from_numpy(rng.integers(0, 256, size=(BATCH, 3, 64, 64), dtype=np.uint8)).cuda()
    return model, flat, obs


@functools.lru_cache(maxsize=None)
def _run(dtype, n, A):
    from impala_amd.resnet import ResnetEngine
    model, flat, obs = _inputs(A)
    dbg = ResnetEngine(model, BATCH, dtype, debug=True)
    prod = ResnetEngine(model, BATCH, dtype)
    o = dict(fwd=[t.cpu().numpy() for t in dbg.forward(obs[:n])])
    o["t"] = {k: dbg.debug_tensor(k, n) for k in dbg.DEBUG_TENSORS}
    o["again"] = [t.cpu().numpy() for t in dbg.forward(obs[:n])]
    o["prod"] = [t.cpu().numpy() for t in prod.forward(obs[:n])]
    o["greedy"] = [t.cpu().numpy() for t in prod.act(obs[:n], True, seed=7, counter=3)]
    o["draw"] = [[t.cpu().numpy() for t in prod.act(obs[:n], False, seed=7, counter=3)] for _ in range(2)]
    return o


def _hold(name, got, ref, as_bf16, bad):
    g, r = np.asarray(got, np.float64).reshape(ref.shape), ref.numpy()
    w = rs.bf16_figures(g, r)[0] if as_bf16 else rs.f32_figures(g, r) / 1e-5
    print(f"{name:6s} worst |d| / bound {w:.3f}")
    if not w <= 1.0:
        bad.append(f"{name}: bound x{w:.3f}")


@pytest.mark.parametrize("dtype,n,A", CASES)
def test_stages_teacher_forced(dtype, n, A):
    _, flat, obs = _inputs(A)
    q = dtype == "bf16"
    P = orc.params(flat, A, quant=q)
    o = _run(dtype, n, A)
    # the body's tensors are exported channels-last, y in the kernel order p*32 + c
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in o["t"].items()}
    s = [t[f"s{i}"].permute(0, 3, 1, 2) for i in range(15)]
    bad = []
    x = obs[:n].cpu().to(torch.float64) / 255
    for st in range(3):
        i0 = 5 * st
        _hold(f"s{i0}", s[i0], orc.pooled(x, P, i0), q, bad)
        for b in (1, 3):
            _hold(f"s{i0 + b}", s[i0 + b], orc.res_t(s[i0 + b - 1], P, i0 + b), q, bad)
            _hold(f"s{i0 + b + 1}", s[i0 + b + 1], orc.res_x(s[i0 + b - 1], s[i0 + b], P, i0 + b + 1), q, bad)
        x = s[i0 + 4]
    y = t["y"].reshape(n, 64, 32).permute(0, 2, 1).reshape(n, 2048)
    _hold("y", y, orc.layer_norm(orc.features(x), P), q, bad)
    _hold("h", t["h"], orc.fc(y, P), q, bad)
    lg, v = orc.heads(t["h"], P)
    _hold("logits", t["heads"][:, :A], lg, False, bad)
    _hold("values", t["heads"][:, 15], v, False, bad)
    assert not bad, bad


@pytest.mark.parametrize("dtype,n,A", CASES)
def test_end_to_end(dtype, n, A):
    _, flat, obs = _inputs(A)
    o = _run(dtype, n, A)
    logits, values = o["fwd"]
    assert np.array_equal(logits, o["t"]["heads"][:, :A]) and np.array_equal(values[:, 0], o["t"]["heads"][:, 15])
    for k in ("again", "prod"):  # two calls, and the handle without the debug stores: the same bits
        assert np.array_equal(o[k][0], logits) and np.array_equal(o[k][1], values), k
    if dtype == "fp32":
        lg, v = orc.forward(orc.params(flat, A), obs[:n].cpu())
        for name, g, r in (("logits", logits, lg.numpy()), ("values", values[:, 0], v.numpy())):
            w = float(np.max(np.abs(g - r) / (1e-4 * np.abs(r) + 1e-5)))
            print(f"{name} worst |d| / (1e-4 |r| + 1e-5) {w:.3f}")
            assert w <= 1.0, name


@pytest.mark.parametrize("dtype,n,A", CASES)
def test_act(dtype, n, A):
    o = _run(dtype, n, A)
    a, logits, values = o["greedy"]
    assert np.array_equal(a[:, 0], np.argmax(logits, axis=1))  # (numpy: the first maximal index)
    (a0, l0, _), (a1, _, _) = o["draw"]
    assert a0.min() >= 0 and a0.max() < A and np.array_equal(a0, a1)
    for lg in (logits, l0):
        assert np.array_equal(lg, o["prod"][0])
    assert np.array_equal(values, o["prod"][1])


def test_refusals():
    model, _, obs = _inputs(6)
    L, sp = _lib.lib(), _lib.stream_ptr(None)
    from impala_amd.resnet import ResnetEngine, default_config
    e = ResnetEngine(model, BATCH)
    e._fresh()
    lg, v = torch.empty(BATCH, 6, device="cuda"), torch.empty(BATCH, device="cuda")
    fwd = lambda p, n: L.resnet_forward(e._h, p, n, _lib.ptr(lg), _lib.ptr(v), sp)  # noqa: E731
    assert fwd(_lib.ptr(obs), 0) == 1001 and fwd(_lib.ptr(obs), BATCH + 1) == 1001
    assert fwd(_lib.ptr(obs) + 1, 1) == 1001
    assert L.resnet_debug_read(e._h, 0, _lib.ptr(lg), 4, sp) == 1001
    cfg, h = default_config(), C.c_void_p()
    cfg.num_actions = 16
    assert L.resnet_create(C.byref(cfg), 0, C.byref(h)) == 1001 and not h
