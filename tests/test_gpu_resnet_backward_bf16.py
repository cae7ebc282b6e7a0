"""The IMPALA ResNet's bf16 training pair on the GPU (train_dtype = bf16), teacher-forced: every exported
gradient against float64 on the kernel's own exported operands (resnet_oracle's parameters with the bf16
operands rounded; a pooled convolution's gradient, which exists in LDS only, scattered by the exported
tap bytes and rounded as pool_gather rounds it).  Shapes as test_gpu_resnet_backward.py's, and n = 65 at
batch 65 for the weight gradients and the bits: with 64 frame groups the smallest n at which a workgroup
adds a second frame to live accumulators and resnet_wreduce_kernel sums 64 slabs.  Bounds: a bf16 tensor
per element ulp(r) + 1e-5 (|r| + rms r); gz, gy (fp32) 1e-5 (|r| + rms r); a parameter gradient rel-L2
max(BLOCK_RL2, 4 s), s the same contraction in torch float32 on the CPU; end to end rel-L2 to float64
autograd min(4 s_b, 0.7), s_b the oracle in torch.bfloat16 on the CPU (0 scores 1.0, a permutation 1.4).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_oracle as orc
from impala_amd import _lib
from oracle import ref_stages as rs
from stage_checks import BLOCK_RL2
from test_gpu_resnet import _inputs

pytestmark = pytest.mark.gpu
CASES = [(1, 15), (3, 2), (17, 6)]
WIDE = CASES + [(65, 6)]


@functools.lru_cache(maxsize=None)
def _case(n, A):
    """(obs u8 [n,3,64,64] on the device, dlogits [n,A], dvalues [n])."""
    base = _inputs(A)[2]
    obs = torch.cat([base.roll(5 * k, 3) for k in range(-(-n // base.shape[0]))])[:n].clone()
    blocks = torch.from_numpy(np.random.default_rng(11).integers(0, 256, size=(3, 8, 8), dtype=np.uint8))
    obs[0] = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2).cuda()
    g = torch.Generator().manual_seed(5)
    return obs, torch.randn(n, A, generator=g), torch.randn(n, generator=g)


def _canon(a):  # [n, 2048] in the kernel order p*32 + c -> c*64 + p
    return a.reshape(len(a), 64, 32).transpose(0, 2, 1).reshape(len(a), 2048)


def _unpool(g, taps):
    """The pool's backward: g, taps [n,HO,HO,C] -> [n,2HO,2HO,C], every element added at its window's tap."""
    n, HO, _, Cc = g.shape
    out = np.zeros((n, 2 * HO, 2 * HO, Cc))
    f, oy, ox, c = np.indices(g.shape)
    np.add.at(out, (f, 2 * oy + taps // 3 - 1, 2 * ox + taps % 3 - 1, c), g)
    return out


@functools.lru_cache(maxsize=None)
def _run(n, A):
    """The engine's outputs, and its exported tensors as float64 torch tensors, the body's NCHW."""
    from impala_amd.resnet import ResnetEngine
    model, B = _inputs(A)[0], max(n, 17)
    obs, dl, dv = _case(n, A)
    eng = ResnetEngine(model, B, "bf16", train=True)
    o = dict(fwd=[t.cpu().numpy() for t in ResnetEngine(model, B, "bf16").forward(obs)])
    o["train"] = [t.cpu().numpy() for t in eng.forward_train(obs)]
    o["grad"] = eng.backward(dl, dv).cpu().numpy()
    raw = {k: eng.debug_tensor(k, None if k == "part" else n).astype(np.float64 if k != "amax" else np.uint32)
           for k in {**eng.DEBUG_TENSORS, **eng.TRAIN_TENSORS}}
    eng.forward_train(obs)
    o["again"] = eng.backward(dl, dv).cpu().numpy()
    preset = torch.randn(model.flat.numel(), generator=torch.Generator().manual_seed(9))
    o["acc"] = eng.backward(dl, dv, out=preset.cuda(), accumulate=True).cpu().numpy()
    o["sum"] = (preset + torch.from_numpy(o["grad"])).numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    o.update({k: t(raw[k]) for k in ("h", "gy", "gz", "lnstat")}, dl=dl.double(), dv=dv.double(),
             x0=obs.cpu().double() / 255, y=t(_canon(raw["y"])), gyc=t(_canon(raw["gy"])),
             z=t(raw["part"].reshape(8, B, 256)[:, :n].sum(0)),
             s=[t(raw[f"s{i}"]).permute(0, 3, 1, 2) for i in range(15)],
             g=[t(raw[f"g{i}"]).permute(0, 3, 1, 2) for i in range(15)])
    am = raw["amax"].view(np.uint8).reshape(n, -1).astype(np.int64)
    for i, (lo, hi, HO, Cc) in zip((0, 5, 10), ((0, 16384, 32, 16), (16384, 24576, 16, 32), (24576, 26624, 8, 32))):
        # (the kernel's own operand: pool_gather rounds the sum of a pixel's windows to bf16 once)
        o[f"gu{i}"] = rs.rne_bf16(t(_unpool(raw[f"g{i}"], am[:, lo:hi].reshape(n, HO, HO, Cc)))).permute(0, 3, 1, 2)
    return o


def _hold(name, got, ref, as_bf16, bad):
    w = rs.bf16_figures(got.numpy(), ref.numpy())[0] if as_bf16 else rs.f32_figures(got.numpy(), ref.numpy()) / 1e-5
    print(f"{name:4s} worst |d| / bound {w:.3f}")
    if not w <= 1.0:
        bad.append(f"{name}: bound x{w:.3f}")


@pytest.mark.parametrize("n,A", CASES)
def test_data_gradients_teacher_forced(n, A):
    o, P, bad = _run(n, A), orc.params(_inputs(A)[1], A, quant=True), []
    s, g = o["s"], o["g"]
    W = lambda i: P[orc.CONV_KEYS[i] + ".weight"]  # noqa: E731
    dgrad = lambda gr, i: F.conv_transpose2d(gr, W(i), padding=1)  # noqa: E731
    z = (o["z"] + P["model.projection.1.bias"]).requires_grad_()
    lg, v = orc.heads(F.gelu(z), P)
    ((lg * o["dl"]).sum() + (v * o["dv"]).sum()).backward()
    _hold("gz", o["gz"], z.grad, False, bad)
    _hold("gy", o["gyc"], o["gz"] @ P["model.projection.1.weight"], False, bad)
    x, (mean, rstd) = s[14].flatten(1), o["lnstat"].T[:, :, None]
    gg, xh = o["gyc"] * P["model.projection.0.weight"], (F.relu(x) - mean) * rstd
    opened = (x > 0) * rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    _hold("g14", g[14], opened.reshape(g[14].shape), True, bad)
    for i0 in (10, 5, 0):
        for b in (3, 1):  # t = s[i0 + b], the block's input s[i0 + b - 1], its output s[i0 + b + 1]
            _hold(f"g{i0 + b}", g[i0 + b], (s[i0 + b] > 0) * dgrad(g[i0 + b + 1], i0 + b + 1), True, bad)
            _hold(f"g{i0 + b - 1}", g[i0 + b - 1], g[i0 + b + 1] + (s[i0 + b - 1] > 0) * dgrad(g[i0 + b], i0 + b), True, bad)
        if i0:
            _hold(f"g{i0 - 1}", g[i0 - 1], dgrad(o[f"gu{i0}"], i0), True, bad)
    assert not bad, bad


def _param_grads(o, dt):
    """The 38 parameter gradients as contractions of the kernel's own exported operands, in dtype dt."""
    c = lambda x: x.to(dt)  # noqa: E731
    out = {}
    for i, key in enumerate(orc.CONV_KEYS):
        x = o["x0"] if i == 0 else o["s"][i - 1] if i % 5 == 0 else F.relu(o["s"][i - 1])
        g = o[f"gu{i}"] if i % 5 == 0 else o["g"][i]
        out[key + ".weight"] = torch.nn.grad.conv2d_weight(c(x), (g.shape[1], x.shape[1], 3, 3), c(g), padding=1)
        out[key + ".bias"] = c(g).sum((0, 2, 3))
    mean, rstd = c(o["lnstat"]).T[:, :, None]
    xh = (F.relu(c(o["s"][14]).flatten(1)) - mean) * rstd
    gy, gz, h, dl, dv = (c(o[k]) for k in ("gyc", "gz", "h", "dl", "dv"))
    vals = [(gy * xh).sum(0), gy.sum(0), gz.T @ c(o["y"]), gz.sum(0), dl.T @ h, dl.sum(0), dv[None] @ h, dv.sum().reshape(1)]
    keys = ["model.projection.0", "model.projection.1", "model.actor", "model.critic"]
    out.update(zip([k + e for k in keys for e in (".weight", ".bias")], vals))
    return {k: v.double().numpy() for k, v in out.items()}


def _hold_flat(flat_grad, ref, bound, A):
    from impala_amd.resnet import param_specs
    off, bad = 0, []
    for k, shape in param_specs(A):
        size = int(np.prod(shape))
        d = rs.rel_l2(np.asarray(flat_grad[off:off + size], np.float64).reshape(shape), ref[k].reshape(shape))
        print(f"{k:44s} rel-L2 {d:.2e} = {d / bound[k]:.3f} of the bound {bound[k]:.1e}")
        if not d <= bound[k]:
            bad.append(f"{k}: {d:.2e} > {bound[k]:.1e}")
        off += size
    assert off == len(flat_grad) and not bad, bad


@pytest.mark.parametrize("n,A", WIDE)
def test_parameter_gradients_teacher_forced(n, A):
    o = _run(n, A)
    ref, f32 = _param_grads(o, torch.float64), _param_grads(o, torch.float32)
    _hold_flat(o["grad"], ref, {k: max(BLOCK_RL2, 4 * rs.rel_l2(f32[k], ref[k])) for k in ref}, A)


def _autograd(A, obs, dl, dv, dt):
    P = {k: v.to(dt).requires_grad_() for k, v in orc.params(_inputs(A)[1], A).items()}
    x = obs.cpu().to(dt) / 255
    for st in range(3):
        x = orc.pooled(x, P, 5 * st)
        for b in (1, 3):
            x = orc.res_x(x, orc.res_t(x, P, 5 * st + b), P, 5 * st + b + 1)
    lg, v = orc.heads(orc.fc(orc.layer_norm(orc.features(x), P), P), P)
    ((lg * dl.to(dt)).sum() + (v * dv.to(dt)).sum()).backward()
    return {k: p.grad.double().numpy() for k, p in P.items()}


@pytest.mark.parametrize("n,A", CASES)
def test_end_to_end_against_float64(n, A):
    ref, low = (_autograd(A, *_case(n, A), dt) for dt in (torch.float64, torch.bfloat16))
    _hold_flat(_run(n, A)["grad"], ref, {k: min(4 * rs.rel_l2(low[k], ref[k]), 0.7) for k in ref}, A)


@pytest.mark.parametrize("n,A", WIDE)
def test_bits(n, A):
    o = _run(n, A)
    assert np.array_equal(o["train"][0], o["fwd"][0]) and np.array_equal(o["train"][1], o["fwd"][1])
    assert np.array_equal(o["grad"], o["again"])
    assert np.array_equal(o["acc"], o["sum"])


def test_public_interface():
    from impala_amd.resnet import ImpalaResNetModel
    A = 6
    model = ImpalaResNetModel((3, 64, 64), A, "cuda", seed=0, train_batch=17, train_dtype="bf16")
    model.flat.copy_(_inputs(A)[0].flat)
    model.params_changed()
    obs, dl, dv = _case(17, A)
    dl, dv = dl.cuda(), dv.cuda()

    def step():
        logits, values = model.forward_train(obs)
        ((logits * dl).sum() + (values[:, 0] * dv).sum()).backward()
        return torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    model.flat_grad.zero_()
    g1 = step()
    assert np.array_equal(g1, _run(17, A)["grad"]) and np.array_equal(g1, model.flat_grad.cpu().numpy())
    assert np.array_equal(step(), g1 + g1)


def test_refusals():
    from impala_amd.resnet import ResnetEngine, default_config
    model = _inputs(6)[0]
    obs, dl, dv = _case(3, 6)
    L, sp = _lib.lib(), _lib.stream_ptr(None)
    dl, dv, g = dl.cuda(), dv.cuda(), torch.zeros(model.flat.numel(), device="cuda")
    e = ResnetEngine(model, 17, "bf16", train=True)
    e.forward_train(obs)
    assert L.resnet_backward(e._h, _lib.ptr(obs), 2, _lib.ptr(dl), _lib.ptr(dv), _lib.ptr(g), 0, sp) == 1001  # another n
    torch.cuda.synchronize()
    assert not g.any()  # nothing was launched
    for dtype, train_dtype in ((1, 0), (0, 1)):
        cfg, h = default_config(), C.c_void_p()
        cfg.train, cfg.dtype, cfg.train_dtype = 1, dtype, train_dtype
        assert L.resnet_create(C.byref(cfg), 0, C.byref(h)) == 1001 and not h
