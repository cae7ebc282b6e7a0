"""The four owners of a native handle (_lib.NativeHandle: Engine, SACEngine, DqnEngine,
NativePrioritizedReplay) share one lifetime: a cheap call works, ``close()`` is idempotent and
leaves ``_h`` None, the same call is then refused by the library's own null-handle check (status
1001 -> RuntimeError; tests/test_dqn_host.py pins that status on the CPU), and dropping the
owner afterwards is silent."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine(dev):
    from impala_amd.engine import Engine
    from impala_amd.model import AtariPPOModel
    e = Engine(AtariPPOModel(device=dev, seed=0), batch_size=1, rollout_length=2)
    obs = torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=dev)
    return e, lambda: e.forward(obs)[0]


def _dqn_engine(dev):
    from impala_amd.dqn import AtariDQNModel, DqnEngine
    e = DqnEngine(AtariDQNModel(device=dev, seed=0), batch_size=1)
    obs = torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=dev)
    return e, lambda: e.forward(obs)


def _sac_engine(dev):
    from impala_amd.sac import SACEngine, SoftActor
    torch.manual_seed(0)
    e = SACEngine.inference(SoftActor((17,), (6,), device=dev), 128)  # what SoftActor.act builds
    x = torch.zeros(4, 17, device=dev)
    return e, lambda: e.act(x, None, 0.0, 1.0, 0.0)


def _native_replay(dev):
    from impala_amd.dqn import NativePrioritizedReplay
    rb = NativePrioritizedReplay(capacity=8, device=dev, seed=0)
    rb.extend((torch.zeros(1, 3, 64, 64, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
               torch.ones(1)))
    return rb, lambda: rb.sample(1)[0]


@pytest.mark.parametrize("make", [_engine, _dqn_engine, _sac_engine, _native_replay],
                         ids=lambda f: f.__name__.strip("_"))
def test_handle_lifetime(make):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    owner, call = make(torch.device("cuda:0"))
    assert owner._h
    out = call()
    torch.cuda.synchronize()
    assert out.numel() and (out.dtype == torch.int64 or bool(torch.isfinite(out).all()))
    owner.close()
    owner.close()
    assert owner._h is None
    with pytest.raises(RuntimeError, match=r"status 1001"):
        call()
    del call, owner
    gc.collect()
