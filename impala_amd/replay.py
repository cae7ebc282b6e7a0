"""Rollout storage feeding the learner.

Reference: ``agents/impala/builder.py:30-36`` builds ``ReplayBuffer(CircularBuffer(1000),
UniformSampler())``; actors ``async_append`` one trajectory ``[s, a, r, discount, logits]``
(``agents/impala/learning.py:71-80``); the learner calls ``warm_up(learning_starts)`` and
``sample(batch_size) -> (keys, batch, probs)`` (``learning.py:116-121``).

Two implementations with that interface:

* ``ReplayBuffer``        host memory, returns the reference's list-of-trajectories batch; the
  batch also carries the rows' host addresses, so the learner stages them with
  ``impala_stage_rows`` (the library's thread pool collates them into a page-locked slot).
* ``DeviceReplayBuffer``  MI355X-first: the circular store lives in HBM (1000 x 247 KB =
  247 MB of 288 GB); an appended trajectory is written into a pinned-host staging ring and
  copied to its HBM slot with an async H2D on a side stream, so each trajectory crosses PCIe
  once however often it is replayed; ``sample`` gathers B slots on the device with the HIP
  gather kernel and returns the collated ``(B,T,...)`` batch already resident in HBM.

``DeviceTransitionBuffer`` is PPO's counterpart (flat transitions, four arrays): the actor's
rollout becomes transitions on the device (``impala_ppo_extend_rollout``) and the step reads
the sampled slots in place.
"""
from __future__ import annotations

import threading
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


def _row_info(item):
    """(host addresses, (dtypes, byte sizes)) of a trajectory's fields when every field is a
    contiguous CPU tensor, else None: what impala_stage_rows needs to read the rows in place."""
    if not all(isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.is_contiguous()
               for t in item):
        return None
    return ([t.data_ptr() for t in item],
            (tuple(t.dtype for t in item), tuple(t.numel() * t.element_size() for t in item)))


class RowBatch(list):
    """The list of B trajectories a replay's ``sample`` returns (the reference's batch format),
    plus, when every sampled trajectory's fields are contiguous host tensors of one layout,
    ``row_ptrs`` -- per field the B rows' host addresses (numpy uint64) -- and ``row_key`` --
    the fields' (dtypes, byte sizes) -- for ``impala_stage_rows``.  The rows are the replay's
    own tensors: an append replaces a slot's list and never writes into a stored tensor, so a
    consumer that keeps the batch keeps its rows."""
    row_ptrs = None
    row_key = None


class ReplayBuffer:
    """CircularBuffer + UniformSampler semantics on the host (reference-compatible)."""

    def __init__(self, capacity: int = 1000, seed: Optional[int] = None):
        self.capacity = int(capacity)
        self._data: List[Optional[list]] = [None] * self.capacity
        # per slot: the fields' host addresses and layout key (_row_info), when known
        self._ptr_tab = np.zeros((self.capacity, 5), dtype=np.uint64)
        self._row_keys: List[Optional[tuple]] = [None] * self.capacity
        self._keys = np.zeros(self.capacity, dtype=np.int64)
        self._next_key = 0
        self._size = 0
        self._cursor = 0
        self._rng = np.random.default_rng(seed)
        self._cv = threading.Condition()

    def __len__(self):
        return self._size

    def reset(self, seed: Optional[int] = None):
        self._rng = np.random.default_rng(seed)

    def append(self, item: Sequence[torch.Tensor]) -> int:
        with self._cv:
            slot = self._cursor
            self._data[slot] = list(item)
            info = _row_info(self._data[slot]) if len(item) == 5 else None
            if info is None:
                self._row_keys[slot] = None
            else:
                self._ptr_tab[slot] = info[0]
                self._row_keys[slot] = info[1]
            key = self._next_key
            self._keys[slot] = key
            self._next_key += 1
            self._cursor = (self._cursor + 1) % self.capacity
            self._size = min(self._size + 1, self.capacity)
            self._cv.notify_all()
            return key

    def extend(self, items) -> List[int]:
        return [self.append(x) for x in items]

    async def async_append(self, item):
        return self.append(item)

    def warm_up(self, learning_starts: Optional[int] = None, timeout: float = 240.0) -> None:
        """Block until ``learning_starts`` items are stored (rlmeta ReplayBuffer.warm_up)."""
        if not learning_starts:
            return
        need = min(int(learning_starts), self.capacity)
        deadline = time.monotonic() + timeout
        with self._cv:
            while self._size < need:
                left = deadline - time.monotonic()
                if left <= 0:
                    raise TimeoutError(f"replay warm_up: {self._size}/{need} after {timeout}s")
                self._cv.wait(left)

    def _indices(self, batch_size: int) -> np.ndarray:
        if self._size == 0:
            raise RuntimeError("sample from an empty replay buffer")
        replace = batch_size > self._size
        return self._rng.choice(self._size, size=batch_size, replace=replace)

    def sample(self, batch_size: int):
        with self._cv:
            idx = self._indices(batch_size)
            batch = RowBatch(self._data[i] for i in idx)
            rk = {self._row_keys[i] for i in idx}
            if len(rk) == 1 and None not in rk:
                batch.row_key = rk.pop()
                batch.row_ptrs = tuple(np.ascontiguousarray(self._ptr_tab[idx, f]) for f in range(5))
            keys = self._keys[idx].copy()
        probs = np.full(batch_size, 1.0 / self._size)
        return keys, batch, probs


class RowSample:
    """DeviceReplayBuffer.sample_rows: the sampled slots (host int64), read in place."""
    __slots__ = ("replay", "idx")

    def __init__(self, replay, idx):
        self.replay, self.idx = replay, np.ascontiguousarray(idx, dtype=np.int64)

    def gather(self, stream=None):
        """The rows collated on the device (what ``sample`` returns), for a caller that cannot
        read them in place."""
        from impala_amd.engine import gather_rollouts
        return self.replay.read_rows(self, lambda fields, idx, st: gather_rollouts(fields, idx, st),
                                     stream)


class DeviceReplayBuffer(ReplayBuffer):
    """HBM-resident circular rollout store with pinned-host staging (see module doc)."""

    def __init__(self, capacity: int = 1000, rollout_length: int = 20, num_actions: int = 15,
                 device="cuda", seed: Optional[int] = None, staging_slots: int = 64):
        super().__init__(capacity, seed)
        self.device = torch.device(device)
        C, T, A = self.capacity, int(rollout_length), int(num_actions)
        self.T, self.A = T, A
        d = self.device
        self.obs = torch.empty(C, T, 3, 64, 64, dtype=torch.uint8, device=d)
        self.act = torch.zeros(C, T, dtype=torch.int64, device=d)
        self.rew = torch.zeros(C, T, dtype=torch.float32, device=d)
        self.disc = torch.zeros(C, T, dtype=torch.float32, device=d)
        self.mu = torch.zeros(C, T, A, dtype=torch.float32, device=d)
        S = int(staging_slots)
        pin = torch.cuda.is_available()
        self._st_obs = torch.empty(S, T, 3, 64, 64, dtype=torch.uint8, pin_memory=pin)
        self._st_small = torch.empty(S, T, 3 + A, dtype=torch.float32, pin_memory=pin)
        self._st_act = torch.empty(S, T, dtype=torch.int64, pin_memory=pin)
        self._st_events = [None] * S
        self._st_next = 0
        self._stream = torch.cuda.Stream(device=d)
        self._pending: List[torch.cuda.Event] = []
        # An append must not overwrite a slot that a queued gather still reads.  sample() numbers
        # its gathers (_gen) and marks the slots each one reads (_slot_gen); an append into a
        # slot read by a gather not yet fenced records ONE event on the gathers' stream (it
        # follows every gather enqueued so far) and its copy waits for it; later appends into
        # slots read before that fence wait for the same event.  So the learner's stream gets
        # at most one event per sample, and none while nothing is appended.
        self._read_stream = None
        self._gen = 0
        self._slot_gen = np.zeros(self.capacity, dtype=np.int64)
        self._fence_gen = 0
        self._fence_ev: Optional[torch.cuda.Event] = None

    def append(self, item: Sequence[torch.Tensor]) -> int:
        s, a, r, g, mu = item
        T = self.T
        with self._cv:
            j = self._st_next
            self._st_next = (j + 1) % len(self._st_events)
            ev = self._st_events[j]
            if ev is not None:
                ev.synchronize()  # staging slot reuse: its previous H2D has finished
            self._st_obs[j].copy_(s.reshape(T, 3, 64, 64))
            self._st_act[j].copy_(a.reshape(T))
            sm = self._st_small[j]
            sm[:, 0].copy_(r.reshape(T))
            sm[:, 1].copy_(g.reshape(T))
            sm[:, 3:].copy_(mu.reshape(T, self.A))
            slot = self._cursor
            with torch.cuda.stream(self._stream):
                read_gen = int(self._slot_gen[slot])
                if read_gen > self._fence_gen:  # read by a gather not yet fenced
                    fence = torch.cuda.Event()
                    fence.record(self._read_stream)
                    self._fence_ev, self._fence_gen = fence, self._gen
                if read_gen > 0:
                    self._stream.wait_event(self._fence_ev)
                self.obs[slot].copy_(self._st_obs[j], non_blocking=True)
                self.act[slot].copy_(self._st_act[j], non_blocking=True)
                small = sm.to(self.device, non_blocking=True)
                self.rew[slot].copy_(small[:, 0])
                self.disc[slot].copy_(small[:, 1])
                self.mu[slot].copy_(small[:, 3:])
                ev = torch.cuda.Event()
                ev.record(self._stream)
            self._st_events[j] = ev
            self._pending.append(ev)
            key = self._next_key
            self._keys[slot] = key
            self._next_key += 1
            self._cursor = (slot + 1) % self.capacity
            self._size = min(self._size + 1, self.capacity)
            self._cv.notify_all()
            return key

    def sample_rows(self, batch_size: int):
        """-> (keys, RowSample, probs): the same draw as ``sample`` (the same generator call),
        without a gather -- the step reads the sampled slots in place
        (``read_rows`` / Engine.train_step_rows).  A slot overwritten between this call and
        the step is read with its new trajectory (the draw is of slots)."""
        with self._cv:
            idx = self._indices(batch_size)
            keys = self._keys[idx].copy()
            size = self._size
        return keys, RowSample(self, idx), np.full(batch_size, 1.0 / size)

    @property
    def fields(self):
        """The ring's five arrays (obs, actions, rewards, discounts, behaviour logits)."""
        return (self.obs, self.act, self.rew, self.disc, self.mu)

    def read_rows(self, rs: "RowSample", enqueue, stream=None):
        """Run ``enqueue(fields, idx, stream)`` -- which enqueues work reading the ring slots
        ``rs.idx`` on ``stream`` (the current stream when None) -- under the lock ``append``
        takes, after that stream waits for every staged append; then mark the slots as read by
        it (the fence an append into them waits for, as for a gather in ``sample``)."""
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        with self._cv:
            if self._pending:
                pending, self._pending = self._pending, []
                for ev in pending:
                    cur.wait_event(ev)
            out = enqueue(self.fields, rs.idx, cur)
            self._read_stream = cur
            self._gen += 1
            self._slot_gen[rs.idx] = self._gen
        return out

    def sample(self, batch_size: int, stream=None):
        """-> (keys, (obs, act, rew, disc, mu) collated on the device, probs).

        The sampled slot indices travel in the gather launch's own arguments
        (impala_gather_rows_hidx), so the learner's stream gets the gather and nothing else: no
        index upload, no event, and nothing here ever waits on the device.  The lock is held
        from picking the slots until the gather is enqueued and its slots marked with its
        generation: an append either lands before -- its H2D event is among the ``pending``
        the gather waits for -- or after, and then its copy waits for a fence event recorded
        behind this gather (see ``__init__``).  No append can slip between the two and
        overwrite a slot the gather is reading."""
        from impala_amd.engine import gather_rollouts
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        with self._cv:
            idx = self._indices(batch_size)
            keys = self._keys[idx].copy()
            pending, self._pending = self._pending, []
            for ev in pending:  # the learner's stream waits for every staged H2D
                cur.wait_event(ev)
            batch = gather_rollouts((self.obs, self.act, self.rew, self.disc, self.mu), idx,
                                    stream)
            self._read_stream = cur
            self._gen += 1
            self._slot_gen[idx] = self._gen
            size = self._size
        probs = np.full(batch_size, 1.0 / size)
        return keys, batch, probs


class DeviceTransitionBuffer(ReplayBuffer):
    """PPO's transition replay in HBM (``agents/ppo/builder.py:30-36``: CircularBuffer(size,
    collate_fn=torch.cat) + UniformSampler, flat transitions ``[s, a, target, pi_ref]``).

    It owns the ring's four device arrays -- obs u8 [C,3,64,64], actions i64 [C], value targets
    f32 [C], behaviour logits f32 [C,A] -- and keeps the base class's cursor, size, keys and
    generator, so for one seed and one number of stored items it draws exactly the slots the
    host ``ReplayBuffer`` draws.

    * ``extend_rollout``  the native ingest (``impala_ppo_extend_rollout``): one rollout of L
      steps becomes K = L - 1 transitions, the lambda-return targets computed on the device.
    * ``extend`` / ``append``  ready-made transition items from foreign actors, collated and
      copied with torch (not a hot path).
    * ``sample_rows``  the draw alone; the step reads the slots in place
      (``Engine.ppo_train_step_rows``).  ``sample`` gathers them on the device.

    It serves ONE host thread and ONE stream at a time, as the native DQN replay does: ingest,
    gathers and in-place steps are all enqueued on the caller's current stream, which alone
    orders a step after the ingests before it and an overwrite after the steps that read the
    slot.  Nothing here waits on the device except the reuse of the pinned staging buffer."""

    def __init__(self, capacity: int = 20000, num_actions: int = 15, device="cuda",
                 seed: Optional[int] = None):
        super().__init__(capacity, seed)
        self._data = []  # (the base class's host rows: unused, the ring lives in HBM)
        self.device = torch.device(device)
        C, A = self.capacity, int(num_actions)
        self.A = A
        d = self.device
        self.obs = torch.empty(C, 3, 64, 64, dtype=torch.uint8, device=d)
        self.act = torch.zeros(C, dtype=torch.int64, device=d)
        self.tgt = torch.zeros(C, dtype=torch.float32, device=d)
        self.mu = torch.zeros(C, A, dtype=torch.float32, device=d)
        self._ring = None       # the library's impala_ppo_ring of the four arrays
        self._st_host = None    # pinned staging bytes of one rollout, and their device copy
        self._st_dev = None
        self._st_event = None   # the last H2D out of _st_host

    @property
    def fields(self):
        """The ring's four arrays (obs, actions, value targets, behaviour logits)."""
        return (self.obs, self.act, self.tgt, self.mu)

    def _advance(self, n: int) -> List[int]:
        """Book n rows appended at the cursor (under the lock): their keys."""
        slots = (self._cursor + np.arange(n)) % self.capacity
        keys = np.arange(self._next_key, self._next_key + n, dtype=np.int64)
        self._keys[slots] = keys
        self._next_key += n
        self._cursor = int((self._cursor + n) % self.capacity)
        self._size = min(self._size + n, self.capacity)
        self._cv.notify_all()
        return keys.tolist()

    # byte layout of one staged rollout: obs | actions | rewards | values | logits | done
    def _stage_views(self, buf, L):
        A, o = self.A, 0
        out = []
        for n, dt in ((L * 12288, torch.uint8), (L * 8, torch.int64), (L * 4, torch.float32),
                      (L * 4, torch.float32), (L * A * 4, torch.float32), (L, torch.uint8)):
            out.append(buf[o:o + n].view(dt))
            o += n
        return out, o

    def extend_rollout(self, obs, actions, rewards, done, logits, values, gamma: float = 0.99,
                       lambda_: float = 0.95) -> List[int]:
        """One rollout of L steps -- obs u8 [L,3,64,64], actions [L], rewards [L], done [L],
        logits [L,A], values [L] (trailing unit dims allowed) -> K = L - 1 transitions appended
        at the cursor with the lambda-return targets of include/impala_hip.h
        (impala_ppo_extend_rollout); returns their keys.  Host tensors are staged through one
        pinned buffer and one H2D copy; device tensors are read where they are."""
        from impala_amd import _lib
        L = int(obs.shape[0])
        A = self.A
        fs = [torch.as_tensor(x) for x in (obs, actions, rewards, values, logits, done)]
        dts = (torch.uint8, torch.int64, torch.float32, torch.float32, torch.float32, torch.uint8)
        shapes = ((L, 3, 64, 64), (L,), (L,), (L,), (L, A), (L,))
        fs = [f.reshape(s) for f, s in zip(fs, shapes)]
        with self._cv:
            if all(f.device == self.device for f in fs):
                dev = [f.to(dt).contiguous() for f, dt in zip(fs, dts)]
            else:
                nbytes = L * (12288 + 8 + 4 + 4 + 4 * A + 1)
                if self._st_host is None or self._st_host.numel() < nbytes:
                    self._st_host = torch.empty(nbytes, dtype=torch.uint8,
                                                pin_memory=torch.cuda.is_available())
                    self._st_dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                elif self._st_event is not None:
                    self._st_event.synchronize()  # the previous H2D has left the pinned buffer
                host, _ = self._stage_views(self._st_host, L)
                for h, f, s in zip(host, fs, shapes):
                    h.view(s).copy_(f)  # (casts to the staged dtype)
                self._st_dev[:nbytes].copy_(self._st_host[:nbytes], non_blocking=True)
                self._st_event = torch.cuda.Event()
                self._st_event.record(torch.cuda.current_stream(self.device))
                dev, _ = self._stage_views(self._st_dev, L)
            if self._ring is None:
                self._ring = _lib.ImpalaPpoRing(*[_lib.ptr(t) for t in self.fields],
                                                self.capacity, A)
            o, a, r, v, mu, d = dev
            _lib.check(_lib.lib().impala_ppo_extend_rollout(
                self._ring, self._cursor, _lib.ptr(o), _lib.ptr(a), _lib.ptr(r), _lib.ptr(d),
                _lib.ptr(mu), _lib.ptr(v), L, float(gamma), float(lambda_),
                _lib.stream_ptr(None)), "impala_ppo_extend_rollout")
            return self._advance(L - 1)

    def extend(self, items) -> List[int]:
        """Ready-made transition items ``[s, a, target, pi_ref]`` (or one collated 4-tuple)."""
        from impala_amd.ppo import collate_transitions
        s, a, t, mu = collate_transitions(items, self.device)
        keys: List[int] = []
        with self._cv:
            for i0 in range(0, s.shape[0], self.capacity):
                n = min(self.capacity, s.shape[0] - i0)
                first = min(n, self.capacity - self._cursor)
                for dst, src in zip(self.fields, (s, a, t, mu.reshape(-1, self.A))):
                    dst[self._cursor:self._cursor + first].copy_(src[i0:i0 + first])
                    if first < n:
                        dst[:n - first].copy_(src[i0 + first:i0 + n])
                keys += self._advance(n)
        return keys

    def append(self, item) -> int:
        return self.extend([item])[0]

    def sample_rows(self, batch_size: int):
        """-> (keys, RowSample, probs): the host generator's draw (the same call the host
        ``ReplayBuffer.sample`` makes), without a gather.  A slot overwritten between this call
        and the step is read with its new transition (the draw is of slots; the stream orders
        the overwrite before the step)."""
        with self._cv:
            idx = self._indices(batch_size)
            keys = self._keys[idx].copy()
            size = self._size
        return keys, RowSample(self, idx), np.full(batch_size, 1.0 / size)

    def read_rows(self, rs: "RowSample", enqueue, stream=None):
        """``enqueue(fields, idx, stream)`` on the caller's stream (see the class note)."""
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        return enqueue(self.fields, rs.idx, cur)

    def sample(self, batch_size: int, stream=None):
        """-> (keys, (obs, actions, targets, logits) gathered on the device, probs)."""
        keys, rs, probs = self.sample_rows(batch_size)
        return keys, rs.gather(stream), probs
