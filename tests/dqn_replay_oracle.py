"""numpy float64 restatement of the dqn_replay contract (include/dqn_hip.h): the counter-based
draw, prefix-sum sampling, and the actor's n-step targets -- the latter both as the header's nested
form and as a transcription of rlax's ``n_step_bootstrapped_returns`` loop (lambda = 1).  Beside
the contract, which sums with np.cumsum, stands a restatement of the kernels' own summation order
(csrc/dqn_replay.hip: block sums, the two-level scan, the prefix inside a block) and
``prefix_discrepancy``, which measures how far the two orders and an 80-bit prefix lie apart: the
distance from a prefix boundary inside which the order may decide a key."""
import numpy as np

M64 = (1 << 64) - 1


def mix(z: int) -> int:
    """The header's mix(z) on Python ints, mod 2^64."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniforms(seed: int, counter: int, n: int) -> np.ndarray:
    """u_j = (mix(mix(seed ^ mix(counter)) + j) >> 11) * 2^-53, j < n."""
    base = mix((seed & M64) ^ mix(counter & M64))
    return np.array([(mix((base + j) & M64) >> 11) * 2.0 ** -53 for j in range(n)], dtype=np.float64)


def weights(priorities, alpha: float) -> np.ndarray:
    return np.power(np.asarray(priorities, dtype=np.float32).astype(np.float64), np.float64(alpha))


def sample(w, size: int, seed: int, counter: int, n: int):
    """-> (keys [n] i64, probabilities [n] f32, margin): the contract on weights w[0..size).
    margin is min_j |u_j * total - nearest prefix boundary| / total (inf when the total is 0): the
    distance of the inputs from the cases where summation order decides the key."""
    w = np.asarray(w, dtype=np.float64)[:size]
    u = uniforms(seed, counter, n)
    C = np.cumsum(w)
    total = C[-1]
    if not total > 0:
        keys = np.minimum(np.floor(u * size).astype(np.int64), size - 1)
        return keys, np.full(n, 1.0 / size, dtype=np.float64).astype(np.float32), np.inf
    x = u * total
    keys = np.minimum(np.searchsorted(C, x, side="right"), size - 1).astype(np.int64)
    edges = np.concatenate([[0.0], C])
    margin = float(np.min(np.abs(x[:, None] - edges[None, :]))) / total if n * size <= 4_000_000 else \
        float(min(np.min(np.abs(xi - edges)) for xi in x)) / total
    return keys, (w[keys] / total).astype(np.float32), margin


# ---------------------------------------------------------------- the kernels' summation order
BLOCK = 512          # DQN_REPLAY_BLOCK: 64 lanes x 8 consecutive rows
SCAN_THREADS = 256   # dqn_replay_host::kScanThreads


def scan_chunk(nb: int) -> int:
    """dqn_replay_host::scan_chunk: block sums per scan thread, ceil(sqrt(nb)) unless 256 threads
    of that many would not cover nb."""
    c = max(1, int(np.ceil(np.sqrt(np.float64(nb)))))
    while c * SCAN_THREADS < nb:
        c += 1
    return c


def _lanes(w, size: int) -> np.ndarray:
    """[nb, 64, 8]: the weights as the lanes load them, rows >= size as 0."""
    w = np.asarray(w, dtype=np.float64)[:size]
    nb = (size + BLOCK - 1) // BLOCK
    x = np.zeros(nb * BLOCK, dtype=np.float64)
    x[:size] = w
    return x.reshape(nb, 64, 8)


def block_sums(w, size: int) -> np.ndarray:
    """replay_block_sum_kernel: each lane's 8 weights added in order, then the 64 lane sums
    through the fixed pairwise tree lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32."""
    x = _lanes(w, size)
    s = x[:, :, 0].copy()
    for k in range(1, 8):
        s = s + x[:, :, k]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def block_prefix(bsum, defect=None):
    """replay_draw_kernel's two-level scan -> (P [nb] inclusive prefix, total).  Scan thread t adds
    its `chunk` consecutive block sums in order; the threads' totals are walked in order into
    exclusive offsets; P = offset + local.  A thread whose first block is past nb holds 0.0, so
    the walk's end over all SCAN_THREADS totals is P[nb - 1] bit for bit: that end is `total`.

    defect (for the tests that show the inputs would notice one; None is the kernel):
      ("drop_offset", t)  scan thread t's offset is left at 0
      ("stale_tail",)     a thread whose first block is past nb holds its predecessor's total"""
    bsum = np.asarray(bsum, dtype=np.float64)
    nb = len(bsum)
    chunk = scan_chunk(nb)
    T = (nb + chunk - 1) // chunk
    local = np.empty(nb, dtype=np.float64)
    tot = np.zeros(SCAN_THREADS, dtype=np.float64)
    for t in range(T):
        seg = np.cumsum(bsum[t * chunk:min(nb, (t + 1) * chunk)])  # (sequential, in order)
        local[t * chunk:t * chunk + len(seg)] = seg
        tot[t] = seg[-1]
    if defect and defect[0] == "stale_tail":
        tot[T:] = tot[T - 1]
    off = np.zeros(SCAN_THREADS, dtype=np.float64)
    run = np.float64(0.0)
    for t in range(SCAN_THREADS):
        off[t] = run
        run = run + tot[t]
    if defect and defect[0] == "drop_offset":
        off[defect[1]] = 0.0
    P = np.repeat(off[:T], chunk)[:nb] + local
    total = float(run)
    if defect is None:
        assert total == P[-1]
    return P, total


def row_prefix(w, size: int) -> np.ndarray:
    """[nb, 64, 8]: E + q, the draw kernel's inclusive prefix inside each block -- q the in-lane
    running sums, E the lane-sequential exclusive scan of the lanes' totals."""
    q = np.cumsum(_lanes(w, size), axis=2)
    E = np.zeros(q.shape[:2], dtype=np.float64)
    E[:, 1:] = np.cumsum(q[:, :-1, 7], axis=1)
    return E[:, :, None] + q


def kernel_prefix(w, size: int) -> np.ndarray:
    """[size]: the inclusive prefix over rows in the kernels' order: the exclusive block prefix
    plus the prefix inside the block."""
    P, _ = block_prefix(block_sums(w, size))
    excl = np.concatenate([[0.0], P[:-1]])
    return (excl[:, None, None] + row_prefix(w, size)).reshape(-1)[:size]


def prefix_discrepancy(w, size: int) -> float:
    """The largest of |kernel-order prefix - P| and |np.cumsum float64 prefix - P| over all rows,
    divided by the total; P is np.cumsum in np.longdouble (80-bit on x86)."""
    w = np.asarray(w, dtype=np.float64)[:size]
    P = np.cumsum(w.astype(np.longdouble))
    if not P[-1] > 0:
        return 0.0
    dk = np.max(np.abs(kernel_prefix(w, size).astype(np.longdouble) - P))
    dc = np.max(np.abs(np.cumsum(w).astype(np.longdouble) - P))
    return float(max(dk, dc) / P[-1])


def _lower_bound(P, x, ge: bool) -> int:
    """replay_lower_bound, step for step (P need not be sorted when a defect is modelled)."""
    lo, hi = 0, len(P)
    while lo < hi:
        mid = (lo + hi) >> 1
        if (P[mid] >= x) if ge else (P[mid] > x):
            hi = mid
        else:
            lo = mid + 1
    return lo


def sample_kernel_order(w, size: int, seed: int, counter: int, n: int, defect=None) -> np.ndarray:
    """-> keys [n]: replay_draw_kernel restated step by step on the kernels' own sums -- the block
    search on P, the residual against the block's E + q, the two fall-backs.  `defect` as in
    block_prefix."""
    w = np.asarray(w, dtype=np.float64)[:size]
    x = _lanes(w, size)
    P, total = block_prefix(block_sums(w, size), defect)
    nb = len(P)
    u = uniforms(seed, counter, n)
    if not total > 0:
        return np.minimum((u * np.float64(size)).astype(np.int64), size - 1)
    inner = row_prefix(w, size).reshape(nb, BLOCK)
    pos = x.reshape(nb, BLOCK) > 0
    keys = np.empty(n, dtype=np.int64)
    for j in range(n):
        target = u[j] * total
        blk = _lower_bound(P, target, False)
        hit = np.zeros(0, dtype=np.int64)
        if blk == nb:
            blk = min(_lower_bound(P, total, True), nb - 1)
        else:
            r = target - (P[blk - 1] if blk > 0 else 0.0)
            hit = np.flatnonzero(pos[blk] & (inner[blk] > r))
        if len(hit):
            row = hit[0]
        else:
            live = np.flatnonzero(pos[blk])
            row = live[-1] if len(live) else 0
        keys[j] = blk * BLOCK + row
    return keys


def gather_offsets(keys, row_bytes: int, offset_bits: int = 64) -> np.ndarray:
    """A model of the gather's address arithmetic: the byte offset of each key's row into the
    ring, kept to `offset_bits` bits (64: what the kernels compute; 32: a truncated offset)."""
    o = np.asarray(keys, dtype=np.uint64) * np.uint64(row_bytes)
    return o if offset_bits >= 64 else o & np.uint64((1 << offset_bits) - 1)


def nstep_targets(rewards, done, q_star, n_step: int, gamma: float) -> np.ndarray:
    """The header's form in float64: K = L - 1 targets; d_t = gamma (1 - done_t), v_t = q_star[t+1],
    m = min(n_step, K - t); target_t = r_t + d_t (r_{t+1} + ... d_{t+m-1} v_{t+m-1})."""
    r = np.asarray(rewards, dtype=np.float64)
    d = np.float64(gamma) * (1.0 - np.asarray(done, dtype=np.float64))
    q = np.asarray(q_star, dtype=np.float64)
    K = len(r) - 1
    out = np.empty(K, dtype=np.float64)
    for t in range(K):
        m = min(n_step, K - t)
        acc = q[t + m]
        for k in range(t + m - 1, t - 1, -1):
            acc = r[k] + d[k] * acc
        out[t] = acc
    return out


def rlax_nstep(r_t, discount_t, v_t, n: int) -> np.ndarray:
    """rlax.n_step_bootstrapped_returns(r_t, discount_t, v_t, n, lambda_t=1.) transcribed:
    bootstrap values v_t[n-1:] padded with v_t[-1], rewards padded with 0 and discounts with 1,
    then n reversed accumulation steps."""
    r_t, discount_t, v_t = (np.asarray(x, dtype=np.float64) for x in (r_t, discount_t, v_t))
    seq_len = len(r_t)
    pad = min(n - 1, seq_len)
    targets = np.concatenate([v_t[n - 1:], np.full(pad, v_t[-1])])
    r_p = np.concatenate([r_t, np.zeros(n - 1)])
    d_p = np.concatenate([discount_t, np.ones(n - 1)])
    v_p = np.concatenate([v_t, np.full(n - 1, v_t[-1])])
    lam = 1.0
    for i in reversed(range(n)):
        r_, d_, v_ = r_p[i:i + seq_len], d_p[i:i + seq_len], v_p[i:i + seq_len]
        targets = r_ + d_ * ((1.0 - lam) * v_ + lam * targets)
    return targets


def rlax_targets(rewards, done, q_star, n_step: int, gamma: float) -> np.ndarray:
    """ApexActor._async_make_replay's call: the first K steps' rewards and discounts, values
    q_star[1:]."""
    r = np.asarray(rewards, dtype=np.float64)[:-1]
    d = np.float64(gamma) * (1.0 - np.asarray(done, dtype=np.float64)[:-1])
    return rlax_nstep(r, d, np.asarray(q_star, dtype=np.float64)[1:], n_step)
