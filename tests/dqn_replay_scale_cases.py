"""The inputs of tests/test_gpu_dqn_replay_scale.py, kept apart from it so that
tests/test_dqn_replay_host.py can show, on the CPU and on the oracle alone, that every draw the
GPU tests make satisfies their input condition: ring sizes, priority patterns with their zero
runs, seeds and counters, the rows of the large ring as a function of the row index, and the edge
rows around the byte offsets 2^31 and 2^32 of the observation ring."""
import itertools

import numpy as np

import dqn_replay_oracle as rorc

B = rorc.BLOCK
ROW = 3 * 64 * 64                     # bytes of one observation row
ALPHA = 0.6
NS = (1, 33, 512)
# rows -> (nb, chunk, active scan threads T)
SCAN_SHAPES = {5 * B + 7: (6, 3, 2), 10 * B: (10, 4, 3), 26 * B - 1: (26, 6, 5), 65 * B + 1: (66, 9, 8)}
PATTERNS = ("exact", "uniform")       # (i) log-uniform, alpha 0.6; (ii) k / 8, alpha 1
BIG = 360_000                         # 704 blocks, chunk 27, 27 scan threads; 4.42 GB of observations
BIG_NS = (33, 512)
# the first rows whose byte offset needs more than 31 / 32 bits: ceil(2^31 / ROW), ceil(2^32 / ROW)
BAND = (174_763, 349_526)
assert (BAND[0] - 1) * ROW < 2 ** 31 <= BAND[0] * ROW and (BAND[1] - 1) * ROW < 2 ** 32 <= BAND[1] * ROW

# chosen on the CPU (tests/test_dqn_replay_host.py asserts the condition for each; the figures are
# in the docstring of tests/test_gpu_dqn_replay_scale.py)
SCAN_SEED = 2025
BIG_SEED = 2025
UPDATE_SEED = 2025
UPDATE_N, UPDATE_COUNTER = 512, 7
STEP_SEED = 99


def counter(n: int) -> int:
    return 10 + n


def geometry(size: int):
    """-> (nb, chunk, T) of the draw kernel's scan at `size` rows."""
    nb = (size + B - 1) // B
    chunk = rorc.scan_chunk(nb)
    return nb, chunk, (nb + chunk - 1) // chunk


def zero_runs(size: int):
    """Row ranges [lo, hi) of exact zeros: the leading run, one scan thread's entire run of
    blocks, and the trailing run (the last block and three rows of the one before, so the last
    block of positive sum is not the last block).  With two scan threads the leading run is
    thread 0's entire run, and so it is on the large ring; elsewhere it ends inside a block."""
    nb, chunk, T = geometry(size)
    run = chunk * B
    if T == 2:
        return [(0, run), ((nb - 1) * B, size)]
    tz = T // 2
    lead = (0, run) if size == BIG else (0, B + 5)
    return [lead, (tz * run, (tz + 1) * run), ((nb - 1) * B - 3, size)]


def priorities(size: int, pattern: str):
    """-> (priorities [size] f32, alpha).  "exact": log-uniform over six decades (as
    test_gpu_dqn_replay.py's shape_priorities), alpha 0.6.  "uniform": k / 8, k uniform in 0..64,
    alpha 1 -- every weight and every partial sum in any order is an exact float64.  Both with
    the zero runs and a zero last row."""
    rng = np.random.default_rng(size)
    if pattern == "exact":
        p, alpha = (10.0 ** rng.uniform(-3, 3, size)).astype(np.float32), ALPHA
    else:
        p, alpha = (rng.integers(0, 65, size) / 8.0).astype(np.float32), 1.0
    p[-1] = 0.0
    for lo, hi in zero_runs(size):
        p[lo:hi] = 0.0
    return p, alpha


def condition(pattern: str, margin: float, discrepancy: float) -> bool:
    """The input condition of a draw: every u * total is further from a prefix boundary than
    summation order can move one.  "exact": 1000 x the measured discrepancy of the kernels' order
    (the factor covers the pairing inside a block sum, should the hardware's differ from the
    restatement's).  "uniform": the key does not depend on the order; 1e-13 covers the two
    roundings of order 1e-16, u * total and the residual."""
    return margin > (1000.0 * discrepancy if pattern == "exact" else 1e-13)


def bands(keys):
    """-> counts of keys below 2^31 bytes, between 2^31 and 2^32, above 2^32."""
    k = np.asarray(keys)
    return int((k < BAND[0]).sum()), int(((k >= BAND[0]) & (k < BAND[1])).sum()), int((k >= BAND[1]).sum())


# ---------------------------------------------------------------- the large ring's rows
_MUL, _SHIFT = 0x1F35A7BD, 20  # (row * ROW + byte) * _MUL < 2^63 for every row below 2^20


def row_bytes(xp, rows):
    """[n, ROW] bytes of the rows `rows` (int64, an array of numpy or a tensor of torch -- `xp` is
    the module): byte j of row r is bits 20..27 of (r * ROW + j) * _MUL, and bytes 0..2 are r
    itself, low byte first, so any two rows below 2^20 differ.  Rows >= BIG are the rows a later
    pass writes over row - BIG."""
    j = xp.arange(ROW, dtype=xp.int64)
    if xp is not np:
        j = j.to(rows.device)
    g = rows.reshape(-1, 1) * ROW + j.reshape(1, -1)
    out = ((g * _MUL) >> _SHIFT) & 0xFF
    for b in range(3):
        out[:, b] = (rows >> (8 * b)) & 0xFF
    return out.astype(np.uint8) if xp is np else out.to(xp.uint8)


def row_actions(rows):
    return rows % 15


def row_targets(xp, rows):
    """(row - 180224) / 65536: finite, exact in float32, distinct for rows below 2^20."""
    t = (rows - 180224) / 65536.0
    return t.astype(np.float32) if xp is np else t.to(xp.float32)


def ring_bytes(offsets, n: int) -> np.ndarray:
    """[len(offsets), n]: the n bytes at each byte offset of the large ring as first filled."""
    g = np.asarray(offsets, dtype=np.int64).reshape(-1, 1) + np.arange(n, dtype=np.int64).reshape(1, -1)
    r, j = g // ROW, g % ROW
    out = ((g * _MUL) >> _SHIFT) & 0xFF
    for b in range(3):
        out = np.where(j == b, (r >> (8 * b)) & 0xFF, out)
    return out.astype(np.uint8)


# ---------------------------------------------------------------- edge rows
# around byte offsets 0, one replay block, 2^30, 2^31, 2^32 and the end of the ring
STEP_ROWS = np.array([0, 1, 511, 512, 87_381, BAND[0] - 2, BAND[0] - 1, BAND[0], BAND[0] + 1, 262_144,
                      BAND[1] - 2, BAND[1] - 1, BAND[1], BAND[1] + 1, BIG - 2, BIG - 1], dtype=np.int64)
STEP_MUST = (0, 511, 512, BAND[0] - 1, BAND[0], BAND[1] - 1, BAND[1], BIG - 1)


def step_priorities():
    """Zero everywhere but the 16 edge rows."""
    p = np.zeros(BIG, dtype=np.float32)
    p[STEP_ROWS] = np.random.default_rng(16).uniform(0.5, 2.0, len(STEP_ROWS)).astype(np.float32)
    return p


# the update at high keys: the six edge keys, 0 and BAND[0] twice with two values each (either
# may land), BIG - 1 twice with one value; the values make each key a few percent of the total
UPDATE_KEYS = np.array([0, BAND[0] - 1, BAND[0], BAND[1] - 1, BAND[1], BIG - 1, BAND[0], 0, BIG - 1],
                       dtype=np.int64)
UPDATE_VALUES = np.array([1.0e8, 1.5e8, 2.0e8, 2.5e8, 3.0e8, 1.25e8, 0.75e8, 2.25e8, 1.25e8], dtype=np.float32)


def update_outcomes():
    """Every priority vector the update may leave over the large ring's "exact" pattern: one of
    the supplied values at each updated key."""
    base, _ = priorities(BIG, "exact")
    uniq = np.unique(UPDATE_KEYS)
    choices = [np.unique(UPDATE_VALUES[UPDATE_KEYS == k]) for k in uniq]
    for vals in itertools.product(*choices):
        p = base.copy()
        p[uniq] = vals
        yield p
