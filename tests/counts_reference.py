"""How the three capped-grid integer kernels walk their input, restated in plain Python / numpy, and the case tables of
tests/test_gpu_counts_sweeps.py: k_confusion_counts (csrc/metrics.hip), k_edge_sym and k_edge_hash (csrc/graph.hip).  Nothing here
says what the kernels compute -- `recount` and `edges_symmetric` do that, from the definition -- only which workgroup, wave, sweep
and lane meets which row, and which thread of the last workgroup adds which partial.  Every case builder ASSERTS what its case is
there for (the sweep a row falls into, the merge round a workgroup is read in, the sweep that holds the edge that breaks the
symmetry), and tests/test_counts_reference.py runs every builder without a GPU: a case that misses its condition fails there.

`stand_in` is the kernel's walk in numpy, built from `cc_owner`'s formula and `cc_merge`, with switchable FAULTS (a wrong stride, a
dropped tail mask, swapped merge columns ...).  The CPU test shows that the clean stand-in equals `recount` and that every fault
changes the counts of some case of the tables: the evidence that the GPU tests would notice such an error, without running a
broken kernel on a GPU."""
import numpy as np

# ---------------------------------------------------------------------------
# k_confusion_counts: the launch geometry (csrc/metrics.hip)
# ---------------------------------------------------------------------------
CC_THREADS = 512
CC_WAVES = CC_THREADS // 64
CC_UNROLL = 4
CC_MAX_BLOCKS = 512
CC_MAX_CHANNELS = 8
CC_SPAN = 64 * CC_UNROLL                      # rows of a wave per sweep
CC_BLOCK_ROWS = CC_THREADS * CC_UNROLL        # rows of a workgroup per sweep: 2048
CC_PARTIAL_BYTES = 32                         # per channel and workgroup: four 64-bit counts
CC_FULL_WORKSPACE = CC_MAX_BLOCKS * CC_MAX_CHANNELS * CC_PARTIAL_BYTES       # ops.CONFUSION_WORKSPACE_BYTES
CC_CAP_ROWS = CC_MAX_BLOCKS * CC_BLOCK_ROWS   # 1,048,576: everything past it runs in sweeps 2, 3, ...


def cc_grid(rows, channels, workspace_bytes=CC_FULL_WORKSPACE):
    """The launcher's grid."""
    return min(-(-rows // CC_BLOCK_ROWS), CC_MAX_BLOCKS, workspace_bytes // (channels * CC_PARTIAL_BYTES))


def cc_sweeps(rows, grid):
    return -(-rows // (grid * CC_BLOCK_ROWS))


def cc_owner(row, grid):
    """(workgroup, wave, sweep, unroll slot, lane) that meets `row`: base = (wg * 8 + wave) * 256 + sweep * grid * 2048 and
    row = base + 64 u + lane."""
    sweep, r = divmod(int(row), grid * CC_BLOCK_ROWS)
    wg, r = divmod(r, CC_BLOCK_ROWS)
    wave, r = divmod(r, CC_SPAN)
    u, lane = divmod(r, 64)
    assert (wg * CC_WAVES + wave) * CC_SPAN + sweep * grid * CC_BLOCK_ROWS + 64 * u + lane == row
    return wg, wave, sweep, u, lane


def cc_stride(channels):
    """(NV, S, PER): values per partial, workgroups the last workgroup reads side by side, rounds it needs for the full grid."""
    nv = 4 * channels
    s = CC_THREADS // nv
    return nv, s, -(-CC_MAX_BLOCKS // s)


FAULTS = ("later_sweeps_skipped", "tail_mask_dropped", "step_short_by_a_wave", "merge_columns_swapped", "merge_later_rounds_dropped")


def cc_merge(partials, channels, fault=None):
    """The last workgroup's two-stage column sum of partials [grid, NV] -> [NV]: thread t < S * NV takes column t % NV of the
    workgroups t // NV + k * S, then thread j < NV adds s_red[k * NV + j] over k < S."""
    nv, s, per = cc_stride(channels)
    partials = np.asarray(partials, dtype=np.int64)
    grid = partials.shape[0]
    assert partials.shape == (grid, nv) and 1 <= grid <= CC_MAX_BLOCKS
    t = np.arange(s * nv)
    j = t % nv
    if fault == "merge_columns_swapped":
        j = j ^ 1
    s_red = np.zeros(s * nv, dtype=np.int64)
    for k in range(1 if fault == "merge_later_rounds_dropped" else per):
        b = t // nv + k * s
        s_red += np.where(b < grid, partials[np.minimum(b, grid - 1), j], 0)
    return s_red.reshape(s, nv).sum(axis=0)


def recount(pred, y, valid):
    """[C, 4] int64 {TP, FN, FP, TN} over the rows with valid > 0; label positive iff y != 0, prediction positive iff pred > 0.5
    (numpy's comparisons are the rule: NaN > x is false, NaN != 0 is true, -0.0 != 0 is false)."""
    v, pos, pp = np.asarray(valid) > 0, np.asarray(y) != 0, np.asarray(pred) > 0.5
    return np.stack([(v & pos & pp).sum(0), (v & pos & ~pp).sum(0), (v & ~pos & pp).sum(0), (v & ~pos & ~pp).sum(0)],
                    axis=-1).astype(np.int64)


def walk(pred, y, valid, grid, fault=None):
    """The workgroups' partials [grid, 4 C] of [rows, C] arrays: every wave counts {valid, valid & label, valid & predicted, all
    three} over its 4 x 64 rows per sweep (rows past the end load row rows - 1 and are masked), a workgroup adds its waves."""
    assert fault is None or fault in FAULTS
    pred, y, valid = (np.asarray(a) for a in (pred, y, valid))
    rows, ch = pred.shape
    nv = 4 * ch
    waves = grid * CC_WAVES
    cnt = np.zeros((waves, ch, 4), dtype=np.int64)
    base = np.arange(waves, dtype=np.int64) * CC_SPAN
    step = waves * CC_SPAN - (CC_SPAN if fault == "step_short_by_a_wave" else 0)
    offs = (64 * np.arange(CC_UNROLL)[:, None] + np.arange(64)[None, :]).reshape(1, -1)
    while True:
        act = np.flatnonzero(base < rows)
        if act.size == 0:
            break
        r = base[act, None] + offs                                      # [waves in range, 256]
        inside = np.ones_like(r, dtype=bool) if fault == "tail_mask_dropped" else r < rows
        rr = np.minimum(r, rows - 1)
        mv = (valid[rr] > 0) & inside[..., None]
        mp, mq = mv & (y[rr] != 0), mv & (pred[rr] > 0.5)
        for k, m in enumerate((mv, mp, mq, mp & mq)):
            cnt[act, :, k] += m.sum(axis=1)
        if fault == "later_sweeps_skipped":
            break
        base = base + step
    return cnt.reshape(grid, CC_WAVES, nv).sum(axis=1)


def record(merged, channels):
    """The record {TP, FN, FP, TN} [C, 4] the last workgroup forms from the four merged sums of every channel."""
    m = np.asarray(merged, dtype=np.int64).reshape(channels, 4)
    v, p, q, tp = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    return np.stack([tp, p - tp, q - tp, v - p - q + tp], axis=-1)


def stand_in(pred, y, valid, grid, fault=None):
    """The kernel in numpy: walk, cc_merge, record -> [C, 4] int64.  fault: one of FAULTS, or None."""
    ch = np.asarray(pred).shape[1]
    return record(cc_merge(walk(pred, y, valid, grid, fault), ch, fault), ch)


# ---------------------------------------------------------------------------
# inputs: every channel with rates of its own, the last row a valid true positive
# ---------------------------------------------------------------------------
def rates(c):
    """(share of valid rows, of positive labels, of positive predictions) of channel c."""
    return 0.55 + 0.05 * c, 0.12 + 0.07 * c, 0.25 + 0.06 * c


def _finish_inputs(pred, y, valid):
    pred[-1], y[-1], valid[-1] = 0.9, 1.0, 1.0
    return pred, y, valid


def _try_inputs(rows, channels, seed):
    rs = np.random.RandomState(seed)
    u = rs.uniform(0, 1, (3, rows, channels))
    rv, rp, rq = (np.array([rates(c)[k] for c in range(channels)]) for k in range(3))
    valid = (u[0] < rv).astype(np.float32)
    y = (u[1] < rp).astype(np.float32)
    pred = (u[2] + (rq - 0.5)).astype(np.float32)                        # > 0.5 in a share rq of the rows
    return _finish_inputs(pred, y, valid)


def counts_are_telling(counts):
    """All 4 C counts differ and none is zero: then a swapped column, a dropped partial or a doubled row changes the record."""
    flat = np.asarray(counts).reshape(-1)
    return bool((flat > 0).all() and len(set(flat.tolist())) == flat.size)


def inputs(rows, channels, seed):
    """(pred, y, valid) float32 [rows, C] on the host, the seed advanced until counts_are_telling (asserted)."""
    for s in range(seed, seed + 64 * 7919, 7919):
        pred, y, valid = _try_inputs(rows, channels, s)
        if counts_are_telling(recount(pred, y, valid)):
            return pred, y, valid
    raise AssertionError(f"no seed gives {4 * channels} distinct non-zero counts on {rows} rows")


# ---------------------------------------------------------------------------
# B1. sweeps at the smallest shapes
# ---------------------------------------------------------------------------
VARIANTS = ("16-byte loads", "4-byte offset")
SWEEP_GRIDS = (1, 2, 3)
SWEEP_K = (1, 2, 3)
SWEEP_TAILS = (0, 1, 63, 64, 65, 255, 257, 2047)
SWEEP_CHANNELS = 4


def sweep_case(grid, k, tail):
    """-> (rows, workspace_bytes): rows = grid * 2048 * k + tail on a grid forced through the workspace size."""
    rows = grid * CC_BLOCK_ROWS * k + tail
    ws = grid * SWEEP_CHANNELS * CC_PARTIAL_BYTES
    assert cc_grid(rows, SWEEP_CHANNELS, ws) == grid and cc_grid(rows, SWEEP_CHANNELS) == grid * k + (tail > 0)     # the clamp decides
    assert cc_sweeps(rows, grid) == k + (tail > 0)
    wg, wave, sweep, u, lane = cc_owner(rows - 1, grid)
    if tail == 0:
        # k whole sweeps: the last row is the last lane of the last workgroup; k >= 2 is the plain `base += step` walk
        assert (wg, wave, sweep, u, lane) == (grid - 1, CC_WAVES - 1, k - 1, CC_UNROLL - 1, 63)
    else:
        # the tail lies in a sweep of its own, in workgroup 0: every other workgroup finds base >= rows there
        assert (wg, sweep) == (0, k) and (wave, u, lane) == ((tail - 1) // CC_SPAN, (tail - 1) % CC_SPAN // 64, (tail - 1) % 64)
        partly = {1: (0, 0, 0), 63: (0, 0, 62), 65: (0, 1, 0), 255: (0, 3, 62), 257: (1, 0, 0), 2047: (7, 3, 62)}
        if tail in partly:                      # the last sweep holds a partly filled wave: the `rr = rows - 1` clamp runs there
            assert (wave, u, lane) == partly[tail] and rows % 64
        if tail == 64:                          # a full slot, and three slots of the same wave wholly past the end
            assert (wave, u, lane) == (0, 0, 63) and rows % 64 == 0 and rows % CC_SPAN
    return rows, ws


def sweep_cases():
    return [(g, k, t) for g in SWEEP_GRIDS for k in SWEEP_K for t in SWEEP_TAILS]


# ---------------------------------------------------------------------------
# B2. one row at a time
# ---------------------------------------------------------------------------
ROW_GRID = 3
ROW_ROWS = 3 * CC_BLOCK_ROWS * 2 + 130
ROW_AT = (0, 63, 64, 255, 256, 2047, 2048, 6143, 6144, 12287, 12288, ROW_ROWS - 1)
ROW_CHANNELS = (1, 4, 8)


def row_case():
    """-> (rows, grid, the rows singled out); asserted: where each of them is met."""
    owners = [cc_owner(r, ROW_GRID) for r in ROW_AT]
    assert owners == [(0, 0, 0, 0, 0), (0, 0, 0, 0, 63), (0, 0, 0, 1, 0), (0, 0, 0, 3, 63), (0, 1, 0, 0, 0), (0, 7, 0, 3, 63),
                      (1, 0, 0, 0, 0), (2, 7, 0, 3, 63), (0, 0, 1, 0, 0), (2, 7, 1, 3, 63), (0, 0, 2, 0, 0), (0, 0, 2, 2, 1)]
    assert cc_sweeps(ROW_ROWS, ROW_GRID) == 3 and {o[0] for o in owners} == {0, 1, 2} and {o[2] for o in owners} == {0, 1, 2}
    for ch in ROW_CHANNELS:
        assert cc_grid(ROW_ROWS, ch, ROW_GRID * ch * CC_PARTIAL_BYTES) == ROW_GRID
    return ROW_ROWS, ROW_GRID, ROW_AT


# ---------------------------------------------------------------------------
# B3. every channel count: the merge's strides
# ---------------------------------------------------------------------------
MERGE_CHANNELS = tuple(range(1, CC_MAX_CHANNELS + 1))


def merge_grids(channels):
    s = cc_stride(channels)[1]
    return (s - 1, s, s + 1, 2 * s + 1, CC_MAX_BLOCKS - 1, CC_MAX_BLOCKS)


def merge_case(channels, grid):
    """-> rows = (grid - 1) * 2048 + 77: one sweep on the natural grid; asserted: the round of the merge the last workgroup's
    partial is read in."""
    nv, s, per = cc_stride(channels)
    rows = (grid - 1) * CC_BLOCK_ROWS + 77
    assert cc_grid(rows, channels) == grid and cc_sweeps(rows, grid) == 1 and cc_owner(rows - 1, grid) == (grid - 1, 0, 0, 1, 12)
    assert s * per >= CC_MAX_BLOCKS > s * (per - 1) and s * nv <= CC_THREADS
    k_last, slot_last = divmod(grid - 1, s)
    want = {s - 1: (0, s - 2), s: (0, s - 1), s + 1: (1, 0), 2 * s + 1: (2, 0), CC_MAX_BLOCKS - 1: divmod(CC_MAX_BLOCKS - 2, s),
            CC_MAX_BLOCKS: (per - 1, (CC_MAX_BLOCKS - 1) % s)}
    assert (k_last, slot_last) == want[grid]
    if grid == s - 1:
        assert grid < s                         # the threads of slot S - 1 find no workgroup at all
    if grid == s + 1:
        assert k_last == 1                      # grid = S + 1 for this channel count: the first partial of the second round
    return rows


def merge_cases():
    """(channels, grid, variant): C = 4 runs both load variants."""
    out = []
    for ch in MERGE_CHANNELS:
        for g in merge_grids(ch):
            for v in (VARIANTS if ch == 4 else VARIANTS[:1]):
                out.append((ch, g, v))
    return out


HOST_ELEMENTS = 600000           # cases of rows * channels up to this size (every grid up to 2 S + 1) are also walked on the host


def on_host(rows, channels):
    return rows * channels <= HOST_ELEMENTS


# ---------------------------------------------------------------------------
# B4. full grid and several sweeps
# ---------------------------------------------------------------------------
FULL_CASES = ((4, 32 * 72020), (8, 2 * CC_CAP_ROWS + 4097))


def full_case(channels, rows):
    """Asserted: 512 workgroups, three sweeps, the last one ragged."""
    grid = cc_grid(rows, channels)
    assert grid == CC_MAX_BLOCKS and cc_sweeps(rows, grid) == 3 and rows > 2 * CC_CAP_ROWS
    wg, wave, sweep, u, lane = cc_owner(rows - 1, grid)
    assert sweep == 2 and wg < grid - 1                                   # the workgroups behind `wg` sit the last sweep out
    if channels == 4:
        assert rows == 2304640 and (wg, wave, u, lane) == (101, 2, 1, 63)         # batch 32 of the default frame
    else:
        assert (wg, wave, u, lane) == (2, 0, 0, 0)                         # one row in a workgroup of its own
    return grid


# ---------------------------------------------------------------------------
# B5. special values outside the first sweep
# ---------------------------------------------------------------------------
SPECIAL_GRID = 2
SPECIAL_ROWS = SPECIAL_GRID * CC_BLOCK_ROWS + 1500
SPECIAL_PRED = (np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), -np.inf, np.inf)
SPECIAL_VALID = (-1.0, 0.5, np.nan, -0.0, 1e-45)
SPECIAL_Y = (-0.0, np.nan, 1e-45, -1.0, 0.0)


def special_case(seed=77):
    """-> (pred, y, valid, rows singled out): every combination of the special values of the three arrays in sweep 2 and in the
    last 64 rows, the other arrays' entries of those rows such that the special value decides (valid 1, label 1, prediction 0.9)."""
    rows, ch = SPECIAL_ROWS, SWEEP_CHANNELS
    pred, y, valid = inputs(rows, ch, seed)
    first = SPECIAL_GRID * CC_BLOCK_ROWS                                  # first row of sweep 2
    combos = [(p, v, t) for p in SPECIAL_PRED for v in SPECIAL_VALID for t in SPECIAL_Y]
    singles = [(p, 1.0, 1.0) for p in SPECIAL_PRED] + [(0.9, v, 1.0) for v in SPECIAL_VALID] + [(0.9, 1.0, t) for t in SPECIAL_Y]
    picked = []
    for k, (p, v, t) in enumerate(combos):                                # sweep 2, from its first row on
        r, c = first + k // ch, k % ch
        pred[r, c], valid[r, c], y[r, c] = p, v, t
        picked.append(r)
    for k, (p, v, t) in enumerate(singles * ch):                          # the last 64 rows (but the very last)
        r, c = rows - 2 - k // ch, k % ch                                 # (15 values: each of them meets every channel)
        pred[r, c], valid[r, c], y[r, c] = p, v, t
        picked.append(r)
    picked = sorted(set(picked))
    assert cc_grid(rows, ch, SPECIAL_GRID * ch * CC_PARTIAL_BYTES) == SPECIAL_GRID and cc_sweeps(rows, SPECIAL_GRID) == 2
    assert all(cc_owner(r, SPECIAL_GRID)[2] == 1 for r in picked) and picked[0] == first
    assert any(rows - 64 <= r < rows - 1 for r in picked) and min(r for r in picked if r >= rows - 64) >= rows - 64
    assert max(r for r in picked if r < rows - 64) < rows - 64 - 100      # two separate groups
    for a in (pred, y, valid):
        assert np.isnan(a).any()
    assert (pred == 0.5).any() and np.signbit(valid[valid == 0]).any() and np.signbit(y[y == 0]).any()
    assert (valid[-1] == 1).all() and (y[-1] == 1).all() and (pred[-1] > 0.5).all()
    return pred, y, valid, picked


# ---------------------------------------------------------------------------
# B6. the ticket across grid sizes, B7. the hand-off at the full grid, B8. the workspace clamp
# ---------------------------------------------------------------------------
TICKET_GRIDS = (512, 1, 43, 512, 2)


def ticket_case(i):
    """-> (rows, workspace_bytes) of launch i of the sequence, four channels."""
    rows, ws = ((CC_CAP_ROWS + 3 * CC_BLOCK_ROWS + 5, CC_FULL_WORKSPACE),        # full grid, a short second sweep
                (1999, CC_FULL_WORKSPACE),
                (43 * CC_BLOCK_ROWS - 5, CC_FULL_WORKSPACE),
                (CC_CAP_ROWS, CC_FULL_WORKSPACE),                                # full grid, exactly one sweep
                (3 * 2 * CC_BLOCK_ROWS + 17, 2 * 4 * CC_PARTIAL_BYTES))[i]       # two workgroups through the workspace, four sweeps
    grid = cc_grid(rows, 4, ws)
    assert grid == TICKET_GRIDS[i] and cc_sweeps(rows, grid) == (2, 1, 1, 1, 4)[i]
    return rows, ws


HANDOFF_ROWS = CC_CAP_ROWS + CC_BLOCK_ROWS
HANDOFF_UPDATES = 16
HANDOFF_REPLAYS = 3


def handoff_case():
    grid = cc_grid(HANDOFF_ROWS, 4)
    assert grid == CC_MAX_BLOCKS and cc_sweeps(HANDOFF_ROWS, grid) == 2 and cc_owner(HANDOFF_ROWS - 1, grid) == (0, 7, 1, 3, 63)
    return HANDOFF_ROWS


CLAMP_ROWS = 5000


def clamp_case(channels=4):
    """-> (rows, bytes of exactly one workgroup's partial): grid 1, three sweeps; one byte less is no workspace at all."""
    per_block = channels * CC_PARTIAL_BYTES
    assert cc_grid(CLAMP_ROWS, channels, per_block) == 1 and cc_sweeps(CLAMP_ROWS, 1) == 3
    assert cc_grid(CLAMP_ROWS, channels, per_block - 1) == 0 and cc_grid(CLAMP_ROWS, channels) == 3
    return CLAMP_ROWS, per_block


# ---------------------------------------------------------------------------
# the edge kernels (csrc/graph.hip): k_edge_sym, k_edge_hash
# ---------------------------------------------------------------------------
EDGE_THREADS = 256
EDGE_MAX_BLOCKS = 2048
EDGE_SWEEP = EDGE_THREADS * EDGE_MAX_BLOCKS       # 524,288 edges per sweep of the capped grid


def edge_grid(n_edges):
    return min(max(-(-n_edges // EDGE_THREADS), 1), EDGE_MAX_BLOCKS)


def edge_owner(e, grid):
    """(workgroup, thread, sweep) that meets edge e."""
    sweep, r = divmod(int(e), grid * EDGE_THREADS)
    return r // EDGE_THREADS, r % EDGE_THREADS, sweep


def edges_kept(ei, n):
    """The entries a CSR keeps: no self loop, both ends in [0, n)."""
    s, d = ei[0], ei[1]
    return (s != d) & (s >= 0) & (d >= 0) & (s < n) & (d < n)


def edges_symmetric(ei, n):
    """The kept edge multiset equals its own transpose (A_hat^T == A_hat), from the definition: sorted keys."""
    k = edges_kept(ei, n)
    s, d = ei[0][k].astype(np.int64), ei[1][k].astype(np.int64)
    return bool(np.array_equal(np.sort(s * n + d), np.sort(d * n + s)))


EDGE_NODES = 4099
EDGE_PAIRS = 262300
EDGE_JUNK_AT = tuple(EDGE_SWEEP + 30 + 37 * i for i in range(6))          # entries both kernels' CSR ignores, all in sweep 2


def edge_case(seed=19):
    """-> (edge_index [2, E] int64, n): 262,300 distinct pairs a < b in both directions in a permuted order (524,600 edges, just
    past one sweep), and six entries a CSR drops (self loops, ends out of range) inserted into sweep 2.  Symmetric (asserted)."""
    n = EDGE_NODES
    rs = np.random.RandomState(seed)
    keys = np.unique(rs.randint(0, n * n, 3 * EDGE_PAIRS))
    a, b = keys // n, keys % n
    keys = keys[a < b]
    assert keys.size >= EDGE_PAIRS
    keys = rs.permutation(keys)[:EDGE_PAIRS]
    a, b = keys // n, keys % n
    assert np.unique(a * n + b).size == EDGE_PAIRS and (a < b).all()
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])[:, rs.permutation(2 * EDGE_PAIRS)]
    assert ei.shape[1] == 524600
    junk = np.array([[5, n, 3, -1, 2, n], [5, 3, n + 7, 2, -4, n]], dtype=np.int64)
    for k, at in enumerate(EDGE_JUNK_AT):
        ei = np.insert(ei, at, junk[:, k], axis=1)
    ei = np.ascontiguousarray(ei.astype(np.int64))
    E = ei.shape[1]
    grid = edge_grid(E)
    assert grid == EDGE_MAX_BLOCKS and EDGE_SWEEP < E < EDGE_SWEEP + 1024 and edge_owner(E - 1, grid)[2] == 1
    kept = edges_kept(ei, n)
    assert (~kept).sum() == len(EDGE_JUNK_AT) and all(not kept[at] and edge_owner(at, grid)[2] == 1 for at in EDGE_JUNK_AT)
    assert kept.sum() == 2 * EDGE_PAIRS and edges_symmetric(ei, n)
    return ei, n


def edge_breaks(n_edges):
    return (0, EDGE_SWEEP - 1, EDGE_SWEEP, n_edges - 1)


def edge_broken(ei, n, e):
    """-> (edge_index with edge e overwritten by a self loop, (source, target) of the edge that is gone): E unchanged, one
    direction missing.  Asserted: the sweep the edge lies in, and that the graph is no longer symmetric."""
    E = ei.shape[1]
    grid = edge_grid(E)
    s, d = int(ei[0, e]), int(ei[1, e])
    assert edges_kept(ei[:, e:e + 1], n)[0]
    out = ei.copy()
    out[1, e] = s
    want = {0: (0, 0, 0), EDGE_SWEEP - 1: (EDGE_MAX_BLOCKS - 1, EDGE_THREADS - 1, 0), EDGE_SWEEP: (0, 0, 1),
            E - 1: ((E - 1 - EDGE_SWEEP) // EDGE_THREADS, (E - 1) % EDGE_THREADS, 1)}       # the edge that breaks symmetry: sweep 1 or 2
    assert edge_owner(e, grid) == want[e] and out.shape == ei.shape and not edges_symmetric(out, n)
    return out, (s, d)


HASH_THREE_SWEEPS = 2 * EDGE_SWEEP + 1


def hash_case(seed=23):
    """A random directed edge list of three sweeps: two whole ones and a single edge."""
    rs = np.random.RandomState(seed)
    ei = rs.randint(0, EDGE_NODES, (2, HASH_THREE_SWEEPS)).astype(np.int64)
    grid = edge_grid(ei.shape[1])
    assert grid == EDGE_MAX_BLOCKS and edge_owner(ei.shape[1] - 1, grid) == (0, 0, 2)
    return ei


# ---------------------------------------------------------------------------
# what the cases reach, for the GPU module's docstring
# ---------------------------------------------------------------------------
def coverage_doc():
    def fmt(values):
        return ", ".join(str(v) for v in sorted(set(values)))

    lines = ["Reached by the case tables of tests/counts_reference.py (generated from them):", "", "k_confusion_counts"]
    sw = [(g, cc_sweeps(sweep_case(g, k, t)[0], g)) for g, k, t in sweep_cases()]
    lines.append(f"  1. sweeps: grids {fmt(g for g, _ in sw)} x sweeps {fmt(s for _, s in sw)}, 4 channels, tails {fmt(SWEEP_TAILS)}; "
                 f"{' and '.join(VARIANTS)}")
    lines.append(f"  2. one row: grid {ROW_GRID}, {cc_sweeps(ROW_ROWS, ROW_GRID)} sweeps, rows {fmt(ROW_AT)}, channel counts {fmt(ROW_CHANNELS)}")
    for ch in MERGE_CHANNELS:
        v = VARIANTS if ch == 4 else ("scalar loads",)
        lines.append(f"  3. merge: {ch} channel{'s' if ch > 1 else ''}, S = {cc_stride(ch)[1]}, grids {fmt(merge_grids(ch))}, one sweep; {' and '.join(v)}")
    for ch, rows in FULL_CASES:
        lines.append(f"  4. full grid: {ch} channels, {rows} rows, grid {full_case(ch, rows)}, {cc_sweeps(rows, CC_MAX_BLOCKS)} sweeps")
    lines.append(f"  5. special values: grid {SPECIAL_GRID}, {cc_sweeps(SPECIAL_ROWS, SPECIAL_GRID)} sweeps, {SPECIAL_ROWS} rows; {' and '.join(VARIANTS)}")
    tk = [(TICKET_GRIDS[i], cc_sweeps(ticket_case(i)[0], TICKET_GRIDS[i])) for i in range(len(TICKET_GRIDS))]
    lines.append("  6. ticket: grids " + ", ".join(f"{g} ({s} sweep{'s' if s > 1 else ''})" for g, s in tk) + " in one sequence on one stream")
    lines.append(f"  7. hand-off: grid {cc_grid(handoff_case(), 4)}, 2 sweeps, {HANDOFF_UPDATES} eager updates and {HANDOFF_REPLAYS} graph replays")
    lines.append(f"  8. workspace clamp: grid 1 from a workspace of one partial, {cc_sweeps(CLAMP_ROWS, 1)} sweeps; one byte less is refused")
    lines += ["", "k_edge_sym", f"  grid {EDGE_MAX_BLOCKS}, 2 sweeps: E = {2 * EDGE_PAIRS + len(EDGE_JUNK_AT)}"
              f" over {EDGE_NODES} nodes, symmetric, and with edge 0, {EDGE_SWEEP - 1}, {EDGE_SWEEP} or E - 1 replaced by a self loop",
              "", "k_edge_hash", f"  grid {EDGE_MAX_BLOCKS}, 2 sweeps (the same graphs, permuted and broken) and 3 sweeps (E = {HASH_THREE_SWEEPS})"]
    return "\n".join(lines)
