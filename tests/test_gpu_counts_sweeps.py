import functools

import numpy as np
import pytest
import torch

import counts_reference as R
import eval_reference as E
from echoglad_amd import evaluators, ops
from echoglad_amd.ops._core import call
from echoglad_amd.topology import commutative_edge_hash

__doc__ = """-m gpu: the three integer kernels that launch a capped grid and walk the rest of their input in grid-stride sweeps, past
their caps -- k_confusion_counts (csrc/metrics.hip: 512 workgroups x 2048 rows per sweep), k_edge_sym and k_edge_hash
(csrc/graph.hip: 2048 x 256 edges per sweep).  Their results are integers, so every comparison is exact: the records against a
torch int64 recount of the device tensors (and counts_reference.recount on the host where the arrays come from there), the
symmetry flag against the definition, the digest against topology.commutative_edge_hash.  History and counter are pre-filled, so
that a record that was not written shows; grids below the natural one are forced through `workspace_bytes`, which the C entry point
clamps the grid by (ops.confusion_counts refuses such a workspace, hence the direct call).  The only tolerance is
coord_reference.Report's rule for the two aggregations over a directed graph's handles, as tests/test_gpu_eval_fp64.py applies it.
tests/test_counts_reference.py checks every case table on the CPU, and shows on a numpy stand-in of the kernel that a skipped
sweep, a dropped tail mask, a short stride and a wrong merge each change the counts of these cases.

""" + R.coverage_doc()

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
FILL = -7                                  # what history holds where no record was written
BBA = evaluators.BalancedBinaryAccuracyEvaluator


# ---------------------------------------------------------------------------
# confusion counts
# ---------------------------------------------------------------------------
def _recount(pred, y, valid):
    """torch recount on the device tensors -> [C, 4] int64 on the device {TP, FN, FP, TN} (test_gpu_balanced_accuracy._recount)."""
    v, pos, pp = valid > 0, y != 0, pred > 0.5
    return torch.stack([(v & pos & pp).sum(0), (v & pos & ~pp).sum(0), (v & ~pos & pp).sum(0), (v & ~pos & ~pp).sum(0)], dim=-1)


def _device_inputs(rows, channels, seed):
    """counts_reference.inputs's distribution, drawn on the device (the arrays past the cap)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rv, rp, rq = (torch.tensor([R.rates(c)[k] for c in range(channels)], device=DEV) for k in range(3))
    valid = (torch.rand(rows, channels, device=DEV, generator=g) < rv).float()
    y = (torch.rand(rows, channels, device=DEV, generator=g) < rp).float()
    pred = torch.rand(rows, channels, device=DEV, generator=g) + (rq - 0.5)
    pred[-1], y[-1], valid[-1] = 0.9, 1.0, 1.0
    return pred, y, valid


def _upload(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _placed(tensors, variant):
    """The same rows 16-byte aligned (the 16-byte-load instance at four channels) or at a 4-byte offset (the scalar-load instance)."""
    out = []
    for t in tensors:
        if variant == R.VARIANTS[0]:
            assert t.data_ptr() % 16 == 0
            out.append(t)
            continue
        buf = torch.empty(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        out.append(v)
    return out


class _Records:
    """A pre-filled history, its counter and a workspace; every launch goes to eg_confusion_counts directly, with the workspace size
    the case asks for, and the expected record is kept on the device until `check` reads everything back once."""

    def __init__(self, capacity, channels):
        self.ch = channels
        self.history = torch.full((capacity + 1, channels, 4), FILL, dtype=torch.int64, device=DEV)
        self.counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.workspace = torch.full((ops.CONFUSION_WORKSPACE_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
        self.want, self.names = [], []

    def launch(self, name, pred, y, valid, workspace_bytes=R.CC_FULL_WORKSPACE, want=None, host_want=None):
        rows, ch = pred.shape
        assert ch == self.ch and all(t.shape == pred.shape and t.dtype == F32 and t.is_contiguous() for t in (pred, y, valid))
        call("eg_confusion_counts", pred, y, valid, rows, ch, self.workspace, int(workspace_bytes), self.history, self.history.shape[0],
             self.counter)
        w = _recount(pred, y, valid) if want is None else want
        self.want.append(w)
        self.names.append((name, None if host_want is None else np.asarray(host_want)))

    def check(self, telling=True, workspace_bytes=None):
        """workspace_bytes: what every launch was given -- the grid wrote that many bytes of partials and not one behind them."""
        n = len(self.want)
        if workspace_bytes is not None:
            assert bool((self.workspace[workspace_bytes:] == 0xA5).all()), "a partial behind the workspace the launch was given"
            assert bool((self.workspace[:workspace_bytes].view(torch.int64) >= 0).all()), "a partial the clamped grid did not write"
        got = self.history.cpu().numpy()
        want = torch.stack(self.want).cpu().numpy()
        assert int(self.counter.item()) == n
        assert (got[n:] == FILL).all()                                   # nothing behind the records was touched
        for k, (name, host_want) in enumerate(self.names):
            assert np.array_equal(got[k], want[k]), (name, got[k].tolist(), want[k].tolist())
            if host_want is not None:
                assert np.array_equal(got[k], host_want), (name, "host recount")
            if telling:
                assert R.counts_are_telling(want[k]), (name, want[k].tolist())
        return got[:n]


@pytest.mark.parametrize("grid", R.SWEEP_GRIDS)
def test_sweeps_at_the_smallest_shapes(grid):
    """1. grid 1, 2, 3 through the workspace size: rows = grid * 2048 * k + tail, both load variants."""
    cases = [(k, t) for g, k, t in R.sweep_cases() if g == grid]
    rec = _Records(len(cases) * len(R.VARIANTS), R.SWEEP_CHANNELS)
    for k, tail in cases:
        rows, ws = R.sweep_case(grid, k, tail)
        host = R.inputs(rows, R.SWEEP_CHANNELS, 1000 * grid + 10 * k + tail)
        dev = _upload(*host)
        for variant in R.VARIANTS:
            rec.launch((grid, k, tail, variant), *_placed(dev, variant), workspace_bytes=ws, host_want=R.recount(*host))
    rec.check(workspace_bytes=grid * R.SWEEP_CHANNELS * R.CC_PARTIAL_BYTES)


@pytest.mark.parametrize("channels", R.ROW_CHANNELS)
def test_one_row_at_a_time(channels):
    """2. everything invalid but one valid true positive at row r of channel c (TP[c] = 1, every other count 0), and the same with
    the row's other channels valid and negative (TN = 1 there)."""
    rows, grid, at = R.row_case()
    ws = grid * channels * R.CC_PARTIAL_BYTES
    rec = _Records(len(at) * channels * 2, channels)
    pred, y, valid = (torch.zeros(rows, channels, device=DEV) for _ in range(3))
    for r in at:
        for c in range(channels):
            for others in (False, True):
                pred[r, c], y[r, c], valid[r, c] = 0.9, 1.0, 1.0
                want = torch.zeros(channels, 4, dtype=torch.int64)
                want[c, 0] = 1
                if others:
                    valid[r, :] = 1.0
                    want[:, 3] = 1
                    want[c, 3] = 0
                rec.launch((r, c, others), pred, y, valid, workspace_bytes=ws, want=want.to(DEV))
                pred[r, c], y[r, c] = 0.0, 0.0
                valid[r, :] = 0.0
    rec.check(telling=False, workspace_bytes=ws)


@pytest.mark.parametrize("channels", R.MERGE_CHANNELS)
def test_every_channel_count_and_the_strides_of_the_merge(channels):
    """3. grid S - 1, S, S + 1, 2 S + 1, 511 and 512 with S = 512 // (4 C), one sweep; four channels with both load variants."""
    cases = [(g, v) for ch, g, v in R.merge_cases() if ch == channels]
    rec = _Records(len(cases), channels)
    for grid in R.merge_grids(channels):
        rows = R.merge_case(channels, grid)
        host = R.inputs(rows, channels, 31 * channels + grid) if R.on_host(rows, channels) else None
        dev = _upload(*host) if host is not None else _device_inputs(rows, channels, 31 * channels + grid)
        for variant in [v for g, v in cases if g == grid]:
            rec.launch((channels, grid, variant), *_placed(dev, variant), host_want=None if host is None else R.recount(*host))
        del dev
    rec.check()


@pytest.mark.parametrize("channels,rows", R.FULL_CASES)
def test_the_full_grid_over_three_sweeps(channels, rows):
    """4. 512 workgroups, three sweeps, the last one ragged: batch 32 of the default frame, and eight channels."""
    assert R.full_case(channels, rows) == R.CC_MAX_BLOCKS
    variants = R.VARIANTS if channels == 4 else R.VARIANTS[:1]
    rec = _Records(len(variants), channels)
    dev = _device_inputs(rows, channels, 4 + channels)
    for variant in variants:
        rec.launch((channels, rows, variant), *_placed(dev, variant))
    rec.check()


def test_special_values_outside_the_first_sweep():
    """5. NaN, 0.5, its successor and the infinities in pred, -1, 0.5, NaN, -0.0 and a denormal in valid, -0.0, NaN, a denormal and -1
    in y, in sweep 2 and in the last 64 rows: numpy's comparisons are the rule."""
    pred, y, valid, _ = R.special_case()
    want = R.recount(pred, y, valid)
    rec = _Records(len(R.VARIANTS), R.SWEEP_CHANNELS)
    dev = _upload(pred, y, valid)
    ws = R.SPECIAL_GRID * R.SWEEP_CHANNELS * R.CC_PARTIAL_BYTES
    for variant in R.VARIANTS:
        rec.launch(("specials", variant), *_placed(dev, variant), workspace_bytes=ws, host_want=want)
    rec.check(telling=False, workspace_bytes=ws)


def test_the_ticket_across_grid_sizes():
    """6. grids 512, 1, 43, 512, 2 on one stream into one history: the self-resetting ticket after every one of them."""
    rec = _Records(len(R.TICKET_GRIDS), 4)
    for i, grid in enumerate(R.TICKET_GRIDS):
        rows, ws = R.ticket_case(i)
        rec.launch((i, grid), *_device_inputs(rows, 4, 60 + i), workspace_bytes=ws)
    got = rec.check()
    assert got.shape == (5, 4, 4) and int(rec.counter.item()) == 5


def test_the_hand_off_at_the_full_grid():
    """7. 16 updates of the evaluator at 512 workgroups and two sweeps, then one captured update replayed on 3 new inputs."""
    rows = R.handoff_case()
    ev = BBA(None, max_updates=R.HANDOFF_UPDATES)
    want = []
    for k in range(R.HANDOFF_UPDATES):
        inp = _device_inputs(rows, 4, 700 + k)
        ev.update(*inp)
        want.append(_recount(*inp))
        del inp
    want = torch.stack(want).cpu().numpy()
    got = ev.counts()
    assert got.shape == (R.HANDOFF_UPDATES, 4, 4) and np.array_equal(got, want)
    assert all(R.counts_are_telling(w) for w in want) and len({w.tobytes() for w in want}) == R.HANDOFF_UPDATES

    ev = BBA(None, max_updates=R.HANDOFF_REPLAYS)
    static = [torch.empty(rows, 4, device=DEV) for _ in range(3)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for s, t in zip(static, _device_inputs(rows, 4, 799)):
            s.copy_(t)
        ev.update(*static)                                                # warm-up: the stream's ticket word is allocated here
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ev.update(*static)
    want = []
    for k in range(R.HANDOFF_REPLAYS):
        inp = _device_inputs(rows, 4, 800 + k)
        for s, t in zip(static, inp):
            s.copy_(t)
        graph.replay()
        want.append(_recount(*inp))
    torch.cuda.synchronize()
    want = torch.stack(want).cpu().numpy()
    assert np.array_equal(ev.counts(), want) and len({w.tobytes() for w in want}) == R.HANDOFF_REPLAYS


@pytest.mark.parametrize("channels", [4, 8])
def test_the_workspace_clamps_the_grid_and_a_smaller_one_is_refused(channels):
    """8. a workspace of exactly one workgroup's partial: grid 1; one byte less: refused before any launch."""
    rows, per_block = R.clamp_case(channels)
    rec = _Records(2, channels)
    inp = _upload(*R.inputs(rows, channels, 80 + channels))
    with pytest.raises(RuntimeError):
        rec.launch("refused", *inp, workspace_bytes=per_block - 1)
    torch.cuda.synchronize()
    assert int(rec.counter.item()) == 0 and bool((rec.history == FILL).all()) and not rec.want
    rec.launch("one partial", *inp, workspace_bytes=per_block, host_want=R.recount(*[t.cpu().numpy() for t in inp]))
    with pytest.raises(RuntimeError):
        rec.launch("refused", *inp, workspace_bytes=per_block - 1)
    rec.check(workspace_bytes=per_block)                                  # grid 1: one partial written, nothing behind it


# ---------------------------------------------------------------------------
# the edge kernels
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edges():
    return R.edge_case()


def _check_aggregates(g, ei, n, touched, title, capsys):
    """ops.gcn_aggregate on the handle and on its backward handle against A_hat x and A_hat^T x built from the edge list on the CPU
    (eval_reference.ahat: float64 the truth, float32 the yardstick, |x| the scale), as tests/test_gpu_eval_fp64.py does."""
    x = E.rand_rows(n, seed=29)
    xg = x.to(DEV)
    Eg = E.edges_of(ei[:, R.edges_kept(ei, n)], n)                       # (the entries out of range are no edges of the reference either)
    rep = E.Report()
    for name, handle, edges in (("A_hat x", g, Eg), ("A_hat^T x", g.bwd, E.transposed(Eg))):
        got = ops.gcn_aggregate(handle, 1, xg).cpu()
        r64, r32, scale = E.ahat(edges, x.double(), 1), E.ahat(edges, x, 1), E.ahat(edges, x.double().abs(), 1)
        rep.check(name, got, r64, r32, scale)
        if touched is not None:
            rows = list(touched)
            rep.check(f"{name}, rows {rows[0]} and {rows[1]} of the missing edge", got[rows], r64[rows], r32[rows], scale[rows])
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


def test_a_symmetric_graph_past_one_sweep_is_its_own_backward_handle(capsys):
    ei, n = _edges()
    g = ops.Graph.csr(torch.from_numpy(ei).to(DEV), n)
    assert g.bwd is g
    _check_aggregates(g, ei, n, None, f"symmetric graph, E = {ei.shape[1]}", capsys)


@pytest.mark.parametrize("which", range(4), ids=["first", "last_of_sweep_1", "first_of_sweep_2", "last"])
def test_one_missing_direction_in_either_sweep_makes_the_graph_directed(which, capsys):
    ei, n = _edges()
    e = R.edge_breaks(ei.shape[1])[which]
    broken, touched = R.edge_broken(ei, n, e)
    g = ops.Graph.csr(torch.from_numpy(broken).to(DEV), n)
    assert g.bwd is not g, f"edge {e} ({touched[0]} -> {touched[1]}) is missing and the handle calls itself symmetric"
    _check_aggregates(g, broken, n, touched, f"edge {e} = {touched[0]} -> {touched[1]} replaced by a self loop", capsys)


def test_the_edge_digest_past_one_sweep():
    ei, n = _edges()
    E_ = ei.shape[1]
    base = ops.edge_hash(torch.from_numpy(ei).to(DEV))
    assert base == commutative_edge_hash(ei) and base[0] == E_
    perm = np.random.RandomState(3).permutation(E_)
    assert ops.edge_hash(torch.from_numpy(np.ascontiguousarray(ei[:, perm])).to(DEV)) == base
    for e in R.edge_breaks(E_):
        broken, _ = R.edge_broken(ei, n, e)
        got = ops.edge_hash(torch.from_numpy(broken).to(DEV))
        assert got == commutative_edge_hash(broken) and got != base and got[0] == E_, e
    three = R.hash_case()
    assert ops.edge_hash(torch.from_numpy(three).to(DEV)) == commutative_edge_hash(three)
