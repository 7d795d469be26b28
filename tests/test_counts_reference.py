"""tests/counts_reference.py without a GPU: the walk of k_confusion_counts and of the edge kernels restated, every case builder of
tests/test_gpu_counts_sweeps.py against the condition it was built for, the numpy stand-in of the kernel against the plain recount
on every case that fits the host, and the evidence that the GPU cases are telling: each fault the stand-in can be given (later
sweeps skipped, tail mask dropped, a short stride, swapped merge columns, merge rounds left out) changes the counts of some case."""
import numpy as np
import pytest

import counts_reference as R
from echoglad_amd.topology import commutative_edge_hash


def test_the_grid_and_owner_formulas_on_the_numbers_the_suite_and_the_workloads_use():
    assert R.cc_grid(216060, 4) == 106 and R.cc_sweeps(216060, 106) == 1            # the largest input of the golden cases
    assert R.cc_grid(14 * 72020, 4) == 493 and R.cc_grid(15 * 72020, 4) == 512 and R.cc_sweeps(15 * 72020, 512) == 2
    assert R.cc_grid(32 * 72020, 4) == 512 and R.cc_sweeps(32 * 72020, 512) == 3
    assert R.CC_FULL_WORKSPACE == 512 * 8 * 32 and R.cc_grid(10 ** 9, 8) == 512 and R.cc_grid(1, 8) == 1
    assert R.cc_grid(10 ** 6, 5, 7 * 5 * 32 + 31) == 7
    assert [R.cc_stride(c) for c in (1, 3, 4, 7, 8)] == [(4, 128, 4), (12, 42, 13), (16, 32, 16), (28, 18, 29), (32, 16, 32)]
    # every row of an array has exactly one owner, and owners do not collide
    for rows, grid in ((5000, 1), (12418, 3), (70000, 5)):
        seen = {R.cc_owner(r, grid) for r in range(rows)}
        assert len(seen) == rows and all(wg < grid and wave < 8 and u < 4 and lane < 64 for wg, wave, _, u, lane in seen)
    assert R.edge_grid(0) == 1 and R.edge_grid(256) == 1 and R.edge_grid(257) == 2 and R.edge_grid(524288) == 2048 == R.edge_grid(10 ** 7)
    assert R.edge_owner(524287, 2048) == (2047, 255, 0) and R.edge_owner(524288, 2048) == (0, 0, 1) and R.edge_owner(300, 2) == (1, 44, 0)


@pytest.mark.parametrize("channels", R.MERGE_CHANNELS)
def test_the_merge_is_a_column_sum_at_every_grid(channels):
    rs = np.random.RandomState(channels)
    for grid in sorted(set(R.merge_grids(channels)) | {1, 2, 3, 100}):
        p = rs.randint(0, 1 << 40, (grid, 4 * channels)).astype(np.int64)
        assert np.array_equal(R.cc_merge(p, channels), p.sum(axis=0)), grid


def test_recount_on_a_hand_made_table():
    nan = np.nan
    #                 TP    FN    FP    TN   invalid ...
    pred = np.array([0.6, 0.5, 0.51, nan, 0.9, 0.9, 0.9], np.float32)[:, None]
    y = np.array([1.0, 2.0, 0.0, -0.0, 1.0, 1.0, nan], np.float32)[:, None]
    valid = np.array([1.0, 0.5, 1e-3, 1.0, 0.0, nan, -1.0], np.float32)[:, None]
    assert R.recount(pred, y, valid).tolist() == [[1, 1, 1, 1]]
    y[6], valid[6] = nan, 1.0                                           # a NaN label is a positive label
    assert R.recount(pred, y, valid).tolist() == [[2, 1, 1, 1]]
    assert R.stand_in(pred, y, valid, 1).tolist() == [[2, 1, 1, 1]]


SMALL = [(g, k, t) for g, k, t in R.sweep_cases()]


@pytest.mark.parametrize("grid", R.SWEEP_GRIDS)
def test_sweep_cases_meet_their_conditions_and_the_stand_in_recounts_them(grid):
    for g, k, tail in SMALL:
        if g != grid:
            continue
        rows, ws = R.sweep_case(g, k, tail)
        pred, y, valid = R.inputs(rows, R.SWEEP_CHANNELS, 1000 * g + 10 * k + tail)
        want = R.recount(pred, y, valid)
        assert R.counts_are_telling(want) and want[:, 0].min() >= 1
        assert np.array_equal(R.stand_in(pred, y, valid, g), want), (g, k, tail)


def test_the_one_row_case_meets_its_conditions():
    rows, grid, at = R.row_case()
    for ch in R.ROW_CHANNELS:
        for r in at:
            for c in (0, ch - 1):
                pred, y, valid = (np.zeros((rows, ch), np.float32) for _ in range(3))
                pred[r, c], y[r, c], valid[r, :] = 0.9, 1.0, 1.0
                want = np.zeros((ch, 4), np.int64)
                want[:, 3] = 1
                want[c] = (1, 0, 0, 0)
                assert np.array_equal(R.recount(pred, y, valid), want) and np.array_equal(R.stand_in(pred, y, valid, grid), want)


MERGE = sorted({(ch, g) for ch, g, _ in R.merge_cases()})


def test_merge_cases_cover_every_channel_count_and_both_variants_at_four():
    cases = R.merge_cases()
    assert {c for c, _, _ in cases} == set(range(1, 9)) and len(cases) == 8 * 6 + 6
    assert {v for c, _, v in cases if c == 4} == set(R.VARIANTS) and {v for c, _, v in cases if c != 4} == {R.VARIANTS[0]}
    for ch, grid in MERGE:
        rows = R.merge_case(ch, grid)
        assert R.on_host(rows, ch) == (grid < 511)


@pytest.mark.parametrize("channels", R.MERGE_CHANNELS)
def test_the_stand_in_recounts_the_merge_cases_that_fit_the_host(channels):
    for ch, grid in MERGE:
        rows = R.merge_case(ch, grid)
        if ch != channels or not R.on_host(rows, ch):
            continue
        pred, y, valid = R.inputs(rows, ch, 31 * ch + grid)
        want = R.recount(pred, y, valid)
        partials = R.walk(pred, y, valid, grid)
        assert np.array_equal(R.record(R.cc_merge(partials, ch), ch), want), (ch, grid)
        # the merge's faults on the same partials: columns swapped always shows; rounds k >= 1 left out shows once grid > S
        s = R.cc_stride(ch)[1]
        assert not np.array_equal(R.record(R.cc_merge(partials, ch, "merge_columns_swapped"), ch), want), (ch, grid)
        dropped = R.record(R.cc_merge(partials, ch, "merge_later_rounds_dropped"), ch)
        assert np.array_equal(dropped, want) == (grid <= s), (ch, grid)


def test_the_remaining_confusion_cases_meet_their_conditions():
    for ch, rows in R.FULL_CASES:
        assert R.full_case(ch, rows) == 512
    for i in range(len(R.TICKET_GRIDS)):
        R.ticket_case(i)
    assert R.handoff_case() == 1048576 + 2048
    assert R.clamp_case(4) == (5000, 128) and R.clamp_case(8) == (5000, 256)
    pred, y, valid, picked = R.special_case()
    want = R.recount(pred, y, valid)
    assert np.array_equal(R.stand_in(pred, y, valid, R.SPECIAL_GRID), want)
    # the special rows matter: the same arrays with those rows made plain give other counts
    p2, y2, v2 = pred.copy(), y.copy(), valid.copy()
    p2[picked], y2[picked], v2[picked] = 0.9, 1.0, 1.0
    assert not np.array_equal(R.recount(p2, y2, v2), want)


def _fault_table():
    """fault -> the sweep cases (grid, k, tail) whose counts it changes."""
    caught = {f: [] for f in R.FAULTS}
    for g, k, tail in SMALL:
        rows, _ = R.sweep_case(g, k, tail)
        pred, y, valid = R.inputs(rows, R.SWEEP_CHANNELS, 1000 * g + 10 * k + tail)
        want = R.recount(pred, y, valid)
        for f in R.FAULTS:
            if not np.array_equal(R.stand_in(pred, y, valid, g, f), want):
                caught[f].append((g, k, tail))
    return caught


def test_every_fault_changes_the_counts_of_the_cases_built_for_it():
    caught = _fault_table()
    multi = [(g, k, t) for g, k, t in SMALL if k + (t > 0) >= 2]
    assert caught["later_sweeps_skipped"] == multi                      # every case with a second sweep, and no other
    # a stride short by one wave stays below `rows` even in a single whole sweep: wave 0 walks the last wave's rows again
    assert caught["step_short_by_a_wave"] == SMALL
    # out-of-range lanes of a wave that is still in range count row rows - 1, a valid true positive in every channel
    assert caught["tail_mask_dropped"] == [(g, k, t) for g, k, t in SMALL if (g * 2048 * k + t) % 256]
    assert caught["merge_columns_swapped"] == SMALL                     # all 4 C counts differ: any swap shows
    assert caught["merge_later_rounds_dropped"] == []                   # needs grid > S: the merge cases (above), grids S + 1 and up
    full = R.cc_stride(4)[1] + 1
    pred, y, valid = R.inputs(R.merge_case(4, full), 4, 5)
    assert not np.array_equal(R.stand_in(pred, y, valid, full, "merge_later_rounds_dropped"), R.recount(pred, y, valid))
    # the one-row cases see a skipped sweep and a short stride as well: the row is simply not counted, or counted twice
    rows, grid, _ = R.row_case()
    pred, y, valid = (np.zeros((rows, 1), np.float32) for _ in range(3))
    pred[6144], y[6144], valid[6144] = 0.9, 1.0, 1.0
    assert R.stand_in(pred, y, valid, grid).tolist() == [[1, 0, 0, 0]]
    assert R.stand_in(pred, y, valid, grid, "later_sweeps_skipped").tolist() == [[0, 0, 0, 0]]
    pred[:], y[:], valid[:] = 0, 0, 0
    pred[6143], y[6143], valid[6143] = 0.9, 1.0, 1.0                    # the last row of sweep 1: a short stride meets it again
    assert R.stand_in(pred, y, valid, grid, "step_short_by_a_wave").tolist() == [[2, 0, 0, 0]]


def test_edge_cases_meet_their_conditions():
    ei, n = R.edge_case()
    E = ei.shape[1]
    assert E == 524606 and n == R.EDGE_NODES and ei.dtype == np.int64
    base = commutative_edge_hash(ei)
    assert base[0] == E
    perm = np.random.RandomState(3).permutation(E)
    assert commutative_edge_hash(ei[:, perm]) == base
    for e in R.edge_breaks(E):
        out, (s, d) = R.edge_broken(ei, n, e)
        assert (out[:, e] == s).all() and s != d and (np.delete(out, e, axis=1) == np.delete(ei, e, axis=1)).all()
        assert commutative_edge_hash(out) != base
        # the reverse direction is still there, once
        assert ((out[0] == d) & (out[1] == s)).sum() == 1 and ((out[0] == s) & (out[1] == d)).sum() == 0
    h = R.hash_case()
    assert h.shape == (2, 2 * 524288 + 1) and not R.edges_symmetric(h, n)
    # the definition on hand-made lists
    tri = np.array([[0, 1, 1, 2, 5, 9], [1, 0, 2, 1, 5, 0]], dtype=np.int64)
    assert R.edges_symmetric(tri, 3) and not R.edges_symmetric(tri, 10) and R.edges_kept(tri, 3).tolist() == [True] * 4 + [False] * 2


def test_the_gpu_modules_docstring_is_generated_from_the_tables():
    import test_gpu_counts_sweeps as G
    doc = R.coverage_doc()
    assert doc in G.__doc__
    for word in ("k_confusion_counts", "k_edge_sym", "k_edge_hash", "grids 1, 2, 3 x sweeps 1, 2, 3, 4", "8 channels, S = 16, grids 15, 16, 17, 33, 511, 512",
                 "4 channels, 2304640 rows, grid 512, 3 sweeps", "E = 524606", "E = 1048577"):
        assert word in doc, word
