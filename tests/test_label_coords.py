"""CPU: coordinate labels -- the closed form of the one-hot rows (data.label_rows), the ``labels="coords"`` samples and batches,
and eg_node_labels' argument checks (nothing is launched here).  Everything is 0.0 / 1.0 or an integer: exact comparisons only."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from echoglad_amd import _lib, data, losses

CONFIGS = [(16, 3, False), (30, 3, False), (16, 4, False), (16, 2, True)]      # (F, naux, main only); 16/4: an aux level of side F


def _rows_by_nonzero(coords, frame, naux, main_only):
    """[n_levels, K] from np.nonzero of the host labels: one ``1`` per level, in level order."""
    return np.stack([np.nonzero(data.node_labels(c, frame, naux, main_only))[0] for c in coords], axis=1)


@pytest.mark.parametrize("frame,naux,main_only", [(16, 3, False), (30, 3, False), (64, 2, False), (224, 7, False), (16, 2, True)])
def test_label_rows_match_the_references_labels(golden_dir, frame, naux, main_only):
    d = np.load(os.path.join(golden_dir, "labels.npz"))
    key = f"F{frame}_A{naux}_mo{int(main_only)}"
    coords, ones = d[key + "_coords"], d[key + "_ones"]
    assert (coords < 0).any()                                          # the fixture includes -1 (numpy's wrap-around)
    rows = data.label_rows(coords, frame, naux, main_only)
    assert rows.dtype == np.int64 and rows.shape == (ones.shape[1], len(coords))
    assert np.array_equal(rows.T, ones)                                # the reference's own create_node_labels
    assert np.array_equal(rows, _rows_by_nonzero(coords, frame, naux, main_only))
    levels = losses.level_grids(frame, naux, main_only)
    for (start, side), r in zip(levels, rows):
        assert ((r >= start) & (r < start + side * side)).all()


@pytest.mark.parametrize("frame,naux,main_only", CONFIGS)
def test_label_rows_exhaustive(frame, naux, main_only):
    """Every (h, w) in [-F, F)^2 against np.nonzero(node_labels)."""
    vs = np.arange(-frame, frame)
    coords = np.stack(np.meshgrid(vs, vs, indexing="ij"), axis=-1).reshape(-1, 2)
    assert np.array_equal(data.label_rows(coords, frame, naux, main_only), _rows_by_nonzero(coords, frame, naux, main_only))


def test_label_rows_out_of_range_raises_where_node_labels_does():
    for args in (([16, 0], 16, 3), ([0, -17], 16, 2, True)):
        with pytest.raises(IndexError):
            data.node_labels(*args)
        with pytest.raises(IndexError):
            data.label_rows([args[0]], *args[1:])
    assert data.label_rows([[15, -16]], 16, 3).shape == (4, 1)       # the last values inside


def test_coords_sample_carries_the_same_landmarks_as_the_dense_one():
    kw = dict(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True)
    dense, sparse = data.SyntheticEchoDataset(**kw), data.SyntheticEchoDataset(labels="coords", **kw)
    np.random.seed(78)
    torch.manual_seed(0)
    a = dense[0]
    np.random.seed(78)
    torch.manual_seed(0)
    b = sparse[0]
    assert not hasattr(b, "y") and not hasattr(b, "valid_labels")
    assert b.label_coords.dtype == torch.int32 and tuple(b.label_coords.shape) == (4, 2)
    assert b.label_valid.dtype == torch.float32 and torch.equal(b.label_valid, torch.ones(4))
    rows = data.label_rows(b.label_coords.numpy(), 16, 3)
    want = np.stack([np.nonzero(a.y[:, c].numpy())[0] for c in range(4)], axis=1)
    assert np.array_equal(rows, want)
    assert torch.equal(a.node_coord_y, b.node_coord_y) and torch.equal(a.x, b.x)
    assert torch.equal(b.node_coord_y, b.label_coords.to(torch.float32))
    with pytest.raises(ValueError):
        data.SyntheticEchoDataset(labels="sparse", **kw)


def test_collate_stacks_the_coordinates():
    np.random.seed(3)
    ds = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True, labels="coords")
    b = data.collate([ds[0], ds[1], ds[2]], ds.topology)
    assert not hasattr(b, "y") and not hasattr(b, "valid_labels")
    assert tuple(b.label_coords.shape) == (3, 4, 2) and b.label_coords.dtype == torch.int32
    assert tuple(b.label_valid.shape) == (3, 4) and b.label_valid.dtype == torch.float32
    assert list(b.label_levels) == losses.level_grids(16, 3) and b.label_frame_size == 16
    assert torch.equal(b.label_coords.reshape(12, 2).to(torch.float32), b.node_coord_y)
    moved = data.to_device(b, "meta")
    assert moved.label_coords.device.type == "meta" and moved.label_valid.device.type == "meta"
    assert list(moved.label_levels) == losses.level_grids(16, 3)
    dense = data.collate([data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16)[0]])
    assert not hasattr(dense, "label_coords") and tuple(dense.y.shape) == (340, 4)       # the default is unchanged
    assert data.device_labels_(dense) is dense                                            # nothing to expand: a no-op


def test_copy_batch_checks_cpu_coordinates_before_it_writes():
    np.random.seed(4)
    ds = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True, labels="coords")
    static = data.collate([ds[0], ds[1]], ds.topology)
    static.y = torch.full((2 * 340, 4), 7.0)                          # what device_labels_ would own: copy_batch_ leaves it alone
    good = data.collate([ds[2], ds[3]], ds.topology)
    bad = data.collate([ds[4], ds[5]], ds.topology)
    bad.label_coords = bad.label_coords.clone()
    bad.label_coords[1, 2, 0] = 16
    before = {k: v.clone() for k, v in vars(static).items() if torch.is_tensor(v)}
    with pytest.raises(IndexError):
        data.copy_batch_(static, bad)
    for k, v in before.items():
        assert torch.equal(getattr(static, k), v), k                   # nothing was written, x included
    bad.label_coords[1, 2, 0] = -17
    with pytest.raises(IndexError):
        data.copy_batch_(static, bad)
    data.copy_batch_(static, good)
    assert torch.equal(static.label_coords, good.label_coords) and torch.equal(static.x, good.x)
    assert torch.equal(static.y, before["y"])


def test_node_labels_entry_point_refuses_bad_arguments(built_lib):
    """EG_ERR_ARG with a message for every bad argument; the device pointers are null throughout, so nothing can be launched."""
    lib = _lib.load()

    def arr(*v):
        return (ct.c_int * len(v))(*v)

    start, side = arr(0, 4, 20, 84), arr(2, 4, 8, 16)                  # F = 16, naux = 3: 340 rows

    def call(batch=2, n_rows=340, start=start, side=side, n_levels=4, frame=16):
        return lib.eg_node_labels(None, None, batch, n_rows, start, side, n_levels, frame, None, None, None)

    cases = [(dict(batch=0), "batch"), (dict(n_levels=0), "n_levels"), (dict(n_levels=17), "n_levels"),
             (dict(n_rows=339), "does not fit"), (dict(start=arr(0, 4, 20, 85)), "does not fit"),
             (dict(start=arr(0, 4, -1, 84)), "does not fit"), (dict(side=arr(2, 4, 0, 16)), "does not fit"),
             (dict(frame=15), "frame_size"), (dict(side=arr(2, 4, 8, 15)), "frame_size"),
             (dict(), "NULL")]                                          # all else fine: null coords / labels
    for kw, word in cases:
        assert call(**kw) == _lib.EG_ERR_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.SIGNATURES["eg_node_labels"][1] == [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_int,
                                                    ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    assert "eg_node_labels" in _lib.TAKES_STREAM and _lib.ABI_VERSION >= 144


def test_ops_wrapper_refuses_host_tensors():
    from echoglad_amd import ops
    coords = torch.zeros(2, 4, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="coords must be a CUDA"):
        ops.node_labels(coords, None, 2, losses.level_grids(16, 3), 16, torch.zeros(680, 4))
