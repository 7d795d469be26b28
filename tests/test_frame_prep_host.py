"""Host side of the device frame preparation (csrc/frame_prep.hip, eg_frame_prep): the header's declaration, the wrapper's refusals,
data.affine_matrix / data.prep_coords and the fp64 restatement (tests/frame_prep_reference.py) against what the reference's own
functions recorded in tests/golden/frame_prep.npz, and the raw-frame mode of SyntheticEchoDataset / collate / copy_batch_.  No GPU."""
import ctypes as ct
import os
import types

import numpy as np
import pytest
import torch

import frame_prep_reference as R
import make_frame_prep_golden as G
from echoglad_amd import _lib, data, ops


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_prep.npz"))


def _matrices(name):
    """(forward, inverse) float32 [3, 2, 3] of a case's three frames, from data.affine_matrix."""
    _, _, W, _, crop, _ = G.CASES[name]
    pairs = [data.affine_matrix(tx=tx, ty=ty, sx=crop / W, sy=crop / W, rotation_theta=rot, shear_theta=sh) for tx, ty, rot, sh in G.PARAMS]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def test_header_declares_eg_frame_prep():
    assert _lib.ABI_VERSION >= 147
    hdr = open(_lib.HEADER_PATH).read()
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in hdr and "147: eg_frame_prep" in hdr
    res, args = _lib.SIGNATURES["eg_frame_prep"]
    p, i = ct.c_void_p, ct.c_int
    assert res is ct.c_int
    assert args == [p, i, i, i, i, i, p, i, i, p, i, p, p, p, i, p, p, p]
    assert "eg_frame_prep" in _lib.TAKES_STREAM
    assert "frame_prep.hip" in __import__("echoglad_amd.build", fromlist=["SOURCES"]).SOURCES


def test_ops_refuses_cpu_tensors_and_wrong_arguments():
    src = torch.zeros(2, 1, 8, 8, dtype=torch.uint8)
    out = torch.zeros(2, 1, 4, 4)
    m = torch.zeros(2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_prep(src, out)
    with pytest.raises(RuntimeError, match="needs matrix_inv"):
        ops.frame_prep(src, out, warp_size=6)
    with pytest.raises(RuntimeError, match="without a warp stage"):
        ops.frame_prep(src, out, matrix_inv=m)
    with pytest.raises(RuntimeError, match="warp_size must be >= 0"):
        ops.frame_prep(src, out, warp_size=-1)
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        ops.frame_prep(src.to(torch.int16), out)
    with pytest.raises(RuntimeError, match=r"\[B, C, Hs, Ws\]"):
        ops.frame_prep(src[0], out)


def test_affine_matrix_equals_the_references(golden):
    for name in G.CASES:
        fwd, inv = _matrices(name)
        assert fwd.dtype == inv.dtype == np.float32 and fwd.shape == inv.shape == (3, 2, 3)
        # the reference multiplies and inverts in float32: a few ulp of entries of magnitude <= 2
        assert np.abs(fwd - golden[name + "_matrix"][:, :2]).max() <= 2e-6, name
        assert np.abs(inv - golden[name + "_matrix_inv"][:, :2]).max() <= 2e-6, name
    f, i = data.affine_matrix()
    assert np.array_equal(f, np.eye(3, dtype=np.float32)[:2]) and np.array_equal(i, f)


def test_prep_coords_equals_the_references_integers(golden):
    for name, (_, _, W, F, crop, _) in G.CASES.items():
        src, coords = G.case_inputs(name)
        assert G.input_digest(src, coords) == str(golden[name + "_digest"]), name
        fwd, _ = _matrices(name)
        q = R.landmark_q_fp64(coords, F, fwd, crop, W)
        assert np.abs(q - np.round(q)).min() >= 2.0 ** -10, name          # none where float32 and fp64 may truncate differently
        got = data.prep_coords(coords, F, fwd, crop, W)
        assert got.dtype == np.int32 and np.array_equal(got, golden[name + "_coords"]), name
        assert np.array_equal(got, np.trunc(q))
        flipped = data.prep_coords(coords, F, fwd, crop, W, flip=G.FLIP)
        want = got.copy()
        want[1, :, 1] = F - want[1, :, 1] - 1
        assert np.array_equal(flipped, want)
    # no warp stage: frame-space integers are only truncated (and flipped: -1 becomes F)
    c = np.array([[[-1.0, -1.0], [15.0, 0.0], [3.9, 15.0], [-0.5, 7.0]]], dtype=np.float32)
    assert data.prep_coords(c, 16).tolist() == [[[-1, -1], [15, 0], [3, 15], [0, 7]]]
    assert data.prep_coords(c, 16, flip=[1]).tolist() == [[[-1, 16], [15, 15], [3, 0], [0, 8]]]
    assert data.prep_coords(np.full((1, 4, 2), np.nan), 16)[0, 0, 0] == np.iinfo(np.int32).min
    with pytest.raises(ValueError):
        data.prep_coords(c, 16, warp_size=8)


@pytest.mark.parametrize("name", list(G.CASES))
def test_restatement_equals_the_reference_and_torch_fp64(golden, name):
    _, _, W, F, _, _ = G.CASES[name]
    src, _ = G.case_inputs(name)
    _, inv = _matrices(name)
    got = R.frame_prep_fp64(src, F, inv, W)
    # the reference computes in float32: a source coordinate of magnitude <= 40 carries up to ~4 ulp (1.5e-5 of a pixel), the
    # bilinear blend has slope <= 1 per pixel and axis on values in [0, 1], two axes, two stages
    err = np.abs(got - golden[name + "_frame"]).max()
    t64 = R.torch_composition(src, F, inv, W, dtype=torch.float64).numpy()
    e64 = np.abs(got - t64).max()
    print(name, "restatement vs reference float32: %.3g, vs torch fp64: %.3g" % (err, e64))
    assert err <= 1e-4 and e64 <= 1e-12
    # ... with gray, a flip, three channels and a float32 source; and without a warp stage
    src3, _ = G.case_inputs(name, channels=3, dtype="float32")
    for gray in (False, True):
        a = R.frame_prep_fp64(src3, F, inv, W, flip=G.FLIP, gray=gray)
        b = R.torch_composition(src3, F, inv, W, flip=G.FLIP, gray=gray, dtype=torch.float64).numpy()
        assert a.shape == (3, 1 if gray else 3, F, F) and np.abs(a - b).max() <= 1e-12
    a = R.frame_prep_fp64(src, F)
    assert np.abs(a - R.torch_composition(src, F, dtype=torch.float64).numpy()).max() <= 1e-12


def _parent_sample(ds):
    """SyntheticEchoDataset.__getitem__ as it was before raw frames existed: the frame first, then the landmarks."""
    frame = ds.transform(torch.randn((1, 224, 224))).unsqueeze(0)
    coords = data.draw_coords(ds.frame_size)
    return frame, coords


@pytest.mark.parametrize("labels", ["dense", "coords"])
def test_prepared_samples_are_what_they_were(labels):
    ds = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True, labels=labels)
    assert ds.frames == "prepared"
    np.random.seed(5); torch.manual_seed(5)
    got = [ds[k] for k in range(3)]
    np.random.seed(5); torch.manual_seed(5)
    for g in got:
        frame, coords = _parent_sample(ds)
        assert torch.equal(g.x, frame) and torch.equal(g.node_coord_y, torch.tensor(coords, dtype=torch.float32))
        assert not hasattr(g, "raw_frame")
        if labels == "coords":
            assert torch.equal(g.label_coords, torch.from_numpy(coords.astype(np.int32))) and not hasattr(g, "y")
        else:
            want = np.stack([data.node_labels(c, 16, 3) for c in coords], axis=1)
            assert torch.equal(g.y, torch.from_numpy(want)) and not hasattr(g, "label_coords")
    b = data.collate(got, ds.topology)
    assert tuple(b.x.shape) == (3, 1, 16, 16) and not hasattr(b, "raw_frame")


def test_raw_samples_and_batches():
    np.random.seed(9)
    ds = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True, labels="coords", frames="raw",
                                   crop_size=40, warp_size=38, flip_p=0.5, make_gray=True,
                                   augment={"rotation": (-0.2, 0.2), "shear": (-0.1, 0.1), "translation": (-0.05, 0.05)})
    samples = [ds[k] for k in range(4)]
    for g in samples:
        assert g.raw_frame.dtype == torch.uint8 and tuple(g.raw_frame.shape) == (1, 3, 40, 40)
        assert g.raw_coords.dtype == torch.float32 and tuple(g.raw_coords.shape) == (4, 2)
        assert tuple(g.prep_matrix.shape) == tuple(g.prep_matrix_inv.shape) == (2, 3) and g.prep_matrix.dtype == torch.float32
        assert g.prep_flip.dtype == torch.uint8 and g.prep_flip.dim() == 0
        assert (g.prep_crop_size, g.prep_warp_size, g.prep_frame_size, g.prep_gray) == (40, 38, 16, True)
        assert not hasattr(g, "x") and not hasattr(g, "label_coords") and not hasattr(g, "node_coord_y")
        assert hasattr(g, "label_valid") and hasattr(g, "node_coords") and g.label_frame_size == 16
        # forward and inverse belong together
        full = lambda m: np.vstack([m.numpy().astype(np.float64), [0, 0, 1]])
        assert np.abs(full(g.prep_matrix) @ full(g.prep_matrix_inv) - np.eye(3)).max() < 1e-6
    b = data.collate(samples, ds.topology)
    assert tuple(b.raw_frame.shape) == (4, 3, 40, 40) and tuple(b.raw_coords.shape) == (4, 4, 2)
    assert tuple(b.prep_matrix.shape) == tuple(b.prep_matrix_inv.shape) == (4, 2, 3) and tuple(b.prep_flip.shape) == (4,)
    assert (b.prep_crop_size, b.prep_warp_size, b.prep_frame_size, b.prep_gray) == (40, 38, 16, True)
    assert not hasattr(b, "x") and not hasattr(b, "label_coords") and not hasattr(b, "node_coord_y")
    assert tuple(b.label_valid.shape) == (4, 4) and tuple(b.node_coords.shape) == (16, 2)
    # copy_batch_ copies the raw attributes like any other and leaves x / label_coords / node_coord_y of the static batch alone
    static = data.collate([ds[k] for k in range(4)], ds.topology)
    static.x = torch.full((4, 1, 16, 16), 7.0)
    static.label_coords = torch.full((4, 4, 2), 7, dtype=torch.int32)
    data.copy_batch_(static, b)
    assert torch.equal(static.raw_frame, b.raw_frame) and torch.equal(static.prep_matrix_inv, b.prep_matrix_inv)
    assert torch.equal(static.raw_coords, b.raw_coords) and torch.equal(static.prep_flip, b.prep_flip)
    assert float(static.x.min()) == 7.0 and int(static.label_coords.min()) == 7
    # a landmark that leaves [-F, F) is refused on the host, before anything is copied
    bad = data.collate(samples, ds.topology)
    bad.raw_coords = bad.raw_coords.clone()
    bad.raw_coords[1, 2, 0] = 200.0
    before = static.raw_frame.clone()
    with pytest.raises(IndexError):
        data.copy_batch_(static, bad)
    assert torch.equal(static.raw_frame, before)
    # no warp stage: frame-space integer landmarks, one channel, no matrices; dense labels are prepared on the host
    np.random.seed(9)
    ds2 = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, use_coordinate_graph=True, frames="raw", crop_size=28, flip_p=1.0)
    g = ds2[0]
    assert tuple(g.raw_frame.shape) == (1, 1, 28, 28) and not hasattr(g, "prep_matrix") and int(g.prep_flip) == 1
    want = data.prep_coords(g.raw_coords.numpy(), 16, flip=[1])[0]
    assert torch.equal(g.node_coord_y, torch.from_numpy(want.astype(np.float32)))
    assert torch.equal(g.y, torch.from_numpy(np.stack([data.node_labels(c, 16, 3) for c in want], axis=1)))
    with pytest.raises(ValueError):
        data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, frames="cooked")
    with pytest.raises(ValueError):
        data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16, frames="raw", augment={"rotation": (0, 1)})


def test_device_frames_is_a_no_op_without_raw_frames():
    ds = data.SyntheticEchoDataset(num_aux_graphs=3, frame_size=16)
    b = data.collate([ds[0], ds[1]], ds.topology)
    x = b.x
    assert data.device_frames_(b) is b and b.x is x
    empty = types.SimpleNamespace()
    assert data.device_frames_(empty) is empty and not vars(empty)
