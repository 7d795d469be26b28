#!/usr/bin/env python3
"""Generate tests/golden/frame_prep.npz by RUNNING THE REFERENCE'S OWN ``UICLVLandmark.get_affine_matrix``, ``transform_image``,
``apply_matrix_to_coords`` and ``normalize_coord`` / ``unnormalize_coord`` (src/core/datasets.py) in this container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_frame_prep_golden.py

The reference tree is imported read-only with its missing third-party modules stubbed (the recipe of make_golden.py).  Only OUTPUT
DATA is written.  The inputs are not stored: ``case_inputs`` regenerates them from the recorded seeds with numpy.random.default_rng
(the tests import it from here, on machines without the reference tree), and the fixture records a digest of them so that a
drifting regeneration fails the test instead of comparing against other data.

Per case (small shapes only, one channel, uint8 sources, three frames with three different matrices):
  <case>_matrix, <case>_matrix_inv   float32 [3, 3, 3]   get_affine_matrix(...) and its .inverse(), as get() builds them
  <case>_frame                       float32 [3, 1, F, F] transform_image(frame.float().div(255), inverse, W), then the resize to F.  There is
                                     no torchvision here: the resize is interpolate(bilinear, align_corners=False), what a tensor Resize
                                     without antialiasing computes.
  <case>_coords                      int64 [3, 4, 2]      normalize_coord -> apply_matrix_to_coords -> unnormalize_coord -> * F / W ->
                                     astype('int'), get()'s lines for the landmarks
  <case>_digest                      sha256 of the regenerated inputs
"""
import hashlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

import numpy as np

# name -> (src_h, src_w, warp, frame, crop, seed); crop: the side the landmarks are normalised by
CASES = {
    "s40_w38_f16": (40, 40, 38, 16, 40, 301),        # rotation 0.3, shear 0.1 and a shift: part of the output is zero padding
    "s37_w29_f16": (37, 37, 29, 16, 37, 302),        # all sizes odd
    "s20_w24_f24": (20, 20, 24, 24, 20, 303),        # the resize is the identity; upsampling warp, a wide band of padding
    "s24x40_w38_f30": (24, 40, 38, 30, 40, 304),     # a rectangular source, F not a multiple of any tile
}
# (tx, ty, rotation_theta, shear_theta) of the three frames of every case; the scale is crop / warp (the reference's only use)
PARAMS = [(0.05, -0.04, 0.3, 0.1), (0.0, 0.1, -0.2, 0.0), (0.0, 0.0, 0.0, 0.0)]
FLIP = [0, 1, 0]


def case_inputs(name, channels=1, dtype="uint8"):
    """(src [3, channels, src_h, src_w] uint8 or float32, coords float32 [3, 4, 2] in crop pixels) of one case."""
    sh, sw, _, _, crop, seed = CASES[name]
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0.2 * crop, 0.8 * crop, size=(3, 4, 2)).astype(np.float32)
    src = rng.integers(0, 256, size=(3, channels, sh, sw)).astype(np.uint8)
    if dtype != "uint8":
        src = (rng.standard_normal((3, channels, sh, sw)) * 0.5 + src / 255.0).astype(np.float32)
    return src, coords


def input_digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Dataset:
        def __init__(self, *a, **k):
            pass

    tg = mod("torch_geometric")
    tg.data = mod("torch_geometric.data", Dataset=_Dataset)
    tg.utils = mod("torch_geometric.utils", from_networkx=None)
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms")
    tv.transforms.functional = mod("torchvision.transforms.functional", hflip=lambda x: x)
    for name in ("imageio", "cv2"):
        try:
            __import__(name)
        except Exception:
            mod(name)


def main():
    import torch
    _install_stubs()
    sys.path.insert(0, REF)
    from src.core import datasets as RD                  # reference code, executed not copied
    ds = RD.UICLVLandmark
    # transform_image is a method that only calls self.apply_matrix_to_coords
    me = types.SimpleNamespace(apply_matrix_to_coords=ds.apply_matrix_to_coords)
    out = {}
    for name, (sh, sw, W, F, crop, seed) in CASES.items():
        src, coords = case_inputs(name)
        mats, invs, frames, marks = [], [], [], []
        for b, (tx, ty, rot, shear) in enumerate(PARAMS):
            m = ds.get_affine_matrix(tx=tx, ty=ty, sx=crop / W, sy=crop / W, rotation_theta=rot, shear_theta=shear)
            inv = m.inverse()
            frame = torch.from_numpy(src[b]).float().div(255)
            frame = ds.transform_image(me, image=frame, transform_matrix=inv, out_image_size=W)          # [1, W, W]
            frame = torch.nn.functional.interpolate(frame.unsqueeze(0), size=(F, F), mode="bilinear", align_corners=False)
            c = ds.normalize_coord(coord=torch.from_numpy(coords[b]), image_size=crop)
            c = ds.apply_matrix_to_coords(transform_matrix=m, coord=c)
            c = ds.unnormalize_coord(coord=c, image_size=W).squeeze().cpu().detach().numpy()
            c = (c * F / W).astype("int")
            mats.append(m.numpy()); invs.append(inv.numpy()); frames.append(frame[0].numpy()); marks.append(c)
        out[name + "_matrix"] = np.stack(mats).astype(np.float32)
        out[name + "_matrix_inv"] = np.stack(invs).astype(np.float32)
        out[name + "_frame"] = np.stack(frames).astype(np.float32)
        out[name + "_coords"] = np.stack(marks).astype(np.int64)
        out[name + "_digest"] = np.array(input_digest(src, coords))
        pad = float((out[name + "_frame"] == 0).mean())
        print(name, out[name + "_frame"].shape, "zero output pixels: %.1f %%" % (100 * pad), out[name + "_coords"][0].tolist())
    np.savez_compressed(os.path.join(HERE, "frame_prep.npz"), **out)


if __name__ == "__main__":
    main()
