"""Not a test: the rule of eg_frame_prep (include/echoglad_hip.h) restated per pixel in numpy fp64, and the composition of torch
operators it stands for (affine_grid, grid_sample, interpolate, flip) in a chosen dtype.  The GPU and host tests compare the kernel,
the restatement and torch with one another; nothing here calls the package."""
import numpy as np
import torch

GRAY = (0.2989, 0.587, 0.114)


def source_values(src) -> np.ndarray:
    """v of the rule in fp64: src / 255 for uint8, src itself for float32."""
    a = np.asarray(src)
    return a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)


def _tap(v, y, x):
    """v [C, Hs, Ws] at integer index arrays (y, x) of one shape, 0 outside -> [C, *shape]."""
    Hs, Ws = v.shape[1:]
    ok = (y >= 0) & (y < Hs) & (x >= 0) & (x < Ws)
    return np.where(ok[None], v[:, np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)], 0.0)


def warp_fp64(v, matrix_inv, W: int) -> np.ndarray:
    """v [B, C, Hs, Ws] fp64, matrix_inv [B, 2, 3] -> the warped image [B, C, W, W]."""
    B, C, Hs, Ws = v.shape
    m = np.asarray(matrix_inv, dtype=np.float64)
    n = (2.0 * np.arange(W) + 1.0) / W - 1.0
    nh, nw = n[:, None], n[None, :]
    out = np.empty((B, C, W, W))
    for b in range(B):
        sh = m[b, 0, 0] * nh + m[b, 0, 1] * nw + m[b, 0, 2]
        sw = m[b, 1, 0] * nh + m[b, 1, 1] * nw + m[b, 1, 2]
        y, x = ((sh + 1.0) * Hs - 1.0) / 2.0, ((sw + 1.0) * Ws - 1.0) / 2.0
        y0, x0 = np.floor(y), np.floor(x)
        fy, fx = y - y0, x - x0
        y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
        out[b] = ((1 - fy) * (1 - fx) * _tap(v[b], y0, x0) + (1 - fy) * fx * _tap(v[b], y0, x0 + 1) +
                  fy * (1 - fx) * _tap(v[b], y0 + 1, x0) + fy * fx * _tap(v[b], y0 + 1, x0 + 1))
    return out


def _resize_axis(S: int, F: int):
    s = np.maximum((np.arange(F) + 0.5) * S / F - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, S - 1), s - i0


def resize_fp64(img, F: int) -> np.ndarray:
    """interpolate(bilinear, align_corners=False), no antialiasing: [B, C, H, W] -> [B, C, F, F]."""
    i0, i1, ly = _resize_axis(img.shape[2], F)
    j0, j1, lx = _resize_axis(img.shape[3], F)
    ly, lx = ly[:, None], lx[None, :]
    g = lambda i, j: img[:, :, i[:, None], j[None, :]]
    return (1 - ly) * (1 - lx) * g(i0, j0) + (1 - ly) * lx * g(i0, j1) + ly * (1 - lx) * g(i1, j0) + ly * lx * g(i1, j1)


def frame_prep_fp64(src, F: int, matrix_inv=None, warp_size: int = 0, flip=None, gray: bool = False) -> np.ndarray:
    """The pixel rule of eg_frame_prep in fp64: src [B, C, Hs, Ws] uint8 / float32 -> [B, C_out, F, F]."""
    v = source_values(src)
    if warp_size > 0:
        v = warp_fp64(v, matrix_inv, warp_size)
    out = resize_fp64(v, F)
    if gray:
        out = (GRAY[0] * out[:, 0] + GRAY[1] * out[:, 1] + GRAY[2] * out[:, 2])[:, None]
    if flip is not None:
        out = out.copy()
        for b in np.flatnonzero(np.asarray(flip)):
            out[b] = out[b][..., ::-1]
    return out


def torch_composition(src, F: int, matrix_inv=None, warp_size: int = 0, flip=None, gray: bool = False, dtype=torch.float32,
                      device="cpu") -> torch.Tensor:
    """The same stages as torch operators in `dtype`, the way the reference's transform_image drives them (the identity
    affine_grid, its two columns swapped to (h, w), the matrix applied with bmm, swapped back, grid_sample(bilinear, zeros,
    align_corners=False)), then interpolate(bilinear, align_corners=False), gray and flip -> [B, C_out, F, F]."""
    x = torch.as_tensor(np.asarray(src)).to(device)
    x = x.to(dtype) / 255 if x.dtype == torch.uint8 else x.to(dtype)
    B = x.shape[0]
    if warp_size > 0:
        W = int(warp_size)
        m = torch.as_tensor(np.asarray(matrix_inv)).to(device=device, dtype=dtype)
        eye = torch.tensor([[[1, 0, 0], [0, 1, 0]]], dtype=dtype, device=device).expand(B, 2, 3)
        grid = torch.nn.functional.affine_grid(eye, [B, 1, W, W], align_corners=False).reshape(B, W * W, 2)
        grid = grid[..., [1, 0]]
        grid = grid.bmm(m[:, :, :2].transpose(1, 2)) + m[:, :, 2].unsqueeze(1)
        grid = grid[..., [1, 0]].reshape(B, W, W, 2)
        x = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    x = torch.nn.functional.interpolate(x, size=(F, F), mode="bilinear", align_corners=False)
    if gray:
        x = (GRAY[0] * x[:, 0] + GRAY[1] * x[:, 1] + GRAY[2] * x[:, 2]).unsqueeze(1)
    if flip is not None:
        f = torch.as_tensor(np.asarray(flip)).to(device).bool().view(B, 1, 1, 1)
        x = torch.where(f, x.flip(-1), x)
    return x


def landmark_q_fp64(coords, frame_size: int, matrix, crop_size: int, warp_size: int) -> np.ndarray:
    """q of the landmark rule before truncation, fp64 [B, 4, 2] (tests discard landmarks whose q is within 2**-10 of an integer)."""
    c = np.asarray(coords, dtype=np.float64).reshape(-1, 4, 2)
    m = np.asarray(matrix, dtype=np.float64).reshape(-1, 2, 3)
    n = c * 2.0 / crop_size - 1.0
    t = np.einsum("bij,bkj->bki", m[:, :, :2], n) + m[:, None, :, 2]
    return (t + 1.0) * warp_size / 2.0 * frame_size / warp_size
