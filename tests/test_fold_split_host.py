"""No GPU: the bf16 bodies of the folded last layer + heads (csrc/gcn_layer_ps_fold_split.hip) as built -- the 16x16x32 instruction,
no packed fp32 vector instruction, no scratch; the counts tests/test_split_no_packed.py pins, on the library with the new object in
it; the host side of the split (ops.split3_planes: hi + mid + lo == w bit for bit, the way tests/native/split3_check.cpp checks the
device function) and the layout of the streamed lo-plane table (ops.fold_lo_table / fold_lo_index)."""
import re

import numpy as np
import torch

from echoglad_amd import build
from echoglad_amd.ops.infer import fold_lo_index, fold_lo_table, split3_planes


def test_fold_split_object_holds_16x16x32_mfmas_no_packed_fp32_and_no_scratch():
    build.build()
    n_mfma, n_packed, n_scratch = build.fold_split_census(build.LIBDIR / "obj" / "gcn_layer_ps_fold_split.o")
    # four bodies: 32 units x 12 with the residual, 16 x 12 without, plain and 'grid-diagonal'
    assert n_mfma == 2 * 384 + 2 * 192 and n_packed == 0 and n_scratch == 0, (n_mfma, n_packed, n_scratch)


def test_the_32x32x16_counts_of_the_split_layer_still_hold():
    lib = build.build()
    n_mfma, n_packed = build.packed_fp32_census(build.LIBDIR / "obj" / "gcn_layer_ps_split.o")
    assert n_mfma == 2 * 96 and n_packed == 0
    kernels = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", build.device_disassembly(lib))
    assert sum(1 for k in kernels if re.search(r"\bv_mfma_f32_32x32x16_bf16\b", k)) == 2
    mixed = [k.split("\n", 1)[0] for k in kernels if re.search(r"\bv_mfma_f32_16x16x32_bf16\b", k) and re.search(r"\bv_pk_\w+_f32\b", k)]
    assert not mixed, mixed
    assert sum(1 for k in kernels if re.search(r"\bv_mfma_f32_16x16x32_bf16\b", k)) == 4


def _patterns():
    rs = np.random.RandomState(1)
    rand = rs.randint(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    # every exponent with a few significands, both signs
    exps = np.arange(0, 255, dtype=np.uint32)[:, None] << 23
    sig = np.array([0, 1, 0x7FFFFF, 0x400001, 0x00FF00, 0x0100FF, 0x7F807F, 0x123456], dtype=np.uint32)[None, :]
    grid = (exps | sig).reshape(-1)
    bits = np.concatenate([rand, grid, grid | np.uint32(0x80000000)])
    w = torch.from_numpy(bits.view(np.float32).copy())
    return w[torch.isfinite(w)]


def test_host_split_is_exact_for_random_patterns_and_every_exponent():
    w = _patterns()
    hi, mid, lo = split3_planes(w)
    for p in (hi, mid, lo):
        assert int((p.view(torch.int32) & 0xFFFF).abs().max()) == 0            # one bf16 value each
    exact = w.abs() >= 2.0 ** -110                                             # (tile.h split3: below, within 2^-133)
    total = (hi + mid) + lo                                                    # both sums are exact: 16 and 24 significant bits
    assert torch.equal(total[exact].view(torch.int32), w[exact].view(torch.int32))
    assert float((total[~exact].double() - w[~exact].double()).abs().max()) < 2.0 ** -133
    same_sign = lambda p: bool(((p == 0) | (torch.signbit(p) == torch.signbit(w))).all())
    assert same_sign(hi) and same_sign(mid) and same_sign(lo)


def test_lo_table_layout_round_trips():
    rs = np.random.RandomState(2)
    m1, w1s = (torch.from_numpy(rs.standard_normal((128, 128)).astype(np.float32)) for _ in range(2))
    table = fold_lo_table(m1, w1s)
    assert table.shape == (2, 4, 4, 2, 4, 16, 8) and table.dtype == torch.int16 and table.is_contiguous()
    assert table.numel() * table.element_size() == 64 * 1024
    ch, k = fold_lo_index()
    flat = (ch * 128 + k).reshape(-1)
    assert torch.equal(flat.sort().values, torch.arange(128 * 128))           # every element of a matrix exactly once
    # lane (kq, i) of wave wv, step s, column block cb, element e  <-  W[32 wv + 16 cb + i][koff(kq) + 8 s + e]
    assert (int(ch[1, 2, 1, 3, 5, 7]), int(k[1, 2, 1, 3, 5, 7])) == (32 * 2 + 16 + 5, 96 + 8 + 7)
    assert (int(ch[3, 0, 0, 1, 15, 0]), int(k[3, 0, 0, 1, 15, 0])) == (15, 64 + 24)
    for m, w in enumerate((m1, w1s)):
        lo = split3_planes(w)[2]
        back = torch.zeros(128, 128, dtype=torch.int32)
        back[ch, k] = table[m].to(torch.int32) << 16
        assert torch.equal(back, lo.view(torch.int32))
