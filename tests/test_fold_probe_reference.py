"""CPU: tests/fold_probe_reference.py, the reference of tests/test_gpu_fold_probe.py -- and the place where that test's bound
BOUND_C is fixed and kept honest.  For every operand family, at the GPU test's own handles, batches and seeds (the aggregated rows of
the `_agg` families are A_hat x in float32 here: natural pieces, as the kernel's are), with ratios in units of S = |a||w|^T per
element:

    fp32 evaluation, three summation orders (k ascending, the kernel's k order, torch.matmul)     <= BOUND_C / 8     (maximum)
    the six-product emulation                                                                     <= BOUND_C / 4     (maximum)
    the emulation without the family's target product                                              > 4 BOUND_C       (MINIMUM: every element)
    the emulation without any other product              changes nothing (<= BOUND_C / 4) or is itself > 4 BOUND_C at every element

so that a family's verdict names products, not noise.  mm_raw and mm_agg also fail on W mid . a hi, the first-order half of what
survives there (about 2e-3 S): a kernel that loses that one fails them too, which is as it should be.  Every figure is printed."""
import numpy as np
import pytest
import torch

import eval_reference as E
import fold_probe_reference as P
from echoglad_amd.ops.infer import fold_lo_index, split3_planes

F64, F32 = torch.float64, torch.float32
# the handles of tests/test_gpu_fold_probe.py: (frame, naux, main_only, coord, conn, diag_main, diag_aux), batch
HANDLES = [((16, 3, False, False, False, False, False), 2), ((16, 3, False, False, False, True, True), 2),
           ((64, 5, False, False, True, False, False), 1), ((64, 6, False, False, False, False, False), 8)]


def _operands(family, handle, B):
    """(operand rows a as float32, float64 rows, weight, target) of a family at a handle."""
    n = E.topology(*handle).num_nodes
    x, w, target = P.FAMILIES[family](B * n, P.SEEDS[family])
    if family in P.AGG:
        Eg = E.topo_edges(*handle)
        return E.ahat(Eg, x, B), E.ahat(Eg, x.to(F64), B), w, target
    return x, x.to(F64), w, target


def test_head_keys_and_split_are_the_librarys():
    assert P.HEAD_KEYS == E.HEAD_KEYS
    packed = P.probe_heads(5)
    assert set(packed) == set(E.HEAD_KEYS) and all(bool(torch.isfinite(v).all()) for v in packed.values())
    rs = np.random.RandomState(1)
    bits = rs.randint(0, 2 ** 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    t = torch.from_numpy(bits.view(np.float32).copy())
    t = torch.cat([t[torch.isfinite(t)], P.bits16(rs, (64, 64)).reshape(-1), P.bits24(rs, (64, 64)).reshape(-1)])
    for mine, theirs in zip(P.split3(t), split3_planes(t)):
        assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32))


def test_probe_heads_hand_one_column_through_bit_for_bit():
    """The unfolded tail of eval_reference.heads_eval in float32 on the probe parameters: relu(u[:, 32 h + j]) exactly."""
    u = E.rand_rows(50, seed=3) * 7.0
    for j in (0, 13, 31):
        packed = P.probe_heads(j)
        h = torch.relu(u).view(-1, 4, 32)
        z = torch.einsum("nhk,hok->nho", h, packed["w2"])
        z = torch.relu(packed["s2"].view(4, 16) * z + packed["t2"].view(4, 16))
        y = (z * packed["w3"]).sum(-1) + packed["b3"]
        assert torch.equal(y, torch.relu(u).view(-1, 4, 32)[:, :, j])


def test_engineered_values_split_into_the_pieces_the_table_claims():
    rs = np.random.RandomState(4)
    ulp = lambda t: torch.ldexp(torch.ones_like(t), torch.frexp(t)[1] - 24)      # the last of a value's 24 bits
    v = P.bits8(rs, (200, 64))
    hi, mid, lo = P.split3(v)
    assert torch.equal(hi, v) and not mid.any() and not lo.any()
    v = P.bits16(rs, (200, 64))
    hi, mid, lo = P.split3(v)
    assert torch.equal(hi + mid, v) and not lo.any()
    assert torch.equal(mid, 0xFF00 * ulp(v))                                     # eight ones right behind hi's bits
    v = P.bits24(rs, (200, 64))
    hi, mid, lo = P.split3(v)
    assert torch.equal((hi + mid) + lo, v)
    assert torch.equal(lo, 0xFF * ulp(v))                                        # the low byte, all ones
    assert bool((mid >= 0x8000 * ulp(v)).all()) and bool((mid < 0x10000 * ulp(v)).all())      # exactly the second byte
    for gen in (P.bits8, P.bits16, P.bits24, P.positive):
        v = gen(rs, (200, 64))
        assert bool((v >= 0.125).all()) and bool((v < 4.0).all())


def test_pair_partners_share_a_lane_group_and_a_k_step():
    """k and k + 1 (k even) sit in the same (kq, step) group of the kernel's operand layout, so the pair cancels inside one MFMA's
    lane; and the order fp32_orders calls the kernel's is fold_lo_index's."""
    _, k = fold_lo_index()                                   # [step, wave, cb, kq, i, e]
    k = k[:, 0, 0, :, 0, :]                                  # [step, kq, e]
    group = {int(k[s, q, e]): (s, q) for s in range(4) for q in range(4) for e in range(8)}
    assert sorted(group) == list(range(128))
    assert all(group[kk] == group[kk + 1] for kk in range(0, 128, 2))
    assert P.kernel_k_order() == [int(v) for v in k.reshape(-1)]


@pytest.mark.parametrize("family", list(P.FAMILIES))
def test_partners_take_back_everything_but_the_products_under_test(family):
    """In exact arithmetic a w^T of a family equals the sum of the surviving piece products of its even k alone."""
    x, w, target = P.FAMILIES[family](40, P.SEEDS[family])
    assert bool((x > 0).all()) and bool((w[:, 0::2] > 0).all()) and bool((w[:, 1::2] < 0).all())
    assert torch.equal(x[:, 0::2], x[:, 1::2]) or family == "hl_raw"
    a64, w64 = x.to(F64), w.to(F64)
    ae, we = (dict(zip(("hi", "mid", "lo"), (p.to(F64) for p in P.split3(t[:, 0::2].contiguous())))) for t in (x, w))
    whole = lambda d: d["hi"] + d["mid"] + d["lo"]
    left = {"mm_raw": whole(ae) @ we["mid"].T, "hl_raw": ae["lo"] @ we["hi"].T, "lh_raw": ae["hi"] @ we["lo"].T,
            "mm_agg": whole(ae) @ we["mid"].T, "lh_agg": whole(ae) @ we["lo"].T}[family]
    # (float64 holds every product here exactly -- at most 48 bits -- and the sums to 2^-53 of their largest partial sum)
    assert float(((a64 @ w64.T) - left).abs().max()) <= 2.0 ** -40
    assert bool((left > 0).all())


@pytest.mark.parametrize("handle,B", HANDLES, ids=str)
@pytest.mark.parametrize("family", list(P.FAMILIES))
def test_bound_separates_rounding_from_a_lost_product(family, handle, B, capsys):
    c = P.BOUND_C
    assert np.log2(c) == round(np.log2(c))
    a, a64, w, target = _operands(family, handle, B)
    u64 = a64 @ w.to(F64).T
    S = P.scale(a64, w)
    assert bool((u64 > 0).all())                             # the probe's ReLU changes nothing
    noise = {name: float(P.per_term(v, u64, S).max()) for name, v in P.fp32_orders(a, w).items()}
    pp = P.piece_products(a, w)
    six = float(P.per_term(P.emulate(a, w, products=pp), u64, S).max())
    lost = {name: P.per_term(P.emulate(a, w, drop=(name,), products=pp), u64, S) for name in P.PRODUCTS}
    with capsys.disabled():
        print(f"\n{family} {handle} B={B}: fp32 / S  " + "  ".join(f"{k} {v:.2e}" for k, v in noise.items())
              + f";  six products {six:.2e};  without {target}: min {float(lost[target].min()):.2e} median "
              f"{float(lost[target].median()):.2e};  c = 2^{int(np.log2(c))} = {c:.2e}")
        print("    without " + "  ".join(f"{k}: {float(v.min()):.2e} .. {float(v.max()):.2e}" for k, v in lost.items() if k != target))
    assert max(noise.values()) <= c / 8, noise
    assert six <= c / 4
    assert float(lost[target].min()) > 4 * c
    for name, r in lost.items():
        if name != target:
            assert float(r.max()) <= c / 4 or float(r.min()) > 4 * c, (name, float(r.min()), float(r.max()))
    if family.startswith("mm"):
        assert float(lost["mid.hi"].min()) > 1e-3            # the first-order half of what survives


def test_mixed_case_names_both_targets(capsys):
    """mm_raw on w1s and lh_agg on m1 over the same rows, the GPU test's one launch with both halves: the same conditions on the sum
    (S is the sum of both halves' scales, so each target weighs about half of what it does alone)."""
    c = P.BOUND_C
    handle, B = HANDLES[0]
    Eg, n = E.topo_edges(*handle), E.topology(*handle).num_nodes
    x, m1, w1s, targets = P.mixed(B * n)
    assert torch.equal(x[:, 0::2], x[:, 1::2])
    a, a64, x64 = E.ahat(Eg, x, B), E.ahat(Eg, x.to(F64), B), x.to(F64)
    u64 = a64 @ m1.to(F64).T + x64 @ w1s.to(F64).T
    S = P.scale(a64, m1) + P.scale(x64, w1s)
    oa, ox = P.fp32_orders(a, m1), P.fp32_orders(x, w1s)
    noise = {name: float(P.per_term(oa[name] + ox[name], u64, S).max()) for name in oa}
    pa, px = P.piece_products(a, m1), P.piece_products(x, w1s)
    both = lambda drop=(): P.emulate(a, m1, drop, pa) + P.emulate(x, w1s, drop, px)
    six = float(P.per_term(both(), u64, S).max())
    lost = {name: P.per_term(both((name,)), u64, S) for name in P.PRODUCTS}
    with capsys.disabled():
        print(f"\nmixed {handle} B={B}: fp32 / S  " + "  ".join(f"{k} {v:.2e}" for k, v in noise.items()) + f";  six products {six:.2e};  "
              + ";  ".join(f"without {t}: min {float(lost[t].min()):.2e}" for t in targets) + f";  c = {c:.2e}")
    assert max(noise.values()) <= c / 8 and six <= c / 4
    for name, r in lost.items():
        if name in targets:
            assert float(r.min()) > 4 * c, (name, float(r.min()))
        else:
            assert float(r.max()) <= c / 4 or float(r.min()) > 4 * c, (name, float(r.min()), float(r.max()))
