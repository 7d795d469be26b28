"""No GPU: the fold of the last GCN layer into the heads' first Linear (nn/_heads.py fold_last_into_heads) against the float64
formula written out, and against the unfolded computation it replaces."""
import numpy as np
import torch

from echoglad_amd.nn._heads import fold_last_into_heads

C = 128


def _params(seed, w_scale=0.08):
    rs = np.random.RandomState(seed)
    f = lambda *shape: torch.from_numpy(rs.uniform(-0.3, 0.3, shape).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((C, C)) * w_scale).astype(np.float32))
    scale = torch.from_numpy((rs.standard_normal(C) * 0.1 + 1.0).astype(np.float32))
    shift = torch.from_numpy((rs.standard_normal(C) * 0.1).astype(np.float32))
    return w, scale, shift, f(C, C), f(C) + 1.0, f(C)


def _formula(w, scale, shift, w1, s1, t1):
    """m1, w1s, c1 in float64, entry by entry as the issue states them."""
    w, w1, s1, t1 = w.double(), w1.double(), s1.double(), t1.double()
    scale = torch.ones(C, dtype=torch.float64) if scale is None else scale.double()
    shift = torch.zeros(C, dtype=torch.float64) if shift is None else shift.double()
    m1 = torch.diag(s1) @ w1 @ torch.diag(scale) @ w
    w1s = torch.diag(s1) @ w1
    c1 = s1 * (w1 @ shift) + t1
    return m1, w1s, c1


def test_fold_equals_the_float64_formula_rounded_once():
    for seed in (0, 1):
        p = _params(seed)
        got = fold_last_into_heads(*p, True)
        want = _formula(*p)
        for g, w64, shape in zip(got, want, ((C, C), (C, C), (C,))):
            assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == shape
            # one rounding of the float64 value: at most half an ulp away, so the float32 nearest to it is the value itself.  (The
            # two float64 evaluations associate their sums differently: 1e-15 relative apart, which moves a rounding only if the
            # value sits within that of a tie -- allow the neighbouring float32 for such an entry, and count them.)
            near = w64.float()
            off = g != near
            assert int(off.sum()) <= 2
            assert float(((g.double() - w64).abs() / w64.abs().clamp_min(1e-30)).max()) <= 2.0 ** -24 * (1 + 1e-6)


def test_fold_reproduces_the_unfolded_heads_input():
    """u = s1 * (h3 w1^T) + t1 with h3 = scale * (a W^T) + shift + r x, against a m1^T + r x w1s^T + c1 from the folded tables."""
    rs = np.random.RandomState(7)
    a = torch.from_numpy(rs.standard_normal((257, C))).double()
    x = torch.from_numpy(rs.standard_normal((257, C))).double()
    w, scale, shift, w1, s1, t1 = _params(3)
    for r in (0, 1):
        m1, w1s, c1 = (t.double() for t in fold_last_into_heads(w, scale, shift, w1, s1, t1, bool(r)))
        h3 = scale.double() * (a @ w.double().T) + shift.double() + r * x
        want = s1.double() * (h3 @ w1.double().T) + t1.double()
        got = a @ m1.T + r * (x @ w1s.T) + c1
        # float32 tables: 2^-24 relative per entry, 128 + 128 + 1 terms of size <= max|want| each
        assert float((got - want).abs().max()) < 257 * 2.0 ** -24 * float(want.abs().max())


def test_scale_and_shift_of_none_mean_one_and_zero():
    w, scale, shift, w1, s1, t1 = _params(4)
    one, zero = torch.ones(C), torch.zeros(C)
    for sc, sh in ((None, None), (scale, None), (None, shift)):
        got = fold_last_into_heads(w, sc, sh, w1, s1, t1, True)
        want = fold_last_into_heads(w, one if sc is None else sc, zero if sh is None else sh, w1, s1, t1, True)
        for g, e in zip(got, want):
            assert torch.equal(g, e)
    assert torch.equal(fold_last_into_heads(w, None, None, w1, s1, t1, True)[2], t1)          # c1 = t1 without a shift


def test_the_tables_do_not_depend_on_the_residual_flag():
    """r multiplies the input inside the kernel: m1 (and w1s, c1) of r = 0 are those of r = 1."""
    p = _params(5)
    with_res, without = fold_last_into_heads(*p, True), fold_last_into_heads(*p, False)
    for g, e in zip(with_res, without):
        assert torch.equal(g, e)
