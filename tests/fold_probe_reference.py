"""What tests/test_gpu_fold_probe.py needs to see ONE product of the folded last layer + heads (k_gcn_layer_ps FOLD / FSPLIT): torch
and numpy on the CPU, no import of the library.

The kernel never writes its first pre-activation u = (A_hat x) m1^T + x w1s^T + c1: four logits per row come out, behind two ReLUs
and two more layers.  Two devices make it observable, per element and per piece product.

1. Probe heads (probe_heads).  The heads' tail is fp32 in both bodies.  With w2[h, 0, j] = 1, w3[h, 0] = 1, s2 = 1, every other
   entry 0, no sigmoid, every product of the tail is by 1 or by 0 and every sum adds zeros: logit[r, h] = relu(u[r, 32 h + j]) bit
   for bit.  32 launches show all 128 columns; a launch with (-m1, -w1s, -c1) shows relu(-u) -- split3 is sign-symmetric.

2. Cancellation pairs (the operand families).  For random operands the second-order piece products have random signs, and a lost
   one costs about 2^-18 / sqrt(K) of S = sum_k |a_k||w_k|: inside fp32 rounding.  Here every value is positive, so those terms add
   up, and everything else cancels exactly: even k carries an engineered pair (a, w), k + 1 -- the same lane group and k-step of the
   kernel (ops.fold_lo_index) -- a partner that takes back all but the products under test.

       family   even k                                           odd k                                  what survives
       mm_raw   a, w: 8 random bits, 8 ones, 8 zeros              a' = a, w' = -hi(w)                    W mid . (a hi + a mid)
       hl_raw   w bf16-exact, a 24 bits with the low 8 set        a' = hi(a) + mid(a), w' = -w           W hi . a lo
       lh_raw   a bf16-exact, w 24 bits with the low 8 set        a' = a, w' = -(hi(w) + mid(w))         W lo . a hi
       mm_agg   x[:, k] positive, w as in mm_raw                  x[:, k + 1] = x[:, k], w' = -hi(w)     W mid . a     (target mid . mid)
       lh_agg   x[:, k] positive, w 24 bits with the low 8 set    the same, w' = -(hi(w) + mid(w))       W lo . a      (target lo . hi)

   `_raw` families drive w1s (the raw rows are the kernel's operand as they stand), `_agg` families m1: the aggregated rows are what
   the kernel computes in fp32 from x, so their pieces are natural -- a duplicated channel of x is a duplicated channel of A_hat x,
   bit for bit, and that is all the cancellation needs.  (W hi . a lo on aggregated rows has no pair for that reason: the identity
   case of the GPU test pins it.)

emulate() is the model of a kernel that has lost a product: the six products of tile.h fs_step in float64, any subset left out.
BOUND_C, the per-term bound of the GPU test, is fixed by tests/test_fold_probe_reference.py from these CPU evaluations alone."""
import numpy as np
import torch

C = 128
F64, F32 = torch.float64, torch.float32
HEAD_KEYS = ("w1", "s1", "t1", "w2", "s2", "t2", "w3", "b3")        # eval_reference.HEAD_KEYS (asserted equal by the CPU test)
KOFF = (0, 64, 32, 96)                                               # tile.h koff16: the k quarter lane group kq reads
# the six products of fs_step in its order, "W piece.a piece"
PRODUCTS = ("lo.hi", "hi.lo", "mid.mid", "mid.hi", "hi.mid", "hi.hi")
# |got - u64| <= BOUND_C * S per element.  One power of two for every family, from the CPU runs of tests/test_fold_probe_reference.py
# (fp32 in three summation orders stays below BOUND_C / 8, the six-product emulation below BOUND_C / 4, the emulation without the
# target product is above 4 BOUND_C at EVERY element: 2^-22 is the smallest power of two that meets all three, 2^-23 fails the first);
# nothing a kernel returned went into it.
BOUND_C = 2.0 ** -22


def probe_heads(j):
    """The packed head parameters that hand relu(u[:, 32 h + j]) through as logit h.  The folded route does not read w1 / s1 / t1."""
    w2 = torch.zeros(4, 16, 32)
    w2[:, 0, j] = 1.0
    w3 = torch.zeros(4, 16)
    w3[:, 0] = 1.0
    return {"w1": torch.zeros(C, C), "s1": torch.ones(C), "t1": torch.zeros(C), "w2": w2, "s2": torch.ones(64), "t2": torch.zeros(64),
            "w3": w3, "b3": torch.zeros(4)}


def _top16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(F32)


def split3(t):
    """tile.h split3 / ops.split3_planes: float32 hi, mid, lo with zero low halves, hi + mid + lo == t bit for bit."""
    t = t.detach().to(F32)
    hi = _top16(t)
    r = t - hi
    mid = _top16(r)
    return hi, mid, _top16(r - mid)


def piece_products(a, w):
    """{name of PRODUCTS: (a piece) (W piece)^T in float64}: a [rows, K], w [cols, K]."""
    pa = dict(zip(("hi", "mid", "lo"), (p.to(F64) for p in split3(a))))
    pw = dict(zip(("hi", "mid", "lo"), (p.to(F64) for p in split3(w))))
    return {name: pa[name.split(".")[1]] @ pw[name.split(".")[0]].T for name in PRODUCTS}


def emulate(a, w, drop=(), products=None):
    """sum over PRODUCTS not in `drop` of (a piece) (W piece)^T, every product and the sum in float64 (products: what
    piece_products(a, w) returned, for several calls on the same operands)."""
    assert all(name in PRODUCTS for name in drop), drop
    products = piece_products(a, w) if products is None else products
    return sum(products[name] for name in PRODUCTS if name not in drop)


def kernel_k_order():
    """k in the order the split body accumulates: k-step, lane group kq (koff 0, 64, 32, 96), element."""
    return [KOFF[kq] + 8 * s + e for s in range(4) for kq in range(4) for e in range(8)]


def fp32_sum(a, w, order):
    """sum_k a[:, k] w[:, k]^T in float32, one k at a time in `order` (product rounded, then added)."""
    an, wn = a.numpy(), w.numpy()
    acc = np.zeros((an.shape[0], wn.shape[0]), dtype=np.float32)
    term = np.empty_like(acc)
    for k in order:
        np.multiply(an[:, k, None], wn[None, :, k], out=term)
        acc += term
    return torch.from_numpy(acc)


def fp32_orders(a, w):
    """{name: float32 a w^T} in three summation orders: k ascending, the kernel's k order, torch.matmul."""
    return {"k ascending": fp32_sum(a, w, range(a.shape[1])), "kernel order": fp32_sum(a, w, kernel_k_order()), "matmul": a @ w.T}


def scale(a64, w, c1=None):
    """S = |a64| |w|^T (+ |c1|), float64, per element."""
    s = a64.to(F64).abs() @ w.to(F64).abs().T
    return s if c1 is None else s + c1.to(F64).abs()


def per_term(got, u64, S):
    """|got - u64| / S per element."""
    return (got.detach().cpu().to(F64) - u64).abs() / S


# ---------------------------------------------------------------------------
# engineered values: positive, exponents 2^-3 .. 2^1
# ---------------------------------------------------------------------------
def _floats(rs, shape, mant):
    e = rs.randint(-3, 2, shape).astype(np.int64)
    bits = ((e + 127) << 23) | mant.astype(np.int64)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).reshape(shape).copy())


def bits8(rs, shape):
    """bf16-exact: the 8 leading significand bits random, nothing below."""
    return _floats(rs, shape, rs.randint(0, 128, shape) << 16)


def bits16(rs, shape):
    """8 random bits, the next 8 all ones, the low 8 zero: hi + mid with the largest mid there is, lo = 0."""
    return _floats(rs, shape, (rs.randint(0, 128, shape) << 16) | 0xFF00)


def bits24(rs, shape):
    """All 24 bits: 8 random, then a one and 7 random (so that mid is exactly the second byte), the low 8 all ones."""
    return _floats(rs, shape, (rs.randint(0, 128, shape) << 16) | 0x8000 | (rs.randint(0, 128, shape) << 8) | 0xFF)


def positive(rs, shape):
    """Any positive fp32 in the same range of exponents."""
    return _floats(rs, shape, rs.randint(0, 1 << 23, shape))


def _paired(even, odd):
    out = torch.empty(even.shape[0], 2 * even.shape[1])
    out[:, 0::2], out[:, 1::2] = even, odd
    return out.contiguous()


def mm_raw(rows, seed):
    rs = np.random.RandomState(seed)
    a, w = bits16(rs, (rows, C // 2)), bits16(rs, (C, C // 2))
    return _paired(a, a), _paired(w, -split3(w)[0]), "mid.mid"


def hl_raw(rows, seed):
    rs = np.random.RandomState(seed)
    a, w = bits24(rs, (rows, C // 2)), bits8(rs, (C, C // 2))
    hi, mid, _ = split3(a)
    return _paired(a, hi + mid), _paired(w, -w), "hi.lo"


def lh_raw(rows, seed):
    rs = np.random.RandomState(seed)
    a, w = bits8(rs, (rows, C // 2)), bits24(rs, (C, C // 2))
    hi, mid, _ = split3(w)
    return _paired(a, a), _paired(w, -(hi + mid)), "lo.hi"


def mm_agg(rows, seed):
    rs = np.random.RandomState(seed)
    x, w = positive(rs, (rows, C // 2)), bits16(rs, (C, C // 2))
    return _paired(x, x), _paired(w, -split3(w)[0]), "mid.mid"


def lh_agg(rows, seed):
    rs = np.random.RandomState(seed)
    x, w = positive(rs, (rows, C // 2)), bits24(rs, (C, C // 2))
    hi, mid, _ = split3(w)
    return _paired(x, x), _paired(w, -(hi + mid)), "lo.hi"


def mixed(rows):
    """A `_raw` and an `_agg` family in one launch (FOLD 1): mm_raw's rows and w1s, lh_agg's m1 -- mm_raw's partner rows are
    duplicates, which is all lh_agg asks of x -> (x, m1, w1s, the two targets)."""
    x, w1s, t_raw = mm_raw(rows, SEEDS["mm_raw"])
    _, m1, t_agg = lh_agg(rows, SEEDS["lh_agg"])
    return x, m1, w1s, (t_raw, t_agg)


RAW = {"mm_raw": mm_raw, "hl_raw": hl_raw, "lh_raw": lh_raw}          # -> (x = the operand rows, w1s, target)
AGG = {"mm_agg": mm_agg, "lh_agg": lh_agg}                            # -> (x, m1, target): the operand rows are A_hat x
FAMILIES = {**RAW, **AGG}
SEEDS = {"mm_raw": 31, "hl_raw": 32, "lh_raw": 33, "mm_agg": 34, "lh_agg": 35}
