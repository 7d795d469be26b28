"""The restatement of eg_heatmap_render (tests/heatmap_render_reference.py), checked without a GPU: every input builder of
tests/test_gpu_heatmap_render.py against the condition it was built for (a case that misses its condition, or whose float32
restatement alone is excused on more than 1 % of its bytes, fails here and not silently on the GPU), float32 against float64
under the rules the GPU test applies to the kernel, and the identity the kernel rests on: p / max p is exp(x - M)."""
import numpy as np
import pytest
import torch

import heatmap_render_reference as R

F64, F32 = torch.float64, torch.float32


def _float32_under_the_gpu_rules(c, cap=R.CAP):
    r64, r32 = c["r64"], c["r32"]
    rep = R.Report()
    rep.check("heat", r32["heat"], r64["heat"], r32["heat"], R.heat_scale(r64))
    rep.check("e", r32["e"], r64["e"], r32["e"], R.weight_scale(r64["e"], r64["xm"]))
    assert not rep.failed(), rep.failed()
    # no transcendental: float32 and float64 disagree only where 0.8f * image * 255 rounds across an integer -- the base candidate's edge
    for name in ("base", "gt"):
        diff = (r32[name].to(torch.int64) - r64[name].to(torch.int64)).abs()
        assert int(diff.max()) <= 1 and int((diff > 0).sum()) <= cap * diff.numel(), name
    bad, excused, total = R.pred_bytes_rule(r32["pred"], r64, r32)
    assert bad == 0 and excused <= cap * total, (bad, excused, total)
    return excused, total


def _identity(c):
    """The reference forms p / max p per channel (evaluators.py:511); the kernel takes exp(x - M)."""
    r64, r32 = c["r64"], c["r32"]
    rep = R.Report()
    for name, r in (("fp64 quotient", r64), ("fp32 quotient", r32)):
        p = r["heat"]
        top = p.amax(dim=(1, 2), keepdim=True)
        q = torch.where(top > 0, p / top, torch.zeros_like(p))              # (an empty channel: 0 / 0 in the reference, 0 here)
        rep.check(name, q, r64["e"], r32["e"], R.weight_scale(r64["e"], r64["xm"]))
    assert not rep.failed(), rep.failed()
    assert float(r64["e"].amax()) == 1.0 and ((r64["e"].amax(dim=(1, 2)) == 1) | (r64["e"].amax(dim=(1, 2)) == 0)).all()


def test_the_cases_cover_every_factor_and_every_pair():
    R._assert_design()
    assert len(R.COMBOS) == 8 and len(R.CASES) == 48 and {c[0] for c in R.CASES} == set(R.SIDES) == set(R.WHAT)
    assert set(R.OUTPUT_SETS[-1]) == {s[0] for s in R.OUTPUT_SETS[:-1]}


@pytest.mark.parametrize("key", R.CASES, ids=lambda k: "side{}-count{}-first{}-start{}-behind{}-ch{}".format(*k))
def test_builder_and_float32_restatement(key):
    c = R.case(*key)
    side, count = key[0], key[1]
    assert c["r64"]["heat"].shape == (count, side, side, 4) and c["r64"]["pred"].shape == (count, side, side, 3)
    assert c["r64"]["pred"].dtype == torch.uint8 and c["r32"]["heat"].dtype == F32
    _float32_under_the_gpu_rules(c)
    _identity(c)
    # the -inf channel is 0 everywhere and draws nothing; the softmax of every other channel sums to 1
    assert c["r64"]["heat"][..., 2].eq(0).all() and c["r64"]["e"][..., 2].eq(0).all()
    s = c["r64"]["heat"].sum(dim=(1, 2))
    assert (s[:, [0, 1, 3]] - 1).abs().max() < 1e-12
    # saturation and the floor at 0: the base image holds 255 where the frame is above 1.25 and 0 where it is below 0
    img = torch.from_numpy(c["image"][key[2]:key[2] + count, 0])
    assert c["r64"]["base"][img > 1.25].eq(255).all() and c["r64"]["base"][img < 0].eq(0).all()


def test_exact_case_allows_no_excused_byte():
    c = R.exact_case()
    for name in ("pred", "gt", "base"):
        assert torch.equal(c["r32"][name], c["r64"][name])
    bad, excused, _ = R.pred_bytes_rule(c["r32"]["pred"], c["r64"], c["r32"])
    assert bad == 0 and excused == 0
    _identity(c)
    assert torch.equal(c["r32"]["e"].to(F64), c["r64"]["e"])


def test_full_size_case():
    c = R.full_case()
    excused, total = _float32_under_the_gpu_rules(c)
    assert total == 2 * 224 * 224 * 3
    _identity(c)


def test_bytes_saturate_truncate_and_drop_nan():
    v = torch.tensor([-1.0, -0.0, 0.0, 0.5 / 255, 1.001 / 255, 127.999 / 255, 1.0, 1.5, float("inf"), float("nan")], dtype=F64)
    assert R.to_bytes(v).tolist() == [0, 0, 0, 0, 1, 127, 255, 255, 255, 0]
    assert R.to_bytes(v.to(F32)).dtype == torch.uint8
    # the constants are the float constants in both types
    assert float(R._f(0.7, F64)) == float(np.float32(0.7)) != 0.7
