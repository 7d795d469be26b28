"""CPU: host-side logic that needs no GPU -- the stacked layout the heads' parameters live in and the packed gradients come back
in, the hand-down of the BatchNorm-backward sums through the per-layer boxes, the optimizer's argument checks."""
import pytest
import torch

from echoglad_amd import nn as egnn


def test_head_parameter_bank_layout_tiles_the_flat_buffer():
    offs = egnn._head_param_offsets()
    sizes = [egnn._HEAD_SIZES[j] for _ in range(4) for j in range(10)]            # params[10 * k + j] has size _HEAD_SIZES[j]
    spans = sorted((o, o + n) for o, n in zip(offs, sizes))
    assert spans[0][0] == 0 and spans[-1][1] == 4 * sum(egnn._HEAD_SIZES)
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))                   # no gap, no overlap
    # the 4 heads' slices of one array are consecutive: the stacked array the kernels take is ONE slice of the bank
    for j in range(10):
        assert [offs[10 * k + j] for k in range(4)] == [offs[j] + k * egnn._HEAD_SIZES[j] for k in range(4)]


def test_move_into_and_views_of():
    ts = [torch.arange(6.0).view(2, 3), torch.arange(4.0) + 10, torch.tensor([7.0])]
    offs, bank, moved = [0, 6, 10], torch.empty(11), {}
    assert not egnn._views_of(bank, ts, offs)
    egnn._move_into(bank, ts, offs, lambda i, v: moved.__setitem__(i, v))
    views = [moved[i] for i in range(3)]
    assert egnn._views_of(bank, views, offs)
    for t, v in zip(ts, views):
        assert v.shape == t.shape and torch.equal(v, t)
    assert torch.equal(bank, torch.cat([t.reshape(-1) for t in ts]))
    views[1] = views[1].clone()                                                  # somebody re-allocated one of them
    assert not egnn._views_of(bank, views, offs)
    assert not egnn._views_of(bank, [v.double() for v in moved.values()], offs)  # wrong dtype


# first element of parameter (head k, array j) = params[10 * k + j] in eg_classifier_bwd's packed gradients (include/echoglad_hip.h:
# dw1 [4,32,128], db1, dgamma1, dbeta1 [4,32], dw2 [4,16,32], db2, dgamma2, dbeta2 [4,16], dw3 [4,16], db3 [4]), as the hand-written
# slices of the function that preceded the table-driven one returned them
_PACKED_HEAD_GRAD_STARTS = (
    0, 16384, 16512, 16640, 16768, 18816, 18880, 18944, 19008, 19072,
    4096, 16416, 16544, 16672, 17280, 18832, 18896, 18960, 19024, 19073,
    8192, 16448, 16576, 16704, 17792, 18848, 18912, 18976, 19040, 19074,
    12288, 16480, 16608, 16736, 18304, 18864, 18928, 18992, 19056, 19075)
_HEAD_GRAD_SHAPES = ((32, 128), (32,), (32,), (32,), (16, 32), (16,), (16,), (16,), (1, 16), (1,))
_PACKED_MLP_GRAD_STARTS = (0, 4352, 4384, 4416, 4448, 4960, 4976, 4992, 5008, 5040)
_MLP_GRAD_SHAPES = ((32, 136), (32,), (32,), (32,), (16, 32), (16,), (16,), (16,), (2, 16), (2,))


def test_unstacked_gradients_are_the_packed_buffers_slices():
    ramp = torch.arange(19076, dtype=torch.float32)
    got = egnn._unstack_head_grads(ramp)
    assert len(got) == 40 and list(_PACKED_HEAD_GRAD_STARTS) == egnn._head_param_offsets()
    for i, (g, start) in enumerate(zip(got, _PACKED_HEAD_GRAD_STARTS)):
        shape = _HEAD_GRAD_SHAPES[i % 10]
        assert tuple(g.shape) == shape, i
        assert torch.equal(g, ramp[start:start + g.numel()].view(shape)), i
        assert g.data_ptr() == ramp.data_ptr() + 4 * start                       # a view, not a copy
    ramp = torch.arange(5042, dtype=torch.float32)
    got = egnn._mlp_grads(ramp)
    assert len(got) == 10
    for g, start, shape in zip(got, _PACKED_MLP_GRAD_STARTS, _MLP_GRAD_SHAPES):
        assert tuple(g.shape) == shape and torch.equal(g, ramp[start:start + g.numel()].view(shape))


def test_sums_hand_down_through_the_boxes():
    """The node of layer i + 1 leaves (key of its dx, sums entry) in layer i's box; layer i gets the entry back only for the very
    dy that dx was -- same address, same version -- and its box is empty afterwards either way."""
    from echoglad_amd.nn._train import _hand_down, _handed_down, new_box
    sums, taps = torch.zeros(256, dtype=torch.float64), torch.zeros(2, 2, 128)

    def filled():
        boxes, dx = [new_box(), new_box()], torch.ones(6, 128)
        _hand_down(boxes[0], dx, sums, 2, 5, taps)
        return boxes, dx
    boxes, dx = filled()
    assert _handed_down(boxes[1], dx) is None and boxes[0][1] is not None        # box i is never visible through box j
    got = _handed_down(boxes[0], dx)                                             # the same tensor at the same version
    assert got is not None and got[0] is sums and got[1:4] == (2, 0, 5) and got[4] is taps
    assert boxes == [[None, None], [None, None]]
    assert _handed_down(boxes[0], dx) is None                                    # consumed: not handed out twice
    boxes, dx = filled()
    assert _handed_down(boxes[0], dx * 1) is None and boxes[0] == [None, None]   # another address
    boxes, dx = filled()
    dx.add_(0)                                                                   # autograd accumulating into dx bumps its version
    assert _handed_down(boxes[0], dx) is None and boxes[0] == [None, None]
    assert _handed_down(None, dx) is None                                        # a layer without a box
    boxes, dx = filled()
    boxes[0][0] = "forward slot"
    _handed_down(boxes[0], dx)
    assert boxes[0] == ["forward slot", None]                                    # (the forward's slot is not the backward's)


def test_adam_argument_checks_and_no_cpu_path():
    from echoglad_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(3))
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            Adam([p], **kw)
    opt = Adam([p], lr=1e-3)
    assert opt.param_groups[0]["capturable"] and opt.param_groups[0]["fused"]    # (what engine.GraphedTrainStep looks for)
    opt.step()                                                                   # no gradient anywhere: nothing to do, nothing launched
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError):
        opt.step()                                                               # a CPU parameter: refused before any launch
