"""-m gpu: the whole training step of test_gpu_embedder_engine.py -- frames -> nn.CNN on the HIP embedder -> UNetNodeFeatureModel on the
HIP front-end -> GNN stack -> heads -> criteria -> capturable Adam -- with the tail's backward in HIP as well
(enable_hip_frontend(True, train=True, tail=True): eg_conv1x1_relu_pack_bwd).  Everything trains, `linears` included, and
torch.backends.cudnn.deterministic stays False: no torch convolution gradient is left in the step.  The protocol is the one of
test_gpu_embedder_engine.py::_protocol, restated: replay k of the captured step equals the eager step under epoch k bit for bit, and
afterwards every parameter and buffer is bit-equal.  The second test is the check DESIGN 3.6c describes: four identical eager forward
+ backward runs of this pairing agree in loss, logits and every gradient -- all 112 tensors."""
import numpy as np
import pytest
import torch

from echoglad_amd import data, engine, losses, ops
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import CNN
from echoglad_amd.ops import pack as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, FRAME, NAUX = 2, 16, 3


def _build():
    np.random.seed(11)
    ds = data.SyntheticEchoDataset(num_aux_graphs=NAUX, frame_size=FRAME)
    batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
    landmark = UNetNodeFeatureModel(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=FRAME,
                                    num_aux_graphs=NAUX, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                    num_gnn_layers=2, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                    classifier_dropout_p=0.5).to(DEV).train().enable_hip_frontend(True, train=True, tail=True)
    embedder = CNN(out_channels=[4], cnn_dropout_p=0.1).to(DEV).train().enable_hip(True, train=True)
    crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, FRAME, NAUX)}
    params = list(landmark.parameters()) + list(embedder.parameters())
    assert all(q.requires_grad for q in params)                          # everything trains, the tail's `linears` included
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    model = {"embedder": embedder, "landmark": landmark}

    def loss_fn():
        preds, coord_preds = engine.forward_batch(model, batch, False)
        ls = engine.compute_loss(crit, preds, batch.y, coord_preds, None, batch.valid_labels, B)
        return sum(ls.values()), preds
    return landmark, embedder, opt, loss_fn


def _count_tail_calls(monkeypatch):
    routed = []
    inner = P._ConvReluPackHipFn.backward
    monkeypatch.setattr(P._ConvReluPackHipFn, "backward", staticmethod(lambda ctx, g: routed.append(1) or inner(ctx, g)))
    return routed


def test_graphed_train_step_with_the_hip_tail_replays_equal_eager_steps(monkeypatch):
    warm, replays = 2, 3
    assert torch.backends.cudnn.deterministic is False
    routed = _count_tail_calls(monkeypatch)
    epoch0 = ops.dropout_epoch()
    try:
        ops.dropout_epoch_set(0)
        # --- the graph: `warm` eager steps, then the capture (which draws the seeds every replay reuses), then `replays` replays
        torch.manual_seed(123)
        lm_g, emb_g, opt_g, loss_g = _build()
        torch.manual_seed(77)
        step = engine.GraphedTrainStep(loss_g, opt_g, warmup=warm)
        assert len(routed) == warm + 1                                     # the tail took its HIP backward
        e0 = ops.dropout_epoch()
        losses_g, preds_g = [], []
        for _ in range(replays):
            out = step()
            losses_g.append(float(out[0]))
            preds_g.append(out[1].clone())
        assert ops.dropout_epoch() == e0 + replays
        # --- the same thing eagerly: `warm` steps, then `replays` steps that all start from the host RNG state the capture started from
        ops.dropout_epoch_set(e0)
        torch.manual_seed(123)
        lm_e, emb_e, opt_e, loss_e = _build()
        torch.manual_seed(77)

        def eager():
            out = loss_e()
            opt_e.zero_grad(set_to_none=True)
            out[0].backward()
            opt_e.step()
            return out
        for _ in range(warm):
            eager()
        rng = torch.get_rng_state()
        for k in range(replays):
            torch.set_rng_state(rng)
            ops.dropout_epoch_set(e0 + k + 1)
            out = eager()
            diff = (out[1].detach() - preds_g[k]).abs()
            print(f"replay {k}: loss {losses_g[k]!r} against eager {float(out[0].detach())!r}; {int((diff > 0).sum())} of {diff.numel()} "
                  f"logits differ, by at most {float(diff.max()):.3e} (largest logit {float(preds_g[k].abs().max()):.3e})")
            assert float(out[0].detach()) == losses_g[k], (k, float(out[0].detach()), losses_g[k])
            assert torch.equal(out[1].detach(), preds_g[k]), k
        for tag, a, b in (("embedder", emb_g, emb_e), ("landmark", lm_g, lm_e)):
            for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
                assert na == nb and torch.equal(pa.detach(), pb.detach()), (tag, na)
            for (na, ba), (nb, bb) in zip(a.named_buffers(), b.named_buffers()):
                assert na == nb and torch.equal(ba, bb), (tag, na)
        assert len(set(losses_g)) == replays, losses_g                     # fresh masks at every replay
        assert torch.backends.cudnn.deterministic is False
    finally:
        ops.dropout_epoch_set(epoch0)


def test_four_identical_eager_runs_agree_in_every_tensor(monkeypatch):
    assert torch.backends.cudnn.deterministic is False
    routed = _count_tail_calls(monkeypatch)
    epoch0 = ops.dropout_epoch()
    try:
        runs = []
        for _ in range(4):
            ops.dropout_epoch_set(5)
            torch.manual_seed(123)
            lm, emb, _, loss_fn = _build()
            torch.manual_seed(77)
            loss, preds = loss_fn()
            loss.backward()
            named = list(lm.named_parameters()) + list(emb.named_parameters())
            assert all(q.grad is not None for _, q in named)
            runs.append([("loss", loss.detach()), ("logits", preds.detach())] + [(n, q.grad) for n, q in named])
        assert len(routed) == 4
        assert len(runs[0]) == 112 and any(n == "linears.3.weight" for n, _ in runs[0])
        for other in runs[1:]:
            for (na, a), (nb, b) in zip(runs[0], other):
                assert na == nb and torch.equal(a, b), na
    finally:
        ops.dropout_epoch_set(epoch0)


def test_tail_with_connection_nodes_raises():
    m = UNetNodeFeatureModel(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=FRAME, num_aux_graphs=NAUX,
                             node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2,
                             output_activation="logit", use_coordinate_graph=False, use_connection_nodes=True)
    with pytest.raises(ValueError, match="use_connection_nodes"):
        m.enable_hip_frontend(True, train=True, tail=True)
