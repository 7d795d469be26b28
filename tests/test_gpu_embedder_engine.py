"""-m gpu: the whole training step with a TRAINABLE embedder -- frames -> nn.CNN on the HIP embedder -> UNetNodeFeatureModel on the HIP
front-end -> GNN stack -> heads -> criteria -> capturable Adam -- as one HIP graph (engine.GraphedTrainStep).  The protocol of
test_gpu_engine.py::test_graphed_train_step_replays_equal_eager_steps_under_the_same_epoch, which has to freeze its torch embedder:
here replay k equals the eager step under epoch k bit for bit, and afterwards every parameter and buffer of the embedder and of the
model is bit-equal.

Two tests run the protocol, because one torch piece is left in this step: the tail's backward (ops/pack.py
`_ConvReluPackFn.backward`) differentiates the model's `linears` (1 x 1 convolutions) with torch, and MIOpen's weight gradient may add
with atomics.  On one MI355X machine the protocol failed at replay 0's logits for that reason alone: of the 112 tensors of one forward
+ backward of this pairing (loss, logits, 110 gradients, the embedder's six among them) four identical eager runs agreed bit for bit
in 111, and the gradient of `linears.3.weight` (frame-sized level, 4 -> 128) differed from run to run by 1.9e-7 to 2.8e-7 of its
largest entry -- with a frozen torch embedder just the same.  On another machine 8 such runs agreed in all 112.
`..._replays_equal_eager_steps` trains everything, as the protocol asks, and sets torch.backends.cudnn.deterministic, torch's switch
for reproducible convolution algorithms (on ROCm: MIOpen's deterministic attribute), for the tail's convolutions; it passed in 5 of 5
runs with the switch.  `..._and_the_tail_frozen` freezes `linears`, so that no weight gradient of torch's is in the step, and needs
no switch."""
import numpy as np
import pytest
import torch

from echoglad_amd import data, engine, losses, ops
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import CNN
from echoglad_amd.ops import embedder as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_graphed_train_step_with_a_trainable_embedder_replays_equal_eager_steps(monkeypatch):
    _protocol(monkeypatch, freeze_tail=False)


def test_graphed_train_step_with_a_trainable_embedder_and_the_tail_frozen(monkeypatch):
    """The same protocol with `linears` frozen: every other parameter -- the embedder's six, the front-end's, the stack's, the
    heads' -- trains, and everything is bit-equal."""
    _protocol(monkeypatch, freeze_tail=True)


def _protocol(monkeypatch, freeze_tail):
    B, frame, naux, warm, replays = 2, 16, 3, 2, 3
    if not freeze_tail:
        monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # the tail's 1 x 1 weight gradients are torch's: see above
    routed = []
    inner = E.embed_block_train
    monkeypatch.setattr(E, "embed_block_train", lambda *a, **k: routed.append(1) or inner(*a, **k))

    def build():
        np.random.seed(11)
        ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame)
        batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
        landmark = UNetNodeFeatureModel(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=frame,
                                        num_aux_graphs=naux, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                        num_gnn_layers=2, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                        classifier_dropout_p=0.5).to(DEV).train().enable_hip_frontend(True, train=True)
        embedder = CNN(out_channels=[4], cnn_dropout_p=0.1).to(DEV).train().enable_hip(True, train=True)
        crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, frame, naux)}
        if freeze_tail:
            for q in landmark.linears.parameters():
                q.requires_grad_(False)
        params = [q for q in landmark.parameters() if q.requires_grad] + list(embedder.parameters())
        assert all(q.requires_grad for q in embedder.parameters())
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        model = {"embedder": embedder, "landmark": landmark}

        def loss_fn():
            preds, coord_preds = engine.forward_batch(model, batch, False)
            ls = engine.compute_loss(crit, preds, batch.y, coord_preds, None, batch.valid_labels, B)
            return sum(ls.values()), preds
        return landmark, embedder, opt, loss_fn

    epoch0 = ops.dropout_epoch()
    try:
        ops.dropout_epoch_set(0)
        # --- the graph: `warm` eager steps, then the capture (which draws the seeds every replay reuses), then `replays` replays
        torch.manual_seed(123)
        lm_g, emb_g, opt_g, loss_g = build()
        torch.manual_seed(77)
        step = engine.GraphedTrainStep(loss_g, opt_g, warmup=warm)
        assert len(routed) == warm + 1                                     # the embedder took the HIP training route
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
        lm_e, emb_e, opt_e, loss_e = build()
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
        assert len(list(emb_g.named_parameters())) == 6 and int(emb_g.conv[0][0].bn.num_batches_tracked) == warm + replays
        assert len(set(losses_g)) == replays, losses_g                     # fresh masks at every replay
    finally:
        ops.dropout_epoch_set(epoch0)
