"""-m gpu: the whole training step of the CNN-pyramid variant -- frames -> nn.CNN on the HIP embedder (trainable) ->
nn.CNNHierarchicalPatchModel with enable_hip_pyramid(True, train=True) -> GNN stack -> heads -> criteria -> capturable Adam -- as one
HIP graph (engine.GraphedTrainStep).  The protocol of tests/test_gpu_embedder_engine.py, restated: replay k equals the eager step
under epoch k bit for bit in the loss and the logits, afterwards every parameter and buffer of both modules is bit-equal, and the
losses differ between replays (fresh masks).  The embedder is trainable, so the pyramid's first block needs dx at side 32: the matrix
data gradient.  No torch convolution is left in this step (every nn.Conv2d of both modules is hooked: none runs), so nothing is frozen
and no determinism switch of torch's is set."""
import numpy as np
import pytest
import torch

from echoglad_amd import data, engine, losses, ops
from echoglad_amd.nn import CNN, CNNHierarchicalPatchModel
from echoglad_amd.ops import embedder as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_graphed_train_step_of_the_cnn_pyramid_replays_equal_eager_steps(monkeypatch):
    B, frame, naux, warm, replays = 2, 32, 4, 2, 3
    routed, torch_convs = [], []
    inner = E.pyramid_block_train
    monkeypatch.setattr(E, "pyramid_block_train", lambda *a, **k: routed.append(int(a[0].shape[2])) or inner(*a, **k))

    def build():
        np.random.seed(11)
        ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame)
        batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
        landmark = CNNHierarchicalPatchModel(cnn_layers_out_width=[16, 8, 4, 2], cnn_dropout_p=0.1, frame_size=frame, num_aux_graphs=naux,
                                             node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2,
                                             output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                             classifier_dropout_p=0.5).to(DEV).train().enable_hip_pyramid(True, train=True)
        embedder = CNN(out_channels=[128], cnn_dropout_p=0.1).to(DEV).train().enable_hip(True, train=True)
        for module in (landmark, embedder):
            for m in module.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.register_forward_hook(lambda mod, inp, out: torch_convs.append(type(mod).__name__))
        crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, frame, naux)}
        params = list(landmark.parameters()) + list(embedder.parameters())
        assert all(q.requires_grad for q in params)
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
        assert routed == [32, 16, 8, 4] * (warm + 1)                       # the pyramid took the HIP training route, block by block
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
        assert int(lm_g.conv[0].bn.num_batches_tracked) == int(lm_g.conv[3].bn.num_batches_tracked) == warm + replays
        assert all(torch.isfinite(q).all() for q in lm_g.parameters())
        assert not torch_convs, torch_convs                                # no torch convolution is left in this step
        assert len(set(losses_g)) == replays, losses_g                     # fresh masks at every replay
    finally:
        ops.dropout_epoch_set(epoch0)
