"""-m gpu: trainer.EvalStep -- the validation step (evaluation-mode forward under no_grad + MSE loss) as ONE captured hipGraph that stays
valid while a TrainStep on the same model moves the weights, with the batch losses summed on the device.

Bars: replay == eager == by-hand evaluation bit for bit (same kernels on the same values); against the CPU oracle the suite's stated bars,
output rel-L2 <= 1e-5 and loss <= 1e-5 relative."""
import pytest
import torch

from tests._golden import rel_l2
from tests._workloads import grid, naca_points, uniform_points
from tests.test_configs_gpu import LOSS_TOL, OUT_TOL, csr_dict, dev, make_model, model_cfg

pytestmark = pytest.mark.gpu


def by_hand(m, kw, p, t):
    """what the parent commit offers a validation loop: model.eval(), no_grad, ops.mse_loss"""
    from gaot_amd import ops
    was = m.training
    m.eval()
    with torch.no_grad():
        y = m(pndata=p, **kw)
        loss = ops.mse_loss(y, t)
    m.train(was)
    return y.clone(), loss.clone()


def clone_model(model, sd, cin, cout):
    from gaot_amd.model.gaot import GAOT
    m = GAOT(cin, cout, model_cfg(model))
    m.load_state_dict(sd)
    return m.to(dev()).train()


@pytest.fixture(scope="module")
def fx():
    """~1k-node mesh, batch 2, three batches of fields; the oracle's prediction and loss of batch 0, computed once"""
    from oracle import gaot_oracle as O
    model, sd, ocfg = make_model(3, 2, [32, 32], C=32, hidden=128, heads=4, radius=0.08, seed=11)
    g = torch.Generator().manual_seed(11)
    lat, x = grid([32, 32]), uniform_points(1000, 2, g)
    ps = [torch.randn(2, 1000, 3, generator=g) for _ in range(3)]
    ts = [torch.randn(2, 1000, 2, generator=g) for _ in range(3)]
    enc, dec = [O.radius_csr(x, lat, 0.08)], [O.radius_csr(lat, x, 0.08)]
    with torch.no_grad():
        pred = O.gaot_forward(sd, ocfg, lat, x, ps[0], None, enc, dec)
        loss = torch.mean((pred - ts[0]) ** 2)
    kw = dict(latent_tokens_coord=lat.to(dev()), xcoord=x.to(dev()), encoder_nbrs=[csr_dict(enc[0])], decoder_nbrs=[csr_dict(dec[0])])
    return dict(model=model, sd=sd, kw=kw, ps=[p.to(dev()) for p in ps], ts=[t.to(dev()) for t in ts], o_pred=pred, o_loss=float(loss))


def test_fx_replay_equals_eager_equals_by_hand_and_tracks_the_oracle(fx):
    from gaot_amd.trainer import EvalStep
    p, t = fx["ps"][0], fx["ts"][0]
    got = {}
    for graph in (True, False):
        m = clone_model(fx["model"], fx["sd"], 3, 2)
        ev = EvalStep(m, use_graph=graph)
        ev.bind(p, t, **fx["kw"])
        l1 = ev.step().clone()
        l2 = ev.step(p, t).clone()
        assert l1.is_cuda and l1.dim() == 0 and torch.equal(l1, l2)
        assert m.training and all(s.training for s in m.modules())
        assert ev.n_captures == (1 if graph else 0)
        got[graph] = (l1.cpu(), ev.prediction.clone().cpu())
    m = clone_model(fx["model"], fx["sd"], 3, 2)
    y, loss = by_hand(m, fx["kw"], p, t)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][0], loss.cpu())
    assert torch.equal(got[True][1], got[False][1]) and torch.equal(got[True][1], y.cpu())
    e_out = rel_l2(got[True][1], fx["o_pred"])
    e_loss = abs(float(got[True][0]) - fx["o_loss"]) / abs(fx["o_loss"])
    print(f"[EvalStep fx] out rel-L2 {e_out:.2e}  loss rel {e_loss:.2e}")
    assert e_out <= OUT_TOL and e_loss <= LOSS_TOL


def test_captured_evaluation_survives_training_on_the_same_model(fx):
    """eval, one TrainStep.step, eval again -- three times: every evaluation sees the current weights without a re-capture, and the training
    run is bit for bit the run without an EvalStep in between"""
    from gaot_amd.trainer import EvalStep, TrainStep
    runs = {}
    for with_eval in (True, False):
        m = clone_model(fx["model"], fx["sd"], 3, 2)
        ts = TrainStep(m, lr=5e-3, weight_decay=1e-5, use_graph=True)
        ts.bind(fx["ps"][1], fx["ts"][1], **fx["kw"])
        assert m.auto_graph is False
        train_losses, eval_losses = [], []
        if with_eval:
            ev = EvalStep(m, use_graph=True)
            ev.bind(fx["ps"][0], fx["ts"][0], **fx["kw"])
            eval_losses.append(ev.step().clone())
            assert ev.n_captures == 1
        for k in range(3):
            train_losses.append(ts.step(fx["ps"][1 + k % 2], fx["ts"][1 + k % 2]).clone())
            if with_eval:
                eval_losses.append(ev.step().clone())
                _, hand = by_hand(m, fx["kw"], fx["ps"][0], fx["ts"][0])          # eager, on the weights as they are now
                assert torch.equal(eval_losses[-1], hand), k
                assert not torch.equal(eval_losses[-1], eval_losses[-2]), k
                assert ev.n_captures == 1 and m.auto_graph is False and m.training
        torch.cuda.synchronize()
        runs[with_eval] = (torch.stack(train_losses).cpu(), torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu())
    assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0], runs[False][0])
    assert torch.equal(runs[True][1], runs[False][1])


def test_running_pair_mean_reset_and_device_result(fx):
    from gaot_amd.trainer import EvalStep
    m = clone_model(fx["model"], fx["sd"], 3, 2)
    ev = EvalStep(m)
    ev.bind(fx["ps"][0], fx["ts"][0], **fx["kw"])
    with pytest.raises(RuntimeError):
        ev.mean_loss()
    losses = []
    for p, t in zip(fx["ps"], fx["ts"]):
        out = ev.step(p, t)
        assert torch.is_tensor(out) and out.is_cuda and out.dim() == 0
        losses.append(float(out.double().item()))
    assert len(set(losses)) == 3 and ev.n_captures == 1          # (the capture's warm-up passes are not counted as batches)
    exact = sum(losses) / 3.0
    assert abs(ev.mean_loss() - exact) <= 2.0 ** -23 * exact
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.mean_loss()
    one = float(ev.step(fx["ps"][2], fx["ts"][2]).double().item())
    assert ev.mean_loss() == one


def test_evaluation_draws_nothing():
    """attention dropout and sampling_strategy='ratio' are training-time draws: two replays on one batch give one loss, the loss of the plain
    evaluation pass, and the model comes back in training mode"""
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import AttentionConfig
    from gaot_amd.trainer import EvalStep
    from oracle import gaot_oracle as O
    model, sd, _ = make_model(2, 1, [16, 16], C=32, hidden=128, heads=4, radius=0.12, seed=5, sampling_strategy="ratio", sample_ratio=0.6)
    cfg = model_cfg(model)
    cfg.args.transformer.attn_config = AttentionConfig(num_heads=4, num_kv_heads=4, atten_dropout=0.2)
    m = GAOT(2, 1, cfg)
    m.load_state_dict(sd)
    m.to(dev()).train()
    g = torch.Generator().manual_seed(5)
    lat, x = grid([16, 16]), uniform_points(700, 2, g)
    p, t = torch.randn(2, 700, 2, generator=g).to(dev()), torch.randn(2, 700, 1, generator=g).to(dev())
    kw = dict(latent_tokens_coord=lat.to(dev()), xcoord=x.to(dev()), encoder_nbrs=[csr_dict(O.radius_csr(x, lat, 0.12))],
              decoder_nbrs=[csr_dict(O.radius_csr(lat, x, 0.12))])
    ev = EvalStep(m)
    ev.bind(p, t, **kw)
    a = ev.step().clone()
    b = ev.step().clone()
    assert torch.equal(a, b) and ev.n_captures == 1
    assert m.training and all(s.training for s in m.modules())
    m.encoder.eval()                                   # flags are put back as they were FOUND, not set to one value
    eager = EvalStep(m, use_graph=False)               # (a replay runs no Python forward: the eager step is the one that flips the flags)
    eager.bind(p, t, **kw)
    assert torch.equal(eager.step(), a)
    assert m.training and not m.encoder.training and m.decoder.training
    m.train()
    _, hand = by_hand(m, kw, p, t)
    assert torch.equal(a, hand)


def test_vx_three_compositions_over_two_buckets_one_capture_each():
    from gaot_amd import plan as P
    from gaot_amd.trainer import EvalStep
    from oracle import gaot_oracle as O
    nS, B, N = 6, 2, 2048
    # (built with training-time neighbour sub-sampling: the static-union path must not draw in evaluation mode either -- the comparison
    # with the plain evaluation pass at the end would be off by far more than rounding)
    model, sd, _ = make_model(3, 1, [32, 32], radius=0.066, seed=4, sampling_strategy="ratio", sample_ratio=0.6)
    g = torch.Generator().manual_seed(9)
    lat = grid([32, 32])
    xs = [naca_points(N, g, 0.15) for _ in range(nS)]
    rs = [0.066 * (1.0 + 0.12 * (i % 3)) for i in range(nS)]          # graphs of three radii: edge totals more than a bucket apart
    enc = [[O.radius_csr(x, lat, r)] for x, r in zip(xs, rs)]
    dec = [[O.radius_csr(lat, x, r)] for x, r in zip(xs, rs)]
    P_all, T_all = torch.randn(nS, N, 3, generator=g), torch.randn(nS, N, 1, generator=g)
    batches = [[0, 3], [2, 5], [3, 0]]                                # two compositions of one bucket, one of another
    tot = [sum(int(enc[i][0][0].numel()) for i in b) for b in batches]
    assert P.edge_bucket(tot[0]) == P.edge_bucket(tot[2]) != P.edge_bucket(tot[1])
    latd, xd = lat.to(dev()), torch.stack(xs).to(dev())
    encd = [[csr_dict(c) for c in row] for row in enc]
    decd = [[csr_dict(c) for c in row] for row in dec]
    for row in encd:                                                  # a dataset resident on the device: every sample has its plan
        P.plan_for(row[0], N)
    for row in decd:
        P.plan_for(row[0], lat.shape[0])
    out = {}
    for graph in (True, False):
        m = clone_model(model, sd, 3, 1)
        ev = EvalStep(m, use_graph=graph)
        b0 = batches[0]
        ev.bind(P_all[b0].to(dev()), T_all[b0].to(dev()), latent_tokens_coord=latd, xcoord=xd[b0], encoder_nbrs=[encd[i] for i in b0],
                decoder_nbrs=[decd[i] for i in b0])
        ls, preds = [], []
        for b in batches:
            ls.append(ev.step(P_all[b].to(dev()), T_all[b].to(dev()), xcoord=xd[b], encoder_nbrs=[encd[i] for i in b], decoder_nbrs=[decd[i] for i in b]).clone())
            preds.append(ev.prediction.clone())
        torch.cuda.synchronize()
        out[graph] = torch.stack(ls).cpu()
        if graph:
            assert ev.n_captures == 2 == len(ev._graph_sets)
            assert abs(ev.mean_loss() - float(out[True].double().mean())) <= 2.0 ** -23 * float(out[True].double().mean())
            # batch 2 is batch 0 with its samples swapped, replayed from batch 0's capture: the rows follow the table uploaded for the step
            assert rel_l2(preds[2][0].cpu(), preds[0][1].cpu()) < 1e-6 and rel_l2(preds[2][1].cpu(), preds[0][0].cpu()) < 1e-6
            assert rel_l2(preds[2][0].cpu(), preds[0][0].cpu()) > 1e-2
    assert torch.equal(out[True], out[False]), (out[True], out[False])
    assert float(out[True][0]) != float(out[True][1])
    # the plain evaluation pass (unions composed on the host) on the last batch: the same numbers to rounding
    m = clone_model(model, sd, 3, 1)
    b = batches[-1]
    _, hand = by_hand(m, dict(latent_tokens_coord=latd, xcoord=xd[b], encoder_nbrs=[encd[i] for i in b], decoder_nbrs=[decd[i] for i in b]),
                      P_all[b].to(dev()), T_all[b].to(dev()))
    assert abs(float(hand) - float(out[True][-1])) <= 1e-5 * abs(float(hand))
