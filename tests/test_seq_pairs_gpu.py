"""-m gpu: sequential training from a PairStore -- the batch of a training / validation step composed on the device from resident
trajectories (csrc/seq_pairs.hip) inside the captured step.

Bars: the composed batches equal the reference's DynamicPairDataset / TestDataset items (tests/golden/seq_pairs.npz) BIT FOR BIT -- every
operation is one correctly rounded fp32 subtraction or division in the reference's order, so there is no tolerance to state; a step fed by
`step_pairs` equals, bit for bit, the step fed the recorded batch through `step(x, y)` (the same kernels on the same values)."""
import numpy as np
import pytest
import torch

from tests import _seq_pairs as F
from tests._workloads import grid, uniform_points
from tests.test_configs_gpu import dev, make_model, model_cfg

pytestmark = pytest.mark.gpu

CASES = F.load_fixture()


def batches_of(order, B):
    """`order` cut into lists of B, the last one filled up with repeats of its head"""
    order = list(order) + list(order[:(-len(order)) % B])
    return [order[i:i + B] for i in range(0, len(order), B)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_every_recorded_item_bit_for_bit(name):
    c = CASES[name]
    store = F.make_store(c, dev())
    L, N, W, U = len(store), store.N, store.input_width(), store.U
    X, Y = c["x"].to(dev()), c["y"].to(dev())
    seen = set()
    for B in (1, 5):
        x = torch.full((B, N, W), float("nan"), device=dev())
        y = torch.full((B, N, U), float("nan"), device=dev())
        order = list(range(L - 1, -1, -1)) + [0, 0, L - 1]          # descending, with repeats
        for b in batches_of(order, B):
            store.compose(torch.tensor(b, dtype=torch.int32, device=dev()), x, y)
            assert torch.equal(x, X[b]) and torch.equal(y, Y[b]), (name, B, b)
            seen.update(b)
    assert seen == set(range(L)) and store.status() == 0
    x, y = store.batch(list(range(L)))          # the allocating form, every item in one launch
    assert torch.equal(x, X) and torch.equal(y, Y)
    # the torch-expression form on the device (what tools/seq_pairs_bench.py times the kernel against) says the same
    xt, yt = store.batch_torch(list(range(L)))
    assert torch.equal(xt, X) and torch.equal(yt, Y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_conditioned_norm_form_drops_the_diff_column_and_returns_the_condition(name):
    c = CASES[name]
    store = F.make_store(c, dev())
    L = len(store)
    X, Y = c["x"].to(dev()), c["y"].to(dev())
    for b in batches_of(range(L - 1, -1, -1), 5) + [[L - 1]]:
        x, y, cond = store.batch(b, conditional_norm=True)
        assert x.shape[-1] == X.shape[-1] - 1 and tuple(cond.shape) == (len(b), 1)
        assert torch.equal(x, X[b][..., :-1]) and torch.equal(cond, X[b][:, 0, -2:-1]) and torch.equal(y, Y[b]), (name, b)
    assert store.status() == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_test_batch_equals_the_recorded_testdataset_items(name):
    c = CASES[name]
    store = F.make_store(c, dev())
    S = c["u"].shape[0]
    ids = list(range(S - 1, -1, -1)) + [0]
    x0, yseq = store.test_batch(ids, c["test_time_indices"])
    assert torch.equal(x0, c["test_x0"].to(dev())[ids]) and torch.equal(yseq, c["test_yseq"].to(dev())[ids])
    x0, yseq = store.test_batch(torch.tensor([1]), c["test_time_indices"][:1])          # no target step: K = 0
    assert torch.equal(x0, c["test_x0"].to(dev())[[1]]) and tuple(yseq.shape) == (1, 0, store.N, store.U)
    assert store.status() == 0


def test_test_batch_feeds_the_rollout_like_the_recorded_items():
    c = CASES["n67_time_der"]
    store = F.make_store(c, dev())
    model, _, _ = make_model(6, 3, [16, 16], C=32, hidden=128, heads=4, radius=0.2, precompute=False, seed=21)
    m = model.to(dev()).eval()
    g = torch.Generator().manual_seed(21)
    lat, xc = grid([16, 16]).to(dev()), uniform_points(67, 2, g).to(dev())
    ti, tv = c["test_time_indices"], c["t"].numpy()
    roll = lambda x0: m.autoregressive_predict(x_batch=x0, time_indices=ti, t_values=tv, stats=c["stats"], stepper_mode="time_der",
                                               latent_tokens_coord=lat, fixed_coord=xc).clone()
    x0, yseq = store.test_batch([0, 1, 2], ti)
    got, want = roll(x0), roll(c["test_x0"].to(dev()))
    assert got.shape == yseq.shape and torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_out_of_range_indices_are_clamped_and_flagged():
    c = CASES["n67_residual"]
    store = F.make_store(c, dev())
    L = len(store)
    X, Y = c["x"].to(dev()), c["y"].to(dev())
    assert store.status() == 0
    x, y = store.batch([3, L, -1, 2 ** 31 - 1, -2 ** 31, 7])
    torch.cuda.synchronize()          # a normal launch: nothing faulted, the stream is alive
    assert store.status() == 1
    rows = [3, L - 1, 0, L - 1, 0, 7]
    assert torch.equal(x, X[rows]) and torch.equal(y, Y[rows])
    store.clear_status()
    x, _ = store.batch([5])
    assert store.status() == 0 and torch.equal(x, X[[5]])
    S = c["u"].shape[0]
    x0, yseq = store.test_batch([S, -1], [0, 2])
    assert store.status() == 1 and torch.equal(x0, c["test_x0"].to(dev())[[S - 1, 0]])
    store.clear_status()
    x0, yseq = store.test_batch([1], [0, 7, -3])          # time indices past the trajectory: clamped, flag bit 1
    assert store.status() == 2 and torch.equal(yseq, c["u"].to(dev())[[1]][:, [6, 0]])


# ---- the captured steps
def fresh(model, sd, cin, cout):
    from gaot_amd.model.gaot import GAOT
    m = GAOT(cin, cout, model_cfg(model))
    m.load_state_dict(sd)
    return m.to(dev()).train()


@pytest.fixture(scope="module")
def pairs_setup():
    """the 257-node case (U = 4, no c, stepper time_der) on an fx grid, its store on the device, three index batches of four"""
    c = CASES["n257_truncated"]
    g = torch.Generator().manual_seed(31)
    kw = dict(latent_tokens_coord=grid([16, 16]).to(dev()), xcoord=uniform_points(257, 2, g).to(dev()))
    model, sd, _ = make_model(6, 4, [16, 16], C=32, hidden=128, heads=4, radius=0.15, precompute=False, seed=31)
    return dict(c=c, store=F.make_store(c, dev()), kw=kw, model=model, sd=sd, X=c["x"].to(dev()), Y=c["y"].to(dev()),
                lists=[[3, 17, 0, 9], [19, 19, 2, 5], [1, 0, 7, 12], [8, 4, 4, 15]])


def test_trainstep_bind_pairs_captured_equals_eager_equals_step_on_recorded_batches(pairs_setup):
    from gaot_amd.trainer import TrainStep
    s = pairs_setup
    runs = {}
    for way in ("captured", "eager", "recorded"):
        m = fresh(s["model"], s["sd"], 6, 4)
        ts = TrainStep(m, lr=5e-3, weight_decay=1e-5, use_graph=way != "eager")
        losses = []
        if way == "recorded":
            ts.bind(s["X"][s["lists"][0]], s["Y"][s["lists"][0]], **s["kw"])
            for b in s["lists"][:3]:
                losses.append(ts.step(s["X"][b], s["Y"][b]).clone())
        else:
            ts.bind_pairs(s["store"], 4, **s["kw"])
            epoch = torch.tensor(sum(s["lists"], []), dtype=torch.int32, device=dev())          # an epoch's order, uploaded once
            for k, b in enumerate(s["lists"][:3]):          # a slice of the device list (no host data), or a host list
                losses.append(ts.step_pairs(epoch[4 * k:4 * k + 4] if k != 1 else b).clone())
            assert ts.n_captures == (1 if way == "captured" else 0)
            with pytest.raises(ValueError, match="whole batches"):
                ts.step_pairs([1, 2])
        torch.cuda.synchronize()
        runs[way] = (torch.stack(losses).cpu(), ts.opt.flat_p.clone().cpu())
    assert s["store"].status() == 0
    print("[bind_pairs] losses", runs["captured"][0].tolist())
    assert len(set(runs["captured"][0].tolist())) == 3
    for way in ("eager", "recorded"):
        assert torch.equal(runs["captured"][0], runs[way][0]), (way, runs["captured"][0], runs[way][0])
        assert torch.equal(runs["captured"][1], runs[way][1]), way


def test_trainstep_bind_pairs_feeds_a_conditioned_norm_model_its_per_step_condition(pairs_setup):
    """three pairs with three different start times: the captured step must hand the model each step's own `condition`"""
    from gaot_amd.trainer import TrainStep
    s = pairs_setup
    model, _, _ = make_model(5, 4, [16, 16], C=32, hidden=128, heads=4, radius=0.15, precompute=False, seed=32)
    sd = {k: v.detach().clone() for k, v in _cond_model(model).state_dict().items()}
    lists = s["lists"][:3]
    conds = [s["X"][b][:, 0, -2:-1].contiguous() for b in lists]
    assert not torch.equal(conds[0], conds[1]) and not torch.equal(conds[1], conds[2])
    m = _cond_model(model, sd)
    ts = TrainStep(m, lr=5e-3, weight_decay=1e-5, use_graph=True)
    ts.bind_pairs(s["store"], 4, conditional_norm=True, **s["kw"])
    got = [ts.step_pairs(b).clone() for b in lists]
    assert ts.n_captures == 1 and tuple(ts._x.shape) == (4, 257, 5)
    torch.cuda.synchronize()
    hand = _cond_model(model, sd)
    th = TrainStep(hand, lr=5e-3, weight_decay=1e-5, use_graph=False)
    want = []
    for b, cond in zip(lists, conds):
        th.bind(s["X"][b][..., :-1].contiguous(), s["Y"][b], condition=cond, **s["kw"])
        want.append(th.step().clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(want)), (got, want)
    assert torch.equal(ts.opt.flat_p, th.opt.flat_p)
    # ... and the condition matters: the same steps with the first step's condition frozen in end elsewhere
    frozen = _cond_model(model, sd)
    tf = TrainStep(frozen, lr=5e-3, weight_decay=1e-5, use_graph=False)
    for b in lists:
        tf.bind(s["X"][b][..., :-1].contiguous(), s["Y"][b], condition=conds[0], **s["kw"])
        tf.step()
    assert not torch.equal(tf.opt.flat_p, th.opt.flat_p)


def _cond_model(model, sd=None):
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import AttentionConfig
    cfg = model_cfg(model)
    a = cfg.args.transformer.attn_config
    cfg.args.transformer.attn_config = AttentionConfig(num_heads=a.num_heads, num_kv_heads=a.num_kv_heads, use_conditional_norm=True)
    torch.manual_seed(33)
    m = GAOT(5, 4, cfg)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dev()).train()


def test_evalstep_bind_pairs_mean_loss_one_capture_and_interleaved_training(pairs_setup):
    from gaot_amd import ops
    from gaot_amd.trainer import EvalStep, TrainStep
    s = pairs_setup
    m = fresh(s["model"], s["sd"], 6, 4)

    def by_hand(b):
        m.eval()
        with torch.no_grad():
            loss = ops.mse_loss(m(pndata=s["X"][b], **s["kw"]), s["Y"][b]).clone()
        m.train()
        return loss

    # (the TrainStep first: its optimizer re-points the parameters at one flat buffer, and a captured evaluation holds their addresses)
    ts = TrainStep(m, lr=5e-3, weight_decay=1e-5, use_graph=True)
    ts.bind_pairs(s["store"], 4, **s["kw"])
    ev = EvalStep(m)
    ev.bind_pairs(s["store"], 4, **s["kw"])
    want = [by_hand(b) for b in s["lists"]]
    got = [ev.step_pairs(b).clone() for b in s["lists"]]
    assert torch.equal(torch.stack(got), torch.stack(want)) and ev.n_captures == 1 and len(set(float(v) for v in got)) == 4
    exact = sum(float(v.double()) for v in want) / 4.0
    assert abs(ev.mean_loss() - exact) <= 2.0 ** -23 * exact
    ev.reset()
    # training on the same model, from the same store, in between: every evaluation sees the current weights, nothing is re-captured
    last = got[0]
    for k in range(3):
        ts.step_pairs(s["lists"][k + 1])
        now = ev.step_pairs(s["lists"][0]).clone()
        assert torch.equal(now, by_hand(s["lists"][0])) and not torch.equal(now, last), k
        last = now
    assert ev.n_captures == 1 and ts.n_captures == 1 and m.training and s["store"].status() == 0
    with pytest.raises(ValueError, match="whole batches"):
        ev.step_pairs([0])
