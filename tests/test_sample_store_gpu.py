"""-m gpu: index-driven static training -- a step's batch gathered (csrc/sample_store.hip) and its vx unions composed (csrc/gno.hip
union_compose_indexed_kernel) on the device from a DEVICE list of sample indices, inside the captured step (static.SampleStore,
trainer.bind_samples / step_samples).

Bars.  The indexed compose kernel and the gather move integers and copy floats: every comparison with the host-fed kernel, with torch
indexing, between replay and eager, and with the host-fed training path at an equal edge capacity is torch.equal -- a difference is a bug, not
rounding.  Against the oracle the bars are tests/test_configs_gpu.py's (LOSS_TOL, GRAD_TOL without a floor: its grad_errors, the comparison
check_step makes), imported, not restated.  Shapes: tests/test_graph_store_gpu.py::_training_data -- 6 NACA meshes of 512 points, a 16 x 16
latent grid, radius 0.133, B = 3; the samples' edge counts differ, so the in-kernel prefix sum has unequal terms.
"""
import dataclasses
import functools

import pytest
import torch

from tests._golden import fp32_noise
from tests._workloads import grid, naca_points, shell_points
from tests.test_configs_gpu import GRAD_TOL, LOSS_TOL, dev, grad_errors, make_model, model_cfg
from tests.test_graph_store_gpu import _training_data

pytestmark = pytest.mark.gpu

RADIUS, B = 0.133, 3
INDEX_LISTS = ([5, 0, 3], [1, 2, 4], [3, 3, 0], [2, 1, 0])
POISON = -7


@functools.lru_cache(maxsize=None)
def _store(scales=(1.0,)):
    """(x, latent on the device, c, u on the device, the device GraphStore): built once per scale set, shared, never modified"""
    from gaot_amd.graphs import GraphBuilder
    x, lat, P_all, T_all = _training_data()
    latd = lat.to(dev())
    return x, latd, P_all.to(dev()), T_all.to(dev()), GraphBuilder().build_store(x.to(dev()), latd, RADIUS, list(scales))


@functools.lru_cache(maxsize=None)
def _permuted_store():
    """samples that are node permutations of ONE mesh with different fields: every sample has the same edge count"""
    from gaot_amd.graphs import GraphBuilder
    g = torch.Generator().manual_seed(43)
    nS, N = 6, 512
    x0 = naca_points(N, g, 0.15) * torch.tensor([1.7, 0.6]) + torch.tensor([0.4, 2.0])
    x = torch.stack([x0[torch.randperm(N, generator=g)] for _ in range(nS)]).contiguous()
    latd = grid([16, 16]).to(dev())
    P_all, T_all = torch.randn(nS, N, 3, generator=g).to(dev()), torch.randn(nS, N, 1, generator=g).to(dev())
    return latd, P_all, T_all, GraphBuilder().build_store(x.to(dev()), latd, RADIUS, [1.0])


def _idx(lst):
    return torch.tensor(lst, dtype=torch.int32, device=dev())


def _sides(store, latd):
    """(side, n_src, n_dst, per-sample dict rows, source coordinates by batch, query coordinates by batch)"""
    return (("encoder", store.N, store.Q, store.encoder, lambda b: store.x_scaled[b].contiguous(), lambda b: latd),
            ("decoder", store.Q, store.N, store.decoder, lambda b: latd, lambda b: store.x_scaled[b].contiguous()))


def _union(store, n_src, n_dst, e_cap):
    from gaot_amd import plan as P
    su = P.StaticUnion(B, n_src, n_dst, store.dim, store.dim, e_cap, dev())
    pl = su.plan
    for t in (pl.index, pl.edge_query, pl._t_edge, pl.splits, pl._t_splits, pl.e_dev, su.src, su.dst):
        t.fill_(POISON)
    return su


def _outputs(su):
    pl = su.plan
    return {"index": pl.index, "edge_query": pl.edge_query, "t_edge": pl._t_edge, "splits": pl.splits, "t_splits": pl._t_splits, "src": su.src,
            "dst": su.dst, "e_real": pl.e_dev}


def _fresh(model, sd, cin=3, cout=1):
    from gaot_amd.model.gaot import GAOT
    m = GAOT(cin, cout, model_cfg(model))
    m.load_state_dict(sd)
    return m.to(dev()).train()


def _weights(m):
    return torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu()


# ------------------------------------------------------------------------------------------------ 1. kernel against kernel
@pytest.mark.parametrize("scales", [(1.0,), (1.0, 0.5)])
def test_indexed_compose_equals_the_host_fed_compose_exactly(scales):
    from gaot_amd import plan as P
    _, latd, _, _, store = _store(scales)
    counts = store.edge_counts
    assert len(set(counts[:, 0].tolist())) > 1                                  # unequal terms for the prefix sum
    for side, n_src, n_dst, rows, src_of, dst_of in _sides(store, latd):
        for k in range(len(scales)):
            table = store.part_table(k, side)
            assert tuple(table.shape) == (store.S, 8) and table.dtype == torch.int64 and table.is_cuda
            assert store.part_table(k, side) is table                           # built once
            for lst in INDEX_LISTS:
                total = int(counts[lst, k].sum())
                e_cap = max(store.batch_edge_capacity(B, k), P.edge_bucket(total))          # (the repeat may pass the capacity of distinct samples)
                want = _union(store, n_src, n_dst, e_cap)
                want.load([rows[i][k][P._PLAN_KEY] for i in lst], src_of(lst), dst_of(lst))
                want.refresh()
                got = _union(store, n_src, n_dst, e_cap)
                got.bind_index(table, store.S, _idx(lst), hold=store)
                got.refresh()
                for (name, a), b in zip(_outputs(got).items(), _outputs(want).values()):
                    assert torch.equal(a, b), (scales, side, k, lst, name)
                assert int(got.plan.e_dev) == total and int(got.flag) == 0, (side, k, lst)
                assert not bool((got.plan.index == POISON).any()) and not bool((got.src == POISON).any())


# ------------------------------------------------------------------------------------------------ 2. contract violations, flagged and in bounds
def test_bad_indices_and_a_short_capacity_are_flagged_and_stay_in_bounds():
    from gaot_amd import plan as P
    _, latd, _, _, store = _store((1.0,))
    S = store.S
    for side, n_src, n_dst, rows, src_of, dst_of in _sides(store, latd):
        table = store.part_table(0, side)
        # an index past the table and a negative one: clamped to S - 1 and 0, flagged
        clamped = [S - 1, 1, 0]
        e_cap = P.edge_bucket(int(store.edge_counts[clamped, 0].sum()))
        got = _union(store, n_src, n_dst, e_cap)
        got.bind_index(table, S, _idx([S + 2, 1, -1]))
        got.refresh()
        assert int(got.flag) & 1 and not int(got.flag) & 4
        want = _union(store, n_src, n_dst, e_cap)
        want.load([rows[i][0][P._PLAN_KEY] for i in clamped], src_of(clamped), dst_of(clamped))
        want.refresh()
        for (name, a), b in zip(_outputs(got).items(), _outputs(want).values()):
            assert torch.equal(a, b), (side, name)
        assert int(got.plan.index.max()) < B * n_src and int(got.plan.index.min()) >= 0
        # a capacity below the batch's edge count: flagged, truncated at the capacity, every entry a valid slot
        lst = [5, 0, 3]
        total = int(store.edge_counts[lst, 0].sum())
        short = total - 100
        got = _union(store, n_src, n_dst, short)
        got.bind_index(table, S, _idx(lst))
        got.refresh()
        pl = got.plan
        assert int(got.flag) & 4 and not int(got.flag) & 1
        assert int(pl.e_dev) == short
        assert int(pl.splits.max()) == short == int(pl.splits[-1]) and int(pl._t_splits.max()) == short == int(pl._t_splits[-1])
        assert bool((pl.splits[1:] >= pl.splits[:-1]).all()) and bool((pl._t_splits[1:] >= pl._t_splits[:-1]).all()) and int(pl.splits.min()) == 0
        assert 0 <= int(pl.index.min()) and int(pl.index.max()) < B * n_src
        assert 0 <= int(pl.edge_query.min()) and int(pl.edge_query.max()) < B * n_dst
        assert 0 <= int(pl._t_edge.min()) and int(pl._t_edge.max()) < short
        # ... and up to the cut it is the union a capacity that fits gives
        full = _union(store, n_src, n_dst, P.edge_bucket(total))
        full.bind_index(table, S, _idx(lst))
        full.refresh()
        assert int(full.flag) == 0
        assert torch.equal(pl.index, full.plan.index[:short]) and torch.equal(pl.edge_query, full.plan.edge_query[:short])
        assert torch.equal(pl.splits, full.plan.splits.clamp(max=short))
    # a table or a list of the wrong kind never reaches the kernel
    su = _union(store, store.N, store.Q, 4096)
    with pytest.raises(ValueError, match="index list"):
        su.bind_index(store.part_table(0, "encoder"), S, torch.zeros(B, dtype=torch.int64, device=dev()))
    with pytest.raises(ValueError, match="table"):
        su.bind_index(store.part_table(0, "encoder")[:, :7], S, _idx([0, 1, 2]))
    with pytest.raises(RuntimeError, match="before any load"):
        su.refresh()


# ------------------------------------------------------------------------------------------------ 3. the gather
@pytest.mark.parametrize("widths", [(3, 1, 2), (5, 3, 3)])
def test_gather_equals_indexing_exactly(widths):
    from gaot_amd.graphs import GraphBuilder
    from gaot_amd.static import SampleStore
    Cc, U, D = widths
    g = torch.Generator().manual_seed(50 + Cc)
    if D == 2:
        _, _, _, _, graphs = _store((1.0,))
    else:          # 301 points: every [N, width] block is an odd number of floats -- no 16-byte piece applies
        x = torch.stack([shell_points(301, g) for _ in range(6)]).contiguous()
        graphs = GraphBuilder().build_store(x.to(dev()), grid([6, 6, 6]).to(dev()), 0.4, [1.0])
    S, N = graphs.S, graphs.N
    assert ((N * Cc) % 4 == 0) == (D == 2)
    c, u = torch.randn(S, N, Cc, generator=g), torch.randn(S, N, U, generator=g)
    data = SampleStore(c, u, graphs=graphs)
    assert len(data) == S and data.vx
    cd, ud = c.to(dev()), u.to(dev())
    for lst in ([4], [2, 0, 2, 5, 1]):
        n = len(lst)
        x_, y_, xc = (torch.full((n, N, w), float(POISON), device=dev()) for w in (Cc, U, D))
        data.compose(_idx(lst), x_, y_, xc)
        assert torch.equal(x_, cd[lst]) and torch.equal(y_, ud[lst]) and torch.equal(xc, graphs.x_scaled[lst]), (widths, lst)
    assert data.status() == 0
    # out of range: clamped, flagged, nothing else read
    x_, y_, xc = (torch.full((2, N, w), float(POISON), device=dev()) for w in (Cc, U, D))
    data.compose(_idx([S, -3]), x_, y_, xc)
    assert data.status() == 1
    assert torch.equal(x_, cd[[S - 1, 0]]) and torch.equal(y_, ud[[S - 1, 0]]) and torch.equal(xc, graphs.x_scaled[[S - 1, 0]])
    data.clear_status()
    assert data.status() == 0
    with pytest.raises(ValueError, match="xcoord"):
        data.compose(_idx([0]), x_[:1], y_[:1])


# ------------------------------------------------------------------------------------------------ 4. replay == eager
def _epoch_batches(data, epochs=2):
    out = []
    for e in range(epochs):
        order = data.epoch_indices(e)
        out += [order[k * B:(k + 1) * B] for k in range(len(data) // B)]
    return out


def test_replay_equals_eager_bit_for_bit_with_one_capture():
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    _, latd, P_all, T_all, store = _store((1.0,))
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, seed=51)
    batches = _epoch_batches(data)
    assert len(batches) == 4 and len({tuple(b.tolist()) for b in batches}) == 4
    runs = {}
    for graph in (True, False):
        m = _fresh(model, sd)
        ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=graph)
        ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
        losses = [ts.step_samples(b if k != 1 else b.tolist()).clone() for k, b in enumerate(batches)]          # device slices, and one host list
        torch.cuda.synchronize()
        assert ts.n_captures == (1 if graph else 0) and len(ts._graph_sets) <= 1
        with pytest.raises(ValueError, match="whole batches"):
            ts.step_samples([1, 2])
        runs[graph] = (torch.stack(losses).cpu(), _weights(m))
    assert data.status() == 0
    print("[bind_samples] losses", runs[True][0].tolist())
    assert bool(torch.isfinite(runs[True][0]).all()) and len(set(runs[True][0].tolist())) == 4
    assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0], runs[False][0])
    assert torch.equal(runs[True][1], runs[False][1])


# ------------------------------------------------------------------------------------------------ 5. == the host-fed path
def test_step_samples_equals_the_host_fed_step_bit_for_bit():
    from gaot_amd import plan as P
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    latd, P_all, T_all, store = _permuted_store()
    counts = store.edge_counts[:, 0].tolist()
    assert len(set(counts)) == 1 and store.batch_edge_capacity(B, 0) == P.edge_bucket(B * counts[0])
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, seed=52)
    batches = [b.tolist() for b in _epoch_batches(data)]
    m = _fresh(model, sd)
    ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=True)
    ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    got = [ts.step_samples(b).clone() for b in batches]
    twin = _fresh(model, sd)
    tt = TrainStep(twin, lr=2e-3, weight_decay=1e-4, use_graph=True)
    feed = lambda b: dict(xcoord=store.x_scaled[b], encoder_nbrs=[store.encoder[i] for i in b], decoder_nbrs=[store.decoder[i] for i in b])
    tt.bind(P_all[batches[0]], T_all[batches[0]], latent_tokens_coord=latd, **feed(batches[0]))
    want = [tt.step(P_all[b], T_all[b], **feed(b)).clone() for b in batches]
    torch.cuda.synchronize()
    assert ts.n_captures == 1 and data.status() == 0
    assert [u.e_cap for u in ts._vx_unions[0] + ts._vx_unions[1]] == [u.e_cap for u in tt._vx_unions[0] + tt._vx_unions[1]]
    assert torch.equal(torch.stack(got), torch.stack(want)), (got, want)
    assert len(set(float(v) for v in got)) == len(got)
    assert torch.equal(_weights(m), _weights(twin))


# ------------------------------------------------------------------------------------------------ 6. against the oracle
def test_multiscale_step_samples_against_the_oracle():
    """loss and every gradient of two shuffled batches against oracle.train_step on the permuted batch, under the bars check_step applies
    (LOSS_TOL; GRAD_TOL per tensor without a floor, through grad_errors with the reference's own fp32 rounding)"""
    from oracle import gaot_oracle as O
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    scales = (1.0, 0.5)
    _, latd, P_all, T_all, store = _store(scales)
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, ocfg = make_model(3, 1, [16, 16], radius=RADIUS, seed=53, scales=list(scales))
    ocfg = dataclasses.replace(ocfg, scales=list(scales))
    m = _fresh(model, sd)
    ts = TrainStep(m, lr=0.0, weight_decay=0.0, use_graph=True)          # lr = 0: the weights stay the oracle's for the second batch
    ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    csr = lambda d: (d["neighbors_index"].cpu(), d["neighbors_row_splits"].cpu())
    for b in _epoch_batches(data, epochs=1):
        lst = b.tolist()
        batch = dict(latent=latd.cpu(), xcoord=store.x_scaled[lst].cpu(), pndata=P_all[lst].cpu(), target=T_all[lst].cpu(),
                     encoder_nbrs=[[csr(d) for d in store.encoder[i]] for i in lst], decoder_nbrs=[[csr(d) for d in store.decoder[i]] for i in lst])
        loss_ref, grads_ref = O.train_step(sd, ocfg, batch)[:2]
        loss = float(ts.step_samples(b))
        for q, v in zip(ts.bucket.params, ts.bucket.views):          # (a replay runs no Python: the gradients are in the step's flat buffer)
            q.grad = v
        e_loss = abs(loss - float(loss_ref)) / abs(float(loss_ref))
        errs = grad_errors(m, grads_ref, fp32_noise(sd, ocfg, batch, grads_ref))
        worst = max(errs, key=errs.get)
        print(f"[step_samples multiscale {lst}] loss rel {e_loss:.2e}  worst grad rel-L2 {errs[worst]:.2e} ({worst})")
        assert e_loss < LOSS_TOL, (lst, e_loss)
        assert errs[worst] < GRAD_TOL, (lst, worst, errs[worst])
    assert ts.n_captures == 1 and data.status() == 0


# ------------------------------------------------------------------------------------------------ 7. EvalStep
def test_evalstep_bind_samples_interleaved_with_training_one_capture():
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import EvalStep, TrainStep
    _, latd, P_all, T_all, store = _store((1.0,))
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, seed=54)
    batches = _epoch_batches(data)
    out = {}
    for graph in (True, False):
        m = _fresh(model, sd)
        ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=True)          # (first: its optimizer re-points the parameters at one flat buffer)
        ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
        ev = EvalStep(m, use_graph=graph)
        ev.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
        ls = []
        for k, b in enumerate(batches):
            ls.append(ev.step_samples(b).clone())
            ts.step_samples(batches[(k + 1) % len(batches)])
        torch.cuda.synchronize()
        out[graph] = (torch.stack(ls).cpu(), ev.mean_loss(), _weights(m))
        assert ev.n_captures == (1 if graph else 0) and ts.n_captures == 1 and m.training and len(ev._graph_sets) <= 1
    assert data.status() == 0
    assert torch.equal(out[True][0], out[False][0]), (out[True][0], out[False][0])
    assert out[True][1] == out[False][1] and torch.equal(out[True][2], out[False][2])
    exact = float(out[False][0].double().mean())
    assert abs(out[True][1] - exact) <= 2.0 ** -23 * exact
    assert len(set(out[True][0].tolist())) == len(batches)                     # every evaluation saw its own batch and the current weights
    # the evaluation loop that exists today (host-fed lists, unions at each batch's own bucket) on the initial weights: the same loss to rounding
    m = _fresh(model, sd)
    TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=False)
    ev = EvalStep(m, use_graph=False)
    b = batches[0].tolist()
    ev.bind(P_all[b], T_all[b], latent_tokens_coord=latd, xcoord=store.x_scaled[b], encoder_nbrs=[store.encoder[i] for i in b],
            decoder_nbrs=[store.decoder[i] for i in b])
    host = float(ev.step())
    assert abs(host - float(out[True][0][0])) < LOSS_TOL * abs(host)


# ------------------------------------------------------------------------------------------------ 8. neighbour sub-sampling on top
def test_ratio_sub_sampling_redraws_on_every_replay_of_the_indexed_step():
    from gaot_amd import ops
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    _, latd, P_all, T_all, store = _store((1.0,))
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, seed=55, sampling_strategy="ratio", sample_ratio=0.6)
    ops.seed_dropout(1234, dev())
    m = _fresh(model, sd)
    ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=True)
    ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    b = _idx([4, 1, 2])
    total = int(store.edge_counts[[4, 1, 2], 0].sum())
    losses, kept = [], []
    for _ in range(3):                                                          # the SAME samples: only the draw changes
        losses.append(float(ts.step_samples(b)))
        drops = ts._vx_unions[0][0].plan.__dict__["_drops"]
        assert len(drops) == 1
        kept.append(int(next(iter(drops.values())).e_dev))
    assert ts.n_captures == 1 and data.status() == 0
    assert all(torch.isfinite(torch.tensor(losses))), losses
    print(f"[step_samples ratio 0.6] kept edges {kept} of {total}")
    assert all(0 < k < total for k in kept) and kept[1] != kept[2]


# ------------------------------------------------------------------------------------------------ 9. fx
def test_fx_sample_store_equals_the_caller_fed_step():
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    g = torch.Generator().manual_seed(56)
    S, N = 6, 509
    coord = (torch.rand(N, 2, generator=g) * 2 - 1).to(dev())
    latd = grid([16, 16]).to(dev())
    c, u = torch.randn(S, N, 3, generator=g).to(dev()), torch.randn(S, N, 1, generator=g).to(dev())
    data = SampleStore(c, u, coord=coord)
    assert not data.vx and len(data) == S
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, precompute=False, seed=56)
    batches = [b.tolist() for b in _epoch_batches(data)][:3]
    m = _fresh(model, sd)
    ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=True)
    ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    got = [ts.step_samples(_idx(b)).clone() for b in batches]
    twin = _fresh(model, sd)
    tt = TrainStep(twin, lr=2e-3, weight_decay=1e-4, use_graph=True)
    tt.bind(c[batches[0]], u[batches[0]], latent_tokens_coord=latd, xcoord=coord)
    want = [tt.step(c[b], u[b]).clone() for b in batches]
    torch.cuda.synchronize()
    assert ts.n_captures == 1 and data.status() == 0
    assert torch.equal(torch.stack(got), torch.stack(want)), (got, want)
    assert torch.equal(_weights(m), _weights(twin))
    with pytest.raises(ValueError, match="comes from the store"):
        ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd, xcoord=coord)


def test_bind_samples_refuses_what_bind_would_not_run_on_static_unions():
    from gaot_amd.static import SampleStore
    from gaot_amd.trainer import TrainStep
    _, latd, P_all, T_all, store = _store((1.0,))
    data = SampleStore(P_all, T_all, graphs=store)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, precompute=False, seed=57)          # the module searches its own graphs
    ts = TrainStep(_fresh(model, sd), use_graph=True)
    with pytest.raises(RuntimeError, match="precompute_edges"):
        ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    model, sd, _ = make_model(3, 1, [16, 16], radius=RADIUS, seed=57)
    ts = TrainStep(_fresh(model, sd), use_graph=True)
    with pytest.raises(ValueError, match="latent grid"):
        ts.bind_samples(data, batch_size=B, latent_tokens_coord=latd * 0.5)
    with pytest.raises(RuntimeError, match="bind_samples\\(\\) first"):
        ts.step_samples([0, 1, 2])
