"""-m gpu: the dataset-level graph builder on the device (gaot_amd/graphs.py GraphStore, csrc/graph_store.hip).

Every comparison is torch.equal.  Pinned below:
  * lists: both directions at every scale equal the per-sample device NeighborSearch on store.x_scaled[s], the host's exact pairwise search
    (and, in 2-D, oracle.radius_csr(exact=True)); the decoder is the transpose of the encoder; x_scaled equals the torch rescale expression;
    edge_counts equal the list lengths -- on samples with ties at dist == r (bounding-box corners land exactly on latent tokens), empty rows,
    a constant coordinate, one very long row, NACA-shaped clouds, 3-D clouds, and sample sets whose rows cross both thresholds of the row sort
    (32 and 4096 entries) in either direction;
  * plans: the plan attached to every dict equals a GeometryPlan built the old way, array for array, and is found by has_plan at first sight;
  * determinism: two builds give equal bytes in every arena, also when every allocation (scratch included) held 0x7f bytes beforehand;
  * training: four shuffled TrainStep steps with graph replay fed from the store's dicts equal, bit for bit, a twin fed from per-sample
    NeighborSearch dicts whose plans were built up front; the store's unions are composed from plans (raw is False) from the first step;
  * a single sample's dicts go through an ordinary B = 1 vx forward and give what the old-way dicts give.
"""
import functools

import pytest
import torch

from tests._workloads import grid, naca_points, shell_points, uniform_points
from tests.test_configs_gpu import dev, make_model

pytestmark = pytest.mark.gpu

SORT_SHORT, SORT_LDS = 32, 4096          # the row-length thresholds csrc/graph_store.hip states (segsort.h on int64)


def _corners(d):
    return torch.tensor([[(-1.0 if (i >> k) & 1 == 0 else 1.0) for k in range(d)] for i in range(1 << d)])


def _spacing(lat_axis_n):
    ax = torch.linspace(-1.0, 1.0, lat_axis_n)
    return float(ax[1] - ax[0])          # the fp32 grid spacing


def _case_2d():
    g = torch.Generator().manual_seed(31)
    lat = grid([16, 16])
    r = _spacing(16)
    c = _corners(2)
    token = lat[5 * 16 + 9]
    ang, rad = torch.rand(296, generator=g) * 6.2832, torch.rand(296, generator=g).sqrt() * 0.4 * r
    samples = [torch.cat([c, uniform_points(296, 2, g)]),
               torch.cat([torch.tensor([[-1.0, 0.3], [1.0, 0.3]]), torch.stack([torch.rand(298, generator=g) * 2 - 1, torch.full((298,), 0.3)], -1)]),
               torch.cat([c, token + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1)])]
    samples += [torch.cat([c, naca_points(296, g, 0.15)]) for _ in range(3)]
    # raw coordinates far from [-1, 1]: rescale has work to do, and maps every bounding-box corner exactly onto a corner token
    x = torch.stack(samples) * torch.tensor([2.5, 0.8]) + torch.tensor([3.0, -1.0])
    return x.contiguous(), lat, r, [1.0, 2.0]


def _case_thresholds():
    """N = 5000: sample 0 is one cluster on a token (encoder rows beyond 4096 entries, all others at most a corner), sample 1 a smaller cluster
    in a uniform cloud (encoder rows between the thresholds)"""
    g = torch.Generator().manual_seed(32)
    lat = grid([16, 16])
    r = _spacing(16)
    c = _corners(2)

    def cluster(n, tok):
        ang, rad = torch.rand(n, generator=g) * 6.2832, torch.rand(n, generator=g).sqrt() * 0.3 * r
        return lat[tok] + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1)
    x = torch.stack([torch.cat([c, cluster(4996, 7 * 16 + 6)]), torch.cat([c, cluster(600, 3 * 16 + 11), uniform_points(4396, 2, g)])])
    return (x * 1.5 - 0.25).contiguous(), lat, r, [1.0, 2.0]


def _case_dense_latent():
    """few points against 80 x 80 tokens: DECODER rows beyond 4096 entries (radius 3 reaches every token) and between the thresholds"""
    g = torch.Generator().manual_seed(33)
    x = torch.stack([torch.cat([_corners(2), uniform_points(36, 2, g)]) for _ in range(2)])
    return (x * 0.5 + 2.0).contiguous(), grid([80, 80]), 3.0, [1.0, 0.05]


def _case_3d():
    g = torch.Generator().manual_seed(34)
    x = torch.stack([torch.cat([_corners(3), shell_points(392, g)]) for _ in range(3)])
    return (x * torch.tensor([1.0, 3.0, 0.25]) + torch.tensor([0.5, -2.0, 7.0])).contiguous(), grid([6, 6, 6]), _spacing(6), [1.0, 2.0]


CASES = {"d2": _case_2d, "thresholds": _case_thresholds, "dense_latent": _case_dense_latent, "d3": _case_3d}


@functools.lru_cache(maxsize=None)
def _built(name):
    """(inputs, the device store, the host reference lists) of a case: built once, shared by the tests, never modified"""
    from gaot_amd.graphs import GraphBuilder, rescale
    from gaot_amd.model.layers.utils.neighbor_search import _exact_pairwise
    x, lat, radius, scales = CASES[name]()
    store = GraphBuilder().build_store(x.to(dev()), lat.to(dev()), radius, scales)
    xs_host = torch.stack([rescale(s) for s in x])
    ref = []
    for s in range(x.shape[0]):
        row = []
        for sc in scales:
            r = torch.tensor(float(radius * sc), dtype=torch.float32)
            row.append((_exact_pairwise(xs_host[s], lat, r, False), _exact_pairwise(lat, xs_host[s], r, False)))
        ref.append(row)
    return x, lat, radius, scales, store, xs_host, ref


def _rows(d):
    sp = d["neighbors_row_splits"]
    return (sp[1:] - sp[:-1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_equal_per_sample_search_exact_pairwise_and_transpose(name):
    from gaot_amd.graphs import rescale
    from gaot_amd.model.layers.utils.neighbor_search import NeighborSearch
    x, lat, radius, scales, store, xs_host, ref = _built(name)
    S, N, Q = x.shape[0], x.shape[1], lat.shape[0]
    latd = lat.to(dev())
    assert store.x_scaled.dtype == torch.float32 and tuple(store.x_scaled.shape) == (S, N, x.shape[2])
    assert torch.equal(store.x_scaled.cpu(), xs_host)                                                        # the torch expression on the host ...
    assert torch.equal(store.x_scaled, torch.stack([rescale(s) for s in x.to(dev())]))                     # ... and on the device
    assert float(store.x_scaled.min()) == -1.0 and float(store.x_scaled.max()) == 1.0
    assert tuple(store.edge_counts.shape) == (S, len(scales)) and store.edge_counts.dtype == torch.int64 and not store.edge_counts.is_cuda
    search = NeighborSearch("auto")
    for s in range(S):
        for k, sc in enumerate(scales):
            r = float(radius * sc)
            enc, dec = store.encoder[s][k], store.decoder[s][k]
            for d in (enc, dec):
                assert d["neighbors_index"].dtype == torch.int64 and d["neighbors_row_splits"].dtype == torch.int64 and d["neighbors_index"].is_cuda
            assert int(store.edge_counts[s, k]) == enc["neighbors_index"].numel() == dec["neighbors_index"].numel()
            # the per-sample device search on the very coordinates the store holds
            for got, want in ((enc, search(store.x_scaled[s], latd, r)), (dec, search(latd, store.x_scaled[s], r))):
                assert torch.equal(got["neighbors_row_splits"], want["neighbors_row_splits"]), (name, s, k)
                assert torch.equal(got["neighbors_index"], want["neighbors_index"]), (name, s, k)
            # the host's exact pairwise search
            for got, want in ((enc, ref[s][k][0]), (dec, ref[s][k][1])):
                assert torch.equal(got["neighbors_row_splits"].cpu(), want["neighbors_row_splits"]), (name, s, k)
                assert torch.equal(got["neighbors_index"].cpu(), want["neighbors_index"]), (name, s, k)
            # decoder == transpose of the encoder: (token, point) pairs re-sorted by (point, token)
            esp, eidx = enc["neighbors_row_splits"].cpu(), enc["neighbors_index"].cpu()
            tok = torch.repeat_interleave(torch.arange(Q), esp[1:] - esp[:-1])
            order = torch.argsort(eidx * Q + tok)
            assert torch.equal(dec["neighbors_index"].cpu(), tok[order])
            assert torch.equal(dec["neighbors_row_splits"].cpu()[1:], torch.cumsum(torch.bincount(eidx, minlength=N), 0))
            assert int(dec["neighbors_row_splits"][0]) == 0 and int(enc["neighbors_row_splits"][0]) == 0


def test_2d_case_has_ties_empty_rows_and_agrees_with_the_oracle():
    from oracle import gaot_oracle as O
    x, lat, radius, scales, store, xs_host, ref = _built("d2")
    ties = 0
    for s in range(x.shape[0]):
        assert bool((xs_host[s][:, None, :] == lat[None, :, :]).all(-1).any())                         # corners sit exactly on tokens
        for k, sc in enumerate(scales):
            r = float(radius * sc)
            dist = (lat[:, None, :] - xs_host[s][None, :, :]).square().sum(-1).sqrt()
            ties += int((dist == torch.tensor(r, dtype=torch.float32)).sum())
            for got, want in ((store.encoder[s][k], O.radius_csr(xs_host[s], lat, r, exact=True)), (store.decoder[s][k], O.radius_csr(lat, xs_host[s], r, exact=True))):
                assert torch.equal(got["neighbors_index"].cpu(), want[0]) and torch.equal(got["neighbors_row_splits"].cpu(), want[1]), (s, k)
    empty = [sum(int((_rows(store.encoder[s][k]) == 0).sum()) for s in range(x.shape[0])) for k in range(2)]
    print(f"[graph store d2] pairs at exactly dist == r: {ties}; empty encoder rows per scale: {empty}")
    assert ties >= 8 and empty[0] >= 10                                                                # what the issue asks of the geometry
    assert (ties, empty) == (90, [932, 667])                                                           # what THIS point set gives: a change in the geometry helpers shows
    # sample 1 (constant coordinate -> the zero-range branch): every point at y = -1; sample 2: one long row, hundreds of empty ones
    assert bool((store.x_scaled[1, :, 1] == -1.0).all())
    rows = _rows(store.encoder[2][0])
    assert int(rows.max()) >= 296 and int((rows == 0).sum()) >= 200


def test_row_lengths_cross_every_threshold_of_the_row_sort():
    """csrc/graph_store.hip sorts rows of <= 32 entries by one thread, of 33 .. 4096 by a workgroup in LDS, longer ones against global memory"""
    def bands(name, side):
        rows = torch.cat([_rows(d) for per_sample in getattr(_built(name)[4], side) for d in per_sample]).cpu()
        return (bool(((rows > 0) & (rows <= SORT_SHORT)).any()), bool(((rows > SORT_SHORT) & (rows <= SORT_LDS)).any()), bool((rows > SORT_LDS).any()))
    assert bands("thresholds", "encoder") == (True, True, True)
    assert bands("dense_latent", "decoder")[1:] == (True, True) and bands("d2", "decoder")[0]


@pytest.mark.parametrize("name", ["d2", "d3", "thresholds"])
def test_attached_plans_equal_plans_built_the_old_way(name):
    from gaot_amd import plan as P
    x, lat, radius, scales, store, _, _ = _built(name)
    N, Q = x.shape[1], lat.shape[0]
    for s in range(x.shape[0]):
        for k in range(len(scales)):
            for d, n_src in ((store.encoder[s][k], N), (store.decoder[s][k], Q)):
                assert P.has_plan(d, n_src)                                                              # before any forward
                got = d[P._PLAN_KEY]
                assert P.plan_for(d, n_src, validate="lazy") is got
                old = P.GeometryPlan(d["neighbors_index"].clone(), d["neighbors_row_splits"].clone(), n_src)
                E = old.E
                assert (got.Q, got.E, got.n_src) == (old.Q, old.E, old.n_src)
                for arr in ("index", "edge_query", "t_edge"):
                    assert getattr(got, arr).dtype == torch.int32 and getattr(got, arr).numel() == max(E, 1)
                    assert torch.equal(getattr(got, arr)[:E], getattr(old, arr)[:E]), (name, s, k, arr)
                assert torch.equal(got.splits, old.splits) and torch.equal(got.t_splits, old.t_splits)
                assert torch.equal(got.deg, old.deg)
                assert (got.max_deg, got.max_t_deg) == (old.max_deg, old.max_t_deg)
                assert got._src_id == (id(d["neighbors_index"]), d["neighbors_index"]._version)
    # a full plan, not a table row: the arrays derived from it equal the old plan's
    latd = lat.to(dev())
    # (samples past the first: their views start at odd 4-byte offsets inside the arenas, unlike a fresh allocation)
    last = x.shape[0] - 1
    assert name != "d2" or int(store.arenas(0)["offsets"][1]) % 4 != 0
    for d, src, qry in ((store.encoder[1][0], store.x_scaled[1], latd), (store.decoder[last][1], latd, store.x_scaled[last]),
                        (store.encoder[0][0], store.x_scaled[0], latd)):
        got = d[P._PLAN_KEY]
        old = P.GeometryPlan(d["neighbors_index"].clone(), d["neighbors_row_splits"].clone(), src.shape[0])
        assert torch.equal(got.edge_features(src, qry), old.edge_features(src, qry))
        assert torch.equal(got.cosine_attention(src, qry)[:got.E], old.cosine_attention(src, qry)[:old.E])
        assert torch.equal(got.geo_stats(src, qry), old.geo_stats(src, qry))
        assert torch.equal(got.inv_deg_edge, old.inv_deg_edge)
        assert torch.equal(got.index_long, old.index_long) and torch.equal(got.edge_query_long, old.edge_query_long)


def _arena_bytes(store, scales):
    out = [store.x_scaled]
    for k in range(len(scales)):
        a = store.arenas(k)
        total = int(a["offsets"][-1])
        out += [a[n] for n in ("enc_splits", "dec_splits", "enc_splits32", "dec_splits32", "offsets")]
        out += [a[n][:total] for n in ("enc_index", "dec_index", "enc_index32", "dec_index32", "enc_edge_query", "dec_edge_query", "enc_t_edge", "dec_t_edge")]
    return out


@pytest.mark.parametrize("name", ["d2", "thresholds", "d3"])
def test_two_builds_give_equal_bytes_whatever_the_scratch_held(name, monkeypatch):
    from gaot_amd import graphs as G
    x, lat, radius, scales, store, _, _ = _built(name)
    first = _arena_bytes(store, scales)
    again = G.GraphBuilder().build_store(x.to(dev()), lat.to(dev()), radius, scales)

    def filled(*shape, dtype, device):          # every allocation of the build, scratch included, holds 0x7f bytes before the kernels run
        t = torch.empty(*shape, dtype=dtype, device=device)
        t.view(torch.uint8).fill_(0x7f)
        return t
    monkeypatch.setattr(G, "_alloc", filled)
    poisoned = G.GraphBuilder().build_store(x.to(dev()), lat.to(dev()), radius, scales)
    monkeypatch.undo()
    assert poisoned.arenas(0)["enc_index"][-1].item() == 0x7f7f7f7f7f7f7f7f                       # (the slack entry past the lists: the fill was in effect)
    for other in (again, poisoned):
        for a, b in zip(first, _arena_bytes(other, scales)):
            assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(store.edge_counts, poisoned.edge_counts) and store.nbytes == again.nbytes > 0


def test_a_part_of_the_split_builds_the_same_samples_and_bad_inputs_are_refused():
    """(the launch count is constant in S by construction -- S appears only in grid dimensions of csrc/graph_store.hip -- and
    `store.launches` is counted from that code, so nothing is asserted about it here)"""
    from gaot_amd import graphs as G
    x, lat, radius, scales, store, _, _ = _built("d2")
    part = G.GraphBuilder().build_store(x[:2].to(dev()), lat.to(dev()), radius, scales)
    for k in range(len(scales)):
        assert torch.equal(part.encoder[1][k]["neighbors_index"], store.encoder[1][k]["neighbors_index"])
        assert torch.equal(part.decoder[0][k]["neighbors_row_splits"], store.decoder[0][k]["neighbors_row_splits"])
    # [S, 1, N, d] is the same split
    four = G.GraphBuilder().build_store(x[:2, None].to(dev()), lat.to(dev()), radius, scales)
    assert torch.equal(four.x_scaled, part.x_scaled) and torch.equal(four.edge_counts, part.edge_counts)
    with pytest.raises(ValueError, match="Unexpected coordinate shape"):
        G.GraphBuilder().build_store(x[0].to(dev()), lat.to(dev()), radius, scales)
    with pytest.raises(ValueError, match="same device"):
        G.GraphBuilder().build_store(x.to(dev()), lat, radius, scales)


def _training_data():
    g = torch.Generator().manual_seed(41)
    nS, N = 6, 512
    x = torch.stack([naca_points(N, g, 0.15) for _ in range(nS)]) * torch.tensor([1.7, 0.6]) + torch.tensor([0.4, 2.0])
    P_all, T_all = torch.randn(nS, N, 3, generator=g), torch.randn(nS, N, 1, generator=g)
    return x.contiguous(), grid([16, 16]), P_all, T_all


def _old_way_dicts(store, latd, radius, plan=True):
    from gaot_amd import plan as P
    from gaot_amd.model.layers.utils.neighbor_search import NeighborSearch
    search = NeighborSearch("auto")
    N, Q = store.x_scaled.shape[1], latd.shape[0]
    enc = [[search(store.x_scaled[s], latd, radius)] for s in range(store.x_scaled.shape[0])]
    dec = [[search(latd, store.x_scaled[s], radius)] for s in range(store.x_scaled.shape[0])]
    if plan:
        for row in enc:
            P.plan_for(row[0], N)
        for row in dec:
            P.plan_for(row[0], Q)
    return enc, dec


def test_trainstep_from_the_store_equals_the_twin_fed_from_per_sample_searches():
    from gaot_amd.graphs import GraphBuilder
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.trainer import TrainStep
    from tests.test_configs_gpu import model_cfg
    radius, B, steps = 0.133, 3, 4
    x, lat, P_all, T_all = _training_data()
    nS = x.shape[0]
    latd = lat.to(dev())
    model, sd, _ = make_model(3, 1, [16, 16], radius=radius, seed=21)
    store = GraphBuilder().build_store(x.to(dev()), latd, radius, [1.0])
    g = torch.Generator().manual_seed(5)
    batches = [torch.randperm(nS, generator=g)[:B].tolist() for _ in range(steps)]
    runs = {}
    for which in ("store", "twin"):
        enc, dec = (store.encoder, store.decoder) if which == "store" else _old_way_dicts(store, latd, radius)
        m = GAOT(3, 1, model_cfg(model))
        m.load_state_dict(sd)
        m.to(dev()).train()
        ts = TrainStep(m, lr=2e-3, weight_decay=1e-4, use_graph=True)
        b0 = batches[0]
        ts.bind(P_all[b0].to(dev()), T_all[b0].to(dev()), latent_tokens_coord=latd, xcoord=store.x_scaled[b0], encoder_nbrs=[enc[i] for i in b0],
                decoder_nbrs=[dec[i] for i in b0])
        losses, raw_first = [], None
        for b in batches:
            losses.append(ts.step(P_all[b].to(dev()), T_all[b].to(dev()), xcoord=store.x_scaled[b], encoder_nbrs=[enc[i] for i in b],
                                  decoder_nbrs=[dec[i] for i in b]).clone())
            if raw_first is None:
                unions = list(m.encoder._static_unions.values()) + list(m.decoder._static_unions.values())
                raw_first = [su.raw for su in unions]
        torch.cuda.synchronize()
        runs[which] = (torch.stack(losses).cpu(), torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu(), raw_first, len(ts._graph_sets))
    (ls, ws, raw_s, sets_s), (lt, wt, _, _) = runs["store"], runs["twin"]
    assert len(raw_s) >= 2 and all(r is False for r in raw_s)                       # composed from the attached plans on the very first step
    assert 1 <= sets_s <= TrainStep.MAX_GRAPH_SETS
    assert bool(torch.isfinite(ls).all())
    assert torch.equal(ls, lt), (ls, lt)
    assert torch.equal(ws, wt)


def test_single_sample_dicts_through_an_ordinary_vx_forward():
    from gaot_amd.graphs import GraphBuilder
    radius = 0.133
    x, lat, P_all, _ = _training_data()
    latd = lat.to(dev())
    model, _, _ = make_model(3, 1, [16, 16], radius=radius, seed=22)
    model.to(dev())
    store = GraphBuilder().build_store(x.to(dev()), latd, radius, [1.0])
    enc, dec = _old_way_dicts(store, latd, radius)
    s = 4
    p = P_all[s:s + 1].to(dev())
    out = {}
    for mode in ("eval", "train"):
        model.train(mode == "train")
        for which, (e, d) in (("store", (store.encoder, store.decoder)), ("old", (enc, dec))):
            with torch.set_grad_enabled(mode == "train"):
                y = model(pndata=p, latent_tokens_coord=latd, xcoord=store.x_scaled[s:s + 1], encoder_nbrs=[e[s]], decoder_nbrs=[d[s]])
            out[(mode, which)] = y.detach().clone()
        assert bool(torch.isfinite(out[(mode, "store")]).all())
        assert torch.equal(out[(mode, "store")], out[(mode, "old")]), mode
