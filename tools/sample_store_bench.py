#!/usr/bin/env python3
"""What feeding a static vx training step from a device index list costs (DESIGN "Index-driven training steps"):
    python tools/sample_store_bench.py [--out profiles/sample_store.json] [--rounds 5] [--samples 48]
At C3's shape (NACA-like meshes of 8 192 nodes, 64 x 64 latent grid, radius 0.033, 3 channels in, 1 out; a split of 48 meshes whose point
density varies as bench.py's C3 dataset does, graphs in one device GraphStore), for batch 16 and batch 4, over the compositions of one
shuffled epoch, two ways of feeding the same model's TrainStep from that one store:
  (a) step_samples(order[kB:(k+1)B])          -- bind_samples: B indices copied, one replay
  (b) step(P[b], T[b], xcoord=store.x_scaled[b], encoder_nbrs=[store.encoder[i] ...], decoder_nbrs=[...])          -- the host-fed loop
Both are warmed up (over every composition, so (b) has captured every bucket it will meet) and timed in alternation in ONE process: a
host clock around windows of whole steps lasting at least 0.5 s that end in a device synchronise.  Best, median and every window are
reported, with the captures on each side and how much the single worst-case capacity pads: e_cap / mean batch edges.
Single-box numbers.  Needs a GPU; prints and writes one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace as NS

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from gaot_amd.graphs import GraphBuilder
from gaot_amd.static import SampleStore
from gaot_amd.trainer import TrainStep
from tests._workloads import grid, naca_points

N = 8192


def build_model(dev):
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import TransformerConfig
    from gaot_amd.model.layers.magno import MAGNOConfig
    torch.manual_seed(0)
    mc = MAGNOConfig(radius=bench.RADIUS, lifting_channels=bench.C_LIFT, precompute_edges=True)
    return GAOT(3, 1, NS(args=NS(magno=mc, transformer=TransformerConfig(patch_size=bench.PATCH, hidden_size=bench.HIDDEN)),
                         latent_tokens_size=bench.LATENT)).to(dev).train()


def alternate(legs, rounds, warm, after_warm, min_seconds=0.5):
    ms = {k: [] for k in legs}
    for fn in legs.values():          # warm-up: captures (every bucket of the host-fed side), plans, allocator
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    after_warm()
    order = list(legs)
    for rnd in range(rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:
            fn = legs[k]
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(10):
                    fn()
                n += 10
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= min_seconds:
                    break
            ms[k].append(dt / n * 1e3)
    return {k: {"best": min(v), "median": statistics.median(v), "range": [min(v), max(v)], "windows": v} for k, v in ms.items()}


def one_batch_size(B, data, store, latd, P_all, T_all, rounds, dev):
    order = data.epoch_indices(0)
    comps = [order[k * B:(k + 1) * B] for k in range(len(data) // B)]
    host = [c.tolist() for c in comps]
    ts_idx = TrainStep(build_model(dev), lr=8e-4, weight_decay=1e-5)
    ts_idx.bind_samples(data, batch_size=B, latent_tokens_coord=latd)
    ts_host = TrainStep(build_model(dev), lr=8e-4, weight_decay=1e-5)
    feed = lambda b: dict(xcoord=store.x_scaled[b], encoder_nbrs=[store.encoder[i] for i in b], decoder_nbrs=[store.decoder[i] for i in b])
    ts_host.bind(P_all[host[0]], T_all[host[0]], latent_tokens_coord=latd, **feed(host[0]))
    count = [0, 0]

    def leg_idx():
        ts_idx.step_samples(comps[count[0] % len(comps)]); count[0] += 1

    def leg_host():
        b = host[count[1] % len(host)]; count[1] += 1
        ts_host.step(P_all[b], T_all[b], **feed(b))
    warm_caps = {}
    ms = alternate({"step_samples": leg_idx, "step_host_fed": leg_host}, rounds, max(12, 3 * len(comps)),
                   lambda: warm_caps.update(step_samples=ts_idx.n_captures, step_host_fed=ts_host.n_captures))
    counts = store.edge_counts[:, 0]
    totals = [int(counts[b].sum()) for b in host]
    cap = store.batch_edge_capacity(B, 0)
    from gaot_amd.plan import edge_bucket
    a, b = ms["step_samples"]["median"], ms["step_host_fed"]["median"]
    return {"batch": B, "compositions": len(comps), "ms_per_step": ms,
            "captures": {"step_samples": ts_idx.n_captures, "step_host_fed": ts_host.n_captures, "host_fed_graph_sets": len(ts_host._graph_sets),
                         "after_warm_up": warm_caps, "what": "captures made in all; after_warm_up: before the first timed window (a difference = re-captures "
                                                             "inside the timed windows: more bucket combinations than TrainStep.MAX_GRAPH_SETS keeps)"},
            "edges": {"e_cap_indexed": cap, "mean_batch_edges": sum(totals) / len(totals), "min_batch_edges": min(totals), "max_batch_edges": max(totals),
                      "e_cap_over_mean_batch_edges": cap / (sum(totals) / len(totals)),
                      "host_fed_buckets": sorted({edge_bucket(t) for t in totals}),
                      "mean_host_fed_bucket_over_mean_batch_edges": sum(edge_bucket(t) for t in totals) / sum(totals)},
            "host_fed_ms_over_step_samples_ms": b / a, "step_samples_faster": a < b, "status_flag": data.status()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sample_store.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_store_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    S = args.samples
    g = torch.Generator().manual_seed(0)
    # bench.py's C3 dataset: the first 16 meshes at one point density, the others spread it a little, as a family of geometries does
    x_all = torch.stack([naca_points(N, g, 0.15 if i < 16 else 0.12 + 0.06 * (i % 8) / 7) for i in range(S)])
    P_all, T_all = torch.randn(S, N, 3, generator=g).to(dev), torch.randn(S, N, 1, generator=g).to(dev)
    latd = grid(bench.LATENT).to(dev)
    store = GraphBuilder().build_store(x_all.to(dev), latd, bench.RADIUS, [1.0])
    data = SampleStore(P_all, T_all, graphs=store)
    counts = store.edge_counts[:, 0]
    out = {"device": torch.cuda.get_device_name(0), "single_box": True, "rounds": args.rounds, "window_seconds_at_least": 0.5,
           "config": f"C3 shape: {S} NACA-like meshes of {N} nodes, {bench.LATENT[0]} x {bench.LATENT[1]} latent grid, radius {bench.RADIUS}, 3 in / 1 out; "
                     f"edges per sample {int(counts.min())} .. {int(counts.max())}; graphs {store.nbytes / 1e6:.0f} MB and fields "
                     f"{(P_all.numel() + T_all.numel()) * 4 / 1e6:.0f} MB resident",
           "results": [one_batch_size(B, data, store, latd, P_all, T_all, args.rounds, dev) for B in args.batches]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
