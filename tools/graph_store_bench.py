#!/usr/bin/env python3
"""What building a vx dataset's graphs costs (DESIGN "GraphBuilder on the device"):
    python tools/graph_store_bench.py [--out profiles/graph_store.json] [--windows 5] [--window-seconds 0.3]
At C3's shape (NACA-like meshes of 8 192 nodes, a 64 x 64 latent grid, radius 0.033), for scales [1.0] and [1.0, 2.0] and S = 8 and 64 samples:
  * `store`: graphs.GraphBuilder().build_store(...) -- batched rescale, count, ONE readback, fill; every dict leaves with its plan;
  * `loop`: the path a user had before -- per sample the rescale expression as torch ops, NeighborSearch both ways per scale, and
    plan.plan_for on every dict (what training needs before it can compose unions from plans).
Both sides are warmed up and timed in alternation in ONE process, several windows per side (each of whole builds for at least
--window-seconds), a host clock around windows that end in a device synchronise; best, median, range and every window are reported, with
the per-sample cost, the store's bytes and its launch count.
Single-box numbers.  Needs a GPU; prints and writes one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gaot_amd import graphs as G
from gaot_amd import plan as P
from gaot_amd.model.layers.utils.neighbor_search import NeighborSearch
from tests._workloads import grid, naca_points

N, LATENT, RADIUS = 8192, [64, 64], 0.033


def loop_build(x, lat, scales):
    search = NeighborSearch("auto")
    n, q = x.shape[1], lat.shape[0]
    enc, dec, xs_all = [], [], []
    for s in range(x.shape[0]):
        xs = G.rescale(x[s])
        xs_all.append(xs)
        e = [search(xs, lat, RADIUS * sc) for sc in scales]
        d = [search(lat, xs, RADIUS * sc) for sc in scales]
        for nb in e:
            P.plan_for(nb, n)
        for nb in d:
            P.plan_for(nb, q)
        enc.append(e)
        dec.append(d)
    return enc, dec, xs_all


def window(fn, min_seconds):
    """ms per build over a window of whole builds lasting at least `min_seconds`, ended by a device synchronise"""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        keep = fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            break
    del keep
    return dt / n * 1e3, n


def summarise(v):
    return {"best": min(v), "median": statistics.median(v), "range": [min(v), max(v)], "windows": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "graph_store.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_store_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    x_all = torch.stack([naca_points(N, g, 0.15) for _ in range(64)]).to(dev)
    lat = grid(LATENT).to(dev)
    builder = G.GraphBuilder()
    out = {"device": torch.cuda.get_device_name(0), "single_box": True, "windows_per_side": args.windows, "window_seconds": args.window_seconds,
           "config": f"C3 shape: NACA-like meshes of {N} nodes, {LATENT[0]} x {LATENT[1]} latent grid, radius {RADIUS}",
           "what": "ms per build of the whole split; store = GraphBuilder.build_store, loop = per-sample rescale (torch ops) + NeighborSearch both ways "
                   "+ plan_for on every dict; alternating windows, host clock around windows that end in a device synchronise",
           "cases": {}}
    for scales in ([1.0], [1.0, 2.0]):
        for S in (8, 64):
            x = x_all[:S].contiguous()
            legs = {"store": lambda: builder.build_store(x, lat, RADIUS, scales), "loop": lambda: loop_build(x, lat, scales)}
            for fn in legs.values():          # warm-up: allocator, library, first-use paths
                window(fn, 0.1)
            ms, builds = {k: [] for k in legs}, {}
            for w in range(args.windows):
                for k in (("store", "loop") if w % 2 == 0 else ("loop", "store")):
                    t, builds[k] = window(legs[k], args.window_seconds)
                    ms[k].append(t)
            store = legs["store"]()
            enc, dec, xs = legs["loop"]()
            same = all(torch.equal(store.encoder[s][k]["neighbors_index"], enc[s][k]["neighbors_index"])
                       and torch.equal(store.decoder[s][k]["neighbors_row_splits"], dec[s][k]["neighbors_row_splits"])
                       and torch.equal(store.x_scaled[s], xs[s]) for s in (0, S - 1) for k in range(len(scales)))
            case = {"store_ms": summarise(ms["store"]), "loop_ms": summarise(ms["loop"]),
                    "store_us_per_sample": statistics.median(ms["store"]) / S * 1e3, "loop_us_per_sample": statistics.median(ms["loop"]) / S * 1e3,
                    "loop_over_store": statistics.median(ms["loop"]) / statistics.median(ms["store"]),
                    "store_nbytes": store.nbytes, "store_launches": store.launches, "host_readbacks_store": 1,
                    "store_launches_what": "kernels of the C entry points, counted from their code (graphs.LAUNCHES_*), not measured; per scale the "
                                           "build also issues two torch subtractions and one host-to-device copy",
                    "edges_per_scale": store.edge_counts.sum(0).tolist(), "equal_bits_to_loop": bool(same), "builds_in_last_window": builds}
            out["cases"][f"S{S}_scales{len(scales)}"] = case
            del store, enc, dec, xs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
