#!/usr/bin/env python3
"""What feeding a sequential (time-pair) training step from the device costs (DESIGN "Sequential training on the device"):
    python tools/seq_pairs_bench.py [--out profiles/seq_pairs.json] [--rounds 5]
At C4's shape (16 384 nodes, batch 4, u(2) + 2 time columns in, 2 out, stepper 'time_der'; 32 resident samples x 21 time steps, 28 pairs):
  * the compose launch alone (gaot_seq_pairs_compose into static buffers, a new index list per call): device events around back-to-back
    calls from Python, and around replays of ONE hipGraph holding 64 such launches (the device's own cost per launch); the bytes the
    algorithm needs over the latter; next to it the same batch through torch ops on the device (`batch_torch`)
  * TrainStep ms/step under `step_pairs` (index slices of one uploaded epoch order) against the same model under `TrainStep.step(x, y)`
    fed (a) by a host DataLoader over an equivalent host dataset (the items built per index on the CPU by torch expressions, default
    collate, pinned memory, non-blocking H2D) and (b) by `batch_torch` on the device.  The legs are warmed up and timed in alternation in
    ONE process, a host clock around windows that end in a device synchronise; best, median and every round are reported.
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
from gaot_amd.sequential import PairStore
from gaot_amd.trainer import TrainStep
from tests._workloads import grid

COPY_RATE_GBPS = 6290.0          # streaming copy rate measured on the MI355X (the share below is against this, not the 8 TB/s spec)
S, T, U, B = 32, 21, 2, 4


class HostPairs(torch.utils.data.Dataset):
    """the reference loader's work per item, on the CPU: one (input, target) pair per flat index"""

    def __init__(self, store):
        self.store = store

    def __len__(self):
        return len(self.store)

    def __getitem__(self, i):
        x, y = self.store.batch_torch([i], check=False)
        return x[0], y[0]


def build_model(dev):
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import TransformerConfig
    from gaot_amd.model.layers.magno import MAGNOConfig
    torch.manual_seed(0)
    mc = MAGNOConfig(radius=bench.RADIUS, lifting_channels=bench.C_LIFT)
    return GAOT(U + 2, U, NS(args=NS(magno=mc, transformer=TransformerConfig(patch_size=bench.PATCH, hidden_size=bench.HIDDEN)),
                             latent_tokens_size=bench.LATENT)).to(dev).train()


def per_call_us(fn, min_ms=300.0):
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_ms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(50):
            fn(reps + i)
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        reps += 50
    return total / reps * 1e3


def alternate(legs, rounds, min_seconds=0.5):
    ms = {k: [] for k in legs}
    for fn in legs.values():          # warm-up: captures, plans, allocator, loader workers
        for _ in range(12):
            fn()
    torch.cuda.synchronize()
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
    return {k: {"best": min(v), "median": statistics.median(v), "rounds": v} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seq_pairs.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq_pairs_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    N = bench.N_NODES
    g = torch.Generator().manual_seed(4)
    u = torch.randn(S, 1, N, U, generator=g) + 0.1 * torch.randn(S, T, N, U, generator=g).cumsum(dim=1)
    t = torch.linspace(0.0, 1.0, T)
    stats = {"u": {"mean": torch.tensor([0.1, -0.2]), "std": torch.tensor([1.5, 0.7])},
             "der": {"mean": torch.tensor([-0.05, 0.03]), "std": torch.tensor([0.8, 1.1])},
             "start_time": {"mean": 0.4, "std": 0.25}, "time_diffs": {"mean": 0.1, "std": 0.05}}
    kw_store = dict(max_time_diff=14, time_step=2, stepper_mode="time_der")
    store = PairStore(u, None, t, stats, device=dev, **kw_store)
    host = PairStore(u, None, t, stats, device="cpu", **kw_store)
    W = store.input_width()
    order = store.epoch_indices(0)
    n_batches = order.numel() // B
    out = {"device": torch.cuda.get_device_name(0), "single_box": True, "rounds": args.rounds,
           "config": f"C4 shape: {N} nodes, batch {B}, in = u({U}) + 2 time columns, out {U}, stepper time_der; {S} samples x {T} time steps resident "
                     f"({u.numel() * 4 / 1e6:.0f} MB), {store.n_pairs} pairs, {len(store)} items"}

    # ---- the composition alone
    x = torch.empty(B, N, W, device=dev)
    y = torch.empty(B, N, U, device=dev)
    sl = lambda i: order[(i % n_batches) * B:(i % n_batches) * B + B]
    hip_us = per_call_us(lambda i: store.compose(sl(i), x, y))
    aten_us = per_call_us(lambda i: store.batch_torch(sl(i), check=False))
    # the same launch without the host in the way: 64 of them (64 index lists) captured back to back in one hipGraph, the replay timed
    store.compose(sl(0), x, y)
    torch.cuda.synchronize()
    chain = torch.cuda.CUDAGraph()
    with torch.cuda.graph(chain):
        for i in range(64):
            store.compose(sl(i), x, y)
    graph_us = per_call_us(lambda i: chain.replay()) / 64
    xt, yt = store.batch_torch(sl(3), check=False)
    store.compose(sl(3), x, y)
    nbytes = B * N * 4 * (2 * U + W + U)          # u_in and u_out read once, x and y written once
    rate = nbytes / (graph_us * 1e-6) / 1e9
    out["compose"] = {"hip_us_per_call_from_python": hip_us, "hip_us_per_launch_in_a_graph": graph_us, "torch_ops_us_per_batch": aten_us,
                      "speedup_per_call": aten_us / hip_us, "bytes_needed": nbytes,
                      "what": "per call = store.compose() issued from Python back to back (argument checks and the ctypes call included); in a graph = 64 "
                              "launches replayed as one hipGraph, per launch: the device's own cost",
                      "GBps_over_graph_launch_time": rate, "share_of_copy_rate": rate / COPY_RATE_GBPS,
                      "us_at_copy_rate": nbytes / COPY_RATE_GBPS * 1e-3, "equal_bits_to_torch_ops": bool(torch.equal(x, xt) and torch.equal(y, yt)),
                      "status_flag": store.status()}

    # ---- the training step, three ways of feeding it
    lat = grid(bench.LATENT).to(dev)
    xc = (torch.rand(N, 2, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    kw = dict(latent_tokens_coord=lat, xcoord=xc)
    ts_pairs = TrainStep(build_model(dev), lr=8e-4, weight_decay=1e-5)
    ts_pairs.bind_pairs(store, B, **kw)
    ts_host = TrainStep(build_model(dev), lr=8e-4, weight_decay=1e-5)
    ts_host.bind(xt, yt, **kw)
    ts_dev = TrainStep(build_model(dev), lr=8e-4, weight_decay=1e-5)
    ts_dev.bind(xt, yt, **kw)
    loader = torch.utils.data.DataLoader(HostPairs(host), batch_size=B, shuffle=True, drop_last=True, num_workers=args.workers, pin_memory=True,
                                         persistent_workers=args.workers > 0, multiprocessing_context="spawn" if args.workers > 0 else None)

    def batches():
        while True:
            for xb, yb in loader:
                yield xb, yb
    it = batches()
    count = [0, 0]

    def leg_pairs():
        ts_pairs.step_pairs(sl(count[0])); count[0] += 1

    def leg_host():
        xb, yb = next(it)
        ts_host.step(xb.to(dev, non_blocking=True), yb.to(dev, non_blocking=True))

    def leg_dev():
        xb, yb = store.batch_torch(sl(count[1]), check=False); count[1] += 1
        ts_dev.step(xb, yb)
    ms = alternate({"step_pairs": leg_pairs, "step_xy_host_dataloader": leg_host, "step_xy_torch_ops_on_device": leg_dev}, args.rounds)
    out["train_step_ms"] = ms
    out["train_step"] = {"n_captures_step_pairs": ts_pairs.n_captures, "dataloader_workers": args.workers, "pinned": True,
                         "host_loader_rate_over_step_pairs_rate": ms["step_pairs"]["median"] / ms["step_xy_host_dataloader"]["median"],
                         "torch_ops_rate_over_step_pairs_rate": ms["step_pairs"]["median"] / ms["step_xy_torch_ops_on_device"]["median"],
                         "status_flag": store.status()}
    del it, loader
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
