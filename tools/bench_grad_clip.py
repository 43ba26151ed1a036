#!/usr/bin/env python3
"""What gradient-norm clipping and the non-finite guard cost at the headline configuration (bench.py's: 16 384 nodes, batch 8, the
whole step as one hipGraph replay):
    python tools/bench_grad_clip.py [--out profiles/grad_clip.json] [--rounds 5] [--steps 200]
TrainSteps of the same build -- default, max_grad_norm=1.0, max_grad_norm=1.0 + skip_nonfinite, and a second instance of the first two
-- are warmed up and then timed in alternation, in an order rotated from round to round (host clock around `steps` replays that end
in a device synchronise; the best and the median round per setting), so the denominator is the default path of the same library
at the same moment and the twins show the spread between two instances of one setting.  The two added launches are also timed on their own:
device events around 200 back-to-back launches on the step's own gradient buffer (norm pass; clipped update against the plain one).
Needs a GPU; prints and writes one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from gaot_amd import _lib, ops
from gaot_amd.ops import _p, _stream
from gaot_amd.trainer import TrainStep

# (the *_b twins repeat a setting in a second instance -- its own model, buffers and captured graph: their distance from the first
# instance is the spread a difference between settings has to exceed)
SETTINGS = [("default", {}), ("clip", dict(max_grad_norm=1.0)), ("clip_skip", dict(max_grad_norm=1.0, skip_nonfinite=True)),
            ("default_b", {}), ("clip_b", dict(max_grad_norm=1.0))]


def per_launch_us(fn, reps=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_clip.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    runs = {}
    for name, kw in SETTINGS:
        ops.register_grad_slots([], [])
        torch.manual_seed(0)
        model = bench.build_model().to(dev).train()
        lat, x, p, t = bench.synthetic(1234, dev)
        ts = TrainStep(model, lr=8e-4, weight_decay=1e-5, use_graph=True, **kw)
        ts.bind(p, t, latent_tokens_coord=lat, xcoord=x)
        for _ in range(10):
            ts.step()
        torch.cuda.synchronize()
        runs[name] = (ts, model)
    ms = {name: [] for name in runs}
    order = list(runs.items())
    for rnd in range(args.rounds):
        for name, (ts, _) in order[rnd % len(order):] + order[:rnd % len(order)]:      # (rotated: no setting keeps one place in the sequence)
            for _ in range(5):
                ts.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts.step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    # the added launches on their own, on the clipped step's buffers (the update is timed on copies: it must not train the model further)
    ts = runs["clip_skip"][0]
    o, n = ts.opt, ts.opt.flat_p.numel()
    pc, mc, vc, gst = o.flat_p.clone(), o.m.clone(), o.v.clone(), o.gstat.clone()
    step = o.step_count.clone()
    part, ticket = torch.empty(256, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    g = ts.bucket.flat
    norm_us = per_launch_us(lambda: lib.gaot_grad_norm_dev(_p(g), n, _p(part), _p(ticket), _p(o.clip), _p(step), 1, _p(gst), _stream()))
    clipped_us = per_launch_us(lambda: lib.gaot_adamw_apply_clipped_dev(_p(pc), _p(g), _p(mc), _p(vc), n, _p(o.hyper), _p(step), _p(gst), _p(o.clip), _stream()))
    plain_us = per_launch_us(lambda: lib.gaot_adamw_apply_dev(_p(pc), _p(g), _p(mc), _p(vc), n, _p(o.hyper), _p(step), _stream()))
    base = min(ms["default"])
    out = {
        "config": {"nodes": bench.N_NODES, "batch": bench.BATCH, "params": sum(q.numel() for q in runs["default"][1].parameters()),
                   "flat_gradient_bytes": 4 * n, "graph_replay": True, "rounds": args.rounds, "steps_per_round": args.steps,
                   "device": torch.cuda.get_device_name(0)},
        "ms_per_step": {k: {"best": min(v), "median": statistics.median(v), "rounds": v} for k, v in ms.items()},
        "overhead_vs_default_pct": {k: {"best": 100.0 * (min(ms[k]) - base) / base,
                                        "median": 100.0 * (statistics.median(ms[k]) - statistics.median(ms["default"])) / statistics.median(ms["default"])}
                                    for k in ("clip", "clip_skip", "default_b", "clip_b")},
        "added_launches_us": {"grad_norm": norm_us, "adamw_apply_clipped": clipped_us, "adamw_apply_plain": plain_us,
                              "grad_norm_read_GBps": 4 * n / (norm_us * 1e-6) / 1e9},
        "grad_norm_last_step": {k: float(runs[k][0].grad_norm) for k in ("clip", "clip_skip")},
        "clip_coef_last_step": {k: float(runs[k][0].opt.clip_coef) for k in ("clip", "clip_skip")},
        "skipped_steps": {k: runs[k][0].skipped_steps for k in ("clip", "clip_skip")},
        "loss_last_step": {k: float(runs[k][0]._loss) for k in runs},
        "default_instances_bit_equal": bool(torch.equal(runs["default"][0].opt.flat_p, runs["default_b"][0].opt.flat_p)),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
