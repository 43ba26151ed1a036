#!/usr/bin/env python3
"""What the evaluation half costs (DESIGN "Evaluation on the device"):
    python tools/eval_bench.py [--out profiles/eval_step.json] [--rounds 5]
  * trainer.EvalStep under hipGraph replay against the evaluation pass the parent commit offers (model.eval(), no_grad, ops.mse_loss,
    a few hundred Python-driven launches): at the bench configuration (16 384 nodes, batch 8) and at the C3 vx shape (8 192-node airfoil
    meshes, batch 16) over shuffled batch compositions.  Both are warmed up and timed in alternation in ONE process, a host clock around
    windows that end in a device synchronise, at least a second of work per leg; best, median and every round are reported.
  * gaot_rel_l1_errors against the reference's expression as ATen ops on the same GPU (the torch_gpu_baseline convention) at the C4 rollout
    shape and at [64, 8, 16384, 4]: device events around back-to-back calls; the bytes the algorithm needs (two tensors read once) over
    that time, as a share of the 6.29 TB/s copy rate measured on this part.
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
from gaot_amd import _lib, metrics, ops
from gaot_amd.trainer import EvalStep
from tests._metrics_ref import Meta, chunk_table
from tests._workloads import naca_points

COPY_RATE_GBPS = 6290.0          # streaming copy rate measured on the MI355X (MI355X notes; the share below is against this, not the 8 TB/s spec)


def by_hand(model, kw, p, t):
    model.eval()
    with torch.no_grad():
        loss = ops.mse_loss(model(pndata=p, **kw), t)
    model.train()
    return loss


def alternate(legs, rounds, min_seconds=0.25):
    """legs: name -> callable(step index).  Rounds of alternating windows; every window runs for at least `min_seconds` (so `rounds` of them are
    more than a second per leg) and ends in a synchronise.  Returns name -> list of ms per step."""
    ms = {k: [] for k in legs}
    counter = {k: 0 for k in legs}
    for k, fn in legs.items():          # warm-up: captures, plans, allocator
        for _ in range(12):
            fn(counter[k]); counter[k] += 1
    torch.cuda.synchronize()
    order = list(legs)
    for rnd in range(rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:
            fn = legs[k]
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(10):
                    fn(counter[k]); counter[k] += 1
                n += 10
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= min_seconds:
                    break
            ms[k].append(dt / n * 1e3)
    return ms


def summary(ms):
    return {k: {"best": min(v), "median": statistics.median(v), "rounds": v} for k, v in ms.items()}


def c2(dev, rounds):
    torch.manual_seed(0)
    model = bench.build_model().to(dev).train()
    lat, x, p, t = bench.synthetic(1234, dev)
    kw = dict(latent_tokens_coord=lat, xcoord=x)
    ev = EvalStep(model)
    ev.bind(p, t, **kw)
    ms = alternate({"evalstep_replay": lambda i: ev.step(p, t), "eager_eval": lambda i: by_hand(model, kw, p, t)}, rounds)
    same = bool(torch.equal(ev.step(p, t), by_hand(model, kw, p, t)))
    return {"config": f"bench configuration: {bench.N_NODES} nodes, batch {bench.BATCH}", "ms_per_step": summary(ms), "n_captures": ev.n_captures,
            "replay_loss_equals_eager_loss_bits": same}


def c3(dev, rounds):
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import TransformerConfig
    from gaot_amd.model.layers.magno import MAGNOConfig
    from gaot_amd.model.layers.utils.neighbor_search import NeighborSearch
    torch.manual_seed(0)
    B, N, NS_DATA = 16, 8192, 48
    mc = MAGNOConfig(radius=bench.RADIUS, lifting_channels=bench.C_LIFT, precompute_edges=True)
    model = GAOT(3, 1, NS(args=NS(magno=mc, transformer=TransformerConfig(patch_size=bench.PATCH, hidden_size=bench.HIDDEN)),
                          latent_tokens_size=bench.LATENT)).to(dev).train()
    g = torch.Generator().manual_seed(0)
    lat = bench.synthetic(0, dev)[0]
    xd = torch.stack([naca_points(N, g, 0.15 if i < B else 0.12 + 0.06 * (i % 8) / 7) for i in range(NS_DATA)]).to(dev)
    pd, td = torch.randn(NS_DATA, N, 3, generator=g).to(dev), torch.randn(NS_DATA, N, 1, generator=g).to(dev)
    ns = NeighborSearch("auto")
    enc = [[ns(xd[i], lat, bench.RADIUS)] for i in range(NS_DATA)]
    dec = [[ns(lat, xd[i], bench.RADIUS)] for i in range(NS_DATA)]
    gsh = torch.Generator().manual_seed(7)
    comps = [torch.randperm(NS_DATA, generator=gsh)[:B].tolist() for _ in range(64)]
    pick = lambda rows, b: [rows[i] for i in b]
    ev = EvalStep(model)
    b0 = comps[0]
    ev.bind(pd[b0], td[b0], latent_tokens_coord=lat, xcoord=xd[b0], encoder_nbrs=pick(enc, b0), decoder_nbrs=pick(dec, b0))

    def replay(i):
        b = comps[i % len(comps)]
        ix = torch.tensor(b, device=dev)
        return ev.step(pd[ix], td[ix], xcoord=xd[ix], encoder_nbrs=pick(enc, b), decoder_nbrs=pick(dec, b))

    def eager(i):
        b = comps[i % len(comps)]
        ix = torch.tensor(b, device=dev)
        return by_hand(model, dict(latent_tokens_coord=lat, xcoord=xd[ix], encoder_nbrs=pick(enc, b), decoder_nbrs=pick(dec, b)), pd[ix], td[ix])
    for i in range(len(comps)):          # every composition once before the clock: the captures of all buckets, the plans of all samples
        replay(i)
    torch.cuda.synchronize()
    caps0 = ev.n_captures
    ms = alternate({"evalstep_replay": replay, "eager_eval": eager}, rounds)
    a, e = float(replay(3)), float(eager(3))
    return {"config": f"C3: NACA0012-shaped vx meshes, {N} nodes, batch {B}, {len(comps)} shuffled compositions of {NS_DATA} resident samples",
            "ms_per_step": summary(ms), "n_captures_before_timing": caps0, "captures_inside_timed_region": ev.n_captures - caps0,
            "replay_vs_eager_loss_rel": abs(a - e) / abs(e)}


def aten_batch_errors(gtr, prd, mean, std, chunks, C):
    """the reference's expression (utils/metrics.py:38-56) as ATen ops, tables already on the device"""
    g, p = (gtr - mean) / std, (prd - mean) / std
    err = torch.abs(g - p).sum(dim=(1, 2))
    ref = torch.abs(g).sum(dim=(1, 2))
    num = torch.zeros(err.shape[0], C, device=gtr.device, dtype=gtr.dtype).index_add_(1, chunks, err)
    den = torch.zeros(err.shape[0], C, device=gtr.device, dtype=gtr.dtype).index_add_(1, chunks, ref)
    return num / (den + 1e-10)


def per_call_us(fn, min_ms=300.0):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_ms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        reps += 50
    return total / reps * 1e3


def rel_l1(dev):
    out = {}
    ce = Meta([0, 1, 2, 3], [0, 1, 1, 2, 3], [0.80, 0., 0., 2.513], [0.31, 0.391, 0.356, 0.185])
    ns = Meta([0, 1], [0, 0], [0.0, 0.0], [0.391, 0.356])
    g = torch.Generator().manual_seed(1)
    for name, md, shape, slab in (("c4_rollout_slab", ns, (4, 10, 16384, 2), True), ("b64_t8_n16384_v4", ce, (64, 8, 16384, 4), False)):
        B, T, N, V = shape
        if slab:          # the device rollout's step-major slab, handed over as the permuted view
            gtr = torch.randn(T, B, N, V, generator=g).to(dev).permute(1, 0, 2, 3)
            prd = (gtr + 0.1 * torch.randn(B, T, N, V, generator=g).to(dev)).permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
        else:
            gtr = torch.randn(*shape, generator=g).to(dev)
            prd = gtr + 0.1 * torch.randn(*shape, generator=g).to(dev)
        tab = metrics._tables(md, dev)
        chunks, C = chunk_table(md)
        ch = torch.tensor(chunks, device=dev)
        mean, std = tab.mean.reshape(1, 1, 1, -1), tab.std.reshape(1, 1, 1, -1)
        ours = metrics.compute_batch_errors(gtr, prd, md)
        theirs = aten_batch_errors(gtr, prd, mean, std, ch, C)
        hip_us = per_call_us(lambda: metrics.compute_batch_errors(gtr, prd, md))
        aten_us = per_call_us(lambda: aten_batch_errors(gtr, prd, mean, std, ch, C))
        # the two launches alone: the C entry point on buffers allocated once (what an ErrorLog.append inside a captured graph would cost)
        lib = _lib.load()
        ws = torch.empty(int(lib.gaot_rel_l1_errors_workspace(B, T, N, V)) // 2, dtype=torch.float64, device=dev)
        res = torch.empty(B, C, device=dev)
        raw = lambda: lib.gaot_rel_l1_errors(ops._p(gtr), gtr.stride(0), gtr.stride(1), ops._p(prd), prd.stride(0), prd.stride(1), B, T, N, V, None, None,
                                             ops._p(tab.mean), ops._p(tab.std), ops._p(tab.chunks), C, ops._p(ws), ops._p(res), C, ops._stream())
        raw_us = per_call_us(raw)
        nbytes = 2 * B * T * N * V * 4
        rate = nbytes / (raw_us * 1e-6) / 1e9
        out[name] = {"shape": list(shape), "step_major_view": slab, "hip_us_per_call": hip_us, "hip_us_two_launches": raw_us, "aten_us_per_call": aten_us,
                     "speedup": aten_us / hip_us, "bytes_needed": nbytes, "GBps_over_launch_time": rate, "share_of_copy_rate": rate / COPY_RATE_GBPS,
                     "what": "per call = the wrapper (workspace and result allocated per call); two launches = the C entry point back to back on one stream",
                     "max_rel_difference_to_aten": float(((ours - theirs).abs() / theirs.abs()).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_step.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="c2,c3,rel_l1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "single_box": True, "rounds": args.rounds}
    which = args.only.split(",")
    if "rel_l1" in which:
        out["rel_l1_errors"] = rel_l1(dev)
    if "c2" in which:
        out["evalstep_c2"] = c2(dev, args.rounds)
    if "c3" in which:
        out["evalstep_c3"] = c3(dev, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
