#!/usr/bin/env python3
"""Attention at head_dim 256 (the 350 M point's processor: 8 x 1 024 tokens, 8 heads of 256) on one GPU.

    python tools/bench_attention_wide.py [--out profiles/attention_wide.json] [--legs attn,model]

Legs, each in a child process of its own under its own time limit (the parent never touches the GPU and stops at the first leg
that fails):
  attn   forward and forward+backward of ops.attention at B 8, S 1024, H 8, Hkv 8, D 256 against F.scaled_dot_product_attention
         in fp32 on the same tensors (what the reference runs, attn.py:114; no autocast), and against ops.attention at D 128 with the
         same B, S, H (half the FLOPs).  Device events around sustained windows (>= 0.5 s each), every shape warmed first, the two
         sides alternating, three rounds; the figure is the median round, the spread is (max - min) / median.
  model  one GAOT with hidden 2048 on 8 heads on the bench mesh (16 384 nodes, batch 8): eager train steps (forward, MSE, backward,
         AdamW), finite loss and gradients, ms per step.  A record, not a comparison.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, S, H = 8, 1024, 8
LEG_LIMIT_S = {"attn": 420, "model": 420}
PEAK_F32_MATRIX_TFLOPS = 157.3


def _window(fn, min_ms=500.0):
    """ms per call over a window of at least `min_ms` (sized from a short calibration window)"""
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        fn()
    e.record(); torch.cuda.synchronize()
    n = max(10, int(min_ms / max(s.elapsed_time(e) / 5, 1e-3)) + 1)
    s.record()
    for _ in range(n):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def _summary(xs):
    med = statistics.median(xs)
    return {"ms": round(med, 4), "spread": round((max(xs) - min(xs)) / med, 4), "rounds": [round(x, 4) for x in xs]}


def leg_attn():
    import torch
    import torch.nn.functional as F
    from gaot_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sides = {}
    for D in (256, 128):
        qkv = torch.randn(B, S, 3 * H * D, device=dev, requires_grad=True)
        go = torch.randn(B, S, H * D, device=dev)

        def ours_fwd(qkv=qkv, D=D):
            with torch.no_grad():
                ops.attention(qkv, H, H, D)

        def ours_fb(qkv=qkv, go=go, D=D):
            o = ops.attention(qkv, H, H, D)
            torch.autograd.grad(o, qkv, go)

        sides[f"ours_d{D}"] = (ours_fwd, ours_fb)
        if D == 256:
            q, k, v = [t.reshape(B, S, H, D).transpose(1, 2).detach().requires_grad_(True) for t in qkv.detach().split(H * D, dim=-1)]
            gt = go.reshape(B, S, H, D).transpose(1, 2)

            def sdpa_fwd(q=q, k=k, v=v):
                with torch.no_grad():
                    F.scaled_dot_product_attention(q, k, v, attn_mask=None, dropout_p=0.0)

            def sdpa_fb(q=q, k=k, v=v, gt=gt):
                o = F.scaled_dot_product_attention(q, k, v, attn_mask=None, dropout_p=0.0)
                torch.autograd.grad(o, (q, k, v), gt)

            sides["sdpa_fp32_d256"] = (sdpa_fwd, sdpa_fb)
            # the two sides compute the same thing on these tensors
            with torch.no_grad():
                o1 = ops.attention(qkv, H, H, D)
                o2 = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, H * D)
            agree = float((o1.double() - o2.double()).norm() / o2.double().norm())
    for fwd, fb in sides.values():      # warm every shape and both directions
        for _ in range(3):
            fwd(); fb()
    torch.cuda.synchronize()
    times = {k: {"fwd": [], "fwd_bwd": []} for k in sides}
    for _ in range(3):
        for name, (fwd, fb) in sides.items():      # alternating sides inside a round
            times[name]["fwd"].append(_window(fwd))
            times[name]["fwd_bwd"].append(_window(fb))
    res = {k: {d: _summary(v) for d, v in t.items()} for k, t in times.items()}
    flop_fwd = 4.0 * B * H * S * S * 256
    ours, ref, half = res["ours_d256"], res["sdpa_fp32_d256"], res["ours_d128"]
    return {"shape": {"B": B, "S": S, "H": H, "Hkv": H, "D": 256}, "times": res, "output_rel_l2_ours_vs_sdpa": agree,
            "ours_over_sdpa": {d: round(ours[d]["ms"] / ref[d]["ms"], 4) for d in ("fwd", "fwd_bwd")},
            "d256_over_d128": {d: round(ours[d]["ms"] / half[d]["ms"], 4) for d in ("fwd", "fwd_bwd")},
            "ours_fwd_tflops": round(flop_fwd / (ours["fwd"]["ms"] * 1e-3) / 1e12, 2),
            "ours_fwd_share_of_f32_matrix_peak": round(flop_fwd / (ours["fwd"]["ms"] * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 4),
            "not_slower_than_sdpa": {d: ours[d]["ms"] <= ref[d]["ms"] for d in ("fwd", "fwd_bwd")}}


def leg_model():
    from types import SimpleNamespace as NS
    import torch
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import TransformerConfig
    from gaot_amd.model.layers.magno import MAGNOConfig
    from gaot_amd.trainer import TrainStep
    dev = torch.device("cuda:0")
    n_nodes, batch, latent = 16384, 8, [64, 64]
    torch.manual_seed(0)
    mcfg = MAGNOConfig(coord_dim=2, radius=0.033, hidden_size=64, mlp_layers=3, lifting_channels=64)
    tcfg = TransformerConfig(patch_size=2, hidden_size=2048)
    model = GAOT(1, 1, NS(args=NS(magno=mcfg, transformer=tcfg), latent_tokens_size=latent)).to(dev).train()
    n_params = sum(p.numel() for p in model.parameters())
    g = torch.Generator().manual_seed(1)
    ax = torch.linspace(-1, 1, latent[0])
    lat = torch.stack(torch.meshgrid(ax, torch.linspace(-1, 1, latent[1]), indexing="ij"), -1).reshape(-1, 2).to(dev)
    x = (torch.rand(n_nodes, 2, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    p = torch.randn(batch, n_nodes, 1, generator=g).to(dev)
    t = torch.randn(batch, n_nodes, 1, generator=g).to(dev)
    ts = TrainStep(model, lr=8e-4, weight_decay=1e-5, use_graph=False)
    ts.bind(p, t, latent_tokens_coord=lat, xcoord=x)
    losses = [float(ts.step()) for _ in range(3)]
    grads_finite = all(bool(torch.isfinite(q.grad).all()) for q in model.parameters() if q.grad is not None)
    n_grads = sum(q.grad is not None for q in model.parameters())
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = 10
    s.record()
    for _ in range(steps):
        last = ts.step()
    e.record(); torch.cuda.synchronize()
    losses.append(float(last))
    ok = all(l == l and abs(l) != float("inf") for l in losses) and grads_finite and n_grads > 0
    return {"config": "GAOT hidden 2048 / 8 heads (head_dim 256), patch 2, latent 64 x 64, 16384 nodes, batch 8, eager TrainStep",
            "parameters": n_params, "losses": losses, "gradient_tensors_checked": n_grads, "finite": ok,
            "ms_per_step": round(s.elapsed_time(e) / steps, 3), "timed_steps": steps}


LEGS = {"attn": leg_attn, "model": leg_model}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_wide.json"))
    ap.add_argument("--legs", default="attn,model")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its JSON")
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_attention_wide: no GPU")
        print("RESULT " + json.dumps(LEGS[args.leg]()), flush=True)
        return
    out = {}
    for leg in args.legs.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True,
                               timeout=LEG_LIMIT_S[leg])
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_attention_wide: leg {leg} ran past its limit of {LEG_LIMIT_S[leg]} s; stopping")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"bench_attention_wide: leg {leg} failed (exit {r.returncode}); stopping")
        out[leg] = json.loads(line[-1][len("RESULT "):])
        print(leg, json.dumps(out[leg]), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
