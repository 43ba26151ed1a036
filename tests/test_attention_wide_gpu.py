"""-m gpu: attention for 128 < head_dim <= 256 (attention_wide.hip: the head dimension split over the waves of a workgroup) against
float64, at the bars of the fp32-MFMA kernels (output 3e-6, gradient 1e-5; the same closed form in fp32 on the CPU sits at
3.2e-7 .. 5.9e-7 on these shapes), and through the model against the oracle."""
import math
from types import SimpleNamespace as NS

import pytest
import torch

from tests._golden import fp32_noise
from tests._workloads import grid, uniform_points
from tests.test_configs_gpu import check_step, csr_dict
from tests.test_ops_gpu import _dropout_factor, dev, rel

pytestmark = pytest.mark.gpu


def _reference(qkv, go, B, S, H, Hkv, D, fac=None):
    r = qkv.clone().double().requires_grad_(True)
    q = r[..., :H * D].reshape(B, S, H, D).transpose(1, 2)
    k = r[..., H * D:(H + Hkv) * D].reshape(B, S, Hkv, D).transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    v = r[..., (H + Hkv) * D:].reshape(B, S, Hkv, D).transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1)
    if fac is not None:
        p = p * fac
    ref = (p @ v).transpose(1, 2).reshape(B, S, H * D)
    ref.backward(go.double())
    return ref.detach(), r.grad


@pytest.mark.parametrize("B,S,H,Hkv,D", [(1, 33, 1, 1, 132), (2, 97, 2, 1, 160), (1, 130, 2, 2, 256), (1, 300, 1, 1, 200),
                                         (1, 257, 4, 2, 192), (1, 64, 1, 1, 250), (1, 160, 2, 2, 255), (1, 7, 1, 1, 129),
                                         (2, 512, 2, 2, 256)])
def test_wide_attention_fwd_bwd(B, S, H, Hkv, D):
    from gaot_amd import ops
    g = torch.Generator().manual_seed(S + D)
    W = (H + 2 * Hkv) * D
    qkv = torch.randn(B, S, W, generator=g)
    go = torch.randn(B, S, H * D, generator=g)
    ref, gref = _reference(qkv, go, B, S, H, Hkv, D)
    d = qkv.to(dev()).requires_grad_(True)
    out = ops.attention(d, H, Hkv, D)
    out.backward(go.to(dev()))
    e_out, e_grad = rel(out, ref), rel(d.grad, gref)
    print(f"[wide {B}x{S}x{H}/{Hkv}x{D}] out {e_out:.2e}  dqkv {e_grad:.2e}")
    assert torch.isfinite(out).all() and torch.isfinite(d.grad).all()
    assert e_out < 3e-6
    assert e_grad < 1e-5


def test_wide_attention_peaked_softmax():
    """one key, in a later key tile, dominates one query: the running-max rescale across tiles and across the wave exchange"""
    from gaot_amd import ops
    g = torch.Generator().manual_seed(4)
    B, S, H, D = 1, 256, 2, 256
    qkv = torch.randn(B, S, 3 * H * D, generator=g)
    qkv[0, 17, :D] *= 6.0
    qkv[0, 201, H * D:H * D + D] = qkv[0, 17, :D] * 1.5
    r = qkv.double()
    q = r[..., :H * D].reshape(B, S, H, D).transpose(1, 2)
    k = r[..., H * D:2 * H * D].reshape(B, S, H, D).transpose(1, 2)
    v = r[..., 2 * H * D:].reshape(B, S, H, D).transpose(1, 2)
    ref = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), -1) @ v).transpose(1, 2).reshape(B, S, H * D)
    out = ops.attention(qkv.to(dev()), H, H, D)
    print(f"[wide peaked] out {rel(out, ref):.2e}")
    assert torch.isfinite(out).all()
    assert rel(out, ref) < 3e-6


@pytest.mark.parametrize("B,S,H,Hkv,D,p", [(1, 150, 2, 2, 160, 0.2), (1, 64, 1, 1, 256, 0.3), (2, 70, 4, 2, 136, 0.5)])
def test_wide_attention_dropout_matches_float64_with_the_same_mask(B, S, H, Hkv, D, p):
    from gaot_amd import ops
    g = torch.Generator().manual_seed(S + D)
    W = (H + 2 * Hkv) * D
    qkv = torch.randn(B, S, W, generator=g)
    go = torch.randn(B, S, H * D, generator=g)
    ops.seed_dropout(1234, dev())
    d = qkv.to(dev()).requires_grad_(True)
    out = ops.attention(d, H, Hkv, D, dropout_p=p)
    out.backward(go.to(dev()))
    seed = int(ops._LAST_DROPOUT_SEED[0].cpu().item())
    fac = _dropout_factor(seed, B, H, S, p)
    assert abs(float((fac > 0).double().mean()) - (1.0 - p)) < 0.02          # the keep rate
    ref, gref = _reference(qkv, go, B, S, H, Hkv, D, fac)
    e_out, e_grad = rel(out, ref), rel(d.grad, gref)
    print(f"[wide dropout {B}x{S}x{H}/{Hkv}x{D} p={p}] out {e_out:.2e}  dqkv {e_grad:.2e}")
    assert e_out < 3e-6
    assert e_grad < 1e-5
    # a second call draws another mask (the counter lives on the device); re-seeding reproduces the first bit for bit
    out2 = ops.attention(d.detach(), H, Hkv, D, dropout_p=p)
    assert rel(out2, ref) > 1e-2
    ops.seed_dropout(1234, dev())
    assert torch.equal(ops.attention(d.detach(), H, Hkv, D, dropout_p=p), out.detach())


def test_wide_attention_is_deterministic_and_captures():
    from gaot_amd import ops
    B, S, H, Hkv, D = 1, 200, 2, 1, 192
    g = torch.Generator().manual_seed(S + D)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).to(dev())
    go = torch.randn(B, S, H * D, generator=g).to(dev())
    runs = []
    for _ in range(2):
        d = qkv.clone().requires_grad_(True)
        out = ops.attention(d, H, Hkv, D)
        out.backward(go)
        runs.append((out.detach().clone(), d.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(gr):
        y = ops.attention(qkv, H, Hkv, D)
    for _ in range(2):
        y.zero_()
        gr.replay()
        assert torch.equal(y, runs[0][0])


# ------------------------------------------------------------------------------------------------ through the model
def _make_model(hidden, heads, kv_heads, positional_embedding="absolute", seed=0):
    """tests.test_configs_gpu.make_model with kv heads and the positional embedding open (latent [16, 16], radius 0.12, C = 32)"""
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.attn import AttentionConfig, TransformerConfig
    from gaot_amd.model.layers.magno import MAGNOConfig
    from oracle import gaot_oracle as O
    torch.manual_seed(seed)
    mcfg = MAGNOConfig(coord_dim=2, radius=0.12, hidden_size=64, mlp_layers=3, lifting_channels=32, precompute_edges=True)
    tcfg = TransformerConfig(patch_size=2, hidden_size=hidden, positional_embedding=positional_embedding,
                             attn_config=AttentionConfig(num_heads=heads, num_kv_heads=kv_heads))
    model = GAOT(2, 1, NS(args=NS(magno=mcfg, transformer=tcfg), latent_tokens_size=[16, 16]))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ocfg = O.OracleConfig(coord_dim=2, radius=0.12, hidden_size=64, lifting_channels=32, patch_size=2, tf_hidden_size=hidden,
                          num_heads=heads, num_kv_heads=kv_heads, positional_embedding=positional_embedding,
                          latent_tokens_size=[16, 16], precompute_edges=True)
    return model, sd, ocfg


@pytest.mark.parametrize("hidden,heads,kv_heads,pos", [(512, 2, 2, "absolute"), (384, 2, 1, "absolute"), (320, 2, 2, "rope")])
def test_wide_head_model_vs_oracle(hidden, heads, kv_heads, pos):
    """head_dim 256, 192 with one kv head, 160 with rope: forward, loss and every gradient of one training step"""
    from oracle import gaot_oracle as O
    model, sd, ocfg = _make_model(hidden, heads, kv_heads, pos, seed=21)
    g = torch.Generator().manual_seed(21)
    lat, x = grid([16, 16]), uniform_points(900, 2, g)
    p, tgt = torch.randn(2, 900, 2, generator=g), torch.randn(2, 900, 1, generator=g)
    enc, dec = [O.radius_csr(x, lat, 0.12)], [O.radius_csr(lat, x, 0.12)]
    batch = dict(latent=lat, xcoord=x, pndata=p, target=tgt, encoder_nbrs=enc, decoder_nbrs=dec)
    loss, grads, _, _, pred = O.train_step(sd, ocfg, batch, return_pred=True)
    model.to(dev()).train()
    assert model.processor.blocks_in_order()[0].attn.head_dim == hidden // heads
    kw = dict(latent_tokens_coord=lat.to(dev()), xcoord=x.to(dev()), encoder_nbrs=[csr_dict(enc[0])], decoder_nbrs=[csr_dict(dec[0])])
    check_step(model, (loss, grads, pred), kw, p.to(dev()), tgt.to(dev()), f"head_dim {hidden // heads}",
               noise=fp32_noise(sd, ocfg, batch, grads))
