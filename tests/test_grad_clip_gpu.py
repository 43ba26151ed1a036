"""-m gpu: global gradient-norm clipping and the non-finite step skip on the device -- the norm kernel against float64, the clipped
flat update against clip_grad_norm_ + torch.optim.AdamW, and TrainStep with the options on (eager, hipGraph replay, staged over a
one-rank RCCL group): a skipped step is bit-neutral, a schedule moves max_grad_norm without re-capture, and with the options
off -- or with a bound nothing reaches -- the step keeps its bits."""
import math
import os
import socket
from types import SimpleNamespace as NS

import pytest
import torch

from tests._golden import Golden
from tests.test_model_gpu import GRAD_L2_TOL, build_model, seed_neighbor_cache

pytestmark = pytest.mark.gpu

U = 2.0 ** -24               # unit roundoff of fp32
INF = float("inf")
WRAP_N = 2048 * 256 * 4 + 5  # past one sweep of the widest grid any flat kernel here uses: the grid-stride loop wraps (and a tail of 1)


def dev():
    return torch.device("cuda:0")


def norm_rel_bound(n: int) -> float:
    """relative error bound of gaot_grad_norm_dev's norm, from its summation lengths (include/gaot_hip.h): min(256, ceil(n4 / 1024))
    workgroups of 256 threads stride over the n4 = n // 4 vectors.  A square (1 rounding) passes the in-vector pair tree (2), then
    its thread's accumulator -- at most `iters` adds plus the scalar tail's one -- then the wave butterfly (6) and the 4-wave tree (2);
    the partials are added in double (nothing at this scale) and the root is rounded to fp32 once, which is 2 roundings' worth on the
    sum of squares.  All terms are positive, so the relative error of the sum is at most the longest chain x 2^-24:
    (chain + tree + 2) x 2^-24 with chain = iters + 1, tree = 10; the square root halves it."""
    n4 = n // 4
    blocks = min(256, max(1, -(-n4 // 1024)))
    iters = -(-n4 // (blocks * 256))
    return 0.5 * ((iters + 1) + 10 + 2) * U


def _lib():
    from gaot_amd import _lib as L
    return L, L.load()


def grad_norm(g, max_norm=INF, skip=False, step=0.0, ticked=False, gstat=None, scratch=None):
    """one gaot_grad_norm_dev launch on fresh (or the given) scratch; returns (gstat, step, ticket) as device tensors"""
    from gaot_amd.ops import _p, _stream
    L, lib = _lib()
    part, ticket = scratch if scratch is not None else (torch.empty(256, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev()))
    clip = torch.tensor([max_norm, 1.0 if skip else 0.0], device=dev())
    st = torch.tensor([step], device=dev())
    gstat = torch.zeros(4, device=dev()) if gstat is None else gstat
    L.check(lib.gaot_grad_norm_dev(_p(g), g.numel(), _p(part), _p(ticket), _p(clip), _p(st), 1 if ticked else 0, _p(gstat), _stream()),
            "gaot_grad_norm_dev")
    return gstat, st, ticket


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 65539, WRAP_N])
def test_norm_kernel_vs_float64(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev())
    want = float(g.double().norm())
    gstat, st, ticket = grad_norm(g)
    got = gstat.tolist()
    err = abs(got[0] - want) / want
    print(f"[grad_norm n={n}] norm {got[0]:.8g} float64 {want:.8g} rel err {err:.2e} bound {norm_rel_bound(n):.2e}")
    assert err <= norm_rel_bound(n)
    assert got[1] == 1.0 and got[2] == 1.0 and got[3] == 0.0           # no bound: coef 1; finite; nothing skipped
    assert int(ticket) == 0 and float(st) == 1.0                        # ticket back at zero; the launch ticked the counter itself
    again, _, _ = grad_norm(g)
    assert torch.equal(again, gstat)                                    # the bits do not depend on scheduling
    # torch's coefficient, and a bound nothing reaches
    half = 0.5 * got[0]
    c, _, _ = grad_norm(g, max_norm=half)
    want_coef = torch.tensor(half, dtype=torch.float32) / (torch.tensor(got[0], dtype=torch.float32) + 1e-6)
    assert abs(float(c[1]) - float(want_coef)) <= 4 * U * float(want_coef) and float(c[0]) == got[0]
    for off in (1e30, INF, 0.0, -1.0):
        assert float(grad_norm(g, max_norm=off)[0][1]) == 1.0


def test_norm_kernel_zero_and_nonfinite_inputs():
    for n in (5, 65539):
        gstat, _, ticket = grad_norm(torch.zeros(n, device=dev()), max_norm=1.0)
        assert gstat.tolist() == [0.0, 1.0, 1.0, 0.0] and int(ticket) == 0
    n = 65539                                                            # 16384 vectors and a scalar tail of 3
    base = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev())
    scratch = (torch.empty(256, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev()))
    for bad in (INF, -INF, float("nan")):
        for pos in (0, n - 1, (n // 4) * 4, (n // 4) * 4 - 1, 1024 * 4 + 1):      # first, last (tail), first tail entry, last vector entry, another workgroup
            g = base.clone()
            g[pos] = bad
            gstat, st, ticket = grad_norm(g, max_norm=1.0, scratch=scratch)
            assert float(gstat[2]) == 0.0 and not math.isfinite(float(gstat[0])), (bad, pos)
            assert int(ticket) == 0 and float(gstat[3]) == 0.0 and float(st) == 1.0      # skipping off: counted nowhere, the step goes on
    # the step counter and the skip count, all four cases of (ticked, skipped)
    g = base.clone()
    g[7] = float("nan")
    gstat = torch.zeros(4, device=dev())
    assert float(grad_norm(g, skip=True, step=5.0, ticked=True, gstat=gstat)[1]) == 4.0        # the loss launch's tick is taken back
    assert float(grad_norm(g, skip=True, step=4.0, ticked=False, gstat=gstat)[1]) == 4.0       # not ticked, not ticking
    assert gstat.tolist()[2:] == [0.0, 2.0]
    assert float(grad_norm(base, skip=True, step=5.0, ticked=True, gstat=gstat)[1]) == 5.0
    assert float(grad_norm(base, skip=True, step=4.0, ticked=False, gstat=gstat)[1]) == 5.0
    assert gstat.tolist()[2:] == [1.0, 2.0]                                                    # the count stays, ok is this step's


LR, WD, B1, B2, EPS = 8e-4, 1e-5, 0.9, 0.999, 1e-8


def _flat_state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (1.0 + k) for k in range(3)]
    return p0, grads


def _clipped_steps(p0, grads, max_norm, skip=False):
    """three updates through gaot_grad_norm_dev + gaot_adamw_apply_clipped_dev; returns (p, m, v, step, first norm)"""
    from gaot_amd.ops import _p, _stream
    L, lib = _lib()
    p, m, v = p0.to(dev()), torch.zeros_like(p0, device=dev()), torch.zeros_like(p0, device=dev())
    hyper = torch.tensor([LR, B1, B2, EPS, WD], device=dev())
    clip = torch.tensor([max_norm, 1.0 if skip else 0.0], device=dev())
    step, gstat = torch.zeros(1, device=dev()), torch.zeros(4, device=dev())
    part, ticket = torch.empty(256, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())
    first = None
    for g in grads:
        g = g.to(dev())
        keep = g.clone()
        L.check(lib.gaot_grad_norm_dev(_p(g), g.numel(), _p(part), _p(ticket), _p(clip), _p(step), 0, _p(gstat), _stream()), "gaot_grad_norm_dev")
        L.check(lib.gaot_adamw_apply_clipped_dev(_p(p), _p(g), _p(m), _p(v), g.numel(), _p(hyper), _p(step), _p(gstat), _p(clip), _stream()),
                "gaot_adamw_apply_clipped_dev")
        assert torch.equal(g.view(torch.int32), keep.view(torch.int32))  # the gradient buffer is not rewritten
        first = float(gstat[0]) if first is None else first
    return p, m, v, step, first


@pytest.mark.parametrize("n", [5, 1021, 65539])
def test_clipped_update_vs_torch_clip_grad_norm_and_adamw(n):
    from gaot_amd.ops import _p, _stream
    L, lib = _lib()
    p0, grads = _flat_state(n, seed=n)
    max_norm = 0.5 * float(grad_norm(grads[0].to(dev()))[0][0])          # half of the first step's MEASURED norm: clipping is active
    p, m, v, step, _ = _clipped_steps(p0, grads, max_norm)
    ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    for g in grads:
        ref.grad = g.double().clone()
        assert float(torch.nn.utils.clip_grad_norm_([ref], max_norm)) > max_norm
        opt.step()
    st = opt.state[ref]
    errs = [float((a.cpu().double() - b).abs().max()) for a, b in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"]))]
    print(f"[clipped adamw n={n}] max abs err p {errs[0]:.2e} m {errs[1]:.2e} v {errs[2]:.2e}")
    assert max(errs) < 2e-5 and float(step) == 3.0                       # the flat-AdamW tolerance of tests/test_model_gpu.py
    # a bound nothing reaches: multiplying by 1.0f is exact -> the bits of the plain flat update
    pc, mc, vc, stepc, _ = _clipped_steps(p0, grads, 1e30)
    pp, mp_, vp = p0.to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    hyper, stepp = torch.tensor([LR, B1, B2, EPS, WD], device=dev()), torch.zeros(1, device=dev())
    for g in grads:
        L.check(lib.gaot_adamw_step_dev(_p(pp), _p(g.to(dev())), _p(mp_), _p(vp), n, _p(hyper), _p(stepp), _stream()), "gaot_adamw_step_dev")
    assert torch.equal(pc, pp) and torch.equal(mc, mp_) and torch.equal(vc, vp) and torch.equal(stepc, stepp)
    assert not torch.equal(p, pp)                                        # (and the clipped run above was another run)


def test_clipped_update_skips_without_a_store():
    n = 1021
    p0, grads = _flat_state(n, seed=3)
    grads[1][n - 1] = float("nan")
    p, m, v, step, _ = _clipped_steps(p0, grads, 1.0, skip=True)
    q, mq, vq, stepq, _ = _clipped_steps(p0, [grads[0], grads[2]], 1.0, skip=True)
    assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq) and float(step) == float(stepq) == 2.0
    assert bool(torch.isfinite(p).all())


# ------------------------------------------------------------------------------------------------ the whole step
def _golden_setup(n_models):
    g = Golden("fx2d_base")
    lat, x, p, tgt = [g.t(k).to(dev()) for k in ("in.latent", "in.xcoord", "in.pndata", "in.target")]
    models = [build_model(g) for _ in range(n_models)]
    for m in models:
        m.train()
        seed_neighbor_cache(m, g, x, lat)
    return models, lat, x, p, tgt


def _params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _trainstep(model, data, **kw):
    from gaot_amd.trainer import TrainStep
    lat, x, p, tgt = data
    ts = TrainStep(model, lr=8e-4, weight_decay=1e-5, **kw)
    ts.bind(p, tgt, latent_tokens_coord=lat, xcoord=x)
    return ts


def test_trainstep_clipped_matches_clip_grad_norm_twin_eager_and_replayed():
    (m_e, m_g, m_b), *data = _golden_setup(3)
    lat, x, p, tgt = data
    opt = torch.optim.AdamW(m_b.parameters(), lr=8e-4, weight_decay=1e-5)
    torch.nn.functional.mse_loss(m_b(latent_tokens_coord=lat, xcoord=x, pndata=p), tgt).backward()
    c = 0.5 * float(torch.nn.utils.clip_grad_norm_(m_b.parameters(), INF))          # half of the twin's first-step norm (the grads stay as they are)
    ts_e = _trainstep(m_e, data, use_graph=False, max_grad_norm=c)
    ts_g = _trainstep(m_g, data, use_graph=True, max_grad_norm=c)
    n_flat = ts_g.bucket.numel
    for k in range(3):
        ts_e.step(); ts_g.step()
        opt.zero_grad()
        torch.nn.functional.mse_loss(m_b(latent_tokens_coord=lat, xcoord=x, pndata=p), tgt).backward()
        want = float(torch.nn.utils.clip_grad_norm_(m_b.parameters(), c))
        opt.step()
        assert want > c
        got = float(ts_g.grad_norm)
        print(f"[trainstep clip step {k}] grad_norm {got:.8g} twin {want:.8g} rel {abs(got - want) / want:.2e} coef {float(ts_g.opt.clip_coef):.6f}")
        assert abs(got - want) <= (norm_rel_bound(n_flat) + GRAD_L2_TOL) * want
        assert float(ts_e.grad_norm) == got and float(ts_g.opt.step_ok) == 1.0
    for (k, a), (_, b) in zip(m_g.named_parameters(), m_b.named_parameters()):
        assert float((a.detach() - b.detach()).abs().max()) < 2e-5, k
    assert torch.equal(_params(m_e), _params(m_g))                                     # replay == eager, bit for bit
    assert ts_g._graphs is not None and ts_g.skipped_steps == 0 and float(ts_g.opt.step_count) == 3.0


def test_trainstep_unreachable_bound_keeps_the_default_steps_bits():
    (m_c, m_d), *data = _golden_setup(2)
    ts_c = _trainstep(m_c, data, use_graph=True, max_grad_norm=1e30)
    ts_d = _trainstep(m_d, data, use_graph=True)
    assert ts_d.opt.clipping is False and ts_d.opt.gstat is None                       # nothing of the feature exists by default
    for _ in range(3):
        ts_c.step(); ts_d.step()
    assert torch.equal(_params(m_c), _params(m_d))
    assert torch.equal(ts_c.opt.m, ts_d.opt.m) and torch.equal(ts_c.opt.v, ts_d.opt.v) and torch.equal(ts_c.opt.step_count, ts_d.opt.step_count)
    assert float(ts_c.opt.clip_coef) == 1.0 and float(ts_c.grad_norm) > 0
    with pytest.raises(RuntimeError):
        ts_d.grad_norm


@pytest.mark.parametrize("graph", [True, False])
def test_skipped_step_is_bit_neutral(graph):
    (m_a, m_b), *data = _golden_setup(2)
    tgt = data[3]
    bad = tgt.clone()
    bad[0, 0, 0] = float("nan")                                                        # a NaN loss: arithmetic, not a fault
    ts = _trainstep(m_a, data, use_graph=graph, skip_nonfinite=True)
    twin = _trainstep(m_b, data, use_graph=graph, skip_nonfinite=True)
    ts.step()
    state = lambda t: [s.clone() for s in (t.opt.flat_p, t.opt.m, t.opt.v, t.opt.step_count)]
    before = state(ts)
    assert ts.skipped_steps == 0 and float(ts.opt.step_ok) == 1.0 and float(ts.opt.step_count) == 1.0      # (the capture's warm-up left nothing behind)
    loss = ts.step(target=bad)
    assert not math.isfinite(float(loss))
    assert all(torch.equal(a, b) for a, b in zip(state(ts), before))
    assert ts.skipped_steps == 1 and float(ts.opt.step_ok) == 0.0 and not math.isfinite(float(ts.grad_norm))
    ts.step(target=tgt)
    twin.step(); twin.step()
    assert all(torch.equal(a, b) for a, b in zip(state(ts), state(twin)))
    assert float(ts.opt.step_count) == 2.0 and ts.skipped_steps == 1 and float(ts.opt.step_ok) == 1.0
    assert ts.opt.state_dict()["state"][0]["step"] == 2.0                              # checkpoints count applied updates


def test_without_skip_nonfinite_the_bad_batch_destroys_the_run():
    """what the option is for"""
    (m_a,), *data = _golden_setup(1)
    bad = data[3].clone()
    bad[0, 0, 0] = float("nan")
    ts = _trainstep(m_a, data, use_graph=False)
    ts.step()
    ts.step(target=bad)
    ts.step(target=data[3])
    assert not bool(torch.isfinite(ts.opt.flat_p).all())


# ------------------------------------------------------------------------------------------------ staged, and a schedule
def _small(seed):
    from gaot_amd.model.gaot import GAOT
    from gaot_amd.model.layers.magno import MAGNOConfig
    from gaot_amd.model.layers.attn import TransformerConfig, AttentionConfig
    torch.manual_seed(seed)
    mcfg = MAGNOConfig(coord_dim=2, radius=0.08, hidden_size=64, mlp_layers=3, lifting_channels=32)
    tcfg = TransformerConfig(patch_size=2, hidden_size=128, attn_config=AttentionConfig(num_heads=4, num_kv_heads=4))
    return GAOT(2, 1, NS(args=NS(magno=mcfg, transformer=tcfg), latent_tokens_size=[32, 32])).to(dev()).train()


def _small_data():
    g = torch.Generator().manual_seed(21)
    ax = torch.linspace(-1, 1, 32)
    lat = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    x = torch.rand(1500, 2, generator=g) * 2 - 1
    return [t.to(dev()) for t in (lat, x, torch.randn(4, 1500, 2, generator=g), torch.randn(4, 1500, 1, generator=g))]


def _small_step(seed, data, **kw):
    from gaot_amd.trainer import TrainStep
    lat, x, p, t = data
    model = _small(seed)
    ts = TrainStep(model, lr=2e-3, weight_decay=1e-4, **kw)
    ts.bind(p, t, latent_tokens_coord=lat, xcoord=x)
    return model, ts


def test_staged_rccl_one_rank_group_takes_the_norm_after_the_last_exchange():
    import torch.distributed as dist
    data = _small_data()
    _, probe = _small_step(5, data, use_graph=False, staged=False, max_grad_norm=1e30)
    probe.step()
    c = 0.5 * float(probe.grad_norm)
    m_u, ts_u = _small_step(5, data, use_graph=False, staged=False, max_grad_norm=c)
    ts_u.step(); ts_u.step()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        m_s, ts_s = _small_step(5, data, use_graph=True, staged=True, max_grad_norm=c)
        assert ts_s.staged and len(ts_s.stage_groups) == 2
        ts_s.force_comm = True
        for k in range(2):
            ts_s.step()
            torch.cuda.synchronize()
            want = float(ts_s.bucket.flat.double().norm())           # the buffer after every group's exchange, still unclipped
            got = float(ts_s.grad_norm)
            assert abs(got - want) <= norm_rel_bound(ts_s.bucket.numel) * want
            assert k > 0 or (got > c and float(ts_s.opt.clip_coef) < 0.51)      # the first step is clipped to half
        assert ts_s._g_opt is not None and not ts_s._merged             # the norm sits in the optimizer's graph, after the waits
    finally:
        dist.destroy_process_group()
    assert float((_params(m_s) - _params(m_u)).abs().max()) < 2e-5


def test_schedule_moves_max_grad_norm_without_recapture():
    data = _small_data()
    _, ts = _small_step(5, data, use_graph=True, max_grad_norm=1e30)
    ts.step()
    n1 = float(ts.grad_norm)
    graphs = ts._graphs
    assert graphs is not None and float(ts.opt.clip_coef) == 1.0
    coefs = []
    for frac in (0.02, 0.005):                                   # far below the norm even where the first steps shrink it severalfold
        c = frac * n1
        ts.opt.param_groups[0]["max_grad_norm"] = c
        ts.step()
        norm = ts.grad_norm.clone()
        want = float(torch.tensor(c, dtype=torch.float32, device=dev()) / (norm + 1e-6))
        coefs.append(float(ts.opt.clip_coef))
        assert want < 1.0 and abs(coefs[-1] - want) <= 4 * U * want      # one rounding each for the sum and the quotient, doubled
        assert ts._graphs is graphs
    assert coefs[1] != coefs[0]
