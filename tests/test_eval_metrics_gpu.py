"""-m gpu: the reference's test metric on the device (gaot_amd/metrics.py over csrc/metrics.hip: gaot_rel_l1_errors, gaot_median_mean).

The bar of every relative-L1 entry is the project's rule, three times the reference's own rounding:  |e - e64| <= (3 d + 2^-22) e64,  with e64
the float64 evaluation and d the recorded distance of the reference's fp32 result from it (tests/golden/eval_metrics.npz; for the seeded large
case, tests/_metrics_ref.py in both precisions); the additive term covers the three final roundings (numerator, denominator, quotient).
Medians are selections: bit-equal to torch.median on the CPU."""
import ctypes as C

import pytest
import torch

from tests import _metrics_ref as R

pytestmark = pytest.mark.gpu

CASES, FINALS = R.load_fixture()


def dev():
    return torch.device("cuda:0")


def check_bar(e, e64, d, what):
    e, e64 = e.detach().cpu().double(), e64.double()
    assert e.shape == e64.shape, (what, e.shape, e64.shape)
    dist = ((e - e64).abs() / e64.abs())
    bar = 3.0 * d + 2.0 ** -22
    print(f"[{what}] worst |e - e64| / e64 = {float(dist.max()):.3e}   bar 3d + 2^-22 = {bar:.3e}   (d = {d:.2e})")
    assert bool(((e - e64).abs() <= bar * e64.abs()).all()), (what, float(dist.max()), bar)


def device_inputs(c):
    """the tensors a caller of the reference's function would hold for this case, on the device, layouts kept: `last_t` is the [:, -1:] VIEW"""
    g, p = c["gtr"].to(dev()), c["prd"].to(dev())
    if c["how"] == "last_t":
        g, p = g[:, -1:], p[:, -1:]
        assert not g.is_contiguous()
    return g, p


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_within_three_times_the_reference_rounding(name):
    from gaot_amd import metrics
    c = CASES[name]
    g, p = device_inputs(c)
    if c["how"] == "denorm":
        um, us = c["u_mean"].to(dev()), c["u_std"].to(dev())
        check_bar(metrics.compute_batch_errors(g, p, c["meta"], denorm=(um, us)), c["ref64"], c["d"], name + " denorm in the kernel")
        check_bar(metrics.compute_batch_errors(g * us + um, p * us + um, c["meta"]), c["ref64"], c["d"], name + " denorm by torch")
        return
    out = metrics.compute_batch_errors(g, p, c["meta"])
    assert out.dtype == torch.float32 and out.is_cuda
    check_bar(out, c["ref64"], c["d"], name)
    if name == "v2_truth_is_mean":
        assert bool(torch.isfinite(out).all()) and float(out[:, 1].min()) > 1e6          # denominator 1e-10 alone: large, finite


def test_scalar_path_for_a_base_offset_by_one_float():
    from gaot_amd import metrics
    c = CASES["v3_n257_b5"]

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=dev(), dtype=torch.float32)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    check_bar(metrics.compute_batch_errors(shifted(c["gtr"]), shifted(c["prd"]), c["meta"]), c["ref64"], c["d"], "offset by one float")
    # the vector path on the same data gives the same bits: the same per-element arithmetic, the same fixed tree
    a = metrics.compute_batch_errors(shifted(c["gtr"]), shifted(c["prd"]), c["meta"])
    b = metrics.compute_batch_errors(c["gtr"].to(dev()), c["prd"].to(dev()), c["meta"])
    assert torch.equal(a, b)


def test_step_major_rollout_slab_goes_in_as_a_permuted_view():
    from gaot_amd import metrics
    c = CASES["v5_t3_b5"]
    slab_g = c["gtr"].permute(1, 0, 2, 3).contiguous().to(dev())          # [T, B, N, V]: what the device rollout fills step by step
    slab_p = c["prd"].permute(1, 0, 2, 3).contiguous().to(dev())
    g, p = slab_g.permute(1, 0, 2, 3), slab_p.permute(1, 0, 2, 3)
    assert not g.is_contiguous() and g.stride(1) > g.stride(0)
    check_bar(metrics.compute_batch_errors(g, p, c["meta"]), c["ref64"], c["d"], "step-major slab")
    # a layout the kernel cannot stride (inner block not contiguous) is made contiguous by the wrapper
    gv = c["gtr"].permute(0, 1, 3, 2).contiguous().to(dev()).permute(0, 1, 3, 2)
    assert gv.stride(3) != 1
    check_bar(metrics.compute_batch_errors(gv, c["prd"].to(dev()), c["meta"]), c["ref64"], c["d"], "variable-major input")


def test_nan_in_one_prediction_poisons_its_entry_only():
    from gaot_amd import metrics
    c = CASES["v3_n257_b5"]
    g, p = c["gtr"].to(dev()), c["prd"].to(dev())
    clean = metrics.compute_batch_errors(g, p, c["meta"])
    p2 = p.clone()
    p2[2, 0, 5, 1] = float("nan")                      # variable 1 -> chunk 1 of sample 2
    out = metrics.compute_batch_errors(g, p2, c["meta"])
    assert bool(torch.isnan(out[2, 1]))
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[2, 1] = False
    assert torch.equal(out[mask], clean[mask])


def test_refusals():
    from gaot_amd import _lib, metrics
    c = CASES["v3_n257_b5"]
    with pytest.raises(TypeError, match="fp32"):
        metrics.compute_batch_errors(c["gtr"].to(dev()).double(), c["prd"].to(dev()).double(), c["meta"])
    with pytest.raises(ValueError):
        metrics.compute_batch_errors(c["gtr"].to(dev())[..., :2], c["prd"].to(dev())[..., :2], c["meta"])
    wide = R.Meta(list(range(33)), list(range(33)), [0.0] * 33, [1.0] * 33)
    with pytest.raises(ValueError, match="32"):
        metrics.compute_batch_errors(torch.zeros(1, 1, 2, 33, device=dev()), torch.zeros(1, 1, 2, 33, device=dev()), wide)
    x = torch.zeros(64, device=dev())
    z = torch.zeros(64, device=dev(), dtype=torch.int32)
    rc = _lib.load().gaot_rel_l1_errors(x.data_ptr(), 0, 0, x.data_ptr(), 0, 0, 1, 1, 1, 33, None, None, x.data_ptr(), x.data_ptr(), z.data_ptr(), 1,
                                        x.data_ptr(), x.data_ptr(), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"32" in _lib.load().gaot_last_error()


@pytest.fixture(scope="module")
def large():
    """[2, 8, 65536, 4]: 64 workgroups per sample; the float64 / fp32 yardsticks computed once on the CPU and left alone"""
    ce = CASES["ce_gauss_last_t"]["meta"]
    g = torch.Generator().manual_seed(2024)
    m = torch.tensor(ce.global_mean, dtype=torch.float32)
    s = torch.tensor(ce.global_std, dtype=torch.float32)
    gtr = m + s * torch.randn(2, 8, 65536, 4, generator=g)
    prd = gtr + 0.1 * s * torch.randn(2, 8, 65536, 4, generator=g)
    e64 = R.batch_errors(gtr.double(), prd.double(), ce)
    e32 = R.batch_errors(gtr, prd, ce)
    d = float(((e32.double() - e64).abs() / e64.abs()).max())
    return dict(meta=ce, gtr=gtr.to(dev()), prd=prd.to(dev()), e64=e64, d=d)


def test_multi_workgroup_case_against_float64(large):
    from gaot_amd import _lib, metrics
    assert _lib.load().gaot_rel_l1_errors_workspace(2, 8, 65536, 4) > 2 * 2 * 2 * 4 * 2          # more than one workgroup per sample
    check_bar(metrics.compute_batch_errors(large["gtr"], large["prd"], large["meta"]), large["e64"], large["d"], "[2, 8, 65536, 4]")
    # the [:, -1:] view of the same tensors: rows 512 KB apart
    ce = large["meta"]
    g, p = large["gtr"][:, -1:], large["prd"][:, -1:]
    e64 = R.batch_errors(g.cpu().double(), p.cpu().double(), ce)
    e32 = R.batch_errors(g.cpu(), p.cpu(), ce)
    check_bar(metrics.compute_batch_errors(g, p, ce), e64, float(((e32.double() - e64).abs() / e64.abs()).max()), "[2, 8, 65536, 4][:, -1:]")


def _raw_call(lib, g, p, tab, ws, out):
    from gaot_amd import _lib
    B, T, N, V = g.shape
    _lib.check(lib.gaot_rel_l1_errors(g.data_ptr(), g.stride(0), g.stride(1), p.data_ptr(), p.stride(0), p.stride(1), B, T, N, V, None, None,
                                      tab.mean.data_ptr(), tab.std.data_ptr(), tab.chunks.data_ptr(), tab.C, ws.data_ptr(), out.data_ptr(), out.stride(0),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gaot_rel_l1_errors")


def test_deterministic_workspace_independent_and_graph_safe(large):
    from gaot_amd import _lib, metrics
    lib = _lib.load()
    g, p = large["gtr"], large["prd"]
    tab = metrics._tables(large["meta"], dev())
    n_ws = lib.gaot_rel_l1_errors_workspace(*g.shape)
    outs = []
    for fill in (0.0, float("nan"), 7.0):          # whatever the workspace and the output held before
        ws = torch.full((n_ws // 2,), fill, device=dev(), dtype=torch.float64)
        out = torch.full((2, tab.C), fill, device=dev(), dtype=torch.float32)
        _raw_call(lib, g, p, tab, ws, out)
        outs.append(out.clone())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], metrics.compute_batch_errors(g, p, large["meta"]))
    # inside a captured graph, replayed on edited inputs: the bits of an eager call on the same inputs
    gs, ps = g.clone(), p.clone()
    ws = torch.full((n_ws // 2,), float("nan"), device=dev(), dtype=torch.float64)
    out = torch.empty(2, tab.C, device=dev(), dtype=torch.float32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _raw_call(lib, gs, ps, tab, ws, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw_call(lib, gs, ps, tab, ws, out)
    for k in range(2):
        ps.copy_(p + 0.01 * (k + 1))
        graph.replay()
        assert torch.equal(out, metrics.compute_batch_errors(gs, ps, large["meta"])), k
        assert not torch.equal(out, outs[0])


# ------------------------------------------------------------------------------------------------ gaot_median_mean
def _columns(n, seed):
    """[n, 5] columns: plain, heavy ties, an inf, a NaN (n > 1), all equal"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 5, generator=g)
    x[:, 1] = torch.randint(0, 3, (n,), generator=g).float() * 0.25
    x[n // 2, 2] = float("inf")
    if n > 1:
        x[n // 3, 3] = float("nan")
    x[:, 4] = 0.125
    return x


@pytest.mark.parametrize("n", [1, 2, 7, 8, 1500])
def test_median_is_the_lower_median_bit_for_bit(n):
    from gaot_amd import metrics
    x = _columns(n, seed=n)
    want = torch.median(x, dim=0).values
    got = metrics.chunk_medians(x.to(dev())).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok].view(torch.int32), want[ok].view(torch.int32)), (n, got, want)
    if n > 1:
        assert bool(torch.isnan(got[3])) and metrics.compute_final_metric(x.to(dev())) != metrics.compute_final_metric(x.to(dev()))     # NaN metric
    # the finite columns alone: the metric is the mean of their medians
    cols = [0, 1, 4] + ([2] if n > 2 else [])          # (n <= 2: the inf IS the column's lower median or its only entry)
    sub = x[:, cols].contiguous()
    exact = float(torch.median(sub.double(), dim=0).values.mean())
    m = metrics.compute_final_metric(sub.to(dev()))
    assert abs(m - exact) <= len(cols) * 2.0 ** -24 * abs(exact), (n, m, exact)
    # a strided log: the same columns read out of a wider buffer
    wide = torch.full((n, 9), 5.0, device=dev())
    wide[:, 2:2 + len(cols)] = sub.to(dev())
    view = wide[:, 2:2 + len(cols)]
    assert view.stride(0) == 9
    assert metrics.compute_final_metric(view) == m
    assert metrics.compute_final_metric(view) == m          # deterministic


@pytest.mark.parametrize("tag", sorted(FINALS))
def test_final_metric_fixture(tag):
    from gaot_amd import metrics
    f = FINALS[tag]
    m = metrics.compute_final_metric(f["errs"].to(dev()))
    assert abs(m - f["ref64"]) <= 3 * 2.0 ** -24 * f["ref64"]


def test_error_log_in_three_uneven_appends_equals_one_call():
    from gaot_amd import metrics
    c = CASES["v5_t3_b5"]
    g, p = c["gtr"].to(dev()), c["prd"].to(dev())
    whole = metrics.compute_batch_errors(g, p, c["meta"])
    log = metrics.ErrorLog(8, c["meta"], device=dev())
    log.rows.fill_(float("nan"))
    for lo, hi in ((0, 1), (1, 4), (4, 5)):
        rows = log.append(g[lo:hi], p[lo:hi])
        assert rows.data_ptr() == log.rows[lo].data_ptr()          # written in place
    assert log.count == 5 and torch.equal(log.errors(), whole)
    assert bool(torch.isnan(log.rows[5:]).all())                   # nothing past the rows appended
    assert log.final_metric() == metrics.compute_final_metric(whole) == pytest.approx(R.final_metric(whole.cpu()), rel=4 * 2.0 ** -24)
    with pytest.raises(ValueError, match="capacity"):
        log.append(g[:4], p[:4])
