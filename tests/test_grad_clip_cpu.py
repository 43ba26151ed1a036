"""Global gradient-norm clipping and the non-finite step skip, the parts that need no GPU: the data-parallel semantics over gloo
(world 2, TrainStep's CPU branch: clip_grad_norm_ + a host-side finite check), FlatAdamW's constructor / state_dict with the
feature off and on, and the C ABI of the two new entries."""
import os
import re
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gaot_amd.trainer import FlatAdamW, FlatGradBucket, TrainStep, shard_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 0.05          # well below the gradient norm of TwoLayer on _data() (asserted), so every step is clipped


class TwoLayer(torch.nn.Module):
    """GAOT's call convention (keyword `pndata`) and a cut point; every parameter receives a gradient"""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(3, 16)
        self.b = torch.nn.Linear(16, 2, bias=False)

    def forward(self, pndata):
        from gaot_amd import ops
        return self.b(ops.cut(torch.tanh(self.a(pndata))))

    def backward_phases(self):
        return [[self.b.weight], [self.a.weight, self.a.bias]]


def _data():
    g = torch.Generator().manual_seed(7)
    return torch.randn(8, 5, 3, generator=g), torch.randn(8, 5, 2, generator=g)


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, mode, staged):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = TwoLayer(seed=100 + rank)                       # ranks start different; rank 0 is broadcast
    x_all, y_all = _data()
    idx = shard_indices(8, rank, world, shuffle=False)
    res = {}
    if mode == "clip":
        ts = TrainStep(model, lr=1e-2, weight_decay=1e-3, staged=staged, max_grad_norm=MAX_NORM)
        ts.bind(x_all[idx], y_all[idx])
        res["norms"] = []
        for _ in range(3):
            ts.step()
            res["norms"].append(float(ts.grad_norm))
        res["skipped"] = ts.skipped_steps
    else:
        ts = TrainStep(model, lr=1e-2, weight_decay=1e-3, staged=staged, skip_nonfinite=True)
        ts.bind(x_all[idx], y_all[idx])
        ts.step()
        res["before"] = _flat(model).tolist()
        state = ts.opt.state_dict()["state"]
        res["steps_before"] = [float(st["step"]) for st in state.values()]
        bad = y_all[idx].clone()
        if rank == 1:                                       # the bad batch reaches ONE rank only
            bad[0, 0, 0] = float("nan")
        ts.step(target=bad)
        res["after_bad"] = _flat(model).tolist()
        res["norm_finite"] = bool(torch.isfinite(ts.grad_norm))
        res["skipped"] = ts.skipped_steps
        state = ts.opt.state_dict()["state"]
        res["steps_after_bad"] = [float(st["step"]) for st in state.values()]
        ts.step(target=y_all[idx])
        res["skipped_end"] = ts.skipped_steps
    res["final"] = _flat(model).tolist()
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        out.put(gathered)
    dist.barrier()
    dist.destroy_process_group()


def _run_two(mode, staged):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, mode, staged)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _single_process(steps, max_norm):
    """plain torch on the concatenated batch: mean of the per-rank mean losses == the global mean loss (equal shards)"""
    model = TwoLayer(seed=100)
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=1e-3)
    x_all, y_all = _data()
    norms = []
    for _ in range(steps):
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(pndata=x_all), y_all).backward()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return _flat(model), norms


def test_two_rank_gloo_clipped_step_matches_single_process_clip_grad_norm():
    """clipping on, world 2, the staged default and the single all-reduce: both ranks end bit-identical, equal to clip_grad_norm_ +
    AdamW on the global batch, and report the norm of the AVERAGED gradient"""
    ref, norms = _single_process(3, MAX_NORM)
    assert min(norms) > 2 * MAX_NORM                         # clipping is active at every step
    for staged in (None, False):
        r0, r1 = _run_two("clip", staged)
        assert r0["final"] == r1["final"]
        assert torch.allclose(torch.tensor(r0["final"]), ref, rtol=1e-5, atol=1e-6)
        assert r0["norms"] == r1["norms"] and r0["skipped"] == r1["skipped"] == 0
        assert torch.allclose(torch.tensor(r0["norms"]), torch.tensor(norms), rtol=1e-5)
    unclipped, _ = _single_process(3, None)
    assert not torch.allclose(ref, unclipped, rtol=1e-3, atol=1e-4)      # and the clipped run is another run


def test_two_rank_gloo_nan_on_one_rank_skips_on_both():
    """skip_nonfinite, a NaN target on rank 1 only: the NaN reaches rank 0 through the sum, both ranks skip, parameters and torch's step
    counters stay where they were, and the next good step goes on from there on both ranks alike"""
    r0, r1 = _run_two("skip", None)
    for r in (r0, r1):
        assert r["after_bad"] == r["before"]                 # bit-equal to the pre-step values
        assert r["skipped"] == 1 and r["skipped_end"] == 1 and not r["norm_finite"]
        assert r["steps_after_bad"] == r["steps_before"] and set(r["steps_before"]) == {1.0}
        assert r["final"] != r["before"] and all(v == v for v in r["final"])
    assert r0["before"] == r1["before"] and r0["after_bad"] == r1["after_bad"] and r0["final"] == r1["final"]
    ref, _ = _single_process(2, None)                        # the two good steps alone
    assert torch.allclose(torch.tensor(r0["final"]), ref, rtol=1e-5, atol=1e-6)


def _bucket():
    torch.manual_seed(0)
    lin = torch.nn.ModuleList([torch.nn.Linear(8, n, bias=(n == 12)) for n in (4, 12, 4, 8)])
    return lin, FlatGradBucket(list(lin.parameters()), groups=[[lin[0].weight, lin[2].weight, lin[3].weight]])


def test_flat_adamw_feature_off_is_unchanged():
    lin, bucket = _bucket()
    opt = FlatAdamW(bucket, lr=3e-4, weight_decay=1e-5)
    assert opt.clipping is False and opt.clip is None and opt.gstat is None
    assert "max_grad_norm" not in opt.param_groups[0] and "skip_nonfinite" not in opt.param_groups[0]
    opt.step_count.fill_(2.0)
    sd = opt.state_dict()
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in lin.parameters()], lr=3e-4, weight_decay=1e-5)
    assert sd["param_groups"][0].keys() == ref.state_dict()["param_groups"][0].keys()      # torch's own keys, nothing added
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    for name in ("grad_norm", "clip_coef", "step_ok", "skipped_steps"):
        try:
            getattr(opt, name)
        except RuntimeError:
            continue
        raise AssertionError(f"{name} must not exist silently with the feature off")


def test_flat_adamw_feature_on_state_dict_roundtrip_and_torch_loads_it():
    lin, bucket = _bucket()
    opt = FlatAdamW(bucket, lr=3e-4, weight_decay=1e-5, max_grad_norm=0.5, skip_nonfinite=True)
    assert opt.clipping and opt.clip.tolist() == [0.5, 1.0] and opt.gstat.tolist() == [0.0] * 4
    assert opt.grad_norm.dim() == 0 and opt.clip_coef.dim() == 0 and opt.step_ok.dim() == 0 and opt.skipped_steps == 0
    assert opt.grad_norm.data_ptr() == opt.gstat.data_ptr()                  # views of the record, not copies
    opt.m.copy_(torch.randn_like(opt.m)); opt.v.copy_(torch.rand_like(opt.v)); opt.step_count.fill_(7.0)
    opt.param_groups[0]["max_grad_norm"] = 0.25                                # a schedule moves it; sync_hyper uploads it
    opt.sync_hyper()
    assert opt.clip.tolist() == [0.25, 1.0]
    opt.param_groups[0]["max_grad_norm"] = None                                # None: no clipping, the guard stays
    opt.sync_hyper()
    assert opt.clip.tolist() == [float("inf"), 1.0]
    opt.param_groups[0]["max_grad_norm"] = 0.25
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 0.25 and sd["param_groups"][0]["skip_nonfinite"] is True
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in lin.parameters()], lr=1.0)
    ref.load_state_dict(sd)                                                    # torch accepts the extra keys
    assert ref.param_groups[0]["lr"] == 3e-4 and all(float(st["step"]) == 7.0 for st in ref.state.values())
    lin2, bucket2 = _bucket()
    opt2 = FlatAdamW(bucket2, lr=1.0, weight_decay=0.0, max_grad_norm=9.0)
    opt2.load_state_dict(sd)
    assert opt2.lr == 3e-4 and opt2.param_groups[0]["max_grad_norm"] == 0.25 and opt2.param_groups[0]["skip_nonfinite"] is True
    assert opt2.clip.tolist() == [0.25, 1.0] and float(opt2.step_count) == 7.0
    for a, b in zip(opt2._views(opt2.m) + opt2._views(opt2.v), opt._views(opt.m) + opt._views(opt.v)):
        assert torch.equal(a, b)                                               # (alignment padding is not state)
    opt3 = FlatAdamW(_bucket()[1], lr=1.0, weight_decay=0.0)                   # built without the feature: the keys are ignored
    opt3.load_state_dict(sd)
    assert not opt3.clipping and "max_grad_norm" not in opt3.param_groups[0]


def test_new_entries_exported_and_declared_with_matching_arity():
    from gaot_amd.build import build
    from gaot_amd import _lib
    build(verbose=False)
    lib = _lib.load()
    assert lib.gaot_abi_version() == 10                                        # an addition only
    header = open(os.path.join(ROOT, "include", "gaot_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gaot_grad_norm_dev", "gaot_adamw_apply_clipped_dev"):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gaot_hip.h"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
        assert "gaot_stream_t" in m.group(1).split(",")[-1]
