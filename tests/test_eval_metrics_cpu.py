"""CPU side of the evaluation metric (gaot_amd/metrics.py, csrc/metrics.hip): the plain-torch restatement in tests/_metrics_ref.py reproduces
what the reference recorded in tests/golden/eval_metrics.npz (float64 to 1e-12, fp32 bit for bit, the pooled 3-D case and the CE-Gauss index
mapping included); the new entry points are exported, declared and bound with matching arity inside ABI 10; host tensors are refused."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, FINALS = R.load_fixture()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_recorded_reference(name):
    c = CASES[name]
    e64 = R.batch_errors(*R.reference_inputs(c, torch.float64), c["meta"])
    assert e64.shape == c["ref64"].shape
    assert float(((e64 - c["ref64"]).abs() / c["ref64"].abs()).max()) <= 1e-12
    e32 = R.batch_errors(*R.reference_inputs(c, torch.float32), c["meta"])
    assert e32.dtype == torch.float32 and torch.equal(e32, c["ref32"])
    d = float(((e32.double() - e64).abs() / e64.abs()).max())
    assert d == c["d"] and 0.0 < d < 1e-5          # the recorded rounding of the reference is not zero: a bar built on it is not vacuous


def test_quirks_pinned_by_the_fixture():
    ce = CASES["ce_gauss_last_t"]["meta"]
    assert len(ce.chunked_variables) == 5 and len(ce.active_variables) == 4          # CE-Gauss: five chunk entries, four active variables
    assert R.chunk_table(ce) == ([0, 1, 1, 2], 3)
    assert R.chunk_table(CASES["v5_t3_b5"]["meta"]) == ([0, 1, 1, 2, 3], 4)            # ids renumbered densely: the skipped entry leaves no hole
    pooled = CASES["ce_gauss_pooled_3d"]
    assert pooled["gtr"].dim() == 3 and pooled["gtr"].shape[0] == 5 and tuple(pooled["ref32"].shape) == (1, 3)      # ONE row for the batch
    flat = CASES["v2_truth_is_mean"]
    assert bool(torch.isfinite(flat["ref32"]).all()) and float(flat["ref32"][:, 1].min()) > 1e6          # denominator = 1e-10 alone


@pytest.mark.parametrize("tag", sorted(FINALS))
def test_final_metric_restatement(tag):
    f = FINALS[tag]
    assert R.final_metric(f["errs"]) == f["ref32"]
    assert abs(R.final_metric(f["errs"].double()) - f["ref64"]) <= 1e-12 * f["ref64"]
    n = f["errs"].shape[0]
    low = torch.sort(f["errs"], dim=0).values[(n - 1) // 2]          # the LOWER median: rank (n - 1) // 2, an input element
    assert torch.equal(torch.median(f["errs"], dim=0).values, low)


def test_new_entries_exported_and_declared_with_matching_arity():
    from gaot_amd.build import build, SOURCES
    from gaot_amd import _lib
    assert "metrics.hip" in SOURCES and len(SOURCES) == 16
    build(verbose=False)
    lib = _lib.load()
    assert lib.gaot_abi_version() == 10                                        # additions only
    header = open(os.path.join(ROOT, "include", "gaot_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, ret in (("gaot_rel_l1_errors", "int"), ("gaot_median_mean", "int"), ("gaot_mse_loss_eval", "int"),
                      ("gaot_rel_l1_errors_workspace", "int64_t")):
        assert hasattr(lib, name), name
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gaot_hip.h"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
        if ret == "int":
            assert "gaot_stream_t" in m.group(1).split(",")[-1]
    # the size query is host arithmetic: it answers without a device, and refuses what the kernel refuses
    assert lib.gaot_rel_l1_errors_workspace(2, 8, 65536, 4) > 0
    assert lib.gaot_rel_l1_errors_workspace(2, 8, 65536, 33) == 0 and lib.gaot_rel_l1_errors_workspace(0, 1, 1, 1) == 0


def test_metrics_refuse_host_tensors():
    from gaot_amd import metrics
    c = CASES["v3_n257_b5"]
    with pytest.raises(RuntimeError, match="device tensors only"):
        metrics.compute_batch_errors(c["gtr"], c["prd"], c["meta"])
    with pytest.raises(RuntimeError, match="device tensors only"):
        metrics.compute_final_metric(torch.rand(5, 2))
    with pytest.raises(RuntimeError, match="device tensors only"):
        metrics.ErrorLog(8, c["meta"], device="cpu")
    with pytest.raises(TypeError):
        metrics.compute_batch_errors(np.zeros((1, 1, 1, 3), dtype=np.float32), np.zeros((1, 1, 1, 3), dtype=np.float32), c["meta"])


def test_nothing_under_gaot_amd_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gaot_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)
