"""The gene decoding's read-out apply pass and map forward as one launch (igcn_node_linear_bn_apply_map_fwd) against the
launches it replaces — igcn_node_linear_bn_fwd followed by igcn_spmm_fwd — bit for bit, on a hand-built map; and one
train step of the full model with the fusion on (this process) and off (a child under the library option bit
IGCN_NO_MAP_FUSED)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _decode_map():
    """Decode structure [6 SNP rows, 700 GO-node columns] (700 = 10 * 64 + 60 nodes for the 512 threads that compute the
    read-out: some own two).  Row lengths (the lists the walk sums): 230 (> 64 * SPMM_LU =
    192: the tail loop), 70 (two stride-64 trips), 64, 13, 1 and 0 (a SNP no node feeds); 378 non-zeros > 8 rows, so
    igcn_spmm_fwd walks them with the long-list kernel."""
    from igcn_amd import ops
    rng = np.random.default_rng(11)
    n_i, n_j = 700, 6
    rows, cols = [], []
    for j, n in enumerate((230, 70, 64, 13, 1, 0)):
        r = np.sort(rng.choice(n_i, size=n, replace=False))
        rows += r.tolist()
        cols += [j] * n
    rows, cols = np.asarray(rows), np.asarray(cols)
    o = np.argsort(cols * n_i + rows)
    return ops.Csr(torch.from_numpy(cols[o]), torch.from_numpy(rows[o]), n_j, n_i, "cuda")


# ------------------------------------------------------------------------------------------------ read-out + decode
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_keep", [True, False])
@pytest.mark.parametrize("groups", [1, 2])
def test_readout_apply_and_decode_map_as_one_launch_bit_for_bit(groups, with_keep, training):
    """igcn_node_linear_bn_apply_map_fwd against igcn_node_linear_bn_fwd (F = 2, D = 1) followed by igcn_spmm_fwd on the
    structure of _decode_map() (6 SNP rows over 700 nodes, the first one 230 entries long: beyond 64 * SPMM_LU): out_d,
    x_d, the saved and the running statistics bit for bit."""
    from igcn_amd import _lib
    from igcn_amd._lib import call, ptr, stream_ptr
    lib = _lib.load()
    dec = _decode_map()
    b, f_in, n, n_j, nnz = 6, 2, dec.n_cols, dec.n_rows, dec.nnz
    assert lib.igcn_node_linear_bn_apply_map_ok(f_in, 1, n, n_j, nnz) == 1
    rng = np.random.default_rng(7 + groups)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s)).float().cuda()     # noqa: E731
    x, w, gamma, beta, val = f(b, f_in, n), f(1, f_in), f(n), f(n), f(1, nnz)
    keep = (torch.from_numpy(rng.integers(0, 2, size=(b, n))).float() * 2.0).cuda() if with_keep else None
    rm0, rv0 = f(n), f(n).abs() + 0.5

    def run(fused):
        rm, rv = rm0.clone(), rv0.clone()
        out = torch.full((b, n, 1), float("nan"), device="cuda")
        mean, rstd = torch.empty(groups, n, device="cuda"), torch.empty(groups, n, device="cuda")
        sc = torch.empty(int(lib.igcn_node_linear_bn_scratch_floats(b, n, groups)), device="cuda")
        y = torch.full((b, 1, n_j), float("nan"), device="cuda")
        head = (ptr(x), ptr(w), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), int(training), 0.1, 1e-5, ptr(keep), ptr(out),
                ptr(mean), ptr(rstd), ptr(sc))
        if fused:
            call("igcn_node_linear_bn_apply_map_fwd", b, f_in, n, groups, *head, n_j, nnz, ptr(dec.row_ptr), ptr(dec.col),
                 ptr(val), nnz, ptr(y), stream_ptr())
        else:
            call("igcn_node_linear_bn_fwd", b, f_in, n, 1, groups, *head, stream_ptr())
            call("igcn_spmm_fwd", b, 1, n_j, n, nnz, ptr(dec.row_ptr), ptr(dec.col), ptr(val), ptr(out), ptr(y), stream_ptr())
        torch.cuda.synchronize()
        return out, y, mean, rstd, rm, rv

    want, got = run(False), run(True)
    assert not torch.isnan(want[0]).any() and not torch.isnan(want[1]).any()
    assert bool((want[0] > 0).any())
    for name, g, w_ in zip(("out_d", "x_d", "mean", "rstd", "running_mean", "running_var"), got, want):
        assert torch.equal(g, w_), name
    assert torch.equal(got[4], rm0) != training          # (the running statistics move in training only)


# ------------------------------------------------------------------------------------------------ model level
FUSED = "igcn_node_linear_bn_apply_map_fwd"


def train_step(record):
    """One train step of the ``full_b32`` model with the maps on the CSR kernels (SPARSE_MIN_BATCH = 0; a 32-graph step
    would take the dense images): loss, every gradient, data.x.grad, and the names of the entry points called."""
    from conftest import load_golden
    from igcn_amd import ops
    from igcn_amd.data import Batch
    from igcn_amd.train import FlatAdam, _single_use_parameters, backward_to_grads, losses
    from test_gpu_model import _full_model
    store = load_golden("full_b32")
    ops.SparseMap.SPARSE_MIN_BATCH = 0
    model, graphs, _ = _full_model(store)
    model.train(True)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = Batch.from_data_list(graphs).to("cuda")
    opt.zero_grad()
    seen = record()
    loss, _, _ = losses(model, data, store["lam"].tolist())
    defer = _single_use_parameters(model)
    backward_to_grads(loss, opt, data, defer=defer)
    torch.cuda.synchronize()
    out = {"grad " + k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    out["data.x.grad"] = data.x.grad.cpu().numpy()
    out["loss"] = loss.detach().cpu().numpy()
    return out, [n[0] for n in seen], defer


_CHILD = r"""
import sys
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import numpy as np
import igcn_amd  # noqa: F401
import test_gpu_map_fused as T
from calltrace import record_calls
class MP:
    setattr = staticmethod(setattr)
out, names, _ = T.train_step(lambda: record_calls(MP))
np.savez(sys.argv[4], __calls=np.array(names), **out)
"""


def test_train_step_is_bit_equal_with_and_without_the_fusion(monkeypatch, tmp_path):
    """Loss, every parameter gradient and data.x.grad of one deferred train step: equal bit for bit between the default
    route (ops.NodeLinearBN with the map as its rider: one launch for the decode read-out's apply pass and the map) and the child's (option bit:
    igcn_node_linear_bn_fwd at D = 1 in front of igcn_spmm_fwd).  The call records show each route."""
    from calltrace import record_calls
    from igcn_amd import ops
    monkeypatch.setattr(ops.SparseMap, "SPARSE_MIN_BATCH", ops.SparseMap.SPARSE_MIN_BATCH)     # restored afterwards
    got, names, defer = train_step(lambda: record_calls(monkeypatch))
    assert defer
    assert names.count(FUSED) == 1 and "igcn_node_linear_bn_fwd" not in names
    map_fwd = [n for n in names if n.startswith("igcn_spmm_fwd")]
    script, out = tmp_path / "child.py", tmp_path / "child.npz"
    script.write_text(_CHILD)
    env = {**os.environ, "IGCN_NO_MAP_FUSED": "1"}
    r = subprocess.run([sys.executable, str(script), ROOT, HERE, os.path.join(HERE, "golden"), str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = np.load(out)
    child = want["__calls"].tolist()
    assert FUSED not in child and child.count("igcn_node_linear_bn_fwd") == 1
    assert len([n for n in child if n.startswith("igcn_spmm_fwd")]) == len(map_fwd) + 1
    assert [n for n in child if "bwd" in n] == [n for n in names if "bwd" in n]          # the backward is the same calls
    assert set(want.files) - {"__calls"} == set(got)
    assert len(got) > 40
    for k, g in got.items():
        assert g.tobytes() == want[k].tobytes(), k
