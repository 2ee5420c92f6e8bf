"""GPU: the first-order PageRank operators built on the device (csrc/pagerank.hip via pagerank.py) -- DiGCN's
`get_appr_directed_adj` and DiGCL's `cal_fast_appr` on CUDA inputs -- against the reference's fixtures, the host (CPU)
path, and themselves (determinism)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import torch

from conftest import load_golden
from tolerance import close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def adjs():
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    return A


def host_appr_pi(ei, n, alpha, w):
    A = adjs()
    pi = A._perron_left_vector(A._transition(ei, w, n, torch.float32), alpha, n, dense_limit=0)
    return pi / pi.sum()


def host_fast(ei, n, alpha, w):
    """fast_appr_power's loop, restated to count its steps -> (pi, steps)."""
    r, c, ww = adjs()._with_self_loops(ei, w, n, torch.float32)
    A = sp.csr_matrix((ww.astype(np.float32), (r, c)), shape=(n, n))
    rs = np.asarray(A.sum(axis=1)).reshape(-1)
    k = rs.nonzero()[0]
    D_1 = sp.csr_matrix((1 / rs[k], (k, k)), shape=(n, n))
    s = 1 / (1 + alpha) / n * np.ones((n, 1))
    z_T = ((alpha * (1 + alpha)) * (rs != 0) + ((1 - alpha) / (1 + alpha) + alpha * (1 + alpha)) * (rs == 0))[np.newaxis, :]
    W = (1 - alpha) * A.T @ D_1
    x, oldx, it = s, np.zeros((n, 1)), 0
    while scipy.linalg.norm(x - oldx) > 1e-6:
        oldx = x
        x = W @ x + s @ (z_T @ x)
        it += 1
        if it >= 100:
            break
    return (x / sum(x)).reshape(-1), it


def row_major(index, value):
    """Entries sorted by (row, column): cal_fast_appr's host path emits scipy's unsorted order inside a row, the device
    path ascending columns."""
    index, value = torch.as_tensor(index), torch.as_tensor(value)
    order = torch.from_numpy(np.lexsort((index[1].numpy(), index[0].numpy())))
    return index[:, order], value[order]


def compare(got, want, rtol, sort_want=False):
    gi, gv = got
    wi, wv = row_major(*want) if sort_want else want
    assert gi.device.type == "cuda" and gv.dtype == torch.float32 and gi.dtype == torch.int64
    assert torch.equal(gi.cpu(), wi), "index differs from the host path"
    gv, wv = gv.cpu().double().numpy(), wv.double().numpy()
    err = np.abs(gv - wv) / np.maximum(np.abs(wv), 1e-30)
    assert err.max(initial=0) <= rtol, err.max()


def check_both(ei, n, w=None, alpha=0.1, appr_pi_tol=1e-9, fast_pi_tol=1e-6):
    """Device operators (and pi, steps) against the host path on CPU inputs."""
    from pytorch_geometric_signed_directed_amd.pagerank import appr_operator, fast_operator
    A = adjs()
    ei_d = ei.to(DEV)
    w_d = None if w is None else w.to(DEV)
    dense = A._perron_left_vector          # up to 2000 nodes the host path uses the float32 dense solver; the device
    A._perron_left_vector = lambda p, a, m: dense(p, a, m, dense_limit=0)   # path is its power iteration at every n
    try:
        want = A.get_appr_directed_adj(alpha, ei, n, torch.float32, w)
    finally:
        A._perron_left_vector = dense
    compare(A.get_appr_directed_adj(alpha, ei_d, n, torch.float32, w_d), want, 1e-6)
    compare(A.cal_fast_appr(alpha, ei_d, n, torch.float32, w_d), A.cal_fast_appr(alpha, ei, n, torch.float32, w), 1e-5,
            sort_want=True)
    _, _, pi, steps_a = appr_operator(ei_d, n, alpha, w_d)
    want = host_appr_pi(ei, n, alpha, w)
    assert np.abs(pi.cpu().numpy() - want).max() <= appr_pi_tol * np.abs(want).max()
    _, _, pi, steps = fast_operator(ei_d, n, alpha, w_d)
    want, want_steps = host_fast(ei, n, alpha, w)
    assert steps == want_steps
    assert np.abs(pi.cpu().numpy() - want).max() <= fast_pi_tol * np.abs(want).max()
    return steps_a


@pytest.mark.parametrize("name,alpha,weighted", [("appr", 0.1, True), ("appr_unw", 0.2, False), ("fast", 0.1, True)])
def test_cuda_matches_reference_fixtures(name, alpha, weighted):
    A = adjs()
    g = load_golden("adjs_digcn")
    ei, w = g.t("edge_index", DEV), (g.t("edge_weight", DEV) if weighted else None)
    fn = A.cal_fast_appr if name == "fast" else A.get_appr_directed_adj
    index, value = fn(alpha, ei, 40, torch.float32, w)
    assert index.device.type == "cuda" and value.device.type == "cuda"
    want_index, want_value = g[name + "_index"], g[name + "_value"]
    if name == "fast":
        want_index, want_value = (t.numpy() for t in row_major(want_index, want_value))
    assert np.array_equal(index.cpu().numpy(), want_index), name
    assert np.abs(value.cpu().numpy() - want_value).max() < 5e-6, name


@pytest.mark.parametrize("n,e", [(5_000, 60_000), (200_000, 4_000_000)])
@pytest.mark.parametrize("weighted", [False, True])
def test_dsbm_against_host_path_and_deterministic(n, e, weighted):
    from pytorch_geometric_signed_directed_amd.graphs import dsbm_for_edges
    from pytorch_geometric_signed_directed_amd.pagerank import appr_operator, fast_operator
    ei, _, _ = dsbm_for_edges(n, e, seed=5)
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64)
    w = (torch.from_numpy(np.random.default_rng(1).uniform(0.2, 2.0, ei.shape[1]).astype(np.float32))
         if weighted else None)
    check_both(ei, n, w)
    ei_d, w_d = ei.to(DEV), None if w is None else w.to(DEV)
    for op in (appr_operator, fast_operator):
        a, b = op(ei_d, n, 0.1, w_d), op(ei_d, n, 0.1, w_d)
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_hub_row_with_20k_in_neighbours():
    rng = np.random.default_rng(2)
    n = 30_000
    hub = np.stack([np.arange(1, 20_001), np.zeros(20_000, dtype=np.int64)])
    rest = rng.integers(0, n, size=(2, 60_000))
    ei = torch.from_numpy(np.concatenate([hub, rest], 1).astype(np.int64))
    w = torch.from_numpy(rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32))
    check_both(ei, n, w)
    check_both(ei.flip(0), n, w)                      # the hub as a row of P (out-degree 20k)


def test_duplicates_self_loops_and_zero_weights():
    ei = torch.tensor([[0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 2],
                       [1, 1, 2, 1, 3, 2, 0, 4, 0, 3, 3]])
    w = torch.tensor([0.5, 0.7, 1.0, 2.0, 0.0, 1.5, 1.0, 3.0, 0.25, 1.0, 0.0])
    check_both(ei, 6, w)
    check_both(ei, 6, None)


def test_isolated_nodes_empty_edge_set_and_single_node():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    check_both(ei, 9)                                 # nodes 3..8 only have their added self-loops
    check_both(torch.empty(2, 0, dtype=torch.int64), 7)
    check_both(torch.empty(2, 0, dtype=torch.int64), 1)
    check_both(torch.tensor([[0], [0]]), 1, torch.tensor([2.0]))


def test_directed_chain_runs_many_batches():
    """A 5k-node chain needs 181 augmented steps on the host path: the stopping flag is read over many batches."""
    n = 5_000
    ei = torch.stack([torch.arange(n - 1), torch.arange(1, n)])
    steps = check_both(ei, n)
    A = adjs()
    pt = ((1 - 0.1) * A._transition(ei, None, n, torch.float32)).T.tocsr()
    x, t, host_steps = np.full(n, 1.0 / (n + 1)), 1.0 / (n + 1), 0
    for _ in range(1000):                             # _perron_left_vector's loop, counted
        nx, nt = pt @ x + t / n, 0.1 * x.sum()
        s = nx.sum() + nt
        nx, nt = nx / s, nt / s
        host_steps += 1
        done = np.abs(nx - x).sum() + abs(nt - t) < 1e-12
        x, t = nx, nt
        if done:
            break
    assert host_steps == 181
    assert steps == host_steps


def test_negative_pi_raises_like_the_host():
    A = adjs()
    ei = torch.tensor([[0, 1, 2, 3, 0, 2], [1, 2, 3, 0, 2, 0]])
    w = torch.tensor([1.0, 1.0, -0.7, 1.0, 1.0, 1.0])          # pi = (0.51, 0.32, 1.05, -0.88)
    with pytest.raises(AssertionError):
        A.get_appr_directed_adj(0.1, ei, 4, torch.float32, w)
    with pytest.raises(AssertionError):
        A.get_appr_directed_adj(0.1, ei.to(DEV), 4, torch.float32, w.to(DEV))


def test_digcn_fed_device_operator_matches_host_operator():
    """DiGCN_node_classification on the device-built first-order operator equals the same model on the host-built one."""
    from pytorch_geometric_signed_directed_amd.graphs import dsbm_for_edges
    from pytorch_geometric_signed_directed_amd.nn import DiGCN_node_classification
    A = adjs()
    n = 3_000
    ei, _, _ = dsbm_for_edges(n, 30_000, seed=9)
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64)
    torch.manual_seed(0)
    x = torch.randn(n, 6)
    model = DiGCN_node_classification(6, 8, 3, 0.0).to(DEV).eval()
    host = A.get_appr_directed_adj(0.1, ei, n, torch.float32)
    dev = A.get_appr_directed_adj(0.1, ei.to(DEV), n, torch.float32)
    with torch.no_grad():
        want = model(x.to(DEV), host[0].to(DEV), host[1].to(DEV))
        got = model(x.to(DEV), dev[0], dev[1])
    close(got, want.cpu().numpy())
