"""GPU: the sparse Gram product (csrc/spgemm.hip) behind `directed_features_in_out` and the device path of
`get_second_directed_adj`, against the reference's fixtures, a float64 scipy restatement, and itself (determinism,
LDS tiers against the global path)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import operator_bars as B
from conftest import load_golden
from test_second_order import FEATURE_CASES, DEGREE_CASES, check_features, feature_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def restated(ei, size, w=None):
    """float64 scipy restatement: (A_in, A_out) as canonical CSR matrices."""
    ei = np.asarray(ei)
    a = sp.coo_matrix((np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64), (ei[0], ei[1])),
                      shape=(size, size)).tocsr()
    c, r = np.asarray(a.sum(0)).ravel(), np.asarray(a.sum(1)).ravel()
    c[c == 0] = 1
    r[r == 0] = 1
    out = []
    for m in (a.T @ sp.diags(1 / c) @ a, a @ sp.diags(1 / r) @ a.T):
        m = m.tocsr()
        m.sum_duplicates()
        m.eliminate_zeros()
        m.sort_indices()
        out.append(m)
    return out


def assert_matches(index, value, m, ref):
    """Structure equal to scipy's, and every element within its own bar of the float64 arbiter `ref`
    (tests/operator_bars.py): one float32 rounding of a float64 sum, plus the scales' float32 sums for the features."""
    coo = m.tocoo()
    assert np.array_equal(index.cpu().numpy(), np.stack([coo.row, coo.col])), "structure differs from scipy"
    B.check_elements("gram", index.cpu().numpy(), value.cpu().numpy(), ref)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_features_cuda_matches_reference(case):
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    g = load_golden("features_in_out")
    ei, size, w = feature_inputs(g, case, DEV)
    got = directed_features_in_out(ei, size, w)
    assert all(t.device.type == "cuda" for t in got)
    check_features(got, g, case)


def test_features_dsbm_against_scipy_and_deterministic():
    from pytorch_geometric_signed_directed_amd.graphs import dsbm_for_edges
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    ei, _, _ = dsbm_for_edges(50_000, 500_000, seed=3)
    rng = np.random.default_rng(0)
    w = rng.uniform(0.2, 2.0, ei.shape[1]).astype(np.float32)
    t_ei, t_w = torch.from_numpy(ei).to(DEV), torch.from_numpy(w).to(DEV)
    got = directed_features_in_out(t_ei, 50_000, t_w)
    a_in, a_out = restated(ei, 50_000, w)
    r_in, r_out = B.features_refs(ei, 50_000, w)
    assert_matches(got[1], got[2], a_in, r_in)
    assert_matches(got[3], got[4], a_out, r_out)
    assert same(got, directed_features_in_out(t_ei, 50_000, t_w))                   # bit-identical rerun
    assert same(got, directed_features_in_out(t_ei, 50_000, t_w, lds_limit=0))      # every row on the global path
    assert same(got, directed_features_in_out(t_ei, 50_000, t_w, lds_limit=1024))   # smallest tier + global


def in_products(ei, n):
    """Products of every row of A_in = A^T diag(s) A: sum over the in-edges (k, i) of rowlen(k)."""
    rowlen = np.bincount(ei[0], minlength=n)
    return np.bincount(ei[1], weights=rowlen[ei[0]], minlength=n).astype(np.int64)


def test_gram_hub_row_beyond_lds():
    """Node 0 has 20 000 in-neighbours, each with ~8 out-edges: its row of A_in = A^T diag(1/c) A has ~180 000 products,
    far above the largest LDS tier, so it takes the global path by default.  Checked through the Gram product alone
    (A_out of this graph would hold a dense 20 000 x 20 000 block); forcing every row to the global path, or no row
    beyond tier 0, gives the same bits."""
    from pytorch_geometric_signed_directed_amd.sparse_gram import coo_rows, from_coo, gram
    rng = np.random.default_rng(7)
    n = 30_000
    src = np.arange(1, 20_001)
    extra_src = rng.integers(1, n, 160_000)
    extra_dst = rng.integers(1, n, 160_000)
    ei = np.stack([np.concatenate([src, extra_src]), np.concatenate([np.zeros_like(src), extra_dst])]).astype(np.int64)
    w = rng.uniform(0.5, 2.0, ei.shape[1]).astype(np.float32)
    assert in_products(ei, n)[0] > 8192 * 8          # ~126 000 products
    t_ei = torch.from_numpy(ei).to(DEV)
    a, at = from_coo(t_ei[0].contiguous(), t_ei[1].contiguous(), torch.from_numpy(w).to(DEV), n, n)
    a_in, _ = restated(ei, n, w)
    c = np.asarray(sp.coo_matrix((w.astype(np.float64), (ei[0], ei[1])), shape=(n, n)).sum(0)).ravel()
    c[c == 0] = 1
    scale = torch.from_numpy(1.0 / c).to(DEV)
    got = gram(a, at, scale)
    assert_matches(coo_rows(got), got.val, a_in, B.gram_ref(ei[0], ei[1], w, n, n, 1.0 / c))
    for limit in (0, 1024, 4096, 1 << 30):
        other = gram(a, at, scale, lds_limit=limit)
        assert torch.equal(other.csr.rowptr, got.csr.rowptr) and torch.equal(other.csr.col, got.csr.col), limit
        assert torch.equal(other.val, got.val), limit


def tiered_graph():
    """500 sources with ~50 random out-edges each; node 0 gets 40 of them as in-neighbours, node 1 120 and node 2 300,
    so the A_in rows of nodes 0, 1, 2 have ~2 000, ~6 000 and ~15 000 products: one row for each workgroup LDS tier
    and one for the global path, beside thousands of tier-0 rows."""
    rng = np.random.default_rng(11)
    n = 5_000
    sources = np.arange(10, 510)
    src = np.repeat(sources, 50)
    dst = rng.integers(10, n, src.size)
    for node, k in ((0, 40), (1, 120), (2, 300)):
        pick = rng.choice(sources, k, replace=False)
        src, dst = np.concatenate([src, pick]), np.concatenate([dst, np.full(k, node)])
    ei = np.stack([src, dst]).astype(np.int64)
    return ei, rng.uniform(0.5, 2.0, ei.shape[1]).astype(np.float32), n


def test_features_every_lds_tier_and_global_path():
    """Rows in (1024, 4096] and (4096, 8192] run the workgroup-per-row tiers (bitonic sort across wavefronts); default,
    lds_limit = 0 / 1024 / 4096 / 8192 are bit-identical and match scipy."""
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    ei, w, n = tiered_graph()
    prods = in_products(ei, n)
    assert 1024 < prods[0] <= 4096 and 4096 < prods[1] <= 8192 and prods[2] > 8192, prods[:3]
    assert (prods <= 1024).sum() > 1000
    t_ei, t_w = torch.from_numpy(ei).to(DEV), torch.from_numpy(w).to(DEV)
    got = directed_features_in_out(t_ei, n, t_w)
    a_in, a_out = restated(ei, n, w)
    r_in, r_out = B.features_refs(ei, n, w)
    assert_matches(got[1], got[2], a_in, r_in)
    assert_matches(got[3], got[4], a_out, r_out)
    for limit in (0, 1024, 4096, 8192):
        assert same(got, directed_features_in_out(t_ei, n, t_w, lds_limit=limit)), limit


def test_second_directed_adj_every_lds_tier():
    from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj
    from pytorch_geometric_signed_directed_amd.utils.directed.get_adjs_DiGCN import _second_directed_adj_device
    ei, w, n = tiered_graph()
    want_i, want_v = get_second_directed_adj(torch.from_numpy(ei), n, torch.float32, torch.from_numpy(w))
    t_ei, t_w = torch.from_numpy(ei).to(DEV), torch.from_numpy(w).to(DEV)
    got_i, got_v = get_second_directed_adj(t_ei, n, torch.float32, t_w)
    assert torch.equal(got_i.cpu(), want_i)
    assert ((got_v.cpu() - want_v).abs() / (1 + want_v.abs())).max().item() <= 5e-6
    for limit in (0, 1024, 4096):
        forced = _second_directed_adj_device(t_ei, n, t_w, lds_limit=limit)
        assert torch.equal(forced[0], got_i) and torch.equal(forced[1], got_v), limit


def test_intersect_at_offsets_beyond_2_to_30():
    """The intersection's binary search at CSR offsets past 2^30, where a midpoint formed as lo + hi would wrap int32:
    one row of each operand placed at the end of shared 4.3 GB column / value buffers."""
    from pytorch_geometric_signed_directed_amd.sparse import CSR
    from pytorch_geometric_signed_directed_amd.sparse_gram import SparseValues, intersect
    rng = np.random.default_rng(5)
    k, width = 3000, 10_000
    x = (1 << 30) + (1 << 20)
    cols_a = np.sort(rng.choice(width, k, replace=False)).astype(np.int32)
    cols_b = np.sort(rng.choice(width, k, replace=False)).astype(np.int32)
    vals = rng.uniform(0.5, 2.0, 2 * k).astype(np.float32)
    col = torch.empty(x + 2 * k, dtype=torch.int32, device=DEV)
    val = torch.empty(x + 2 * k, dtype=torch.float32, device=DEV)
    col[x:] = torch.from_numpy(np.concatenate([cols_a, cols_b])).to(DEV)
    val[x:] = torch.from_numpy(vals).to(DEV)
    ptr_a = torch.tensor([x, x + k], dtype=torch.int32, device=DEV)
    ptr_b = torch.tensor([x + k, x + 2 * k], dtype=torch.int32, device=DEV)
    got = intersect(SparseValues(CSR(1, width, x + k, ptr_a, col, None), val),
                    SparseValues(CSR(1, width, x + 2 * k, ptr_b, col, None), val))
    both, ia, ib = np.intersect1d(cols_a, cols_b, return_indices=True)
    want = ((vals[ia].astype(np.float64) + vals[k + ib]) * 0.5).astype(np.float32)
    assert got.csr.rowptr.tolist() == [0, both.size] and both.size > 0
    assert np.array_equal(got.csr.col.cpu().numpy(), both)
    assert np.array_equal(got.val.cpu().numpy(), want)


def test_features_edge_cases():
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    out = directed_features_in_out(torch.empty(2, 0, dtype=torch.long, device=DEV), 7)
    assert [tuple(t.shape) for t in out] == [(2, 0), (2, 0), (0,), (2, 0), (0,)]
    assert all(t.device.type == "cuda" for t in out)
    # signed weights that cancel: A_in[2, 3] = A[0,2] A[0,3] + A[1,2] A[1,3] = 1 - 1 = 0 is absent
    ei = torch.tensor([[0, 0, 1, 1], [2, 3, 2, 3]], device=DEV)
    w = torch.tensor([1.0, 1.0, 1.0, -1.0], device=DEV)
    for e in (ei, ei.cpu()):
        _, e_in, w_in, _, _ = directed_features_in_out(e, 6, w.to(e.device))
        assert e_in.cpu().tolist() == [[2, 3], [2, 3]] and w_in.cpu().tolist() == [2.0, 2.0]
    # size beyond the largest id: isolated nodes, same entries as size = max + 1
    small = directed_features_in_out(ei, 4, w)
    big = directed_features_in_out(ei, 1000, w)
    assert same(small, big)


def test_features_feed_dgcn_like_reference_features():
    """DGCN_node_classification on device-built features equals the same model on the reference-built ones."""
    from pytorch_geometric_signed_directed_amd.nn import DGCN_node_classification
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    g = load_golden("features_in_out")
    ei, size, w = feature_inputs(g, "weighted", DEV)
    und, e_in, w_in, e_out, w_out = directed_features_in_out(ei, size, w)
    torch.manual_seed(0)
    model = DGCN_node_classification(6, 8, 3, 0.0).to(DEV).eval()
    x = torch.randn(size, 6, generator=torch.Generator().manual_seed(1)).to(DEV)
    got = model(x, und, e_in, e_out, w_in, w_out)
    ref = [g.t("weighted_" + k, DEV) for k in ("undirected", "in_index", "in_weight", "out_index", "out_weight")]
    want = model(x, ref[0], ref[1], ref[3], ref[2].float(), ref[4].float())
    err = ((got - want).abs() / (1 + want.abs())).max().item()
    assert err <= 1e-5, err


@pytest.mark.parametrize("case", DEGREE_CASES)
def test_in_out_degree_cuda_matches_reference(case):
    from pytorch_geometric_signed_directed_amd.utils import in_out_degree
    g = load_golden("in_out_degree")
    ei, size, w = feature_inputs(g, case, DEV)
    got = in_out_degree(ei, size, bool(g[case + "_signed"]), w)
    want = g[case + "_degree"]
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-5 * (1 + np.abs(want).max())


@pytest.mark.parametrize("name,weighted", [("second", True), ("second_unw", False)])
def test_second_directed_adj_cuda_matches_reference(name, weighted):
    from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj
    g = load_golden("adjs_digcn")
    ei = g.t("edge_index", DEV)
    w = g.t("edge_weight", DEV) if weighted else None
    index, value = get_second_directed_adj(ei, 40, torch.float32, w)
    assert index.device.type == "cuda" and index.dtype == torch.int64 and value.dtype == torch.float32
    assert np.array_equal(index.cpu().numpy(), g[name + "_index"])
    assert np.abs(value.cpu().numpy() - g[name + "_value"]).max() < 5e-6


def test_second_directed_adj_cuda_matches_host_path_mid_size():
    from pytorch_geometric_signed_directed_amd.graphs import dsbm_for_edges
    from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj
    from pytorch_geometric_signed_directed_amd.utils.directed.get_adjs_DiGCN import _second_directed_adj_device
    ei, _, _ = dsbm_for_edges(5_000, 40_000, seed=5)
    w = torch.from_numpy(np.random.default_rng(2).uniform(0.5, 2.0, ei.shape[1]).astype(np.float32))
    ei = torch.from_numpy(ei)
    for wt in (w, None):
        want_i, want_v = get_second_directed_adj(ei, 5_000, torch.float32, wt)
        got_i, got_v = get_second_directed_adj(ei.to(DEV), 5_000, torch.float32, None if wt is None else wt.to(DEV))
        assert torch.equal(got_i.cpu(), want_i)
        assert ((got_v.cpu() - want_v).abs() / (1 + want_v.abs())).max().item() <= 5e-6
        forced = _second_directed_adj_device(ei.to(DEV), 5_000, None if wt is None else wt.to(DEV), lds_limit=0)
        assert torch.equal(forced[0], got_i) and torch.equal(forced[1], got_v)


# ---- planted boundaries of the Gram product's tiers, hub batches and the int64 scan ----------------------------------
def squares(p):
    """p as a sum of squares (greedy): run lengths L_k with sum L_k^2 = p."""
    out = []
    while p:
        root = int(np.sqrt(p))
        out.append(root)
        p -= root * root
    return out


def gram_all_limits(b, bt, scale=None):
    """gram at lds_limit None, 0 and every tier cap: all bit-identical; returns the default."""
    from pytorch_geometric_signed_directed_amd.sparse_gram import _tier_caps, gram
    got = gram(b, bt, scale)
    for limit in [0] + _tier_caps():
        other = gram(b, bt, scale, lds_limit=limit)
        assert same((got.csr.rowptr, got.csr.col, got.val), (other.csr.rowptr, other.csr.col, other.val)), limit
    return got


@pytest.mark.parametrize("tier", [0, 1, 2])
def test_gram_rows_at_each_tier_edge(tier):
    """Rows of 1, cap - 1, cap and cap + 1 products for cap = pygsd_gram_tier_cap(tier): cap products fill the bitonic
    sort with no padding, cap + 1 is the next tier's (or the global path's) first row.
    - one run: every product in one column (L_k duplicates of (k, 0), sum L_k^2 = p), integer weights: exact;
    - distinct columns: one row of B with p entries, so C = b b^T and every element is one float32 rounding of an exact
      float64 product: bit-exact."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse_gram import coo_rows, from_coo
    cap = _cabi.lib().pygsd_gram_tier_cap(tier)
    rng = np.random.default_rng(tier)
    for p in (1, cap - 1, cap, cap + 1):
        runs = squares(p)
        r = np.repeat(np.arange(len(runs)), runs)
        c = np.zeros(r.size, np.int64)
        w = rng.integers(1, 4, r.size).astype(np.float32)
        t = [torch.from_numpy(x).to(DEV) for x in (r, c, w)]
        got = gram_all_limits(*from_coo(t[0], t[1], t[2], len(runs), 1))
        ref = B.gram_ref(r, c, w, len(runs), 1, exact=True)
        B.check_elements(f"one run p={p}", coo_rows(got).cpu().numpy(), got.val.cpu().numpy(), ref)
        assert got.csr.nnz == 1 and np.sum([x * x for x in runs]) == p
        b = torch.from_numpy(rng.uniform(0.5, 2.0, p).astype(np.float32)).to(DEV)
        cols = torch.arange(p, dtype=torch.int64, device=DEV)
        got = gram_all_limits(*from_coo(torch.zeros_like(cols), cols, b, 1, p))
        want = (b.double()[:, None] * b.double()[None, :]).float()
        assert torch.equal(got.csr.rowptr.long(), torch.arange(p + 1, device=DEV) * p), p
        assert torch.equal(got.csr.col.view(p, p).long(), cols.expand(p, p)), p
        assert torch.equal(got.val.view(p, p), want), p
        del got, want


def test_gram_hub_batches_bit_identical(monkeypatch):
    """The global path with HUB_BATCH_PRODUCTS = 3 000: several hubs share a batch (the batch-relative key h << 32 | j
    restarts at every batch), one hub (column 400, ~10 000 products) is larger than a batch, and one (column 401) cancels
    to no entry at all (rows 200 and 201 identical, their scales +1 and -1).  Integer weights, scales +-1 / powers of
    two: exact, so held bit-exactly to float64 and bit-identical to the default batching."""
    from pytorch_geometric_signed_directed_amd import sparse_gram
    from pytorch_geometric_signed_directed_amd.sparse_gram import coo_rows, from_coo, gram
    rng = np.random.default_rng(17)
    rows, cols = [], []
    for k in range(200):
        cs = rng.choice(400, 50, replace=False)
        rows += [k] * 51
        cols += list(cs) + [400]
    twin = list(402 + rng.choice(600, 599, replace=False)) + [401]
    rows += [200] * 600 + [201] * 600
    cols += twin + twin
    r, c = np.array(rows), np.array(cols)
    w = rng.integers(1, 4, r.size).astype(np.float32)
    w[r == 201] = w[r == 200]
    scale = 2.0 ** rng.integers(-2, 3, 202).astype(np.float64)
    scale[200], scale[201] = 1.0, -1.0
    t = [torch.from_numpy(x).to(DEV) for x in (r, c, w)]
    b, bt = from_coo(t[0], t[1], t[2], 202, 1002)
    s = torch.from_numpy(scale).to(DEV)
    want = gram(b, bt, s, lds_limit=1024)
    counts = np.bincount(c, weights=np.bincount(r)[r], minlength=1002)
    assert counts[400] > 3000 and counts[401] > 1024 and (counts[:400] > 1024).sum() > 100
    monkeypatch.setattr(sparse_gram, "HUB_BATCH_PRODUCTS", 3000)
    got = gram(b, bt, s, lds_limit=1024)
    assert same((got.csr.rowptr, got.csr.col, got.val), (want.csr.rowptr, want.csr.col, want.val))
    assert int(got.csr.rowptr[402] - got.csr.rowptr[401]) == 0
    ref = B.gram_ref(r, c, w, 202, 1002, scale, exact=True)
    B.check_elements("hub batches", coo_rows(got).cpu().numpy(), got.val.cpu().numpy(), ref)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4097, (1 << 20) + 5])
def test_scan_i64_against_cumsum(n):
    """pygsd_scan_i64 through sparse_gram._scan: exclusive scan with the total at [n], counts up to 2^40 so that the
    running sums pass 2^32 (the int64 claim), bit-exact against numpy."""
    from pytorch_geometric_signed_directed_amd.sparse_gram import _scan
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 1 << 40, n, dtype=np.int64)
    got = _scan(torch.from_numpy(counts).to(DEV)).cpu().numpy()
    want = np.concatenate([[0], np.cumsum(counts)])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if n > 256:
        assert want[-1] > (1 << 32)
