"""GPU: randomised differential checks of the device-built DGCN, DiGCN and DiGCL operators against float64.

Targets: the sparse Gram product (`gram`, rectangular B), the CSR intersection (`intersect`), DGCN's features
(`features`), `in_out_degree` (`degree`), DiGCN's second-order operator (`second`) and the PageRank operators (`appr`,
`fast`).  Each round draws a graph (empty, 1-3 nodes, an isolated tail, duplicate entries, self loops, one hub row and
one hub column) and weights (positive reals, none, small signed integers) from ONE seed; every failure names it:

        PYGSD_FUZZ_EXACT_SEED=<seed> python -m pytest tests/test_gpu_operator_fuzz.py -k <target>

The bars are per element and derived in tests/operator_bars.py, not tuned: u = 2^-24, sum|t| the sum of the magnitudes of
an element's terms, m their number.
- structure: bit-exact, except an element within its cancellation bound (m + 2) 2^-52 sum|t| of zero may be present or
  absent; integer weights with power-of-two or absent scales are exact on both sides and hold presence bit-exactly.
- gram: u |C| + (m + 2) 2^-52 sum|t|: one float32 rounding of a float64 sum.
- intersect: bit-exact ((a + b) * 0.5 in float64 of float32 inputs, rounded once).
- features: the gram bar plus sum |t_k| delta_k for the float32 team sums c_k, r_k behind the scales.
- degree: gamma_h sum|w| over the row for the team sum's tree height h; unit and integer weights bit-exact.
- second: the sum of the pipeline's roundings, element by element (operator_bars.second_ref), with magnitudes for
  signed weights, and the host path: same index but where an element may cancel, values within the existing 5e-6 bar
  or twice the derived one.  Rows whose d is undetermined are left out of the value checks and counted.
- appr: 4u of the host path (two float32 roundings of float64 values within 1e-9 of each other: 2 ulp of float32),
  pi within 1e-9 of its max; fast: 1e-5 of the host path, its float32 power iteration; both scaled by the row sums'
  cancellation kappa.  Signed weights (rows of zero degree, negative pi) hold refusal parity, step counts, pi and the
  rows holding NaN; their index and values are not compared (no structure bar is derived for the union merge).
- step counts equal the host's, except within 1e-9 relative of the tolerance at the deciding step (a near tie): there
  +-1 step is accepted and the device is held to the host run at the device's count.
Every target also asserts that a second call is bit-identical; gram and features across `lds_limit` too.
Skipped and counted, not loosened: draws whose real-valued signed sums are ill-conditioned, appr draws whose iteration
does not converge in 1000 steps (the device must not stop either), and fast draws whose host pi has a negative entry
(no stationary distribution: the iteration diverges on both paths; steps are still held)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import operator_bars as B
from test_gpu_fuzz import draw_graph, rounds

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
PRODUCT_BUDGET = int(os.environ.get("PYGSD_FUZZ_MAX_PRODUCTS", "3000000"))
STATS = {}


def record(target, worst_u=0.0, checks=1, skipped=0):
    st = STATS.setdefault(target, {"rounds": 0, "checks": 0, "worst_u": 0.0, "skipped": 0})
    st["rounds"] += 1 - skipped
    st["checks"] += checks
    st["worst_u"] = max(st["worst_u"], worst_u)
    st["skipped"] += skipped


def weights(rng, e):
    """(kind, float32 weights or None): positive reals, none (unit), or small signed integers."""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return "positive", (rng.random(e) + 0.25).astype(np.float32)
    if kind == 1:
        return "unit", None
    return "signed", rng.choice(np.array([-2, -1, 1, 2], dtype=np.float32), e)


def products(ei, n):
    """Products of A^T A and A A^T: the Gram products' work (and the float64 arbiter's)."""
    if ei.shape[1] == 0:
        return 0
    return int((np.bincount(ei[0], minlength=n).astype(np.int64) ** 2).sum() +
               (np.bincount(ei[1], minlength=n).astype(np.int64) ** 2).sum())


def draw(rng):
    """draw_graph, its edge list halved until the Gram products fit the budget (a hub of 30 000 entries would make a
    dense 30 000^2 block)."""
    n, ei = draw_graph(rng)
    ei = ei.numpy()
    while products(ei, n) > PRODUCT_BUDGET:
        ei = ei[:, :ei.shape[1] // 2]
    return n, ei


def bits(t):
    return {torch.float32: lambda: t.view(torch.int32), torch.float64: lambda: t.view(torch.int64)}.get(t.dtype, lambda: t)()


def bits_equal(a, b):
    """Bit-identical tensors (NaN included: a negative degree's d^-1/2 is NaN on the host path too)."""
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------- gram
def test_fuzz_gram_rectangular():
    from pytorch_geometric_signed_directed_amd.sparse_gram import coo_rows, from_coo, gram
    for seed, rng in rounds("operator_gram"):
        n, ei = draw(rng)
        n_rows, n_cols = n, int(rng.integers(1, B.LONG_ROW // 2 + 1)) if rng.random() < 0.5 else max(1, n // 3 + 1)
        if rng.random() < 0.5:
            n_rows, n_cols = n_cols, n_rows
        r, c = ei[0] % n_rows, ei[1] % n_cols
        while r.size and (np.bincount(r).astype(np.int64) ** 2).sum() > PRODUCT_BUDGET:
            r, c = r[:r.size // 2], c[:c.size // 2]
        kind, w = weights(rng, r.size)
        w = np.ones(r.size, np.float32) if w is None else w
        how = int(rng.integers(0, 3))
        scale = (None if how == 0 else rng.uniform(0.1, 10.0, n_rows) if how == 1
                 else 2.0 ** rng.integers(-4, 5, n_rows).astype(np.float64))
        limit = [None, 0, 1024, 4096, 8192, int(rng.integers(0, 9000))][int(rng.integers(0, 6))]
        what = f"seed={seed} n_rows={n_rows} n_cols={n_cols} e={r.size} {kind} scale={how} lds_limit={limit}"
        b, bt = from_coo(torch.from_numpy(r).to(D), torch.from_numpy(c).to(D), torch.from_numpy(w).to(D), n_rows, n_cols)
        s = None if scale is None else torch.from_numpy(scale).to(D)
        got = gram(b, bt, s, lds_limit=limit)
        assert got.csr.n_rows == n_cols and got.csr.rowptr.numel() == n_cols + 1, what
        again = gram(b, bt, s, lds_limit=limit)
        default = gram(b, bt, s)
        for other, name in ((again, "rerun"), (default, "default lds_limit")):
            assert bits_equal((got.csr.rowptr, got.csr.col, got.val), (other.csr.rowptr, other.csr.col, other.val)), \
                f"gram {what}: {name} not bit-identical"
        ref = B.gram_ref(r, c, w, n_rows, n_cols, scale, exact=kind != "positive" and how != 1)
        worst = B.check_elements(f"gram {what}", coo_rows(got).cpu().numpy(), got.val.cpu().numpy(), ref)
        record("gram", worst, 2)
    report("gram")


# ------------------------------------------------------------------------------------------------------------ intersect
def random_csr(rng, n, width):
    rows, cols = [], []
    for i in range(n):
        k = int(rng.integers(0, min(width, 200) + 1)) if rng.random() < 0.8 else 0
        rows.append(np.full(k, i))
        cols.append(np.sort(rng.choice(width, k, replace=False)))
    r, c = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    v = (rng.random(r.size) * 4 - 2).astype(np.float32)
    return sp.csr_matrix((v.astype(np.float64), (r, c)), shape=(n, width))


def test_fuzz_intersect():
    from pytorch_geometric_signed_directed_amd.sparse import CSR
    from pytorch_geometric_signed_directed_amd.sparse_gram import SparseValues, coo_rows, intersect

    def dev(m):
        m.sort_indices()
        return SparseValues(CSR(m.shape[0], m.shape[1], m.nnz, torch.from_numpy(m.indptr.astype(np.int32)).to(D),
                                torch.from_numpy(m.indices.astype(np.int32)).to(D), None),
                            torch.from_numpy(m.data.astype(np.float32)).to(D))

    for seed, rng in rounds("operator_intersect"):
        n, width = int(rng.integers(1, 400)), int(rng.integers(1, 3000))
        a, b = random_csr(rng, n, width), random_csr(rng, n, width)
        a, b = a.tolil(), b.tolil()
        for i in range(n):                           # rows b = -a, identical rows, rows with half their columns shared
            pick = rng.random()
            if pick < 0.15:
                b.rows[i], b.data[i] = list(a.rows[i]), [-x for x in a.data[i]]
            elif pick < 0.3:
                b.rows[i], b.data[i] = list(a.rows[i]), list(a.data[i])
            elif pick < 0.45 and len(a.rows[i]):
                keep = sorted(set(a.rows[i][::2]) | set(b.rows[i]))
                va = dict(zip(a.rows[i], a.data[i]))
                vb = dict(zip(b.rows[i], b.data[i]))
                b.rows[i] = keep
                b.data[i] = [(-va[j] if rng.random() < 0.5 else vb.get(j, 1.0)) if j in va else vb[j] for j in keep]
        a, b = a.tocsr(), b.tocsr()
        a.data, b.data = a.data.astype(np.float32).astype(np.float64), b.data.astype(np.float32).astype(np.float64)
        what = f"intersect seed={seed} n={n} width={width} nnz={a.nnz}/{b.nnz}"
        got = intersect(dev(a), dev(b))
        again = intersect(dev(a), dev(b))
        assert bits_equal((got.csr.rowptr, got.csr.col, got.val), (again.csr.rowptr, again.csr.col, again.val)), what
        want_i, want_v = B.intersect_ref(a, b)
        assert np.array_equal(coo_rows(got).cpu().numpy(), want_i), f"{what}: structure"
        assert np.array_equal(got.val.cpu().numpy().view(np.uint32), want_v.view(np.uint32)), f"{what}: values"
        record("intersect", 0.0, 2)
    report("intersect")


# ------------------------------------------------------------------------------------------------------------- features
def test_fuzz_features():
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    from pytorch_geometric_signed_directed_amd.utils.directed.features_in_out import _features_host
    for seed, rng in rounds("operator_features"):
        n, ei = draw(rng)
        kind, w = weights(rng, ei.shape[1])
        what = f"features seed={seed} n={n} e={ei.shape[1]} {kind}"
        if B.ill_conditioned_sums(ei, n, w):
            record("features", skipped=1, checks=0)
            continue
        t_ei = torch.from_numpy(ei).to(D)
        t_w = None if w is None else torch.from_numpy(w).to(D)
        got = directed_features_in_out(t_ei, n, t_w)
        limit = [0, 1024, 4096, int(rng.integers(0, 9000))][int(rng.integers(0, 4))]
        assert bits_equal(got, directed_features_in_out(t_ei, n, t_w)), f"{what}: rerun not bit-identical"
        assert bits_equal(got, directed_features_in_out(t_ei, n, t_w, lds_limit=limit)), f"{what}: lds_limit={limit}"
        if ei.shape[1] == 0:
            assert all(t.numel() == 0 for t in got), what
            record("features", 0.0, 1)
            continue
        host = _features_host(torch.from_numpy(ei), n, None if w is None else torch.from_numpy(w))
        assert torch.equal(got[0].cpu(), host[0]), f"{what}: undirected index"
        worst = 0.0
        for (idx, val), ref, name in zip(((got[1], got[2]), (got[3], got[4])), B.features_refs(ei, n, w), ("in", "out")):
            worst = max(worst, B.check_elements(f"{what} A_{name}", idx.cpu().numpy(), val.cpu().numpy(), ref))
        record("features", worst, 2)
    report("features")


# --------------------------------------------------------------------------------------------------------------- degree
def test_fuzz_degree():
    from pytorch_geometric_signed_directed_amd.utils import in_out_degree
    for seed, rng in rounds("operator_degree"):
        n, ei = draw_graph(rng)
        ei = ei.numpy()
        kind, w = weights(rng, ei.shape[1])
        if kind == "unit" and rng.random() < 0.5:
            w = rng.uniform(-3.0, 3.0, ei.shape[1]).astype(np.float32)      # real signed weights
            kind = "real signed"
        signed = w is not None and bool(rng.random() < 0.5)
        what = f"degree seed={seed} n={n} e={ei.shape[1]} {kind} signed={signed}"
        t_ei = torch.from_numpy(ei).to(D)
        t_w = None if w is None else torch.from_numpy(w).to(D)
        got = in_out_degree(t_ei, n, signed, t_w)
        assert torch.equal(got, in_out_degree(t_ei, n, signed, t_w)), f"{what}: rerun not bit-identical"
        want, bound = B.degree_ref(ei, n, w, signed)
        worst = B.check_degree(what, got.cpu().numpy(), want, bound)
        record("degree", worst, 1)
    report("degree")


# --------------------------------------------------------------------------------------------------------------- second
def test_fuzz_second():
    from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj
    from pytorch_geometric_signed_directed_amd.utils.directed.get_adjs_DiGCN import _second_directed_adj_device
    for seed, rng in rounds("operator_second"):
        n, ei = draw(rng)
        kind, w = weights(rng, ei.shape[1])
        what = f"second seed={seed} n={n} e={ei.shape[1]} {kind}"
        t_ei = torch.from_numpy(ei).to(D)
        t_w = None if w is None else torch.from_numpy(w).to(D)
        got_i, got_v = get_second_directed_adj(t_ei, n, torch.float32, t_w)
        again = _second_directed_adj_device(t_ei, n, t_w, lds_limit=int(rng.integers(0, 9000)))
        assert bits_equal((again[0], again[1]), (got_i, got_v)), f"{what}: rerun / lds_limit differ"
        ref, margin, undetermined = B.second_ref(ei, n, w)
        held = ~(undetermined[ref.row] | undetermined[ref.col])
        gi, gv = got_i.cpu().numpy(), got_v.cpu().numpy()
        worst = B.check_elements(what, gi, gv, ref, cancel_on=margin, held=held)
        want_i, want_v = get_second_directed_adj(torch.from_numpy(ei), n, torch.float32,
                                                 None if w is None else torch.from_numpy(w))
        check_against_host(what, gi, gv, want_i.numpy(), want_v.numpy(), ref, margin, held)
        record("second", worst, 3)
        st = STATS["second"]
        st["masked_rows"] = st.get("masked_rows", 0) + int(undetermined.sum())
        st["signed_rounds"] = st.get("signed_rounds", 0) + (kind == "signed")
    report("second")


def check_against_host(what, gi, gv, hi, hv, ref, margin, held):
    """The device against the host path (float64 throughout, rounded once to float32):
    - structure: equal, except elements whose L_in, L_out or sum is within its error bound of zero (margin <= 1);
    - values: the existing 5e-6 (1 + |host|) bar, or twice the element's derived bound where that is wider -- the host
      is within u |v| + 2^-30 |v| <= bound of float64 and the device within bound, so they are within 2 x bound of each
      other (signed weights, where d cancels in part);
    - NaN (d < 0) in the same places.  Rows whose d is undetermined (`held` False) are left out of values and NaN."""
    width = max(ref.n_cols, 1)
    ref_keys = ref.row * width + ref.col
    gk, hk = gi[0] * width + gi[1], hi[0] * width + hi[1]
    diff = np.setxor1d(gk, hk)
    if diff.size:
        pos = np.searchsorted(ref_keys, diff)
        ok = (pos < ref_keys.size) & (ref_keys[np.minimum(pos, ref_keys.size - 1)] == diff)
        assert ok.all() and (margin[pos] <= 1).all(), \
            f"{what}: {diff.size} entries differ from the host path, some where nothing may cancel"
    common, ig, ih = np.intersect1d(gk, hk, return_indices=True)
    pos = np.searchsorted(ref_keys, common)
    keep = held[pos]
    g, h, bound = gv[ig][keep].astype(np.float64), hv[ih][keep].astype(np.float64), ref.bound[pos][keep]
    assert np.array_equal(np.isnan(g), np.isnan(h)), f"{what}: NaN pattern differs from the host path"
    fin = ~np.isnan(h)
    bar = np.maximum(5e-6 * (1 + np.abs(h[fin])), 2 * bound[fin])
    err = np.abs(g[fin] - h[fin])
    assert (err <= bar).all(), f"{what}: {(err > bar).sum()} values beyond the host-path bar, worst {err.max():.3g}"


# ----------------------------------------------------------------------------------------------------- appr and fast
def host_appr(ei, n, alpha, w, steps=None):
    """_perron_left_vector's loop (dense_limit=0), counted: (pi normalised, steps, stopping norm of every step)."""
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    pt = ((1 - alpha) * A._transition(torch.from_numpy(ei), w, n, torch.float32)).T.tocsr()
    x, t, norms = np.full(n, 1.0 / (n + 1)), 1.0 / (n + 1), []
    for _ in range(1000 if steps is None else steps):
        nx, nt = pt @ x + t / n, alpha * x.sum()
        s = nx.sum() + nt
        nx, nt = nx / s, nt / s
        norms.append(np.abs(nx - x).sum() + abs(nt - t))
        x, t = nx, nt
        if steps is None and norms[-1] < 1e-12:
            break
    return x / x.sum(), len(norms), norms


def host_fast_counted(ei, n, alpha, w, steps=None):
    """fast_appr_power's loop (tol 1e-6, at most 100 steps) restated: (pi, steps, norms tested before each step)."""
    import scipy.linalg
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    r, c, ww = A._with_self_loops(torch.from_numpy(ei), w, n, torch.float32)
    M = sp.csr_matrix((ww.astype(np.float32), (r, c)), shape=(n, n))
    rs = np.asarray(M.sum(axis=1)).reshape(-1)
    k = rs.nonzero()[0]
    D_1 = sp.csr_matrix((1 / rs[k], (k, k)), shape=(n, n))
    s = 1 / (1 + alpha) / n * np.ones((n, 1))
    z_T = ((alpha * (1 + alpha)) * (rs != 0) + ((1 - alpha) / (1 + alpha) + alpha * (1 + alpha)) * (rs == 0))[np.newaxis, :]
    W = (1 - alpha) * M.T @ D_1
    x, oldx, it, norms = s, np.zeros((n, 1)), 0, []
    while True:
        norms.append(scipy.linalg.norm(x - oldx))
        if (steps is None and norms[-1] <= 1e-6) or it == steps:
            break
        oldx = x
        x = W @ x + s @ (z_T @ x)
        it += 1
        if steps is None and it >= 100:
            break
    return (x / sum(x)).reshape(-1), it, norms


def host_appr_operator(ei, n, alpha, w, pi):
    """get_appr_directed_adj's symmetrisation from a given pi: (index, float32 values, un-normalised L)."""
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    p = A._transition(torch.from_numpy(ei), w, n, torch.float32)
    with np.errstate(divide="ignore"):
        isq = np.power(pi, -0.5)
    isq[np.isinf(isq)] = 0
    half = sp.diags(np.power(pi, 0.5)) @ p @ sp.diags(isq)
    L = ((half + half.T) / 2.0).tocsr()
    index, value = A._sym_normalised(L, "cpu")
    return index.numpy(), value.numpy(), L


def host_fast_operator(ei, n, alpha, w, steps):
    """cal_fast_appr's host code with exactly `steps` power steps: (index row-major, float32 values, un-normalised L)."""
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    r, c, ww = A._with_self_loops(torch.from_numpy(ei), w, n, torch.float32)
    adj = sp.csr_matrix((ww.astype(np.float32), (r, c)), shape=(n, n))
    L, _ = A.fast_appr_power(adj, alpha=alpha, max_iter=max(steps, 1), tol=0.0)
    coo = L.tocoo()
    index = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
    values = torch.from_numpy(np.asarray(coo.data, dtype=np.float32))
    dis = torch.zeros(n, dtype=values.dtype).index_add_(0, index[0], values).pow(-0.5)
    dis[dis == float("inf")] = 0
    order = np.lexsort((coo.col, coo.row))
    return index.numpy()[:, order], (dis[index[0]] * values * dis[index[1]]).numpy()[order], L


def row_condition(L):
    """kappa_i = sum|L_i.| / |sum L_i.| (inf where the sum is 0 and the row is not empty)."""
    L = L.tocsr()
    s, a = np.asarray(L.sum(1)).ravel(), np.asarray(abs(L).sum(1)).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == 0, 1.0, a / np.abs(s))


def nan_rows(index, value, n):
    out = np.zeros(n, bool)
    out[np.asarray(index)[0][np.isnan(np.asarray(value))]] = True
    return out


def compare_operator(what, got, want_i, want_v, kappa, bar, signed):
    """The device operator (index, values) against the host's.  D^-1/2 L D^-1/2 divides by the row sums of L: a relative
    error e of L's entries becomes e kappa_i in d_i (kappa_i = sum|L_i.| / |sum L_i.|) and half of that in d_i^-1/2.
    kappa = 1 for non-negative weights, where the path's bar holds as it stands.  A row with kappa >= 0.5 / bar has d_i
    of undetermined sign at that bar: it is left out of the NaN comparison.
    Signed weights: L's entries can cancel in the union merge, for which no structure bar is derived -- only the rows
    holding NaN (d < 0) are compared; non-negative weights: index equal, values within bar (1 + (kappa_i + kappa_j) / 2)."""
    gi, gv = got[0].cpu().numpy(), got[1].cpu().double().numpy()
    n = kappa.size
    determined = kappa < 0.5 / bar
    assert np.array_equal(nan_rows(gi, gv, n)[determined], nan_rows(want_i, want_v, n)[determined]), \
        f"{what}: rows holding NaN differ from the host path"
    if signed:
        return 0.0
    assert np.array_equal(gi, want_i), f"{what}: index differs from the host path"
    wv = np.asarray(want_v, dtype=np.float64)
    nan = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nan), f"{what}: NaN pattern differs from the host path"
    err = np.abs(gv[~nan] - wv[~nan]) / np.maximum(np.abs(wv[~nan]), 1e-300)
    lim = bar * np.maximum(1.0, (kappa[gi[0][~nan]] + kappa[gi[1][~nan]]) / 2)
    assert (err <= lim).all(), f"{what}: values {err.max():.3g} from the host path"
    return float(err.max(initial=0))


def near_tie(norms, steps, tol):
    return any(abs(norms[i] - tol) <= 1e-9 * tol for i in range(max(0, steps - 2), min(len(norms), steps + 1)))


def test_fuzz_appr_and_fast():
    """Signed integer weights reach rows of zero degree (a -1 edge cancels the added loop) and negative pi (the host
    refuses appr with AssertionError: the device must too; fast's iteration then diverges on both paths).  Bars: appr
    values 4u of the host path (two float32 roundings of float64 values within 1e-9 of each other), pi within 1e-9 of
    its max; fast values 1e-5 (its float32 iteration), pi 1e-6.  Steps equal the host's but at a near tie, where the
    device is held to the host run at the device's step count."""
    from pytorch_geometric_signed_directed_amd.pagerank import appr_operator, fast_operator
    from pytorch_geometric_signed_directed_amd.utils.directed import get_adjs_DiGCN as A
    for seed, rng in rounds("operator_pagerank"):
        n, ei = draw_graph(rng)
        ei = ei.numpy()
        kind, w = weights(rng, ei.shape[1])
        if kind == "positive" and ei.shape[1] and rng.random() < 0.3:
            w[rng.random(w.size) < 0.2] = 0.0                           # zero weights beside the added loop
        signed = kind == "signed"
        alpha = float(rng.uniform(0.05, 0.5))
        what = f"pagerank seed={seed} n={n} e={ei.shape[1]} {kind} alpha={alpha:.4f}"
        t_ei = torch.from_numpy(ei).to(D)
        t_w = None if w is None else torch.from_numpy(w).to(D)
        c_w = None if w is None else torch.from_numpy(w)
        deg = np.bincount(ei[0], weights=np.ones(ei.shape[1]) if w is None else w, minlength=n) + 1
        STATS.setdefault("zero_degree_rows", {"rows": 0})["rows"] += int((deg == 0).sum())
        # appr: the host refuses a negative pi with AssertionError; the device must refuse it the same way
        dense = A._perron_left_vector      # the host path's power iteration at every n, as the device's
        A._perron_left_vector = lambda p, a, m: dense(p, a, m, dense_limit=0)
        try:
            A.get_appr_directed_adj(alpha, torch.from_numpy(ei), n, torch.float32, c_w)
            refused = False
        except AssertionError:
            refused = True
        finally:
            A._perron_left_vector = dense
        pi_h, steps_h, norms = host_appr(ei, n, alpha, c_w)
        if refused:
            with pytest.raises(AssertionError):
                appr_operator(t_ei, n, alpha, t_w)
            record("appr", 0.0, 1)
        else:
            got = appr_operator(t_ei, n, alpha, t_w)
            again = appr_operator(t_ei, n, alpha, t_w)
            assert bits_equal(got[:3], again[:3]) and got[3] == again[3], f"{what}: appr rerun not bit-identical"
            unconverged = not (norms and norms[-1] < 1e-12)
            if unconverged:
                # no convergence in 1000 steps (signed P: no stationary distribution, the host's pi may even be NaN):
                # the device must not stop either; pi and the operator are not compared
                assert got[3] == steps_h == 1000, f"{what}: appr stopped at {got[3]}, the host ran {steps_h} unconverged"
                record("appr", skipped=1, checks=2)
            else:
                if got[3] != steps_h:
                    assert abs(got[3] - steps_h) == 1 and near_tie(norms, steps_h, 1e-12), \
                        f"{what}: appr steps {got[3]} != host {steps_h}"
                    pi_h = host_appr(ei, n, alpha, c_w, got[3])[0]
                pi = got[2].cpu().numpy()
                assert np.abs(pi - pi_h).max(initial=0) <= 1e-9 * np.abs(pi_h).max(initial=0), f"{what}: appr pi"
                wi, wv, L = host_appr_operator(ei, n, alpha, c_w, pi_h)
                worst = compare_operator(f"{what} appr", got, wi, wv, row_condition(L), 4 * B.U, signed)
                record("appr", worst / B.U, 4)
        # fast
        got = fast_operator(t_ei, n, alpha, t_w)
        again = fast_operator(t_ei, n, alpha, t_w)
        assert bits_equal(got[:3], again[:3]) and got[3] == again[3], f"{what}: fast rerun not bit-identical"
        pi_h, steps_h, norms = host_fast_counted(ei, n, alpha, c_w)
        if got[3] != steps_h:
            assert abs(got[3] - steps_h) == 1 and near_tie(norms, steps_h, 1e-6), \
                f"{what}: fast steps {got[3]} != host {steps_h}"
            pi_h = host_fast_counted(ei, n, alpha, c_w, got[3])[0]
        if (pi_h < 0).any():   # no stationary distribution: the iteration diverges on both paths, steps held above
            record("fast", skipped=1, checks=2)
            continue
        pi = got[2].cpu().numpy()
        assert np.abs(pi - pi_h).max(initial=0) <= 1e-6 * np.abs(pi_h).max(initial=0), f"{what}: fast pi"
        if got[3] == steps_h:
            wi, wv = A.cal_fast_appr(alpha, torch.from_numpy(ei), n, torch.float32, c_w)
            order = np.lexsort((wi[1].numpy(), wi[0].numpy()))
            wi, wv = wi.numpy()[:, order], wv.numpy()[order]
        else:
            wi, wv, _ = host_fast_operator(ei, n, alpha, c_w, got[3])
        L = host_fast_operator(ei, n, alpha, c_w, got[3])[2]
        compare_operator(f"{what} fast", got, wi, wv, row_condition(L), 1e-5, signed)
        record("fast", 0.0, 4)
    report("appr")
    report("fast")
    report("zero_degree_rows")


def report(target):
    """The target's record on stdout (pytest -s): rounds, checks, worst error in units of u, skipped draws."""
    import json
    print(f"\noperator fuzz {target}:", json.dumps(STATS.get(target, {}), sort_keys=True))
