"""CPU: the float64 arbiters and element checks of tests/test_gpu_operator_fuzz.py (tests/operator_bars.py).  Each
arbiter reproduces the reference's fixtures, so a wrong arbiter cannot let the GPU tests pass unchecked; each check
accepts the host path's own output and rejects mutated copies of it (a value moved past its bar, an entry dropped, two
entries of a row swapped, the scale of node k replaced by that of node k + 1)."""
import numpy as np
import pytest
import torch

import operator_bars as B
from conftest import load_golden
from test_second_order import DEGREE_CASES, FEATURE_CASES, canonical


def feature_case(case):
    g = load_golden("features_in_out")
    return g, g[case + "_edge_index"], int(g[case + "_size"]), g.get(case + "_edge_weight")


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_features_arbiter_reproduces_fixtures(case):
    g, ei, size, w = feature_case(case)
    for ref, name in zip(B.features_refs(ei, size, w), ("in", "out")):
        want_i, want_v = canonical(g[f"{case}_{name}_index"], g[f"{case}_{name}_weight"])
        keep = ref.val != 0
        assert np.array_equal(np.stack([ref.row[keep], ref.col[keep]]), want_i), (case, name)
        assert np.all(np.abs(ref.val[keep] - want_v) <= 1e-5 * np.abs(want_v)), (case, name)


@pytest.mark.parametrize("case", DEGREE_CASES)
def test_degree_arbiter_reproduces_fixtures(case):
    g = load_golden("in_out_degree")
    want, bound = B.degree_ref(g[case + "_edge_index"], int(g[case + "_size"]), g.get(case + "_edge_weight"),
                               bool(g[case + "_signed"]))
    assert want.shape == g[case + "_degree"].shape
    assert np.all(np.abs(want - g[case + "_degree"]) <= 1e-6 * np.abs(g[case + "_degree"]) + 1e-12), case
    assert np.all(bound >= 0)


@pytest.mark.parametrize("name,weighted", [("second", True), ("second_unw", False)])
def test_second_arbiter_reproduces_fixtures(name, weighted):
    g = load_golden("adjs_digcn")
    ref, margin, _ = B.second_ref(g["edge_index"], 40, g["edge_weight"] if weighted else None)
    keep = ref.val != 0
    assert np.array_equal(np.stack([ref.row[keep], ref.col[keep]]), g[name + "_index"]), name
    assert np.all(np.abs(ref.val[keep] - g[name + "_value"]) <= 1e-5 * np.abs(g[name + "_value"])), name
    assert np.all(margin[keep] > 1)                      # positive weights: nothing may cancel
    bar = ref.bound[keep] / np.abs(ref.val[keep]) / B.U
    assert 10 < bar.min() and bar.max() < 60, (bar.min(), bar.max())   # the budget of second_ref's docstring


def test_intersect_arbiter_against_a_hand_built_row():
    import scipy.sparse as sp
    a = sp.csr_matrix((np.array([1.0, 2.0, 3.0, 0.5]), ([0, 0, 0, 1], [1, 4, 7, 2])), shape=(3, 9))
    b = sp.csr_matrix((np.array([-1.0, 1.0, 0.25, 9.0]), ([0, 0, 0, 2], [1, 4, 8, 2])), shape=(3, 9))
    index, value = B.intersect_ref(a, b)
    assert index.tolist() == [[0], [4]] and value.tolist() == [1.5]   # (1 - 1) cancels, 7 / 8 / row 1 / row 2 unmatched


# ---------------------------------------------------------------------------------------------------------- mutations
def host_features(case):
    from pytorch_geometric_signed_directed_amd.utils.directed.features_in_out import _features_host
    g, ei, size, w = feature_case(case)
    return ei, size, w, _features_host(torch.from_numpy(ei), size, None if w is None else torch.from_numpy(w))


def mutants(index, value, ref, rng):
    """(name, index, value) copies of a correct output, each one defect away from it."""
    index, value = np.array(index), np.array(value, dtype=np.float64)
    width = max(ref.n_cols, 1)
    pos = np.searchsorted(ref.row * width + ref.col, index[0] * width + index[1])
    k = int(rng.integers(0, value.size))
    bar = ref.bound[pos[k]]
    v = value.copy()
    v[k] = ref.val[pos[k]] + np.sign(ref.val[pos[k]]) * 2 * bar              # twice its own bar away from float64
    yield "value past its bar", index, v
    keep = np.ones(value.size, bool)
    keep[k] = False
    yield "entry dropped", index[:, keep], value[keep]
    rows = index[0]
    multi = np.flatnonzero((rows[1:] == rows[:-1]) & (value[1:] != value[:-1]))
    if multi.size:
        j = int(multi[0])
        v = value.copy()
        v[j], v[j + 1] = v[j + 1], v[j]
        yield "two entries of a row swapped", index, v


def test_gram_check_rejects_one_u_beyond_its_bar():
    """The gram bar is one rounding: a value scaled by 1 + 4u (4 x the bar) is refused; the float32 rounding passes."""
    rng = np.random.default_rng(3)
    r, c = rng.integers(0, 30, 300), rng.integers(0, 20, 300)
    w = rng.uniform(0.5, 2.0, 300).astype(np.float32)
    ref = B.gram_ref(r, c, w, 30, 20)
    index, value = np.stack([ref.row, ref.col]), ref.val.astype(np.float32)
    assert B.check_elements("rounded", index, value, ref) <= 1.0
    k = int(np.argmax(np.abs(ref.val)))
    v = ref.val.copy()
    v[k] *= 1 + 4 * B.U
    with pytest.raises(AssertionError, match="beyond the bar"):
        B.check_elements("1 + 4u", index, v, ref)


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_features_check_accepts_host_and_rejects_mutants(case):
    ei, size, w, host = host_features(case)
    rng = np.random.default_rng(len(case))
    refs = B.features_refs(ei, size, w)
    for (idx, val), ref in zip(((host[1], host[2]), (host[3], host[4])), refs):
        B.check_elements(case, idx.numpy(), val.numpy(), ref)
        for name, i2, v2 in mutants(idx.numpy(), val.numpy(), ref, rng):
            with pytest.raises(AssertionError):
                B.check_elements(f"{case} {name}", i2, v2, ref)
    # the scale of node k read from node k + 1: A_in built with c[k + 1] in place of c[k]
    ww = np.ones(ei.shape[1]) if w is None else np.asarray(w, np.float64)
    import scipy.sparse as sp
    a = sp.coo_matrix((ww, (ei[0], ei[1])), shape=(size, size)).tocsr()
    c = np.asarray(a.sum(0)).ravel()
    c[c == 0] = 1
    k = int(np.flatnonzero(np.diff(c) != 0)[0])
    c[k] = c[k + 1]
    wrong = (a.T @ sp.diags(1 / c) @ a).tocsr()
    wrong.sort_indices()
    coo = wrong.tocoo()
    with pytest.raises(AssertionError):
        B.check_elements(f"{case} shifted scale", np.stack([coo.row, coo.col]), coo.data.astype(np.float32), refs[0])


@pytest.mark.parametrize("name,weighted", [("second", True), ("second_unw", False)])
def test_second_check_accepts_host_and_rejects_mutants(name, weighted):
    from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj
    g = load_golden("adjs_digcn")
    w = g["edge_weight"] if weighted else None
    index, value = get_second_directed_adj(torch.from_numpy(g["edge_index"]), 40, torch.float32,
                                           None if w is None else torch.from_numpy(w))
    ref, margin, _ = B.second_ref(g["edge_index"], 40, w)
    B.check_elements(name, index.numpy(), value.numpy(), ref, cancel_on=margin)
    rng = np.random.default_rng(5)
    for what, i2, v2 in mutants(index.numpy(), value.numpy(), ref, rng):
        with pytest.raises(AssertionError):
            B.check_elements(f"{name} {what}", i2, v2, ref, cancel_on=margin)
    k = int(np.argmax(np.abs(ref.val)))
    v = value.numpy().astype(np.float64)
    v[k] *= 1 + 64 * B.U                                  # past the ~25-30u budget
    with pytest.raises(AssertionError, match="beyond the bar"):
        B.check_elements(f"{name} 1 + 64u", index.numpy(), v, ref, cancel_on=margin)


@pytest.mark.parametrize("case", DEGREE_CASES)
def test_degree_check_accepts_host_and_rejects_mutants(case):
    from pytorch_geometric_signed_directed_amd.utils import in_out_degree
    g = load_golden("in_out_degree")
    ei, size, w, signed = g[case + "_edge_index"], int(g[case + "_size"]), g.get(case + "_edge_weight"), bool(
        g[case + "_signed"])
    want, bound = B.degree_ref(ei, size, w, signed)
    host = in_out_degree(torch.from_numpy(ei), size, signed, None if w is None else torch.from_numpy(w)).numpy()
    B.check_degree(case, host, want, bound)
    k = int(np.argmax(np.abs(want)))
    bad = host.astype(np.float64).copy()
    bad.flat[k] = want.flat[k] * (1 + 4 * B.U) + 2 * bound.flat[k]
    with pytest.raises(AssertionError):
        B.check_degree(f"{case} past its bar", bad, want, bound)
    node = k // want.shape[1]
    shifted = host.copy()
    shifted[node] = host[(node + 1) % size]              # node k's degrees read from node k + 1
    if not np.array_equal(shifted, host):
        with pytest.raises(AssertionError):
            B.check_degree(f"{case} shifted", shifted, want, bound)
