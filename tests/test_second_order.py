"""CPU: DGCN's `directed_features_in_out` and the `in_out_degree` features against fixtures made by the reference's own
code (tools/gen_golden_second_order.py), and the int32 guard of the sparse Gram product."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

FEATURE_CASES = ("weighted", "unweighted", "signed", "padded")
DEGREE_CASES = ("weighted", "unweighted", "signed_abs", "signed", "signed_cancel")


def canonical(index, value):
    """Entries sorted row-major (the reference's unweighted edge_out has unsorted columns inside a row)."""
    index = np.asarray(index)
    order = np.lexsort((index[1], index[0]))
    return index[:, order], np.asarray(value)[order]


def is_canonical(index):
    index = np.asarray(index)
    keys = index[0].astype(np.int64) * (int(index.max(initial=0)) + 1) + index[1]
    return bool(np.all(np.diff(keys) > 0))


def check_features(got, g, case):
    und, e_in, w_in, e_out, w_out = [t.cpu() for t in got]
    assert und.dtype == e_in.dtype == e_out.dtype == torch.int64
    assert w_in.dtype == w_out.dtype == torch.float32
    assert np.array_equal(und.numpy(), g[case + "_undirected"]), case
    for idx, val, name in ((e_in, w_in, "in"), (e_out, w_out, "out")):
        assert is_canonical(idx.numpy()), (case, name)
        want_i, want_v = canonical(g[f"{case}_{name}_index"], g[f"{case}_{name}_weight"])
        assert np.array_equal(idx.numpy(), want_i), (case, name)
        err = np.abs(val.numpy().astype(np.float64) - want_v) / (1 + np.abs(want_v))
        assert err.max() <= 1e-5, (case, name, err.max())


def feature_inputs(g, case, device="cpu"):
    ei = g.t(case + "_edge_index", device)
    w = g.t(case + "_edge_weight", device)
    return ei, int(g[case + "_size"]), w


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_directed_features_in_out_cpu_matches_reference(case):
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out
    g = load_golden("features_in_out")
    ei, size, w = feature_inputs(g, case)
    check_features(directed_features_in_out(ei, size, w), g, case)


def test_directed_features_in_out_exports_and_empty_graph():
    from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out as a
    from pytorch_geometric_signed_directed_amd.utils.directed import directed_features_in_out as b
    assert a is b
    out = a(torch.empty(2, 0, dtype=torch.long), 5)
    assert [tuple(t.shape) for t in out] == [(2, 0), (2, 0), (0,), (2, 0), (0,)]


@pytest.mark.parametrize("case", DEGREE_CASES)
def test_in_out_degree_cpu_matches_reference(case):
    from pytorch_geometric_signed_directed_amd.utils import in_out_degree
    g = load_golden("in_out_degree")
    ei, size, w = feature_inputs(g, case)
    got = in_out_degree(ei, size, bool(g[case + "_signed"]), w)
    want = g[case + "_degree"]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.abs(got.numpy() - want).max() <= 1e-5 * (1 + np.abs(want).max())


def test_in_out_degree_signed_needs_weights():
    from pytorch_geometric_signed_directed_amd.utils import in_out_degree
    with pytest.raises(ValueError):
        in_out_degree(torch.tensor([[0, 1], [1, 0]]), 2, signed=True)


def test_signed_cancelling_pair_is_in_fixture():
    g = load_golden("in_out_degree")
    ei, w = g["signed_cancel_edge_index"], g["signed_cancel_edge_weight"]
    pair = (ei[0] == 3) & (ei[1] == 5)
    assert pair.sum() == 2 and w[pair].sum() == 0


def test_gram_emit_refuses_an_nnz_beyond_int32():
    """The int32 guard: a synthetic count of 2^31 entries is refused with a message naming the limit, before any pointer
    is touched (nothing is allocated)."""
    import threading
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse_gram import check_nnz
    lib = _cabi.lib()
    failures = []

    def calls():   # on a thread of its own: the error string is thread-local, this thread's stays ""
        try:
            guarded(lib)
        except AssertionError as exc:
            failures.append(exc)

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert not failures, failures
    with pytest.raises(RuntimeError, match="2\\^31 - 1"):
        check_nnz((1 << 31))
    check_nnz((1 << 31) - 1)


def guarded(lib):
    rc = lib.pygsd_gram_emit(None, None, None, None, 1, 1 << 31, None, None, None, None)
    assert rc != 0 and b"2^31 - 1" in lib.pygsd_last_error()
    rc = lib.pygsd_csr_intersect_emit(None, None, None, None, None, None, 1, None, 1 << 31, None, None, None, None)
    assert rc != 0 and b"2^31 - 1" in lib.pygsd_last_error()
    need = ctypes.c_size_t(0)
    assert lib.pygsd_gram_hub_workspace(1 << 31, ctypes.byref(need)) != 0
    assert [lib.pygsd_gram_tier_cap(t) for t in range(3)] == [1024, 4096, 8192]
