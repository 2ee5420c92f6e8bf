"""Generates tests/golden/features_in_out.npz and tests/golden/in_out_degree.npz from the reference's own, unmodified
`directed_features_in_out` and `in_out_degree` (imported over oracle/pyg_shim, as oracle/gen_golden.py does).  Needs
the reference checkout next to the build; the GPU box never runs it.

    python tools/gen_golden_second_order.py [reference root]

Every case is checked against an independent dense float64 restatement (<= 2e-6 * scale; with signed weights the scale
is that of the same sums over |terms|, since the reference divides by float32 degrees) before it is written:
    A_in = A^T diag(1/c) A, A_out = A diag(1/r) A^T  (c, r = column / row sums of the summed-duplicates A, 0 -> 1)
    in_out_degree: row / column sums of |w| (unsigned) or of (|A| +- A) / 2 (signed).
Fixtures are data only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "oracle", "pyg_shim"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_geometric_signed_directed.utils.directed.features_in_out import directed_features_in_out  # noqa: E402
from torch_geometric_signed_directed.utils.general.in_out_degree import in_out_degree  # noqa: E402

from oracle.gen_golden import toy_graph  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TOL = 2e-6


def dense(ei, w, n):
    a = np.zeros((n, n))
    np.add.at(a, (ei[0], ei[1]), np.ones(ei.shape[1]) if w is None else w.astype(np.float64))
    return a


def densify(index, value, n):
    m = np.zeros((n, n))
    np.add.at(m, (index[0], index[1]), value.astype(np.float64))
    return m


def check(name, got, want, terms=None):
    """terms: the same sum over |terms| -- the scale of the rounding when signed terms cancel."""
    scale = max(1.0, float(np.abs(want if terms is None else terms).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err <= TOL, f"{name}: reference differs from the float64 restatement by {err:.3e}"


def features_case(out, name, ei, w, size):
    res = directed_features_in_out(torch.from_numpy(ei), size, None if w is None else torch.from_numpy(w))
    und, e_in, w_in, e_out, w_out = [r.numpy() for r in res]
    a = dense(ei, w, size)
    c, r = a.sum(0), a.sum(1)
    c[c == 0] = 1
    r[r == 0] = 1
    b = np.abs(a)
    check(name + " A_in", densify(e_in, w_in, size), a.T @ np.diag(1 / c) @ a, b.T @ np.diag(1 / np.abs(c)) @ b)
    check(name + " A_out", densify(e_out, w_out, size), a @ np.diag(1 / r) @ a.T, b @ np.diag(1 / np.abs(r)) @ b.T)
    pairs = np.unique(np.concatenate([ei[0] * size + ei[1], ei[1] * size + ei[0]]))
    assert np.array_equal(und, np.stack([pairs // size, pairs % size])), name
    out.update({f"{name}_edge_index": ei, f"{name}_size": np.int64(size), f"{name}_undirected": und,
                f"{name}_in_index": e_in, f"{name}_in_weight": w_in, f"{name}_out_index": e_out,
                f"{name}_out_weight": w_out})
    if w is not None:
        out[f"{name}_edge_weight"] = w


def degree_case(out, name, ei, w, size, signed):
    got = np.asarray(in_out_degree(torch.from_numpy(ei), size, signed, None if w is None else torch.from_numpy(w)))
    a = dense(ei, w, size)
    if signed:
        pos, neg = (np.abs(a) + a) / 2, (np.abs(a) - a) / 2
        want = np.stack([pos.sum(1), neg.sum(1), pos.sum(0), neg.sum(0)], 1)
    else:
        a = dense(ei, None if w is None else np.abs(w), size)
        want = np.stack([a.sum(1), a.sum(0)], 1)
    check(name, got, want)
    out.update({f"{name}_edge_index": ei, f"{name}_size": np.int64(size), f"{name}_signed": np.bool_(signed),
                f"{name}_degree": got.astype(np.float32)})
    if w is not None:
        out[f"{name}_edge_weight"] = w


def main():
    os.makedirs(OUT, exist_ok=True)
    feats = {}
    ei, w = toy_graph(301)
    features_case(feats, "weighted", ei, w, 40)
    ei, _ = toy_graph(302, weighted=False)
    features_case(feats, "unweighted", ei, None, 40)
    ei, w = toy_graph(304, signed=True)   # seed 303 has a column sum that nearly cancels in the reference's float32
    features_case(feats, "signed", ei, w, 40)
    ei, w = toy_graph(305, n=30, e=90)
    features_case(feats, "padded", ei, w, 37)                 # size beyond the largest id
    np.savez_compressed(os.path.join(OUT, "features_in_out.npz"), **feats)

    degs = {}
    ei, w = toy_graph(311)
    degree_case(degs, "weighted", ei, w, 40, False)
    ei, _ = toy_graph(312, weighted=False)
    degree_case(degs, "unweighted", ei, None, 40, False)
    ei, w = toy_graph(313, signed=True)
    degree_case(degs, "signed_abs", ei, w, 40, False)
    degree_case(degs, "signed", ei, w, 40, True)
    # a signed duplicate pair that cancels: (3, 5) carries +1.5 and -1.5, so A[3, 5] = 0 after summing
    ei2 = np.concatenate([ei, np.array([[3, 3], [5, 5]])], 1)
    w2 = np.concatenate([w, np.array([1.5, -1.5], dtype=np.float32)])
    keep = ~((ei2[0] == 3) & (ei2[1] == 5))
    keep[-2:] = True
    degree_case(degs, "signed_cancel", ei2[:, keep], w2[keep], 40, True)
    np.savez_compressed(os.path.join(OUT, "in_out_degree.npz"), **degs)
    print("wrote features_in_out.npz (%d arrays), in_out_degree.npz (%d arrays)" % (len(feats), len(degs)))


if __name__ == "__main__":
    main()
