"""Times the second-order operator builds on the GPU: `directed_features_in_out` (DGCN's A_in / A_out) and the device path
of `get_second_directed_adj` (DiGCN's intersected P^T P / P P^T), on DSBM graphs, plus the host scipy path at 200k / 4M for
the ratio.  Device times are hipEvent pairs around whole calls after a warm-up call at the same size (median of
--repeats); host times a wall clock.  One JSON object to --out.  Off bench.py's timed path.

    python tools/bench_second_order.py --out profiles/second_order.json
    rocprofv3 --kernel-trace --stats -d <dir> -o k -- python tools/bench_second_order.py --sizes 1m --repeats 1 --no-host

Products = the multiply-adds of the Gram products (sum over k of rowlen(k)^2 for A^T A-shaped ones).
Every size is also checked: --check-rows random rows of each output (and, for DiGCN, the rows their normalisation reads)
are recomputed on the host with float64 scipy, independently of the device code; index equality and the largest
relative value error go into the JSON."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from pytorch_geometric_signed_directed_amd.graphs import dsbm_for_edges  # noqa: E402
from pytorch_geometric_signed_directed_amd.utils import directed_features_in_out  # noqa: E402
from pytorch_geometric_signed_directed_amd.utils.directed import get_second_directed_adj  # noqa: E402

SIZES = {"200k": (200_000, 4_000_000), "1m": (1_000_000, 20_000_000), "c5": (2_000_000, 52_000_000)}


def products(ei: torch.Tensor, n: int, loops: bool):
    """(products of the row-side Gram, products of the column-side Gram)."""
    extra = 1 if loops else 0
    out = []
    for side in (0, 1):
        d = torch.bincount(ei[side], minlength=n).double() + extra
        out.append(int((d * d).sum()))
    return out


def _rows_of(index, value, rows):
    """Entries of the given rows from a device [2, nnz] row-major index: (list of column arrays, list of value arrays)."""
    r = torch.from_numpy(rows).to(index.device)
    lo = torch.searchsorted(index[0], r).tolist()
    hi = torch.searchsorted(index[0], r + 1).tolist()
    return ([index[1, a:b].cpu().numpy() for a, b in zip(lo, hi)], [value[a:b].cpu().numpy() for a, b in zip(lo, hi)])


def _compare(index, value, want, rows):
    """want: scipy CSR whose row t is output row rows[t].  -> (structure equal, max |got - want| / (1 + |want|))."""
    cols, vals = _rows_of(index, value, rows)
    equal, err = True, 0.0
    for t in range(rows.size):
        w = want.getrow(t)
        w.sort_indices()
        equal &= bool(np.array_equal(cols[t], w.indices))
        if cols[t].size == w.indices.size and w.nnz:
            err = max(err, float((np.abs(vals[t].astype(np.float64) - w.data) / (1 + np.abs(w.data))).max()))
    return equal, err


def _canon(m):
    m = m.tocsr()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def check_features(ei, n, res, rows):
    a = sp.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n)).tocsr()
    c, r = np.asarray(a.sum(0)).ravel(), np.asarray(a.sum(1)).ravel()
    c[c == 0] = 1
    r[r == 0] = 1
    a_in = _canon(a.tocsc()[:, rows].T @ sp.diags(1 / c) @ a)
    a_out = _canon(a[rows] @ sp.diags(1 / r) @ a.T)
    eq_in, err_in = _compare(res[1], res[2], a_in, rows)
    eq_out, err_out = _compare(res[3], res[4], a_out, rows)
    return {"rows": int(rows.size), "index_equal": eq_in and eq_out, "max_rel_err": max(err_in, err_out)}


def check_second(ei, n, res, rows):
    loops = np.arange(n)
    rr, cc = np.concatenate([ei[0], loops]), np.concatenate([ei[1], loops])
    deg = np.bincount(rr, minlength=n).astype(np.float64)
    p = sp.csr_matrix((1.0 / deg[rr], (rr, cc)), shape=(n, n))
    pc = p.tocsc()

    def merged(sel):
        l_in, l_out = _canon(pc[:, sel].T @ p), _canon(p[sel] @ p.T)
        return _canon((l_in.multiply(l_out != 0) + l_out.multiply(l_in != 0)) / 2.0)

    m = merged(rows)
    need = np.unique(np.concatenate([rows, m.indices]))
    d = np.zeros(n)
    d[need] = np.asarray(merged(need).sum(1)).ravel()
    dis = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), 0.0)
    coo = m.tocoo()
    want = sp.csr_matrix((dis[rows[coo.row]] * coo.data * dis[coo.col], (coo.row, coo.col)), shape=m.shape)
    eq, err = _compare(res[0], res[1], want, rows)
    return {"rows": int(rows.size), "index_equal": eq, "max_rel_err": err}


def device_time(fn, repeats):
    fn()                                           # warm-up at the same size
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times, res = [], None
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), times, res, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200k,1m,c5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host scipy path at 200k")
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "cases": []}
    for key in args.sizes.split(","):
        n, e = SIZES[key]
        t0 = time.time()
        ei_np, _, _ = dsbm_for_edges(n, e, seed=11)
        ei = torch.from_numpy(ei_np)
        gen_s = time.time() - t0
        ei_d = ei.to(dev)
        torch.cuda.synchronize()
        case = {"size": key, "nodes": n, "edges": int(ei.shape[1]), "generate_s": round(gen_s, 1)}

        p_in, p_out = products(ei, n, loops=False)
        ms, all_ms, res, peak = device_time(lambda: directed_features_in_out(ei_d, n), args.repeats)
        case["features_in_out"] = {"products": p_in + p_out, "nnz_in": int(res[2].numel()), "nnz_out": int(res[4].numel()),
                                   "ms": ms, "ms_all": all_ms, "products_per_s": (p_in + p_out) / (ms * 1e-3),
                                   "peak_device_bytes": peak}
        rows = np.sort(np.random.default_rng(1).choice(n, args.check_rows, replace=False))
        case["features_in_out"]["check"] = check_features(ei_np, n, res, rows)
        del res
        q_in, q_out = products(ei, n, loops=True)
        ms, all_ms, res, peak = device_time(lambda: get_second_directed_adj(ei_d, n, torch.float32), args.repeats)
        case["second_directed_adj"] = {"products": q_in + q_out, "nnz": int(res[1].numel()), "ms": ms, "ms_all": all_ms,
                                       "products_per_s": (q_in + q_out) / (ms * 1e-3), "peak_device_bytes": peak}
        case["second_directed_adj"]["check"] = check_second(ei_np, n, res, rows)
        dev_second = res
        if key == "200k" and not args.no_host:
            t0 = time.time()
            host_feat = directed_features_in_out(ei, n)
            case["features_in_out"]["host_s"] = time.time() - t0
            t0 = time.time()
            host_second = get_second_directed_adj(ei, n, torch.float32)
            case["second_directed_adj"]["host_s"] = time.time() - t0
            for name in ("features_in_out", "second_directed_adj"):
                c = case[name]
                c["host_over_device"] = c["host_s"] / (c["ms"] * 1e-3)
            case["second_directed_adj"]["same_index_as_host"] = bool(torch.equal(dev_second[0].cpu(), host_second[0]))
            case["second_directed_adj"]["max_abs_diff_vs_host"] = float((dev_second[1].cpu() - host_second[1]).abs().max())
            case["features_in_out"]["same_index_as_host"] = bool(torch.equal(host_feat[1], directed_features_in_out(ei_d, n)[1].cpu()))
        del dev_second
        torch.cuda.empty_cache()
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
