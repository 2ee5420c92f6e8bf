"""Host side of csrc/pagerank.hip (include/pygsd_hip.h): the first-order PageRank operators of DiGCN
(`get_appr_directed_adj`) and DiGCL (`cal_fast_appr`) built on the device.

Both start from A + I as two int32 CSRs (A and A^T, ascending columns in every row, duplicate edges adjacent), run a
float64 power iteration for the stationary vector pi, merge row i of P with row i of P^T into
L = (Pi^1/2 P Pi^-1/2 + Pi^-1/2 P^T Pi^1/2) / 2 and normalise it by its row sums.  `appr_operator` and `fast_operator`
return the operator together with pi and the number of power steps."""
import math
from typing import Optional, Tuple

import torch

from . import _cabi
from ._cabi import check, ptr, stream_ptr
from .sparse import CSR, csr_from_coo
from .sparse_build import sort_keys
from .sparse_gram import SparseValues, _scan, check_nnz, coo_rows

Tensor = torch.Tensor

BATCH = 8           # power steps enqueued between two reads of the stopping flag
WORK = 3 * 1024 + 2  # PYGSD_PAGERANK_WORK


def _loops_sorted(edge_index: Tensor, n: int, edge_weight: Optional[Tensor]):
    """(A, A^T) CSRs of A + I and their float64 weights in slot order: existing self-loops are kept and n more appended,
    entries sorted by (row, column) with a stable sort, so duplicate edges stay separate, adjacent slots."""
    dev = edge_index.device
    loops = torch.arange(n, dtype=torch.int64, device=dev)
    row = torch.cat([edge_index[0], loops]).contiguous()
    col = torch.cat([edge_index[1], loops]).contiguous()
    _cabi.check_node_ids((n, row), (n, col))
    w = (torch.ones(edge_index.size(1), dtype=torch.float64, device=dev) if edge_weight is None
         else edge_weight.detach().to(device=dev, dtype=torch.float64))
    w = torch.cat([w, torch.ones(n, dtype=torch.float64, device=dev)])
    bits = max(1, (n - 1).bit_length())
    _, perm = sort_keys((row << bits) | col, 2 * bits)
    perm = perm.long()
    row, col, w = row[perm], col[perm], w[perm]
    fwd = csr_from_coo(row, col, n, n, validate=False)
    bwd = csr_from_coo(col, row, n, n, validate=False)
    return fwd, w[fwd.perm.long()], bwd, w[bwd.perm.long()]


def _lanes(nnz: int, n: int) -> int:
    """Lanes per row of the step kernel: the power of two at or above the mean row length, at most a wavefront."""
    lanes = 1
    while lanes < 64 and lanes * n < nnz:
        lanes *= 2
    return lanes


def power_iteration(mt: CSR, val: Tensor, n: int, *, mode: int, alpha: float, x0: float, t0: float = 0.0,
                    c: float = 0.0, z: Optional[Tensor] = None, tol: float, max_steps: int) -> Tuple[Tensor, int]:
    """Runs pygsd_pagerank_step over M^T (`mt`, values `val`: float64 (1 - alpha) P^T in mode 0, float32 W in mode 1)
    from x = x0 (and t = t0) until its stopping rule holds.  Returns (x, completed steps); one status read per batch."""
    dev = val.device
    x = torch.full((n,), x0, dtype=torch.float64, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    work = torch.zeros(WORK, dtype=torch.float64, device=dev)
    work[WORK - 2] = t0
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    lib = _cabi.lib()
    v64, v32 = (val, None) if mode == 0 else (None, val)
    lanes = _lanes(mt.nnz, n)
    for _ in range(max_steps // BATCH + 2):      # the last step's rule is evaluated at the start of the next batch
        check(lib.pygsd_pagerank_step(mode, ptr(mt.rowptr), ptr(mt.col), ptr(v64), ptr(v32), ptr(z), n, lanes, alpha,
                                      c, tol, max_steps, BATCH, ptr(x), ptr(y), ptr(work), WORK, ptr(status),
                                      stream_ptr()), "pygsd_pagerank_step")
        done, steps = status.tolist()
        if done:
            return x, steps
    raise RuntimeError(f"pygsd_pagerank_step: no stop after {steps} steps (limit {max_steps})")


def _normalise(x: Tensor) -> Tensor:
    pi = torch.empty_like(x)
    work = torch.empty(WORK, dtype=torch.float64, device=x.device)
    check(_cabi.lib().pygsd_pagerank_normalise(ptr(x), x.numel(), ptr(work), WORK, ptr(pi), stream_ptr()),
          "pygsd_pagerank_normalise")
    return pi


def _symmetrise(fwd: CSR, fw: Tensor, bwd: CSR, bw: Tensor, sq: Tensor, isq: Tensor, n: int, fast: bool,
                inv: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Union merge of P and P^T rows, then D^-1/2 L D^-1/2 -> (int64 [2, nnz] row-major index, float32 values)."""
    lib = _cabi.lib()
    dev = fw.device
    f64, f32 = (ptr(fw), None) if not fast else (None, ptr(fw))
    t64, t32 = (ptr(bw), None) if not fast else (None, ptr(bw))
    args = (ptr(fwd.rowptr), ptr(fwd.col), f64, f32, ptr(bwd.rowptr), ptr(bwd.col), t64, t32, ptr(inv), ptr(sq),
            ptr(isq), n, int(fast))
    s = stream_ptr()
    count = torch.zeros(n, dtype=torch.int64, device=dev)
    check(lib.pygsd_pagerank_union_count(*args, ptr(count), s), "pygsd_pagerank_union_count")
    c_ptr = _scan(count)
    nnz = int(c_ptr[-1])
    check_nnz(nnz, "PageRank operator")
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float64, device=dev)
    check(lib.pygsd_pagerank_union_emit(*args, ptr(c_ptr), nnz, ptr(rowptr), ptr(col), ptr(val), s),
          "pygsd_pagerank_union_emit")
    out = torch.empty(nnz, dtype=torch.float32, device=dev)
    dis = torch.empty(n, dtype=torch.float64, device=dev)
    check(lib.pygsd_pagerank_scale(ptr(rowptr), ptr(col), ptr(val), n, int(fast), ptr(dis), ptr(out), s),
          "pygsd_pagerank_scale")
    m = SparseValues(CSR(n, n, nnz, rowptr, col, None), out)
    return coo_rows(m), out


def appr_operator(edge_index: Tensor, num_nodes: int, alpha: float, edge_weight: Optional[Tensor] = None):
    """DiGCN's approximate-PageRank Laplacian on the device (get_appr_directed_adj).  pi: the dominant left
    eigenvector of [[(1 - alpha) P, alpha 1], [1^T / n, 0]] restricted to the nodes and normalised to sum 1, by the
    host path's power iteration (stop when |dx|_1 + |dt| < 1e-12, at most 1000 steps).
    Returns (index, value, pi, steps); a negative component of pi raises AssertionError, as the host path does."""
    _cabi.require_gpu(edge_index)
    n = int(num_nodes)
    if n == 0:
        raise ZeroDivisionError("float division by zero")   # as the host path's 1 / n
    t0 = 1.0 / (n + 1)
    with _cabi.on_device(edge_index.device):
        fwd, fw, bwd, bw = _loops_sorted(edge_index, n, edge_weight)
        deg = torch.empty(n, dtype=torch.float64, device=fw.device)
        check(_cabi.lib().pygsd_pagerank_row_sum_f64(ptr(fwd.rowptr), ptr(fw), n, ptr(deg), stream_ptr()),
              "pygsd_pagerank_row_sum_f64")
        inv = torch.where(deg != 0, 1.0 / torch.where(deg != 0, deg, torch.ones_like(deg)), torch.zeros_like(deg))
        fw = inv[coo_rows(SparseValues(fwd, fw))[0]] * fw
        bw = inv[bwd.col.long()] * bw
        x, steps = power_iteration(bwd, (1 - alpha) * bw, n, mode=0, alpha=alpha, x0=t0, t0=t0, tol=1e-12,
                                   max_steps=1000)
        pi = _normalise(x)
        assert not bool((pi < 0).any())
        isq = pi.pow(-0.5)
        isq[torch.isinf(isq)] = 0
        index, value = _symmetrise(fwd, fw, bwd, bw, pi.sqrt(), isq, n, False)
    return index, value, pi, steps


def fast_operator(edge_index: Tensor, num_nodes: int, alpha: float, edge_weight: Optional[Tensor] = None):
    """DiGCL's PageRank Laplacian on the device (cal_fast_appr / fast_appr_power with tol 1e-6, at most 100 steps):
    x <- W x + s (z^T x) with W = (1 - alpha) A^T D^-1 in float32 entries, pi = x / sum(x).
    Returns (index, value, pi, steps)."""
    _cabi.require_gpu(edge_index)
    n = int(num_nodes)
    c = 1 / (1 + alpha) / n                              # n = 0 raises here, as on the host
    with _cabi.on_device(edge_index.device):
        fwd, fw, bwd, bw = _loops_sorted(edge_index, n, edge_weight)
        fw, bw = fw.float(), bw.float()
        inv = torch.empty(n, dtype=torch.float32, device=fw.device)
        z = torch.empty(n, dtype=torch.float64, device=fw.device)
        wt = torch.empty_like(bw)
        check(_cabi.lib().pygsd_pagerank_fast_prepare(ptr(fwd.rowptr), ptr(fwd.col), ptr(fw), ptr(bwd.rowptr),
                                                      ptr(bwd.col), ptr(bw), n, alpha, ptr(inv), ptr(z), ptr(wt),
                                                      stream_ptr()), "pygsd_pagerank_fast_prepare")
        if math.sqrt(n) * c > 1e-6:                      # the host tests |x0 - 0| > tol before its first step
            x, steps = power_iteration(bwd, wt, n, mode=1, alpha=alpha, x0=c, c=c, z=z, tol=1e-6, max_steps=100)
        else:
            x, steps = torch.full((n,), c, dtype=torch.float64, device=fw.device), 0
        pi = _normalise(x)
        index, value = _symmetrise(fwd, fw, bwd, bw, pi.pow(0.5), pi.pow(-0.5), n, True, inv)
    return index, value, pi, steps
