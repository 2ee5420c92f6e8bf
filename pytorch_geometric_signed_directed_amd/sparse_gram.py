"""Host side of the sparse Gram product C = B^T diag(s) B and the CSR intersection merge (csrc/spgemm.hip,
include/pygsd_hip.h): the second-order proximity operators of DGCN and DiGCN.

`gram` runs the pipeline: count the products of every output row, bin the rows by that count (three LDS tiers, one
block per row; longer rows -- hubs -- take the global-memory path in batches), scan the exact row lengths and pack the
int32 CSR.  Two device->host reads per call: the product total and the nnz.  Every path sums a column's products in the
same order, so the result does not depend on the binning (`lds_limit`)."""
import ctypes
from typing import Optional, Tuple

import torch

from . import _cabi
from ._cabi import check, ptr, stream_ptr
from .sparse import CSR

Tensor = torch.Tensor

INT32_MAX = (1 << 31) - 1
HUB_BATCH_PRODUCTS = 1 << 26  # products of one hub batch (the global path's workspace is ~48 bytes per product)


def _tier_caps():
    lib = _cabi.lib()
    return [lib.pygsd_gram_tier_cap(t) for t in range(3)]


def check_nnz(nnz: int, what: str = "sparse Gram product"):
    """An int32 CSR holds at most 2^31 - 1 entries; refuse larger outputs before allocating them."""
    if nnz > INT32_MAX:
        raise RuntimeError(f"{what}: {nnz} entries; an int32 CSR holds at most 2^31 - 1 = {INT32_MAX}")


def _scan(counts: Tensor) -> Tensor:
    """int64 exclusive scan with the total at [n] (pygsd_scan_i64)."""
    n = counts.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=counts.device)
    lib = _cabi.lib()
    need = ctypes.c_size_t(0)
    check(lib.pygsd_scan_i64_workspace(n, ctypes.byref(need)), "pygsd_scan_i64_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=counts.device)
    check(lib.pygsd_scan_i64(ptr(counts), n, ptr(out), ptr(ws), need.value, stream_ptr()), "pygsd_scan_i64")
    return out


class SparseValues:
    """A CSR (sparse.CSR: int32 rowptr / col, perm unused) with float32 values in slot order."""
    __slots__ = ("csr", "val")

    def __init__(self, csr: CSR, val: Tensor):
        self.csr, self.val = csr, val


def gram(b: SparseValues, bt: SparseValues, scale: Optional[Tensor] = None, *, lds_limit: Optional[int] = None) -> SparseValues:
    """C = B^T diag(scale) B as an int32 CSR of shape [B.n_cols, B.n_cols] with ascending columns, float32 values rounded
    once from a float64 sum; exact-zero sums are dropped.

    b, bt: B and B^T over the same entries (bt row i lists the (k, B[k, i])), duplicates allowed (they add).
    scale: float64 [B.n_rows] or None (ones).
    lds_limit: rows with more products than this take the global-memory (hub) path; the rest are held in LDS.
    Default (None): the largest LDS tier.  0 sends every row to the global path."""
    _cabi.require_gpu(b.val, bt.val)
    dev = b.val.device
    n_out, n_k = b.csr.n_cols, b.csr.n_rows
    if bt.csr.n_rows != n_out or bt.csr.n_cols != n_k or bt.csr.nnz != b.csr.nnz:
        raise ValueError("gram: `bt` must be the transpose of `b`")
    if scale is not None:
        if scale.dtype != torch.float64 or scale.numel() != n_k:
            raise ValueError(f"gram: scale must be float64 [{n_k}]")
        scale = scale.contiguous()
    caps = _tier_caps()
    limit = caps[-1] if lds_limit is None else max(0, min(int(lds_limit), caps[-1]))
    if b.csr.nnz == 0:   # no products (and no column buffer for pygsd_gram_count to read): C is empty
        return SparseValues(CSR(n_out, n_out, 0, torch.zeros(n_out + 1, dtype=torch.int32, device=dev),
                                torch.empty(0, dtype=torch.int32, device=dev), None),
                            torch.empty(0, dtype=torch.float32, device=dev))
    lib = _cabi.lib()
    with _cabi.on_device(dev):
        s = stream_ptr()
        bv, tv = b.val.contiguous(), bt.val.contiguous()
        count = torch.zeros(n_out, dtype=torch.int64, device=dev)
        check(lib.pygsd_gram_count(ptr(bt.csr.rowptr), ptr(bt.csr.col), ptr(b.csr.rowptr), n_out, ptr(count), s),
              "pygsd_gram_count")
        prod_ptr = _scan(count)
        n_prod = int(prod_ptr[-1])
        rowptr = torch.zeros(n_out + 1, dtype=torch.int32, device=dev)
        if n_prod == 0:
            return SparseValues(CSR(n_out, n_out, 0, rowptr, torch.empty(0, dtype=torch.int32, device=dev), None),
                                torch.empty(0, dtype=torch.float32, device=dev))
        tmp_col = torch.empty(n_prod, dtype=torch.int32, device=dev)
        tmp_val = torch.empty(n_prod, dtype=torch.float32, device=dev)
        row_nnz = torch.zeros(n_out, dtype=torch.int64, device=dev)
        args = (ptr(b.csr.rowptr), ptr(b.csr.col), ptr(bv), ptr(bt.csr.rowptr), ptr(bt.csr.col), ptr(tv), ptr(scale))
        lo = 0
        for tier, cap in enumerate(caps):
            hi = min(cap, limit)
            if hi <= lo:
                continue
            rows = torch.nonzero((count > lo) & (count <= hi)).flatten().to(torch.int32)
            if rows.numel():
                check(lib.pygsd_gram_rows(*args, ptr(rows), rows.numel(), tier, ptr(prod_ptr), ptr(tmp_col),
                                          ptr(tmp_val), ptr(row_nnz), s), "pygsd_gram_rows")
            lo = hi
        hubs = torch.nonzero(count > limit).flatten()
        if hubs.numel():
            _hub_rows(lib, args, hubs, count, prod_ptr, tmp_col, tmp_val, row_nnz, s)
        c_ptr = _scan(row_nnz)
        nnz, worst = torch.stack([c_ptr[-1], row_nnz.min()]).tolist()    # one read for both
        if worst < 0:   # pygsd_gram_rows marks a row listed above its tier's cap with -1 instead of computing it
            raise RuntimeError("sparse Gram product: a row was binned above its LDS tier's capacity")
        check_nnz(nnz)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        val = torch.empty(nnz, dtype=torch.float32, device=dev)
        check(lib.pygsd_gram_emit(ptr(prod_ptr), ptr(tmp_col), ptr(tmp_val), ptr(c_ptr), n_out, nnz, ptr(rowptr),
                                  ptr(col), ptr(val), s), "pygsd_gram_emit")
    return SparseValues(CSR(n_out, n_out, nnz, rowptr, col, None), val)


def _hub_rows(lib, args, hubs, count, prod_ptr, tmp_col, tmp_val, row_nnz, s):
    """The global path, in batches of consecutive hub rows of at most HUB_BATCH_PRODUCTS products (a longer row is a
    batch of its own; beyond 2^31 - 1 products the C entry refuses it)."""
    counts = count[hubs].tolist()
    start = 0
    while start < len(counts):
        end, total = start + 1, counts[start]
        while end < len(counts) and total + counts[end] <= HUB_BATCH_PRODUCTS:
            total += counts[end]
            end += 1
        rows = hubs[start:end].to(torch.int32)
        off = torch.zeros(end - start + 1, dtype=torch.int64, device=hubs.device)
        off[1:] = torch.cumsum(count[hubs[start:end]], 0)
        need = ctypes.c_size_t(0)
        check(lib.pygsd_gram_hub_workspace(total, ctypes.byref(need)), "pygsd_gram_hub_workspace")
        ws = torch.empty(need.value, dtype=torch.uint8, device=hubs.device)
        check(lib.pygsd_gram_hub(*args, ptr(rows), ptr(off), rows.numel(), total, ptr(prod_ptr), ptr(tmp_col),
                                 ptr(tmp_val), ptr(row_nnz), ptr(ws), need.value, s), "pygsd_gram_hub")
        start = end


def intersect(a: SparseValues, b: SparseValues) -> SparseValues:
    """Entries present in both CSRs (same shape, ascending columns per row) with (a + b) != 0, value (a + b) / 2."""
    _cabi.require_gpu(a.val, b.val)
    dev = a.val.device
    n = a.csr.n_rows
    lib = _cabi.lib()
    with _cabi.on_device(dev):
        s = stream_ptr()
        pa = (ptr(a.csr.rowptr), ptr(a.csr.col), ptr(a.val), ptr(b.csr.rowptr), ptr(b.csr.col), ptr(b.val))
        count = torch.zeros(n, dtype=torch.int64, device=dev)
        check(lib.pygsd_csr_intersect_count(*pa, n, ptr(count), s), "pygsd_csr_intersect_count")
        c_ptr = _scan(count)
        nnz = int(c_ptr[-1])
        check_nnz(nnz, "CSR intersection")
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        val = torch.empty(nnz, dtype=torch.float32, device=dev)
        check(lib.pygsd_csr_intersect_emit(*pa, n, ptr(c_ptr), nnz, ptr(rowptr), ptr(col), ptr(val), s),
              "pygsd_csr_intersect_emit")
    return SparseValues(CSR(n, a.csr.n_cols, nnz, rowptr, col, None), val)


def coo_rows(m: SparseValues) -> Tensor:
    """int64 [2, nnz] (row, col) of a CSR in slot order (row-major)."""
    counts = (m.csr.rowptr[1:] - m.csr.rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(m.csr.n_rows, dtype=torch.int64, device=m.val.device), counts,
                                  output_size=m.csr.nnz)
    return torch.stack([row, m.csr.col.long()])


def from_coo(row: Tensor, col: Tensor, w: Tensor, n_rows: int, n_cols: int) -> Tuple[SparseValues, SparseValues]:
    """(M, M^T) as CSRs with values in slot order from COO entries (ids already validated)."""
    from .sparse import csr_from_coo, gather_values
    fwd = csr_from_coo(row, col, n_rows, n_cols, validate=False)
    bwd = csr_from_coo(col, row, n_cols, n_rows, validate=False)
    return SparseValues(fwd, gather_values(w, fwd.perm)), SparseValues(bwd, gather_values(w, bwd.perm))
