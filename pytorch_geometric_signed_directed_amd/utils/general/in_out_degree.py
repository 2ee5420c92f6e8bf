"""Node degree features: reference utils/general/in_out_degree.py:in_out_degree.

Unsigned: [N, 2] = (row sums, column sums) of |w| (abs taken per edge; w = ones when absent).
Signed: [N, 4] = (in_pos, in_neg, out_pos, out_neg) from A_p = (|A| + A) / 2 and A_n = (|A| - A) / 2 AFTER duplicate edges
are summed; "in" = row sums, "out" = column sums, as the reference names them.
CUDA tensors are reduced with the device segment sums (pygsd_segment_sum_f32); CPU tensors with scipy."""
from typing import Optional

import numpy as np
import scipy.sparse as sp
import torch

from ... import _cabi
from ...sparse import CSR, csr_from_coo, segment_sum_raw
from ...sparse_build import sort_keys


def _sums_device(row, col, w, n):
    by_row = csr_from_coo(row, col, n, n, validate=False)
    by_col = csr_from_coo(col, row, n, n, validate=False)
    return (segment_sum_raw(by_row.rowptr, by_row.perm, w, n, by_row),
            segment_sum_raw(by_col.rowptr, by_col.perm, w, n, by_col))


def _coalesce_device(row, col, w, n):
    """Duplicate (row, col) entries summed, in row-major order."""
    keys = row * n + col
    srt, perm = sort_keys(keys, max(1, int(n * n - 1).bit_length()))
    head = torch.ones_like(srt, dtype=torch.bool)
    head[1:] = srt[1:] != srt[:-1]
    starts = torch.nonzero(head).flatten()
    rowptr = torch.cat([starts, torch.tensor([srt.numel()], device=srt.device)]).to(torch.int32)
    runs = CSR(starts.numel(), 0, srt.numel(), rowptr, None, perm)
    vals = segment_sum_raw(rowptr, perm, w, starts.numel(), runs)
    u = srt[starts]
    return u // n, u % n, vals


def in_out_degree(edge_index: torch.LongTensor, size: Optional[int] = None, signed: bool = False,
                  edge_weight: Optional[torch.FloatTensor] = None) -> torch.Tensor:
    r"""Get the in degrees and out degrees of nodes.

    Arg types:
        * **edge_index** (torch.LongTensor) The edge index.
        * **size** (int, optional) - The node number (default: largest id + 1).
        * **signed** (bool, optional) - Whether to take into account signed edge weights and to return signed 4D
          features. Default is False and to only account for absolute degrees.
        * **edge_weight** (PyTorch Tensor, optional) - One-dimensional edge weights. (default: :obj:`None`)

    Return types:
        * **degree** (Torch.Tensor) - float32 [|V|, 2] (in, out) when signed=False, otherwise [|V|, 4] with in-pos,
          in-neg, out-pos, out-neg degrees.  Returned on the device of :attr:`edge_index` (the reference always returns a
          CPU tensor).
    """
    if signed and edge_weight is None:
        raise ValueError('Edge weight input should not be None when generating features based on edge signs!')
    dev = edge_index.device
    n = int(size) if size is not None else (int(edge_index.max()) + 1 if edge_index.numel() else 0)
    if edge_index.is_cuda:
        row, col = edge_index[0].contiguous(), edge_index[1].contiguous()
        _cabi.check_node_ids((n, row), (n, col))
        if edge_weight is None:
            w = torch.ones(row.numel(), dtype=torch.float32, device=dev)
        else:
            w = edge_weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        if not signed:
            return torch.stack(_sums_device(row, col, w.abs(), n), dim=1)
        if row.numel() == 0:
            return torch.zeros(n, 4, dtype=torch.float32, device=dev)
        ur, uc, a = _coalesce_device(row, col, w, n)
        pos, neg = (a.abs() + a) / 2, (a.abs() - a) / 2
        in_pos, out_pos = _sums_device(ur, uc, pos.contiguous(), n)
        in_neg, out_neg = _sums_device(ur, uc, neg.contiguous(), n)
        return torch.stack([in_pos, in_neg, out_pos, out_neg], dim=1)
    ei = edge_index.detach().cpu().numpy().astype(np.int64)
    w = np.ones(ei.shape[1]) if edge_weight is None else edge_weight.detach().cpu().double().numpy()
    if not signed:
        w = np.abs(w)
    a = sp.coo_matrix((w, (ei[0], ei[1])), shape=(n, n)).tocsr()
    a.sum_duplicates()
    if signed:
        pos, neg = a.copy(), a.copy()
        pos.data = (np.abs(a.data) + a.data) / 2
        neg.data = (np.abs(a.data) - a.data) / 2
        cols = [pos.sum(axis=1), neg.sum(axis=1), pos.sum(axis=0).T, neg.sum(axis=0).T]
    else:
        cols = [a.sum(axis=1), a.sum(axis=0).T]
    return torch.from_numpy(np.concatenate([np.asarray(c).reshape(-1, 1) for c in cols], axis=1)).float()
