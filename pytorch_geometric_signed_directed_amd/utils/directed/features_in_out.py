"""DGCN's input pipeline: reference utils/directed/features_in_out.py:directed_features_in_out.

The reference loops over the N nodes and adds one sparse outer product per node into an N x N CSR matrix (O(N nnz)).
Both paths here compute the same second-order proximities as sparse Gram products:
    A_in  = A^T diag(1 / c) A      c = column sums of A (the reference's `out_degree`)
    A_out = A   diag(1 / r) A^T    r = row sums of A (`in_degree`)
with duplicate edges summed, existing self loops kept and none added, and sums equal to 0 replaced by 1.
CUDA tensors take the HIP path (csrc/spgemm.hip through sparse_gram.gram); CPU tensors a scipy sparse product in float64.
Indices are int64 in row-major order with ascending columns (the reference's unweighted `edge_out` comes out with columns
unsorted inside a row: a scipy artefact); values are float32."""
from typing import Optional, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from ... import _cabi
from ...sparse import segment_sum_raw
from ...sparse_build import sort_keys
from ...sparse_gram import coo_rows, from_coo, gram


def _undirected_device(row, col, size):
    """to_undirected(edge_index): the sorted, unique (row, col) pairs of both orientations."""
    keys = torch.cat([row * size + col, col * size + row])
    bits = max(1, int(size * size - 1).bit_length())
    srt, _ = sort_keys(keys, bits)
    keep = torch.ones_like(srt, dtype=torch.bool)
    keep[1:] = srt[1:] != srt[:-1]
    u = srt[keep]
    return torch.stack([u // size, u % size])


def _undirected_host(ei: np.ndarray, size: int) -> torch.Tensor:
    keys = np.unique(np.concatenate([ei[0] * size + ei[1], ei[1] * size + ei[0]]))
    return torch.from_numpy(np.stack([keys // size, keys % size]).astype(np.int64))


def _safe_inverse(d: torch.Tensor) -> torch.Tensor:
    d = d.double()
    return 1.0 / torch.where(d == 0, torch.ones_like(d), d)


def _features_device(edge_index, size, edge_weight, lds_limit):
    dev = edge_index.device
    row, col = edge_index[0].contiguous(), edge_index[1].contiguous()
    _cabi.check_node_ids((size, row), (size, col))
    w = (torch.ones(row.numel(), dtype=torch.float32, device=dev) if edge_weight is None
         else edge_weight.detach().to(device=dev, dtype=torch.float32).contiguous())
    a, at = from_coo(row, col, w, size, size)
    r = segment_sum_raw(a.csr.rowptr, None, a.val, size, a.csr)
    c = segment_sum_raw(at.csr.rowptr, None, at.val, size, at.csr)
    a_in = gram(a, at, _safe_inverse(c), lds_limit=lds_limit)
    a_out = gram(at, a, _safe_inverse(r), lds_limit=lds_limit)
    return _undirected_device(row, col, size), coo_rows(a_in), a_in.val, coo_rows(a_out), a_out.val


def _canonical(m) -> Tuple[torch.Tensor, torch.Tensor]:
    m = m.tocsr()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    coo = m.tocoo()
    index = torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64))
    return index, torch.from_numpy(coo.data.astype(np.float32))


def _features_host(edge_index, size, edge_weight):
    ei = edge_index.detach().cpu().numpy().astype(np.int64)
    w = np.ones(ei.shape[1]) if edge_weight is None else edge_weight.detach().cpu().double().numpy()
    a = sp.coo_matrix((w, (ei[0], ei[1])), shape=(size, size)).tocsr()
    c = np.asarray(a.sum(axis=0)).reshape(-1)
    r = np.asarray(a.sum(axis=1)).reshape(-1)
    c[c == 0] = 1
    r[r == 0] = 1
    e_in, w_in = _canonical(a.T @ sp.diags(1.0 / c) @ a)
    e_out, w_out = _canonical(a @ sp.diags(1.0 / r) @ a.T)
    return _undirected_host(ei, size), e_in, w_in, e_out, w_out


def directed_features_in_out(edge_index: torch.LongTensor, size: int, edge_weight: Optional[torch.FloatTensor] = None,
                             device: str = 'cpu', *, lds_limit: Optional[int] = None
                             ) -> Tuple[torch.LongTensor, torch.LongTensor, torch.FloatTensor, torch.LongTensor,
                                        torch.FloatTensor]:
    r"""Computes directed in-degree and out-degree features (DGCN's second-order proximities).

    Arg types:
        * **edge_index** (PyTorch LongTensor) - The edge indices.
        * **size** (int) - The number of nodes; may exceed the largest id (isolated nodes).
        * **edge_weight** (PyTorch Tensor, optional) - One-dimensional edge weights. (default: :obj:`None`, ones)
        * **device** (str, optional) - Ignored, as in the reference: outputs go on the device of :attr:`edge_index`.
        * **lds_limit** (int, optional) - CUDA only: rows of the Gram products with more products than this take the
          global-memory path (default: the largest LDS tier).  The result does not depend on it.

    Return types:
        * **index_undirected** (PyTorch LongTensor) - Undirected edge_index (sorted, unique, self loops kept).
        * **edge_in** (PyTorch LongTensor) - Inwards edge indices (row-major, ascending columns).
        * **in_weight** (PyTorch Tensor) - Inwards edge weights.
        * **edge_out** (PyTorch LongTensor) - Outwards edge indices (row-major, ascending columns).
        * **out_weight** (PyTorch Tensor) - Outwards edge weights.
    """
    size = int(size)
    dev = edge_index.device
    if edge_index.numel() == 0:
        e = torch.empty(2, 0, dtype=torch.long, device=dev)
        v = torch.empty(0, dtype=torch.float32, device=dev)
        return e, e.clone(), v, e.clone(), v.clone()
    if edge_index.is_cuda:
        return _features_device(edge_index, size, edge_weight, lds_limit)
    return _features_host(edge_index, size, edge_weight)
