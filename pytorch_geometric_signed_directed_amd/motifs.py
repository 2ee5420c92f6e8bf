"""Host side of csrc/motifs.hip (include/pygsd_hip.h): the triangle-motif neighbourhoods of SDGNN and SiGAT built on the
device.

`signed_neighbourhoods` turns an [E, 3] (source, target, sign) list into the sorted unique keys u * n + v of U = P u N with
their P / N flags and the typed CSR (one entry per neighbour w of u, mask bit 0: w in out_P(u), 1: out_N(u), 2: in_P(u),
3: in_N(u)).  `motif_counts` gives, for every key (u, v), the 16 common-neighbour counts of the host path's `_motif_counts`
at (u, v) -- int32 [|U|, 16], counter 4 g + 2 x + y.  `sdgnn_lists` / `sdgnn_weights` / `sigat_lists` derive the models' edge lists and
SDGNN's triangle weights from them.  Every list is in ascending (first row, second row) order."""
import ctypes
from typing import List, NamedTuple, Optional

import torch

from . import _cabi
from ._cabi import check, ptr, stream_ptr
from .sparse_build import sort_keys
from .sparse_gram import check_nnz

Tensor = torch.Tensor

LANE_MAX_SHORT = 64   # keys whose shorter typed list is at most this long take tier 0 (one lane per key)
TIERS = (0, 1)        # 0: one lane per key, 1: one wavefront per key
# SDGNN's balanced-motif masks over the 16 counters (nn/models.py: SDGNN.build_edge_lists)
SDGNN_POS = (0, 4, 7, 11, 12, 15)
SDGNN_NEG = (1, 2, 6, 9, 10, 13)


class Neighbourhoods(NamedTuple):
    n: int
    keys: Tensor     # int64 [K]: u * n + v, ascending, unique
    flags: Tensor    # uint8 [K]: bit 0 = in P, bit 1 = in N
    rowptr: Tensor   # int32 [n + 1]
    col: Tensor      # int32 [nnz], ascending within a row
    mask: Tensor     # uint8 [nnz]


def _bits(x: int) -> int:
    return max(1, int(x).bit_length())


def signed_neighbourhoods(edge_index_s: Tensor, n: int) -> Neighbourhoods:
    """P / N: the distinct (source, target) pairs with sign > 0 / < 0 (duplicate listings collapse, sign 0 is ignored, a
    pair may be in both).  An id outside [0, n) of a kept row raises ValueError, as the host path's scipy does."""
    _cabi.require_gpu(edge_index_s)
    n = int(n)
    dev = edge_index_s.device
    if edge_index_s.dim() != 2 or edge_index_s.size(1) != 3:
        raise ValueError(f"edge_index_s must be [E, 3] (source, target, sign), got {tuple(edge_index_s.shape)}")
    if n < 0 or n > (1 << 31) - 1:
        raise ValueError(f"node_num {n} out of range: int32 columns hold at most 2^31 - 1 nodes")
    lib = _cabi.lib()
    with _cabi.on_device(dev):
        es = edge_index_s.detach()
        sign = es[:, 2]
        keep = sign != 0
        src, dst, neg = es[keep, 0].long(), es[keep, 1].long(), sign[keep] < 0
        if src.numel() and bool(((src < 0) | (src >= n) | (dst < 0) | (dst >= n)).any()):
            raise ValueError(f"edge_index_s: node ids must lie in [0, {n})")
        if src.numel():
            srt, _ = sort_keys(((src * n + dst) << 1) | neg.long(), _bits(2 * n * n - 1))
            pair = srt >> 1
            head = torch.ones_like(pair, dtype=torch.bool)
            head[1:] = pair[1:] != pair[:-1]
            tail = torch.ones_like(head)
            tail[:-1] = head[1:]
            keys = pair[head]
            # within a pair's run the positive listing sorts first and the negative one last
            flags = (((srt[head] & 1) == 0).to(torch.uint8) | (((srt[tail] & 1) == 1).to(torch.uint8) << 1))
        else:
            keys = torch.empty(0, dtype=torch.int64, device=dev)
            flags = torch.empty(0, dtype=torch.uint8, device=dev)
        k = keys.numel()
        check_nnz(2 * k, "typed motif neighbourhoods")
        need = ctypes.c_size_t(0)
        check(lib.pygsd_motif_workspace(k, ctypes.byref(need)), "pygsd_motif_workspace")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(2 * k, dtype=torch.int32, device=dev)
        mask = torch.empty(2 * k, dtype=torch.uint8, device=dev)
        check(lib.pygsd_motif_neighbourhoods(ptr(keys), ptr(flags), k, n, ptr(rowptr), ptr(col), ptr(mask), ptr(ws),
                                             need.value, stream_ptr()), "pygsd_motif_neighbourhoods")
        nnz = int(rowptr[-1]) if k else 0
    return Neighbourhoods(n, keys, flags, rowptr, col[:nnz], mask[:nnz])


def motif_counts(nb: Neighbourhoods, *, tier: Optional[int] = None) -> Tensor:
    """int32 [|U|, 16]: row i = the 16 counts of key i.  tier: None bins every key by the length of its shorter typed
    list (at most LANE_MAX_SHORT: one lane, else one wavefront); 0 or 1 sends every key to that tier."""
    if tier is not None and tier not in TIERS:
        raise ValueError(f"tier must be None or one of {TIERS}, got {tier}")
    k = nb.keys.numel()
    dev = nb.keys.device
    counts = torch.empty(k, 16, dtype=torch.int32, device=dev)
    if k == 0:
        return counts
    lib = _cabi.lib()
    with _cabi.on_device(dev):
        s = stream_ptr()
        args = (ptr(nb.keys), k, nb.n, ptr(nb.rowptr), ptr(nb.col), ptr(nb.mask))
        if tier is not None:
            check(lib.pygsd_motif_count(*args, None, k, tier, ptr(counts), s), "pygsd_motif_count")
            return counts
        deg = nb.rowptr[1:] - nb.rowptr[:-1]
        short = torch.minimum(deg[nb.keys // nb.n], deg[nb.keys % nb.n])
        lane = short <= LANE_MAX_SHORT
        for t, sel in ((0, lane), (1, ~lane)):
            ids = torch.nonzero(sel).flatten().to(torch.int32)
            if ids.numel():
                check(lib.pygsd_motif_count(*args, ptr(ids), ids.numel(), t, ptr(counts), s), "pygsd_motif_count")
    return counts


def probe_work(nb: Neighbourhoods) -> int:
    """Sum over the keys of min(d_u, d_v): the binary searches the count kernel performs."""
    deg = (nb.rowptr[1:] - nb.rowptr[:-1]).long()
    return int(torch.minimum(deg[nb.keys // nb.n], deg[nb.keys % nb.n]).sum()) if nb.keys.numel() else 0


def _csr_rows(nb: Neighbourhoods) -> Tensor:
    counts = (nb.rowptr[1:] - nb.rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(nb.n, dtype=torch.int64, device=nb.keys.device), counts,
                                   output_size=nb.col.numel())


def _typed(nb: Neighbourhoods, rows: Tensor, bits: int) -> Tensor:
    """[2, m] (u, w) over the CSR entries whose mask meets `bits`, ascending."""
    sel = (nb.mask & bits) != 0
    return torch.stack([rows[sel], nb.col[sel].long()])


def _pairs(nb: Neighbourhoods, idx: Tensor) -> Tensor:
    key = nb.keys[idx]
    return torch.stack([key // nb.n, key % nb.n])


def sdgnn_weights(nb: Neighbourhoods, counts: Tensor) -> Tensor:
    """int64 [|U|]: the balanced-motif count of every key -- the negative mask where the pair is in N, else the
    positive one."""
    pos = counts[:, list(SDGNN_POS)].long().sum(1)
    neg = counts[:, list(SDGNN_NEG)].long().sum(1)
    return torch.where((nb.flags & 2) != 0, neg, pos)


def sdgnn_lists(nb: Neighbourhoods) -> List[Tensor]:
    """[P, P^T, N, N^T] as int64 [2, .]: positive out-, positive in-, negative out-, negative in-neighbours."""
    rows = _csr_rows(nb)
    return [_typed(nb, rows, b) for b in (1, 4, 2, 8)]


def sigat_lists(nb: Neighbourhoods, counts: Tensor) -> List[Tensor]:
    """SiGAT's 38 lists: P u P^T, P, P^T, N u N^T, N, N^T, then P & (c_k > 0) and N & (c_k > 0) for k = 0 .. 15."""
    rows = _csr_rows(nb)
    out = [_typed(nb, rows, b) for b in (1 | 4, 1, 4, 2 | 8, 2, 8)]
    hit = counts > 0
    sel = torch.cat([hit & ((nb.flags & 1) != 0)[:, None], hit & ((nb.flags & 2) != 0)[:, None]], 1)   # [K, 32]
    nz = torch.nonzero(sel.t())                     # (list, key) in list-major, ascending key order
    sizes = torch.bincount(nz[:, 0], minlength=32).tolist() if nz.numel() else [0] * 32
    pairs = _pairs(nb, nz[:, 1])
    out += [p.contiguous() for p in torch.split(pairs, sizes, dim=1)]
    return out


def tri_weight_matrix(nb: Neighbourhoods, weight: Tensor):
    """SDGNN's `tri_weight` as a scipy csc_matrix with every key of U stored (explicit zeros included), from one
    device -> host copy."""
    import scipy.sparse as sp
    n, k = nb.n, nb.keys.numel()
    # the keys are in CSR order already: row pointers by search, columns and values as they stand
    indptr = torch.searchsorted(nb.keys, torch.arange(n + 1, dtype=torch.int64, device=nb.keys.device) * n)
    host = torch.cat([indptr, nb.keys % max(n, 1), weight.long()]).cpu().numpy()
    csr = sp.csr_matrix((host[n + 1 + k:], host[n + 1:n + 1 + k], host[:n + 1]), shape=(n, n))
    return csr.tocsc()


def lookup(nb: Neighbourhoods, values: Tensor, edge_index: Tensor) -> Tensor:
    """values[i] at the key of every listed edge (duplicates included) of an int64 [2, E] list of keys of U."""
    q = edge_index[0].long() * nb.n + edge_index[1].long()
    return values[torch.searchsorted(nb.keys, q)]
