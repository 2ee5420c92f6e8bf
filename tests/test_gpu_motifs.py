"""GPU: the triangle-motif counts (csrc/motifs.hip, motifs.py) behind the device path of SDGNN's and SiGAT's
`build_edge_lists`, against the reference's fixtures, the host path's scipy products (integer-exact, so bit for bit), and
itself (every tier, run to run)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bigdata
from conftest import load_golden
from tolerance import close

pytestmark = pytest.mark.gpu
D = "cuda:0"


def as_set(t):
    return set(map(tuple, t.t().tolist()))


def ascending(t):
    """Every device list is in ascending (first row, second row) order, without repeats."""
    if t.size(1) < 2:
        return True
    key = t[0] * (int(t.max()) + 1) + t[1]
    return bool((key[1:] > key[:-1]).all())


def host_counts_at(es, n, keys):
    """int64 [K, 16]: the host path's `_motif_counts` read at the device's keys (u * n + v), by a sorted merge."""
    from pytorch_geometric_signed_directed_amd.nn.models import _motif_counts, _signed_matrices
    P, N = _signed_matrices(es.cpu(), n)
    keys = keys.cpu().numpy()
    out = np.zeros((keys.size, 16), np.int64)
    for k, m in enumerate(_motif_counts(P, N)):
        coo = m.tocoo()
        kk = coo.row.astype(np.int64) * n + coo.col
        idx = np.searchsorted(keys, kk)
        hit = idx < keys.size
        hit[hit] &= keys[idx[hit]] == kk[hit]
        out[idx[hit], k] = coo.data[hit]
    return out, P, N


def host_keys(P, N, n):
    u = ((P + N) > 0).tocoo()
    return np.sort(u.row.astype(np.int64) * n + u.col)


def bare(cls, n):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.node_num, m.device = n, torch.device("cpu")
    return m


def check_against_host(es, n, tier=None):
    """Counts, flags, both models' lists and SDGNN's tri_weight of the device path against the host path."""
    from pytorch_geometric_signed_directed_amd import motifs
    from pytorch_geometric_signed_directed_amd.nn.models import SDGNN, SiGAT
    nb = motifs.signed_neighbourhoods(es.to(D), n)
    counts = motifs.motif_counts(nb, tier=tier)
    want, P, N = host_counts_at(es, n, nb.keys)
    assert np.array_equal(nb.keys.cpu().numpy(), host_keys(P, N, n))
    keys = nb.keys.cpu().numpy()
    flags = nb.flags.cpu().numpy()
    assert np.array_equal(flags & 1, np.asarray(P[keys // n, keys % n]).ravel() if keys.size else flags & 1)
    assert np.array_equal((flags >> 1) & 1, np.asarray(N[keys // n, keys % n]).ravel() if keys.size else flags & 1)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want)
    for cls in (SDGNN, SiGAT):
        host, dev = bare(cls, n), bare(cls, n)
        dev.device = torch.device(D)
        want_lists, got_lists = host.build_edge_lists(es.cpu()), dev.build_edge_lists(es.to(D))
        assert len(got_lists) == len(want_lists)
        for i, (g, w) in enumerate(zip(got_lists, want_lists)):
            assert g.is_cuda and g.dtype == torch.int64 and g.dim() == 2 and g.size(0) == 2, i
            assert as_set(g) == as_set(w) and g.size(1) == w.size(1), (cls.__name__, i)
            assert ascending(g), (cls.__name__, i)
        if cls is SDGNN:
            assert isinstance(dev.tri_weight, sp.csc_matrix) and dev.tri_weight.shape == (n, n)
            assert abs(dev.tri_weight.tocsr() - host.tri_weight.tocsr()).sum() == 0
    return counts


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------

def load_into(model, g):
    model.load_state_dict({k[3:]: g.t(k) for k in g if k.startswith("sd.")}, strict=True)
    return model.to(D).eval()


def test_sdgnn_fixture_on_the_device():
    from pytorch_geometric_signed_directed_amd.nn import SDGNN
    g = load_golden("model_sdgnn")
    m = SDGNN(40, g.t("edge_index_s", D), in_dim=8, out_dim=8, layer_num=2, init_emb=g.t("init_emb"))
    want = sp.coo_matrix((g["tri_val"], (g["tri_row"], g["tri_col"])), shape=(40, 40)).tocsr()
    assert isinstance(m.tri_weight, sp.csc_matrix)
    assert abs(m.tri_weight.tocsr() - want).sum() == 0
    m = load_into(m, g)
    assert all(e.is_cuda for e in m.edge_lists) and m.layers[0].edge_lists is m.edge_lists
    z = m()
    close(z, g["z"])
    pos, neg = m.pos_edge_index, m.neg_edge_index
    close(m.loss_sign(z, pos, neg), g["loss_sign"])
    close(m.loss_direction(z, pos, neg), g["loss_direction"])
    close(m.loss_tri(z, pos, neg), g["loss_tri"])
    close(m.loss(), g["loss_total"])


def test_sigat_fixture_on_the_device():
    from pytorch_geometric_signed_directed_amd.nn import SiGAT
    g = load_golden("model_sigat")
    m = SiGAT(40, g.t("edge_index_s", D), in_dim=8, out_dim=8, init_emb=g.t("init_emb"))
    assert [e.size(1) for e in m.edge_lists] == g["list_sizes"].tolist()
    host = SiGAT(40, g.t("edge_index_s"), in_dim=8, out_dim=8, init_emb=g.t("init_emb"))
    for a, b in zip(m.edge_lists, host.edge_lists):
        assert as_set(a) == as_set(b)
    m = load_into(m, g)
    close(m(), g["z"])
    close(m.loss(), g["loss"])


# ---- 2. counts against the host at 100 k nodes / 1 M entries -----------------------------------------------------------------

def signed_list(pe, ps):
    ei, sign = bigdata.load(pe), bigdata.load(ps)
    return torch.from_numpy(np.stack([ei[0], ei[1], np.asarray(sign).astype(np.int64)], 1))


@pytest.mark.parametrize("kind", ["sdsbm", "ssbm"])
def test_counts_match_host_products_at_100k(kind):
    from pytorch_geometric_signed_directed_amd import motifs
    n = 100_000
    es = signed_list(*(bigdata.sdsbm_graph(n, 1_000_000) if kind == "sdsbm" else bigdata.ssbm_graph(n, 1_000_000)))
    nb = motifs.signed_neighbourhoods(es.to(D), n)
    counts = motifs.motif_counts(nb)
    want, P, N = host_counts_at(es, n, nb.keys)
    assert np.array_equal(nb.keys.cpu().numpy(), host_keys(P, N, n))
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want)
    assert want.sum() > 0
    for tier in motifs.TIERS:
        assert torch.equal(motifs.motif_counts(nb, tier=tier), counts), tier


# ---- 3. corner cases ---------------------------------------------------------------------------------------------------------

def corner_graph():
    rows = [
        (0, 0, 1), (1, 1, -1), (2, 2, 1), (2, 2, -1),        # self-loops of both signs, one pair listed with both
        (0, 1, 1), (0, 1, 1), (1, 0, -1), (1, 0, -1),        # duplicates; a reciprocal pair of opposite signs
        (0, 2, 1), (0, 2, -1), (2, 0, 1),                    # a pair with both signs, reciprocal
        (1, 2, -1), (2, 3, 1), (3, 1, -1), (3, 0, 1),
        (4, 0, 0), (0, 4, 0), (5, 6, 0),                     # sign 0: ignored (node 4, 5, 6 then isolated)
        (7, 8, 1), (8, 7, 1), (8, 9, -1), (9, 7, 1), (7, 9, -1), (9, 9, 1),
        (3, 3, -1), (3, 2, 1), (2, 1, 1), (1, 3, 1),
    ]
    return torch.tensor(rows, dtype=torch.int64), 12                     # nodes 10, 11 isolated


def test_corner_cases_match_host():
    es, n = corner_graph()
    for tier in (None, 0, 1):
        check_against_host(es, n, tier)


def test_random_small_graphs_match_host():
    g = torch.Generator().manual_seed(5)
    for n, e in ((1, 3), (2, 8), (7, 40), (30, 400), (200, 3000)):
        es = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g),
                          torch.randint(-1, 2, (e,), generator=g)], 1)
        check_against_host(es, n)


@pytest.mark.parametrize("case", ["no_negative", "no_positive", "empty", "all_sign_zero"])
def test_empty_sets(case):
    from pytorch_geometric_signed_directed_amd import motifs
    from pytorch_geometric_signed_directed_amd.nn.models import SDGNN, SiGAT
    es, n = corner_graph()
    if case == "no_negative":
        es = es[es[:, 2] > 0]
    elif case == "no_positive":
        es = es[es[:, 2] < 0]
    elif case == "empty":
        es = es[:0]
    else:
        es = es.clone()
        es[:, 2] = 0
    check_against_host(es, n)
    if case in ("empty", "all_sign_zero"):
        nb = motifs.signed_neighbourhoods(es.to(D), n)
        assert nb.keys.numel() == 0 and motifs.motif_counts(nb).shape == (0, 16)
        assert int(nb.rowptr.abs().sum()) == 0
        for cls in (SDGNN, SiGAT):
            m = bare(cls, n)
            m.device = torch.device(D)
            lists = m.build_edge_lists(es.to(D))
            assert all(t.shape == (2, 0) and t.is_cuda for t in lists)
        m = bare(SDGNN, n)
        m.build_edge_lists(es.to(D))
        assert m.tri_weight.shape == (n, n) and abs(m.tri_weight).sum() == 0


# ---- 4. hubs and tiers -------------------------------------------------------------------------------------------------------

def hub_graph(n_leaves, seed=7):
    """Two adjacent hubs (nodes 0 and 1, linked both ways with both signs) and `n_leaves` leaves, each linked to each hub
    with probability 0.75 in a random direction and sign, plus a sparse random leaf-leaf layer."""
    rng = np.random.default_rng(seed)
    n = n_leaves + 2
    leaves = np.arange(2, n)
    rows = [np.array([[0, 1, 1], [1, 0, -1], [0, 1, -1], [1, 0, 1]])]
    for hub in (0, 1):
        pick = leaves[rng.random(n_leaves) < 0.75]
        out = rng.random(pick.size) < 0.5
        sign = np.where(rng.random(pick.size) < 0.6, 1, -1)
        src, dst = np.where(out, hub, pick), np.where(out, pick, hub)
        rows.append(np.stack([src, dst, sign], 1))
    m = 2 * n_leaves
    rows.append(np.stack([rng.choice(leaves, m), rng.choice(leaves, m), np.where(rng.random(m) < 0.7, 1, -1)], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.int64)), n


def test_hub_tiers_match_host():
    """Hubs of ~7.5 k neighbours (the host products stay small): every tier equals the host path bit for bit."""
    es, n = hub_graph(10_000)
    base = check_against_host(es, n)
    for tier in (0, 1):
        assert torch.equal(check_against_host(es, n, tier), base)


def test_large_hubs_every_tier_and_run_identical():
    """Hubs of ~50 k mixed in- and out-neighbours: tiers and repeated runs give identical bits; the hub-hub keys and a
    sample of leaf-hub keys equal a direct host set intersection."""
    from pytorch_geometric_signed_directed_amd import motifs
    from pytorch_geometric_signed_directed_amd.nn.models import _signed_matrices
    es, n = hub_graph(66_000)
    nb = motifs.signed_neighbourhoods(es.to(D), n)
    deg = (nb.rowptr[1:] - nb.rowptr[:-1])
    assert int(deg[0]) > 45_000 and int(deg[1]) > 45_000
    base = motifs.motif_counts(nb)
    assert torch.equal(motifs.motif_counts(nb), base)
    again = motifs.signed_neighbourhoods(es.to(D), n)
    assert all(torch.equal(a, b) for a, b in zip(again[1:], nb[1:]))
    for tier in motifs.TIERS:
        assert torch.equal(motifs.motif_counts(nb, tier=tier), base), tier
    P, N = _signed_matrices(es, n)
    cache = {}

    def typed(name, side, u):           # side 0: out-neighbours (CSR row), 1: in-neighbours (CSC column)
        if (name, side, u) not in cache:
            m = (P if name == "P" else N).tocsr() if side == 0 else (P if name == "P" else N).tocsc()
            cache[name, side, u] = set(m.indices[m.indptr[u]:m.indptr[u + 1]].tolist())
        return cache[name, side, u]
    keys = nb.keys.cpu().numpy()
    rng = np.random.default_rng(0)
    hub_keys = np.nonzero((keys // n < 2) & (keys % n < 2))[0]
    leaf_hub = np.nonzero(((keys // n < 2) ^ (keys % n < 2)))[0]
    sample = np.concatenate([hub_keys, rng.choice(leaf_hub, 200, replace=False), rng.choice(keys.size, 200)])
    got = base.cpu().numpy()
    for i in sample:
        u, v = divmod(int(keys[i]), n)
        for g, (su, sv) in enumerate(((0, 1), (0, 0), (1, 0), (1, 1))):   # 0 = out, 1 = in
            for x, xn in enumerate("PN"):
                for y, yn in enumerate("PN"):
                    assert got[i, 4 * g + 2 * x + y] == len(typed(xn, su, u) & typed(yn, sv, v)), (u, v, g, x, y)


# ---- 5 / 6. no host path, no scipy in the triangle loss ----------------------------------------------------------------------

def _raise(*_a, **_k):
    raise AssertionError("the host path ran")


def test_device_construction_takes_no_host_path(monkeypatch):
    from pytorch_geometric_signed_directed_amd.nn import SDGNN, SiGAT, models
    monkeypatch.setattr(models, "_signed_matrices", _raise)
    monkeypatch.setattr(models, "_motif_counts", _raise)
    es, n = hub_graph(2_000)
    emb = torch.randn(n, 8, generator=torch.Generator().manual_seed(0))
    sd = SDGNN(n, es.to(D), in_dim=8, out_dim=8, init_emb=emb.to(D))
    sg = SiGAT(n, es.to(D), in_dim=8, out_dim=8, init_emb=emb.to(D))
    assert all(e.is_cuda for e in sd.edge_lists) and len(sg.edge_lists) == 38 and all(e.is_cuda for e in sg.edge_lists)
    assert sd.tri_weight.nnz > 0


class _NoScipy:
    def tocsr(self):
        raise AssertionError("the triangle loss looked up scipy")


def test_triangle_loss_without_scipy():
    from pytorch_geometric_signed_directed_amd.nn import SDGNN
    es, n = hub_graph(2_000)
    es = torch.cat([es, es[:50]])                                  # duplicate listings reach the loss too
    emb = torch.randn(n, 8, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(3)
    dev = SDGNN(n, es.to(D), in_dim=8, out_dim=8, init_emb=emb.clone()).to(D)
    torch.manual_seed(3)
    host = SDGNN(n, es, in_dim=8, out_dim=8, init_emb=emb.clone()).to(D)
    host.load_state_dict(dev.state_dict())
    dev.loss_tri.edge_weight = _NoScipy()
    z = dev()
    close(dev.loss_tri(z, dev.pos_edge_index, dev.neg_edge_index),
          host.loss_tri(host(), host.pos_edge_index, host.neg_edge_index))
    close(dev.loss(), host.loss())


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["SDGNN", "SiGAT"])
def test_three_steps_device_built_vs_host_built(model):
    from pytorch_geometric_signed_directed_amd import nn as pnn
    cls = getattr(pnn, model)
    es, n = hub_graph(3_000, seed=11)
    emb = torch.randn(n, 8, generator=torch.Generator().manual_seed(2))
    losses = []
    for src in (es.to(D), es):
        torch.manual_seed(4)
        m = cls(n, src, in_dim=8, out_dim=8, init_emb=emb.clone()).to(D)
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        run = []
        for _ in range(3):
            opt.zero_grad()
            loss = m.loss()
            loss.backward()
            opt.step()
            run.append(loss.detach())
        losses.append(torch.stack(run))
    close(losses[0], losses[1].cpu().numpy())


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [(0, 12, 1), (-1, 0, -1), (3, -2, 1)])
def test_out_of_range_ids_raise(bad):
    from pytorch_geometric_signed_directed_amd import motifs
    from pytorch_geometric_signed_directed_amd.nn import SDGNN
    es, n = corner_graph()
    es = torch.cat([es, torch.tensor([bad])])
    with pytest.raises(ValueError):
        motifs.signed_neighbourhoods(es.to(D), n)
    with pytest.raises(ValueError):
        SDGNN(n, es.to(D), in_dim=4, out_dim=4, init_emb=torch.zeros(n, 4))
