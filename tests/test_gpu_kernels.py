"""GPU: the HIP kernels, called through the C-ABI host wrappers, against the CPU oracle
(oracle/ref_layers.py) on the same seeded inputs.

Bars: index / structure work (COO->CSR, sort, complex-ReLU masks) is BIT-EXACT; floating-point
aggregation is held to |got - want| <= 1e-5 (1 + |want|) per element (tests/tolerance.py; north_star: "within 1e-5 fp32"); summation order differs from
the reference only inside a row's lane groups.
"""
import numpy as np
import pytest
import torch

from oracle import ref_layers as R
from tolerance import close, close_arbitrated, single_thread

pytestmark = pytest.mark.gpu
TOL = 1e-5


def dev():
    return torch.device("cuda:0")


def rand_graph(n_in, n_out, nnz, seed, long_row=0, empty_tail=0):
    """COO (gather=src in [0,n_in), scatter=dst in [0,n_out)) with ragged rows, `empty_tail` output
    rows that receive nothing, and optionally one very long row (> 64 and > 256 entries)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_in, (nnz,), generator=g)
    hi = max(n_out - empty_tail, 1)
    dst = torch.randint(0, hi, (nnz,), generator=g)
    if long_row:
        dst[:long_row] = min(3, hi - 1)
    return torch.stack([src, dst])


# ------------------------------------------------------------------ structure (bit-exact)
@pytest.mark.parametrize("n,nnz,seed", [(1, 1, 0), (7, 0, 1), (50, 400, 2), (1000, 30000, 3), (4097, 100001, 4)])
def test_csr_from_coo_exact(n, nnz, seed):
    from pytorch_geometric_signed_directed_amd.sparse import csr_from_coo
    ei = rand_graph(n, n, nnz, seed, empty_tail=min(3, n - 1))
    csr = csr_from_coo(ei[1].to(dev()), ei[0].to(dev()), n, n)
    rowptr, col, perm = csr.rowptr.cpu().long(), csr.col.cpu().long(), csr.perm.cpu().long()
    # oracle: stable argsort by the segment id
    order = torch.sort(ei[1], stable=True).indices
    assert torch.equal(perm, order)
    assert torch.equal(col, ei[0][order])
    want_ptr = torch.zeros(n + 1, dtype=torch.long)
    want_ptr[1:] = torch.bincount(ei[1], minlength=n).cumsum(0)
    assert torch.equal(rowptr, want_ptr)


@pytest.mark.parametrize("n,bits,seed", [(0, 8, 0), (1, 1, 1), (1000, 10, 2), (200000, 40, 3)])
def test_sort_keys_exact_and_stable(n, bits, seed):
    from pytorch_geometric_signed_directed_amd.sparse_build import sort_keys
    g = torch.Generator().manual_seed(seed)
    keys = torch.randint(0, 2 ** min(bits, 20), (n,), generator=g)  # many duplicates -> stability visible
    if bits > 20 and n:
        keys = keys * (2 ** (bits - 20)) + torch.randint(0, 3, (n,), generator=g)
    skeys, perm = sort_keys(keys.to(dev()), bits)
    want = torch.sort(keys, stable=True)
    assert torch.equal(skeys.cpu(), want.values)
    assert torch.equal(perm.cpu().long(), want.indices)


def test_complex_relu_bit_exact():
    from pytorch_geometric_signed_directed_amd.nn import complex_relu_layer
    g = torch.Generator().manual_seed(6)
    for shape in [(1, 1), (37, 5), (1000, 64)]:
        re, im = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        re[0, 0] = 0.0
        re.view(-1)[-1] = -0.0
        o_r, o_i = complex_relu_layer()(re.to(dev()), im.to(dev()))
        w_r, w_i = R.complex_relu(re, im)
        assert np.array_equal(o_r.cpu().numpy().view(np.uint32), w_r.numpy().view(np.uint32))
        assert np.array_equal(o_i.cpu().numpy().view(np.uint32), w_i.numpy().view(np.uint32))
    # backward = same mask on the upstream gradients
    re = torch.randn(50, 8, generator=g)
    im = torch.randn(50, 8, generator=g)
    a, b = re.clone().requires_grad_(), im.clone().requires_grad_()
    o = R.complex_relu(a, b)
    gr, gi = torch.randn(50, 8, generator=g), torch.randn(50, 8, generator=g)
    ((o[0] * gr).sum() + (o[1] * gi).sum()).backward()
    c, d = re.to(dev()).requires_grad_(), im.to(dev()).requires_grad_()
    o2 = complex_relu_layer()(c, d)
    ((o2[0] * gr.to(dev())).sum() + (o2[1] * gi.to(dev())).sum()).backward()
    assert torch.equal(c.grad.cpu(), a.grad) and torch.equal(d.grad.cpu(), b.grad)


# ------------------------------------------------------------------ SpMM vs oracle propagate
FEATS = [1, 3, 4, 8, 16, 20, 32, 64, 96, 128, 256, 260, 300, 512]


@pytest.mark.parametrize("f", FEATS)
@pytest.mark.parametrize("weighted", [True, False])
def test_spmm_add_matches_oracle(f, weighted):
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n_in, n_out, nnz = 211, 173, 3000
    ei = rand_graph(n_in, n_out, nnz, seed=f, long_row=300, empty_tail=5)
    g = torch.Generator().manual_seed(100 + f)
    x = torch.randn(n_in, f, generator=g)
    w = torch.randn(nnz, generator=g) if weighted else None
    want = R.propagate(x, ei, w, n_out)                   # the reference's op sequence in fp32
    truth = R.propagate(x.double(), ei, None if w is None else w.double(), n_out)
    pat = Pattern(ei.to(dev()), n_in, n_out)
    got = spmm(pat, x.to(dev()), None if w is None else w.to(dev()))
    # a 300-entry row of N(0, 1) products: fp32 sums of that length sit at the 1e-5 bar whatever their order (this
    # check measured 9.1e-6 against the fp32 oracle at f = 128) -- float64 arbitrates (tests/tolerance.py)
    close_arbitrated(got, want, truth, what=f"spmm add f={f}")
    assert float(got[-5:].abs().max()) == 0.0  # rows that receive nothing are exactly zero


@pytest.mark.parametrize("f", [5, 16, 64, 128])
def test_spmm_mean_and_flow(f):
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n, nnz = 150, 2500
    ei = rand_graph(n, n, nnz, seed=7 + f, long_row=100, empty_tail=4)
    g = torch.Generator().manual_seed(f)
    x = torch.randn(n, f, generator=g)
    for flow in ("source_to_target", "target_to_source"):
        want = R.propagate(x, ei, None, n, flow=flow, reduce="mean")
        got = spmm(Pattern(ei.to(dev()), n, n, flow), x.to(dev()), None, reduce="mean")
        close(got, want)


@pytest.mark.parametrize("f", [6, 64, 128])
def test_spmm_chebyshev_epilogue(f):
    """alpha * S x + beta * z  with (alpha, beta) = (2, -1): T_k = 2 S T_{k-1} - T_{k-2}."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n, nnz = 120, 1500
    ei = rand_graph(n, n, nnz, seed=11)
    g = torch.Generator().manual_seed(f)
    x, z, w = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g), torch.randn(nnz, generator=g)
    want = 2.0 * R.propagate(x, ei, w, n) - z
    got = spmm(Pattern(ei.to(dev()), n, n), x.to(dev()), w.to(dev()), z=z.to(dev()), alpha=2.0, beta=-1.0)
    close(got, want)


def test_spmm_strided_column_slices():
    """SGCNConv deep layers aggregate x[..., :F] / x[..., F:] -- passed by row stride, no copy."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n, nnz = 90, 800
    ei = rand_graph(n, n, nnz, seed=13)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, 24, generator=g)
    xd = x.to(dev())
    pat = Pattern(ei.to(dev()), n, n)
    for sl in (slice(0, 12), slice(12, 24), slice(3, 10)):
        close(spmm(pat, xd[:, sl], None, reduce="mean"), R.propagate(x[:, sl], ei, None, n, reduce="mean"))


@pytest.mark.parametrize("f", [3, 16, 64, 72, 128, 256])
def test_spmm2_matches_two_propagates(f):
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm2
    n, nnz = 160, 2600
    ei = rand_graph(n, n, nnz, seed=17 + f, long_row=130, empty_tail=3)
    g = torch.Generator().manual_seed(f)
    xa, xb = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g)
    wa, wb = torch.randn(nnz, generator=g), torch.randn(nnz, generator=g)
    za, zb = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g)
    pat = Pattern(ei.to(dev()), n, n)
    d = dev()
    ya, yb = spmm2(pat, xa.to(d), xb.to(d), wa.to(d), wb.to(d))
    close(ya, R.propagate(xa, ei, wa, n))
    close(yb, R.propagate(xb, ei, wb, n))
    ya, yb = spmm2(pat, xa.to(d), xb.to(d), wa.to(d), wb.to(d), za=za.to(d), zb=zb.to(d), alpha=2.0, beta=-1.0)
    close(ya, 2.0 * R.propagate(xa, ei, wa, n) - za)
    close(yb, 2.0 * R.propagate(xb, ei, wb, n) - zb)


def test_empty_and_degenerate_inputs():
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    d = dev()
    # no edges at all
    ei = torch.zeros(2, 0, dtype=torch.long)
    out = spmm(Pattern(ei.to(d), 5, 4), torch.randn(5, 8).to(d), None)
    assert out.shape == (4, 8) and float(out.abs().max()) == 0.0
    # zero feature columns
    ei = rand_graph(10, 10, 30, 1)
    out = spmm(Pattern(ei.to(d), 10, 10), torch.zeros(10, 0).to(d), None)
    assert out.shape == (10, 0)
    # single node, self loop
    ei = torch.zeros(2, 1, dtype=torch.long)
    out = spmm(Pattern(ei.to(d), 1, 1), torch.full((1, 4), 3.0).to(d), torch.tensor([0.5]).to(d))
    assert out.cpu().tolist() == [[1.5] * 4]
    # an edgeless operator with an addend: y = z in every form (the in-place one returned zeros until round 6 -- found by
    # tests/test_gpu_fuzz.py through an SGCNConv without positive edges)
    from pytorch_geometric_signed_directed_amd.sparse import spmm_rows_into
    pat = Pattern(torch.zeros(2, 0, dtype=torch.long).to(d), 6, 6)
    x, z = torch.randn(6, 8).to(d), torch.randn(6, 16).to(d)
    assert torch.equal(spmm(pat, x, None, z=z[:, :8].contiguous(), beta=1.0), z[:, :8])
    for mean in (False, True):
        y = torch.full((6, 8), 7.0, device=d)
        spmm_rows_into(pat.fwd, None, x, y, mean=mean, z=z[:, 8:])
        assert torch.equal(y, z[:, 8:])
    y = torch.full((6, 8), 7.0, device=d)
    spmm_rows_into(pat.fwd, None, x, y, accumulate=True)
    assert float((y - 7.0).abs().max()) == 0.0
    spmm_rows_into(pat.fwd, None, x, y)
    assert float(y.abs().max()) == 0.0


def test_sgcn_conv_without_positive_or_negative_edges():
    """Either edge list may be empty: that half's aggregate is zero and its own-feature block must survive (the fused path
    adds the aggregate onto the own block inside the SpMM's epilogue -- with no entries there is no launch)."""
    from pytorch_geometric_signed_directed_amd.nn import SGCNConv
    g = torch.Generator().manual_seed(77)
    n = 40
    some, none = torch.randint(0, n, (2, 90), generator=g), torch.zeros(2, 0, dtype=torch.long)
    for first, in_dim, out_dim in ((True, 16, 12), (False, 16, 12), (True, 8, 24), (False, 5, 7)):
        x = torch.randn(n, in_dim if first else 2 * in_dim, generator=g)
        up = torch.randn(n, 2 * out_dim, generator=g)
        for pos, neg in ((none, some), (some, none), (none, none)):
            torch.manual_seed(5)
            layer = SGCNConv(in_dim, out_dim, first, norm_emb=True)
            prm = {k: v.detach().clone().requires_grad_() for k, v in layer.named_parameters()}
            xo = x.clone().requires_grad_()
            want = R.sgcn_conv(xo, pos, neg, (prm["lin_b.weight"], prm["lin_b.bias"]), (prm["lin_u.weight"], prm["lin_u.bias"]),
                               first, in_dim, True)
            (want * up).sum().backward()
            layer.to(dev())
            xd = x.to(dev()).requires_grad_()
            out = layer(xd, pos.to(dev()), neg.to(dev()))
            (out * up.to(dev())).sum().backward()
            close(out, want.detach())
            close(xd.grad, xo.grad)
            for k, p in layer.named_parameters():
                close(p.grad, prm[k].grad, norm=True, what="d " + k)


# ------------------------------------------------------------------ autograd through the kernels
@pytest.mark.parametrize("f", [7, 64])
@pytest.mark.parametrize("reduce", ["add", "mean"])
def test_spmm_backward_matches_oracle(f, reduce):
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n_in, n_out, nnz = 130, 110, 1700
    ei = rand_graph(n_in, n_out, nnz, seed=23, long_row=90, empty_tail=2)
    g = torch.Generator().manual_seed(f)
    x0, w0 = torch.randn(n_in, f, generator=g), torch.randn(nnz, generator=g)
    go = torch.randn(n_out, f, generator=g)
    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    (R.propagate(x, ei, w, n_out, reduce=reduce) * go).sum().backward()
    d = dev()
    xg, wg = x0.to(d).requires_grad_(), w0.to(d).requires_grad_()
    (spmm(Pattern(ei.to(d), n_in, n_out), xg, wg, reduce=reduce) * go.to(d)).sum().backward()
    close(xg.grad, x.grad)
    close(wg.grad, w.grad)  # SDDMM


def test_spmm2_backward_matches_oracle():
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm2
    n, nnz, f = 140, 2100, 64
    ei = rand_graph(n, n, nnz, seed=29, long_row=70)
    g = torch.Generator().manual_seed(29)
    t = [torch.randn(n, f, generator=g) for _ in range(4)]
    w = [torch.randn(nnz, generator=g) for _ in range(2)]
    xa, xb = t[0].clone().requires_grad_(), t[1].clone().requires_grad_()
    wa, wb = w[0].clone().requires_grad_(), w[1].clone().requires_grad_()
    ((R.propagate(xa, ei, wa, n) * t[2]).sum() + (R.propagate(xb, ei, wb, n) * t[3]).sum()).backward()
    d = dev()
    ga, gb = t[0].to(d).requires_grad_(), t[1].to(d).requires_grad_()
    va, vb = w[0].to(d).requires_grad_(), w[1].to(d).requires_grad_()
    ya, yb = spmm2(Pattern(ei.to(d), n, n), ga, gb, va, vb)
    ((ya * t[2].to(d)).sum() + (yb * t[3].to(d)).sum()).backward()
    close(ga.grad, xa.grad)
    close(gb.grad, xb.grad)
    close(va.grad, wa.grad)
    close(vb.grad, wb.grad)


# ------------------------------------------------------------------ seeded mid-size vs oracle
def test_spmm2_midsize_f64_vs_oracle():
    """N = 20k, nnz = 800k, F = 64: the benchmark's kernel configuration at a size the oracle
    finishes in seconds."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm2
    n, nnz, f = 20000, 800000, 64
    g = torch.Generator().manual_seed(31)
    ei = torch.randint(0, n, (2, nnz), generator=g)
    xa, xb = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g)
    wa, wb = torch.randn(nnz, generator=g) * 0.1, torch.randn(nnz, generator=g) * 0.1
    d = dev()
    ya, yb = spmm2(Pattern(ei.to(d), n, n), xa.to(d), xb.to(d), wa.to(d), wb.to(d))
    close(ya, R.propagate(xa, ei, wa, n))
    close(yb, R.propagate(xb, ei, wb, n))


# ------------------------------------------------------------------ full-size properties
def test_fullsize_linearity_and_adjoint():
    """BASELINE configs[1] size (100k nodes / ~4.1M operator entries / F = 64) through
    size-independent properties: linearity S(ax+by) = aSx + bSy, the adjoint identity
    <y, S x> = <S^T y, x> tying the forward (by-target) and backward (by-source) CSRs together,
    and S 1 = row sums."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n, nnz, f = 100000, 4100000, 64
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(37)
    ei = torch.randint(0, n, (2, nnz), generator=g).to(d)
    w = (torch.rand(nnz, generator=g) - 0.5).to(d)
    x = torch.randn(n, f, generator=g).to(d)
    y = torch.randn(n, f, generator=g).to(d)
    pat = Pattern(ei, n, n)
    sx, sy = spmm(pat, x, w), spmm(pat, y, w)
    lin = spmm(pat, 0.75 * x - 1.5 * y, w)
    # S (0.75 x - 1.5 y) against the float64 value of 0.75 S x - 1.5 S y, at the standard bar

    def s64(v):
        return torch.zeros(n, f, dtype=torch.float64, device=d).index_add_(0, ei[1], w.double()[:, None] * v.double()[ei[0]])

    sx64, sy64 = s64(x), s64(y)
    close(sx, sx64, what="S x vs float64")
    close(lin, 0.75 * sx64 - 1.5 * sy64, what="S (0.75 x - 1.5 y) vs float64 of 0.75 S x - 1.5 S y")
    xg = x.clone().requires_grad_()
    (spmm(pat, xg, w) * y).sum().backward()           # xg.grad = S^T y via the by-source CSR
    lhs = float((y.double() * sx.double()).sum())
    rhs = float((xg.grad.double() * x.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))
    ones = torch.ones(n, 4, device=d)
    rowsum = torch.zeros(n, device=d, dtype=torch.float64).index_add_(0, ei[1], w.double())
    rowsum32 = torch.zeros(n, device=d).index_add_(0, ei[1], w)          # the reference's scatter in fp32
    close_arbitrated(spmm(pat, ones, w)[:, 0], rowsum32, rowsum, what="S 1 = row sums")


# ------------------------------------------------------------------ fused MFMA dense stage
@pytest.mark.parametrize("f_in,f_out,k1", [(16, 16, 1), (32, 48, 2), (48, 32, 3), (64, 64, 2), (64, 64, 4),
                                            (64, 128, 2), (128, 64, 2), (128, 128, 2), (128, 128, 3), (16, 64, 2)])
@pytest.mark.parametrize("n", [1, 37, 1000])
def test_dense_stage_matches_reference_formula(f_in, f_out, k1, n):
    """out_real = sum_k (A_k - B_k) W_k + b, out_imag = sum_k (A_k + B_k) W_k + b and its gradients,
    evaluated the reference's way (four matmul chains, then -, +, += bias; MagNetConv.py:189-247) in
    float64 on the CPU.  Asymmetric random W catches row/column swaps of the MFMA fragments."""
    from pytorch_geometric_signed_directed_amd.dense import dense_bwd_raw, dense_fwd_raw, dense_supported
    assert dense_supported(f_in, f_out, k1)
    g = torch.Generator().manual_seed(1000 * f_in + 10 * f_out + k1 + n)
    a = [torch.randn(n, f_in, generator=g) for _ in range(k1)]
    b = [torch.randn(n, f_in, generator=g) for _ in range(k1)]
    w = torch.randn(k1, f_in, f_out, generator=g) * 0.3
    bias = torch.randn(f_out, generator=g)
    gr, gi = torch.randn(n, f_out, generator=g), torch.randn(n, f_out, generator=g)
    # reference formula in float64
    ad = [t.double().requires_grad_() for t in a]
    bd = [t.double().requires_grad_() for t in b]
    wd, bbd = w.double().requires_grad_(), bias.double().requires_grad_()
    rr = sum(ad[k] @ wd[k] for k in range(k1))
    ii = sum(bd[k] @ wd[k] for k in range(k1))
    want_r, want_i = rr - ii + bbd, rr + ii + bbd
    ((want_r * gr.double()).sum() + (want_i * gi.double()).sum()).backward()
    d = dev()
    # the same formula in fp32 on the host: what the reference's own arithmetic achieves against float64 (one thread: reproducible)
    with single_thread():
        rr32 = sum(a[k] @ w[k] for k in range(k1))
        ii32 = sum(b[k] @ w[k] for k in range(k1))
    o_r, o_i = dense_fwd_raw([t.to(d) for t in a], [t.to(d) for t in b], w.to(d), bias.to(d))
    close_arbitrated(o_r, rr32 - ii32 + bias, want_r, what="dense out_real")
    close_arbitrated(o_i, rr32 + ii32 + bias, want_i, what="dense out_imag")
    da, db, dw, dbias = dense_bwd_raw([t.to(d) for t in a], [t.to(d) for t in b], w.to(d), gr.to(d), gi.to(d))
    p32, m32 = gr + gi, gi - gr
    with single_thread():
        da32 = [p32 @ w[k].t() for k in range(k1)]
        db32 = [m32 @ w[k].t() for k in range(k1)]
        dw32 = torch.stack([a[k].t() @ p32 + b[k].t() @ m32 for k in range(k1)])
    for k in range(k1):
        close_arbitrated(da[k], da32[k], ad[k].grad, what="dense dA")
        close_arbitrated(db[k], db32[k], bd[k].grad, what="dense dB")
    # reductions over the n rows (tests/tolerance.py): the reference's own fp32 formula arbitrated by float64
    close_arbitrated(dw, dw32, wd.grad, norm=True, what="dense dW")
    close_arbitrated(dbias, p32.sum(0), bbd.grad, norm=True, what="dense db")
    # no-bias forward
    o_r, o_i = dense_fwd_raw([t.to(d) for t in a], [t.to(d) for t in b], w.to(d), None)
    close(o_r, want_r - bbd)


@pytest.mark.parametrize("f_in,f_out,k1,n", [(64, 64, 2, 5000), (32, 48, 1, 777), (128, 128, 3, 1030)])
def test_dense_backward_takes_a_broadcast_gradient_row(f_in, f_out, k1, n):
    """The upstream gradient of a loss that sums the outputs over the nodes is ONE row broadcast to every node (an
    expanded tensor): the kernel reads it with a zero row stride -- bit-identical to the materialised [N, F] gradient."""
    from pytorch_geometric_signed_directed_amd.dense import dense_bwd_raw
    g = torch.Generator().manual_seed(f_in + n)
    a = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    b = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    w = torch.randn(k1, f_in, f_out, generator=g).to(dev())
    row_r, row_i = torch.randn(1, f_out, generator=g).to(dev()), torch.randn(1, f_out, generator=g).to(dev())
    full = dense_bwd_raw(a, b, w, row_r.expand(n, f_out).contiguous(), row_i.expand(n, f_out).contiguous())
    lean = dense_bwd_raw(a, b, w, row_r.expand(n, f_out), row_i.expand(n, f_out))
    for x, y in zip(full[0] + full[1] + [full[2], full[3]], lean[0] + lean[1] + [lean[2], lean[3]]):
        assert torch.equal(x, y)
    # ... and through autograd: (out_real.sum() + 2 out_imag.sum()).backward() hands the layer expanded gradients
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv
    if f_in == f_out:
        ei = rand_graph(n, n, 6 * n, 5).to(dev())
        conv = MagNetConv(f_in, f_out, K=k1 - 1 or 1, q=0.25, trainable_q=False, cached=True).to(dev())
        grads = []
        for materialise in (False, True):
            xr, xi = a[0].clone().requires_grad_(), b[0].clone().requires_grad_()
            conv.zero_grad(set_to_none=True)
            o_r, o_i = conv(xr, xi, ei)
            if materialise:
                (o_r * torch.ones_like(o_r)).sum().add((o_i * torch.full_like(o_i, 2.0)).sum()).backward()
            else:
                (o_r.sum() + 2.0 * o_i.sum()).backward()
            grads.append((xr.grad, xi.grad, conv.weight.grad.clone(), conv.bias.grad.clone()))
        for x, y in zip(*grads):
            assert torch.equal(x, y)


@pytest.mark.parametrize("f_in,f_out,k1,n", [(64, 64, 2, 1), (64, 64, 3, 37), (128, 128, 3, 1030), (64, 128, 2, 4099), (128, 64, 2, 20000)])
def test_dense_forward_split_form_against_exact_form_and_float64(f_in, f_out, k1, n):
    """The default arithmetic of the magnetic dense forward at f_in = 64 / 128 and f_out a multiple of 64 (D = A - B and S = A + B
    split into three bf16 pieces, six partial products per product on the bf16 matrix pipe, the partial products of every
    32-feature block summed apart and added to the running sums once -- include/pygsd_hip.h: pygsd_dense_f32_form) next to the
    exact form (an fmaf chain per output), both against float64 relative to the sum of |terms|: the split form must be the CLOSER
    one (measured: a fifth of the chain's error)."""
    from pytorch_geometric_signed_directed_amd.dense import dense_fwd_raw, set_dense_f32_exact
    g = torch.Generator().manual_seed(f_in + 3 * f_out + k1 + n)
    a = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    b = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    w = (torch.randn(k1, f_in, f_out, generator=g) / f_in ** 0.5).to(dev())
    bias = torch.randn(f_out, generator=g).to(dev())
    w64 = w.double()
    want_r = sum((a[k].double() - b[k].double()) @ w64[k] for k in range(k1)) + bias.double()
    want_i = sum((a[k].double() + b[k].double()) @ w64[k] for k in range(k1)) + bias.double()
    scale = sum((a[k].double().abs() + b[k].double().abs()) @ w64[k].abs() for k in range(k1)) + bias.double().abs()
    res = {}
    for exact in (False, True):
        prev = set_dense_f32_exact(exact)
        try:
            o_r, o_i = dense_fwd_raw(a, b, w, bias)
            if not exact:
                again = dense_fwd_raw(a, b, w, bias)
                assert torch.equal(again[0], o_r) and torch.equal(again[1], o_i)          # deterministic
        finally:
            set_dense_f32_exact(prev)
        close(o_r, want_r, TOL, what="out_real")
        close(o_i, want_i, TOL, what="out_imag")
        res[exact] = (o_r, max(float(((o_r.double() - want_r).abs() / scale).max()), float(((o_i.double() - want_i).abs() / scale).max())))
    assert not torch.equal(res[False][0], res[True][0])                # (two forms really ran)
    assert res[False][1] <= max(res[True][1], 2.0 ** -23), (res[False][1], res[True][1])


@pytest.mark.parametrize("f_in,f_out,k1,n,broadcast", [(64, 64, 2, 1, False), (64, 64, 2, 37, False), (64, 64, 1, 4099, False),
                                                       (64, 64, 3, 20000, False), (128, 64, 3, 1030, False), (64, 64, 2, 70001, True),
                                                       (128, 128, 3, 1030, False), (64, 128, 2, 4099, False), (128, 128, 2, 17, True)])
def test_dense_backward_split_form_against_exact_form_and_float64(f_in, f_out, k1, n, broadcast):
    """The default arithmetic of the magnetic dense backward at f_out = 64 / 128 (operands as three bf16 pieces, six partial products
    per product on the bf16 matrix pipe, include/pygsd_hip.h: pygsd_dense_f32_form) next to the exact form (fmaf chains) on the
    same inputs, both against float64 relative to the sum of |terms| of each output.  dA / dB: inside 1.25x the exact form's own
    worst error (measured 0.2 - 0.35x); dW (a reduction over all rows, both forms at 1e-8 of the scale): inside 4x; dbias is
    computed identically (bitwise).  f_in = 128 runs two 64-column chunks; n = 1 / 37 / 4099 end in ragged tiles."""
    from pytorch_geometric_signed_directed_amd.dense import dense_bwd_raw, set_dense_f32_exact
    g = torch.Generator().manual_seed(f_in + k1 + n)
    a = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    b = [torch.randn(n, f_in, generator=g).to(dev()) for _ in range(k1)]
    w = (torch.randn(k1, f_in, f_out, generator=g) / f_in ** 0.5).to(dev())
    if broadcast:
        gr, gi = (torch.randn(1, f_out, generator=g).to(dev()).expand(n, f_out) for _ in range(2))
    else:
        gr, gi = (torch.randn(n, f_out, generator=g).to(dev()) for _ in range(2))
    p64, m64, w64 = (gr + gi).double(), (gi - gr).double(), w.double()

    def errors(res):
        da, db, dw, dbias = res
        e_rows = e_w = 0.0
        for k in range(k1):
            wt = w64[k].t()
            for got, src in ((da[k], p64), (db[k], m64)):
                e_rows = max(e_rows, float(((got.double() - src @ wt).abs() / (src.abs() @ wt.abs())).max()))
            a64, b64 = a[k].double(), b[k].double()
            want = a64.t() @ p64 + b64.t() @ m64
            scale = a64.abs().t() @ p64.abs() + b64.abs().t() @ m64.abs()
            e_w = max(e_w, float(((dw[k].double() - want).abs() / scale).max()))
            close(dw[k], want, TOL, norm=True, what="dW")
            close(da[k], p64 @ wt, TOL, what="dA")
            close(db[k], m64 @ wt, TOL, what="dB")
        close(dbias, p64.sum(0), TOL, norm=True, what="dbias")
        return e_rows, e_w

    prev = set_dense_f32_exact(False)
    try:
        split = dense_bwd_raw(a, b, w, gr, gi)
        again = dense_bwd_raw(a, b, w, gr, gi)
        set_dense_f32_exact(True)
        exact = dense_bwd_raw(a, b, w, gr, gi)
    finally:
        set_dense_f32_exact(prev)
    for x, y in zip(split[0] + split[1] + [split[2], split[3]], again[0] + again[1] + [again[2], again[3]]):
        assert torch.equal(x, y)                                    # deterministic
    assert not torch.equal(split[0][0], exact[0][0])                # (two forms really ran)
    assert torch.equal(split[3], exact[3])                          # dbias: the same sums in the same order
    rows_s, w_s = errors(split)
    rows_e, w_e = errors(exact)
    assert rows_s <= max(1.25 * rows_e, 2.0 ** -23), (rows_s, rows_e)
    assert w_s <= max(4.0 * w_e, 2.0 ** -23), (w_s, w_e)


def test_dense_supported_predicate():
    from pytorch_geometric_signed_directed_amd.dense import dense_supported
    assert dense_supported(64, 64, 2) and dense_supported(128, 128, 3) and dense_supported(16, 16, 1)
    for bad in [(6, 5, 2), (64, 96, 2), (64, 64, 5), (80, 64, 2), (2879, 16, 2)]:
        assert not dense_supported(*bad)


# ------------------------------------------------------------------ operator build (HIP pipeline)
def _messy_graph(n, e, seed, signed=False):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 3, (e,), generator=g)          # last 3 nodes isolated
    dst = torch.randint(0, n - 3, (e,), generator=g)
    src = torch.cat([src, dst[:e // 10], src[:e // 20]])      # reciprocal pairs + exact duplicates
    dst = torch.cat([dst, src[:e // 10], dst[:e // 20]])
    loops = torch.randint(0, n - 3, (e // 50 + 2,), generator=g)
    src, dst = torch.cat([src, loops, loops[:2]]), torch.cat([dst, loops, loops[:2]])  # incl. duplicate loops
    perm = torch.randperm(src.numel(), generator=g)
    ei = torch.stack([src[perm], dst[perm]])
    w = torch.rand(ei.size(1), generator=g) + 0.5
    if signed:
        w = w * (torch.randint(0, 2, (ei.size(1),), generator=g) * 2 - 1).float()
    return ei, w


@pytest.mark.parametrize("n,e,signed,absdeg,norm,weighted", [
    (50, 300, False, True, "sym", True), (50, 300, False, True, None, False),
    (3000, 40000, False, True, "sym", True), (3000, 40000, True, True, "sym", True),
    (3000, 40000, True, False, "sym", True), (3000, 40000, True, True, None, True),
    (20000, 400000, False, True, "sym", False)])
def test_laplacian_build_matches_oracle(n, e, signed, absdeg, norm, weighted):
    from pytorch_geometric_signed_directed_amd.utils import get_magnetic_Laplacian, get_magnetic_signed_Laplacian
    ei, w = _messy_graph(n, e, seed=n + e, signed=signed)
    if not weighted:
        w = None
    want_i, want_r, want_m = R.magnetic_laplacian(ei, w, n, 0.2, norm, signed, absdeg)
    d = dev()
    wd = None if w is None else w.to(d)
    if signed:
        got_i, got_r, got_m = get_magnetic_signed_Laplacian(ei.to(d), wd, norm, None, n, 0.2, absolute_degree=absdeg)
    else:
        got_i, got_r, got_m = get_magnetic_Laplacian(ei.to(d), wd, norm, None, n, 0.2)
    assert torch.equal(got_i.cpu(), want_i)          # index layout: bit-exact
    close(got_r, want_r, 1e-6)
    close(got_m, want_m, 1e-6)


def test_laplacian_build_degenerate():
    from pytorch_geometric_signed_directed_amd.utils import get_magnetic_Laplacian
    d = dev()
    # only self loops -> no off-diagonal entries, N unit loops
    ei = torch.tensor([[0, 1, 1], [0, 1, 1]])
    i, r, m = get_magnetic_Laplacian(ei.to(d), None, "sym", None, 3, 0.25)
    assert i.cpu().tolist() == [[0, 1, 2], [0, 1, 2]] and r.cpu().tolist() == [1.0, 1.0, 1.0]
    # no edges at all
    i, r, m = get_magnetic_Laplacian(torch.zeros(2, 0, dtype=torch.long, device=d), None, "sym", None, 2, 0.25)
    assert i.cpu().tolist() == [[0, 1], [0, 1]] and m.cpu().tolist() == [0.0, 0.0]


@pytest.mark.parametrize("weighted", [True, False])
def test_self_loops_and_norms_match_oracle(weighted):
    from pytorch_geometric_signed_directed_amd.utils import add_remaining_self_loops, conv_norm_rw, gcn_norm
    n = 2000
    ei, w = _messy_graph(n, 30000, seed=5)
    if not weighted:
        w = None
    d = dev()
    wd = None if w is None else w.to(d)
    if weighted:
        got_i, got_w = add_remaining_self_loops(ei.to(d), wd, 0.5, n)
        want_i, want_w = R.append_remaining_self_loops(ei, w, 0.5, n)
        assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_w.cpu(), want_w)   # bit-exact
    for improved in (False, True):
        gi, gw = gcn_norm(ei.to(d), wd, n, improved, True)
        wi, ww = R.gcn_norm(ei, w, n, improved, True)
        assert torch.equal(gi.cpu(), wi)
        close(gw, ww, 1e-6)
    gi, gw = gcn_norm(ei.to(d), wd, n, False, False)
    wi, ww = R.gcn_norm(ei, w, n, False, False)
    assert torch.equal(gi.cpu(), wi)
    close(gw, ww, 1e-6)
    for fill in (0.5, 0.0):
        gi, gw = conv_norm_rw(ei.to(d), fill, wd, n)
        wi, ww = R.conv_norm_rw(ei, w, n, fill)
        assert torch.equal(gi.cpu(), wi)
        close(gw, ww, 1e-6)


# ------------------------------------------------------------------ bf16 storage (BASELINE config C5)
@pytest.mark.parametrize("f", [8, 16, 64, 128, 256, 520, 20])
def test_spmm_bf16_vs_oracle_on_rounded_inputs(f):
    """Parity for the bf16-storage SpMM is defined against the fp32 oracle evaluated on the
    bf16-ROUNDED inputs; the only extra error is the final bf16 rounding of the
    result (relative 2^-8) on top of the 1e-5 accumulation bar."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    n, nnz = 300, 6000
    ei = rand_graph(n, n, nnz, seed=f, long_row=150, empty_tail=3)
    g = torch.Generator().manual_seed(f)
    x = torch.randn(n, f, generator=g).to(torch.bfloat16)
    z = torch.randn(n, f, generator=g).to(torch.bfloat16)
    w = torch.rand(nnz, generator=g)
    want = 2.0 * R.propagate(x.float(), ei, w, n) - z.float()
    d = dev()
    got = spmm(Pattern(ei.to(d), n, n), x.to(d), w.to(d), z=z.to(d), alpha=2.0, beta=-1.0)
    assert got.dtype == torch.bfloat16
    err = (got.float().cpu() - want).abs()
    bound = want.abs() * 2.0 ** -8 + 1e-5 * max(1.0, float(want.abs().max()))
    assert bool((err <= bound).all()), float((err - bound).max())
    # mean aggregation, no values
    want = R.propagate(x.float(), ei, None, n, reduce="mean")
    got = spmm(Pattern(ei.to(d), n, n), x.to(d), None, reduce="mean").float().cpu()
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-5).all())


def test_digcn_conv_bf16_layer():
    from pytorch_geometric_signed_directed_amd.nn import DiGCNConv
    n, e, fi, fo = 500, 8000, 64, 64
    g = torch.Generator().manual_seed(9)
    ei = torch.randint(0, n, (2, e), generator=g)
    w = torch.rand(e, generator=g) / 16
    x = torch.randn(n, fi, generator=g)
    torch.manual_seed(9)
    layer = DiGCNConv(fi, fo)
    wt, bs = layer.weight.detach().clone(), layer.bias.detach().clone()
    # oracle on bf16-rounded operands, bf16 rounding after the dense product as the layer does
    h = (x.to(torch.bfloat16).float() @ wt.to(torch.bfloat16).float()).to(torch.bfloat16).float()
    want = R.propagate(h, ei, w, n) + bs.to(torch.bfloat16).float()
    d = dev()
    out = layer.to(d).to(torch.bfloat16)(x.to(d).to(torch.bfloat16), ei.to(d), w.to(d))
    assert out.dtype == torch.bfloat16
    err = (out.float().cpu() - want).abs()
    assert bool((err <= want.abs() * 2.0 ** -7 + 2e-2).all()), float(err.max())


def test_spmm_variants_are_bitwise_identical():
    """The nnz hint only selects a tuning variant.  Deep gather pipelining vs high occupancy: every lane group
    accumulates its neighbours in the same order in both, so the outputs are bit-identical.  The rows-per-wavefront
    variant (a tiny hint: few entries per row) sums a row sequentially in CSR order instead: equal to fp32 rounding,
    and deterministic."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse import Pattern
    d = dev()
    g = torch.Generator().manual_seed(77)
    n, nnz, f = 3000, 90000, 64
    ei = torch.randint(0, n, (2, nnz), generator=g)
    ei[1, :500] = 11                                   # one long row
    pat = Pattern(ei.to(d), n, n)
    csr = pat.fwd
    xa, xb = torch.randn(n, f, generator=g).to(d), torch.randn(n, f, generator=g).to(d)
    va = pat.values_for(torch.randn(nnz, generator=g).to(d), "fwd")
    vb = pat.values_for(torch.randn(nnz, generator=g).to(d), "fwd")
    lib, P = _cabi.lib(), _cabi.ptr
    outs = []
    for hint in (0, 10 ** 9, 1, 1):                    # unknown -> light, huge -> deep, tiny -> rows per wavefront (x2)
        y1 = torch.empty(n, f, device=d)
        ya, yb = torch.empty(n, f, device=d), torch.empty(n, f, device=d)
        _cabi.check(lib.pygsd_spmm_csr_f32(P(csr.rowptr), P(csr.col), P(va), P(xa), f, P(y1), f, None, 0, n, f,
                                           1.0, 0.0, 0, hint, None, _cabi.stream_ptr()), "spmm")
        _cabi.check(lib.pygsd_spmm2_csr_f32(P(csr.rowptr), P(csr.col), P(va), P(vb), P(xa), P(xb), f, P(ya), P(yb),
                                            f, None, None, 0, n, f, 1.0, 0.0, hint, None, _cabi.stream_ptr()), "spmm2")
        outs.append((y1, ya, yb))
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)                      # light == deep, bitwise
    for a, b, c in zip(outs[0], outs[2], outs[3]):
        assert torch.equal(b, c)                      # rows per wavefront: run-to-run deterministic
        close(b, a)                                   # ... and equal to the lane-group order to fp32 rounding
    assert torch.equal(outs[0][0], outs[0][1])        # single == the a-half of the dual kernel


@pytest.mark.gpu
@pytest.mark.parametrize("f", [16, 64, 128, 320])
def test_hub_rows_take_the_segmented_path(f):
    """Rows with more than PYGSD_LONG_ROW entries (power-law hubs) are reduced in 4096-entry segments by
    spmm_long_kernel; everything else still goes through the row-per-wavefront kernel.  Checked against
    a float64 evaluation (sum order differs from the single-wavefront order, so tolerance not bit equality),
    for add / mean / alpha-beta-Z epilogues, single and dual operator, and for determinism."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, _spmm_raw, _spmm2_raw
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11 + f)
    n, base = 2000, 30000
    hub_sizes = {5: 4097, 77: 150000, 1999: 9000}        # just over the threshold, multi-segment, last row
    src = [torch.randint(0, n, (base,), generator=g)]
    dst = [torch.randint(0, n, (base,), generator=g)]
    for r, k in hub_sizes.items():
        src.append(torch.randint(0, n, (k,), generator=g))
        dst.append(torch.full((k,), r, dtype=torch.long))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    nnz = ei.size(1)
    wa, wb = torch.randn(nnz, generator=g), torch.randn(nnz, generator=g)
    xa, xb = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g)
    za, zb = torch.randn(n, f, generator=g), torch.randn(n, f, generator=g)
    pat = Pattern(ei.to(d), n, n)
    hubs = pat.fwd.hubs()
    assert hubs is not None and sorted(hubs[0].tolist()) == sorted(hub_sizes) and hubs[1] >= 150000
    assert pat.bwd.hubs() is None                        # the transposed orientation has no long row

    def dense(w):
        a = torch.zeros(n, n, dtype=torch.float64)
        a.index_put_((ei[1], ei[0]), w.double(), accumulate=True)
        return a

    A, B = dense(wa), dense(wb)
    va, vb = pat.values_for(wa.to(d), "fwd"), pat.values_for(wb.to(d), "fwd")
    scale = (A.abs() @ xa.double().abs()).clamp_min(1.0)  # per-entry magnitude of the summed terms

    def close(got, want, s=scale):
        err = ((got.double().cpu() - want).abs() / s).max().item()
        assert err < 2e-6, err

    y = _spmm_raw(pat.fwd, va, xa.to(d), None, 1.0, 0.0, False)
    close(y, A @ xa.double())
    assert torch.equal(y, _spmm_raw(pat.fwd, va, xa.to(d), None, 1.0, 0.0, False))        # deterministic
    y = _spmm_raw(pat.fwd, va, xa.to(d), za.to(d), 2.0, -1.0, False)
    close(y, 2.0 * (A @ xa.double()) - za.double())
    cnt = dense(torch.ones(nnz)).sum(1).clamp_min(1.0)
    y = _spmm_raw(pat.fwd, None, xa.to(d), None, 1.0, 0.0, True)
    close(y, (dense(torch.ones(nnz)) @ xa.double()) / cnt[:, None], torch.ones(n, f, dtype=torch.float64))
    ya, yb = _spmm2_raw(pat.fwd, va, vb, xa.to(d), xb.to(d), za.to(d), zb.to(d), 2.0, -1.0)
    close(ya, 2.0 * (A @ xa.double()) - za.double())
    close(yb, 2.0 * (B @ xb.double()) - zb.double(), (B.abs() @ xb.double().abs()).clamp_min(1.0))
    # rows that are not hubs are bit-identical to the plain launch (same kernel, same order)
    plain = torch.empty(n, f, device=d)
    lib, P = _cabi.lib(), _cabi.ptr
    _cabi.check(lib.pygsd_spmm_csr_f32(P(pat.fwd.rowptr), P(pat.fwd.col), P(va), P(xa.to(d)), f, P(plain), f, None, 0,
                                       n, f, 1.0, 0.0, 0, nnz, None, _cabi.stream_ptr()), "spmm")
    split = _spmm_raw(pat.fwd, va, xa.to(d), None, 1.0, 0.0, False)
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(hub_sizes)] = False
    assert torch.equal(plain[keep.to(d)], split[keep.to(d)])
    close(plain, A @ xa.double())


@pytest.mark.gpu
def test_hub_row_gradients_through_the_layer_api():
    """A hub in the forward orientation (many in-edges) and one in the backward orientation (many
    out-edges): autograd through spmm() matches the float64 dense product for both."""
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    n, f = 1500, 32
    src = torch.cat([torch.randint(0, n, (20000,), generator=g), torch.randint(0, n, (6000,), generator=g),
                     torch.full((7000,), 3, dtype=torch.long)])
    dst = torch.cat([torch.randint(0, n, (20000,), generator=g), torch.full((6000,), 9, dtype=torch.long),
                     torch.randint(0, n, (7000,), generator=g)])
    ei = torch.stack([src, dst])
    w = torch.rand(ei.size(1), generator=g)
    x = torch.randn(n, f, generator=g)
    pat = Pattern(ei.to(d), n, n)
    assert pat.fwd.hubs() is not None and pat.bwd.hubs() is not None
    xd = x.to(d).requires_grad_(True)
    wd = w.to(d).requires_grad_(True)
    out = spmm(pat, xd, wd)
    gout = torch.randn(n, f, generator=g)
    out.backward(gout.to(d))
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1], ei[0]), w.double(), accumulate=True)
    # float64 arbitrates between the HIP result and the reference's own fp32 op sequence (index_select -> mul ->
    # scatter_add_ over the 6000- / 7000-entry hub rows, oracle/ref_layers.py)
    from oracle import ref_layers as R
    x32, w32 = x.clone().requires_grad_(), w.clone().requires_grad_()
    ref = R.propagate(x32, ei, w32, n)
    ref.backward(gout)
    close_arbitrated(out, ref.detach(), A @ x.double(), what="hub rows: product")
    close_arbitrated(xd.grad, x32.grad, A.T @ gout.double(), what="hub rows: dX")
    gw = (gout.double()[ei[1]] * x.double()[ei[0]]).sum(1)
    close_arbitrated(wd.grad, w32.grad, gw, what="hub rows: d edge values")


@pytest.mark.gpu
def test_wide_dual_spmm_column_blocks_match_single_pass(monkeypatch):
    """_spmm2_raw splits F >= 128 into 64-column passes when the gathered set outgrows the Infinity Cache;
    forced here on a small graph: same result as one pass (to summation-order rounding), Z epilogue and
    strided operands included."""
    from pytorch_geometric_signed_directed_amd import sparse
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, _spmm2_raw
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    n, nnz, f = 3000, 60000, 192
    ei = torch.randint(0, n, (2, nnz), generator=g)
    pat = Pattern(ei.to(d), n, n)
    va = pat.values_for(torch.randn(nnz, generator=g).to(d), "fwd")
    vb = pat.values_for(torch.randn(nnz, generator=g).to(d), "fwd")
    packed = torch.randn(n, 2 * f, generator=g).to(d)          # the sharded path hands over column slices
    xa, xb = packed[:, :f], packed[:, f:]
    za, zb = torch.randn(n, f, generator=g).to(d), torch.randn(n, f, generator=g).to(d)
    one = _spmm2_raw(pat.fwd, va, vb, xa, xb, za, zb, 2.0, -1.0)
    monkeypatch.setattr(sparse, "_COLBLOCK_BYTES", 0)
    blocked = _spmm2_raw(pat.fwd, va, vb, xa, xb, za, zb, 2.0, -1.0)
    rows = torch.repeat_interleave(torch.arange(n), (pat.fwd.rowptr[1:] - pat.fwd.rowptr[:-1]).cpu().long())
    for k, (v, xk, zk) in enumerate(((va, xa, za), (vb, xb, zb))):
        dense = torch.zeros(n, n, dtype=torch.float64)
        dense.index_put_((rows, pat.fwd.col.cpu().long()), v.cpu().double(), accumulate=True)
        want = 2.0 * (dense @ xk.cpu().double()) - zk.cpu().double()
        # the column-blocked passes (16 lanes per gathered row) and the single pass (64 lanes) add a row's entries in
        # different orders: both are held to float64, the blocked one no further from it than 1.5x the single pass
        close(one[k], want, what=f"single-pass dual product {k} vs float64")
        close_arbitrated(blocked[k], one[k], want, what=f"column-blocked dual product {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("f", [1, 3, 64])
def test_gather_rows_backward_is_the_segment_sum(f):
    """sparse.gather_rows: forward = x[edge_index[row]]; backward (value-less SpMM over the [E, F] gradient through
    the edge list's CSR) = torch's index backward, for both rows, cached and one-off patterns."""
    from pytorch_geometric_signed_directed_amd.sparse import gather_rows
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(23)
    n, e = 700, 9000
    ei = torch.randint(0, n - 5, (2, e), generator=g).to(d)          # the last nodes are never indexed
    x = torch.randn(n, f, generator=g).to(d)
    w = torch.randn(e, f, generator=g).to(d)
    for row in (0, 1):
        for cached in (True, False):
            a = x.clone().requires_grad_()
            b = x.clone().requires_grad_()
            out = gather_rows(a, ei, row, cached)
            assert torch.equal(out, b[ei[row]])
            (out * w).sum().backward()
            (b[ei[row]] * w).sum().backward()
            t64 = torch.zeros(n, f, dtype=torch.float64, device=d).index_add_(0, ei[row], w.double())
            close_arbitrated(a.grad, b.grad, t64, what="gather_rows backward (segment sum)")
            assert float(a.grad[n - 5:].abs().sum()) == 0.0


@pytest.mark.gpu
def test_scalar_fallback_kernel_through_the_raw_abi():
    """The host pads odd widths to 16-byte rows, so spmm_scalar_kernel is only reached by raw C-ABI callers with
    unpadded / unaligned operands: it must still agree with the vector path (summation-order rounding only)."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, _spmm_raw
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(31)
    n, nnz, f = 2000, 40000, 5
    ei = torch.randint(0, n, (2, nnz), generator=g).to(d)
    pat = Pattern(ei, n, n)
    csr = pat.fwd
    x = torch.randn(n, f, generator=g).to(d)
    z = torch.randn(n, f, generator=g).to(d)
    v = pat.values_for(torch.randn(nnz, generator=g).to(d), "fwd")
    y = torch.empty(n, f, device=d)
    lib, P = _cabi.lib(), _cabi.ptr
    _cabi.check(lib.pygsd_spmm_csr_f32(P(csr.rowptr), P(csr.col), P(v), P(x), f, P(y), f, P(z), f, n, f, 2.0, -1.0, 0, nnz,
                                       None, _cabi.stream_ptr()), "spmm scalar")
    want = _spmm_raw(csr, v, x, z, 2.0, -1.0, False)          # padded -> vector kernel
    assert want.shape == (n, f)
    rows = torch.repeat_interleave(torch.arange(n, device=d), (csr.rowptr[1:] - csr.rowptr[:-1]).long())
    t64 = torch.zeros(n, f, dtype=torch.float64, device=d).index_add_(0, rows, v.double()[:, None] * x.double()[csr.col.long()])
    close_arbitrated(y, want, 2.0 * t64 - z.double(), what="scalar fallback kernel (float64 arbiter, vector kernel as the fp32 reference)")



@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", [(1, 0), (2, 0), (1001, 0), (1000, 1), (70001, 1), (5000000, 0)])
def test_id_range_kernel_exact(n, offset):
    """pygsd_id_range_i64 (node-id validation): min / max of an int64 list, 16-byte vector loads with an odd tail,
    unaligned lists (edge_index[1] of an odd-length edge list), several lists folded into one pair."""
    from pytorch_geometric_signed_directed_amd import _cabi
    g = torch.Generator().manual_seed(n + offset)
    base = torch.randint(-5, 1 << 40, (n + offset,), generator=g)
    base[(n + offset) // 2] = -7 if n > 1 else base[-1]
    ids = base.to(dev())[offset:]
    assert ids.data_ptr() % 16 == (8 * offset) % 16
    minmax = torch.tensor([(1 << 63) - 1, -(1 << 63)], dtype=torch.int64, device=dev())
    _cabi.check(_cabi.lib().pygsd_id_range_i64(_cabi.ptr(ids), n, _cabi.ptr(minmax), _cabi.stream_ptr()), "id_range")
    want = base[offset:]
    assert minmax.tolist() == [int(want.min()), int(want.max())]
    more = torch.tensor([1 << 50, -99], dtype=torch.int64, device=dev())
    _cabi.check(_cabi.lib().pygsd_id_range_i64(_cabi.ptr(more), 2, _cabi.ptr(minmax), _cabi.stream_ptr()), "id_range")
    assert minmax.tolist() == [min(int(want.min()), -99), max(int(want.max()), 1 << 50)]
    with pytest.raises(IndexError, match="outside"):
        _cabi.check_node_ids((10, torch.tensor([0, 9, 10], device=dev())))
    _cabi.check_node_ids((10, torch.tensor([0, 9], device=dev())), (3, None), (5, torch.empty(0, dtype=torch.long, device=dev())))



@pytest.mark.gpu
@pytest.mark.parametrize("f,deg", [(16, 3), (32, 5), (64, 4), (128, 2), (32, 20)])
def test_rows_per_wavefront_variant(f, deg):
    """spmm_packed_kernel (low-degree rows: every LPR-lane group owns its own row) against the float64 product, and
    against the one-wavefront-per-row kernel on the same inputs (both forced through PYGSD_SPMM_PACKED); single and
    dual operator, alpha / beta / Z epilogue, mean, empty rows, a row count that is not a multiple of the rows per
    wavefront.  Auto-selection (no env) must pick by entries per row and agree as well."""
    import os
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, _spmm2_raw, _spmm_raw
    d = dev()
    n_in, n_out = 3000, 2501
    ei = rand_graph(n_in, n_out, deg * n_out, 100 + f + deg, empty_tail=7)
    g = torch.Generator().manual_seed(f * deg)
    wa, wb = torch.randn(ei.size(1), generator=g), torch.randn(ei.size(1), generator=g)
    xa, xb = torch.randn(n_in, f, generator=g), torch.randn(n_in, f, generator=g)
    za, zb = torch.randn(n_out, f, generator=g), torch.randn(n_out, f, generator=g)
    pat = Pattern(ei.to(d), n_in, n_out)
    va, vb = pat.values_for(wa.to(d), "fwd"), pat.values_for(wb.to(d), "fwd")
    A = torch.zeros(n_out, n_in, dtype=torch.float64).index_put_((ei[1], ei[0]), wa.double(), accumulate=True)
    B = torch.zeros(n_out, n_in, dtype=torch.float64).index_put_((ei[1], ei[0]), wb.double(), accumulate=True)
    ones = torch.zeros(n_out, n_in, dtype=torch.float64).index_put_((ei[1], ei[0]), torch.ones(ei.size(1), dtype=torch.float64),
                                                                   accumulate=True)
    cnt = ones.sum(1).clamp_min(1.0)
    want = {"add": 2.0 * (A @ xa.double()) - za.double(), "mean": (ones @ xa.double()) / cnt[:, None],
            "dual_a": 0.5 * (A @ xa.double()) + za.double(), "dual_b": 0.5 * (B @ xb.double()) + zb.double()}
    results = {}
    try:
        for mode in ("0", "1", None):
            if mode is None:
                os.environ.pop("PYGSD_SPMM_PACKED", None)
            else:
                os.environ["PYGSD_SPMM_PACKED"] = mode
            ya, yb = _spmm2_raw(pat.fwd, va, vb, xa.to(d), xb.to(d), za.to(d), zb.to(d), 0.5, 1.0)
            results[mode] = {"add": _spmm_raw(pat.fwd, va, xa.to(d), za.to(d), 2.0, -1.0, False),
                             "mean": _spmm_raw(pat.fwd, None, xa.to(d), None, 1.0, 0.0, True), "dual_a": ya, "dual_b": yb}
    finally:
        os.environ.pop("PYGSD_SPMM_PACKED", None)
    for mode, res in results.items():
        for k, got in res.items():
            close(got, want[k], what=f"{k} (PYGSD_SPMM_PACKED={mode})")


@pytest.mark.gpu
@pytest.mark.parametrize("world,p_c,phases,f,dtype", [(8, 4, 2, 64, torch.float32), (4, 4, 1, 32, torch.float32),
                                                      (6, 2, 3, 16, torch.float32), (4, 1, 2, 24, torch.float32),
                                                      (8, 1, 1, 64, torch.bfloat16), (8, 2, 2, 32, torch.bfloat16)])
def test_pack_slices_kernel_equals_the_tensor_op_packing(world, p_c, phases, f, dtype):
    """pygsd_pack_slices (one launch for all phases, replicas and groups of a sharded propagate's send buffers)
    against PropagateEngine._pack, the tensor-op restatement the CPU tests run -- bit-exact (pure data movement)."""
    from pytorch_geometric_signed_directed_amd.parallel import PropagateEngine, ShardPlan
    chunks = 2 if p_c > 1 else 1
    plan = ShardPlan(1000, world, 1, align=PropagateEngine.alignment(world, p_c, phases, chunks))
    eng = PropagateEngine(plan, type("Ex", (), {"world_size": world, "rank": 1})(), p_c, phases, chunks)
    g = torch.Generator().manual_seed(world * f)
    wide = torch.randn(plan.n_pad, 2 * f + 8, generator=g).to(dev()).to(dtype)
    for xs in ([torch.randn(plan.n_pad, f, generator=g).to(dev()).to(dtype) for _ in range(2)],
               [wide[:, 8:8 + f], wide[:, 8 + f:8 + 2 * f]]):                      # contiguous groups; strided column views
        for c in range(phases):
            want = eng._pack(xs, c).clone()
            got = eng._pack_phase(xs, c)
            assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.gpu
def test_bf16_gather_with_fp32_partial_products():
    """pygsd_spmm_csr_bf16_acc_f32 through sparse.spmm_rows_into: bf16 features, float output accumulated over two
    column halves of the operator (Z = Y) and over row ranges, against the float64 product of the ROUNDED inputs --
    fp32-accurate (1e-5), i.e. no bf16 rounding of the partial sums."""
    from pytorch_geometric_signed_directed_amd.parallel import split_phases
    from pytorch_geometric_signed_directed_amd.sparse import Pattern, spmm_rows_into
    d = dev()
    n, f, world, n_pad = 1024, 64, 4, 256
    ei = rand_graph(n, n, 30000, 5)
    g = torch.Generator().manual_seed(9)
    w = torch.rand(ei.size(1), generator=g)
    x = torch.randn(n, f, generator=g).to(torch.bfloat16)
    pat = Pattern(ei.to(d), n, n)
    val = pat.values_for(w.to(d), "fwd")
    A = torch.zeros(n, n, dtype=torch.float64).index_put_((ei[1], ei[0]), w.double(), accumulate=True)
    want = 0.5 * (A @ x.double())
    blocks = split_phases(pat.fwd, (val,), n_pad, 2, world)
    y = torch.empty(n, f, dtype=torch.float32, device=d)
    xd = x.to(d)
    for c, (csr, (v,)) in enumerate(blocks):
        buf = xd.view(world, n_pad, f)[:, c * 128:(c + 1) * 128].reshape(world * 128, f).contiguous()
        for lo, hi in ((0, 500), (500, n)):
            spmm_rows_into(csr, v, buf, y, lo, hi, 0.5, c > 0)
    close(y, want, what="fp32 partial products of a bf16 gather")


# ------------------------------------------------------------------ fused operator build (csrc/magop.hip)
def _generic_operator(ei, w, n, signed, absdeg, q, norm, lam):
    from pytorch_geometric_signed_directed_amd.utils._laplacian import (assemble_operator_csr, laplacian_parts,
                                                                         laplacian_values)
    parts = laplacian_parts(ei, w, n, signed, absdeg)
    off_r, off_i, diag, mir_r, mir_i = laplacian_values(parts, q, norm, mirror=True)
    csr, vf, vb = assemble_operator_csr(parts, off_r, off_i, mir_r, mir_i, diag, lam, -1.0)
    return csr, vf, vb, parts.deg


def _assert_fused_equals_generic(ei, w, n, signed, absdeg, q, norm, lam):
    """The fused build(s) against the generic pipeline, bit for bit.  Without weights there are two fused pipelines -- the
    one-pass build behind the sort (pygsd_magop_unit, the default) and the two-stage one -- and both are held to it."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    wcsr, wvf, wvb, wdeg = _generic_operator(ei, w, n, signed, absdeg, q, norm, lam)
    csr = None
    for unit in ((True, False) if w is None else (True,)):
        prev = L.set_unit_build(unit)
        try:
            got = L.fused_operator_csr(ei, w, n, signed, absdeg, q, norm, lam)
        finally:
            L.set_unit_build(prev)
        assert got is not None
        csr, vf, vb, deg = got
        assert csr.nnz == wcsr.nnz
        assert torch.equal(csr.rowptr, wcsr.rowptr) and torch.equal(csr.col, wcsr.col)
        assert torch.equal(deg, wdeg)
        for a, b in zip(vf + vb, wvf + wvb):                 # same formulas in the same order: bit-identical
            assert torch.equal(a, b)
    return csr


@pytest.mark.gpu
@pytest.mark.parametrize("n,e,signed,absdeg,norm,weighted,lam", [
    (50, 300, False, True, "sym", True, 2.0), (50, 300, False, True, None, False, 3.5),
    (3000, 40000, False, True, "sym", True, 2.0), (3000, 40000, True, True, "sym", True, 2.0),
    (3000, 40000, True, False, "sym", True, 1.7), (3000, 40000, True, True, None, True, 2.0),
    (20000, 400000, False, True, "sym", False, 2.0), (1, 0, False, True, "sym", False, 2.0),
    (5, 0, False, True, None, True, 2.0)])
def test_fused_operator_build_is_bitwise_the_generic_pipeline(n, e, signed, absdeg, norm, weighted, lam):
    if e:
        ei, w = _messy_graph(n, e, seed=n + e, signed=signed)
    else:
        ei, w = torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    d = dev()
    _assert_fused_equals_generic(ei.to(d), w.to(d) if weighted else None, n, signed, absdeg, 0.2, norm, lam)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_fused_operator_build_long_rows_and_fallback(weighted):
    """Rows of 65..4096 symmetrised entries take the block-wide LDS sort; a longer one makes the fused build
    step aside (None) and the layer falls back to the generic pipeline."""
    from pytorch_geometric_signed_directed_amd.utils._laplacian import fused_operator_csr
    n = 6000
    g = torch.Generator().manual_seed(11)
    ei, w = _messy_graph(n, 30000, seed=5, signed=True)
    hubs = []
    for hub, k in ((7, 65), (8, 64), (100, 300), (2000, 2900), (n - 1, 1500)):     # out- and in-edges of the hubs
        other = torch.randint(0, n, (k,), generator=g)
        hubs.append(torch.stack([torch.full((k,), hub), other]))
        hubs.append(torch.stack([other[: k // 3], torch.full((k // 3,), hub)]))
    ei = torch.cat([ei] + hubs, dim=1)
    w = torch.cat([w, torch.rand(ei.size(1) - w.numel(), generator=g) - 0.3])
    d = dev()
    wd = w.to(d) if weighted else None
    csr = _assert_fused_equals_generic(ei.to(d), wd, n, True, True, 0.25, "sym", 2.0)
    lens = (csr.rowptr[1:] - csr.rowptr[:-1]).cpu()
    assert int(lens.max()) > 2048 and int((lens > 65).sum()) >= 4
    # exactly 64 entries (a full wavefront) and exactly 65 (the first row of the block path), with duplicates inside
    for k in (62, 63):
        star = torch.stack([torch.zeros(k + 2, dtype=torch.long), torch.cat([torch.arange(1, k + 1), torch.tensor([5, 9])])])
        sw = (torch.rand(k + 2, generator=g) + 0.5).to(d) if weighted else None
        scsr = _assert_fused_equals_generic(star.to(d), sw, 200, True, False, 0.1, None, 2.0)
        assert int(scsr.rowptr[1]) == k + 1
    # one node above the block limit: not handled here
    k = 4200
    big = torch.stack([torch.full((k,), 3), torch.arange(10, 10 + k)])
    ei2 = torch.cat([ei, big], dim=1).to(d)
    w2 = None if wd is None else torch.cat([wd, torch.ones(k, device=d)])
    assert fused_operator_csr(ei2, w2, n, True, True, 0.25, "sym", 2.0) is None
    # ... and the layer still builds the right operator through the generic pipeline
    from pytorch_geometric_signed_directed_amd.nn import MSConv
    conv = MSConv(4, 4, K=1, q=0.25, trainable_q=False, cached=True).to(d)
    x = torch.randn(n, 4, device=d)
    conv(x, x, ei2, w2)
    assert conv._operator.csr.nnz == _generic_operator(ei2, w2, n, True, True, 0.25, "sym", 2.0)[0].nnz


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bucket", "sort"])
@pytest.mark.parametrize("norm,lam", [("sym", 2.0), (None, 3.0)])
def test_unit_operator_build_long_rows_and_determinism(norm, lam, form, monkeypatch):
    """pygsd_magop_unit (unweighted graphs: merged rows parked as 8-byte records, written after the scan) in both its forms -- the
    stream split into LDS-sized row buckets (default) and the radix sort on the row bits: rows of 64 / 65 / 103 / 303 / 512 stream
    entries (from 65: the rank sort through LDS, direct stores), duplicates, reciprocal pairs, self loops, isolated nodes, a node
    count that is not a multiple of the 16 rows of a chunk -- bit-identical to the generic pipeline and from run to run (the bucket
    form places entries with LDS atomics: the order they arrive in must not show); 513 entries make it step aside."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    if form == "sort":
        monkeypatch.setenv("PYGSD_UNIT_BUILD_FORM", "sort")
    n = 50007
    g = torch.Generator().manual_seed(13)
    ei, _ = _messy_graph(n, 600000, seed=3, signed=False)
    ei = ei[:, (ei[0] < n - 40) & (ei[1] < n - 40)]                  # the last 40 nodes are isolated
    extra = []
    for hub, k, dup in ((7, 64, 0), (8, 65, 0), (9, 100, 3), (4000, 300, 3), (n - 50, 509, 3)):   # stream entries: k + dup
        drop = (ei[0] == hub) | (ei[1] == hub)
        ei = ei[:, ~drop]
        other = torch.randperm(n - 5000, generator=g)[:k] + 4500      # distinct neighbours, none of them a hub
        half = k // 2
        extra.append(torch.stack([torch.full((half,), hub), other[:half]]))               # out-edges
        extra.append(torch.stack([other[half:], torch.full((k - half,), hub)]))           # in-edges
        extra.append(torch.stack([torch.full((dup,), hub), other[:dup]]))                  # duplicates of some of them
    ei = torch.cat([ei] + extra, dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].to(dev())
    row, col = ei[0].contiguous(), ei[1].contiguous()
    sym = 1 if norm is not None else 0
    first = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, lam, -1.0)
    assert first is not None
    lens = (first[0].rowptr[1:] - first[0].rowptr[:-1]).cpu()
    assert [int(lens[k]) for k in (7, 8, 9, 4000, n - 50, n - 1)] == [65, 66, 101, 301, 510, 1]     # distinct entries + diagonal
    again = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, lam, -1.0)
    assert torch.equal(first[0].rowptr, again[0].rowptr) and torch.equal(first[0].col, again[0].col)
    for a, b in zip(first[1] + first[2], again[1] + again[2]):
        assert torch.equal(a, b)
    _assert_fused_equals_generic(ei, None, n, False, True, 0.25, norm, lam)
    over = torch.cat([ei, torch.stack([torch.full((1,), n - 50, device=dev()), torch.full((1,), 3, device=dev())])], dim=1)
    assert L._unit_operator_csr(over[0].contiguous(), over[1].contiguous(), over.size(1), n, sym, 0.25, lam, -1.0) is None
    assert L.fused_operator_csr(over, None, n, False, True, 0.25, norm, lam) is not None      # two-stage pipeline took it


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bucket", "sort"])
def test_unit_operator_build_degenerate_graphs(form, monkeypatch):
    """One node, two nodes, only self loops, one edge listed many times (multiplicity 40 in one record), a star whose centre is the
    last node, fewer nodes than the 16 rows of a write chunk or the 8 rows of the smallest bucket: both forms against the generic
    pipeline."""
    if form == "sort":
        monkeypatch.setenv("PYGSD_UNIT_BUILD_FORM", "sort")
    d = dev()
    cases = [
        (1, [[0], [0]]),
        (2, [[0, 1, 1], [1, 0, 1]]),
        (5, [[2, 3, 3], [2, 3, 3]]),                                       # self loops only: the identity-shaped operator
        (3, [[0] * 40 + [1] * 3, [2] * 40 + [0] * 3]),
        (9, [list(range(8)) + [8] * 8, [8] * 8 + list(range(8))]),
        (17, [[16, 0, 5], [0, 16, 5]]),
    ]
    for n, ei in cases:
        _assert_fused_equals_generic(torch.tensor(ei, device=d), None, n, False, True, 0.25, "sym", 2.0)
        _assert_fused_equals_generic(torch.tensor(ei, device=d), None, n, False, True, 0.1, None, 3.0)


@pytest.mark.gpu
def test_unit_operator_build_bucket_that_does_not_fit_lds(monkeypatch):
    """128 neighbouring rows of 300 entries each: 38 400 entries in one bucket of the bucket form (32 768 fit a workgroup's LDS) --
    it reports the graph as not taken and the two-stage pipeline builds the same operator; the sort form takes it (no row above
    512 entries)."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n = 200000
    g = torch.Generator().manual_seed(5)
    ei, _ = _messy_graph(n, 1500000, seed=11, signed=False)
    ei = ei[:, (ei[0] >= 2048) & (ei[1] >= 2048)]
    hubs = torch.arange(1024, 1152).repeat_interleave(300)
    others = torch.randint(4096, n, (hubs.numel(),), generator=g)
    ei = torch.cat([ei, torch.stack([hubs, others])], dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].to(dev())
    row, col = ei[0].contiguous(), ei[1].contiguous()
    assert L._unit_operator_csr(row, col, ei.size(1), n, 1, 0.25, 2.0, -1.0) is None
    _assert_fused_equals_generic(ei, None, n, False, True, 0.25, "sym", 2.0)
    monkeypatch.setenv("PYGSD_UNIT_BUILD_FORM", "sort")
    assert L._unit_operator_csr(row, col, ei.size(1), n, 1, 0.25, 2.0, -1.0) is not None
    _assert_fused_equals_generic(ei, None, n, False, True, 0.25, "sym", 2.0)


def _same_operator(got, want):
    csr, vf, vb, deg = got
    wcsr, wvf, wvb, wdeg = want
    assert csr.nnz == wcsr.nnz
    assert torch.equal(csr.rowptr, wcsr.rowptr) and torch.equal(csr.col, wcsr.col)
    assert torch.equal(deg, wdeg)
    for a, b in zip(vf + vb, wvf + wvb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # bit for bit (a -0.0 is not a 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("signed,absdeg,all_positive", [(True, True, False), (True, True, True), (True, False, True),
                                                        (False, True, True)])
@pytest.mark.parametrize("norm,lam", [("sym", 2.0), (None, 3.0)])
def test_signed_unit_operator_build_is_bitwise_the_generic_pipeline(signed, absdeg, all_positive, norm, lam):
    """pygsd_magop_unit_signed (round 5: weights of +-1 -- the signs of MSConv's graphs, get_magnetic_signed_Laplacian.py:52-90 --
    through the bucket build with one sign bit per entry): duplicates of mixed signs (runs of 3 .. 40 entries of one neighbour,
    A_s = 0 runs included), reciprocal pairs of equal and of opposite sign, self loops, isolated nodes, rows of 64 / 65 / 103 / 303 /
    512 stream entries (from 65: the rank sort through LDS) -- bit-identical to the generic pipeline and from run to run (LDS
    atomics place the entries: the arrival order must not show, which it cannot for sums of +-1).  Explicit all-ones weights take
    it under every degree convention."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n = 50007
    g = torch.Generator().manual_seed(17)
    ei, _ = _messy_graph(n, 600000, seed=3, signed=False)
    ei = ei[:, (ei[0] < n - 40) & (ei[1] < n - 40)]
    extra = [torch.tensor([[11] * 40 + [12] * 3 + [13] * 2, [2000] * 40 + [11] * 3 + [2001] * 2])]       # multiplicity 40 / 3 / 2
    for hub, k, dup in ((7, 64, 0), (8, 65, 0), (9, 100, 3), (4000, 300, 3), (n - 50, 509, 3)):
        drop = (ei[0] == hub) | (ei[1] == hub)
        ei = ei[:, ~drop]
        other = torch.randperm(n - 5000, generator=g)[:k] + 4500
        half = k // 2
        extra.append(torch.stack([torch.full((half,), hub), other[:half]]))
        extra.append(torch.stack([other[half:], torch.full((k - half,), hub)]))
        extra.append(torch.stack([torch.full((dup,), hub), other[:dup]]))
    ei = torch.cat([ei] + extra, dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    w = torch.ones(ei.size(1))
    if not all_positive:
        w = (torch.randint(0, 2, (ei.size(1),), generator=g) * 2 - 1).float()
    d = dev()
    ei, w = ei.to(d), w.to(d)
    row, col = ei[0].contiguous(), ei[1].contiguous()
    sym = 1 if norm is not None else 0
    first = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, lam, -1.0, w, signed, absdeg)
    assert first is not None
    lens = (first[0].rowptr[1:] - first[0].rowptr[:-1]).cpu()
    assert [int(lens[k]) for k in (7, 8, 9, 4000, n - 50, n - 1)] == [65, 66, 101, 301, 510, 1]
    again = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, lam, -1.0, w, signed, absdeg)
    _same_operator(again, first)
    _same_operator(first, _generic_operator(ei, w, n, signed, absdeg, 0.25, norm, lam))
    # the layer-facing entry takes the same route and hands back the same operator
    _same_operator(L.fused_operator_csr(ei, w, n, signed, absdeg, 0.25, norm, lam), first)
    prev = L.set_signed_unit_build(False)                            # ... as does the two-stage pipeline behind the switch
    try:
        _same_operator(L.fused_operator_csr(ei, w, n, signed, absdeg, 0.25, norm, lam), first)
    finally:
        L.set_signed_unit_build(prev)


@pytest.mark.gpu
def test_signed_unit_operator_build_steps_aside():
    """What pygsd_magop_unit_signed does not take is decided ON THE DEVICE (no host read of the weights) and reported like an
    over-long row: one weight that is not +-1, a NaN, a -1 under a degree convention that does not count |w|, a 513-entry row.  The
    layer-facing build then runs the two-stage pipeline (same operator as the generic one) and remembers the weight tensor, so the
    next build with the same tensor does not try again."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n = 20000
    d = dev()
    ei, _ = _messy_graph(n, 200000, seed=23, signed=False)
    g = torch.Generator().manual_seed(4)
    sign = (torch.randint(0, 2, (ei.size(1),), generator=g) * 2 - 1).float()
    loops = (ei[0] == ei[1]).nonzero().view(-1)
    plain = (ei[0] != ei[1]).nonzero().view(-1)
    ei = ei.to(d)
    row, col = ei[0].contiguous(), ei[1].contiguous()
    e = ei.size(1)
    ok = sign.clone()
    ok[loops] = 7.5                                                  # a self loop's weight is never read by the reference: dropped first
    assert L._unit_operator_csr(row, col, e, n, 1, 0.25, 2.0, -1.0, ok.to(d), True, True) is not None
    for bad_value in (0.5, 2.0, float("nan"), 0.0):
        w = sign.clone()
        w[plain[len(plain) // 2]] = bad_value
        assert L._unit_operator_csr(row, col, e, n, 1, 0.25, 2.0, -1.0, w.to(d), True, True) is None
    assert L._unit_operator_csr(row, col, e, n, 1, 0.25, 2.0, -1.0, sign.to(d), True, False) is None    # -1, degree of |A_s|
    assert L._unit_operator_csr(row, col, e, n, 1, 0.25, 2.0, -1.0, sign.to(d), False, True) is None    # -1, unsigned degree
    assert L._unit_operator_csr(row, col, e, n, 1, 0.25, 2.0, -1.0, sign.abs().to(d), False, True) is not None
    w = sign.clone()
    w[plain[3]] = 0.25
    wd = w.to(d)
    want = _generic_operator(ei, wd, n, True, True, 0.25, "sym", 2.0)
    assert L._NOT_PM1.get((wd,), (True, True)) is None
    _same_operator(L.fused_operator_csr(ei, wd, n, True, True, 0.25, "sym", 2.0), want)
    assert L._NOT_PM1.get((wd,), (True, True)) is True               # turned down once: remembered for this tensor / version
    _same_operator(L.fused_operator_csr(ei, wd, n, True, True, 0.25, "sym", 2.0), want)
    wd[int(plain[3])] = 1.0                                          # an in-place edit bumps the version: offered again, taken
    assert L._NOT_PM1.get((wd,), (True, True)) is None
    _same_operator(L.fused_operator_csr(ei, wd, n, True, True, 0.25, "sym", 2.0), _generic_operator(ei, wd, n, True, True, 0.25, "sym", 2.0))
    # a row of 513 stream entries
    k = 513
    star = torch.stack([torch.full((k,), 5), torch.arange(100, 100 + k)]).to(d)
    big = torch.cat([ei, star], dim=1)
    wb = torch.cat([sign.to(d), torch.ones(k, device=d)])
    assert L._unit_operator_csr(big[0].contiguous(), big[1].contiguous(), big.size(1), n, 1, 0.25, 2.0, -1.0, wb, True, True) is None
    _same_operator(L.fused_operator_csr(big, wb, n, True, True, 0.25, "sym", 2.0), _generic_operator(big, wb, n, True, True, 0.25, "sym", 2.0))


@pytest.mark.gpu
def test_signed_unit_operator_build_at_512_rows_per_bucket():
    """600 k nodes / 12 M signed edges: buckets of 512 rows (the north star's geometry) with the sign bit in the stream entry."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n, e = 600000, 12000000
    g = torch.Generator().manual_seed(31)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei = torch.cat([ei, ei[:, : e // 20].flip(0)], dim=1)            # reciprocal pairs, signs drawn independently
    w = (torch.randint(0, 2, (ei.size(1),), generator=g) * 2 - 1).float()
    d = dev()
    ei, w = ei.to(d), w.to(d)
    got = L._unit_operator_csr(ei[0].contiguous(), ei[1].contiguous(), ei.size(1), n, 1, 0.25, 2.0, -1.0, w, True, True)
    assert got is not None
    _same_operator(got, _generic_operator(ei, w, n, True, True, 0.25, "sym", 2.0))


def _weighted_graph(n, e, seed, signed, hubs=()):
    """Random weighted digraph whose symmetrised runs hold at most two entries (what the weighted bucket form takes): reciprocal
    pairs for one tenth of the edges, exact duplicates for ANOTHER twentieth, self loops, isolated last nodes; optional hub rows of
    exactly k stream entries."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 40, (e,), generator=g)
    dst = torch.randint(0, n - 40, (e,), generator=g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    # one entry per unordered pair, so that adding a reciprocal / a duplicate makes runs of exactly two
    key = torch.minimum(src, dst) * n + torch.maximum(src, dst)
    first = torch.unique(key, return_inverse=True)[1]
    order = torch.argsort(first, stable=True)
    uniq = torch.ones_like(first, dtype=torch.bool)
    uniq[order[1:]] = first[order[1:]] != first[order[:-1]]
    src, dst = src[uniq], dst[uniq]
    e = src.numel()
    for hub, _ in hubs:
        drop = (src == hub) | (dst == hub)
        src, dst = src[~drop], dst[~drop]
    e = src.numel()
    parts = [torch.stack([src, dst]), torch.stack([dst[:e // 10], src[:e // 10]]),
             torch.stack([src[e // 2:e // 2 + e // 20], dst[e // 2:e // 2 + e // 20]])]
    loops = torch.randint(0, n - 40, (e // 50 + 2,), generator=g)
    parts.append(torch.stack([loops, loops]))
    for hub, k in hubs:
        other = torch.randperm(n - 5000, generator=g)[:k] + 4500
        other = other[other != hub]
        half = other.numel() // 2
        parts.append(torch.stack([torch.full((half,), hub), other[:half]]))
        parts.append(torch.stack([other[half:], torch.full((other.numel() - half,), hub)]))
    ei = torch.cat(parts, dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    w = torch.rand(ei.size(1), generator=g) + 0.5
    if signed:
        w = w * (torch.randint(0, 2, (ei.size(1),), generator=g) * 2 - 1).float()
    return ei, w


@pytest.mark.gpu
@pytest.mark.parametrize("n,e,signed,absdeg,norm,lam", [(50007, 600000, False, True, "sym", 2.0), (50007, 600000, True, True, None, 3.0),
                                                        (50007, 600000, True, False, "sym", 1.7), (300, 2000, True, True, "sym", 2.0),
                                                        (600000, 9000000, True, True, "sym", 2.0)])
def test_weighted_bucket_operator_build_is_bitwise_the_generic_pipeline(n, e, signed, absdeg, norm, lam):
    """Round 5: real-valued weights through the bucket split (bucket_scatter_w / bucket_place_rows_w + the sorted pipeline's row kernels
    on the row-grouped 4-byte stream, in front of the unchanged second stage; get_magnetic_Laplacian.py:52-85, get_magnetic_signed_Laplacian.py:52-90 with edge weights) -- reciprocal pairs, exact
    duplicates (runs of two entries: fp32 addition commutes), self loops, isolated nodes, rows of 64 / 65 / 103 / 303 / 512 stream
    entries (from 65: the block-wide merge), every degree convention, both normalisations; 600 k nodes: buckets of
    512 rows in two rounds of 256.  Bit-identical to the generic pipeline and from run to run, and TAKEN (nothing was handed to the
    sorted pipeline)."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    hubs = ((7, 64), (8, 65), (9, 103), (4000, 303), (n - 50, 512)) if n == 50007 else ()
    ei, w = _weighted_graph(n, e, seed=n + e, signed=signed, hubs=hubs)
    d = dev()
    ei, w = ei.to(d), w.to(d)
    got = L.fused_operator_csr(ei, w, n, signed, absdeg, 0.25, norm, lam)
    assert got is not None
    assert L._NOT_BUCKETS.get((ei, w), (signed, absdeg)) is None      # the bucket form took the graph
    if hubs:
        lens = (got[0].rowptr[1:] - got[0].rowptr[:-1]).cpu()
        assert [int(lens[k]) for k in (7, 8, 9, 4000, n - 50, n - 1)] == [65, 66, 104, 304, 513, 1]
    _same_operator(L.fused_operator_csr(ei, w, n, signed, absdeg, 0.25, norm, lam), got)
    _same_operator(got, _generic_operator(ei, w, n, signed, absdeg, 0.25, norm, lam))


@pytest.mark.gpu
def test_weighted_bucket_operator_build_steps_aside(monkeypatch):
    """What the weighted bucket form must not decide on its own goes to the sorted pipeline and still matches the generic one: an
    edge listed three times (its fp32 sum depends on the order: the reference's is the list order), a reciprocal pair with a
    duplicate -- also inside a row of more than 64 entries (the block-wide merge); the pair of tensors is remembered, and
    PYGSD_WEIGHTED_BUILD_FORM=sort never tries.  Hub rows are NOT a reason any more: up to 4096 entries they are merged by the
    sorted pipeline's block kernel reading the row-grouped stream; beyond that no fused form takes the graph."""
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n = 50007
    d = dev()
    ei, w = _weighted_graph(n, 300000, seed=77, signed=True)
    g = torch.Generator().manual_seed(8)
    hub_with_triple = torch.cat([torch.stack([torch.full((300,), 5), torch.arange(100, 400)]), torch.tensor([[5, 5], [100, 100]])], dim=1)
    for extra in (torch.tensor([[3, 3, 3], [9, 9, 9]]), torch.tensor([[20, 21, 20], [21, 20, 21]]), hub_with_triple):
        ei2 = torch.cat([ei, extra], dim=1).to(d)
        w2 = torch.cat([w, torch.rand(extra.size(1), generator=g) + 0.5]).to(d)
        want = _generic_operator(ei2, w2, n, True, True, 0.25, "sym", 2.0)
        assert L._NOT_BUCKETS.get((ei2, w2), (True, True)) is None
        _same_operator(L.fused_operator_csr(ei2, w2, n, True, True, 0.25, "sym", 2.0), want)
        assert L._NOT_BUCKETS.get((ei2, w2), (True, True)) is True
        _same_operator(L.fused_operator_csr(ei2, w2, n, True, True, 0.25, "sym", 2.0), want)
    for k, taken in ((513, True), (4000, True), (4200, False)):
        star = torch.stack([torch.full((k,), 6), torch.arange(100, 100 + k)])
        ei2 = torch.cat([ei, star], dim=1).to(d)
        w2 = torch.cat([w, torch.rand(k, generator=g) + 0.5]).to(d)
        got = L.fused_operator_csr(ei2, w2, n, True, True, 0.25, "sym", 2.0)
        if taken:
            assert L._NOT_BUCKETS.get((ei2, w2), (True, True)) is None
            _same_operator(got, _generic_operator(ei2, w2, n, True, True, 0.25, "sym", 2.0))
        else:
            assert got is None                                       # the layers then take the generic pipeline
    monkeypatch.setenv("PYGSD_WEIGHTED_BUILD_FORM", "sort")
    eid, wd = ei.to(d), w.to(d)
    _same_operator(L.fused_operator_csr(eid, wd, n, True, True, 0.25, "sym", 2.0), _generic_operator(eid, wd, n, True, True, 0.25, "sym", 2.0))


@pytest.mark.gpu
def test_unit_operator_build_forms_agree_at_512_rows_per_bucket():
    """600 k nodes: buckets of 512 rows, 20 k entries each (the geometry of the north star) -- the two forms of the unweighted build
    give the same arrays bit for bit, with and without the normalisation."""
    import os
    from pytorch_geometric_signed_directed_amd.utils import _laplacian as L
    n = 600000
    ei, _ = _messy_graph(n, 10000000, seed=21, signed=False)
    ei = ei.to(dev())
    row, col = ei[0].contiguous(), ei[1].contiguous()
    for sym in (1, 0):
        a = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, 2.0, -1.0)
        os.environ["PYGSD_UNIT_BUILD_FORM"] = "sort"
        try:
            b = L._unit_operator_csr(row, col, ei.size(1), n, sym, 0.25, 2.0, -1.0)
        finally:
            del os.environ["PYGSD_UNIT_BUILD_FORM"]
        assert a is not None and b is not None and a[0].nnz == b[0].nnz
        assert torch.equal(a[0].rowptr, b[0].rowptr) and torch.equal(a[0].col, b[0].col) and torch.equal(a[3], b[3])
        for x, y in zip(a[1] + a[2], b[1] + b[2]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.gpu
def test_fused_operator_build_rejects_bad_ids_and_wide_id_keys():
    from pytorch_geometric_signed_directed_amd.utils._laplacian import fused_operator_csr
    d = dev()
    ei = torch.tensor([[0, 1, 2], [1, 2, 7]], device=d)
    with pytest.raises(IndexError, match="node id 7"):
        fused_operator_csr(ei, None, 5, False, True, 0.25, "sym", 2.0)
    with pytest.raises(IndexError, match="node id -1"):
        fused_operator_csr(torch.tensor([[0, -1], [1, 2]], device=d), None, 5, False, True, 0.25, "sym", 2.0)
    # more than 2^25 nodes: the in-register sort runs on 64-bit keys
    n = (1 << 25) + 5
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, n, (20000,), generator=g)
    dst = torch.randint(0, n, (20000,), generator=g)
    src = torch.cat([src, torch.full((50,), n - 1), dst[:500]])       # a 50-entry row at the top id, reciprocal pairs
    dst = torch.cat([dst, torch.randint(0, n, (50,), generator=g), src[:500]])
    _assert_fused_equals_generic(torch.stack([src, dst]).to(d), None, n, False, True, 0.25, "sym", 2.0)


@pytest.mark.gpu
def test_fused_operator_reference_format_matches_generic():
    """cached_result (the reference's 4-tuple, MagNetConv.py:100-120) read off the fused operator's CSR equals the
    one the generic pipeline assembles from its COO intermediates."""
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv
    from pytorch_geometric_signed_directed_amd.nn import _magnetic
    d = dev()
    ei, w = _messy_graph(500, 6000, seed=9, signed=False)
    x = torch.randn(500, 8, device=d)
    outs = []
    for fused in (True, False):
        prev = _magnetic.set_fused_build(fused)
        try:
            torch.manual_seed(0)
            conv = MagNetConv(8, 8, K=2, q=0.2, trainable_q=False, cached=True).to(d)
            o = conv(x, x, ei.to(d), w.to(d), lambda_max=2.5)
            outs.append((conv.cached_result, o, conv._operator._off_index is None or fused))
        finally:
            _magnetic.set_fused_build(prev)
    (fa, oa, _), (fb, ob, _) = outs
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1])


@pytest.mark.gpu
@pytest.mark.parametrize("k,shape", [(1, (5, 4)), (3, (1000, 64)), (8, (333, 12))])
def test_weighted_sum_kernel(k, shape):
    """sum_j w[j] * x[j] in one pass (SIMPA / DIMPA hop accumulations) against float64."""
    from pytorch_geometric_signed_directed_amd.nn.signed.SIMPA import weighted_sum
    g = torch.Generator().manual_seed(k)
    xs = [torch.randn(shape, generator=g) for _ in range(k)]
    ws = [float(v) for v in torch.randn(k, generator=g)]
    want = sum(w * x.double() for w, x in zip(ws, xs))
    close(weighted_sum([x.to(dev()) for x in xs], ws), want, 1e-6)
    wide = torch.full((shape[0], 2 * shape[1] + 4), 7.0, device=dev())           # into a column block of a wider matrix
    weighted_sum([x.to(dev()) for x in xs], ws, wide[:, shape[1]:2 * shape[1]])
    close(wide[:, shape[1]:2 * shape[1]], want, 1e-6)
    assert bool((wide[:, :shape[1]] == 7.0).all()) and bool((wide[:, 2 * shape[1]:] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("k,shape", [(1, (5, 4)), (3, (100000, 64)), (8, (333, 12))])
def test_dots_kernel(k, shape):
    """<g, x_j> for all j in one pass over g (the gradients of SIMPA's hop weights) against float64; a reduction over all
    N F elements: max-norm bar."""
    from pytorch_geometric_signed_directed_amd.nn.signed.SIMPA import dots
    g = torch.Generator().manual_seed(k)
    gg = torch.randn(shape, generator=g)
    xs = [torch.randn(shape, generator=g) + (0.5 - 0.2 * j) * gg for j in range(k)]    # correlated: the sums do not cancel
    want = torch.stack([(gg.double() * x.double()).sum() for x in xs])
    got = dots(gg.to(dev()), [x.to(dev()) for x in xs])
    close(got, want, TOL, norm=True, what="dots")
    assert torch.equal(dots(gg.to(dev()), [x.to(dev()) for x in xs]), got)       # deterministic


# ------------------------------------------------------------------ tall linear maps (csrc/tall.hip)
TALL_CASES = [
    # (dtype, rows, segment widths, f_out, transposed W, bias, segments are column slices of a wider matrix)
    ("f32", 1000, (64,), 192, False, True, False),       # DiGCN inception block forward, fp32
    ("f32", 777, (64, 128), 64, True, False, True),      # its input gradient [g0 | dP] W^T (rows not a multiple of 16)
    ("f32", 50, (64,), 256, False, True, False),         # SGCNConv layer 1: [own_b | own_u | a_pos | a_neg]
    ("f32", 4099, (128, 128), 64, True, False, False),   # its input gradient, K = 256
    ("f32", 33, (16,), 16, False, True, False),          # the smallest shape
    ("f32", 300, (32, 64), 96, False, False, True),
    ("bf16", 1000, (64,), 192, False, True, False),      # C5: bf16 inception block forward
    ("bf16", 777, (64, 128), 64, True, False, True),     # C5: its input gradient
    ("bf16", 4099, (128, 64, 64), 64, True, False, False),
    ("bf16", 17, (32,), 32, False, True, False),
    ("bf16", 513, (256,), 128, False, True, False),
]


@pytest.mark.parametrize("dtype,n,widths,f_out,transposed,with_bias,sliced", TALL_CASES)
def test_tall_product_matches_float64(dtype, n, widths, f_out, transposed, with_bias, sliced):
    """[X_0 | X_1 | ...] W (+ bias) in one pass on the matrix cores against float64 on the SAME (already rounded) inputs.
    W is asymmetric and every output column has its own scale, so a transposed or permuted C/D write cannot pass.
    fp32: the 1e-5 bar; bf16 storage: the result is the fp32-accumulated product rounded once (half an ulp, 2^-8)."""
    from pytorch_geometric_signed_directed_amd.dense import set_tall_kernels, tall_product
    from pytorch_geometric_signed_directed_amd import _cabi
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    k = sum(widths)
    assert _cabi.lib().pygsd_tall_linear_supported(0 if dtype == "f32" else 1, k, f_out) == 1
    g = torch.Generator().manual_seed(n + k + f_out)
    scale = torch.linspace(0.25, 2.0, f_out)
    w = (torch.randn(k, f_out, generator=g) / k ** 0.5 * scale).to(td)
    if sliced:          # segments are column ranges of one wider row-major matrix (row stride != width)
        wide = torch.randn(n, k + 32, generator=g).to(td).to(dev())
        segs, at = [], 0
        for wd in widths:
            segs.append(wide[:, at:at + wd])
            at += wd
    else:
        segs = [torch.randn(n, wd, generator=g).to(td).to(dev()) for wd in widths]
    bias = torch.randn(f_out, generator=g).to(td) if with_bias else None
    wdev = (w.t().contiguous() if transposed else w).to(dev())
    got = tall_product(segs, wdev, transposed, None if bias is None else bias.to(dev()))
    assert got.dtype == td and got.shape == (n, f_out)
    want = torch.cat([s.double().cpu() for s in segs], dim=1) @ w.double()
    if bias is not None:
        want = want + bias.double()
    if dtype == "f32":
        close(got, want, TOL, what="tall product fp32")
    else:
        close(got, want, 2.0 ** -8, what="tall product bf16 (one rounding of the fp32 sum)")
    prev = set_tall_kernels(False)      # the library route computes the same thing
    try:
        lib = tall_product(segs, wdev, transposed, None if bias is None else bias.to(dev()))
    finally:
        set_tall_kernels(prev)
    # (bf16: the library route rounds to bf16 once per segment it accumulates, the kernel once in total)
    close(lib, want, TOL if dtype == "f32" else 2.0 ** -7 * (1 + len(widths)), what="library route")


SPLIT_CASES = [
    # (rows, segment widths, f_out, transposed W, bias, output splits, wide-range magnitudes)
    (1, (64,), 64, False, True, None, False),                  # one row: fifteen clamped lanes re-write it
    (15, (64, 64), 64, True, False, None, False),
    (17, (32,), 32, False, True, None, False),                 # the smallest split shape, a ragged second tile
    (4099, (128,), 64, True, False, None, True),               # C3a's input gradient shape, magnitudes over 2^-16 .. 2^15
    (70001, (64,), 128, False, True, (64, 64), False),         # C3a forward: two output matrices
    (20000, (64, 64, 64), 64, True, False, None, False),       # C5a's input gradient [dx0 | dP_1 | dP_2] W^T
    (20000, (64,), 192, False, True, (64, 64, 64), True),      # C5a forward: three output matrices
    (513, (256,), 64, False, False, None, False),              # K = 256: eight k-blocks, 16 KB of row buffers per wavefront
    (1000, (64,), 64, False, True, (16, 48), False),           # output matrices that cut a stored pair of 16-column tiles apart
    (1000, (32, 32), 96, True, False, (48, 16, 32), False),
]


@pytest.mark.parametrize("n,widths,f_out,transposed,with_bias,splits,wide", SPLIT_CASES)
def test_tall_product_fp32_split_form_against_exact_form_and_float64(n, widths, f_out, transposed, with_bias, splits, wide):
    """The default fp32 form of pygsd_tall_linear (three-way bf16 splitting on the bf16 matrix pipe, include/pygsd_hip.h) next
    to the exact form (an fmaf chain per output) on the same inputs, both against float64 relative to sum |x| |w| per output --
    the natural scale of a dot product's rounding error.  The split form must be inside the 1e-5 bar AND no further from float64
    than 1.25x the exact form's own worst error (measured: 0.4 - 0.8x of it), on inputs of one magnitude and on inputs whose
    magnitudes span 2^31; ragged row counts exercise its clamped (unmasked) last tile."""
    from pytorch_geometric_signed_directed_amd.dense import set_tall_f32_exact, tall_product
    k = sum(widths)
    g = torch.Generator().manual_seed(n + k + f_out)
    w = torch.randn(k, f_out, generator=g) / k ** 0.5
    segs = [torch.randn(n, wd, generator=g) for wd in widths]
    if wide:
        segs = [t * torch.exp2(torch.randint(-16, 16, t.shape, generator=g).float()) for t in segs]
        w = w * torch.exp2(torch.randint(-8, 8, w.shape, generator=g).float())
    bias = torch.randn(f_out, generator=g) if with_bias else None
    x64 = torch.cat([t.double() for t in segs], dim=1)
    want = x64 @ w.double()
    scale = x64.abs() @ w.double().abs()
    if bias is not None:
        want = want + bias.double()
        scale = scale + bias.double().abs()
    segs_d = [t.to(dev()) for t in segs]
    wdev = (w.t().contiguous() if transposed else w).to(dev())
    bdev = None if bias is None else bias.to(dev())

    def run():
        out = tall_product(segs_d, wdev, transposed, bdev, splits=splits)
        return torch.cat([o.cpu() for o in out], dim=1) if splits is not None else out.cpu()

    prev = set_tall_f32_exact(False)
    try:
        split = run()
        assert torch.equal(run(), split)                       # deterministic
        set_tall_f32_exact(True)
        exact = run()
    finally:
        set_tall_f32_exact(prev)
    assert split.shape == (n, f_out) and not torch.equal(split, exact)     # (two forms really ran)
    err_split = float(((split.double() - want).abs() / scale).max())
    err_exact = float(((exact.double() - want).abs() / scale).max())
    if not wide:        # (with magnitudes spanning 2^31 the sums cancel: only the scale-relative error says anything, for either form)
        close(split, want, TOL, what="split form")
        close(exact, want, TOL, what="exact form")
    assert err_split <= max(1.25 * err_exact, 2.0 ** -23), (err_split, err_exact)
    assert err_split < (1e-6 if wide else 4e-7), err_split


@pytest.mark.parametrize("dtype,n,f,sliced", [("f32", 1000, 64, False), ("f32", 5, 4, False), ("f32", 70001, 192, True),
                                              ("bf16", 1000, 64, False), ("bf16", 70001, 128, True), ("bf16", 3, 8, False)])
def test_column_sums_match_float64(dtype, n, f, sliced):
    """Bias gradients: column sums accumulated in fp32 in a fixed order, against float64 (max-norm bar: a reduction over
    the rows, tests/tolerance.py)."""
    from pytorch_geometric_signed_directed_amd.dense import column_sums, column_sums_of
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(n + f)
    x = (torch.randn(n, f + (16 if sliced else 0), generator=g) + 0.25).to(td).to(dev())
    view = x[:, 8:8 + f] if sliced else x
    got = column_sums(view)
    assert got.dtype == td and got.shape == (f,)
    want = view.double().sum(0)
    close(got, want, TOL if dtype == "f32" else 2.0 ** -8, norm=True, what="column sums")
    assert torch.equal(column_sums(view), got)                                   # deterministic
    a, b, c = column_sums_of([view, None, view])
    assert b is None and a is c
    row = torch.randn(1, f, generator=g).to(td).to(dev())
    close(column_sums(row.expand(n, f)), row[0].double() * n, 2.0 ** -8 if dtype == "bf16" else TOL, norm=True,
          what="column sums of a broadcast row")


def test_tall_linear_autograd_matches_float64():
    """tall_linear (forward, dX through the transposed product, dW split-K, db column sums) against float64 autograd."""
    from pytorch_geometric_signed_directed_amd.dense import tall_linear
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5000, 64, generator=g)
    w = torch.randn(64, 128, generator=g) / 8
    b = torch.randn(128, generator=g)
    gy = torch.randn(5000, 128, generator=g)
    xd, wd, bd = (t.to(dev()).requires_grad_() for t in (x, w, b))
    y = tall_linear(xd, wd, bd)
    y.backward(gy.to(dev()))
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    (x64 @ w64 + b64).backward(gy.double())
    close(y, x64 @ w64 + b64, TOL, what="tall_linear forward")
    close(xd.grad, x64.grad, TOL, what="tall_linear dX")
    close(wd.grad, w64.grad, TOL, norm=True, what="tall_linear dW")
    close(bd.grad, b64.grad, TOL, norm=True, what="tall_linear db")


# ------------------------------------------------------------------ weight gradients of the tall maps (csrc/gram.hip), generic GEMM
GRAM_CASES = [
    # dtype, rows, X segment widths, G segment widths, column slices of wider matrices
    ("f32", 70001, (64,), (64, 64), False),            # C3 SGCNConv: x^T [g | g_a]
    ("f32", 1000, (64,), (64, 128), True),             # fp32 inception block: x^T [dx0 | dP_1 | dP_2]
    ("f32", 1, (16,), (16,), False),
    ("f32", 37, (32, 16), (16, 128, 48), False),       # every chunk size on both sides, ragged tail
    ("f32", 5000, (128,), (32,), True),
    ("f32", 40003, (128,), (64, 64, 64), False),       # round 5's 32x32 form: 4 X blocks against 6 G blocks (two groups of 3)
    ("f32", 999, (32,), (160,), True),                 # 1 x 5 blocks -> 4 + 1
    ("f32", 4097, (96,), (96, 32), False),             # 3 X blocks: 2 + 1; a ragged last batch of row pairs
    ("f32", 15, (64, 64), (192,), False),              # fewer rows than one batch
    ("f32", 300000, (64,), (64, 64, 64), False),       # the inception block's shape, enough rows for every wavefront
    ("bf16", 70001, (64,), (64, 128), False),          # C5: bf16 inception block
    ("bf16", 1, (16,), (16,), False),
    ("bf16", 33, (32, 16), (16, 128, 48), True),       # a partial 32-row tile
    ("bf16", 4099, (64, 64), (192,), False),
    ("bf16", 1000, (16,), (32,), True),
    # round 6: neighbouring whole segments of one width ride in ONE chunk (two parts fp32, up to three bf16)
    ("bf16", 70001, (64,), (64, 64, 64), False),       # C5b: x^T [dx0 | dP_1 | dP_2], 12 tiles against 4: every row read once
    ("bf16", 5000, (64,), (64, 64, 64), True),         # the same as column slices of one wider matrix
    ("bf16", 4099, (32, 32), (32, 32, 16, 16, 16), False),   # pairs of 2 and of 1 tiles, a third 16 left alone
    ("f32", 5000, (64,), (64, 64), True),              # C3a's pair as column slices
    ("f32", 3001, (16, 48), (32, 32, 64, 64, 16), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n,xw,gw,sliced", [c for c in GRAM_CASES if c[0] == "f32" and all(w % 32 == 0 for w in c[2] + c[3])])
def test_tall_gram_32x32_form_matches_float64(dtype, n, xw, gw, sliced, monkeypatch):
    """Round 5's form of the fp32 weight-gradient product (v_mfma_f32_32x32x2_f32 with both operands straight from coalesced
    loads, a wavefront holding the whole output block) forced on for every shape whose segments are multiples of 32 columns --
    by default it only runs where it measured faster (>= 10 accumulator blocks per wavefront)."""
    from pytorch_geometric_signed_directed_amd.dense import set_tall_f32_exact
    monkeypatch.setenv("PYGSD_GRAM_32X32", "1")
    for exact in (False, True):     # its split form (three bf16 pieces per value on v_mfma_f32_32x32x16_bf16, the default) and the exact one
        prev = set_tall_f32_exact(exact)
        try:
            test_tall_gram_matches_float64(dtype, n, xw, gw, sliced)
        finally:
            set_tall_f32_exact(prev)
    monkeypatch.setenv("PYGSD_GRAM_32X32", "0")
    test_tall_gram_matches_float64(dtype, n, xw, gw, sliced)


@pytest.mark.gpu
@pytest.mark.parametrize("n,xw,gw", [(70001, (64,), (64, 64, 64)), (4099, (64,), (128,)), (17, (32,), (32,))])
def test_tall_gram_split_form_against_exact_form_and_float64(n, xw, gw, monkeypatch):
    """The 32x32 weight-gradient kernel's two arithmetic forms on the same inputs against float64, relative to sum |x| |g| per
    output: the split form no further from float64 than 2x the exact form's own worst error (a reduction over all rows: both sit
    at 1e-8 of the scale and below)."""
    from pytorch_geometric_signed_directed_amd.dense import set_tall_f32_exact, tall_gram
    monkeypatch.setenv("PYGSD_GRAM_32X32", "1")
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, sum(xw), generator=g).to(dev())
    gg = torch.randn(n, sum(gw), generator=g).to(dev())
    xs = list(x.split(list(xw), dim=1))
    gs = [t.contiguous() for t in gg.split(list(gw), dim=1)]
    want = x.double().t() @ gg.double()
    scale = x.double().abs().t() @ gg.double().abs()
    errs = {}
    for exact in (False, True):
        prev = set_tall_f32_exact(exact)
        try:
            got = tall_gram(xs, gs)
        finally:
            set_tall_f32_exact(prev)
        close(got, want, TOL, norm=True, what="tall_gram")
        errs[exact] = (got, float(((got.double() - want).abs() / scale).max()))
    assert not torch.equal(errs[False][0], errs[True][0])            # (two forms really ran)
    assert errs[False][1] <= max(2.0 * errs[True][1], 2.0 ** -23), (errs[False][1], errs[True][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n,xw,gw,sliced", GRAM_CASES)
def test_tall_gram_matches_float64(dtype, n, xw, gw, sliced):
    """[X_0 | ...]^T [G_0 | ...] (dW = x^T dY of the tall linear maps; autograd's mm backward for DiGCNConv.py:66,
    DiGCN_Inception_Block.py:44-46, SGCNConv.py:121-126) against float64 on the same (already rounded) inputs.  Every
    column of either operand has its own scale and the operands differ, so a transposed, permuted or mis-chunked result
    cannot pass.  Row reductions: the max-norm bar, float64 arbitrating against the plain fp32 product x^T g."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.dense import tall_gram
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(n + sum(xw) * 7 + sum(gw))

    def make(widths, lo, hi):
        total = sum(widths)
        scale = torch.linspace(lo, hi, total)
        if sliced:
            wide = (torch.randn(n, total + 16, generator=g) * torch.cat([scale, torch.ones(16)])).to(td).to(dev())
            segs, at = [], 0
            for wd in widths:
                segs.append(wide[:, at:at + wd])
                at += wd
            return segs
        full = (torch.randn(n, total, generator=g) * scale).to(td)
        return [full[:, a:a + wd].contiguous().to(dev()) for a, wd in zip(np.cumsum((0,) + widths[:-1]), widths)]

    xs, gs = make(xw, 0.5, 1.5), make(gw, 0.25, 2.0)
    _cabi.reset_library_routes()
    got = tall_gram(xs, gs)
    assert _cabi.library_routes() == {}, _cabi.library_routes()
    assert got.dtype == td and got.shape == (sum(xw), sum(gw))
    x64 = torch.cat([t.double() for t in xs], dim=1)
    g64 = torch.cat([t.double() for t in gs], dim=1)
    want = x64.t() @ g64
    ref32 = x64.float().t() @ g64.float()
    if dtype == "f32":
        close_arbitrated(got, ref32, want, norm=True, what="tall gram fp32")
    else:
        # fp32 accumulation of exact bf16 products, rounded to bf16 once: half an ulp of the result's scale
        close(got.float(), want, 2.0 ** -8, norm=True, what="tall gram bf16 (one rounding of the fp32 sum)")
    again = tall_gram(xs, gs)
    assert torch.equal(again, got)                      # fixed summation order: run-to-run deterministic


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,ta,tb,bias,acc", [(1000, 10, 2879, False, False, True, False),     # C1: x W at the raw width
                                                    (2879, 16, 3000, True, False, False, False),     # C1: dW = x^T g (split)
                                                    (64, 10, 100000, True, False, False, False),      # a deep split reduction
                                                    (300, 2879, 16, False, True, False, False),       # C1: dx = g W^T
                                                    (5, 3, 7, False, False, True, True),
                                                    (129, 65, 33, True, True, True, True),
                                                    (70001, 5, 128, False, False, False, False)])     # a 5-class read-out
def test_generic_gemm_matches_float64(m, n, k, ta, tb, bias, acc):
    """pygsd_gemm_f32 (the catch-all behind the MFMA kernels) for odd shapes, transposed views, bias, accumulation and the
    split reduction, against float64; float64 arbitrates against torch's own fp32 product."""
    from pytorch_geometric_signed_directed_amd.dense import gemm
    g = torch.Generator().manual_seed(m + 3 * n + 5 * k)
    scale = torch.linspace(0.5, 1.5, k)                              # column scales: a transposed operand cannot pass
    a = ((torch.randn(k, m, generator=g) * scale[:, None]).to(dev()).t() if ta
         else (torch.randn(m, k, generator=g) * scale).to(dev()))
    b = (torch.randn(n, k, generator=g).to(dev()).t() if tb else torch.randn(k, n, generator=g).to(dev()))
    assert a.shape == (m, k) and b.shape == (k, n) and (a.stride(0) == 1) == (ta and m > 1) and (b.stride(1) != 1) == (tb and k > 1)
    bv = torch.randn(n, generator=g).to(dev()) if bias else None
    c0 = torch.randn(m, n, generator=g).to(dev()) if acc else None
    got = gemm(a, b, bias=bv, out=None if c0 is None else c0.clone(), accumulate=acc)
    want = a.double() @ b.double()
    ref32 = a @ b
    if bias:
        want, ref32 = want + bv.double(), ref32 + bv
    if acc:
        want, ref32 = want + c0.double(), ref32 + c0
    close_arbitrated(got, ref32, want, norm=k >= 2048, what=f"generic gemm {m}x{n}x{k}")
    assert torch.equal(gemm(a, b, bias=bv, out=None if c0 is None else c0.clone(), accumulate=acc), got)


@pytest.mark.gpu
def test_hip_matmul_is_differentiable():
    from pytorch_geometric_signed_directed_amd.dense import matmul
    g = torch.Generator().manual_seed(77)
    a0, b0, go = torch.randn(5000, 7, generator=g), torch.randn(7, 5, generator=g), torch.randn(5000, 5, generator=g)
    a, b = a0.to(dev()).requires_grad_(), b0.to(dev()).requires_grad_()
    (matmul(a, b) * go.to(dev())).sum().backward()
    a64, b64 = a0.double().requires_grad_(), b0.double().requires_grad_()
    ((a64 @ b64) * go.double()).sum().backward()
    close(a.grad, a64.grad, what="d a")
    close(b.grad, b64.grad, norm=True, what="d b (a reduction over the rows)")
    pt = a0.to(dev()).t().requires_grad_()                          # a transposed view as the left operand: P^T (A P)
    (matmul(pt, go.to(dev())) * b0.to(dev())).sum().backward()
    close(pt.grad, (go.double() @ b0.double().t()).t(), what="d (transposed view)")


# ------------------------------------------------------------------ piece layouts (round 5: the sharded layers' dense stage)
def _piece_engine(world, p_c, phases, chunks, n_nodes=20011):
    from pytorch_geometric_signed_directed_amd.parallel import PropagateEngine, ShardPlan
    align = PropagateEngine.alignment(world, p_c, phases, chunks)
    plan = ShardPlan(n_nodes, world, 1, align=align)
    return plan, PropagateEngine(plan, type("Ex", (), {"world_size": world, "rank": 1})(), p_c, phases, chunks)


@pytest.mark.gpu
@pytest.mark.parametrize("world,p_c,phases,chunks,f", [(8, 4, (0.4, 0.6), (0.5, 0.36, 0.14), 64), (8, 4, 2, 2, 128),
                                                       (4, 2, (0.3, 0.3, 0.4), (0.8, 0.2), 64), (8, 4, 1, 1, 64)])
def test_dense_stage_through_piece_layouts_is_bitwise_the_plain_one(world, p_c, phases, chunks, f):
    """pygsd_magnetic_dense_fwd_pieces_f32 / _bwd_pieces_f32 / pygsd_gather_pieces_f32 (round 5): the last Chebyshev term read
    straight out of a return exchange's receive buffer, the last gradient term stored straight into an inbound exchange's send
    buffers (every replica), the merge with its addend in one pass -- against the plain kernels on the merged / un-packed
    operands, bit for bit, with the engine's own layouts (uneven phases / chunks included) and a row count that is no multiple
    of the 16-row tiles (the pad rows behind it must stay untouched)."""
    from pytorch_geometric_signed_directed_amd.dense import PieceOperand, dense_bwd_raw, dense_fwd_raw, gather_pieces
    d = dev()
    plan, eng = _piece_engine(world, p_c, phases, chunks)
    n_pad, n_real, fw = plan.n_pad, plan.n_pad - 37, f // p_c
    g = torch.Generator().manual_seed(5)
    x_r, x_i, t_r, t_i = (torch.randn(n_pad, f, generator=g).to(d) for _ in range(4))
    w = (torch.randn(2, f, f, generator=g) * 0.2).to(d)
    bias = torch.randn(f, generator=g).to(d)
    g_r, g_i = torch.randn(n_pad, f, generator=g).to(d), torch.randn(n_pad, f, generator=g).to(d)
    # T_1 as the return exchange leaves it
    rl = eng.return_layout(2, fw)
    off = rl.offsets(n_pad, f).to(d)
    recv = torch.full((eng.block_rows * 2 * fw,), float("nan"), device=d)
    recv[off] = t_r
    recv[off + fw] = t_i
    recv = recv.view(eng.block_rows, 2 * fw)
    prod = PieceOperand(recv, 0, fw, rl)
    # forward
    want = dense_fwd_raw([x_r, t_r], [x_i, t_i], w, bias)
    got = dense_fwd_raw([x_r], [x_i], w, bias, last_in=prod)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the merge, alone and with an addend
    m_r, m_i = gather_pieces(prod, n_pad, f)
    assert torch.equal(m_r, t_r) and torch.equal(m_i, t_i)
    z_r, z_i = gather_pieces(prod, n_pad, f, z=[x_r, x_i])
    assert torch.equal(z_r, x_r + t_r) and torch.equal(z_i, x_i + t_i)
    assert [torch.equal(a, b) for a, b in zip(eng._merge(recv, 2), (t_r, t_i))] == [True, True]      # the engine's merge takes the kernel
    # backward: read T_1 in place, store dT_1 into the send buffers
    wda, wdb, wdw, wdbias = dense_bwd_raw([x_r, t_r], [x_i, t_i], w, g_r, g_i, rows=n_real)
    lay, bufs = eng.send_layout(2, f, x_r)
    for b in bufs:
        b.fill_(float("nan"))
    out = PieceOperand(bufs[0], 0, fw, lay)
    da, db, dw, dbias = dense_bwd_raw([x_r], [x_i], w, g_r, g_i, rows=n_real, last_in=prod, last_out=out)
    assert da[1] is None and db[1] is None
    assert torch.equal(da[0], wda[0]) and torch.equal(db[0], wdb[0]) and torch.equal(dw, wdw) and torch.equal(dbias, wdbias)
    for c in range(eng.phases):                                    # every replica of every phase = what packing dT_1 produces
        rows = slice(eng.phase_bounds[c], min(eng.phase_bounds[c + 1], n_real))
        want_pack = eng._pack([wda[1], wdb[1]], c).clone()          # (writes the same persistent buffer: compare copies)
        lead = want_pack.shape[:-2]
        hi = rows.stop - rows.start
        got_c = bufs[c]
        # _pack just overwrote bufs[c]: run the kernel again and compare the real rows, then the untouched pad rows
        for b in bufs:
            b.fill_(float("nan"))
        dense_bwd_raw([x_r], [x_i], w, g_r, g_i, rows=n_real, last_in=prod, last_out=out)
        if hi > 0:
            assert torch.equal(got_c[..., :hi, :], want_pack[..., :hi, :]), (c, lead)
        assert bool(torch.isnan(got_c[..., max(hi, 0):, :]).all())
    # mixed use: plain operands in, packed gradients out (the row layout's form) and the reverse
    da2, db2, dw2, _ = dense_bwd_raw([x_r, t_r], [x_i, t_i], w, g_r, g_i, rows=n_real, last_out=out)
    assert torch.equal(dw2, wdw) and torch.equal(da2[0], wda[0]) and da2[1] is None
    da3, db3, dw3, _ = dense_bwd_raw([x_r], [x_i], w, g_r, g_i, rows=n_real, last_in=prod)
    assert torch.equal(dw3, wdw) and torch.equal(da3[1], wda[1]) and torch.equal(db3[1], wdb[1])


ODD_WIDTHS = (20, 48, 80, 160, 320)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("k", ODD_WIDTHS)
def test_no_width_of_a_tall_linear_map_reaches_a_library(dtype, k):
    """Round 6: behind the MFMA tiles of pygsd_tall_linear / pygsd_tall_gram / pygsd_column_sums sits a generic HIP GEMM for
    bf16 as well as fp32 (pygsd_gemm_bf16), so x W + b of ANY width (DiGCNConv.py:66 at 20, 48, 80, 160 or 320 columns) and
    its three gradients take zero hipBLASLt / rocBLAS / torch-reduction routes -- and agree with float64 on the same
    (already rounded) operands: fp32 to the suite's bar, bf16 to one rounding of the fp32 sum."""
    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.dense import tall_linear
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    n = 5000                                                    # (tall reductions count as routes from 4096 rows)
    for f_out in ODD_WIDTHS:
        g = torch.Generator().manual_seed(1000 * k + f_out)
        x = torch.randn(n, k, generator=g).to(td)
        w = (torch.randn(k, f_out, generator=g) / k ** 0.5).to(td)
        b = torch.randn(f_out, generator=g).to(td)
        gy = torch.randn(n, f_out, generator=g).to(td)
        xd, wd, bd = (t.to(dev()).requires_grad_() for t in (x, w, b))
        _cabi.reset_library_routes()
        y = tall_linear(xd, wd, bd)
        y.backward(gy.to(dev()))
        torch.cuda.synchronize()
        assert _cabi.library_routes() == {}, (dtype, k, f_out, _cabi.library_routes())
        x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
        (x64 @ w64 + b64).backward(gy.double())
        tol = TOL if dtype == "f32" else 2.0 ** -8
        assert y.dtype == td and xd.grad.dtype == td and wd.grad.dtype == td and bd.grad.dtype == td
        close(y, x64 @ w64 + b64, tol, what=f"odd-width tall_linear forward {k}x{f_out} {dtype}")
        close(xd.grad, x64.grad, tol, what=f"odd-width dX {k}x{f_out} {dtype}")
        close(wd.grad, w64.grad, tol, norm=True, what=f"odd-width dW {k}x{f_out} {dtype}")
        close(bd.grad, b64.grad, tol, norm=True, what=f"odd-width db {k}x{f_out} {dtype}")


@pytest.mark.gpu
def test_generic_bf16_gemm_strides_addend_and_rounding():
    """pygsd_gemm_bf16 by itself: transposed views, an fp32 addend, fp32 and bf16 outputs, a split reduction -- against float64."""
    from pytorch_geometric_signed_directed_amd.dense import gemm_bf16
    g = torch.Generator().manual_seed(9)
    a = torch.randn(70, 33, generator=g).bfloat16().to(dev())
    b = torch.randn(33, 21, generator=g).bfloat16().to(dev())
    z = torch.randn(70, 21, generator=g).to(dev())
    bias = torch.randn(21, generator=g).bfloat16().to(dev())
    want = a.double() @ b.double() + z.double() + bias.double()
    got32 = gemm_bf16(a, b, bias=bias, addend=z, out_dtype=torch.float32)
    assert got32.dtype == torch.float32
    close(got32, want, TOL, what="generic bf16 GEMM, fp32 result")
    got16 = gemm_bf16(a, b, bias=bias, addend=z)
    assert got16.dtype == torch.bfloat16
    assert torch.equal(got16, got32.bfloat16())                 # ONE rounding of the same fp32 sums
    at = torch.randn(33, 70, generator=g).bfloat16().to(dev())  # A as a transposed view
    close(gemm_bf16(at.t(), b, out_dtype=torch.float32), at.double().t() @ b.double(), TOL, what="transposed A")
    tall_a = torch.randn(20000, 20, generator=g).bfloat16().to(dev())
    tall_b = torch.randn(20000, 48, generator=g).bfloat16().to(dev())
    close(gemm_bf16(tall_a.t(), tall_b, out_dtype=torch.float32), tall_a.double().t() @ tall_b.double(), TOL, norm=True,
          what="split reduction over 20000 rows")


@pytest.mark.gpu
def test_content_fingerprint_sees_any_change_and_nothing_else():
    """pygsd_fingerprint_u64 (memo.py's content check): equal bytes -> equal fingerprints whatever the alignment of the buffer;
    one changed element, two swapped elements, one appended byte -> different ones; deterministic across launches."""
    from pytorch_geometric_signed_directed_amd import _cabi
    g = torch.Generator().manual_seed(4)
    base = torch.randint(0, 2 ** 31, (2, 100003), generator=g).to(dev())

    def fp(t):
        return int(_cabi.fingerprint(t).item())
    a = fp(base)
    assert a == fp(base) == fp(base.clone())                       # deterministic, content only
    shifted = torch.empty(base.numel() + 1, dtype=torch.int64, device=dev())[1:].view(2, -1)     # 8-byte (not 16-byte) aligned storage
    shifted.copy_(base)
    assert shifted.data_ptr() % 16 == 8 and fp(shifted) == a
    one = base.clone()
    one[1, 77777] += 1
    assert fp(one) != a
    swapped = base.clone()
    swapped[0, 5], swapped[0, 6] = base[0, 6].clone(), base[0, 5].clone()
    assert (base[0, 5] == base[0, 6]) or fp(swapped) != a          # position-dependent: a permutation does not cancel
    floats = torch.randn(999, generator=g).to(dev())
    assert fp(floats) != fp(floats * 1.0000001) or True            # (may round to the same floats)
    assert fp(floats) == fp(floats.clone()) != fp(floats[:-1])
    bytes_ = torch.arange(0, 203, dtype=torch.uint8, device=dev())             # a 3-byte tail
    assert fp(bytes_) == fp(bytes_.clone()) != fp(torch.cat([bytes_[:-1], bytes_[-1:] + 1]))
    assert fp(torch.empty(0, device=dev())) == 0
    strided = base.t()                                             # non-contiguous view: fingerprinted through a copy
    assert fp(strided) == fp(strided.contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_generic_gemm_random_shapes_and_strides(dtype):
    """pygsd_gemm_f32 / pygsd_gemm_bf16 over 60 random problems: odd sizes (1 .. 300), A and / or B as transposed views or column
    slices of wider matrices, bias on / off, an addend (accumulate) on / off, reductions long enough to be split -- against
    float64 on the same (already rounded) operands."""
    from pytorch_geometric_signed_directed_amd.dense import gemm, gemm_bf16
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(2024)
    for case in range(60):
        m, n = (int(torch.randint(1, 300, (1,), generator=g)) for _ in range(2))
        k = int(torch.randint(1, 300, (1,), generator=g)) if case % 6 else int(torch.randint(5000, 9000, (1,), generator=g))
        ta, tb, sliced = (bool(torch.randint(0, 2, (1,), generator=g)) for _ in range(3))
        pad = 3 if sliced else 0
        a_store = torch.randn((k, m + pad) if ta else (m, k + pad), generator=g).to(td).to(dev())
        b_store = torch.randn((n, k + pad) if tb else (k, n + pad), generator=g).to(td).to(dev())
        a = (a_store[:, :m].t() if ta else a_store[:, :k])
        b = (b_store[:, :k].t() if tb else b_store[:, :n])
        bias = torch.randn(n, generator=g).to(td).to(dev()) if case % 2 else None
        z = torch.randn(m, n, generator=g).to(dev()) if case % 3 == 0 else None
        want = a.double() @ b.double()
        if bias is not None:
            want = want + bias.double()
        if z is not None:
            want = want + z.double()
        if dtype == "f32":
            out = None if z is None else z.clone()
            got = gemm(a, b, bias=bias, out=out, accumulate=z is not None)
        else:
            got = gemm_bf16(a, b, bias=bias, addend=z, out_dtype=torch.float32)
        scale = float(a.double().abs().max() * b.double().abs().max()) * k ** 0.5 + 1.0
        err = float((got.double() - want).abs().max()) / scale
        assert got.shape == (m, n) and err <= 2e-6, (case, m, n, k, ta, tb, sliced, err)
