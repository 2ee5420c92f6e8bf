"""GPU: the BASELINE configurations at their STATED sizes, on one GPU and node-sharded over 8 ranks, against a float64
evaluation (VERDICT r2 "sharded correctness at real size").

  north star  MagNetConv K = 1, h = 64, DSBM 1M nodes / 20M edges          (nn/directed/MagNetConv.py:122-249)
  C4          MSGNN's signed MSConv K = 2, h = 128, SDSBM 1M / 20M          (nn/general/MSConv.py:121-230, MSGNN.py:130-131)
  C5          DiGCN_InceptionBlock bf16, 2M nodes / ~52M entries / operator  (nn/directed/DiGCN_Inception_Block.py:31-47)

The arbiter is oracle/sparse_f64_torch.py -- the float64 formulas of oracle/sparse_f64.py on torch tensors (pinned to
the scipy evaluation on the host, tests/test_oracle_sparse_f64.py), evaluated here ON THE DEVICE in float64 with
coalesce / index_add_ only: the scipy evaluation of C4 needs minutes of one host core.  One GPU: every row is compared.
Sharded, 8 ranks: plan, distributed operator build, phases, row chunks, packing, both exchanges, merges and the
parameter all-reduce are the production code at the sizes and with the int32 / padding / alignment arithmetic of the
real run.  The magnetic configurations run their eight ranks as THREADS of this process (parallel.ThreadExchange: the
same SPMD code, collectives as rendezvous + copies; forward / backward driven by hand, tests/sharding_cpu.py) and compare
EVERY local row of every rank: eight PROCESSES sharing the one test GPU took minutes per layer construction at this
size (runtime queue scheduling between device contexts; measured 1.3 s -> 60..560 s), which the process-per-rank tests of
tests/test_gpu_sharded.py only tolerate because they are small.  C5 (whose ranks need the autograd engine: parameter hooks)
runs as four gloo processes and reports 1024 sampled rows: the test GPU is shared, and with this process four ranks are
the most that hold it at once.

Bars: fp32 outputs and input gradients per element |d| <= 1e-5 (1 + |want|); dW / db (row reductions) max-norm 1e-5;
bf16 (C5) 3 * 2^-8 of the max norm against float64 on bf16-rounded inputs and parameters."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bigdata
import fullsize as FS
import sharding_cpu as C
from tolerance import RECORDS, TOL

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
BF16_TOL = FS.BF16_TOL
WORLD = 8
PROCESS_WORLD = 4          # ranks as processes on the one shared test GPU (C5): with this process, five hold the device


def _record(what, err, tol, norm):
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    RECORDS.append(dict(err, test=test, what=what, bar="norm" if norm else "abs", tol=tol))
    worst = err["max_norm_rel_err"] if norm else err["max_mixed_err"]
    assert worst <= tol, (f"{what}: {'max-norm relative' if norm else '|d| / (1 + |want|)'} error {worst:.3e} > {tol} "
                          f"(abs {err['max_abs_err']:.3e}, |want| <= {err['max_abs_want']:.3g})")


def _check(got, want, what, tol=TOL, norm=False):
    """tolerance.close on the device (the arrays are up to 2M x 64): same bar, same record."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    _record(what, FS.errors(got.detach(), want.detach()), tol, norm)


@pytest.fixture(scope="module", params=list(FS.MAGNETIC))
def magnetic(request):
    """Float64 reference of one configuration (all rows, on the device), shared by its tests."""
    name = request.param
    want = FS.magnetic_reference(name, D)
    yield name, want
    del want
    torch.cuda.empty_cache()


def test_one_gpu_every_row_vs_float64(magnetic):
    """The un-sharded layer at the stated size, ALL rows of outputs and input gradients, dW, db."""
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv, MSConv
    name, want = magnetic
    cfg = FS.MAGNETIC[name]
    h, k = cfg["h"], cfg["k"]
    p_ei, p_sign, feats = FS.magnetic_files(name)
    layer = (MSConv if cfg["signed"] else MagNetConv)(h, h, k, 0.25, False, cached=True).to(D)
    weight, bias = FS.magnetic_params(name)
    with torch.no_grad():
        layer.weight.copy_(weight)
        layer.bias.copy_(bias)
    xr, xi, gr, gi = (FS.dev_tensor(p, D) for p in feats)
    xr.requires_grad_()
    xi.requires_grad_()
    o_r, o_i = layer(xr, xi, FS.dev_tensor(p_ei, D), None if p_sign is None else FS.dev_tensor(p_sign, D))
    ((o_r * gr).sum() + (o_i * gi).sum()).backward()
    for got, ref, what in ((o_r, want[0], "out_real"), (o_i, want[1], "out_imag"), (xr.grad, want[2], "dx_real"),
                           (xi.grad, want[3], "dx_imag")):
        _check(got, ref, f"{name} one GPU {what} (all rows) vs float64")
    _check(layer.weight.grad, want[4], f"{name} one GPU dW vs float64", norm=True)
    _check(layer.bias.grad, want[5], f"{name} one GPU db vs float64", norm=True)


@pytest.mark.parametrize("layout", ["auto", "rows", "auto+cached-inputs"])
def test_sharded_8_ranks_every_row_vs_float64(magnetic, layout):
    """8 ranks (threads, one device), default pipeline (auto = 2 x 4 grid, 2 phases x 2 return chunks; rows = all-gather
    layout, 2 phases), distributed operator build: EVERY local row of out_real / out_imag / dx_real / dx_imag of every
    rank, and the all-reduced dW / db, vs float64."""
    from pytorch_geometric_signed_directed_amd.parallel import ShardedMagNetConv
    name, want = magnetic
    cfg = FS.MAGNETIC[name]
    n, h, k = cfg["n"], cfg["h"], cfg["k"]
    p_ei, p_sign, feats = FS.magnetic_files(name)
    ei = FS.dev_tensor(p_ei, D)                               # read-only, shared by the eight ranks
    sign = None if p_sign is None else FS.dev_tensor(p_sign, D)
    weight, bias = FS.magnetic_params(name)

    # "+cached-inputs" (round 5): the forward's inbound exchange memoised -- the step is run TWICE and the second one, which reads
    # the kept pieces (joined, multiplied in a single walk with the un-phased operator rows), is the one checked
    cached = layout.endswith("+cached-inputs")
    layout = layout.split("+")[0]

    def body(rank, exchange):
        layer = ShardedMagNetConv(h, h, k, 0.25, n, ei, sign, device=D, layout=layout, signed=cfg["signed"],
                                  exchange=exchange, cache_input_exchange=cached)
        with torch.no_grad():
            layer.weight.copy_(weight)
            layer.bias.copy_(bias)
        plan, eng = layer.plan, layer.engine
        a, b, ga, gb = (FS.shard(p, plan, h, D) for p in feats)
        outs = C.sharded_magnetic_step(layer, a, b, ga, gb)
        if cached:
            assert len(layer._input_memo) == 1
            outs = C.sharded_magnetic_step(layer, a, b, ga, gb)
        return plan, (layer.layout, eng.p_r, eng.p_c, eng.phases, eng.return_chunks), outs, layer.global_nnz

    res = C.run_ranks_as_threads(WORLD, body)
    shape = res[0][1]
    from pytorch_geometric_signed_directed_amd.parallel import default_pipeline, split_spec
    d_ph, d_rc = (split_spec(v)[0] for v in default_pipeline(WORLD, layout == "auto"))      # (counts: the pieces may be uneven)
    assert shape == (("grid", 2, 4, d_ph, d_rc) if layout == "auto" else ("rows", 8, 1, d_ph, 1)), shape
    tag = f"{name} 8 ranks {shape[0]} {shape[1]}x{shape[2]} C{shape[3]} R{shape[4]}"
    assert sum(r[0].n_local for r in res) == n and len({r[3] for r in res}) == 1
    for j, what in enumerate(("out_real", "out_imag", "dx_real", "dx_imag")):
        got = torch.cat([r[2][j][:r[0].n_local] for r in res])          # contiguous ownership: rank order = row order
        _check(got, want[j], f"{tag} {what} (all rows) vs float64")
        assert all(float(r[2][j][r[0].n_local:].abs().sum()) == 0 for r in res)     # pad rows stay out of the graph
    for r in res:                                                         # all-reduced: the same sums on every rank
        assert torch.equal(r[2][4], res[0][2][4]) and torch.equal(r[2][5], res[0][2][5])
    _check(res[0][2][4], want[4], f"{tag} dW vs float64", norm=True)
    _check(res[0][2][5], want[5], f"{tag} db vs float64", norm=True)


# ------------------------------------------------------------------------------------------------ C5
@pytest.fixture(scope="module")
def inception():
    ref = FS.inception_reference(D)
    yield ref
    del ref
    torch.cuda.empty_cache()


def test_c5_one_gpu_bf16_every_row_vs_float64(inception):
    from pytorch_geometric_signed_directed_amd.nn import DiGCN_InceptionBlock
    outs, dx, grads = inception
    n, h = FS.C5["n"], FS.C5["h"]
    ib = DiGCN_InceptionBlock(h, h)
    ib.load_state_dict(FS.inception_params())
    ib.to(D).to(torch.bfloat16)
    p_x, p_g = bigdata.features(n, h, 6, 2)
    x = FS.dev_tensor(p_x, D).to(torch.bfloat16).requires_grad_()
    go = FS.dev_tensor(p_g, D)
    (e1, w1), (e2, w2) = [(FS.dev_tensor(a, D), FS.dev_tensor(b, D)) for a, b in bigdata.digcn_operators(n, FS.C5["e"], seed=3)]
    got = ib(x, e1, w1, e2, w2)
    sum(((k + 1.0) * o.float() * go).sum() for k, o in enumerate(got)).backward()
    for k, (o, ref) in enumerate(zip(got, outs)):
        _check(o.float(), ref, f"C5 one GPU x{k} (bf16, all rows) vs float64", BF16_TOL, norm=True)
    _check(x.grad.float(), dx, "C5 one GPU dx (bf16, all rows) vs float64", BF16_TOL, norm=True)
    for name, prm in ib.named_parameters():
        _check(prm.grad.float(), grads[name], f"C5 one GPU d {name} (bf16) vs float64", BF16_TOL, norm=True)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _inception_rank(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorch_geometric_signed_directed_amd.parallel import ShardedDiGCNInceptionBlock
        n, h = FS.C5["n"], FS.C5["h"]
        (e1, w1), (e2, w2) = [(FS.dev_tensor(a, D), FS.dev_tensor(b, D)) for a, b in bigdata.digcn_operators(n, FS.C5["e"], seed=3)]
        layer = ShardedDiGCNInceptionBlock(h, h, n, e1, w1, e2, w2, device=D)
        layer.load_state_dict(FS.inception_params())
        layer.to(torch.bfloat16)
        del e1, w1, e2, w2
        plan = layer.plan
        p_x, p_g = bigdata.features(n, h, 6, 2)
        a = FS.shard(p_x, plan, h, D).to(torch.bfloat16).requires_grad_()
        go = FS.shard(p_g, plan, h, D)
        outs = layer(a)
        sum(((k + 1.0) * o.float() * go).sum() for k, o in enumerate(outs)).backward()
        rows = FS.sample_rows(n)
        mine = rows[(rows >= plan.lo) & (rows < plan.hi)]
        loc = torch.from_numpy(mine - plan.lo).to(D)
        ret[rank] = dict(rows=mine, vals=[t.detach().float()[loc].cpu().numpy() for t in outs + (a.grad,)],
                         grads={k: p.grad.float().cpu().numpy() for k, p in layer.named_parameters()},
                         phases=layer.engine.phases)
    finally:
        dist.destroy_process_group()


def test_c5_sharded_4_ranks_bf16_sampled_rows_vs_float64(inception):
    """The sharded inception block in bf16 at the stated size, four gloo processes on the one GPU (row layout, one
    all-gather shared by both convolutions): 1024 sampled rows and the all-reduced parameter gradients."""
    outs, dx, grads = inception
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_inception_rank, args=(PROCESS_WORLD, _free_port(), ret), nprocs=PROCESS_WORLD, join=True)
    assert len(ret) == PROCESS_WORLD
    rows = np.concatenate([ret[r]["rows"] for r in range(PROCESS_WORLD)])
    assert np.array_equal(rows, FS.sample_rows(FS.C5["n"]))
    idx = torch.from_numpy(rows).to(D)
    for k, ref in enumerate(outs + [dx]):
        got = torch.from_numpy(np.concatenate([ret[r]["vals"][k] for r in range(PROCESS_WORLD)])).to(D)
        scale = max(1.0, float(ref.abs().max()))               # relative to the WHOLE matrix's scale, as on one GPU
        err = float((got.double() - ref[idx]).abs().max())
        _record(f"C5 {PROCESS_WORLD} ranks {'x%d' % k if k < 3 else 'dx'} (bf16, {FS.N_SAMPLE} rows) vs float64",
                {"max_abs_err": err, "max_mixed_err": err / scale, "max_norm_rel_err": err / scale, "max_abs_want": scale},
                BF16_TOL, True)
    for name, ref in grads.items():
        _check(torch.from_numpy(ret[0]["grads"][name]).to(D), ref, f"C5 {PROCESS_WORLD} ranks d {name} (bf16) vs float64", BF16_TOL, norm=True)


# ------------------------------------------------------------------------------------------------ C3
# BASELINE config 3: "SSSNET / SGCN signed scatter-aggregate on synthetic SSBM 500k nodes / 10M +- edges, h = 64".
# The arbiter is the float64 evaluation of oracle/sparse_f64_torch.py (pinned on the host against the dense formulas, the
# reference op sequence in float64 and the fixtures recorded from the reference: tests/test_oracle_sparse_f64.py); every
# check also runs the reference's own fp32 op sequence (oracle/ref_layers.py: index_select -> mul -> scatter_add_) on the
# device and records ITS distance from float64 -- the HIP result must be inside the 1e-5 bar around the float64 value, or
# no further from it than 1.5x the reference sequence is (tolerance.close_arbitrated's rule, evaluated on the device).
C3 = dict(n=500000, entries=10000000, h=64, hop=2, fill=0.5)


def _check_arbitrated(got, ref32, truth, what, norm=False):
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    err, ref = FS.errors(got.detach(), truth.detach()), FS.errors(ref32.detach(), truth.detach())
    apart = FS.errors(got.detach(), ref32.detach())             # HIP <-> the reference's fp32 op sequence, directly (round 5)
    key = "max_norm_rel_err" if norm else "max_mixed_err"
    bar = max(TOL, 1.5 * ref[key])
    bar_ref = max(TOL, 2.0 * ref[key])
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    RECORDS.append(dict(err, test=test, what=what + " (float64 arbiter)", bar="norm" if norm else "abs", tol=bar,
                        reference_sequence_err_vs_f64=ref[key], hip_vs_reference_sequence=apart[key],
                        hip_vs_reference_sequence_bar=bar_ref))
    assert err[key] <= bar, (f"{what} vs float64: {err[key]:.3e} > max({TOL}, 1.5 x {ref[key]:.3e} of the fp32 reference "
                             f"sequence) (abs {err['max_abs_err']:.3e}, |want| <= {err['max_abs_want']:.3g})")
    assert apart[key] <= bar_ref, (f"{what} vs the fp32 reference sequence: {apart[key]:.3e} > max({TOL}, 2 x {ref[key]:.3e} = "
                                   f"the reference's own distance from float64)")


@pytest.fixture(scope="module")
def ssbm_c3():
    p_ei, p_sign = bigdata.ssbm_graph(C3["n"], C3["entries"], seed=2)
    ei, sign = FS.dev_tensor(p_ei, D), FS.dev_tensor(p_sign, D)
    pos, neg = ei[:, sign > 0].contiguous(), ei[:, sign < 0].contiguous()
    g = torch.Generator(device="cuda").manual_seed(21)
    w_pos = torch.rand(pos.size(1), device=D, generator=g) + 0.5
    w_neg = torch.rand(neg.size(1), device=D, generator=g) + 0.5
    yield pos, neg, w_pos, w_neg
    torch.cuda.empty_cache()


def _randn(*shape, seed):
    return torch.randn(*shape, device=D, generator=torch.Generator(device="cuda").manual_seed(seed))


@pytest.mark.parametrize("directed", [False, True])
def test_c3_simpa_hop2_every_row_vs_float64(ssbm_c3, directed):
    """SIMPA (SSSNET's aggregation, nn/signed/SIMPA.py:77-139) at C3's stated size, weighted operators: every row of the
    output and of the input gradients, and the hop-weight gradients (pygsd_dots_f32) -- the one-node _StreamFn with its
    backward summands folded into the SpMM epilogues, on the low-degree kernel variant the 5-entry rows select."""
    from oracle import ref_layers as R
    from oracle import sparse_f64_torch as T64
    from pytorch_geometric_signed_directed_amd.nn import SIMPA
    pos, neg, w_pos, w_neg = ssbm_c3
    n, h, hop, fill = C3["n"], C3["h"], C3["hop"], C3["fill"]
    k = 4 if directed else 2
    xs = [_randn(n, h, seed=30 + j) for j in range(k)]
    go = _randn(n, k * h, seed=40)
    layer = SIMPA(hop, fill, directed).to(D)
    with torch.no_grad():
        for j, prm in enumerate(layer.parameters()):
            prm.copy_(torch.rand(prm.shape, generator=torch.Generator().manual_seed(50 + j)) + 0.5)
    names = [nm for nm, _ in layer.named_parameters()]

    def run(fn, dtype):
        ins = [x.detach().clone().to(dtype).requires_grad_() for x in xs]
        prm = {nm: p.detach().clone().to(dtype).requires_grad_() for nm, p in layer.named_parameters()}
        out = fn(pos, w_pos.to(dtype), neg, w_neg.to(dtype), ins[0], ins[1], prm, hop, fill, directed, *ins[2:])
        (out * go.to(dtype)).sum().backward()
        return [out.detach()] + [x.grad for x in ins] + [prm[nm].grad for nm in names]

    truth, ref32 = run(T64.simpa, torch.float64), run(R.simpa, torch.float32)
    ins = [x.clone().requires_grad_() for x in xs]
    out = layer(pos, w_pos, neg, w_neg, *ins)
    (out * go).sum().backward()
    got = [out] + [x.grad for x in ins] + [p.grad for p in layer.parameters()]
    tag = f"C3 SIMPA hop {hop} {'directed' if directed else 'undirected'}"
    labels = ["feat"] + ["dx_" + s for s in ("p", "n", "pt", "nt")[:k]] + ["d" + nm for nm in names]
    for a, r, t, what in zip(got, ref32, truth, labels):
        _check_arbitrated(a, r, t, f"{tag} {what} (all rows)", norm=what.startswith("d_"))


def test_c3_dimpa_hop2_every_row_vs_float64():
    """DIMPA (nn/directed/DIMPA.py:32-59) on a DSBM graph of C3's size (500k nodes / 10M weighted directed edges)."""
    from oracle import ref_layers as R
    from oracle import sparse_f64_torch as T64
    from pytorch_geometric_signed_directed_amd.nn import DIMPA
    n, h, hop, fill = C3["n"], C3["h"], C3["hop"], C3["fill"]
    ei = FS.dev_tensor(bigdata.dsbm_graph(n, C3["entries"], seed=5), D)
    w = torch.rand(ei.size(1), device=D, generator=torch.Generator(device="cuda").manual_seed(22)) + 0.5
    x_s, x_t, go = _randn(n, h, seed=31), _randn(n, h, seed=32), _randn(n, 2 * h, seed=41)
    layer = DIMPA(hop, fill).to(D)
    with torch.no_grad():
        for j, prm in enumerate(layer.parameters()):
            prm.copy_(torch.rand(prm.shape, generator=torch.Generator().manual_seed(60 + j)) + 0.5)

    def run(fn, dtype):
        a, b = (t.detach().clone().to(dtype).requires_grad_() for t in (x_s, x_t))
        ws, wt = (p.detach().clone().to(dtype).requires_grad_() for p in (layer._w_s, layer._w_t))
        out = fn(a, b, ei, w.to(dtype), ws, wt, hop, fill)
        (out * go.to(dtype)).sum().backward()
        return out.detach(), a.grad, b.grad, ws.grad, wt.grad

    truth, ref32 = run(T64.dimpa, torch.float64), run(R.dimpa, torch.float32)
    a, b = x_s.clone().requires_grad_(), x_t.clone().requires_grad_()
    out = layer(a, b, ei, w)
    (out * go).sum().backward()
    got = (out, a.grad, b.grad, layer._w_s.grad, layer._w_t.grad)
    for g_, r, t, what in zip(got, ref32, truth, ("feat", "dx_s", "dx_t", "d_w_s", "d_w_t")):
        _check_arbitrated(g_, r, t, f"C3-size DIMPA hop {hop} {what} (all rows)", norm=what.startswith("d_"))


def test_c3_sssnet_model_every_row_vs_float64(ssbm_c3):
    """SSSNET_node_clustering (nn/signed/SSSNET_node_clustering.py:90-160; 64 features, hidden 64, 5 clusters, hop 2) in
    eval mode on C3's SSBM with unit weights: normalised embedding, log-probabilities, probabilities (every row), the
    gradient of the features and of EVERY parameter (MLP weights through the tall products, hop weights, head)."""
    from oracle import sparse_f64_torch as T64
    from pytorch_geometric_signed_directed_amd.nn import SSSNET_node_clustering
    pos, neg, _, _ = ssbm_c3
    n, h, hop, fill = C3["n"], C3["h"], C3["hop"], C3["fill"]
    torch.manual_seed(17)
    model = SSSNET_node_clustering(h, h, 5, 0.5, hop, fill).to(D).eval()
    with torch.no_grad():
        model._bias.uniform_(-0.5, 0.5)
    feats = _randn(n, h, seed=33)
    gz, gl, gp = _randn(n, 2 * h, seed=42), _randn(n, 5, seed=43), _randn(n, 5, seed=44)
    w_pos, w_neg = torch.ones(pos.size(1), device=D), torch.ones(neg.size(1), device=D)

    x64 = feats.double().requires_grad_()
    sd64 = {k: v.detach().double().requires_grad_() for k, v in model.state_dict().items()}
    z64, lp64, pr64 = T64.sssnet(pos, w_pos, neg, w_neg, x64, sd64, hop, fill)
    ((z64 * gz.double()).sum() + (lp64 * gl.double()).sum() + (pr64 * gp.double()).sum()).backward()

    # the reference's own op sequence in fp32 on the device (torch.mm MLPs, ref_layers.simpa, torch.mm head)
    from oracle import ref_layers as R
    x32 = feats.clone().requires_grad_()
    sd32 = {k: v.detach().clone().requires_grad_() for k, v in model.state_dict().items()}
    xs32 = [torch.mm(torch.relu(torch.mm(x32, sd32[f"_w_{s}0"])), sd32[f"_w_{s}1"]) for s in ("p", "n")]
    z32 = R.simpa(pos, w_pos, neg, w_neg, xs32[0], xs32[1], {"_w_p": sd32["_simpa._w_p"], "_w_n": sd32["_simpa._w_n"]},
                  hop, fill)
    o32 = torch.mm(z32, sd32["_W_prob"]) + sd32["_bias"]
    zn32, lp32, pr32 = torch.nn.functional.normalize(z32), torch.log_softmax(o32, 1), torch.softmax(o32, 1)
    ((zn32 * gz).sum() + (lp32 * gl).sum() + (pr32 * gp).sum()).backward()

    x = feats.clone().requires_grad_()
    z, logp, pred, prob = model(pos, w_pos, neg, w_neg, x)
    ((z * gz).sum() + (logp * gl).sum() + (prob * gp).sum()).backward()
    _check_arbitrated(z, zn32, z64.detach(), "C3 SSSNET normalised embedding (all rows)")
    _check_arbitrated(logp, lp32, lp64.detach(), "C3 SSSNET log-probabilities (all rows)")
    _check_arbitrated(prob, pr32, pr64.detach(), "C3 SSSNET probabilities (all rows)")
    assert float((pred != lp64.argmax(1)).float().mean()) <= 1e-4           # ties within rounding only
    _check_arbitrated(x.grad, x32.grad, x64.grad, "C3 SSSNET d features (all rows)")
    for name, prm in model.named_parameters():
        _check_arbitrated(prm.grad, sd32[name].grad, sd64[name].grad, f"C3 SSSNET d {name}", norm=True)


def test_c3_sgcn_every_row_and_parameter_gradients_vs_float64(ssbm_c3):
    """SGCNConv first (64 -> 32) and deep (32 + 32 -> 32) aggregation at C3's size: every row of the output and of dx, and
    the lin_b / lin_u weight and bias gradients (the products over the 500k rows; nn/signed/SGCNConv.py:94-126)."""
    from oracle import ref_layers as R
    from oracle import sparse_f64_torch as T64
    from pytorch_geometric_signed_directed_amd.nn import SGCNConv
    pos, neg, _, _ = ssbm_c3
    n, h = C3["n"], C3["h"]
    for first in (True, False):
        in_dim, o = (h, h // 2) if first else (h // 2, h // 2)
        torch.manual_seed(5 if first else 6)
        conv = SGCNConv(in_dim, o, first_aggr=first).to(D)
        x, go = _randn(n, h, seed=34 + first), _randn(n, 2 * o, seed=45 + first)
        names = ("lin_b.weight", "lin_b.bias", "lin_u.weight", "lin_u.bias")
        sd = conv.state_dict()

        def run(fn, dtype):
            a = x.detach().clone().to(dtype).requires_grad_()
            prm = [sd[nm].detach().clone().to(dtype).requires_grad_() for nm in names]
            out = fn(a, pos, neg, (prm[0], prm[1]), (prm[2], prm[3]), first, in_dim)
            (out * go.to(dtype)).sum().backward()
            return [out.detach(), a.grad] + [p.grad for p in prm]

        truth, ref32 = run(T64.sgcn_conv, torch.float64), run(R.sgcn_conv, torch.float32)
        b = x.clone().requires_grad_()
        out = conv(b, pos, neg)
        (out * go).sum().backward()
        got = [out, b.grad] + [dict(conv.named_parameters())[nm].grad for nm in names]
        tag = f"C3 SGCNConv {'first' if first else 'deep'}"
        for a, r, t, what in zip(got, ref32, truth, ("out", "dx") + tuple("d " + nm for nm in names)):
            _check_arbitrated(a, r, t, f"{tag} {what}", norm=what.startswith("d "))


def test_c3_sharded_signed_layers_8_ranks_forward_every_row_vs_float64(ssbm_c3):
    """Round 5 (review: the sharded signed layers were checked at toy sizes only): ShardedSGCNConv (first aggregation, 64 -> 32)
    and ShardedSIMPA (hop 2, undirected, weighted operators) at BASELINE config 3's stated size -- SSBM 500k nodes / 10M +-
    entries -- over 8 ranks in the row layout, EVERY row of every rank's output against float64 (and the reference's fp32 op
    sequence beside it).  The ranks run as threads of one process (parallel.ThreadExchange: the same SPMD code, collectives as
    rendezvous + copies), forward only: autograd's single worker thread per device cannot rendezvous with itself, and the
    backward of these layers is autograd's composition of the pieces the 2 - 4-process tests of tests/test_gpu_sharded.py check
    with gradients (nn/signed/SGCNConv.py:94-126, nn/signed/SIMPA.py:77-139)."""
    from oracle import ref_layers as R
    from oracle import sparse_f64_torch as T64
    from pytorch_geometric_signed_directed_amd.nn import SGCNConv
    from pytorch_geometric_signed_directed_amd.parallel import ShardedSGCNConv, ShardedSIMPA
    pos, neg, w_pos, w_neg = ssbm_c3
    n, h, hop, fill = C3["n"], C3["h"], C3["hop"], C3["fill"]
    o = h // 2
    torch.manual_seed(5)
    sd = {k: v.to(D) for k, v in SGCNConv(h, o, first_aggr=True).state_dict().items()}
    x, xp, xn = _randn(n, h, seed=61), _randn(n, h, seed=62), _randn(n, h, seed=63)
    hop_w = {"_w_p": (torch.rand(hop + 1, 1, generator=torch.Generator().manual_seed(70)) + 0.5).to(D),
             "_w_n": (torch.rand(int((1 + hop) * hop / 2), 1, generator=torch.Generator().manual_seed(71)) + 0.5).to(D)}

    def body(rank, exchange):
        with torch.no_grad():
            conv = ShardedSGCNConv(h, o, True, n, pos, neg, device=D, exchange=exchange)
            conv.load_state_dict(sd)
            out = conv(conv.shard_rows(x))
            simpa = ShardedSIMPA(hop, fill, n, pos, w_pos, neg, w_neg, device=D, exchange=exchange)
            for k, v in hop_w.items():
                getattr(simpa, k).copy_(v)
            feat = simpa(simpa.shard_rows(xp), simpa.shard_rows(xn))
        assert conv.plan.bounds == simpa.plan.bounds
        return conv.plan, out, feat

    res = C.run_ranks_as_threads(WORLD, body)
    assert sum(r[0].n_local for r in res) == n
    got_conv = torch.cat([r[1][:r[0].n_local] for r in res])
    got_simpa = torch.cat([r[2][:r[0].n_local] for r in res])
    assert all(float(r[1][r[0].n_local:].abs().sum()) == 0 and float(r[2][r[0].n_local:].abs().sum()) == 0 for r in res)
    with torch.no_grad():
        def sgcn(fn, dt):
            p = {k: v.to(dt) for k, v in sd.items()}
            return fn(x.to(dt), pos, neg, (p["lin_b.weight"], p["lin_b.bias"]), (p["lin_u.weight"], p["lin_u.bias"]), True, h)

        def simpa_ref(fn, dt):
            prm = {k: v.to(dt) for k, v in hop_w.items()}
            return fn(pos, w_pos.to(dt), neg, w_neg.to(dt), xp.to(dt), xn.to(dt), prm, hop, fill, False)

        _check_arbitrated(got_conv, sgcn(R.sgcn_conv, torch.float32), sgcn(T64.sgcn_conv, torch.float64),
                          "C3 ShardedSGCNConv first, 8 ranks (all rows)")
        _check_arbitrated(got_simpa, simpa_ref(R.simpa, torch.float32), simpa_ref(T64.simpa, torch.float64),
                          f"C3 ShardedSIMPA hop {hop}, 8 ranks (all rows)")
