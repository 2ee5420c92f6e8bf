"""bench.py -- edges/sec (fwd+bwd) of MagNetConv on a synthetic DSBM graph, one JSON line.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--nodes 1000000] [--edges 20000000]
                    [--hidden 64] [--no-cpu-baseline] [--layout auto|rows|grid] [--phases C] [--return-chunks R]
                    [--dump-outputs DIR] [--full]

Metric (BASELINE.json): input edges per second, forward + backward of ONE MagNetConv layer
(K=1, q=0.25, sym normalisation, in = out = hidden, fp32), operator cached (steady state), on a DSBM
graph (5 clusters, cyclic meta-graph eta=0.1, size_ratio 1.5) of 1M nodes / 20M edges; inputs
resident in HBM before the timed region.  A "step" = layer forward + loss.backward() with
loss = out_real.sum() + out_imag.sum() and gradients w.r.t. x_real, x_imag, weight, bias.

Timing.  W warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides; `value` and
`ms_per_step` come from that wall-clock interval (max over ranks).  Every timed step is also bracketed by HIP
events on the compute stream: `ms_per_step_median` / `_min` / `_max` are their statistics.  The per-launch
event recorder (pygsd_prof_*) is OFF in that pass; a second, untimed pass of min(K, PROF_STEPS) steps runs with it on
and feeds the `roofline` object (average launch duration of the dominant kernel, measured live in this run).  Beyond
those, a default run does only fixed work of a few seconds (inputs, operator build, a 2 x 1 GiB copy), so its length
follows K: a caller can size K from one run's `ms_per_step`.  `--full` adds the secondary legs -- three more K-step
passes (dense upstream gradient, with and without its loss; exact-fp32 dense stage), the x4 DRAM-bound graph, the other
BASELINE configurations, live PMC traffic and the CPU baseline -- about a minute more, independent of K.

N > 1.  `python bench.py --gpus N` works as typed: without WORLD_SIZE in the environment it re-executes itself
under `python -m torch.distributed.run --nproc-per-node N` (one rank per GPU, RCCL); the driver's own torchrun
launch is detected and used as is.  The same graph is sharded by node range over the ranks (strong scaling;
parallel.ShardedMagNetConv: equal-work ranges, grid or row layout, exchanges overlapped with the partial
products).  The `exchange` object reports, per step, the compute-stream time of the propagates split into
product / exposed exchange wait / packing, and the duration of the exchanges run alone.

`--dump-outputs DIR` writes what the LAST timed step handed its caller -- out_real, out_imag and the gradients of x_real,
x_imag, weight and bias -- to DIR/<name>.npy (float32), at most DUMP_BYTES in all: the [N, F] arrays on a fixed, seeded sample
of rows once they no longer fit whole (the same rows for every run and rank count).  The inputs depend on the arguments alone,
so two builds of the library can be compared output for output.

Extra objects in the JSON line: `roofline` (dominant kernel = the fused dual-value SpMM; algorithmic bytes per
SURVEY.md 8(d); `achievable_peak` = a streaming float4 copy of 2 x 1 GiB timed in this run) and, with `--full`,
`cpu_baseline` (the oracle's reference op sequence on this box's host cores, rank 0, N=1: operator cached and, as the
reference defaults to, rebuilt every forward) and `configs`.  Without `--full` the fields of the secondary legs are null
and `roofline.traffic` / `dram_bound_reference` are replayed from the tracked captures under profiles/, labelled so.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
DUMP_BYTES = 48 << 20  # --dump-outputs: the most written in all
DUMP_SEED = 20240      # --dump-outputs: the row sample of the [N, F] outputs
PROF_STEPS = 10        # steps of the instrumented pass (per-launch averages need no more)


def spmm_bytes(nnz, n, f, s=4):
    """ALGORITHMIC bytes of one SpMM Y = S X (edge-centric gather model, int32 CSR,
    no cache-reuse credit): nnz * (col 4 + val 4 + gathered row F*s) + N*F*s (write) + rowptr."""
    return nnz * (8 + f * s) + n * f * s + 4 * (n + 1)


def build_inputs(n, e, hidden, device, seed=0):
    from pytorch_geometric_signed_directed_amd import graphs
    ei, _, p = graphs.dsbm_for_edges(n, e, seed=seed)
    g = torch.Generator().manual_seed(0)
    x_real = torch.randn(n, hidden, generator=g)
    x_imag = torch.randn(n, hidden, generator=g)
    edge_index = torch.from_numpy(ei)
    return edge_index.to(device), x_real.to(device), x_imag.to(device), p


def cpu_baseline(hidden, steps=4, n=100000, e=2000000, threads=None):
    """Reference op sequence (index_select -> mul -> scatter_add_, 4 propagates per order incl. the
    reference's duplicates, autograd backward) on the host cores: `cached=True` (steady state, comparable with the
    GPU figure) and `cached=False` (the reference's default, MagNetConv.py:45,157-181: operator rebuilt by every
    forward).  Median of `steps` timed steps each, after one warm-up."""
    from oracle import ref_layers as R
    from pytorch_geometric_signed_directed_amd import graphs
    # ATen's index_select / scatter_add_ stop scaling long before a 256-thread host is full (measured
    # on the GPU box, EPYC 9575F: 8 thr 3.8 s, 32 thr 3.2 s, 128 thr 4.7 s, 256 thr 28 s per step), so
    # the baseline runs on the best-performing thread count, and reports that count as `cores`.
    available = os.cpu_count() or 1
    cores = threads or min(available, 32)
    torch.set_num_threads(cores)
    ei_np, _, _ = graphs.dsbm_for_edges(n, e, seed=0)
    ei = torch.from_numpy(ei_np)
    g = torch.Generator().manual_seed(0)
    xr = torch.randn(n, hidden, generator=g, requires_grad=True)
    xi = torch.randn(n, hidden, generator=g, requires_grad=True)
    torch.manual_seed(0)
    w = torch.empty(2, hidden, hidden).uniform_(-1, 1).mul_((6.0 / (2 * hidden)) ** 0.5).requires_grad_()
    b = torch.zeros(hidden, requires_grad=True)
    cached_op = R.magnet_operator(ei, None, n, 0.25, "sym", 2.0)

    def step(op=None):
        op = op if op is not None else R.magnet_operator(ei, None, n, 0.25, "sym", 2.0)
        o_r, o_i = R.magnet_conv(xr, xi, op, w, b, duplicate=True)
        (o_r.sum() + o_i.sum()).backward()

    def once(op):
        t0 = time.perf_counter()
        step(op)
        return time.perf_counter() - t0

    once(cached_op)  # warm-up
    once(None)
    t_cached, t_rebuilt = [], []
    for _ in range(steps):          # interleaved, so that slow drifts of the host hit both legs alike
        t_cached.append(once(cached_op))
        t_rebuilt.append(once(None))
    t0 = time.perf_counter()
    R.magnet_operator(ei, None, n, 0.25, "sym", 2.0)
    build_s = time.perf_counter() - t0
    med_c, med_u = statistics.median(t_cached), statistics.median(t_rebuilt)
    edges = ei.size(1)
    return {"value": edges / med_c, "unit": "edges/s", "cores": cores, "cores_available": available, "kind": "port",
            "cpu_model": cpu_model(),
            "value_uncached": edges / med_u, "operator_build_seconds": build_s,
            "seconds_per_step": {"cached_median": med_c, "cached_min": min(t_cached), "cached_max": max(t_cached),
                                 "uncached_median": med_u, "uncached_min": min(t_rebuilt), "uncached_max": max(t_rebuilt)},
            "scaled_from": "C2 size (DSBM 100k nodes / 2M edges = north-star / 10): the reference's per-propagate "
                           "[nnz, F] message temporaries are 10.7 GB each at the north-star size; edges/s of this "
                           "path is size-independent to first order (gather / scatter bound), so the figure is "
                           "quoted as measured, not rescaled",
            "sample": f"oracle/ref_layers.magnet_conv (reference op sequence, 4 propagates/order), DSBM {n} nodes / "
                      f"{edges} edges, h={hidden}: `value` = operator cached, median of {len(t_cached)} fwd+bwd steps "
                      f"({med_c:.2f} s/step); `value_uncached` = operator rebuilt every forward (reference default, "
                      f"MagNetConv.py:45), median of {len(t_rebuilt)} ({med_u:.2f} s/step); {cores} of "
                      f"{available} host threads (ATen scatter_add_ anti-scales beyond)"}


def cpu_model():
    """The host CPU's model string ("core count and CPU model stated"): lscpu, else /proc/cpuinfo."""
    try:
        for ln in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except Exception:  # noqa: BLE001
        pass
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.lower().startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def baseline_configs(timeout_s=240):
    """The other single-GPU BASELINE.json configurations, timed in THIS run (a child process of tools/bench_configs.py in its
    compact mode, after the headline has released the device): C2 MagNetConv 100k / 2M, C3a SGCNConv and C3b SIMPA hop 2 on
    SSBM 500k / 10M, C4 MSConv K=2 h=128 on SDSBM 1M / 20M (on ONE GPU), C5a / C5b DiGCN inception block fp32 / bf16 on 2M
    nodes / 52M entries per operator.  Per configuration: fwd+bwd ms per step (eager, operator cached), the dominant kernel
    class (all of them are SpMM-bound) with its average launch, and that kernel's algorithmic rate as a fraction of the 8 TB/s
    HBM peak (SURVEY.md 8(d) byte model, tools/bench_configs.py)."""
    path = os.path.join(ROOT, "gpurun_out", "bench_configs_compact.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    env = dict(os.environ, PYGSD_CONFIGS="C2,C3a,C3b,C4,C5a,C5b", PYGSD_CONFIGS_COMPACT="1", PYGSD_CONFIGS_OUT=path)
    env.pop("WORLD_SIZE", None)
    t0 = time.perf_counter()
    try:
        if os.path.exists(path):
            os.unlink(path)
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_configs.py")], cwd=ROOT, env=env,
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=timeout_s)
        if run.returncode != 0 or not os.path.exists(path):
            return {"error": f"tools/bench_configs.py rc={run.returncode}: {run.stderr[-300:]}"}
        with open(path) as fh:
            raw = json.load(fh)
    except Exception as exc:  # noqa: BLE001 -- a secondary leg must not cost the headline
        return {"error": repr(exc)[:300]}

    def dominant(kernels):
        best = max(kernels.items(), key=lambda kv: kv[1]["launches_per_step"] * kv[1]["ms_per_launch"])
        return best[0], best[1]

    def entry(rec, ms, gbps_key, what):
        name, k = dominant(rec["kernels"])
        gbps = rec.get(gbps_key) if gbps_key else None
        return {"workload": what, "ms_per_step": ms, "dominant_kernel_class": name,
                "dominant_kernel_ms_per_step": k["launches_per_step"] * k["ms_per_launch"],
                "dominant_kernel_launches_per_step": k["launches_per_step"],
                "spmm_algorithmic_GBps": gbps, "frac": (gbps / HBM_PEAK_GBS) if gbps else None,
                "gathered_set_MiB": rec.get("gathered_set_MiB")}
    out = {}
    r = raw.get("C2_magnetconv_100k_2M_h64")
    if r:
        out["C2"] = entry(r, r["ms_per_step"], "spmm2_alg_GBps", "MagNetConv K=1 h=64 fp32, DSBM 100k nodes / 2M edges")
    r = raw.get("C3_sgcnconv_first")
    if r:
        out["C3a"] = entry(r, r["ms_per_step"], "spmm_alg_GBps_fwd_pair", "SGCNConv first_aggr h=64 fp32, SSBM 500k nodes / 10M signed entries")
    r = raw.get("C3_simpa_hop2")
    if r:
        out["C3b"] = entry(r, r["ms_per_step"], "spmm_alg_GBps", "SIMPA hop 2 h=64 fp32, SSBM 500k nodes / 10M signed entries")
    r = raw.get("C4_msconv_1M_20M_h128_K2_1gpu")
    if r:
        out["C4_one_gpu"] = entry(r, r["ms_per_step"], "spmm2_alg_GBps", "MSConv K=2 h=128 fp32, SDSBM 1M nodes / 20M edges, on ONE GPU")
    c5 = raw.get("C5_digcn_inception_block_1gpu") or {}
    for tag, key, label in (("C5a", "float32", "fp32"), ("C5b", "bfloat16", "bf16")):
        r = c5.get(key)
        if r:
            out[tag] = entry(r, r["ms_per_block_step"], "spmm_alg_GBps",
                             f"DiGCN_InceptionBlock h=64 {label}, 2M nodes / {r.get('nnz_per_operator')} entries per operator, on ONE GPU")
    out["seconds"] = time.perf_counter() - t0
    out["note"] = ("fwd+bwd per step, eager, operator cached, 10 (C5: 5) steps after warm-up, in a child process of this run "
                   "(tools/bench_configs.py, compact mode); frac = the SpMM's algorithmic bytes (SURVEY.md 8(d): every operand "
                   "read once, every result written once) / its average launch / 8 TB/s -- at or below a 256 MiB gathered set "
                   "that is an on-die rate, not a DRAM rate")
    return out


def rccl_version():
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(t) for t in v) if isinstance(v, tuple) else str(v)
    except Exception:  # noqa: BLE001
        return None


def device_identities(dist, device):
    """One record per rank -- host, process, HIP device index, device name, UUID and PCI bus id -- gathered over the process
    group, so that a multi-GPU line proves by itself that its N ranks ran on N distinct GPUs."""
    props = torch.cuda.get_device_properties(device)
    me = {"rank": dist.get_rank(), "host": socket.gethostname(), "pid": os.getpid(), "device_index": device.index,
          "name": props.name, "uuid": str(getattr(props, "uuid", None)),
          "pci_bus_id": (f"{getattr(props, 'pci_domain_id', 0):04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}"
                         if hasattr(props, "pci_bus_id") else None),
          "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES")}
    try:                                  # (an identity record must never cost the run its result line)
        box = [None] * dist.get_world_size()
        dist.all_gather_object(box, me)
        distinct = len({(r["host"], r["uuid"], r["pci_bus_id"]) for r in box})
        return {"ranks": box, "distinct_devices": distinct}
    except Exception as exc:  # noqa: BLE001
        return {"ranks": [me], "distinct_devices": None, "error": repr(exc)[:200]}


def stream_copy_rate(device, gib=1.0, reps=7):
    """GB/s (read + write) of the library's streaming float4 copy on `gib` GiB: the achievable-HBM yardstick."""
    from pytorch_geometric_signed_directed_amd import _cabi
    n = int(gib * (1 << 30)) // 4
    src = torch.empty(n, dtype=torch.float32, device=device).normal_()
    dst = torch.empty_like(src)
    lib = _cabi.lib()
    times = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _cabi.check(lib.pygsd_stream_copy_f32(_cabi.ptr(src), _cabi.ptr(dst), n, _cabi.stream_ptr()), "pygsd_stream_copy_f32")
        b.record()
        b.synchronize()
        if k >= 2:
            times.append(a.elapsed_time(b))
    assert torch.equal(src[:1024], dst[:1024])
    return 2.0 * n * 4 / (statistics.median(times) * 1e-3) / 1e9


def measure_traffic(args, kernel_substring="spmm_vec_kernel"):
    """HBM-side bytes per launch of the dominant kernel, measured NOW: two rocprofv3 passes (FETCH_SIZE, then WRITE_SIZE --
    counters only, one pass each, as MI355X_MICROARCH.md prescribes: they do not fit one pass) over a 3-step child run of
    this script on the same workload.  The counters are in KiB; on gfx950 FETCH_SIZE tallies the 128-byte requests of wide
    reads as 64 bytes, so fetched bytes = FETCH_SIZE x 1024 x 2; WRITE_SIZE x 1024 as is.  -> (bytes, note) or (None, why)."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    child = [sys.executable, os.path.abspath(__file__), "--no-cpu-baseline", "--no-pmc", "--no-x4", "--no-configs", "--steps", "3",
             "--warmup", "1",
             "--nodes", str(args.nodes), "--edges", str(args.edges), "--hidden", str(args.hidden)]
    env = dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    means = {}
    work = tempfile.mkdtemp(prefix="pygsd_pmc_")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out_dir = os.path.join(work, counter)
            run = subprocess.run([exe, "--pmc", counter, "--output-format", "csv", "-d", out_dir, "-o", "b", "--"] + child,
                                 env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
            if run.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} exited {run.returncode}: {run.stderr[-200:]}"
            per = {}
            for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    # the DUAL variant of the vector SpMM (template arguments <LPR, dual = true, deep>)
                    if (kernel_substring in row["Kernel_Name"] and "true," in row["Kernel_Name"].split(kernel_substring)[1][:24]
                            and row["Counter_Name"] == counter):
                        key = row["Dispatch_Id"]
                        per[key] = per.get(key, 0.0) + float(row["Counter_Value"])
            if not per:
                return None, f"no {counter} samples of {kernel_substring} in the child run"
            vals = sorted(per.values())
            means[counter] = (sum(vals) / len(vals), len(vals))
        total = (means["FETCH_SIZE"][0] * 2.0 + means["WRITE_SIZE"][0]) * 1024.0
        note = (f"MEASURED IN THIS RUN: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes, counters only) over a "
                f"3-step child run of this command; mean over {means['FETCH_SIZE'][1]} / {means['WRITE_SIZE'][1]} launches of "
                f"the dual SpMM; bytes = FETCH_SIZE x 1024 x 2 (gfx950 tallies 128-byte requests as 64) + WRITE_SIZE x 1024 "
                f"(MI355X_MICROARCH.md, HBM section)")
        return total, note
    except Exception as exc:  # noqa: BLE001 -- a measurement aid must not cost the result line
        return None, f"{type(exc).__name__}: {exc}"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def self_launch(args_list, gpus):
    """`python bench.py --gpus N` typed by hand: re-execute under torch.distributed.run, one rank per GPU."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + args_list
    return subprocess.call(cmd, env=env)


def dram_bound_replay():
    """Fallback only: the x4 figure REPLAYED from a separate, tracked capture (tools/northstar_x4.py ->
    profiles/r4_northstar_x4.json); null if the file is missing."""
    path = os.path.join(ROOT, "profiles", "r4_northstar_x4.json")
    try:
        rec = json.load(open(path))
        k = rec["dual_spmm"]
        return {"source": "profiles/r4_northstar_x4.json (tools/northstar_x4.py, a separate run -- replayed, not measured here)",
                "measured_in_this_run": False,
                "workload": rec["workload"], "gathered_set_GiB": rec["gathered_set_GiB"],
                "achieved": k["algorithmic_GBps"], "frac": k["fraction_of_8TBps"],
                "streaming_copy_GBps_same_run": k["streaming_copy_GBps_same_run"],
                "frac_of_streaming_copy": k["fraction_of_streaming_copy"], "ms_per_launch": k["ms_per_launch"]}
    except (OSError, KeyError, ValueError):
        return None


def dram_bound_reference(device, hidden, copy_rate, scale=4, steps=6):
    """The same layer and kernel where the gathered set is 8x the Infinity Cache (DSBM `scale` x 1M nodes / `scale` x 20M edges:
    2 x 4M x 64 x 4 B = 1.9 GiB gathered) -- a DRAM-bound fraction beside the fabric-side `frac` of the headline, MEASURED IN
    THIS RUN (round 5; rounds 3-4 replayed a separate capture): graph sampled on the host (~10 s), operator built once, 2 warm-up
    + `steps` fwd+bwd steps with the per-launch recorder on.  Any failure falls back to the tracked replay, labelled so."""
    from pytorch_geometric_signed_directed_amd import _cabi, graphs
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv
    try:
        n, e_target = 1000000 * scale, 20000000 * scale
        t0 = time.perf_counter()
        ei_np, _, p = graphs.dsbm_for_edges(n, e_target, seed=1)
        ei = torch.from_numpy(ei_np).to(device)
        del ei_np
        gen_s = time.perf_counter() - t0
        g = torch.Generator().manual_seed(0)
        xr = torch.randn(n, hidden, generator=g).to(device).requires_grad_()
        xi = torch.randn(n, hidden, generator=g).to(device).requires_grad_()
        torch.manual_seed(0)
        layer = MagNetConv(hidden, hidden, K=1, q=0.25, trainable_q=False, cached=True).to(device)

        def step():
            layer.zero_grad(set_to_none=True)
            xr.grad = xi.grad = None
            o_r, o_i = layer(xr, xi, ei)
            (o_r.sum() + o_i.sum()).backward()

        for _ in range(2):
            step()
        torch.cuda.synchronize(device)
        _cabi.prof_reset()
        _cabi.prof_enable(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(device)
        ms = (time.perf_counter() - t0) / steps * 1e3
        _cabi.prof_enable(False)
        launches, total_ms = _cabi.prof_collect("spmm2")
        _cabi.prof_reset()
        nnz = layer._operator.nnz
        alg = spmm_bytes(nnz, n, hidden) + spmm_bytes(nnz - n, n, hidden)
        per_launch = total_ms / max(launches, 1)
        gbps = alg / per_launch / 1e6
        e = int(ei.size(1))
        del layer, xr, xi, ei
        torch.cuda.empty_cache()
        return {"source": "MEASURED IN THIS RUN (bench.py::dram_bound_reference): same layer, same kernel, graph x" + str(scale),
                "measured_in_this_run": True,
                "workload": f"MagNetConv K=1 q=0.25 sym cached, DSBM {n} nodes / {e} edges (p={p:.3e}), h={hidden}, fp32, fwd+bwd",
                "gathered_set_GiB": 2 * n * hidden * 4 / 2 ** 30, "infinity_cache_MiB": 256,
                "operator_nnz": int(nnz), "steps": steps, "ms_per_step": ms, "edges_per_s": e / ms * 1e3,
                "launches": int(launches), "ms_per_launch": per_launch, "algorithmic_bytes_per_launch": alg,
                "achieved": gbps, "frac": gbps / HBM_PEAK_GBS,
                "streaming_copy_GBps_same_run": copy_rate,
                "frac_of_streaming_copy": gbps / copy_rate if copy_rate else None,
                "graph_generation_s": gen_s}
    except Exception as exc:  # noqa: BLE001 -- a side measurement must not cost the result line
        rec = dram_bound_replay()
        if rec is not None:
            rec["source"] = f"live x{scale} run failed ({type(exc).__name__}: {exc}); " + rec["source"]
        return rec


def exchange_report(args, layer_s, xr_loc, xi_loc, dist, device, world, hidden, sync, reduce_max, fallback_note):
    """The `exchange` object of a sharded run: schedule, per-propagate compute-stream split (the engine's timing of the
    instrumented pass), every collective of one propagate timed ALONE, and who ran where (world size, RCCL version, one device
    identity per rank)."""
    summary = layer_s.engine.timing_summary() or {}
    layer_s.engine.profile(False)
    # the exchanges alone (nothing to overlap with): every collective of one propagate timed on its own -- the
    # first multi-GPU run calibrates the link rate the single-GPU rehearsal assumed (61 GB/s per direction)
    eng = layer_s.engine
    esz = xr_loc.element_size()

    def timed_collective(fn):
        ts = []
        for _ in range(5):
            sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn().wait()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return reduce_max(statistics.median(ts))

    inbound_ms, return_ms, in_bytes_per_link, back_bytes_per_link = [], [], [], []
    for c in range(eng.phases):                       # (the pieces may be uneven: round 5's default schedule)
        send_c = eng._pack([xr_loc.detach(), xi_loc.detach()], c).clone()
        buf_c = send_c.new_empty((world, eng.phase_rows[c], send_c.size(-1)))
        inbound_ms.append(timed_collective(lambda: eng.ex.all_to_all(buf_c, send_c) if eng.grid
                                           else eng.ex.all_gather(buf_c, send_c)))
        in_bytes_per_link.append((send_c[0].numel() if eng.grid else send_c.numel()) * esz)
    if eng.grid:
        fw2 = 2 * (hidden // eng.p_c)
        for r in range(eng.return_chunks):
            back = xr_loc.new_zeros((world, eng.chunk_rows[r], fw2))
            recv = torch.empty_like(back)
            back_bytes_per_link.append(back[0].numel() * esz)
            return_ms.append(timed_collective(lambda: eng.ex.all_to_all(recv, back)))
    alone_total = sum(inbound_ms) + sum(return_ms)

    def rate(nbytes, ms):
        return nbytes / (ms * 1e-3) / 1e9 if ms and world > 1 else None
    exchange = {"layout": layer_s.layout, "p_r": eng.p_r, "p_c": eng.p_c, "phases": eng.phases,
                "return_chunks": eng.return_chunks, "phase_rows": eng.phase_rows,
                "return_chunk_rows": eng.chunk_rows if eng.grid else None, "propagates_per_step": 2,
                "propagate_ms": summary.get("total_ms"), "product_ms": summary.get("product_ms"),
                "pack_ms": summary.get("pack_ms"), "merge_ms": summary.get("merge_ms"),
                "exposed_exchange_ms": summary.get("exposed_exchange_ms"),
                "exchange_alone_ms": alone_total,
                "collectives_alone": {
                    "inbound_ms_per_phase": inbound_ms, "inbound_bytes_per_link": in_bytes_per_link,
                    "inbound_GBps_per_link": [rate(b, t) for b, t in zip(in_bytes_per_link, inbound_ms)],
                    "return_ms_per_chunk": return_ms, "return_bytes_per_link": back_bytes_per_link,
                    "return_GBps_per_link": [rate(b, t) for b, t in zip(back_bytes_per_link, return_ms)],
                    "assumed_by_the_rehearsal_GBps_per_link": 61.0},
                "cache_input_exchange": bool(args.cache_input_exchange),
                "backend": dist.get_backend(), "world_size": dist.get_world_size(), "devices": device_identities(dist, device),
                "rccl_version": rccl_version(),
                "blocking_collectives": bool(getattr(layer_s.exchange, "synchronous", False)),
                "TORCH_NCCL_AVOID_RECORD_STREAMS": os.environ.get("TORCH_NCCL_AVOID_RECORD_STREAMS"),
                "fallback": fallback_note,
                "node_range_sizes": layer_s.plan.sizes, "n_pad": layer_s.plan.n_pad,
                "note": "per propagate, compute-stream time of rank 0: product = partial SpMM launches, exposed = "
                        "the compute stream waiting for an inbound phase or the return; exchange_alone = the same "
                        "collectives with nothing to overlap"}
    return exchange


def dump_outputs(directory, n, row_arrays, params, rank, device, plan=None, exchange=None):
    """--dump-outputs: `row_arrays` (name -> [rows, F] tensor: all N rows, or with `plan` this rank's local rows) and `params`
    (name -> tensor, the same on every rank) -> directory/<name>.npy in float32, written by rank 0.  The row arrays are written
    whole if they fit in DUMP_BYTES beside the rest, else on DUMP_SEED's sample of rows, sorted.  Sharded, every rank fills the
    sampled rows it owns and the rows are summed over the ranks (each row is owned by exactly one)."""
    import numpy as np
    names = list(row_arrays)
    widths = [row_arrays[k].size(1) for k in names]
    fit = max(1, (DUMP_BYTES - sum(4 * p.numel() for p in params.values())) // (4 * sum(widths)))
    if n <= fit:
        rows = torch.arange(n)
    else:
        rows = torch.sort(torch.randperm(n, generator=torch.Generator().manual_seed(DUMP_SEED))[:fit]).values
    if plan is None:
        idx = rows.to(device)
        got = [row_arrays[k].detach()[idx].float() for k in names]
    else:
        mine = (rows >= plan.lo) & (rows < plan.hi)
        loc = (rows[mine] - plan.lo).to(device)
        packed = torch.zeros((rows.numel(), sum(widths)), dtype=torch.float32, device=device)
        packed[mine.to(device)] = torch.cat([row_arrays[k].detach()[loc].float() for k in names], dim=1)
        exchange.all_reduce(packed)
        got = packed.split(widths, dim=1)
    if rank != 0:
        return
    os.makedirs(directory, exist_ok=True)
    for name, t in list(zip(names, got)) + list(params.items()):
        np.save(os.path.join(directory, name + ".npy"), t.detach().float().cpu().numpy())


def parity_guard(layer_s, xr_loc, xi_loc, x_real, x_imag, edge_index, n, hidden, rank, device):
    """Un-timed parity guard of the sharded mode: sampled rows of the sharded outputs and input gradients, and the
    all-reduced dW / db, against the UN-SHARDED HIP layer run on rank 0 with the same parameters (that layer is held
    to a float64 evaluation at this size by tests/test_gpu_fullsize.py).  In the JSON line; rc != 0 above the bar.
    """
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv
    parity = None
    k_rows = min(1024, n)
    gen = torch.Generator().manual_seed(12345)
    rows = torch.sort(torch.randperm(n, generator=gen)[:k_rows]).values
    layer_s.zero_grad(set_to_none=True)
    xr_loc.grad = xi_loc.grad = None
    o_r, o_i = layer_s(xr_loc, xi_loc)
    (o_r.sum() + o_i.sum()).backward()
    plan = layer_s.plan
    mine = (rows >= plan.lo) & (rows < plan.hi)
    loc = (rows[mine] - plan.lo).to(device)
    got = torch.zeros((k_rows, 4 * hidden), dtype=torch.float32, device=device)
    got[mine.to(device)] = torch.cat([t.detach()[loc] for t in (o_r, o_i, xr_loc.grad, xi_loc.grad)], dim=1)
    layer_s.exchange.all_reduce(got)                  # every sampled row is owned by exactly one rank
    if rank == 0:
        ref = MagNetConv(hidden, hidden, K=1, q=0.25, trainable_q=False, cached=True).to(device)
        with torch.no_grad():
            ref.weight.copy_(layer_s.weight)
            ref.bias.copy_(layer_s.bias)
        a = x_real.detach().clone().requires_grad_()
        b = x_imag.detach().clone().requires_grad_()
        w_r, w_i = ref(a, b, edge_index)
        (w_r.sum() + w_i.sum()).backward()
        idx = rows.to(device)
        want = torch.cat([t.detach()[idx] for t in (w_r, w_i, a.grad, b.grad)], dim=1).double()
        d = (got.double() - want).abs()
        mixed = float((d / (1.0 + want.abs())).max())

        def norm_err(x, y):
            return float((x.double() - y.double()).abs().max()) / max(1.0, float(y.abs().max()))
        dw_err = norm_err(layer_s.weight.grad, ref.weight.grad)
        db_err = norm_err(layer_s.bias.grad, ref.bias.grad)
        ok = mixed <= 1e-5 and dw_err <= 1e-5 and db_err <= 1e-5
        parity = {"ok": ok, "rows": int(k_rows), "max_err_rows": mixed, "max_abs_err_rows": float(d.max()),
                  "max_abs_want": float(want.abs().max()), "dW_norm_err": dw_err, "db_norm_err": db_err,
                  "bar": "|d| <= 1e-5 (1 + |want|) per element of out_real / out_imag / dx_real / dx_imag on the "
                         "sampled rows; max-norm 1e-5 for dW / db", "against": "un-sharded HIP MagNetConv on rank 0, "
                         "same parameters, same inputs (float64-verified at this size by tests/test_gpu_fullsize.py)",
                  "operator_nnz_matches": bool(layer_s.global_nnz == ref._operator.nnz)}
        parity["ok"] = bool(parity["ok"] and parity["operator_nnz_matches"])
        del ref, a, b, w_r, w_i
    return parity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--edges", type=int, default=20000000)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--layout", choices=("auto", "rows", "grid"), default="auto",
                    help="multi-GPU work layout (parallel.ShardedMagNetConv): rows = all-gather of whole feature "
                         "blocks, grid = p_r x p_c process grid with column-slice all-to-alls (auto picks grid "
                         "above two ranks)")
    ap.add_argument("--phases", default=None,
                    help="column phases of the pipelined propagate: a count (equal pieces) or fractions, e.g. 0.4,0.6 "
                         "(default: parallel.DEFAULT_PHASES)")
    ap.add_argument("--return-chunks", default=None,
                    help="row chunks of the grid's return: a count or fractions, e.g. 0.5,0.36,0.14 (default: "
                         "parallel.DEFAULT_RETURN_CHUNKS)")
    ap.add_argument("--grid-cols", type=int, default=None,
                    help="column slices of the grid (default: chosen from the world size); 1 with --layout grid runs the "
                         "grid SCHEDULE (all-to-all in, row-chunked all-to-all back) on one slice -- with --force-sharded "
                         "the whole pipeline over RCCL on a single rank")
    ap.add_argument("--force-sharded", action="store_true",
                    help="use the node-sharded layer even with one rank (exercises the RCCL path on 1 GPU)")
    ap.add_argument("--no-parity", action="store_true", help="skip the un-timed parity guard of the sharded mode")
    ap.add_argument("--cache-input-exchange", action="store_true",
                    help="sharded mode, OFF by default: memoise the forward propagate's inbound exchange while the input features are "
                         "the same tensors at the same version (a first layer's features do not change between training steps); "
                         "recorded in the `exchange` object -- the default line repeats every exchange in every step")
    ap.add_argument("--no-x4", action="store_true",
                    help="do not run the DRAM-bound x4 graph (4M nodes / 80M edges, ~25 s) that feeds "
                         "`roofline.dram_bound_reference`; the tracked capture is replayed instead, labelled so")
    ap.add_argument("--no-configs", action="store_true",
                    help="do not time the other single-GPU BASELINE configurations (C2, C3a, C3b, C4 on one GPU, C5a, C5b; ~40 s in a "
                         "child process) into the line's `configs` object")
    ap.add_argument("--cpu-baseline-northstar", action="store_true",
                    help="run the CPU baseline at the NORTH-STAR size as well (1M nodes / 20M edges: ~100 GB of host memory, "
                         "minutes) -> `cpu_baseline.northstar`; run once into profiles/, not part of the default line")
    ap.add_argument("--no-pmc", action="store_true",
                    help="do not measure `roofline.traffic` live (two rocprofv3 --pmc passes of a short child run of this "
                         "script); the value is then replayed from profiles/pmc_traffic.json and labelled so")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary legs: the dense-gradient and exact-fp32 passes (K steps each), the x4 "
                         "DRAM-bound graph, the other BASELINE configurations, live PMC traffic and the CPU baseline "
                         "(about a minute more; --no-x4 / --no-configs / --no-pmc / --no-cpu-baseline drop single legs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (out_real, out_imag, grad_x_real, "
                         "grad_x_imag, grad_weight, grad_bias) as DIR/<name>.npy in float32, the [N, F] arrays on a fixed, "
                         "seeded sample of rows (at most 48 MiB in all), e.g. --dump-outputs bench_outputs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    # Only the JSON line may reach stdout.  RCCL prints a version banner through C stdio on stdout (flushed at
    # exit, i.e. AFTER the result line), so the real stdout is kept aside for the result and fd 1 is pointed at
    # stderr for everything else (C libraries and stray prints alike).
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the HIP path)")
    if os.environ.get("PYGSD_BENCH_SHARE_GPU") == "1":   # test hook: all ranks on cuda:0 (needs the gloo backend)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    sharded = world > 1 or args.force_sharded
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import datetime
        backend = os.environ.get("PYGSD_DIST_BACKEND", "nccl")   # "nccl" is RCCL on ROCm
        # the engine keeps its exchange buffers for its own lifetime and orders their reuse with events, so the
        # allocator need not be told about the communication stream (record_stream would pin blocks until that
        # stream's events retire); recorded in the `exchange` object
        os.environ.setdefault("TORCH_NCCL_AVOID_RECORD_STREAMS", "1")
        limit = datetime.timedelta(seconds=int(os.environ.get("PYGSD_DIST_TIMEOUT_S", "300")))   # a hang becomes an error
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device, timeout=limit)
        else:
            dist.init_process_group(backend, timeout=limit)

    from pytorch_geometric_signed_directed_amd import _cabi
    from pytorch_geometric_signed_directed_amd.nn import MagNetConv

    n, hidden = args.nodes, args.hidden
    edge_index, x_real, x_imag, p = build_inputs(n, args.edges, hidden, device)
    e = edge_index.size(1)
    torch.manual_seed(0)
    layer_s = None
    dense_g = {}

    def backward(o_r, o_i, loss):
        """"sum": the headline's loss: out_real.sum() + out_imag.sum() -- autograd hands the layer ONE gradient
        row broadcast over the nodes, which the dense backward reads with row stride 0.  "dense": a dense [N, F] upstream
        gradient per output, as a real training loss delivers (examples/magnet_node.py:22-27: NLL over log-softmax), handed to
        the layer as is (g ~ N(0, 1), resident before the timed region): the layer's own cost with nothing broadcast.
        "dense_loss": the same gradient through a loss inside the step, (o_r * g_r).sum() + (o_i * g_i).sum() -- its two
        products, two reductions and two gradient products are timed with the layer."""
        if loss == "sum":
            (o_r.sum() + o_i.sum()).backward()
            return
        key = tuple(o_r.shape)
        if key not in dense_g:
            gen = torch.Generator(device=o_r.device).manual_seed(777)
            dense_g[key] = (torch.randn(o_r.shape, generator=gen, device=o_r.device),
                            torch.randn(o_i.shape, generator=gen, device=o_i.device))
        g_r, g_i = dense_g[key]
        if loss == "dense":
            torch.autograd.backward((o_r, o_i), (g_r, g_i))
        else:
            ((o_r * g_r).sum() + (o_i * g_i).sum()).backward()
    if not sharded:
        layer = MagNetConv(hidden, hidden, K=1, q=0.25, trainable_q=False, cached=True).to(device)
        x_real.requires_grad_()
        x_imag.requires_grad_()

        def step(loss="sum"):
            layer.zero_grad(set_to_none=True)
            x_real.grad = x_imag.grad = None
            o_r, o_i = layer(x_real, x_imag, edge_index)
            backward(o_r, o_i, loss)
            return o_r, o_i

        def op_nnz():
            return layer._operator.nnz
    else:
        from pytorch_geometric_signed_directed_amd.parallel import DistExchange, ShardedMagNetConv
        fallback_note = None

        def make_sharded(layout, phases, chunks, synchronous):
            ls = ShardedMagNetConv(hidden, hidden, K=1, q=0.25, num_nodes=n, edge_index=edge_index, edge_weight=None,
                                   device=device, layout=layout, phases=phases, return_chunks=chunks,
                                   grid_cols=args.grid_cols, exchange=DistExchange(synchronous=synchronous),
                                   cache_input_exchange=args.cache_input_exchange)
            a = ls.shard_rows(x_real).requires_grad_()
            b = ls.shard_rows(x_imag).requires_grad_()
            return ls, a, b

        def sharded_step(ls, a, b, loss="sum"):
            ls.zero_grad(set_to_none=True)
            a.grad = b.grad = None
            o_r, o_i = ls(a, b)
            backward(o_r, o_i, loss)
            return o_r, o_i

        def agree(failed: bool) -> bool:
            """True if ANY rank failed (decided over a gloo side group: it must work when RCCL does not)."""
            if world == 1:
                return failed
            flag = torch.tensor([1.0 if failed else 0.0])
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=control)
            return bool(flag.item())

        control = dist.new_group(backend="gloo") if (world > 1 and dist.get_backend() != "gloo") else None
        if world > 1 and control is None:
            control = dist.group.WORLD
        err = None
        try:
            from pytorch_geometric_signed_directed_amd.parallel import split_spec

            def spec(raw):
                if raw is None:
                    return None
                count, fracs = split_spec(raw)
                return fracs if fracs is not None else count
            layer_s, xr_loc, xi_loc = make_sharded(args.layout, spec(args.phases), spec(args.return_chunks), False)
            sharded_step(layer_s, xr_loc, xi_loc)
            torch.cuda.synchronize(device)
        except Exception as exc:  # noqa: BLE001 -- an RCCL failure of the pipelined schedule must not cost the whole run
            err = f"{type(exc).__name__}: {exc}"
        if agree(err is not None):
            # the asynchronous grid schedule failed somewhere: one blocking all-gather per propagate instead, reason kept
            fallback_note = ("pipelined schedule failed (" + (err or "on another rank") + "); fell back to the row layout, "
                             "one phase, blocking collectives")
            sys.stderr.write("bench.py: " + fallback_note + "\n")
            layer_s, xr_loc, xi_loc = make_sharded("rows", 1, 1, True)

        def step(loss="sum"):
            return sharded_step(layer_s, xr_loc, xi_loc, loss)

        def op_nnz():
            return layer_s.global_nnz

    def sync():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(device)

    def reduce_max(v):
        if dist is None:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=device)
        if dist.get_backend() == "gloo":
            t = t.cpu()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for _ in range(args.warmup):
        step()
    # ---- pass 1: the headline.  K steps between barriers; per-step HIP events; no per-launch recorder.
    sync()
    marks = []
    t0 = time.perf_counter()
    for k in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if k + 1 < args.steps:
            step()
        else:
            last = step()                    # the last step's outputs (--dump-outputs); earlier ones are not kept
        b.record()
        marks.append((a, b))
    sync()
    dt = reduce_max(time.perf_counter() - t0)
    per_step = [a.elapsed_time(b) for a, b in marks]
    med = reduce_max(statistics.median(per_step))
    if args.dump_outputs:
        # the gradients are still the last timed step's: every step sets them anew (zero_grad(set_to_none=True))
        lyr, xr_, xi_ = (layer, x_real, x_imag) if layer_s is None else (layer_s, xr_loc, xi_loc)
        params = {"grad_weight": lyr.weight.grad}
        if lyr.bias is not None:
            params["grad_bias"] = lyr.bias.grad
        dump_outputs(args.dump_outputs, n, {"out_real": last[0], "out_imag": last[1], "grad_x_real": xr_.grad,
                                            "grad_x_imag": xi_.grad}, params, rank, device,
                     plan=None if layer_s is None else layer_s.plan, exchange=None if layer_s is None else layer_s.exchange)
    last = None

    # ---- pass 1b / 1c (labelled, beside the headline): the same K steps with a DENSE upstream gradient, so that the
    # headline does not lean on its loss: `out.sum()` lets the dense backward read one broadcast row (ldg = 0) where a real
    # loss delivers [N, F] per output (+2 N F 4 B of reads per step).
    def timed_pass(loss):
        for _ in range(2):
            step(loss)
        sync()
        t_begin = time.perf_counter()
        for _ in range(args.steps):
            step(loss)
        sync()
        return reduce_max(time.perf_counter() - t_begin) / args.steps * 1e3

    ms_dense = ms_dense_loss = ms_exact = None
    if args.full:
        ms_dense = timed_pass("dense")
        ms_dense_loss = timed_pass("dense_loss")
        dense_g.clear()
        # ---- pass 1d (labelled): the headline's K steps with every dense product as an fp32 fmaf chain on
        # v_mfma_f32_16x16x4_f32.  The dense stage runs by default on the bf16 matrix pipe with its fp32 operands split three
        # ways (include/pygsd_hip.h: pygsd_dense_f32_form): fp32-accurate (closer to float64 than the chain, DESIGN.md
        # section 7), not a reduced precision -- the line carries both so that nobody has to take that on trust.
        from pytorch_geometric_signed_directed_amd.dense import set_dense_f32_exact
        was_exact = set_dense_f32_exact(True)
        try:
            ms_exact = timed_pass("sum")
        finally:
            set_dense_f32_exact(was_exact)
        step()                               # back on the headline's loss for the instrumented pass

    # ---- pass 2 (untimed): per-launch recorder and propagate instrumentation on.
    prof_steps = min(args.steps, PROF_STEPS)
    _cabi.prof_reset()
    _cabi.prof_enable(True)
    if layer_s is not None:
        layer_s.engine.profile(True)
    sync()
    for _ in range(prof_steps):
        step()
    sync()
    _cabi.prof_enable(False)
    launches, kernel_ms = _cabi.prof_collect("spmm2")
    other = {k: _cabi.prof_collect(k) for k in ("dense", "dense_bwd")}
    _cabi.prof_reset()
    exchange = None
    if layer_s is not None:
        exchange = exchange_report(args, layer_s, xr_loc, xi_loc, dist, device, world, hidden, sync, reduce_max, fallback_note)
    parity = None
    if layer_s is not None and not args.no_parity:
        parity = parity_guard(layer_s, xr_loc, xi_loc, x_real, x_imag, edge_index, n, hidden, rank, device)
    if rank == 0:
        nnz = op_nnz()                      # E_s + N (folded diagonal)
        e_s = nnz - n
        parallelism = "single GPU"
        launches_per_product = 1
        if layer_s is not None:
            eng = layer_s.engine
            launches_per_product = eng.phases - 1 + (eng.return_chunks if eng.grid else 1)
            parallelism = (f"node-range ownership x{world} (equal-work ranges), {layer_s.layout} layout"
                           + (f" {eng.p_r} x {eng.p_c} grid" if eng.grid else "")
                           + f", {eng.phases} column phases" + (f" x {eng.return_chunks} return chunks" if eng.grid else "")
                           + ", exchanges overlapped with the partial products (RCCL)")
        if layer_s is None:
            # one fused launch = the real SpMM (E_s + N entries) + the imaginary SpMM (E_s entries)
            alg_total = (spmm_bytes(nnz, n, hidden) + spmm_bytes(e_s, n, hidden)) * launches
        else:
            # a rank's launches of one product together traverse its row block once: entries / p_r at width F / p_c
            eng = layer_s.engine
            rows, width = eng.block_rows, hidden // eng.p_c
            loc = layer_s.local_nnz
            per_product = spmm_bytes(loc, rows, width) + spmm_bytes(max(loc - rows, 0), rows, width)
            alg_total = per_product * (launches / max(launches_per_product, 1))
        avg_ms = kernel_ms / max(launches, 1)
        achieved = alg_total / (kernel_ms * 1e-3) / 1e9 if launches else 0.0
        copy_rate = stream_copy_rate(device)
        traffic, traffic_source = None, None
        if layer_s is None and args.full and not args.no_pmc:
            traffic, traffic_source = measure_traffic(args)
            if traffic is None:
                traffic_source = "live PMC measurement failed (" + str(traffic_source) + "); "
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if traffic is None and os.path.exists(pmc) and layer_s is None:
            with open(pmc) as fh:
                rec = json.load(fh)
            if rec.get("nodes") == n and rec.get("hidden") == hidden and rec.get("n_gpus", 1) == world:
                traffic = rec.get("hbm_bytes_per_launch")
                traffic_source = ((traffic_source or "") + "profiles/pmc_traffic.json -- REPLAYED from a separate rocprofv3 "
                                  "--pmc run of this command (tools/capture_profiles.sh), not measured in this run: "
                                  + str(rec.get("source", "")))
        line = {
            "metric": "edges/sec (fwd+bwd) MagNetConv, 1M nodes/20M edges, h=64; % HBM roofline",
            "value": e * args.steps / dt,
            "unit": "edges/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "ms_per_step_median": med,
            "ms_per_step_min": min(per_step),
            "ms_per_step_max": max(per_step),
            "value_at_median": e / (med * 1e-3),
            "ms_per_step_dense_grad": ms_dense,
            "value_dense_grad": e / (ms_dense * 1e-3) if ms_dense else None,
            "ms_per_step_dense_grad_with_loss": ms_dense_loss,
            "dense_grad_note": "same K steps, operator cached, with a dense [N, F] upstream gradient per output (g ~ N(0,1), "
                               "resident) instead of the broadcast row that `out.sum()` hands the layer: `ms_per_step_dense_grad` "
                               "= torch.autograd.backward((o_r, o_i), (g_r, g_i)) -- the layer alone, as under a real loss "
                               "(examples/magnet_node.py:22-27); `..._with_loss` = ((o_r*g_r).sum() + (o_i*g_i).sum()).backward(), "
                               "the loss's own element-wise passes timed with it",
            "ms_per_step_exact_fp32_dense": ms_exact,
            "value_exact_fp32_dense": e / (ms_exact * 1e-3) if ms_exact else None,
            "dense_arithmetic_note": "fp32 storage, fp32 accumulation everywhere.  Headline: the dense stage's products (forward and "
                                     "backward) run on the bf16 matrix pipe with each fp32 operand split into three bf16 pieces and "
                                     "the six largest partial products kept -- error vs float64 relative to the sum of |terms|: "
                                     "forward 4.6e-8 (fp32 fmaf chain 2.4e-7), backward dA / dB 0.9e-7 (chain 3.0e-7): "
                                     "profiles/r5s_dense_fwd_forms.json, r5p_dense_bwd_forms.json -- the library's default; "
                                     "`ms_per_step_exact_fp32_dense` = the same K steps with fmaf chains on the exact fp32 MFMA "
                                     "(PYGSD_DENSE_F32=exact).  The SpMM is plain fp32 in both",
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"MagNetConv K=1 q=0.25 sym cached, DSBM(5 clusters, cyclic eta=0.1, "
                                   f"size_ratio 1.5, p={p:.3e}) {n} nodes / {e} edges, h={hidden}, fp32",
                       "nodes": n, "edges": e, "hidden": hidden, "operator_nnz": int(nnz),
                       "parallelism": parallelism},
            "roofline": {"bound": "hbm",
                         "kernel": "spmm_vec_kernel<LPR, dual, deep> (pygsd_spmm2_csr_f32)",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS,
                         "achievable_peak": copy_rate,
                         "frac_of_achievable": achieved / copy_rate if copy_rate else None,
                         "limiter": "L2-miss (fabric) traffic served by Infinity Cache + HBM together: the gathered "
                                    "feature set (2 x N x F x 4 B) is of the order of the 256 MiB Infinity Cache, so "
                                    "`achieved` is a fabric-side rate and may exceed what DRAM alone delivers "
                                    "(`achievable_peak` = streaming float4 copy of 2 x 1 GiB in this run); gfx950's "
                                    "rocprofv3 exposes no MALL-hit / DRAM-side split (TCC_EA0_RDREQ_DRAM counts "
                                    "requests routed to the memory side, cache hits included)",
                         "traffic": traffic, "traffic_source": traffic_source,
                         "launches": int(launches), "avg_launch_ms": avg_ms,
                         "algorithmic_bytes_per_launch": alg_total / max(launches, 1),
                         "dram_bound_reference": None},
            "kernel_ms_per_step": {"spmm2": kernel_ms / prof_steps,
                                   **{k: v[1] / prof_steps for k, v in other.items()}},
        }
        if world == 1 and layer_s is None and args.full and not args.no_x4:
            # the headline's tensors are no longer needed: free them before the 4M-node graph moves in
            del layer, x_real, x_imag, edge_index
            torch.cuda.empty_cache()
            line["roofline"]["dram_bound_reference"] = dram_bound_reference(device, hidden, copy_rate)
        else:
            line["roofline"]["dram_bound_reference"] = dram_bound_replay()
        if exchange is not None:
            line["exchange"] = exchange
        if parity is not None:
            line["parity"] = parity
        if world == 1 and layer_s is None and args.full and not args.no_configs:
            torch.cuda.empty_cache()         # (the child process needs the device's memory: C4 and C5 hold 10 - 20 GB)
            line["configs"] = baseline_configs()
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(hidden)
            if args.cpu_baseline_northstar:
                try:
                    big = cpu_baseline(hidden, steps=2, n=n, e=args.edges)
                    big["scaled_from"] = "nothing: the north-star size itself"
                    line["cpu_baseline"]["northstar"] = big
                except Exception as exc:  # noqa: BLE001 -- host memory
                    line["cpu_baseline"]["northstar"] = {"error": repr(exc)[:300]}
        result_out.write(json.dumps(line) + "\n")
        result_out.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if parity is not None and not parity["ok"]:
        sys.stderr.write("bench.py: PARITY GUARD FAILED: " + json.dumps(parity) + "\n")
        sys.exit(3)


if __name__ == "__main__":
    main()
