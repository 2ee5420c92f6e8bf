"""Times SDGNN's and SiGAT's `build_edge_lists` (the triangle-motif neighbourhoods) on the host (scipy products) and on the
device (csrc/motifs.hip), on signed graphs of several sizes.  Device times are wall clocks around whole calls with a device
synchronisation, after a warm-up call at the same size (median of --repeats); host times a wall clock, each host build in a
child process of its own under --host-limit seconds (a build that does not finish is recorded as not completed).
One JSON object to --out.  Off bench.py's timed path.

    python tools/bench_motifs.py --out profiles/motifs.json
    rocprofv3 --kernel-trace --stats -d <dir> -o k -- python tools/bench_motifs.py --sizes c3 --repeats 1 --no-host --out <tmp>
    python tools/bench_motifs.py --merge-stats <dir>/.../k_kernel_stats.csv --out profiles/motifs.json

Probes = sum over the keys (u, v) of U = P u N of min(d_u, d_v), d the typed-neighbourhood sizes: the binary searches the
intersection kernel performs.  Every device run is checked against the host path where the host path finished."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = {"100k": (100_000, 1_000_000), "200k": (200_000, 4_000_000), "c3": (500_000, 10_000_000), "hub": (66_000, None)}
KERNELS = ("motif_lane_kernel", "motif_wave_kernel")


def graph(size):
    """int64 [E, 3] (source, target, sign) and the node count.  100k / 200k: SDSBM (directed); c3: SSBM (both
    orientations, the size GATConv / SNEAConv are benchmarked at); hub: the hub graph of tests/test_gpu_motifs.py."""
    import bigdata
    n, e = SIZES[size]
    if size == "hub":
        from test_gpu_motifs import hub_graph
        es, n = hub_graph(n)
        return es, n
    pe, ps = bigdata.ssbm_graph(n, e) if size == "c3" else bigdata.sdsbm_graph(n, e)
    ei, sign = bigdata.load(pe), bigdata.load(ps)
    return torch.from_numpy(np.stack([ei[0], ei[1], np.asarray(sign).astype(np.int64)], 1)), n


def bare(name, n, device):
    from pytorch_geometric_signed_directed_amd.nn import models
    m = getattr(models, name).__new__(getattr(models, name))
    torch.nn.Module.__init__(m)
    m.node_num, m.device = n, torch.device(device)
    return m


def device_case(es, n, repeats):
    from pytorch_geometric_signed_directed_amd import motifs
    dev = torch.device("cuda:0")
    es = es.to(dev)
    out = {}
    for name in ("SDGNN", "SiGAT"):
        m = bare(name, n, dev)
        m.build_edge_lists(es)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(repeats):
            t = time.perf_counter()
            lists = m.build_edge_lists(es)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        out[name] = {"ms": float(np.median(ms)), "ms_all": ms, "peak_device_bytes": torch.cuda.max_memory_allocated(),
                     "list_sizes": [int(t.size(1)) for t in lists]}
    nb = motifs.signed_neighbourhoods(es, n)
    torch.cuda.synchronize()
    t = time.perf_counter()
    nb = motifs.signed_neighbourhoods(es, n)
    torch.cuda.synchronize()
    out["neighbourhoods_ms"] = (time.perf_counter() - t) * 1e3
    counts = {}
    for tier in (None, 0, 1):
        motifs.motif_counts(nb, tier=tier)
        torch.cuda.synchronize()
        t = time.perf_counter()
        c = motifs.motif_counts(nb, tier=tier)
        torch.cuda.synchronize()
        counts["default" if tier is None else f"tier{tier}"] = (time.perf_counter() - t) * 1e3
    out["counts_ms"] = counts
    deg = (nb.rowptr[1:] - nb.rowptr[:-1]).long()
    short = torch.minimum(deg[nb.keys // n], deg[nb.keys % n])
    out["keys"] = int(nb.keys.numel())
    out["typed_entries"] = int(nb.col.numel())
    out["max_typed_degree"] = int(deg.max())
    out["probes"] = int(short.sum())
    out["wave_tier_keys"] = int((short > motifs.LANE_MAX_SHORT).sum())
    out["probes_per_s_default"] = out["probes"] / (counts["default"] * 1e-3)
    out["counts_sha"] = int(torch.sum(c.long() * torch.arange(1, 17, device=dev)).item())
    return out


HOST_CHILD = r"""
import sys, time, json
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
sys.argv = ["x"]
import tools.bench_motifs as B
es, n = B.graph({size!r})
res = {{}}
for name in ("SDGNN", "SiGAT"):
    m = B.bare(name, n, "cpu")
    t = time.perf_counter()
    lists = m.build_edge_lists(es)
    res[name] = {{"s": time.perf_counter() - t, "list_sizes": [int(x.size(1)) for x in lists]}}
print(json.dumps(res))
"""


def host_case(size, limit):
    code = HOST_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), size=size)
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"completed": False, "limit_s": limit}
    if p.returncode != 0:
        return {"completed": False, "error": p.stderr.strip().splitlines()[-1:] if p.stderr else p.returncode}
    return {"completed": True, **json.loads(p.stdout.strip().splitlines()[-1])}


def merge_stats(path, out):
    rows = list(csv.DictReader(open(path)))
    res = json.load(open(out)) if os.path.exists(out) else {}
    stats = {}
    for r in rows:
        for k in KERNELS + ("nb_", "radix", "scan"):
            if k in r["Name"]:
                stats[r["Name"][:120]] = {"calls": int(r["Calls"]), "total_ms": int(r["TotalDurationNs"]) / 1e6,
                                          "avg_ms": float(r["AverageNs"]) / 1e6}
    res["kernel_stats"] = {"source": os.path.basename(path), "kernels": stats}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100k,200k,c3,hub")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-limit", type=float, default=300.0)
    ap.add_argument("--host-sizes", default="100k,200k,c3", help="sizes whose host path is attempted")
    ap.add_argument("--merge-stats", default=None, help="rocprofv3 kernel_stats.csv to merge into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motifs.json"))
    a = ap.parse_args()
    if a.merge_stats:
        merge_stats(a.merge_stats, a.out)
        return
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "host_limit_s": a.host_limit, "cases": []}
    for size in a.sizes.split(","):
        t = time.perf_counter()
        es, n = graph(size)
        case = {"size": size, "nodes": n, "rows": int(es.size(0)), "generate_s": round(time.perf_counter() - t, 1)}
        case["device"] = device_case(es, n, a.repeats)
        if not a.no_host and size in a.host_sizes.split(","):
            case["host"] = host_case(size, a.host_limit)
            if case["host"]["completed"]:
                for name in ("SDGNN", "SiGAT"):
                    h, d = case["host"][name], case["device"][name]
                    case[f"{name}_host_over_device"] = h["s"] / (d["ms"] * 1e-3)
                    case[f"{name}_same_list_sizes"] = h["list_sizes"] == d["list_sizes"]
        elif not a.no_host:
            case["host"] = "not measured"
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
