"""Exhaustive ungapped scan throughput on one GPU (development harness; bench.py carries the judged line).
    python scripts/bench_ungapped_scan.py --families 20000 --members 50 --queries 32 --steps 5 --out profiles/ungapped_scan_bench.json
Workload: --queries queries drawn by the generator of BASELINE.json configs[2] with bench.py's seed (the generator is asked for
--queries of them, which are drawn the same way as bench.py's 10 000 but are not its first ones), against all of its targets
(everything resident).  Warm-up, then --steps timed runs in this process: kernel time from mmgpu_scan_last_kernel_ms, wall time
around run + synchronize.  Yardstick, in the same process: mmgpu_sw_prepare in MMGPU_SW_SCORE_END mode (the Gotoh forward scan)
over the same queries against the first --slice targets, and the scan's own rate on that same slice.  Cells = query length x
target length summed over the pairs a kernel scores.  --profile: the same queries run as profile queries in the two scan runs (each
query's [20][qlen] profile is its letters' substitution rows; the Gotoh yardstick keeps the sequence queries)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime per process)
import mmseqs2_amd
from mmseqs2_amd import capi, workloads as wl

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=20000)
ap.add_argument("--members", type=int, default=50)
ap.add_argument("--queries", type=int, default=32)
ap.add_argument("--slice", type=int, default=100000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--max-hits", type=int, default=300)
ap.add_argument("--min-score", type=int, default=15)
ap.add_argument("--profile", action="store_true", help="run the scan's queries as profile queries (mmgpu_scan_query::profile)")
ap.add_argument("--out", default="")
args = ap.parse_args()

m = dict(np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz")))
mat = m["blosum62_sw"]
t0 = time.time()
(qres, qoff), (tres, toff), _, _ = wl.config3_prefilter(args.families, args.members, max(args.queries, 1), seed=10)
t_gen = time.time() - t0
qs = wl.split(qres, qoff)[:args.queries]
cbs = [capi.host_comp_bias(mat.astype(np.int16), m["blosum62_pback"], q)[1] for q in qs]
queries = [dict(q=q, comp_bias=cb, identity_id=None) for q, cb in zip(qs, cbs)]
if args.profile:
    queries = [dict(profile=np.ascontiguousarray(mat[:20, q]), identity_id=None) for q in qs]
qlen_sum = int(sum(len(q) for q in qs))
gpu = mmseqs2_amd.MMGpu(0)


def timed(batch, steps, warmup):
    for _ in range(warmup):
        batch.run()
    gpu.synchronize()
    wall, kern = [], []
    for _ in range(steps):
        t = time.perf_counter()
        batch.run()
        gpu.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        kern.append(batch.kernel_ms())
    return dict(kernel_ms=[round(x, 3) for x in kern], wall_ms=[round(x, 3) for x in wall], kernel_ms_median=float(np.median(kern)),
                wall_ms_median=float(np.median(wall)))


def scan_rate(res, off, tag):
    gpu.load_targets(res, off, 21)
    cells = qlen_sum * int(off[-1])
    b = gpu.scan_prepare(mat, queries, min_score=args.min_score, max_hits=args.max_hits)
    r = timed(b, args.steps, args.warmup)
    hits, counts = b.fetch()
    b.free()
    r.update(targets=len(off) - 1, residues=int(off[-1]), cells=cells, listed=int(counts.sum()),
             cells_per_s=cells / (r["kernel_ms_median"] * 1e-3), cells_per_s_wall=cells / (r["wall_ms_median"] * 1e-3))
    print(tag, json.dumps({k: v for k, v in r.items() if k not in ("kernel_ms", "wall_ms")}), flush=True)
    return r


out = dict(workload="%d queries drawn as configs[2]'s are (families %d x members %d), all targets resident" % (len(qs), args.families, args.members),
           queries=len(qs), query_kind="profile" if args.profile else "sequence", query_residues=qlen_sum, steps=args.steps, warmup=args.warmup, t_gen_s=round(t_gen, 1))
out["scan_full"] = scan_rate(tres, toff, "scan, all targets:")
n_slice = min(args.slice, len(toff) - 1)
sres, soff = tres[:int(toff[n_slice])], toff[:n_slice + 1]
out["scan_slice"] = scan_rate(sres, soff, "scan, slice:")
# the yardstick: the Gotoh forward scan (score + end positions) over the same pairs of the slice
ids = np.arange(n_slice, dtype=np.uint32)
sw = gpu.sw_prepare(mat, 11, 1, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0) for q, cb in zip(qs, cbs)], mode=0)
r = timed(sw, args.steps, args.warmup)
r.update(targets=n_slice, cells=int(sw.cells), cells_per_s=sw.cells / (r["kernel_ms_median"] * 1e-3),
         cells_per_s_wall=sw.cells / (r["wall_ms_median"] * 1e-3))
sw.free()
out["gotoh_slice"] = r
out["ratio_scan_over_gotoh_slice"] = out["scan_slice"]["cells_per_s"] / r["cells_per_s"]
out["ratio_scan_full_over_gotoh_slice"] = out["scan_full"]["cells_per_s"] / r["cells_per_s"]
cus, name = gpu.device_info()
out["device"] = dict(name=name, compute_units=cus)
gpu.close()
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
