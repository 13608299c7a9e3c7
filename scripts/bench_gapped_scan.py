"""Exhaustive gapped scan on one GPU (development harness; bench.py carries the judged line).
    python scripts/bench_gapped_scan.py --families 20000 --members 50 --queries 32 --steps 5 --out profiles/gapped_scan_bench.json
Workload: --queries queries drawn as scripts/bench_ungapped_scan.py draws them, against the generator's targets.  In one process,
each step with --warmup warm-up runs and --steps timed runs (kernel time from the batches' own events, medians with min and max):
  (a) mmgpu_gscan_* over the first --slice targets,
  (b) mmgpu_sw_prepare(MMGPU_SW_SCORE_END) over the same pairs given as host lists - the same forward kernels, the yardstick of
      (a)'s alignment share,
  (c) mmgpu_gscan_* over all targets with the default pair_budget (chunks),
and the ungapped scan (mmgpu_scan_*) over all targets, whose whole kernel time stands beside (c)'s planner + selection share.
The gapped runs report the planner, alignment, identity and selection shares (mmgpu_gscan_stage_ms)."""
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
ap.add_argument("--min-evalue-score", type=int, default=60)
ap.add_argument("--out", default="")
args = ap.parse_args()

m = dict(np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz")))
mat = m["blosum62_sw"]
t0 = time.time()
(qres, qoff), (tres, toff), _, _ = wl.config3_prefilter(args.families, args.members, max(args.queries, 1), seed=10)
t_gen = time.time() - t0
qs = wl.split(qres, qoff)[:args.queries]
cbs = [capi.host_comp_bias(mat.astype(np.int16), m["blosum62_pback"], q)[1] for q in qs]
queries = [dict(q=q, comp_bias=cb, identity_id=None, min_evalue_score=args.min_evalue_score) for q, cb in zip(qs, cbs)]
qlen_sum = int(sum(len(q) for q in qs))
gpu = mmseqs2_amd.MMGpu(0)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[round(float(x), 3) for x in xs])


def timed(batch, stages):
    for _ in range(args.warmup):
        batch.run()
    gpu.synchronize()
    wall, kern, per = [], [], []
    for _ in range(args.steps):
        t = time.perf_counter()
        batch.run()
        gpu.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        kern.append(batch.kernel_ms())
        if stages:
            per.append(batch.stage_ms())
    r = dict(kernel_ms=spread(kern), wall_ms=spread(wall))
    if stages:
        for name in ("planner", "sw", "identity", "select"):
            r[name + "_ms"] = spread([p[0][name] for p in per])
        r["chunks"] = per[-1][1]
    return r


def gscan(res, off, tag):
    gpu.load_targets(res, off, 21)
    cells = qlen_sum * int(off[-1])
    t = time.perf_counter()
    b = gpu.gscan_prepare(mat, 11, 1, queries, min_score=args.min_score, max_hits=args.max_hits)
    prep = (time.perf_counter() - t) * 1e3
    r = timed(b, True)
    hits, counts = b.fetch()
    b.free()
    r.update(targets=len(off) - 1, residues=int(off[-1]), cells=cells, listed=int(counts.sum()), prepare_wall_ms=round(prep, 1),
             cells_per_s=cells / (r["kernel_ms"]["median"] * 1e-3), sw_cells_per_s=cells / (r["sw_ms"]["median"] * 1e-3))
    print(tag, json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
    return r, hits, counts


out = dict(workload="%d queries drawn as configs[2]'s are (families %d x members %d)" % (len(qs), args.families, args.members),
           queries=len(qs), query_residues=qlen_sum, steps=args.steps, warmup=args.warmup, t_gen_s=round(t_gen, 1))
n_slice = min(args.slice, len(toff) - 1)
sres, soff = tres[:int(toff[n_slice])], toff[:n_slice + 1]
out["a_gscan_slice"], hits, counts = gscan(sres, soff, "(a) gapped scan, slice:")
# (b) the same pairs as host lists; the gapped scan's lists must be what these scores select
ids = np.arange(n_slice, dtype=np.uint32)
t = time.perf_counter()
sw = gpu.sw_prepare(mat, 11, 1, [dict(q=q, comp_bias=cb, targets=ids, min_start_score=0) for q, cb in zip(qs, cbs)], mode=0)
prep = (time.perf_counter() - t) * 1e3
r = timed(sw, False)
rec = sw.fetch().reshape(len(qs), n_slice)
r.update(targets=n_slice, cells=int(sw.cells), prepare_wall_ms=round(prep, 1), cells_per_s=sw.cells / (r["kernel_ms"]["median"] * 1e-3))
sw.free()
for k in range(len(qs)):
    sc = rec[k]["score"].astype(np.int64)
    adm = np.flatnonzero((sc > args.min_score) & (sc >= args.min_evalue_score))
    want = adm[np.lexsort((adm, -sc[adm]))][:args.max_hits]
    assert np.array_equal(hits[k]["id"][:int(counts[k])], want) and np.array_equal(hits[k]["score"][:int(counts[k])], sc[want]), k
out["b_sw_host_lists_slice"] = r
print("(b) host lists, slice:", json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
a_sw, b_k = out["a_gscan_slice"]["sw_ms"], r["kernel_ms"]
out["a_sw_minus_b_ms"] = a_sw["median"] - b_k["median"]
out["b_spread_ms"] = b_k["max"] - b_k["min"]
out["a_sw_within_b_spread"] = bool(out["a_sw_minus_b_ms"] <= out["b_spread_ms"])
out["c_gscan_full"], _, _ = gscan(tres, toff, "(c) gapped scan, all targets:")
# the ungapped scan over all targets in the same session (it has no per-stage timer: its whole kernel time is reported)
b = gpu.scan_prepare(mat, [dict(q=q, comp_bias=cb, identity_id=None) for q, cb in zip(qs, cbs)], min_score=args.min_score, max_hits=args.max_hits)
out["ungapped_scan_full"] = timed(b, False)
b.free()
cus, name = gpu.device_info()
out["device"] = dict(name=name, compute_units=cus)
gpu.close()
print(json.dumps(out))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
