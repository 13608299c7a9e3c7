"""Ungapped diagonal rescoring on one GPU (development harness; bench.py carries the judged line).
    python scripts/bench_rescore.py --families 8000 --members 64 --false-hits 16 --steps 5 --out profiles/rescore_bench.json
Workload, linclust-like: --families representative sequences of 150 .. 500 residues are the queries; every family has --members
targets, each a mutated copy of its representative with up to 20 residues cut off either end; a query's list holds its members on
their true diagonal (the cut at the front) and --false-hits random targets on random diagonals of -20 .. 20, shuffled.  For each
mode 0, 1, 2: --warmup warm-up runs and --steps timed runs of one prepared batch; kernel time from the batch's own events (medians
with min and max).  Reported per mode: hits/s, cells/s (cells = the lengths of the diagonals scored) and residue bytes/s = 2 bytes
a cell (one query and one target letter), the figure to hold against what HBM / L2 deliver: the kernel reads every residue of a
diagonal once and writes 24 bytes a hit."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime per process)
import mmseqs2_amd
from mmseqs2_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=8000)
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--false-hits", type=int, default=16)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default="")
args = ap.parse_args()

mat = np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz"))["blosum62_sw"]
rng = np.random.default_rng(12)
t0 = time.time()
F, M = args.families, args.members
reps = [rng.integers(0, 20, int(n)).astype(np.uint8) for n in rng.integers(150, 501, F)]
targets, front = [], np.zeros(F * M, np.int64)
for f, rep in enumerate(reps):
    cuts = rng.integers(0, 21, (M, 2))
    noise = rng.integers(0, 20, (M, len(rep))).astype(np.uint8)
    keep = rng.random((M, len(rep))) < 0.7
    fam = np.where(keep, rep[None, :], noise)
    for m in range(M):
        targets.append(fam[m, cuts[m, 0]:len(rep) - cuts[m, 1]])
        front[f * M + m] = cuts[m, 0]
tlen = np.array([len(t) for t in targets], np.int64)
toff = np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint64)
tres = np.concatenate(targets)
hits, cells = [], 0
for f, rep in enumerate(reps):
    own = np.stack([np.arange(f * M, (f + 1) * M), front[f * M:(f + 1) * M]], axis=1)
    false = np.stack([rng.integers(0, F * M, args.false_hits), rng.integers(-20, 21, args.false_hits)], axis=1)
    h = np.concatenate([own, false])
    h = h[rng.permutation(len(h))]
    hits.append(h)
    D, tl = h[:, 1], tlen[h[:, 0]]
    cells += int(np.where(D >= 0, np.minimum(tl, len(rep) - D), np.minimum(tl + D, len(rep))).sum())
n_hits = int(sum(len(h) for h in hits))
t_gen = time.time() - t0


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[round(float(x), 3) for x in xs])


gpu = mmseqs2_amd.MMGpu(0)
gpu.load_targets(tres, toff, 21)
out = dict(workload="%d queries (representatives of 150 .. 500 residues), %d members and %d false hits each" % (F, M, args.false_hits),
           queries=F, targets=F * M, hits=n_hits, cells=cells, mean_diagonal=round(cells / n_hits, 1), steps=args.steps, warmup=args.warmup,
           t_gen_s=round(t_gen, 1), modes={})
for mode in (capi.RESCORE_HAMMING, capi.RESCORE_SUBSTITUTION, capi.RESCORE_ALIGNMENT):
    t = time.perf_counter()
    b = gpu.rescore_prepare(mat, reps, hits, mode)
    prep = (time.perf_counter() - t) * 1e3
    for _ in range(args.warmup):
        b.run()
    gpu.synchronize()
    wall, kern = [], []
    for _ in range(args.steps):
        t = time.perf_counter()
        b.run()
        gpu.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        kern.append(b.kernel_ms())
    rec = b.fetch()
    b.free()
    assert len(rec) == n_hits and int(rec["diag_len"].astype(np.int64).sum()) <= cells
    k = float(np.median(kern)) * 1e-3
    r = dict(kernel_ms=spread(kern), wall_ms=spread(wall), prepare_wall_ms=round(prep, 1), hits_per_s=n_hits / k, cells_per_s=cells / k,
             residue_bytes_per_s=2 * cells / k, record_bytes_per_s=24 * n_hits / k, hits_above_0=int((rec["score"] > 0).sum()))
    out["modes"][str(mode)] = r
    print("mode %d:" % mode, json.dumps({a: (v["median"] if isinstance(v, dict) else v) for a, v in r.items()}), flush=True)
cus, name = gpu.device_info()
out["device"] = dict(name=name, compute_units=cus)
gpu.close()
print(json.dumps(out))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
