"""linclust's k-mer matching stage on one GPU (development harness; bench.py carries the judged line).
    python scripts/bench_kmermatch.py --families 64000 --members 64 --steps 5 --out profiles/kmermatch_bench.json
Workload: bench_rescore.py's families - --families representatives of 150 .. 500 residues, every family --members mutated copies
(70 % of the residues kept) with up to 20 residues cut off either end; the copies are the database.  linclust's defaults for it:
k from the database size, 13 letters (the reduction table recorded in tests/golden/kmermatch.npz), 20 k-mers per sequence, -c 0.8.
One process, --warmup warm-up runs, then --steps timed runs of one prepared batch; the time per stage (extract, sort 1, group,
sort 2, vote) from the batch's own events, medians with min and max; the record counts at each stage.
Held against: the extraction against reading each residue once and writing each selected record once (16 bytes); each sort against
its key and value bytes read and written once per 8-bit digit pass of the bits it sorts.  HBM_BYTES_PER_S is the data-sheet figure.
--stock: where oracle/_ref/mmseqs_stock is present, the same database through `createdb` and
`kmermatcher --linclust-version 1 --threads 16`, its wall time and whether its lists equal the device's."""
import argparse, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime per process)
import mmseqs2_amd
from mmseqs2_amd import capi, dbio

HBM_BYTES_PER_S = 8.0e12
STOCK = os.path.join(ROOT, "oracle", "_ref", "mmseqs_stock")

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=64000)
ap.add_argument("--members", type=int, default=64)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--stock", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()

rng = np.random.default_rng(12)
t0 = time.time()
F, M = args.families, args.members
parts, lens = [], []
for n in rng.integers(150, 501, F):
    rep = rng.integers(0, 20, int(n)).astype(np.uint8)
    cuts = rng.integers(0, 21, (M, 2))
    fam = np.where(rng.random((M, n)) < 0.7, rep[None, :], rng.integers(0, 20, (M, n)).astype(np.uint8))
    col = np.arange(n)[None, :]
    keep = (col >= cuts[:, :1]) & (col < n - cuts[:, 1:])
    parts.append(fam[keep])      # row-major: member after member
    lens.append(keep.sum(axis=1))
res = np.concatenate(parts)
lens = np.concatenate(lens).astype(np.int64)
off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
del parts
t_gen = time.time() - t0
n_seqs, n_res = len(lens), int(off[-1])

g = np.load(os.path.join(ROOT, "tests", "golden", "kmermatch.npz"))
default = json.loads(bytes(g["settings"]).decode())[0]      # the recorded default setting: its 13-letter reduction table
k, alph = capi.kmermatch_defaults(0.0, n_res)
assert alph == default["alph_size"]
par = dict(k=k, alph_size=alph, reduce=default["reduce"], kmers_per_seq=20, kmers_per_seq_scale=0.0, hash_shift=67, cov_thr=0.8, cov_mode=0,
           include_only_extendable=0)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[round(float(x), 3) for x in xs])


gpu = mmseqs2_amd.MMGpu(0)
t = time.perf_counter()
gpu.load_targets(res, off, 21)
t_load = time.perf_counter() - t
b = gpu.kmermatch_prepare(par)
for _ in range(args.warmup):
    b.run()
wall, total, stage = [], [], {s: [] for s in capi.KMERMATCH_STAGES}
for _ in range(args.steps):
    t = time.perf_counter()
    b.run()
    gpu.synchronize()
    wall.append((time.perf_counter() - t) * 1e3)
    ms, per = b.stage_ms()
    total.append(ms)
    for s in capi.KMERMATCH_STAGES:
        stage[s].append(per[s])
counts = b.counts()
t = time.perf_counter()
d_off, d_rec = b.fetch()
t_fetch = time.perf_counter() - t
b.free()
med = {s: float(np.median(stage[s])) * 1e-3 for s in stage}
n_rec, n_pairs = counts["n_records"], counts["n_pairs"]
id_bits = max(1, int(np.ceil(np.log2(n_seqs))))
models = dict(
    extract=dict(bytes=n_res + 16 * n_rec, note="every residue read once, every record (8-byte k-mer, 8-byte value) written once"),
    sort1=dict(bytes=2 * 16 * n_rec * (2 + 8), note="15 length bits (2 digit passes) and 64 k-mer bits (8): 16 bytes a record read and written per pass"),
    sort2=dict(bytes=2 * 10 * n_pairs * (2 + int(np.ceil((32 + id_bits) / 8))),
               note="16 diagonal bits (2 digit passes) and %d pair bits: 10 bytes a record read and written per pass" % (32 + id_bits)))
for s, m in models.items():
    m["bytes_per_s"] = m["bytes"] / med[s] if med[s] > 0 else 0.0
    m["fraction_of_hbm"] = m["bytes_per_s"] / HBM_BYTES_PER_S
out = dict(workload="%d families x %d members: %d sequences, %d residues" % (F, M, n_seqs, n_res), sequences=n_seqs, residues=n_res, params=par,
           counts=counts, steps=args.steps, warmup=args.warmup, t_gen_s=round(t_gen, 1), load_targets_s=round(t_load, 2), fetch_s=round(t_fetch, 3),
           run_wall_ms=spread(wall), run_events_ms=spread(total), stage_ms={s: spread(v) for s, v in stage.items()}, models=models,
           hbm_bytes_per_s_assumed=HBM_BYTES_PER_S)
cus, name = gpu.device_info()
out["device"] = dict(name=name, compute_units=cus)
gpu.close()

if args.stock and os.path.exists(STOCK):
    letters = "ACDEFGHIKLMNPQRSTVWYX"
    with tempfile.TemporaryDirectory() as tmp:
        t = time.perf_counter()
        text = np.frombuffer(letters.encode(), np.uint8)[res]
        with open(os.path.join(tmp, "db.fasta"), "wb") as fh:
            for i in range(n_seqs):
                fh.write(b">s%d\n" % i)
                fh.write(text[int(off[i]):int(off[i + 1])].tobytes())
                fh.write(b"\n")
        db, result = os.path.join(tmp, "db"), os.path.join(tmp, "res")
        subprocess.run([STOCK, "createdb", os.path.join(tmp, "db.fasta"), db, "--shuffle", "0", "--dbtype", "1", "-v", "1"], check=True, stdout=subprocess.DEVNULL)
        t_db = time.perf_counter() - t
        t = time.perf_counter()
        log = subprocess.run([STOCK, "kmermatcher", db, result, "--linclust-version", "1", "--threads", "16", "-v", "3"], check=True,
                             stdout=subprocess.PIPE).stdout.decode()
        t_stock = time.perf_counter() - t
        lists = dbio.read_db(result)
        equal, lines = True, 0
        for i in range(n_seqs):
            want = [tuple(int(x) for x in ln.split("\t")[:3]) for ln in lists[i].decode().splitlines()]
            got = d_rec[int(d_off[i]):int(d_off[i + 1])]
            lines += len(want)
            if [(int(r["id"]), int(r["score"]), int(r["diagonal"].astype(np.int16))) for r in got] != want:
                equal = False
                break
        out["stock"] = dict(kmermatcher_wall_s=round(t_stock, 2), fasta_and_createdb_s=round(t_db, 1), threads=16, lists_equal=bool(equal), lines=lines,
                            timers=[ln for ln in log.splitlines() if ln.startswith("Time for") or ln.startswith("Sort")])
print(json.dumps(out))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
