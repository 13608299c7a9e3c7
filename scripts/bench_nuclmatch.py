"""linclust's k-mer matching stage over nucleotides on one GPU (development harness; bench.py carries the judged line).
    python scripts/bench_nuclmatch.py --families 6000 --members 16 --steps 5 --stock --out profiles/nuclmatch_bench.json
Workload: families as bench_rescore.py makes them, over A C G T - --families representatives with log-normal lengths around 1 500
residues (200 .. 30 000), every family --members mutated copies (90 % of the residues kept) with up to 20 residues cut off either
end, every second copy reverse-complemented; the copies are the database.  linclust's nucleotide defaults for it: k from the database
size, 60 k-mers per sequence, scale 0.2, -c 0.8.  6 000 x 16 (96 000 sequences, 1.6e8 residues) is the size at which the stock binary
takes about a second with 16 threads.
One process, --warmup warm-up runs, then --steps timed runs of one prepared batch; the time per stage (extract, sort 1, group,
sort 2, vote) from the batch's own events, medians with min and max; the record counts at each stage.
Held against: the extraction against reading each residue once and writing each selected record once (16 bytes); each sort against
its key and value bytes read and written once per 8-bit digit pass of the bits it sorts.  HBM_BYTES_PER_S is the data-sheet figure.
--stock: where oracle/_ref/mmseqs_stock is present, the same database through `createdb --dbtype 2` and
`kmermatcher --linclust-version 1 --threads 16`, its wall time and whether its lists equal the device's.
--no-device: only the stock binary is timed (choosing a size on a machine without a GPU)."""
import argparse, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
STOCK = os.path.join(ROOT, "oracle", "_ref", "mmseqs_stock")

ap = argparse.ArgumentParser()
ap.add_argument("--families", type=int, default=6000)
ap.add_argument("--members", type=int, default=16)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--stock", action="store_true")
ap.add_argument("--no-device", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()

rng = np.random.default_rng(12)
t0 = time.time()
F, M = args.families, args.members
parts, lens = [], []
for n in np.clip(rng.lognormal(np.log(1500.0), 0.5, F), 200, 30000).astype(int):
    rep = rng.integers(0, 4, int(n)).astype(np.uint8)
    cuts = rng.integers(0, 21, (M, 2))
    fam = np.where(rng.random((M, n)) < 0.9, rep[None, :], rng.integers(0, 4, (M, n)).astype(np.uint8))
    for m in range(M):
        s = fam[m, cuts[m, 0]:n - cuts[m, 1]]
        parts.append((s[::-1] ^ 2) if m % 2 else s)      # A<->T, C<->G are code ^ 2
        lens.append(len(s))
res = np.concatenate(parts).astype(np.uint8)
lens = np.asarray(lens, np.int64)
off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
del parts
t_gen = time.time() - t0
n_seqs, n_res = len(lens), int(off[-1])


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[round(float(x), 3) for x in xs])


out = dict(workload="%d families x %d members: %d sequences, %d residues, longest %d" % (F, M, n_seqs, n_res, int(lens.max())), sequences=n_seqs,
           residues=n_res, steps=args.steps, warmup=args.warmup, t_gen_s=round(t_gen, 1))
d_off = d_rec = None
if not args.no_device:
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import mmseqs2_amd
    from mmseqs2_amd import capi
    par = dict(k=capi.nuclmatch_defaults(n_res), kmers_per_seq=60, kmers_per_seq_scale=0.2, hash_shift=67, cov_thr=0.8, cov_mode=0, include_only_extendable=0)
    gpu = mmseqs2_amd.MMGpu(0)
    t = time.perf_counter()
    gpu.load_targets(res, off, 5)
    t_load = time.perf_counter() - t
    b = gpu.nuclmatch_prepare(par)
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
    sort1_passes = int(np.ceil((15 + id_bits) / 8)) + 2 + 8
    models = dict(
        extract=dict(bytes=n_res + 16 * n_rec, note="every residue read once, every record (8-byte k-mer, 8-byte value) written once"),
        sort1=dict(bytes=2 * 16 * n_rec * sort1_passes,
                   note="%d id and position bits, 15 length bits and 63 k-mer bits (%d digit passes): 16 bytes a record read and written per pass" % (15 + id_bits, sort1_passes)),
        sort2=dict(bytes=2 * 10 * n_pairs * (2 + int(np.ceil((32 + id_bits) / 8))),
                   note="16 diagonal bits (2 digit passes) and %d pair bits: 10 bytes a record read and written per pass" % (32 + id_bits)))
    for s, m in models.items():
        m["bytes_per_s"] = m["bytes"] / med[s] if med[s] > 0 else 0.0
        m["fraction_of_hbm"] = m["bytes_per_s"] / HBM_BYTES_PER_S
    out.update(params=par, counts=counts, load_targets_s=round(t_load, 2), fetch_s=round(t_fetch, 3), run_wall_ms=spread(wall), run_events_ms=spread(total),
               stage_ms={s: spread(v) for s, v in stage.items()}, models=models, hbm_bytes_per_s_assumed=HBM_BYTES_PER_S,
               negative_scores=int((d_rec["score"] < 0).sum()))
    cus, name = gpu.device_info()
    out["device"] = dict(name=name, compute_units=cus)
    gpu.close()

if args.stock and os.path.exists(STOCK):
    from mmseqs2_amd import dbio
    with tempfile.TemporaryDirectory() as tmp:
        t = time.perf_counter()
        text = np.frombuffer(b"ACTGN", np.uint8)[res]
        with open(os.path.join(tmp, "db.fasta"), "wb") as fh:
            for i in range(n_seqs):
                fh.write(b">s%d\n" % i)
                fh.write(text[int(off[i]):int(off[i + 1])].tobytes())
                fh.write(b"\n")
        db, result = os.path.join(tmp, "db"), os.path.join(tmp, "res")
        subprocess.run([STOCK, "createdb", os.path.join(tmp, "db.fasta"), db, "--shuffle", "0", "--dbtype", "2", "-v", "1"], check=True, stdout=subprocess.DEVNULL)
        t_db = time.perf_counter() - t
        t = time.perf_counter()
        log = subprocess.run([STOCK, "kmermatcher", db, result, "--linclust-version", "1", "--threads", "16", "-c", "0.8", "-v", "3"], check=True,
                             stdout=subprocess.PIPE).stdout.decode()
        t_stock = time.perf_counter() - t
        out["stock"] = dict(kmermatcher_wall_s=round(t_stock, 2), fasta_and_createdb_s=round(t_db, 1), threads=16,
                            timers=[ln for ln in log.splitlines() if ln.startswith("Time for") or ln.startswith("Sort")])
        if d_rec is not None:
            lists = dbio.read_db(result)
            equal, lines = True, 0
            for i in range(n_seqs):
                want = [tuple(int(x) for x in ln.split("\t")[:3]) for ln in lists[i].decode().splitlines()]
                got = d_rec[int(d_off[i]):int(d_off[i + 1])]
                lines += len(want)
                if [(int(r["id"]), int(r["score"]), int(r["diagonal"].astype(np.int16))) for r in got] != want:
                    equal = False
                    out["stock"]["first_difference"] = dict(list=i, device=[[int(r["id"]), int(r["score"]), int(r["diagonal"].astype(np.int16))] for r in got][:8],
                                                            stock=[list(w) for w in want][:8])
                    break
            out["stock"].update(lists_equal=bool(equal), lines=lines)
print(json.dumps(out))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
