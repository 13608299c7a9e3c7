"""Child process of tests/test_bt_gpu.py test_lane_kernel_alone (test infrastructure; needs the GPU): started with
MMGPU_BT_LANE_KERNEL=1 - the library reads the switch once per process - it sends the band-class cases of tests/bt_cases.py for
three parameter sets, the engineered ties at BLOSUM62 11/1 and two profile-query pairs through mmgpu_sw_traceback, compares status / string / ident / bt_len with the
restatement itself and prints one JSON line; the library's MMGPU_TRACE lines go to stderr for the parent to read.
Exit status 0 = ran to the end (the parent asserts on the counts), 1 = mismatches."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("blosum62_11_1", "blosum62_6_5", "pam30_25_2")


def main():
    import mmseqs2_amd
    from mmseqs2_amd import workloads as wl
    from oracle.pyoracle import Oracle
    from tests import bt_cases as bc
    from tests import sw_param_cases as pc
    if not os.environ.get("MMGPU_BT_LANE_KERNEL"):
        print("bt_gpu_check.py: MMGPU_BT_LANE_KERNEL is not set", file=sys.stderr)
        return 2
    oracle = Oracle()
    sets = pc.load_param_vectors()
    gpu = mmseqs2_amd.MMGpu(0)
    rep = dict(compared=0, mismatches=0, profile_pairs=0, ties={}, sets={}, first=[])
    for key in KEYS:
        v = sets[key]
        cases, n_refused = bc.band_cases(oracle, v, 500 + sum(map(ord, key)), wide=key == "blosum62_11_1", log=lambda s: None)
        b = bc.run_cases(gpu, v, cases)
        tally, bad = bc.check_traceback(b, cases, key)
        b.free()
        rep["compared"] += tally.n
        rep["mismatches"] += len(bad)
        rep["first"] += [repr(x) for x in bad[:3]]
        rep["sets"][key] = str(tally)
    # the engineered ties (the default path sends them through the wave kernel only): 'ef' is the lane kernel's `hsel` rule
    v = sets["blosum62_11_1"]
    cases, _ = bc.tie_cases(oracle, v, log=lambda s: None)
    b = bc.run_cases(gpu, v, cases)
    tally, bad = bc.check_traceback(b, cases, "ties")
    b.free()
    bad_labels = {x[1] for x in bad}
    for c in cases:
        if c["label"] not in bad_labels:
            rep["ties"][c["kind"]] = rep["ties"].get(c["kind"], 0) + 1
    rep["compared"] += tally.n
    rep["mismatches"] += len(bad)
    rep["first"] += [repr(x) for x in bad[:3]]
    # two profile queries (the kernel reads the query's own score rows instead of matrix + bias), one of them of two tiles
    mat = sets["blosum62_11_1"]["mat"]
    rng = np.random.default_rng(9)
    queries, targets = [], []
    for k, L in enumerate((180, 600)):
        prof, cons = bc.profile_query(rng, mat, L)
        targets.append(wl.mutate(rng, cons, 0.8, max_indels=5, max_indel_len=12))
        queries.append(dict(q=cons, comp_bias=None, profile=prof, targets=np.array([k], np.uint32), min_start_score=0))
    tres, toff = wl.seqs_from_list(targets)
    gpu.load_targets(tres, toff, 21)
    b = gpu.sw_prepare(mat, 11, 1, queries, mode=1)
    b.run()
    info, strs = b.traceback(np.arange(2, dtype=np.uint32))
    b.free()
    for k, qd in enumerate(queries):
        o = oracle.sw_align_profile(qd["profile"], qd["q"], targets[k], 21, 11, 1, need_start=True, need_bt=True)
        ok = o["bt"] != "" and int(info[k]["status"]) == 0 and strs[k] == o["bt"] and int(info[k]["ident"]) == o["ident"]
        rep["profile_pairs"] += 1
        rep["compared"] += 1
        if not ok:
            rep["mismatches"] += 1
            rep["first"].append("profile pair %d: status %d" % (k, int(info[k]["status"])))
    gpu.close()
    print(json.dumps(rep))
    return 1 if rep["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
