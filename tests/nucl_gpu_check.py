"""Child process of tests/test_nucl_params_gpu.py test_16_lane_kernel_on_the_device (test infrastructure; needs the GPU): started
with MMGPU_NUCL_LANES=16 and MMGPU_TRACE=1 - the library reads the first once per process - it sends the recorded vectors of three
settings (tests/golden/nucl_param_vectors.npz; none with a negative z-drop, see DEVICE_KEYS of the parent) and a reduced queue
test (more pairs than alignments in flight, every copy against the restatement) through mmgpu_nucl_align and prints one JSON
line; the library's trace lines go to stderr for the parent to read.
Exit status 0 = everything equal, 1 = differences, 2 = not set up."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("stock_10_1_z40", "stock_30_30_z40", "transitions_5_2_z40")


def main():
    if os.environ.get("MMGPU_NUCL_LANES") != "16" or not os.environ.get("MMGPU_TRACE"):
        print("nucl_gpu_check.py: MMGPU_NUCL_LANES=16 and MMGPU_TRACE=1 must be set", file=sys.stderr)
        return 2
    import mmseqs2_amd
    from oracle.pyoracle import NuclOracle
    from tests import nucl_common as nc
    from tests import nucl_param_cases as npc
    rep = dict(compared=0, mismatches=0, first=[], queue_pairs=0)
    vectors = npc.load_param_vectors()
    gpu = mmseqs2_amd.MMGpu(0)
    for key in KEYS:
        v = vectors[key]
        bad = npc.fixture_mismatches(gpu, v, v["cases"])
        rep["compared"] += len(v["cases"])
        rep["mismatches"] += len(bad)
        rep["first"] += [repr((key,) + b) for b in bad[:3]]
    # reduced queue test: the 16-lane kernel holds 64 alignments per compute unit (the long pairs are shorter: scratch per alignment)
    g = nc.golden()
    mat, rl = g["mat"], g["reverse"]
    cus, _ = gpu.device_info()
    queries, targets, distinct = npc.queue_pairs(rl, seed=31, n_short=196, n_long=4, long_len=400)
    expected = npc.oracle_results(NuclOracle(), queries, targets, distinct, mat, rl, 5, 2, 40)
    copies = -(-2 * 64 * cus // len(distinct))
    which = np.random.default_rng(6).permutation(np.tile(np.arange(len(distinct)), copies))
    npc.load_targets(gpu, targets)
    hits, strs = gpu.nucl_align(mat, rl, queries, npc.pair_array(distinct)[which], 5, 2, 40, 4, 4)
    bad = [(k, int(w)) for k, w in enumerate(which) if int(hits[k]["status"]) != 0 or npc.hit_tuple(hits[k]) != expected[w][0]
           or strs[k] != expected[w][1]]
    errs = npc.tiling_errors(hits, gpu.last_nucl_bt_used)
    rep["queue_pairs"] = len(which)
    rep["compared"] += len(which)
    rep["mismatches"] += len(bad) + len(errs)
    rep["first"] += [repr(("queue",) + b) for b in bad[:3]] + errs
    gpu.close()
    print(json.dumps(rep))
    return 0 if rep["mismatches"] == 0 and rep["compared"] == 360 + rep["queue_pairs"] > 360 else 1


if __name__ == "__main__":
    sys.exit(main())
