"""What a failed call leaves behind in a context (include/mmgpu.h: mmgpu_load_targets, mmgpu_pf_load_index, mmgpu_pf_build_index):
a call refused for its arguments leaves the resident targets and index answering bit for bit as before, a mmgpu_load_targets that
fails while it packs leaves an empty, consistent context, and a message names the entry point that was called."""
import ctypes

import numpy as np
import pytest

from mmseqs2_amd import capi
from tests import pf_common as pc
from tests import pf_gpu_check as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(gpu, matrices):
    """The golden case resident, the answers of a 4-query prefilter batch and of an alignment batch over 40 targets recorded."""
    g = pc.golden()
    thr = int(g["kmer_thr"])
    tab = chk.load_case(gpu, g, g["tres"], g["toff"], thr)
    s3, i3 = capi.host_score_matrix(g["vtml80_kmer16"], 3, lib=gpu.L)
    qs = pc.golden_queries(g)[:4]
    for qd in qs:
        qd["identity_id"] = None
    sw_q = [dict(q=qs[0]["q"], comp_bias=None, targets=np.arange(40, dtype=np.uint32), min_start_score=0)]
    c = dict(g=g, thr=thr, tab=tab, s3=s3, i3=i3, qs=qs, sw_q=sw_q, mat=matrices["blosum62_sw"])
    c["pf"] = gpu.pf_batch(qs, thr, max_hits=300, ref_bins=2)[:3]
    c["sw"] = gpu.sw_batch(c["mat"], 11, 1, sw_q, mode=1)
    c["index"] = gpu.pf_debug_index(6, 21)
    assert int(c["pf"][1].sum()) > 0 and len(c["index"][1]) > 0
    yield c
    chk.load_case(gpu, g, g["tres"], g["toff"], thr)      # the module's golden case for the tests that follow


def restore(gpu, c):
    g = c["g"]
    gpu.load_targets(g["tres"], g["toff"], 21)
    gpu.pf_load_index(6, 21, True, c["s3"], c["i3"], c["tab"]["offsets"], c["tab"]["ids"], c["tab"]["pos"], g["blosum62_ungapped"])


def answers_as_recorded(gpu, c):
    hits, counts, status = gpu.pf_batch(c["qs"], c["thr"], max_hits=300, ref_bins=2)[:3]
    assert np.array_equal(counts, c["pf"][1]) and np.array_equal(status, c["pf"][2])
    for qi in range(len(c["qs"])):
        n = int(counts[qi])
        assert np.array_equal(hits[qi][:n], c["pf"][0][qi][:n])
    assert np.array_equal(gpu.sw_batch(c["mat"], 11, 1, c["sw_q"], mode=1), c["sw"])


def index_as_recorded(gpu, c):
    for got, exp in zip(gpu.pf_debug_index(6, 21), c["index"]):
        assert np.array_equal(got, exp)


def test_refused_load_targets_keeps_the_context(gpu, case):
    g = case["g"]
    try:
        descending = g["toff"].copy()
        assert descending[5] < descending[6]
        descending[5], descending[6] = descending[6], descending[5]
        with pytest.raises(capi.MMGpuError, match="mmgpu_load_targets: offsets not monotone"):
            gpu.load_targets(g["tres"], descending, 21)
        answers_as_recorded(gpu, case)
        index_as_recorded(gpu, case)
        with pytest.raises(capi.MMGpuError, match="mmgpu_load_targets: sequence longer than 65535"):
            gpu.load_targets(np.zeros(65536, np.uint8), np.array([0, 65536], np.uint64), 21)
        answers_as_recorded(gpu, case)
        index_as_recorded(gpu, case)
    finally:
        restore(gpu, case)


def test_load_targets_that_fails_while_packing_leaves_an_empty_context(gpu, case):
    g = case["g"]
    try:
        res = g["tres"].copy()
        res[int(g["toff"][700]) + 3] = 21      # == alphabet: found only while the residues are packed
        with pytest.raises(capi.MMGpuError, match="mmgpu_load_targets: residue code >= alphabet"):
            gpu.load_targets(res, g["toff"], 21)
        with pytest.raises(capi.MMGpuError, match="no targets loaded"):
            gpu.sw_batch(case["mat"], 11, 1, case["sw_q"], mode=1)
        with pytest.raises(capi.MMGpuError, match="no index"):
            gpu.pf_batch(case["qs"], case["thr"], max_hits=300, ref_bins=2)
        with pytest.raises(capi.MMGpuError, match="no index"):
            gpu.pf_debug_index(6, 21)
    finally:
        restore(gpu, case)
    answers_as_recorded(gpu, case)


def test_refused_index_call_keeps_the_index(gpu, case):
    g = case["g"]
    tab = case["tab"]
    unsorted3 = np.ascontiguousarray(case["s3"][:, ::-1])      # every row ascending
    try:
        with pytest.raises(capi.MMGpuError, match="mmgpu_pf_load_index: score3 rows are not sorted by descending score"):
            gpu.pf_load_index(6, 21, True, unsorted3, case["i3"], tab["offsets"], tab["ids"], tab["pos"], g["blosum62_ungapped"])
        index_as_recorded(gpu, case)
        answers_as_recorded(gpu, case)
        with pytest.raises(capi.MMGpuError, match="mmgpu_pf_build_index: score3 rows are not sorted by descending score"):
            gpu.pf_build_index(6, 21, True, unsorted3, case["i3"], g["vtml80_kmer16"], case["thr"], g["blosum62_ungapped"])
        index_as_recorded(gpu, case)
        answers_as_recorded(gpu, case)
    finally:
        restore(gpu, case)


def test_message_names_its_entry_point(gpu, case):
    g = case["g"]
    try:
        with pytest.raises(capi.MMGpuError, match=r"mmgpu_pf_build_index: k must be in \[4, 15\]"):
            gpu.pf_build_index(3, 21, True, None, None, g["vtml80_kmer16"], case["thr"], g["blosum62_ungapped"])
        # a NULL ungapped matrix: the descriptor by hand (the wrapper would not build one)
        s3 = np.ascontiguousarray(case["s3"], np.int16)
        i3 = np.ascontiguousarray(case["i3"], np.uint32)
        km = np.ascontiguousarray(g["vtml80_kmer16"], np.int16)
        d = capi.PfIndexDesc(6, 21, 1, capi._ptr(s3), capi._ptr(i3), s3.shape[1], None, None, 0, None, None, None, None, 0, None)
        rc = gpu.L.mmgpu_pf_build_index(gpu.ctx, ctypes.byref(d), capi._ptr(km), case["thr"])
        assert rc != 0 and gpu.L.mmgpu_last_error().decode() == "mmgpu_pf_build_index: NULL table"
        index_as_recorded(gpu, case)
        answers_as_recorded(gpu, case)
    finally:
        restore(gpu, case)
