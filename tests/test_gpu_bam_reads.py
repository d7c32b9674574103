"""rb_dev_bam_reads (k_bamreads.hip) and rb_host_bam_reads through the C ABI, bit for bit against the plain-Python model of
tests/bam_reads_util.py (test_bam_reads_inputs.py holds the model and the case generators to what they claim): SEQ at every byte phase,
the reference sum at every seam of the row and wavefront form, who enters the pileup, the prefix maximum at every seam of its scan up to
the serial top level, first_unsorted, sentinels behind every output, the refusals -- and the composition rb_dev_bam_records ->
rb_dev_bam_reads -> rb_devreads_nucfreq on the stream against rb_host_nucfreq on host-decoded arrays."""
import numpy as np
import pytest

import rustybam_amd
import bam_rec_util as B
import bam_reads_util as R
import nf_util as N

pytestmark = pytest.mark.gpu
GUARD = 8
A5 = 0xA5A5A5A5A5A5A5A5
E_INVALID = -1  # RB_E_INVALID
NAMES = R.OUTS + ("first_unsorted",)


@pytest.fixture(scope="module")
def shape():
    return rustybam_amd.bam_reads_shape()


def _check(got, want, labels=None):
    n = len(want["start_key"])
    for k in NAMES:
        m = 1 if k == "first_unsorted" else n
        bad = np.nonzero(got[k][:m] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} of {m} differ, first {[(labels[i] if labels else int(i), int(got[k][i]), int(want[k][i])) for i in bad[:4]]}"
        assert len(got[k]) == m + GUARD and (got[k][m:] == A5).all(), f"{k}: written behind the {m} entries"


def _run_cases(engine, cases):
    data, off, ln = B.stream([b for _, b in cases])
    got = engine.bam_reads(data, off, ln, guard=GUARD)
    m = B.model(data, off, ln)
    for k in B.COLS + ("op_off",):  # (the columns the call reads are the model's)
        assert np.array_equal(got[k][:len(m[k])], m[k]), k
    _check(got, R.model(data, off, ln, m), [lb for lb, _ in cases])
    return (data, off, ln), got


def _run_uniform(engine, u, **kw):
    data, off, ln = R.uniform_stream(u)
    got = engine.bam_reads(data, off, ln, guard=GUARD, **kw)
    _check(got, R.uniform_model(u, off))
    return (data, off, ln), got


def test_shape_query(shape):
    assert shape[0] == 16 * 4 and shape[2] == 64 * 4 and shape[1] >= shape[0] and shape[3] >= 64 and shape[3] % 64 == 0


GROUPS = {"seq": lambda s: R.seq_cases(), "ref": R.ref_cases, "enters": lambda s: R.enters_cases()}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_case_equals_the_model(engine, shape, group):
    _run_cases(engine, GROUPS[group](shape))


def test_the_groups_dealt_into_one_another(engine, shape):
    """the four records of a wavefront are of different kinds; the long CIGARs share wavefronts with short ones"""
    lists = [R.seq_cases(), R.ref_cases(shape), R.enters_cases()]
    n = max(len(ls) for ls in lists)
    _run_cases(engine, [ls[k % len(ls)] for k in range(n) for ls in lists])


def test_record_counts_of_the_scan(engine, shape):
    """0, 1, a wavefront's and a workgroup's seams; the workgroups' maxima in their first and last records, runs of reads that do not enter
    across the seams, a tid step; enough workgroups to reach the scan's top level, plus 1"""
    for n in R.scan_counts(shape[3]):
        _run_uniform(engine, R.scan_file(n, shape[3]))


@pytest.mark.parametrize("label", sorted(R.unsorted_files()))
def test_first_unsorted(engine, label):
    u, want = R.unsorted_files()[label]
    _, got = _run_uniform(engine, u)
    assert int(got["first_unsorted"][0]) == want


def test_second_call_and_host_twin_write_the_same(engine, shape):
    """whatever the buffers held: the outputs of a second call on other garbage, and rb_host_bam_reads' columns of both calls"""
    cases = (R.seq_cases() + R.enters_cases() + R.ref_cases(shape))[:700]
    (data, off, ln), got = _run_cases(engine, cases)
    again = engine.bam_reads(data, off, ln, guard=GUARD)
    for k in NAMES:
        assert again[k].tobytes() == got[k].tobytes(), k
    host = engine.host_bam_reads(data, off, ln)
    n, total = len(cases), int(got["op_off"][len(cases)])
    for k in B.COLS + R.OUTS:
        assert np.array_equal(host[k], got[k][:n]), k
    assert np.array_equal(host["op_off"], got["op_off"][:n + 1]) and np.array_equal(host["ops"][:total], got["ops"][:total])
    assert host["first_unsorted"][0] == got["first_unsorted"][0]
    u = R.scan_file(2 * shape[3] + 3, shape[3])
    data, off, ln = R.uniform_stream(u)
    host = engine.host_bam_reads(data, off, ln)
    want = R.uniform_model(u, off)
    for k in NAMES:
        assert np.array_equal(host[k], want[k]), k


def test_refusals(engine):
    """a misaligned scratch and a needed NULL: RB_E_INVALID, and nothing is written"""
    u, _ = R.unsorted_files()["at_1"]
    data, off, ln = R.uniform_stream(u)
    got = engine.bam_reads(data, off, ln, guard=GUARD, keep=True)
    try:
        d, n = got["dev"], len(off)
        scr = (d["reads_scratch"] + 255) & ~255
        args = [d["data"], d["rec_off"], d["rec_len"], n, d["tid"], d["pos"], d["flag"], d["op_off"], d["ops"], d["status"], d["seq_off"], d["start_key"],
                d["end_key_pmax"], d["first_unsorted"], scr]
        assert engine.dev_bam_reads(*args, check=False) == 0
        bad = list(args)
        bad[14] = scr + 128
        assert engine.dev_bam_reads(*bad, check=False) == E_INVALID
        for k in (0, 1, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14):
            bad = list(args)
            bad[k] = 0
            assert engine.dev_bam_reads(*bad, check=False) == E_INVALID, k
        bad = list(args)
        bad[3], bad[13] = 0, 0  # (n == 0 still needs first_unsorted)
        assert engine.dev_bam_reads(*bad, check=False) == E_INVALID
        engine.sync()
        for k in NAMES:
            after = np.zeros_like(got[k])
            engine._down(after, d[k])
            engine.sync()
            assert after.tobytes() == got[k].tobytes(), k
    finally:
        got["free"]()


@pytest.mark.parametrize("seed", [3, 4])
def test_composition_with_nucfreq_on_the_stream(engine, seed):
    """rb_dev_bam_records -> rb_dev_bam_reads -> rb_devreads_nucfreq with seq = the stream, on a slice with i0 > 0, against rb_host_nucfreq on
    the host-decoded arrays of the same reads: counts, read_status and counters"""
    rng = np.random.default_rng(seed)
    reads = N.random_reads(rng, 500, n_contig=2, span=5000, max_ops=14)
    data, off, ln = R.reads_stream(reads)
    got = engine.bam_reads(data, off, ln, guard=GUARD, keep=True)
    try:
        d, n = got["dev"], reads.n
        assert np.array_equal(got["tid"][:n], reads.tid) and np.array_equal(got["l_seq"][:n], reads.l_seq) and (got["status"][:n + 1] == 0).all()
        md = {k: got[k][:n + 1] for k in R.OUTS}
        regions = [(1, 1200, 2600), (1, 2000, 2100), (1, 2599, 4000), (1, 1500, 1500)]  # (contig 1: the slice starts behind contig 0's reads)
        i0, i1 = R.slice_of(md, 1, 1200, 4000)
        assert int((reads.tid == 0).sum()) <= i0 < i1 <= n and i0 > 100
        rg = np.array(regions, np.int64)
        want = engine.nucfreq(*reads.slice(i0, i1).args(), rg[:, 0], rg[:, 1], rg[:, 2])
        have = engine.devreads_nucfreq(i1 - i0, d["ops"], d["op_off"] + 8 * i0, d["data"], d["seq_off"] + 8 * i0, d["l_seq"] + 4 * i0, d["tid"] + 4 * i0,
                                       d["pos"] + 8 * i0, d["flag"] + 4 * i0, rg[:, 0], rg[:, 1], rg[:, 2])
        assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1]) and have[2] == want[2]
        assert want[2]["n_covered"] > 2000 and (want[1] != 0).any() and (want[1] == 0).sum() > 50
        whole = engine.nucfreq(*reads.args(), rg[:, 0], rg[:, 1], rg[:, 2])  # (the slice holds every read that reaches the regions)
        assert np.array_equal(whole[0], want[0])
        # the lines of the same slice
        seg_cnt, seg_pos, seg_n = [0, 1400], [1200, 2000], [1400, 100]
        want_t = engine.nucfreq_text(*reads.slice(i0, i1).args(), rg[:, 0], rg[:, 1], rg[:, 2], seg_cnt, seg_pos, seg_n, mode=rustybam_amd.capi.NFT_SMALL)
        have_t = engine.devreads_nucfreq_text(i1 - i0, d["ops"], d["op_off"] + 8 * i0, d["data"], d["seq_off"] + 8 * i0, d["l_seq"] + 4 * i0,
                                              d["tid"] + 4 * i0, d["pos"] + 8 * i0, d["flag"] + 4 * i0, rg[:, 0], rg[:, 1], rg[:, 2], seg_cnt, seg_pos, seg_n,
                                              mode=rustybam_amd.capi.NFT_SMALL)
        assert [s[3] for s in have_t[0]] == [s[3] for s in want_t[0]] and sum(len(s[3]) for s in want_t[0]) > 1000
        assert np.array_equal(have_t[1], want_t[1]) and have_t[2] == want_t[2]
    finally:
        got["free"]()
