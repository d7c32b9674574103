"""rb_dev_bam_records (k_bam.hip) through the C ABI, bit for bit against the plain-Python model of tests/bam_rec_util.py
(test_bam_rec_inputs.py holds the model to sam_util.read_bam and to the oracle, and the case generators to what they claim): the gather at
every source byte phase and destination dword phase, the aux walk at every type, length, threshold and way to stop, the long-CIGAR
convention, the three refusals in their order, sentinels behind every output array and behind ops[total]."""
import numpy as np
import pytest

import rustybam_amd
import bam_rec_util as B
import sam_util as U

pytestmark = pytest.mark.gpu
GUARD = 8
A5 = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}


def _check(got, want, labels, cap=None):
    n = len(labels)
    for k in B.COLS + ("op_off",):
        m = n + (k == "op_off")
        bad = np.nonzero(got[k][:m] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} records differ, first {[(labels[min(i, n - 1)], int(got[k][i]), int(want[k][i])) for i in bad[:4]]}"
        assert (got[k][m:].view(f"u{got[k].itemsize}") == A5[got[k].itemsize]).all(), f"{k}: written behind the {m} entries"
    total = int(want["op_off"][n])
    cap = len(got["ops"]) - GUARD if cap is None else cap
    k = min(total, cap)
    bad = np.nonzero(got["ops"][:k] != want["ops"][:k])[0]
    if len(bad):
        r = int(np.searchsorted(want["op_off"], bad[0], side="right")) - 1
        raise AssertionError(f"ops: {len(bad)} words differ, first at {bad[0]} = word {int(bad[0] - want['op_off'][r])} of {labels[r]}: "
                             f"{got['ops'][bad[0]]:#x} for {want['ops'][bad[0]]:#x}")
    assert (got["ops"][k:] == 0xA5A5A5A5).all(), f"written at or behind ops[{k}] (total {total}, capacity {cap})"


def _run(engine, cases, **kw):
    data, off, ln = B.stream([b for _, b in cases])
    return (data, off, ln), engine.bam_records(data, off, ln, guard=GUARD, **kw), B.model(data, off, ln)


@pytest.fixture(scope="module")
def shape():
    return rustybam_amd.bam_shape()


def test_shape_query(shape):
    assert shape[0] == 16 * 16 and shape[2] == 64 * 16 and shape[1] >= shape[0] and shape[3] == 16 * 4 and shape[5] == 64 * 4 and shape[4] >= shape[3]


GROUPS = {"gather": lambda s: B.gather_cases(s[4]), "aux": lambda s: B.aux_cases(s[1]), "cg": lambda s: B.cg_cases(), "status": lambda s: B.status_cases(),
          "fields": lambda s: B.field_cases()}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_case_equals_the_model(engine, shape, group):
    cases = GROUPS[group](shape)
    _, got, want = _run(engine, cases)
    _check(got, want, [lb for lb, _ in cases])
    if group == "status":
        assert sorted(set(want["status"].tolist())) == [0, 1, 2, 3]
    if group == "cg":
        n_ops = np.diff(want["op_off"]).tolist()
        assert 65536 in n_ops and 70000 in n_ops


@pytest.fixture(scope="module")
def mixed(shape):
    """the case lists dealt into one another, so that the four records of a wavefront are of different kinds (the two largest CIGARs left out)"""
    lists = [B.aux_cases(shape[1]), B.status_cases(), [c for c in B.cg_cases() if c[0] not in ("applies_65536", "applies_70000")], B.field_cases()]
    small = [c for c in B.gather_cases(shape[4]) if len(c[1]) < 400]
    out, k = [], 0
    while len(out) < 2049:
        out.append(small[k % len(small)])
        for ls in lists:
            out.append(ls[k % len(ls)])
        k += 1
    assert k > max(len(ls) for ls in lists)
    return out


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257, 2049])
def test_records_per_call(engine, mixed, n):
    cases = mixed[:n]
    _, got, want = _run(engine, cases)
    _check(got, want, [lb for lb, _ in cases])
    assert got["op_off"][0] == 0


@pytest.mark.parametrize("short_by", ["one", "all"])
def test_a_short_ops_array(engine, mixed, short_by):
    """the truncation contract: RB_OK, every column and op_off exact, nothing at or behind ops[ops_cap]"""
    cases = mixed[:600]
    data, off, ln = B.stream([b for _, b in cases])
    want = B.model(data, off, ln)
    total = int(want["op_off"][-1])
    assert total > 1000
    cap = total - 1 if short_by == "one" else 0
    got = engine.bam_records(data, off, ln, ops_cap=cap, guard=GUARD)
    _check(got, want, [lb for lb, _ in cases], cap=cap)
    assert int(got["op_off"][len(cases)]) == total > cap


def test_second_call_and_host_twin_write_the_same(engine, mixed):
    cases = mixed[:700]
    (data, off, ln), got, want = _run(engine, cases)
    _check(got, want, [lb for lb, _ in cases])
    again = engine.bam_records(data, off, ln, guard=GUARD)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes(), k
    host = engine.host_bam_records(data, off, ln)
    n, total = len(cases), int(want["op_off"][-1])
    for k in B.COLS:
        assert np.array_equal(host[k], got[k][:n]), k
    assert np.array_equal(host["op_off"], got["op_off"][:n + 1]) and np.array_equal(host["ops"][:total], got["ops"][:total]) and (host["ops"][total:] == 0).all()
    short = engine.host_bam_records(data, off, ln, ops_cap=total - 5)
    assert np.array_equal(short["op_off"], host["op_off"]) and np.array_equal(short["ops"], host["ops"][:total - 5])


def _md_case_records():
    """a record per MD seam case of sam_util.md_cases: one M of as many bases as the MD accounts for, where that can be packed"""
    out = []
    for i, (label, s, _, _, _) in enumerate(U.md_cases(rustybam_amd.md_shape())):
        k = sum(U.md_host(s.split(b"\0")[0])[:2])
        cg = [(k, "M")] if 0 < k < 2**28 else [(20, "M")]
        out.append(dict(name=f"md{i}", ref=0, pos=1000 + i, flag=16 * (i % 2), l_seq=20, cigar=cg, md=s, nm=None))
    return out


def test_composition_columns_to_rows_equal_the_span_model(engine):
    """the columns as they lie on the device go into rb_dev_scan_records, rb_dev_parse_md (text = data) and rb_dev_aln_stats"""
    recs = U.span_cases() + list(U.panic_cases().values()) + _md_case_records()
    data = U.bam_bytes(U.REFS, recs)
    refs, off, ln = B.hop(data)
    want = B.model(data, off, ln)
    n = len(recs)
    as_read = B.records_of(data, off, ln, want, refs)
    for r, x in zip(recs, as_read):  # (an MD with a NUL inside ends there in a BAM)
        assert x["cigar"] == r["cigar"] and (r["flag"] & 4 or x["md"] == (None if r["md"] is None else bytes(r["md"]).split(b"\0")[0])), r["name"]
    got = engine.bam_records(data, off, ln, guard=GUARD, keep=True)
    try:
        _check(got, want, [r["name"] for r in recs])
        d = got["dev"]
        bufs = []
        try:
            zero = engine._up(bufs, np.zeros(n, np.uint64))
            strand = engine._up(bufs, np.full(n, ord("+"), np.uint8))
            red = engine._up(bufs, np.zeros(n, rustybam_amd.REDUCE_DT))
            md4, mst = np.full((n + GUARD, 4), 0xA5A5A5A5, np.uint32), np.full(n + GUARD, 0xA5, np.uint8)
            rows = np.frombuffer(np.full((n + GUARD) * 80, 0xA5, np.uint8).tobytes(), rustybam_amd.ALN_DT).copy()
            d_md, d_mst, d_rows = engine._up(bufs, md4), engine._up(bufs, mst), engine._up(bufs, rows)
            view = engine.batch_view(n, int(want["op_off"][-1]), d["ops"], d["op_off"], zero, zero, zero, zero, strand, 0)
            engine.dev_scan_records(view, red, 0)
            engine.dev_parse_md(d["data"], d["md_off"], d["md_end"], n, d_md, d_mst)
            engine.dev_aln_stats(view, red, d["pos"], d["flag"], d["l_seq"], d_md, d_mst, d["has_md"], d_rows)
            engine.sync()
            engine._down(rows, d_rows), engine._down(md4, d_md), engine._down(mst, d_mst)
        finally:
            engine.sync()
            for b in bufs:
                engine.dev_free(b)
    finally:
        got["free"]()
    assert (rows[n:].view(np.uint8) == 0xA5).all() and (md4[n:] == 0xA5A5A5A5).all() and (mst[n:] == 0xA5).all()
    bad = [r["name"] for r, g in zip(as_read, rows) if not r["flag"] & 4 and g.tobytes() != U.span_model(r).tobytes()]
    assert not bad, f"{len(bad)} rows differ from the span model, first {bad[:6]}"
    for r, g4, gs in zip(as_read, md4, mst):  # and the MD counts of every record that has one, needed by its CIGAR or not
        if not r["flag"] & 4 and r["md"] is not None:
            assert (tuple(int(x) for x in g4), int(gs)) == U.md_model(r["md"]), r["name"]
    ok = sum(1 for r, g in zip(as_read, rows) if not r["flag"] & 4 and g["status"] == 0)
    assert ok > 400  # (most MD seam cases refine their M: the MD the device found is the one its CIGAR needs)
