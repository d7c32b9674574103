"""rb_dev_parse_md and rb_dev_aln_stats (k_alnstats.hip) through the C ABI on the deep record set of tests/sam_deep_util.py and on a
randomised differential, bit for bit against the plain-Python models of tests/sam_util.py (test_sam_deep_inputs.py holds them to the
oracle on these same inputs).  The MD text buffer of the deep set is the SAM text itself: offsets into it, real neighbours, every phase.
Floats are compared as their 32 bits, sentinels stand behind every output, and the host twins must write the same bytes."""
import numpy as np
import pytest

import rustybam_amd
import sam_deep_util as D
import sam_util as U
from rbtest_util import pack

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def shape():
    assert rustybam_amd.md_shape() == D.SHAPE, "the deep set is built for another shape of rb_k_parse_md"
    return D.SHAPE


def _check_md(out, status, want, labels):
    n = len(want)
    bad = [i for i in range(n) if (tuple(int(x) for x in out[i]), int(status[i])) != want[i]]
    assert not bad, f"{len(bad)} strings differ, first: {[labels[i] for i in bad[:8]]}; got {out[bad[0]]} / {status[bad[0]]} want {want[bad[0]]}"
    assert (out[n:] == 0xA5A5A5A5).all() and (status[n:] == 0xA5).all(), "written behind the n results"


def _columns(mapped):
    cig = [pack("".join(f"{n}{c}" for n, c in r["cigar"])) for r in mapped]
    op_off = np.zeros(len(mapped) + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cig])
    return np.concatenate(cig).astype(np.uint32), op_off, dict(pos=[r["pos"] for r in mapped], flag=[r["flag"] for r in mapped], l_seq=[r["l_seq"] for r in mapped],
                                                                  has_md=np.array([r["md"] is not None for r in mapped], np.uint8))


def _through_the_abi(engine, refs, recs):
    """the records' columns through parse_md (on the SAM text), the record scan and aln_stats -> (mapped, md out, md status, rows)"""
    mapped = D.mapped_of(recs)
    n = len(mapped)
    sam, md_off, md_end = D.sam_with_md_extents(refs, recs)
    md, md_status = engine.parse_md(sam, md_off, md_end, guard=GUARD)
    h_md, h_status = engine.host_parse_md(sam, md_off, md_end)
    assert h_md.tobytes() == md[:n].tobytes() and h_status.tobytes() == md_status[:n].tobytes(), "rb_host_parse_md differs from rb_dev_parse_md"
    ops, op_off, c = _columns(mapped)
    z = np.zeros(n, np.uint64)
    red, _ = engine.scan_records(ops, op_off, z, z, z, z, np.full(n, ord("+"), np.uint8))
    kw = dict(md=md[:n], md_status=md_status[:n], has_md=c["has_md"])
    rows = engine.aln_stats(ops, op_off, red, c["pos"], c["flag"], c["l_seq"], guard=GUARD, **kw)
    host = engine.host_aln_stats(ops, op_off, red, c["pos"], c["flag"], c["l_seq"], **kw)
    assert host.tobytes() == rows[:n].tobytes(), "rb_host_aln_stats differs from rb_dev_aln_stats"
    assert (rows[n:].view(np.uint8) == 0xA5).all(), "written behind the n rows"
    return mapped, md, md_status, rows[:n]


def _check_rows(rows, mapped):
    want = [U.span_model(r) for r in mapped]
    bad = [i for i, (g, w) in enumerate(zip(rows, want)) if g.tobytes() != w.tobytes()]  # (floats as their bits)
    assert not bad, f"{len(bad)} rows differ, first: {[(i, mapped[i]['name']) for i in bad[:8]]}; got {rows[bad[0]]} want {want[bad[0]]}"
    return want


def test_the_deep_set_equals_the_models(engine, shape):
    refs, recs = D.deep_set(shape)
    mapped, md, md_status, rows = _through_the_abi(engine, refs, recs)
    assert len(mapped) == D.N_MAPPED
    _check_md(md, md_status, [U.md_model(r["md"] or b"") for r in mapped], [r["name"] for r in mapped])
    want = _check_rows(rows, mapped)
    declined = [i for i, w in enumerate(rows) if w["status"] & U.ALN_MD_STATUS]
    assert declined == list(D.DECLINE_AT) and all(w["status"] == U.ALN_OK for i, w in enumerate(want) if i not in declined)
    assert sum(1 for s in md_status[:len(mapped)] if s == U.MD_UNUSUAL) > D.N_DECLINES  # (a padded number in an MD nobody asks about)


@pytest.mark.parametrize("name", sorted(set(D.PANIC_AT) - {"cigar_text"}))  # (the SAM line edit has no records of its own)
def test_a_panic_row_deep_in_the_set(engine, shape, name):
    """the replaced record's row is the panic, and every other row is what it was"""
    refs, _ = D.deep_set(shape)
    v = D.panic_variants(shape)[name]
    mapped, md, md_status, rows = _through_the_abi(engine, refs, v["recs"])
    _check_md(md, md_status, [U.md_model(r["md"] or b"") for r in mapped], [r["name"] for r in mapped])
    want = _check_rows(rows, mapped)
    assert [i for i, w in enumerate(want) if w["status"] != U.ALN_OK and not w["status"] & U.ALN_MD_STATUS] == [v["index"]]
    assert 32 <= rows[v["index"]]["status"] < U.ALN_MD_STATUS


@pytest.fixture(scope="module")
def hostile(shape):
    strs = D.random_md_strings(shape)
    want = [U.md_model(s) for s in strs]
    assert any(w[1] == U.MD_UNUSUAL for w in want) and any(w[1] == U.MD_OK and len(s) > shape[1] for s, w in zip(strs, want))
    return strs, want


def test_hostile_strings_back_to_back(engine, hostile):
    strs, want = hostile
    text, off, end = D.pack_strings(strs)
    assert len(text) == sum(map(len, strs))  # no byte between them
    out, status = engine.parse_md(text, off, end, guard=GUARD)
    _check_md(out, status, want, [f"#{i} ({len(s)} bytes)" for i, s in enumerate(strs)])
    unusual = [i for i, w in enumerate(want) if w[1] == U.MD_UNUSUAL]
    assert (out[unusual] == 0).all() and (status[unusual] == U.MD_UNUSUAL).all()  # zeroed, and the status says so
    h_out, h_status = engine.host_parse_md(text, off, end)
    assert h_out.tobytes() == out[:len(strs)].tobytes() and h_status.tobytes() == status[:len(strs)].tobytes()


@pytest.mark.parametrize("phase", range(16))
def test_hostile_strings_at_every_phase(engine, hostile, phase):
    strs, want = hostile
    text, off, end = D.pack_strings(strs, phase)
    assert all(int(o) % 16 == phase for o in off)
    out, status = engine.parse_md(text, off, end, guard=GUARD)
    _check_md(out, status, want, [f"#{i} ({len(s)} bytes) at phase {phase}" for i, s in enumerate(strs)])
