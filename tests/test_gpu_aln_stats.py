"""rb_dev_parse_md and rb_dev_aln_stats (k_alnstats.hip) through the C ABI, bit for bit against the plain-Python models of tests/sam_util.py
(test_sam_inputs.py holds those to the oracle): MD strings at every lane, step and threshold seam of the kernel, spans at every
combination of clips and every panic, floats compared as their 32 bits, sentinels behind every output."""
import numpy as np
import pytest

import rustybam_amd
import sam_util as U
from rbtest_util import pack

pytestmark = pytest.mark.gpu
GUARD = 8


def _check_md(out, status, want, labels, n):
    bad = [labels[i] for i in range(n) if (tuple(int(x) for x in out[i]), int(status[i])) != want[i]]
    assert not bad, f"{len(bad)} strings differ, first: {bad[:8]}; e.g. got {out[labels.index(bad[0])]} want {want[labels.index(bad[0])]}"
    assert (out[n:] == 0xA5A5A5A5).all() and (status[n:] == 0xA5).all(), "written behind the n results"


@pytest.fixture(scope="module")
def md_seams(engine):
    """one call over every seam case, shared by the tests below: (cases, text, off, end, out, status, want)"""
    shape = rustybam_amd.md_shape()
    cases = U.md_cases(shape)
    text, off, end = U.md_layout(cases)
    out, status = engine.parse_md(text, off, end, guard=GUARD)
    want = [U.md_model(c[1]) for c in cases]
    return cases, text, off, end, out, status, want


def test_shape_query():
    row_step, row_max, wave_step = rustybam_amd.md_shape()
    assert row_step == 16 * 16 and wave_step == 64 * 16 and row_max >= row_step


def test_md_every_seam_case_equals_the_model(md_seams):
    cases, _, _, _, out, status, want = md_seams
    _check_md(out, status, want, [c[0] for c in cases], len(cases))
    by = {c[0]: i for i, c in enumerate(cases)}
    assert tuple(out[by["KA6"]]) == (23, 3, 1, 4) and tuple(out[by["empty"]]) == (0, 0, 0, 0) and status[by["empty"]] == U.MD_OK
    assert tuple(out[by["999999999"]]) == (999999999, 0, 0, 0)
    unusual = {c[0] for c, s in zip(cases, status) if s == U.MD_UNUSUAL}
    assert unusual == {"ten_digits", "ten_zeros", "all_256_bytes_back_and_forth"}  # and only those
    assert (out[[by[k] for k in unusual]] == 0).all()


def test_md_host_twin_and_second_call_write_the_same(engine, md_seams):
    cases, text, off, end, out, status, _ = md_seams
    n = len(cases)
    h_out, h_status = engine.host_parse_md(text, off, end)
    assert np.array_equal(h_out, out[:n]) and np.array_equal(h_status, status[:n])
    out2, status2 = engine.parse_md(text, off, end, guard=GUARD)
    assert out2.tobytes() == out.tobytes() and status2.tobytes() == status.tobytes()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257])
def test_md_strings_per_call(engine, md_seams, n):
    """n strings, back to back without a byte between them: short ones, one of every form of the kernel, one unusual"""
    cases = md_seams[0]
    row_max = rustybam_amd.md_shape()[1]
    pick = [c for c in cases if c[0] in ("KA6", "ten_digits", f"length_{row_max + 1}", "caret_end", "deletion_run_17", "empty", "wraps_2^32")]
    strs = [pick[i % len(pick)][1] if i % 3 == 0 else b"%dA%d^CG%d" % (i, 7 * i, i % 5) for i in range(n)]
    labels = [f"#{i}" for i in range(n)]
    text = b"".join(strs)
    end = np.cumsum([len(s) for s in strs]).astype(np.uint64)
    off = np.concatenate([[0], end[:-1]]).astype(np.uint64)
    out, status = engine.parse_md(text, off, end, guard=GUARD)
    _check_md(out, status, [U.md_model(s) for s in strs], labels, n)


def test_md_empty_and_reversed_extents_read_nothing(engine, md_seams):
    _, text, off, end, _, _, _ = md_seams
    n = 9
    o = np.array([int(off[5 + i]) + 3 for i in range(n)], np.uint64)
    e = o.copy()
    e[::2] -= 2  # an end in front of the start
    out, status = engine.parse_md(text, o, e, guard=GUARD)
    assert (out[:n] == 0).all() and (status[:n] == U.MD_OK).all() and (out[n:] == 0xA5A5A5A5).all() and (status[n:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------- spans
def _long_cases():
    """more ops between the two ends than a lane checks alone: a hard clip deep inside, a pad (legal) deep inside, neither"""
    body = "3=1X2I4=1D" * 40
    return [U._rec("long_ok", "5H" + body + "6=7S", 16), U._rec("long_pad_inside", "5S" + body + "2P" + body + "6=", 0),
            U._rec("long_H_inside", body + "3H" + body + "6=", 0), U._rec("long_H_inside_ends_in_D", "2S" + body + "3H" + body + "6=4D", 16),
            U._rec("long_H_behind_last_base", body + "6=3H2S", 0, l_seq=2 + 40 * 10 + 6)]


def _aln_inputs(recs):
    cig = [pack("".join(f"{n}{c}" for n, c in r["cigar"])) for r in recs]
    op_off = np.zeros(len(recs) + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cig])
    ops = np.concatenate(cig + [np.zeros(0, np.uint32)]).astype(np.uint32)
    mds = [r["md"] or b"" for r in recs]
    md_end = np.cumsum([len(m) for m in mds]).astype(np.uint64)
    md_off = np.concatenate([[0], md_end[:-1]]).astype(np.uint64)
    cols = dict(pos=[r["pos"] for r in recs], flag=[r["flag"] for r in recs], l_seq=[r["l_seq"] for r in recs],
                has_md=np.array([r["md"] is not None for r in recs], np.uint8))
    return ops, op_off, b"".join(mds), md_off, md_end, cols


def _run_aln(engine, recs, with_md=True):
    ops, op_off, md_text, md_off, md_end, c = _aln_inputs(recs)
    n = len(recs)
    z = np.zeros(n, np.uint64)
    red, _ = engine.scan_records(ops, op_off, z, z, z, z, np.full(n, ord("+"), np.uint8))
    kw = {}
    if with_md:
        md, md_status = engine.parse_md(md_text, md_off, md_end)
        kw = dict(md=md, md_status=md_status, has_md=c["has_md"])
    rows = engine.aln_stats(ops, op_off, red, c["pos"], c["flag"], c["l_seq"], guard=GUARD, **kw)
    host = engine.host_aln_stats(ops, op_off, red, c["pos"], c["flag"], c["l_seq"], **kw)
    assert host.tobytes() == rows[:n].tobytes(), "rb_host_aln_stats differs from rb_dev_aln_stats"
    assert (rows[n:].view(np.uint8) == 0xA5).all(), "written behind the n rows"
    return rows[:n]


def _check_rows(rows, recs, want):
    bad = [r["name"] for r, g, w in zip(recs, rows, want) if g.tobytes() != w.tobytes()]  # (floats as their bits)
    first = [r["name"] for r in recs].index(bad[0]) if bad else 0
    assert not bad, f"{len(bad)} rows differ, first: {bad[:8]}; {bad[:1]}: got {rows[first]} want {want[first]}"


@pytest.fixture(scope="module")
def all_recs():
    return [r for r in U.span_cases() if not r["flag"] & 4] + list(U.panic_cases().values()) + _long_cases()


def test_spans_equal_the_model(engine, all_recs):
    rows = _run_aln(engine, all_recs)
    want = [U.span_model(r) for r in all_recs]
    _check_rows(rows, all_recs, want)
    st = {r["name"]: int(w["status"]) for r, w in zip(all_recs, want)}
    assert st["ends_in_D"] == st["ends_in_N"] == st["only_I"] == st["no_ops"] == U.ALN_NONE and st["starts_with_D"] == st["starts_with_HD"] == U.ALN_DEL_FIRST
    assert st["H_in_the_middle"] == st["long_H_inside"] == st["long_H_inside_ends_in_D"] == U.ALN_HARDCLIP and st["md_disagrees"] == U.ALN_MD_ASSERT
    assert st["long_ok"] == st["long_pad_inside"] == st["long_H_behind_last_base"] == st["H_behind_the_last_base"] == st["md_with_eq"] == U.ALN_OK
    assert st["md_zero_padded"] == (U.ALN_MD_STATUS | U.MD_UNUSUAL)
    fl = {r["name"]: int(g["flags"]) for r, g in zip(all_recs, rows)}
    assert fl["m_without_md"] == fl["m_without_md2"] == U.ALN_WARN_M and fl["md_refines"] == 0 and fl["clip_00_0"] == 0


def test_spans_without_any_md(engine, all_recs):
    """has_md NULL: no record has an MD"""
    recs = [dict(r, md=None) for r in all_recs]
    _check_rows(_run_aln(engine, recs, with_md=False), recs, [U.span_model(r) for r in recs])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_alignments_per_call(engine, all_recs, n):
    recs = [dict(all_recs[(5 * i) % len(all_recs)], pos=1000 + i) for i in range(n)]
    _check_rows(_run_aln(engine, recs), recs, [U.span_model(r) for r in recs])
