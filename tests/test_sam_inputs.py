"""The inputs and models of the SAM stats tests (tests/sam_util.py) hold what they claim, and the models agree with the oracle: the MD
model with rbo_parse_md_for_stats on every string of the seam cases, the span model's lines with the oracle CLI on the BAM twin of every
record set the GPU tests use.  No GPU here: a model that drifted would otherwise pass or fail the GPU tests for the wrong reason."""
import ctypes as C
import gzip
import os

import pytest

import sam_util as U

SHAPES = [(256, 2048, 1024), (256, 512, 1024), (256, 4096, 1024)]  # the shipped shape and two a variant build could have


def _oracle_md(oracle, s):
    m4 = (C.c_uint32 * 4)()
    oracle.lib().rbo_parse_md_for_stats(bytes(s), m4)
    return tuple(m4)


@pytest.mark.parametrize("shape", SHAPES)
def test_md_cases_hold_what_they_claim_and_the_model_equals_the_oracle(oracle, shape):
    row_step, row_max, wave_step = shape
    cases = U.md_cases(shape)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    text, off, end = U.md_layout(cases)
    assert len(text) % 16 == 0
    unusual = set()
    for (label, s, phase, before, after), o, e in zip(cases, off, end):
        o, e = int(o), int(e)
        assert text[o:e] == s and o % 16 == phase and text[o - 1:o] == before and text[e:e + 1] == after, label
        counts, status = U.md_model(s)
        if status == U.MD_UNUSUAL:
            unusual.add(label)
        if 0 not in s:  # (the oracle takes a C string)
            assert U.md_host(s) == _oracle_md(oracle, s), label
        if status == U.MD_OK:
            assert counts == U.md_host(s), label
    assert unusual == {"ten_digits", "ten_zeros", "all_256_bytes_back_and_forth"} and U.md_model(b"10A3T0T10^ACGT") == ((23, 3, 1, 4), U.MD_OK)
    by = dict((c[0], c[1]) for c in cases)
    assert U.md_model(by["wraps_2^32"])[0][0] == (5 * 999999999) % 2**32 and 5 * 999999999 > 2**32
    assert set(by["all_256_bytes"]) == set(range(256))
    assert U.md_model(by["caret_caret"])[0] == (7, 0, 1, 1) and U.md_model(by["caret_digit"])[0] == (12, 1, 0, 0) and U.md_model(by["caret_end"])[0] == (12, 1, 0, 0)
    # the splits really straddle: k digits of the d in front of the boundary
    for d in range(1, 10):
        for k in range(d + 1):
            for label, at in ((f"lane_split_{d}_{k}", 16), (f"row_step_split_{d}_{k}", row_step), (f"row_step_split_at_end_{d}_{k}", row_step)):
                s = by[label]
                assert s[at - k:at - k + d] == b"123456789"[:d] and not s[at - k - 1:at - k].isdigit() and len(s) <= row_max, label
            s = by[f"wave_step_split_{d}_{k}"]
            assert s[wave_step - k:wave_step - k + d] == b"123456789"[:d] and len(s) > row_max
            s = by[f"wave_step_split_at_end_{d}_{k}"]
            assert s.endswith(b"A" + b"123456789"[:d]) and (len(s) - d + k) % wave_step == 0 and len(s) > row_max
    for label, at in (("lane", 16), ("row_step", row_step), ("wave_step", wave_step)):
        assert by[f"caret_last_of_{label}"][at - 1:at + 1] == b"^A" and by[f"caret_last_of_{label}_then_digit"][at - 1:at + 1] == b"^5"
    assert len(by["caret_last_of_wave_step"]) > row_max >= len(by["caret_last_of_row_step"])
    assert {len(by[f"length_{n}"]) for n in (row_max - 1, row_max, row_max + 1)} == {row_max - 1, row_max, row_max + 1}


def _twin_lines(oracle, tmp_path, refs, recs, name):
    bam = tmp_path / f"{name}.bam"
    U.write_bam(bam, refs, recs)
    return {qbed: oracle.cli("stats", *(["--qbed"] if qbed else []), bam) for qbed in (False, True)}


def test_span_model_equals_the_oracle_on_the_bam_twin(oracle, tmp_path):
    recs = U.span_cases()
    assert len({r["name"] for r in recs}) == len(recs) and sum(1 for r in recs if r["flag"] & 16) > 16
    got = _twin_lines(oracle, tmp_path, U.REFS, recs, "span")
    for qbed in (False, True):
        out, rc = U.stats_model(U.REFS, recs, qbed)
        assert (rc, out) == got[qbed] and rc == 0 and out.count(b"\n") == len(recs)  # header + every record but the unmapped one
    rows = {r["name"]: U.span_model(r) for r in recs if not r["flag"] & 4}
    assert rows["md_refines"]["equal"] == 28 and rows["md_refines"]["diff"] == 3 and rows["md_with_eq"]["equal"] == 10
    assert rows["m_without_md"]["flags"] == U.ALN_WARN_M and rows["md_refines"]["flags"] == 0
    assert rows["md_zero_padded"]["status"] == (U.ALN_MD_STATUS | U.MD_UNUSUAL)


@pytest.mark.parametrize("name", sorted(U.panic_cases()))
def test_panic_cases_panic_in_the_oracle_after_the_lines_before_them(oracle, tmp_path, name):
    good = U.span_cases()[:3]
    recs = good + [U.panic_cases()[name]] + U.span_cases()[3:6]
    got = _twin_lines(oracle, tmp_path, U.REFS, recs, name)
    for qbed in (False, True):
        out, rc = U.stats_model(U.REFS, recs, qbed)
        assert (rc, out) == got[qbed] and rc == 101 and out.count(b"\n") == 1 + 3, name
    assert U.span_model(U.panic_cases()[name])["status"] >= 32


@pytest.mark.parametrize("bam", ["asm_small.bam", "stats.bam", "test.bam", "test_nucfreq.bam"])
def test_golden_bam_reader_and_model_equal_the_oracle(oracle, golden, bam):
    refs, recs = U.read_bam(os.path.join(golden, bam))
    for qbed in (False, True):
        out, rc = U.stats_model(refs, recs, qbed)
        assert (rc, out) == oracle.cli("stats", *(["--qbed"] if qbed else []), os.path.join(golden, bam)), bam
    # the twin written back from the records is the same BAM as far as stats goes, and its SAM text has one line per record
    sam = U.sam_text(refs, recs)
    lines = [ln for ln in sam.split(b"\n") if ln and not ln.startswith(b"@")]
    assert len(lines) == len(recs) and all(ln.count(b"\t") >= 10 for ln in lines)
    for ln, r in zip(lines, recs):
        f = ln.split(b"\t")
        assert f[0].decode() == r["name"] and int(f[1]) == r["flag"] and int(f[3]) == r["pos"] + 1 and len(f[9]) == max(r["l_seq"], 1)


def test_the_reference_sam_fixture_is_the_nucfreq_bam(golden):
    raw = open(os.path.join(golden, "test.sam"), "rb").read()
    assert len(raw) == 819
    refs, recs = U.read_bam(os.path.join(golden, "test_nucfreq.bam"))
    head = [ln for ln in raw.split(b"\n") if ln.startswith(b"@SQ")]
    assert [(h.split(b"\t")[1][3:].decode(), int(h.split(b"\t")[2][3:])) for h in head] == refs
    lines = [ln.split(b"\t") for ln in raw.split(b"\n") if ln and not ln.startswith(b"@")]
    assert len(lines) == len(recs) == 2
    for f, r in zip(lines, recs):
        assert len(f) == 18 and f[5] == b"27M1D73M" and int(f[1]) == 16 == r["flag"] and int(f[3]) == r["pos"] + 1 and f[2].decode() == refs[r["ref"]][0]
        assert "".join(f"{n}{c}" for n, c in r["cigar"]) == "27M1D73M" and len(f[9]) == r["l_seq"] and r["md"] is None
        assert not any(x.startswith(b"MD:Z:") for x in f[11:])
    assert gzip.compress(raw)[:2] == b"\x1f\x8b"
