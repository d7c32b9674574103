"""The inputs and the model of the rb_dev_bam_records tests (tests/bam_rec_util.py) hold what they claim: the model's columns are what
sam_util.read_bam reads from the golden BAMs and from the synthetic sets, model + sam_util.stats_model is the oracle's output byte for byte
on every well-formed file (CG long CIGARs and two MD tags included), and the case generators cover every phase and threshold they are
there for.  No GPU here."""
import gzip
import os

import numpy as np
import pytest

import bam_rec_util as B
import sam_deep_util as D
import sam_util as U

SHAPES = [(256, 16384, 1024, 64, 4096, 256), (256, 2048, 1024, 64, 1024, 256)]  # the shipped shape and one a variant build could have


def _same_records(got, want):
    assert len(got) == len(want)
    for g, x in zip(got, want):
        for k in ("name", "ref", "pos", "flag", "l_seq", "cigar", "md"):
            if k in ("cigar", "md") and x["flag"] & 4:  # (an unmapped record: the call reports neither)
                continue
            assert g[k] == x[k], (x["name"], k, g[k], x[k])


@pytest.mark.parametrize("bam", ["asm_small.bam", "stats.bam", "test.bam"])
def test_model_reads_the_golden_bams_as_read_bam_does_and_gives_the_oracles_lines(oracle, golden, bam):
    path = os.path.join(golden, bam)
    data = gzip.decompress(open(path, "rb").read())
    refs, off, ln = B.hop(data)
    m = B.model(data, off, ln)
    want_refs, want = U.read_bam(path)
    assert refs == want_refs and (m["status"] == 0).all() and len(want) > 0
    recs = B.records_of(data, off, ln, m, refs)
    _same_records(recs, want)
    for qbed in (False, True):
        out, rc = U.stats_model(refs, recs, qbed)
        assert (rc, out) == oracle.cli("stats", *(["--qbed"] if qbed else []), path)


def _synthetic_sets():
    return {"span": (U.REFS, U.span_cases()), "panic": (U.REFS, list(U.panic_cases().values())), "deep": D.deep_set(D.SHAPE)}


@pytest.mark.parametrize("which", ["span", "panic", "deep"])
def test_model_reads_the_synthetic_sets_as_read_bam_does(tmp_path, which):
    refs, recs = _synthetic_sets()[which]
    data = U.bam_bytes(refs, recs)
    r2, off, ln = B.hop(data)
    m = B.model(data, off, ln)
    assert r2 == refs and (m["status"] == 0).all()
    path = tmp_path / "set.bam"
    U.write_bam(path, refs, recs)
    _same_records(B.records_of(data, off, ln, m, refs), U.read_bam(path)[1])
    _same_records(B.records_of(data, off, ln, m, refs), recs)


def _well_formed(cases):
    """the cases the oracle reads as the model does: no broken record, no unterminated Z, no overrunning B (the oracle reads past those)"""
    bad = ("unterminated", "overrun", "left_behind_3_is_a_head", "unknown_type", "op_nibbles", "md_as_H", "B_unknown_subtype")
    return [(lb, b) for lb, b in cases if not any(x in lb for x in bad)]


@pytest.mark.parametrize("which", ["aux", "cg", "fields"])
def test_model_and_stats_model_equal_the_oracle_on_well_formed_case_files(oracle, tmp_path, which):
    shape = SHAPES[0]
    cases = {"aux": B.aux_cases(shape[1]), "cg": B.cg_cases(), "fields": [c for c in B.field_cases() if "tid_" not in c[0]]}[which]  # (a mapped record without a reference is not well formed)
    cases = _well_formed(cases)
    assert len(cases) >= 3
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    assert (m["status"] == 0).all()
    recs = B.records_of(data, off, ln, m, B.REFS)
    labels = [lb for lb, _ in cases]
    if which == "cg":
        by = dict(zip(labels, recs))
        assert len(by["applies_3"]["cigar"]) == 3 and len(by["applies_65536"]["cigar"]) == 65536 and len(by["applies_70000"]["cigar"]) == 70000
        assert all(len(by[k]["cigar"]) == 2 for k in ("first_op_not_S", "S_length_is_not_l_seq", "subtype_i", "subtype_S", "tag_is_not_CG"))
        assert len(by["n_cigar_0"]["cigar"]) == 0 and len(by["two_tags_the_last_wins"]["cigar"]) == 3 and len(by["applies_zero_words_in_tag"]["cigar"]) == 0
        assert by["in_front_of_md"]["md"] == by["behind_md"]["md"] == b"3" and len(by["behind_md"]["cigar"]) == 3
    if which == "aux":
        by = dict(zip(labels, recs))
        assert by["md_twice"]["md"] == B.MD20 and by["md_twice_second_empty"]["md"] == b"" and by["md_absent"]["md"] is None
        assert by["md_as_i_is_not_md"]["md"] is None and by["Z_with_md_inside"]["md"] == B.MD20 and len(by["md_len_5000"]["md"]) == 5000
    path = tmp_path / f"{which}.bam"
    with gzip.open(path, "wb", compresslevel=1) as f:
        f.write(data)
    # a panic ends the reference's output: a new file begins behind every record that is one, so that every case is held to the oracle
    files, cur = [], []
    for r, (_, b) in zip(recs, cases):
        cur.append((r, b))
        if U.stats_model(B.REFS, [r], False)[1]:
            files.append(cur)
            cur = []
    files += [cur] if cur else []
    assert sum(len(f) for f in files) == len(cases)
    for k, fl in enumerate(files):
        path = tmp_path / f"{which}_{k}.bam"
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(B.stream([b for _, b in fl])[0])
        for qbed in (False, True):
            out, rc = U.stats_model(B.REFS, [r for r, _ in fl], qbed)
            assert (rc, out) == oracle.cli("stats", *(["--qbed"] if qbed else []), path), (which, k, [r["name"] for r, _ in fl][-3:])


def test_ill_formed_cases_are_what_they_claim():
    """held to the model only: what the walk found before it stopped counts"""
    shape = SHAPES[0]
    cases = B.aux_cases(shape[1])
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    by = {lb: i for i, (lb, _) in enumerate(cases)}

    def mdv(lb):
        i = by[lb]
        return data[int(m["md_off"][i]):int(m["md_end"][i])] if m["has_md"][i] else None
    assert mdv("md_unterminated") == b"3A3" and int(m["md_end"][by["md_unterminated"]]) == int(off[by["md_unterminated"]]) + int(ln[by["md_unterminated"]])
    assert mdv("md_unterminated_empty") == b"" and mdv("Z_unterminated_behind_md") == B.MD20 and len(mdv("wave_md_unterminated")) == 700
    assert mdv("unknown_type_in_front") is None and mdv("unknown_type_behind") == B.MD20
    assert mdv("B_head_overruns") == mdv("B_head_overruns_by_one") == mdv("B_array_overruns") == mdv("B_array_overruns_2^32") == B.MD20
    assert mdv("B_array_overrun_hides_md") is None and mdv("B_array_fits_exactly") == B.MD20 and mdv("md_as_H_is_not_md") is None
    for k in range(4):
        i = by[f"left_behind_{k}"]
        assert mdv(f"left_behind_{k}") == B.MD20 and cases[i][1].endswith((b"A" * 4 + b"ZZ\0"[:k]))
    assert len(mdv("wave_two_mds")) == 2500


@pytest.mark.parametrize("shape", SHAPES)
def test_case_generators_cover_what_they_claim(shape):
    aux_max, copy_max = shape[1], shape[4]
    # ---- gather: every source byte phase of a 16-byte group and every destination dword phase, with every n_cigar
    cases = B.gather_cases(copy_max)
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    src = B.source_of(data, off, ln, m)
    seen16, seen4 = set(), {}
    for (lb, _), s, d0, d1 in zip(cases, src, m["op_off"][:-1], m["op_off"][1:]):
        if not lb.startswith("gather_") or s is None:
            continue
        nc = int(d1 - d0)
        seen16.add((s % 16, int(d0) % 4))
        seen4.setdefault(nc, set()).add((s % 4, int(d0) % 4))
    assert seen16 == {(a, b) for a in range(16) for b in range(4)}
    want_nc = set(B.N_CIGARS + (copy_max - 1, copy_max, copy_max + 1)) - {0}
    assert set(seen4) == want_nc
    for nc in want_nc:
        assert seen4[nc] == {(a, b) for a in range(4) for b in range(4)}, nc
    names = {data[int(o) + 8] for (lb, _), o in zip(cases, off) if lb.startswith("gather_")}
    assert names == set(range(1, 21))
    # ---- aux: the NUL of an MD at every byte of a group, every MD length, the aux area at the threshold
    cases = B.aux_cases(aux_max)
    assert len({lb for lb, _ in cases}) == len(cases)
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    by = {lb: i for i, (lb, _) in enumerate(cases)}
    assert {int(m["md_end"][by[f"nul_phase_{p}"]]) % 16 for p in range(16)} == set(range(16))
    for n in list(range(34)) + [255, 256, 257, 5000]:
        i = by[f"md_len_{n}"]
        assert m["has_md"][i] and int(m["md_end"][i] - m["md_off"][i]) == n
    for d in (-1, 0, 1):
        for sfx in ("", "_md_first"):
            i = by[f"aux_area_{aux_max + d}{sfx}"]
            b = cases[i][1]
            aux0 = 32 + b[8] + 4 * 1 + 10 + 20
            assert len(b) - aux0 == aux_max + d and m["has_md"][i]
    for lb in ("wave_many_small_fields", "wave_long_Z_then_md", "wave_md_unterminated", "wave_two_mds"):
        assert len(cases[by[lb]][1]) > aux_max + 900 and m["has_md"][by[lb]]
    # ---- CG: the tag at every byte phase, applied
    cases = B.cg_cases()
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    src = B.source_of(data, off, ln, m)
    by = {lb: i for i, (lb, _) in enumerate(cases)}
    assert {src[by[f"tag_phase_{p}"]] % 16 for p in range(16)} == set(range(16))
    assert all(int(m["op_off"][by[f"tag_phase_{p}"] + 1] - m["op_off"][by[f"tag_phase_{p}"]]) == 21 for p in range(16))
    i = by["unmapped_with_tag"]
    assert m["op_off"][i + 1] == m["op_off"][i] and m["flag"][i] == 4
    # ---- statuses, in the order of the checks; every other column zero
    cases = B.status_cases()
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    st = {lb: int(m["status"][i]) for i, (lb, _) in enumerate(cases)}
    assert st["block_size_31"] == st["block_size_0"] == st["short_block_comes_first"] == B.BAM_SHORT_BLOCK
    assert st["block_size_32_no_name"] == st["l_read_name_0"] == st["name_without_nul"] == st["name_nul_only_inside"] == st["broken_unmapped_bad_name"] == B.BAM_BAD_NAME
    assert st["block_size_32_says_a_name"] == st["short_by_one"] == st["l_seq_2^32-1"] == st["l_seq_2^32-2"] == st["l_seq_wraps_to_fit_in_32_bits"] == B.BAM_NO_FIT
    assert st["n_cigar_says_more"] == st["no_fit_comes_before_bad_name"] == st["broken_unmapped_no_fit"] == B.BAM_NO_FIT
    assert st["block_size_33"] == st["fits_exactly"] == st["name_255"] == st["good_unmapped"] == st["ok_in_front"] == st["ok_behind"] == B.BAM_OK
    b = dict(cases)["l_seq_wraps_to_fit_in_32_bits"]
    assert (32 + 3 + (0xAAAAAAAA + 1) // 2 + 0xAAAAAAAA) % 2**32 <= len(b)  # (a sum in 32 bits would let it pass)
    for i in np.nonzero(m["status"])[0]:
        assert all(int(m[k][i]) == 0 for k in B.COLS if k != "status") and m["op_off"][i + 1] == m["op_off"][i]
    # ---- fields
    cases = B.field_cases()
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    assert {-1, B.INT32_MIN} <= set(m["tid"].tolist()) and {-1, B.INT32_MIN} <= set(m["pos"].tolist()) and m["pos"].dtype == np.int64
    assert 0xFFFF in m["flag"].tolist() and 0xFFFB in m["flag"].tolist()
    assert set((m["ops"][-7:] & 15).tolist()) == set(range(9, 16))
