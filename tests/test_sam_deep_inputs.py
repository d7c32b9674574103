"""The deep record set of tests/sam_deep_util.py holds what it claims, and the models of tests/sam_util.py agree with the oracle on it: the
stats lines of the BAM twin (main set and every deep panic variant) and rbo_parse_md_for_stats on every generated MD string and on the
hostile strings of the randomised differential.  No GPU here: test_gpu_cli_stats_deep.py and test_gpu_aln_stats_deep.py compare the
product with these models and this oracle, and a generator that drifted must not let them pass for the wrong reason."""
import collections
import ctypes as C
import gzip
import re
import struct

import pytest

import sam_deep_util as D
import sam_util as U

SHAPE = (256, 2048, 1024)


@pytest.fixture(scope="module")
def deep():
    assert D.SHAPE == SHAPE
    refs, recs = D.deep_set(SHAPE)
    return refs, recs, D.mapped_of(recs)


def _oracle_md(oracle, s):
    m4 = (C.c_uint32 * 4)()
    oracle.lib().rbo_parse_md_for_stats(bytes(s), m4)
    return tuple(m4)


def _cg(r):
    return "".join(f"{n}{c}" for n, c in r["cigar"])


def test_the_generator_is_seeded(deep):
    refs, recs, _ = deep
    D._CACHE.clear()
    assert D.deep_set(SHAPE) == (refs, recs)


def test_record_count_and_unmapped_records(deep):
    refs, recs, mapped = deep
    n = len(mapped)
    assert n == D.N_MAPPED >= 600 and n % 4 and n % 256 and n > 2 * 256
    assert len({r["name"] for r in recs}) == len(recs)
    un = [r for r in recs if r["flag"] & 4]
    assert len(un) > 20 and any(r["ref"] < 0 for r in un) and any(r["ref"] >= 0 for r in un)
    # interleaved: unmapped records in front of mapped ones of every block, and the file's last record is mapped
    at = [i for i, r in enumerate(recs) if r["flag"] & 4]
    behind = [sum(1 for r in recs[:i] if not r["flag"] & 4) for i in at]
    assert {b // 256 for b in behind} == {0, 1, 2} and not recs[-1]["flag"] & 4
    sam = U.sam_text(refs, recs)
    assert len(sam) < 4 << 20 and sam.count(b"\n") == len(recs) + 1 + len(refs)
    assert sum(1 for r in un if r["ref"] < 0) == sam.count(b"\t*\t0\t60\t*\t")


def test_every_md_follows_from_its_cigar(deep):
    _, _, mapped = deep
    with_md = [r for r in mapped if r["md"] is not None]
    assert len(with_md) > 300
    for r in with_md:
        c = U.counters(r["cigar"])
        (m, mm, ic, ib), unusual = U._md_counts(r["md"])
        assert m + mm == c["equal"] + c["diff"] and ib == c["del"] and ic == sum(1 for n, o in r["cigar"] if o == "D" and n), r["name"]
        assert mm >= sum(n for n, o in r["cigar"] if o == "X") and r["md"][-1:].isdigit() and r["md"][:1].isdigit()


def test_md_lengths_and_wavefront_mixing(deep):
    _, _, mapped = deep
    row_step, row_max, wave_step = SHAPE
    lens = [len(r["md"] or b"") for r in mapped]
    for n in (row_max - 1, row_max, row_max + 1, 2 * row_max + 1):
        assert n in lens
    assert sum(1 for n in lens if n > 3 * wave_step) >= 8 and max(lens) > 4 * wave_step
    assert sum(1 for n in lens if n > row_max) >= 60  # dozens of wavefronts walk a string whole
    groups = [mapped[i:i + 4] for i in range(0, len(mapped) - 3, 4)]
    n_long = collections.Counter(sum(1 for r in g if len(r["md"] or b"") > row_max) for g in groups)
    assert set(n_long) == {0, 1, 2, 3, 4}
    # a long string and a record without MD in one wavefront, and one in the last (partial) wavefront's neighbourhood
    assert any(any(r["md"] is None for r in g) and any(len(r["md"] or b"") > row_max for r in g) for g in groups)


def test_cigar_ends_and_strands(deep):
    _, _, mapped = deep
    seen = set()
    for r in mapped:
        ops = [c for _, c in r["cigar"]]
        lead = "".join(ops[:2 if ops[:2] == ["H", "S"] else (1 if ops[0] in "HS" else 0)])
        k = 2 if ops[-2:] == ["S", "H"] else (1 if ops[-1] in "HS" else 0)
        trail = "".join(ops[len(ops) - k:])
        seen.add((lead, trail, r["flag"] & 16))
    assert seen == {(a, b, f) for a in ("", "H", "S", "HS") for b in ("", "S", "H", "SH") for f in (0, 16)}
    cg = [_cg(r) for r in mapped]
    for tail in ("2P", "0D", "0N", "3I", "3I2P"):
        for trail in D.TRAILS:
            assert any(c.endswith(tail + trail) and not c[:-len(tail + trail)][-1:] in "HS" for c in cg), (tail, trail)
    for lead in D.LEADS:
        assert any(c.startswith(lead + "3I") for c in cg), lead
    rev = sum(1 for r in mapped if r["flag"] & 16)
    assert .4 < rev / len(mapped) < .6


def test_ops_between_the_ends(deep):
    _, _, mapped = deep
    by = collections.defaultdict(list)
    for r in mapped:
        n = D.between_ends(r)
        by["lane" if n <= D.LANE_SCAN else ("one_step" if n <= 64 else ("two_steps" if n <= 128 else "more"))].append(r)
    assert all(len(by[k]) >= 4 for k in ("lane", "one_step", "two_steps", "more")), {k: len(v) for k, v in by.items()}
    assert {D.between_ends(r) for r in mapped} >= {32, 33, 64, 65}  # both sides of the lane / wavefront threshold and of one step
    for k in ("one_step", "two_steps", "more"):  # a pad deep inside: legal
        assert any("P" in [c for _, c in r["cigar"][20:-20]] for r in by[k]), k
    assert max(len(r["cigar"]) for r in mapped) > 2000


def test_md_situations_columns_and_declines(deep):
    refs, recs, mapped = deep
    sit = collections.Counter(D.situation(r) for r in mapped)
    assert all(sit[k] >= 40 for k in ("MD_refines", "MD_ignored", "M_without_MD", "no_M")), sit
    rows = [U.span_model(r) for r in mapped]
    assert sum(1 for w in rows if w["flags"] & U.ALN_WARN_M) == sit["M_without_MD"]
    assert .05 < sum(1 for r in mapped if r["l_seq"] == 0) / len(mapped) < .3
    assert [i for i, r in enumerate(mapped) if r["ref"] == 1] == [D.ON_SECOND_REF]
    ends = [r["pos"] + U.counters(r["cigar"])["t_bases"] for r in mapped]
    assert max(ends) == refs[0][1] < 2**31 and sum(1 for e in ends if e > refs[0][1] - 3) > 10 and all(r["pos"] >= 0 for r in mapped)
    assert all(e <= refs[r["ref"]][1] for e, r in zip(ends, mapped))
    # the designed declines: exactly the records whose row asks for the host
    declines = [i for i, w in enumerate(rows) if w["status"] == (U.ALN_MD_STATUS | U.MD_UNUSUAL)]
    assert declines == list(D.DECLINE_AT) and len(declines) == D.N_DECLINES
    assert {i // 256 for i in declines} == {0, 1, 2} and declines[-1] == len(mapped) - 1 and recs[-1] is not None and recs[-1]["name"] == mapped[-1]["name"]
    assert D.WARN_BEHIND_DECLINE - 1 in declines and rows[D.WARN_BEHIND_DECLINE]["flags"] == U.ALN_WARN_M
    row_max = SHAPE[1]
    assert any(len(mapped[i]["md"]) > row_max for i in declines) and any(len(mapped[i]["md"]) <= row_max for i in declines)
    for i in declines:
        assert max(len(x) for x in re.findall(rb"\d+", mapped[i]["md"])) >= 10 and D.situation(mapped[i]) == "MD_refines"
    # a padded number in an MD that is never asked about is no decline
    assert sum(1 for i, r in enumerate(mapped) if r["md"] and U.md_model(r["md"])[1] == U.MD_UNUSUAL and i not in declines) >= 3
    assert all(w["status"] == U.ALN_OK for i, w in enumerate(rows) if i not in declines)


def _twin(oracle, tmp_path, refs, recs, name, qbed):
    bam = tmp_path / f"{name}.bam"
    if not bam.exists():
        U.write_bam(bam, refs, recs)
    return oracle.cli("stats", *(["--qbed"] if qbed else []), bam)


@pytest.mark.parametrize("qbed", [False, True])
def test_the_oracle_prints_every_mapped_record_and_the_model_agrees(oracle, deep, tmp_path, qbed):
    refs, recs, mapped = deep
    rc, out = _twin(oracle, tmp_path, refs, recs, "deep", qbed)
    assert rc == 0 and out.count(b"\n") == 1 + len(mapped)
    lines = out.split(b"\n")[1:-1]
    assert all(r["name"].encode() == ln.split(b"\t")[0 if qbed else 5] for r, ln in zip(mapped, lines))  # no record is left out
    assert (out, rc) == U.stats_model(refs, recs, qbed)


def test_panic_variants_panic_in_the_oracle_behind_the_lines_before_them(oracle, deep, tmp_path):
    refs, recs, mapped = deep
    variants = D.panic_variants(SHAPE)
    assert set(variants) == set(D.PANIC_AT) and len(variants) == 7
    main = {q: _twin(oracle, tmp_path, refs, recs, "deep", q)[1] for q in (False, True)}
    want_status = {"md_disagrees_long": U.ALN_MD_ASSERT, "hardclip_deep": U.ALN_HARDCLIP, "starts_with_D": U.ALN_DEL_FIRST, "decline_and_hardclip": U.ALN_HARDCLIP,
                   "ends_in_D": U.ALN_NONE, "ends_in_N": U.ALN_NONE}
    for name, v in variants.items():
        k = v["index"]
        assert k > 256 and k // 256 != D.DECLINE_AT[0] // 256 and k not in D.DECLINE_AT and any(d < k for d in D.DECLINE_AT), name
        assert len(v["recs"]) == len(recs) and [a["name"] for a in D.mapped_of(v["recs"])[:k]] == [a["name"] for a in mapped[:k]]
        sam = D.variant_sam(refs, v)
        if v["sam_edit"]:
            assert name == "cigar_text" and v["recs"] == recs
            a, b = U.sam_text(refs, recs).split(b"\n"), sam.split(b"\n")
            diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
            assert len(a) == len(b) and diff == [len(refs) + 1 + D.file_index(recs, k)] and b[diff[0]].split(b"\t")[5] == D.BAD_CIGAR
            continue
        assert sam == U.sam_text(refs, v["recs"])
        assert U.span_model(D.mapped_of(v["recs"])[k])["status"] == want_status[name], name
        for qbed in (False, True):
            rc, out = _twin(oracle, tmp_path, refs, v["recs"], name, qbed)
            assert rc == 101 and out.count(b"\n") == 1 + k and main[qbed].startswith(out), name  # exactly the lines in front of the record
            assert (out, rc) == U.stats_model(refs, v["recs"], qbed), name
    row_max, wave_step = SHAPE[1], SHAPE[2]
    bad = {n: D.mapped_of(v["recs"])[v["index"]] for n, v in variants.items()}
    assert len(bad["md_disagrees_long"]["md"]) > 3 * wave_step > row_max
    c = U.counters(bad["md_disagrees_long"]["cigar"])
    m4 = U.md_host(bad["md_disagrees_long"]["md"])
    assert m4[0] + m4[1] == c["diff"] + 1
    for n in ("hardclip_deep", "decline_and_hardclip"):
        ops = [o for _, o in bad[n]["cigar"]]
        h = [i for i, o in enumerate(ops) if o == "H" and 0 < i < len(ops) - 1]
        j = next(i for i, o in enumerate(ops) if o in "MIS=X")
        assert len(h) == 1 and D.between_ends(bad[n]) > D.LANE_SCAN and h[0] > j
        if n == "hardclip_deep":
            assert h[0] - j > 64 and j + D.between_ends(bad[n]) - h[0] > 64
    assert U.md_model(bad["decline_and_hardclip"]["md"])[1] == U.MD_UNUSUAL and D.situation(bad["decline_and_hardclip"]) == "MD_refines"
    assert bad["starts_with_D"]["cigar"][1][1] == "D" and bad["ends_in_D"]["cigar"][-3][1] == "D"


def test_md_model_equals_the_oracle_on_every_generated_and_every_random_string(oracle, deep):
    _, _, mapped = deep
    strs = [r["md"] for r in mapped if r["md"] is not None]
    for v in D.panic_variants(SHAPE).values():
        strs.append(D.mapped_of(v["recs"])[v["index"]]["md"])
    rand = D.random_md_strings(SHAPE)
    top = 2 * SHAPE[1] + 64
    assert len(rand) == D.N_RANDOM and min(map(len, rand)) == 0 and max(map(len, rand)) == top and all(0 not in s for s in rand)
    assert rand == D.random_md_strings(SHAPE)  # seeded
    assert sum(1 for s in rand if len(s) > SHAPE[1]) > 150 and any(s and s[0] >= 0x80 for s in rand)
    seen = set().union(*map(set, rand))
    assert seen >= set(b"0123456789ACGTZ^acgt/:@[]_`") and any(b >= 0x80 for b in seen)
    n_unusual = 0
    for s in strs + rand:
        if s is None:
            continue
        counts, status = U.md_model(s)
        got = _oracle_md(oracle, s)
        assert U.md_host(s) == got, s[:80]
        if status == U.MD_OK:
            assert counts == got
        else:
            n_unusual += 1
            assert counts == (0, 0, 0, 0) and status == U.MD_UNUSUAL
    assert 20 < n_unusual < len(rand) // 2  # both kinds are well represented
    # the packings keep every string whole and put it where they say
    for phase in (None, 0, 7, 15):
        text, off, end = D.pack_strings(rand, phase)
        assert all(text[int(o):int(e)] == s for s, o, e in zip(rand, off, end))
        assert all(int(o) % 16 == phase for o in off) if phase is not None else len(text) == sum(map(len, rand))


def test_md_extents_in_the_sam_text_and_the_line_layouts(deep):
    refs, recs, mapped = deep
    sam, off, end = D.sam_with_md_extents(refs, recs)
    assert sam == U.sam_text(refs, recs) and len(off) == len(mapped)
    for r, o, e in zip(mapped, off, end):
        o, e = int(o), int(e)
        if r["md"] is None:
            assert (o, e) == (0, 0)
        else:
            assert sam[o:e] == r["md"] and sam[o - 6:o] == b"\tMD:Z:" and sam[e:e + 1] in b"\t\n"
    assert len({int(o) % 16 for o in off if o}) == 16  # an MD string sits at every phase
    assert int(end[-1]) == len(sam) - 1
    for place in ("first", "middle", "last", "cycle"):
        text = D.layout_sam(refs, recs, place)
        lines = [ln.split(b"\t") for ln in text.split(b"\n")[1 + len(refs):-1]]
        assert len(lines) == len(recs)
        for i, (r, f) in enumerate(zip(recs, lines)):
            at = [k for k, x in enumerate(f[11:]) if x.startswith(b"MD:Z:")]
            assert f[0].decode() == r["name"] and f[5].decode() == (_cg(r) or "*")
            assert at == ([] if r["md"] is None else [{"first": 0, "middle": 2, "last": 3}[place if place != "cycle" else ("first", "middle", "last")[i % 3]]])
            assert r["md"] is None or f[11 + at[0]][5:] == r["md"]
    two = D.layout_sam(refs, recs, "cycle", second_md=True)
    for r, ln in zip(recs, two.split(b"\n")[1 + len(refs):-1]):
        mds = [x for x in ln.split(b"\t")[11:] if x.startswith(b"MD:Z:")]
        assert len(mds) == (0 if r["md"] is None else 2) and (not mds or (mds[0][5:] == r["md"] != mds[1][5:]))
    bare = D.layout_sam(refs, recs, "last", last="nothing")
    assert bare.endswith(mapped[-1]["md"]) and D.layout_sam(refs, recs, "last") == bare + b"\n" and D.layout_sam(refs, recs, last="empty").endswith(b"\n\n")


def test_bgzf_writer(deep):
    """blocks of irregular sizes that hop from header to header, inflate to the data and end in the 28-byte end-of-file block"""
    refs, recs, _ = deep
    data = U.bam_bytes(refs, recs)
    raw = U.bgzf_bytes(data, D.BGZF_SIZES)
    assert gzip.decompress(raw) == data and len(raw) < len(data)
    at, sizes = 0, []
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 10:at + 16] == b"\x06\x00BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", raw, at + bsize - 4)[0])
        at += bsize
    assert at == len(raw) and sizes[-1] == 0 and raw[-28:] == U.bgzf_bytes(b"") and sum(sizes) == len(data)
    assert sizes[:len(D.BGZF_SIZES)] == list(D.BGZF_SIZES) and len(sizes) > 2 * len(D.BGZF_SIZES) and 1 in sizes and max(sizes) == 0xFF00
