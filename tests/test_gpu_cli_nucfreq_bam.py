"""`rb nucfreq` with the BAM decoded on the device (RB_NUCFREQ_DEV_DECODE=1: load_bam_reads_dev -- rb_dev_bam_records, rb_dev_bam_reads, then
rb_devreads_nucfreq[_text] on slices of the resident columns) against the host decode (RB_GENERAL_PATH=1) and the oracle CLI, byte for
byte, with equal exit codes.  RB_TIMING=1 makes the route name itself on stderr: the line is there on the first run and not on the second."""
import gzip
import random
import re
import struct

import pytest

import bam_rec_util as B
import bam_reads_util as R
import sam_util as U
from test_gpu_cli import RB, rb_run, _write_bam  # noqa: F401  (the front end's runner and the minimal BAM writer)

pytestmark = pytest.mark.gpu
ROUTE = b"[rb timing] nucfreq_bam: rb_dev_bam_records, rb_dev_bam_reads"
RANGES = re.compile(rb"nucfreq_bam: (\d+) ranges of the stream back to back, (\d+) records, (\d+) bytes")
FORMS = {"small": (["-s"], {}), "full_text": ([], {"RB_NUCFREQ_TEXT": "1"}), "full_host_formatter": ([], {})}


def _panic(stderr):
    return [l for l in stderr.splitlines() if b"panicked" in l]


def three(oracle, args, env=None, want_rc=0, route=True, host_is_the_reference=False):
    """`rb nucfreq args` with the device decode, with RB_GENERAL_PATH=1, and the oracle: -> (the device run, the output all three agree on).
    host_is_the_reference: a broken file, which the oracle's reader does not refuse as the host decode (htslib's rules) does: the bytes,
    the exit code and the panic are the host decode's"""
    e = dict(env or {})
    new = rb_run("nucfreq", *args, env={**e, "RB_TIMING": "1", "RB_NUCFREQ_DEV_DECODE": "1"})
    if new.returncode < 0 or new.returncode in (134, 139) or b"illegal memory access" in new.stderr:  # nothing more is started on a card that faulted
        pytest.exit(f"rb nucfreq {args} ended with {new.returncode}: {new.stderr[-400:]!r}", returncode=3)
    old = rb_run("nucfreq", *args, env={**e, "RB_TIMING": "1", "RB_NUCFREQ_DEV_DECODE": "1", "RB_GENERAL_PATH": "1"})
    orc, oout = (old.returncode, old.stdout) if host_is_the_reference else oracle.cli("nucfreq", *args)
    assert (new.returncode, old.returncode, orc) == (want_rc, want_rc, want_rc), (args, new.stderr[-400:])
    assert new.stdout == oout, args
    assert old.stdout == oout, args
    assert (ROUTE in new.stderr) == route and new.stderr.count(ROUTE) <= 1 and ROUTE not in old.stderr, (args, new.stderr[-400:])
    assert _panic(new.stderr) == _panic(old.stderr) and (len(_panic(new.stderr)) == 1) == (want_rc != 0)
    return new, oout


@pytest.fixture(scope="module")
def asm_recs(golden):
    """(contig, start, end) of the alignments of asm_small.bam"""
    r = rb_run("stats", f"{golden}/asm_small.bam")
    assert r.returncode == 0
    return [(f[0].decode(), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in r.stdout.splitlines()[1:])]


@pytest.mark.parametrize("no_bai", [False, True])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_golden_files_regions_and_interleaved_beds(oracle, golden, tmp_path, asm_recs, form, no_bai):
    """--region, and --bed of 240 regions on interleaved contigs, with the index and without (in this file the regions' members touch: one
    range at the most; test_three_index_ranges_back_to_back has several)"""
    extra, env = FORMS[form]
    env = {**env, **({"RB_NO_BAI": "1"} if no_bai else {})}
    name, r_st, _ = asm_recs[0]
    new, out = three(oracle, ["--region", f"{name}:{r_st + 10001}-{r_st + 12050}"] + extra + [f"{golden}/asm_small.bam"], env=env)
    assert out.count(b"\n") > 2000
    rnd = random.Random(5)
    lines = []
    for k in range(240):
        name, r_st, r_en = asm_recs[rnd.randrange(len(asm_recs))] if k % 7 else asm_recs[k % 3]
        a = rnd.randrange(max(r_st - 2000, 0), r_en + 2000)
        lines.append(f"{name}\t{a}\t{a + (0 if k % 41 == 0 else rnd.randrange(1, 3000))}" + (f"\tid{k}" if k % 3 == 0 else ""))
    assert len({l.split("\t")[0] for l in lines}) >= 2 and [l.split("\t")[0] for l in lines] != sorted(l.split("\t")[0] for l in lines)
    bed = tmp_path / "many.bed"
    bed.write_text("\n".join(lines) + "\n")
    new, out = three(oracle, ["--bed", str(bed)] + extra + [f"{golden}/asm_small.bam"], env=env)
    assert out.count(b"\n") > 1000
    new, out = three(oracle, ["-r", "CHROMOSOME_I:2-102"] + extra + [f"{golden}/test_nucfreq.bam"], env=env)
    assert out.count(b"\n") == 102
    bed.write_text("CHROMOSOME_I\t0\t50\tfirst\nCHROMOSOME_I\t20\t80\nCHROMOSOME_I\t500\t900\n")
    three(oracle, ["-b", str(bed)] + extra + [f"{golden}/test_nucfreq.bam"], env=env)


@pytest.fixture(scope="module")
def islands(tmp_path_factory):
    """bam_reads_util.three_islands as BGZF in members of 512 bytes with its .bai, and a twin whose index ends inside a record of the FIRST
    island that runs on into the next member"""
    d = tmp_path_factory.mktemp("islands")
    refs, recs, bed = R.three_islands()
    raw, bai, start = R.bgzf_and_bai(refs, recs)
    cut = next(r for r in range(10, 30) if (start[r] + 10) // 512 < (start[r + 1] - 1) // 512)
    (d / "islands.bam").write_bytes(raw)
    (d / "islands.bam.bai").write_bytes(bai)
    (d / "cut.bam").write_bytes(raw)
    (d / "cut.bam.bai").write_bytes(R.bgzf_and_bai(refs, recs, cut_in=cut)[1])
    (d / "r.bed").write_text(bed)
    return dict(bam=str(d / "islands.bam"), cut_bam=str(d / "cut.bam"), bed=str(d / "r.bed"), cut=cut, n=len(recs))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_three_index_ranges_back_to_back(oracle, islands, form):
    """three disjoint ranges of members in the one device buffer: the second and third at a base above 0, rounded up to 16 bytes, their records
    placed by `base - a` with a > 0; the route says how many ranges and records it took"""
    extra, env = FORMS[form]
    new, out = three(oracle, ["--bed", islands["bed"]] + extra + [islands["bam"]], env=env)
    m = RANGES.search(new.stderr)
    assert m and (int(m.group(1)), int(m.group(2))) == (3, 90), new.stderr[-400:]
    assert int(m.group(3)) % 16 == 0 and sum(1 for l in out.splitlines() if not l.startswith(b"#")) == 3 * 126 + 10
    whole, out2 = three(oracle, ["--bed", islands["bed"]] + extra + [islands["bam"]], env={**env, "RB_NO_BAI": "1"})
    m = RANGES.search(whole.stderr)
    assert m and (int(m.group(1)), int(m.group(2))) == (1, islands["n"]) and out2 == out


def test_a_range_that_ends_inside_a_record_and_is_not_the_last(oracle, islands):
    """the index ends inside a record of the first range: bam_next's panic there, the later ranges are not looked at"""
    new, out = three(oracle, ["--bed", islands["bed"], "-s", islands["cut_bam"]], want_rc=101, host_is_the_reference=True)
    m = RANGES.search(new.stderr)
    assert b"truncated BAM file (inside a record)" in new.stderr and out == b""
    assert m and (int(m.group(1)), int(m.group(2))) == (1, islands["cut"]), new.stderr[-400:]


def _synthetic():
    refs = [("chrA", 50000), ("chrB", 30000)]
    recs = [
        dict(name="r1", ref=0, pos=100, flag=0, l_seq=50, cigar=[(5, "S"), (20, "M"), (3, "I"), (4, "D"), (22, "M")]),
        dict(name="r2_longer_name", ref=0, pos=110, flag=16, l_seq=30, cigar=[(2, "H"), (10, "="), (1, "X"), (100, "N"), (19, "M"), (3, "H")]),
        dict(name="dup", ref=0, pos=115, flag=1024, l_seq=10, cigar=[(10, "M")]),
        dict(name="sec", ref=0, pos=118, flag=256, l_seq=10, cigar=[(10, "M")]),
        dict(name="qcfail", ref=0, pos=119, flag=512, l_seq=10, cigar=[(10, "M")]),
        dict(name="r3", ref=0, pos=4090, flag=0, l_seq=21, cigar=[(21, "M")]),
        dict(name="r4", ref=1, pos=0, flag=16, l_seq=12, cigar=[(12, "M")]),
    ]
    real = [(10, "M"), (2, "I"), (6, "D"), (28, "M")]  # htslib's long-cigar convention: <l_seq>S<ref_len>N in the record, the real cigar in CG:B,I
    cg = b"CGBI" + struct.pack("<i", len(real)) + b"".join(struct.pack("<I", (l << 4) | "MIDNSHP=X".index(c)) for l, c in real)
    recs.append(dict(name="long_cigar_in_CG", ref=1, pos=100, flag=0, l_seq=40, cigar=[(40, "S"), (44, "N")], aux=cg))
    recs.append(dict(name="un", ref=-1, pos=-1, flag=4, l_seq=5, cigar=[]))
    return refs, recs


@pytest.mark.parametrize("form", sorted(FORMS))
def test_synthetic_file_in_a_plain_gzip_container(oracle, tmp_path, form):
    """soft clips, deletions, reverse strands, filtered flags and one long-CIGAR record; one gzip member, no BGZF blocks, no index"""
    extra, env = FORMS[form]
    p = tmp_path / "s.bam"
    _write_bam(str(p), *_synthetic())
    assert p.read_bytes()[3] & 4 == 0  # (no extra field: not BGZF)
    lines = {}
    for a in ("chrA:1-50000", "chrA:105-125", "chrB:1-4294967295", "chrA:4097-4100", "chrB:90-160"):
        new, out = three(oracle, ["-r", a] + extra + [str(p)], env=env)
        lines[a] = sum(1 for l in out.splitlines() if not l.startswith(b"#"))
    assert lines["chrA:1-50000"] == 140 + 21  # r1 and r2 merge; r3; the filtered reads add nothing
    assert lines["chrB:90-160"] == 44         # the CG tag's cigar, not <l_seq>S<ref_len>N


def test_timing_laps_of_the_route(oracle, golden):
    new, _ = three(oracle, ["-r", "CHROMOSOME_I:2-102", "-s", f"{golden}/test_nucfreq.bam"])
    for lap in (b"read + inflate", b"record hop", b"H2D stream + record places", b"decode + columns D2H"):
        assert new.stderr.count(lap) == 1, lap
    assert new.stderr.index(b"decode + columns D2H") < new.stderr.index(ROUTE)


def test_unsorted_file_panics_the_same(oracle, tmp_path):
    refs, recs = _synthetic()
    recs[0], recs[5] = recs[5], recs[0]
    p = tmp_path / "u.bam"
    _write_bam(str(p), refs, recs)
    assert oracle.cli("nucfreq", "-r", "chrA:1-5000", str(p))[0] == 101
    new, out = three(oracle, ["-r", "chrA:1-5000", str(p)], want_rc=101, host_is_the_reference=True)
    assert b"not coordinate sorted" in new.stderr


@pytest.mark.parametrize("cut", ["inside_a_record", "inside_a_block_size", "behind_the_last_record"])
def test_a_file_that_ends_early(oracle, tmp_path, cut):
    refs, recs = _synthetic()
    data = U.bam_bytes(refs, [dict(r, md=None) for r in recs if "aux" not in r])
    _, off, ln = B.hop(data)
    at = {"inside_a_record": int(off[4]) + 37, "inside_a_block_size": int(off[4]) - 2, "behind_the_last_record": len(data)}[cut]
    p = tmp_path / "cut.bam"
    with gzip.open(p, "wb", compresslevel=1) as f:
        f.write(data[:at])
    rc = 0 if cut == "behind_the_last_record" else 101
    new, out = three(oracle, ["-r", "chrA:1-5000", "-s", str(p)], want_rc=rc, host_is_the_reference=rc != 0)
    said = {"inside_a_record": b"truncated BAM file (inside a record)", "inside_a_block_size": b"truncated BAM file (inside a block_size field)"}
    assert (said[cut] in new.stderr) if rc else len(out) > 100


def test_a_record_the_device_refuses_takes_the_host_decode(oracle, tmp_path):
    """a name that is not NUL-terminated: the decline -- the host decode's bytes and message, and no route line"""
    bodies = [B.body(name=b"ok\0", pos=100, words=[B.w(30, "M")], l_seq=30), B.body(name=b"abc", pos=120, words=[B.w(3, "M")], l_seq=3),
              B.body(name=b"ok\0", pos=130, words=[B.w(30, "M")], l_seq=30)]
    p = tmp_path / "bad_name.bam"
    with gzip.open(p, "wb", compresslevel=1) as f:
        f.write(B.stream(bodies)[0])
    new, out = three(oracle, ["-r", "chrA:1-5000", str(p)], want_rc=101, route=False, host_is_the_reference=True)
    assert out == b"" and b"read name is not NUL-terminated" in new.stderr and b"rb_dev_bam" not in new.stderr


def test_unknown_contig_after_printed_regions(oracle, golden, tmp_path):
    """exit 101, and the regions in front of the unknown contig are printed"""
    bed = tmp_path / "r.bed"
    bed.write_text("CHROMOSOME_I\t0\t50\tfirst\nCHROMOSOME_I\t20\t80\nnope\t0\t10\nCHROMOSOME_I\t0\t50\n")
    for form in sorted(FORMS):
        extra, env = FORMS[form]
        new, out = three(oracle, ["-b", str(bed)] + extra + [f"{golden}/test_nucfreq.bam"], env=env, want_rc=101)
        assert len(out) > 50 and b"Is this region (nope:1-10) in your reference/bam?" in new.stderr


def test_the_route_is_opt_in(oracle, golden):
    """without RB_NUCFREQ_DEV_DECODE the host decodes (profiles/nucfreq_bam_summary.md: one of the eight measured lines misses the pass mark)"""
    a = ["-r", "CHROMOSOME_I:2-102", "-s", f"{golden}/test_nucfreq.bam"]
    r = rb_run("nucfreq", *a, env={"RB_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == oracle.cli("nucfreq", *a)[1] and ROUTE not in r.stderr
