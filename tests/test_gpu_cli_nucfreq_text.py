"""`rb nucfreq` on the device text route (rb_host_nucfreq_text: the lines printed on the device) against the oracle CLI, byte for byte.
RB_TIMING=1 makes the route name itself on stderr; RB_GENERAL_PATH=1 takes the host formatter and must print the same bytes.  --small
takes the text route by default, the full format with RB_NUCFREQ_TEXT=1 (profiles/nucfreq_text_summary.md): the tests set it for both."""
import random

import pytest

from test_gpu_cli import RB, rb_run, _write_bam  # noqa: F401  (the front end's runner and the minimal BAM writer)

pytestmark = pytest.mark.gpu
ROUTE = b"[rb timing] nucfreq_text:"


def both_routes(oracle, args, env=None, want_rc=0):
    """`rb nucfreq args` on the text route and on the host route, and the oracle: -> the output all three agree on"""
    e = dict(env or {})
    new = rb_run("nucfreq", *args, env={**e, "RB_TIMING": "1", "RB_NUCFREQ_TEXT": "1"})
    old = rb_run("nucfreq", *args, env={**e, "RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
    orc, oout = oracle.cli("nucfreq", *args)
    assert (new.returncode, old.returncode, orc) == (want_rc, want_rc, want_rc), (args, new.stderr[-400:])
    assert new.stdout == oout, args
    assert old.stdout == oout, args
    assert ROUTE not in old.stderr
    return new, oout


@pytest.fixture(scope="module")
def asm_recs(golden):
    """(contig, start, end) of the alignments of asm_small.bam"""
    r = rb_run("stats", f"{golden}/asm_small.bam")
    assert r.returncode == 0
    return [(f[0].decode(), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in r.stdout.splitlines()[1:])]


@pytest.mark.parametrize("small", [False, True])
def test_region_and_bed_with_ids_across_print_pieces(oracle, golden, tmp_path, asm_recs, small):
    """-r and --bed with ids, a region that crosses 1 Mbp print pieces with covered positions either side of the seam"""
    name, r_st, _ = asm_recs[0]
    bed = tmp_path / "r.bed"
    bed.write_text(f"{name}\t{r_st + 5000}\t{r_st + 5200}\tmy_id\n{name}\t{max(r_st - 300, 0)}\t{r_st + 300}\n{name}\t{r_st - 999500}\t{r_st + 1500}\tlong\n")
    a = ["--region", f"{name}:{r_st + 10001}-{r_st + 10050}", "--bed", str(bed)] + (["--small"] if small else []) + [f"{golden}/asm_small.bam"]
    new, out = both_routes(oracle, a)
    assert ROUTE in new.stderr
    if small:
        assert out.count(b"#") == 1 + 1 + 1 + 2 and out.count(b"\tlong\n") == 2
    else:
        assert out.count(b"#chr\tstart") == 1 + 1 + 1 + 2 and out.count(b"\tmy_id\n") == 200


@pytest.mark.parametrize("small", [False, True])
def test_ka13_fixture(oracle, golden, small):
    new, out = both_routes(oracle, ["-r", "CHROMOSOME_I:2-102"] + (["-s"] if small else []) + [f"{golden}/test_nucfreq.bam"])
    assert ROUTE in new.stderr and out.count(b"\n") == 102


@pytest.mark.parametrize("no_bai", [False, True])
def test_many_interleaved_regions(oracle, golden, tmp_path, asm_recs, no_bai):
    """240 small regions, contigs interleaved, some overlapping, some empty, every third with an id; with the index and without"""
    rnd = random.Random(3)
    lines = []
    for k in range(240):
        name, r_st, r_en = asm_recs[rnd.randrange(len(asm_recs))] if k % 7 else asm_recs[k % 3]
        a = rnd.randrange(max(r_st - 2000, 0), r_en + 2000)
        b = a + (0 if k % 41 == 0 else rnd.randrange(1, 3000))
        lines.append(f"{name}\t{a}\t{b}" + (f"\tid{k}" if k % 3 == 0 else ""))
    bed = tmp_path / "many.bed"
    bed.write_text("\n".join(lines) + "\n")
    for extra in ([], ["-s"]):
        new, out = both_routes(oracle, ["--bed", str(bed)] + extra + [f"{golden}/asm_small.bam"], env={"RB_NO_BAI": "1"} if no_bai else None)
        assert ROUTE in new.stderr and out.count(b"\n") > 1000


def _deep_bam(path):
    """300 reads of 60 bases staggered by one, then by three: depths of one, two and three digits"""
    refs = [("chrS", 5000), ("chrT", 900)]
    recs = [dict(name=f"r{i}", ref=0, pos=95 + (i if i < 150 else 150 + 3 * (i - 150)), flag=0, l_seq=60, cigar=[(60, "M")]) for i in range(300)]
    recs += [dict(name=f"t{i}", ref=1, pos=10 + i // 4, flag=16 if i % 2 else 0, l_seq=40, cigar=[(10, "S"), (30, "M")]) for i in range(500)]
    _write_bam(str(path), refs, recs)


@pytest.mark.parametrize("small", [False, True])
def test_synthetic_depth_two_and_three_digits(oracle, tmp_path, small):
    p = tmp_path / "deep.bam"
    _deep_bam(p)
    new, out = both_routes(oracle, ["-r", "chrS:1-5000"] + (["-s"] if small else []) + [str(p)])
    assert ROUTE in new.stderr
    body = [l for l in out.splitlines() if not l.startswith(b"#")]
    widths = {len(l.split(b"\t")[0 if small else 3]) for l in body}
    assert {1, 2} <= widths
    bed = tmp_path / "t.bed"
    bed.write_text("chrT\t0\t900\tdeep\nchrS\t100\t400\n")
    new, out = both_routes(oracle, ["--bed", str(bed)] + (["-s"] if small else []) + [str(p)])
    widths = {len(l.split(b"\t")[0 if small else 3]) for l in out.splitlines() if not l.startswith(b"#")}
    assert {1, 2, 3} <= widths


def test_unknown_contig_after_printed_regions(oracle, golden, tmp_path):
    """exit 101, and the regions in front of the unknown contig are printed"""
    bed = tmp_path / "r.bed"
    bed.write_text("CHROMOSOME_I\t0\t50\tfirst\nCHROMOSOME_I\t20\t80\nnope\t0\t10\nCHROMOSOME_I\t0\t50\n")
    for extra in ([], ["-s"]):
        new, out = both_routes(oracle, ["-b", str(bed)] + extra + [f"{golden}/test_nucfreq.bam"], want_rc=101)
        assert ROUTE in new.stderr and len(out) > 50
        assert b"Is this region (nope:1-10) in your reference/bam?" in new.stderr


def test_over_long_id_takes_the_host_formatter(oracle, golden, tmp_path):
    """TAB + id + LF of more than 255 bytes: the same bytes, from the host formatter"""
    bed = tmp_path / "r.bed"
    bed.write_text("CHROMOSOME_I\t0\t60\t" + "x" * 254 + "\n")
    new, out = both_routes(oracle, ["-b", str(bed), f"{golden}/test_nucfreq.bam"])
    assert ROUTE not in new.stderr and out.count(b"x" * 254) > 40
    bed.write_text("CHROMOSOME_I\t0\t60\t" + "x" * 253 + "\n")  # (255 bytes with TAB and LF: still the device's)
    new, out = both_routes(oracle, ["-b", str(bed), f"{golden}/test_nucfreq.bam"])
    assert ROUTE in new.stderr and out.count(b"x" * 253) > 40


def test_default_routes(oracle, golden):
    """without RB_NUCFREQ_TEXT: --small is printed on the device, the full format by the host formatter; the oracle's bytes either way"""
    for extra, on_device in ((["-s"], True), ([], False)):
        a = ["-r", "chr22:10024001-10027000"] + extra + [f"{golden}/asm_small.bam"]
        r = rb_run("nucfreq", *a, env={"RB_TIMING": "1"})
        orc, oout = oracle.cli("nucfreq", *a)
        assert (r.returncode, orc) == (0, 0) and r.stdout == oout and oout.count(b"\n") > 2000
        assert (ROUTE in r.stderr) == on_device
