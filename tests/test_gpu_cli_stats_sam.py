"""`rb stats [--qbed] <SAM>`: the reference reads "sam/bam/cram" through htslib (cli.rs:49-60).  The oracle reads BAM only, so the yardstick
for a SAM file is the oracle on the BAM twin of the same records (tests/sam_util.py; test_sam_inputs.py holds the twins and the models to
the oracle) -- never `rb` itself.  Every twin goes in as a file, on stdin, gzipped, and through the record route (RB_GENERAL_PATH=1); on
the default route the device must have left no record to the host but the designed ones."""
import gzip
import os
import re
import subprocess

import pytest

import sam_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
ROUTES = ["file", "stdin", "gz", "general"]


def rb_run(*args, env=None, stdin=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    return subprocess.run([RB, *map(str, args)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, **(env or {})})


def run_route(route, sam, tmp_path, qbed, name="in"):
    """-> (exit code, stdout, records left to the host / None on the record route, stderr)"""
    q = ["--qbed"] if qbed else []
    env = {"RB_TIMING": "1"}
    if route == "stdin":
        r = rb_run("stats", *q, "-", env=env, stdin=sam)
    else:
        path = tmp_path / (f"{name}.sam.gz" if route == "gz" else f"{name}.sam")
        if route == "gz":
            with gzip.open(path, "wb", compresslevel=1) as f:
                f.write(sam)
        else:
            path.write_bytes(sam)
        r = rb_run("stats", *q, path, env=dict(env, RB_GENERAL_PATH="1") if route == "general" else env)
    m = re.search(rb"stats_sam_text: records left to the host (\d+) of (\d+)", r.stderr)
    assert (b"stats_sam_text" in r.stderr) == (route != "general"), r.stderr[-400:]  # the timing output names the device entry point
    return r.returncode, r.stdout, (int(m.group(1)) if m else None), r.stderr


@pytest.fixture(scope="module")
def twins(oracle, golden, tmp_path_factory):
    """name -> (SAM text, {qbed: oracle's (exit code, stdout) on the BAM twin}, records the device leaves to the host by design)"""
    d = tmp_path_factory.mktemp("twins")
    out = {}
    for name in ("asm_small", "stats", "test"):
        bam = os.path.join(golden, name + ".bam")
        refs, recs = U.read_bam(bam)
        out[name] = (U.sam_text(refs, recs), {q: oracle.cli("stats", *(["--qbed"] if q else []), bam) for q in (False, True)}, 0)
    recs = U.span_cases()
    bam = d / "synthetic.bam"
    U.write_bam(bam, U.REFS, recs)
    out["synthetic"] = (U.sam_text(U.REFS, recs), {q: oracle.cli("stats", *(["--qbed"] if q else []), bam) for q in (False, True)}, 1)  # md_zero_padded
    return out


@pytest.mark.parametrize("qbed", [False, True])
def test_the_reference_sam_fixture(oracle, golden, qbed):
    q = ["--qbed"] if qbed else []
    r = rb_run("stats", *q, f"{golden}/test.sam")
    orc, oout = oracle.cli("stats", *q, f"{golden}/test_nucfreq.bam")
    assert (r.returncode, orc) == (0, 0) and r.stdout == oout and r.stdout.count(b"\n") == 3
    assert r.stderr.count("contains 'M'".encode()) == 2  # M without MD: the warning, once per record


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["asm_small", "stats", "test", "synthetic"])
def test_sam_twins_equal_the_oracle_on_the_bam(twins, tmp_path, name, route):
    sam, want, left_by_design = twins[name]
    for qbed in (False, True):
        rc, out, left, err = run_route(route, sam, tmp_path, qbed)
        assert (rc, out) == want[qbed] and rc == 0 and out.count(b"\n") > 5, (name, route, qbed, err[-300:])
        assert left == (None if route == "general" else left_by_design), (name, route, left)
    if name == "synthetic":
        assert b"\tunmapped\t" not in out and out.count(b"\n") == len(U.span_cases())  # header + every record but the unmapped one


@pytest.mark.parametrize("route", ["file", "general"])
@pytest.mark.parametrize("name", sorted(U.panic_cases()))
def test_a_panic_mid_file_leaves_the_lines_before_it(oracle, tmp_path, name, route):
    recs = U.span_cases()[:3] + [U.panic_cases()[name]] + U.span_cases()[3:6]
    bam = tmp_path / "twin.bam"
    U.write_bam(bam, U.REFS, recs)
    for qbed in (False, True):
        want = oracle.cli("stats", *(["--qbed"] if qbed else []), bam)
        rc, out, left, err = run_route(route, U.sam_text(U.REFS, recs), tmp_path, qbed)
        assert (rc, out) == want and rc == 101 and out.count(b"\n") == 1 + 3, (name, route, err[-300:])
        assert b"panicked" in err and left in (None, 0)


def _line(rec, **over):
    f = U.sam_line(U.REFS, rec).rstrip(b"\n").split(b"\t")
    for k, v in over.items():
        f[int(k[1:])] = v
    return b"\t".join(f) + b"\n"


@pytest.mark.parametrize("route", ["file", "general"])
def test_loud_refusals(tmp_path, route):
    """a mapped record the reference dies on (or htslib treats by version): exit 101 naming the line, after the lines before it"""
    good = U.span_cases()[:4]
    head = U.sam_text(U.REFS, good)
    ok = run_route(route, head, tmp_path, False)
    assert ok[0] == 0
    r = good[1]
    bad = {
        "rname_star": _line(r, c2=b"*"), "rname_unknown": _line(r, c2=b"chrZ"), "pos_0": _line(r, c3=b"0"), "pos_text": _line(r, c3=b"12x"),
        "flag_text": _line(r, c1=b"sixteen"), "ten_columns": b"\t".join(_line(r).split(b"\t")[:10]) + b"\n",
        "seq_length": _line(r, c9=b"N" * (r["l_seq"] + 1)), "long_cigar_tag": _line(r).rstrip(b"\n") + b"\tCG:B:I,10,20\n",
        "cigar_text": _line(r, c5=b"10=3Q"), "cigar_2^28": _line(r, c5=b"268435456=", c9=b"*"),
    }
    for name, line in bad.items():
        rc, out, left, err = run_route(route, head + line + U.sam_line(U.REFS, good[0]), tmp_path, False, name=name)
        assert rc == 101 and out == ok[1], (name, route, rc, err[-300:])
        assert b"line 8" in err, (name, err[-300:])  # 3 header lines, 4 records, then the bad one


def test_designed_declines_are_recomputed_on_the_host(oracle, tmp_path):
    """a CIGAR number and an MD number of ten or more digits are left to the host, those records alone, and are no panic"""
    recs = U.span_cases()[:5] + [U._rec("padded_md", "30M", md=b"000000000010A19")] + U.span_cases()[5:8]
    bam = tmp_path / "twin.bam"
    U.write_bam(bam, U.REFS, recs)
    sam = U.sam_text(U.REFS, recs).replace(b"\t20=2X3I10=2D8=4S\t", b"\t0000000020=2X3I10=2D8=4S\t", 1)
    assert sam != U.sam_text(U.REFS, recs)
    rc, out, left, err = run_route("file", sam, tmp_path, False)
    assert (rc, out) == oracle.cli("stats", bam) and rc == 0 and left == 2, err[-300:]
    assert run_route("general", sam, tmp_path, False)[:2] == (rc, out)


def test_gpus_cram_bam_on_stdin_and_text_that_is_no_sam(oracle, golden, tmp_path):
    sam = tmp_path / "x.sam"
    sam.write_bytes(open(f"{golden}/test.sam", "rb").read())
    assert rb_run("--gpus", 2, "stats", sam).returncode == 2  # as orient / filter: one GPU
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM\x03\x00" + bytes(64))
    r = rb_run("stats", cram)
    assert r.returncode == 101 and b"CRAM" in r.stderr
    # BAM on stdin is read once and still takes the BAM route
    r = rb_run("stats", "-", stdin=open(f"{golden}/test.bam", "rb").read(), env={"RB_TIMING": "1"})
    assert (r.returncode, r.stdout) == oracle.cli("stats", f"{golden}/test.bam") and b"stats_sam_text" not in r.stderr
    txt = tmp_path / "x.txt"
    txt.write_bytes(b"hello\tworld\n")
    r = rb_run("stats", txt)
    assert r.returncode == 101 and b"is not a BAM file" in r.stderr
