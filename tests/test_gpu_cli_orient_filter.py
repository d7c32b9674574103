"""`rb orient [--scaffold --insert I]` and `rb filter [-p L] [-a A] [-q Q]` at the file level: stdout and the exit status must be, byte for
byte, the ORACLE's (oracle.cli; never the code under test) on every route -- the device text route from a file and from stdin
(rb_host_pairs_text) and the record route (RB_GENERAL_PATH=1)."""
import subprocess

import pytest

import pairs_rec_util as pr
from test_gpu_cli_chain import RB, rb_run

pytestmark = pytest.mark.gpu
ENTRY = b"rb_host_pairs_text"


def check_all_routes(oracle, args, paf_path, rc_want=0):
    """`rb <args> paf` on the three routes against the oracle -> (stdout, the runs)"""
    rc, want = oracle.cli(*args, paf_path)
    text = open(paf_path, "rb").read()
    runs = {"file": rb_run(*args, paf_path, env={"RB_TIMING": "1"}), "stdin -": rb_run(*args, "-", env={"RB_TIMING": "1"}, stdin=text),
            "stdin": rb_run(*args, env={"RB_TIMING": "1"}, stdin=text), "record route": rb_run(*args, paf_path, env={"RB_GENERAL_PATH": "1", "RB_TIMING": "1"})}
    for how, r in runs.items():
        assert r.returncode == (101 if rc else 0) == rc_want, (how, args, rc, r.stderr[-300:])
        assert r.stdout == want, (how, args, len(r.stdout), len(want), r.stderr[-300:])
    return want, runs


ASM = [("orient",), ("orient", "--scaffold"), ("orient", "-s", "-i", "0"), ("orient", "--scaffold", "--insert", "500"), ("filter",), ("filter", "--paired-len", "1000000"),
       ("filter", "-p", "1000000", "-a", "5000", "-q", "100"), ("filter", "--aln", "20000"), ("filter", "--query", "60000000")]


@pytest.mark.parametrize("args", ASM, ids=[" ".join(a) for a in ASM])
def test_asm_small(oracle, golden, args):
    want, runs = check_all_routes(oracle, args, f"{golden}/asm_small.paf")
    n = open(f"{golden}/asm_small.paf", "rb").read().count(b"\n")
    if args[0] == "orient":
        assert want.count(b"\n") == n
    elif len(args) > 1:
        assert 0 < want.count(b"\n") < n, "the filter drops some records and keeps others"
    for how in ("file", "stdin -"):
        assert ENTRY in runs[how].stderr and b"assemble lines" in runs[how].stderr, (how, runs[how].stderr)
        assert (b"scaffold: sort" in runs[how].stderr) == ("--scaffold" in args or "-s" in args)
    assert ENTRY not in runs["record route"].stderr


_orient, _filter = pr.orient_text_cases(), pr.filter_text_cases()


@pytest.mark.parametrize("c", _orient, ids=[c.name for c in _orient])
@pytest.mark.parametrize("sep", ["\t", " "], ids=["tabs", "spaces"])
def test_hand_made_orient(oracle, tmp_path, c, sep):
    """a flipped and an unflipped pair, a sum of 0, two queries of equal order whose runs interleave (tests/test_pairs_rec_inputs.py), extra tags in
    front of and behind cg:Z:"""
    paf = tmp_path / "in.paf"
    paf.write_bytes(pr.paf_text(c, sep=sep, tags=("tp:A:P", "NM:i:3")))
    m = pr.model(c)
    want, runs = check_all_routes(oracle, ("orient",), str(paf))
    assert want == pr.lines_of(c, m)
    want, runs = check_all_routes(oracle, ("orient", "--scaffold", "--insert", c.insert), str(paf))
    assert want == pr.lines_of(c, m, scaffold=True) and b"qc+::qd+::qa+\t" in want
    assert ENTRY in runs["file"].stderr and ENTRY in runs["stdin"].stderr and ENTRY not in runs["record route"].stderr


@pytest.mark.parametrize("c", _filter, ids=[c.name for c in _filter])
def test_hand_made_filter(oracle, tmp_path, c):
    paf = tmp_path / "in.paf"
    paf.write_bytes(pr.paf_text(c))
    want, runs = check_all_routes(oracle, ("filter", *pr.filter_flags(c)), str(paf))
    assert want == pr.lines_of(c, pr.model(c))
    assert ENTRY in runs["file"].stderr and ENTRY in runs["stdin"].stderr and ENTRY not in runs["record route"].stderr


@pytest.mark.parametrize("args", [("orient",), ("orient", "--scaffold"), ("filter", "--paired-len", "100")], ids=" ".join)
def test_a_line_with_a_non_numeric_column(oracle, tmp_path, args):
    c = pr.orient_text_cases()[0]
    lines = pr.paf_text(c).splitlines(True)
    bad = lines[3].split(b"\t")
    bad[2] = b"x7"
    paf = tmp_path / "skip.paf"
    paf.write_bytes(b"".join(lines[:5] + [b"\t".join(bad)] + lines[5:]))
    want, runs = check_all_routes(oracle, args, str(paf))
    assert want.count(b"\n") > 0
    for how, r in runs.items():
        assert r.stderr.count(b"Unable to parse PAF record. Skipping line 6") == 1, (how, r.stderr)
    assert ENTRY in runs["file"].stderr


@pytest.mark.parametrize("args", [("orient",), ("orient", "--scaffold"), ("filter",)], ids=" ".join)
def test_an_empty_file(oracle, tmp_path, args):
    empty = tmp_path / "empty.paf"
    empty.write_bytes(b"")
    want, runs = check_all_routes(oracle, args, str(empty))
    assert want == b"" and ENTRY in runs["file"].stderr


GOOD = "qa 100 0 10 + T 1000 0 10 0 0 60 cg:Z:10=\n"
FROM_FILE_PANICS = {"integrity": GOOD + "qb 100 0 10 + T 1000 20 31 0 0 60 cg:Z:10=\n", "cigar": GOOD + "qb 100 0 10 + T 1000 20 30 0 0 60 cg:Z:10=3\n",
                    "cigar before integrity": "qb 100 0 10 + T 1000 20 31 0 0 60 cg:Z:10=\n" + "qb 100 0 10 + T 1000 20 30 0 0 60 cg:Z:1x0=\n"}


@pytest.mark.parametrize("args", [("orient",), ("filter",)], ids=" ".join)
@pytest.mark.parametrize("name", list(FROM_FILE_PANICS))
def test_panics_of_from_file(oracle, tmp_path, name, args):
    """a CIGAR that disagrees with its coordinates, a malformed one, and both: 101, nothing printed, on every route"""
    paf = tmp_path / "panic.paf"
    paf.write_text(FROM_FILE_PANICS[name].replace(" ", "\t"))
    want, runs = check_all_routes(oracle, args, str(paf), rc_want=101)
    assert want == b"" and all(r.stderr.count(b"thread 'main' panicked") == 1 for r in runs.values())


@pytest.mark.parametrize("args", [("orient",), ("orient", "--scaffold"), ("filter",)], ids=" ".join)
def test_a_pair_of_span_zero(oracle, tmp_path, args):
    """orient's divide by zero (the device declines, the record route panics as the reference does); the filter's defaults drop the record"""
    zero = tmp_path / "zero.paf"
    zero.write_text((GOOD + "qi 100 0 5 + T 1000 50 50 0 0 60 cg:Z:5I\n").replace(" ", "\t"))
    if args[0] == "orient":
        want, runs = check_all_routes(oracle, args, str(zero), rc_want=101)
        assert want == b"" and all(b"divide by zero" in r.stderr for r in runs.values()) and ENTRY in runs["file"].stderr
    else:
        want, runs = check_all_routes(oracle, args, str(zero))
        assert want.count(b"\n") == 1


def test_a_flipped_record_that_ends_behind_its_query_length(oracle, tmp_path):
    """q_len < q_en under a flipped pair: the device declines, the record route prints the wrapped coordinates as the oracle does"""
    paf = tmp_path / "wrap.paf"
    paf.write_text("QW 10 0 20 - T 100 0 20 0 0 60 cg:Z:20=\nQW 10 2 6 + T 100 30 34 0 0 60 cg:Z:4=\nQK 50 0 9 - T 100 50 59 0 0 60 cg:Z:9=\n".replace(" ", "\t"))
    want, runs = check_all_routes(oracle, ("orient",), str(paf))
    assert b"QW-\t10\t18446744073709551606\t10\t+" in want
    assert all(ENTRY in runs[how].stderr for how in ("file", "stdin -")), "the device route ran, declined, and the record route printed"


def test_which_route_runs(golden):
    """with RB_TIMING=1 the file and the stdin runs name the entry point and its device laps, the RB_GENERAL_PATH=1 run does not"""
    paf = f"{golden}/asm_small.paf"
    text = open(paf, "rb").read()
    for args in (["orient"], ["orient", "--scaffold"], ["filter", "--paired-len", "1000000"]):
        for r in (rb_run(*args, paf, env={"RB_TIMING": "1"}), rb_run(*args, "-", env={"RB_TIMING": "1"}, stdin=text), rb_run(*args, env={"RB_TIMING": "1"}, stdin=text)):
            assert r.returncode == 0 and ENTRY in r.stderr and b"pair keys" in r.stderr and b"pairs records" in r.stderr and b"format cigars" in r.stderr, r.stderr
        r = rb_run(*args, paf, env={"RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
        assert r.returncode == 0 and ENTRY not in r.stderr and b"pairs records" not in r.stderr, r.stderr


def test_refused_combinations_stay_refused(golden):
    paf, bed = f"{golden}/asm_small.paf", f"{golden}/asm_small.bed"
    for a in (["--gpus", "2", "orient", paf], ["--gpus", "2", "filter", "-p", "5", paf], ["--gpus", "2", "orient", "--scaffold", paf],
              ["orient", "--paired-len", "5", paf], ["liftover", "--bed", bed, "--aln", "5", paf], ["break-paf", "--orient", "--scaffold", paf],
              ["liftover", "--bed", bed, "--orient", paf], ["break-paf", "--scaffold", paf]):
        r = rb_run(*a)
        assert r.returncode == 2 and r.stdout == b"", (a, r.stderr)


def test_inside_a_real_pipe(oracle, golden):
    """the README's recipe between break-paf and stats, as processes joined by pipes, against the oracle's commands run one behind the other"""
    paf = f"{golden}/asm_small.paf"
    rc, out = oracle.cli("break-paf", "--max-size", 100, paf)
    for st in (("orient",), ("filter", "--paired-len", 100000), ("stats", "--paf")):
        rc2, out = oracle.cli(*st, "-", stdin=out)
        rc = rc or rc2
    assert rc == 0 and out.count(b"\n") > 100
    cmd = f"{RB} break-paf --max-size 100 {paf} | {RB} orient | {RB} filter --paired-len 100000 | {RB} stats --paf"
    r = subprocess.run(["bash", "-o", "pipefail", "-c", cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == out, (r.returncode, len(r.stdout), len(out), r.stderr[-300:])
