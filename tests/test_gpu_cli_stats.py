"""`rb liftover --stats` / `rb break-paf --stats` (and --stats-qbed) at the file level: stdout and the return code must be those of the
pipeline `rb <cmd> ... | rb stats --paf [--qbed] -` -- here the ORACLE's pipeline: oracle.cli(cmd ...) piped into oracle.cli("stats",
"--paf", "-").  The return code is the first command's.  Every route prints the same bytes: the whole-file text route (a file, stdin) and
the record route (RB_GENERAL_PATH=1)."""
import hashlib
import json
import os
import subprocess

import pytest

from golden.make_digests import tile_bed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
FLAGS = {"--stats": [], "--stats-qbed": ["--qbed"]}
HEADERS = {"--stats": b"#reference_name\t", "--stats-qbed": b"#query_name\t"}


def rb_run(*args, env=None, stdin=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    return subprocess.run([RB, *map(str, args)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=None if env is None else {**os.environ, **env})


def pipeline(oracle, cmd, flag):
    """(return code, stdout) of `oracle cmd | oracle stats --paf [--qbed] -`, and the first command's own stdout"""
    rc, paf = oracle.cli(*cmd)
    rc2, out = oracle.cli("stats", "--paf", *FLAGS[flag], "-", stdin=paf)
    assert rc2 == 0
    return rc, out, paf


def check_all_routes(oracle, cmd, paf_path, flag, min_lines=1):
    """cmd (without the PAF path) + flag on the file, on the file by the record route, and on stdin"""
    rc, want, plain = pipeline(oracle, [*cmd, paf_path], flag)
    assert rc == 0 and want.startswith(HEADERS[flag]) and want.count(b"\n") == 1 + plain.count(b"\n") and plain.count(b"\n") >= min_lines
    for what, r in (("text route", rb_run(*cmd, flag, paf_path)), ("record route", rb_run(*cmd, flag, paf_path, env={"RB_GENERAL_PATH": "1"})),
                    ("stdin", rb_run(*cmd, flag, stdin=open(paf_path, "rb").read()))):
        assert r.returncode == rc, (what, cmd, flag, r.stderr[-300:])
        assert r.stdout == want, (what, cmd, flag, len(r.stdout), len(want))
    return want, plain


@pytest.fixture(scope="module")
def beds(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("stats_beds")
    tile = str(d / "tile.bed")
    tile_bed(tile)
    recs = [l.split("\t") for l in open(f"{golden}/asm_small.paf")]
    whole = d / "whole.bed"  # a window [0, t_len) per target: every record lies inside its window and keeps its own (empty) id
    whole.write_text("".join(f"{t}\t0\t{n}\n" for t, n in dict((f[5], f[6]) for f in recs).items()))
    q = d / "q.bed"          # windows in QUERY coordinates that do hit: a stretch of every fifth record's query span
    q.write_text("".join(f"{f[0]}\t{int(f[2]) + 100}\t{min(int(f[3]), int(f[2]) + 30000)}\n" for f in recs[::5]))
    return {"asm_small": f"{golden}/asm_small.bed", "tile": tile, "whole": str(whole), "q": str(q)}


@pytest.mark.parametrize("flag", list(FLAGS))
@pytest.mark.parametrize("bed", ["asm_small", "tile", "whole"])
def test_liftover_stats(oracle, golden, beds, bed, flag):
    want, plain = check_all_routes(oracle, ["liftover", "--bed", beds[bed]], f"{golden}/asm_small.paf", flag, min_lines=5)
    if bed == "whole":
        assert b"\tid:Z:\t" in plain  # (rows that are inside their window: RB_HIT_INSIDE, the whole record's CIGAR)


@pytest.mark.parametrize("flag", list(FLAGS))
def test_liftover_qbed_stats(oracle, golden, beds, flag):
    check_all_routes(oracle, ["liftover", "--qbed", "--bed", beds["q"]], f"{golden}/asm_small.paf", flag, min_lines=5)


@pytest.mark.parametrize("flag", list(FLAGS))
@pytest.mark.parametrize("max_size", [100, 7])
def test_break_paf_stats(oracle, golden, max_size, flag):
    check_all_routes(oracle, ["break-paf", "--max-size", max_size], f"{golden}/asm_small.paf", flag, min_lines=50)


def test_legacy_policy_and_short_flags(oracle, golden, beds):
    paf = f"{golden}/asm_small.paf"
    rc, want, _ = pipeline(oracle, ["--bsearch", "legacy", "break-paf", "--max-size", "100", paf], "--stats")
    r = rb_run("--bsearch", "legacy", "break-paf", "-m", "100", "--stats", paf)
    assert (r.returncode, r.stdout) == (rc, want)
    rc, want, _ = pipeline(oracle, ["liftover", "--qbed", "--bed", beds["q"], paf], "--stats-qbed")
    r = rb_run("lo", "-q", "-b", beds["q"], "--stats-qbed", paf)
    assert (r.returncode, r.stdout) == (rc, want)


def test_m_cigar_warns_once(oracle, tmp_path):
    paf = tmp_path / "m.paf"
    paf.write_text("Q1 100 0 21 + T 100 0 22 0 0 60 cg:Z:5M2I3M3D9=2X\nQ2 100 5 17 - T 100 30 42 0 0 60 cg:Z:4=3M5=\nQ3 100 0 9 + T 100 50 59 0 0 60 cg:Z:9=\n".replace(" ", "\t"))
    bed = tmp_path / "m.bed"
    bed.write_text("T\t2\t20\nT\t31\t40\nT\t45\t70\n")
    for cmd in (["liftover", "--bed", bed], ["break-paf", "--max-size", "2"]):
        for flag in FLAGS:
            rc, want, plain = pipeline(oracle, [*cmd, paf], flag)
            assert rc == 0 and plain.count(b"\n") >= 3
            for env in (None, {"RB_GENERAL_PATH": "1"}):
                r = rb_run(*cmd, flag, paf, env=env)
                assert (r.returncode, r.stdout) == (rc, want), (cmd, flag, env)
                assert r.stderr.count(b"cigar string contains 'M'") == 1, r.stderr
    only_eq = tmp_path / "eq.paf"
    only_eq.write_text("Q3 100 0 9 + T 100 50 59 0 0 60 cg:Z:9=\n".replace(" ", "\t"))
    assert b"contains 'M'" not in rb_run("liftover", "--bed", bed, "--stats", only_eq).stderr


PANICS = {
    # the window's edge is not among the aligned positions of the record: RB_ST_PANIC_NOTFOUND (liftover.rs:31)
    "notfound": "Q 100 0 15 + T 100 0 10 0 0 60 cg:Z:5S10=\n",
    # target span 6 != 5 reference bases: check_integrity().unwrap() (paf.rs:70)
    "integrity": "Q 10 0 5 + T 10 0 5 0 0 60 cg:Z:5=\nQ 10 0 5 + T 10 0 6 0 0 60 cg:Z:5=\n",
}


@pytest.mark.parametrize("case,cmd", [("notfound", "liftover"), ("integrity", "liftover"), ("integrity", "break-paf")])
def test_where_the_plain_command_panics(oracle, tmp_path, case, cmd):
    """stdout is the second command's header alone, the exit status 101 and stderr what the plain command says"""
    bed = tmp_path / "r.bed"
    bed.write_text("T\t0\t5\n")
    paf = tmp_path / f"{case}.paf"
    paf.write_text(PANICS[case].replace(" ", "\t"))
    cmd = ["liftover", "--bed", bed] if cmd == "liftover" else ["break-paf"]
    for env in (None, {"RB_GENERAL_PATH": "1"}):
        said = rb_run(*cmd, paf, env=env)
        assert said.returncode == 101 and said.stdout == b""
        for flag in FLAGS:
            rc, want, plain = pipeline(oracle, [*cmd, paf], flag)
            assert rc == 101 and plain == b"" and want.count(b"\n") == 1 and want.startswith(HEADERS[flag])
            r = rb_run(*cmd, flag, paf, env=env)
            assert (r.returncode, r.stdout) == (101, want), (case, cmd, flag, env, r.stdout, r.stderr)
            assert r.stderr == said.stderr and b"panicked" in r.stderr


def test_refused_combinations(golden):
    paf, bed = f"{golden}/asm_small.paf", f"{golden}/asm_small.bed"
    for a in (["--gpus", "2", "liftover", "--bed", bed, "--stats", paf], ["--gpus", "2", "break-paf", "--stats-qbed", paf],
              ["liftover", "--largest", "--bed", bed, "--stats", paf], ["liftover", "-l", "--bed", bed, "--stats-qbed", paf]):
        r = rb_run(*a)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.count(b"\n") == 1 and b"--stats" in r.stderr, (a, r.stderr)


def test_without_the_flags_nothing_changes(golden, beds):
    """the plain commands print the bytes they printed before the flags existed (digests recorded in tests/golden)"""
    dig = json.load(open(os.path.join(golden, "digests.json")))
    paf = f"{golden}/asm_small.paf"
    for key, a in (("liftover_asm_small_bed", ["liftover", "--bed", beds["asm_small"], paf]), ("liftover_tile_100kb", ["liftover", "--bed", beds["tile"], paf]),
                   ("break_paf_100_modern", ["break-paf", "--max-size", "100", paf]), ("break_paf_100_legacy", ["--bsearch", "legacy", "break-paf", "--max-size", "100", paf])):
        r = rb_run(*a)
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == dig[key]["md5"], key
