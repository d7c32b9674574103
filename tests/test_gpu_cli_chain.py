"""`rb liftover --bed W --break N [--stats | --stats-qbed]` at the file level: stdout must be, byte for byte, what the pipeline
`rb break-paf --max-size N in.paf | rb liftover --bed W - [| rb stats --paf [--qbed] -]` prints -- here the ORACLE's pipeline: oracle.cli
("break-paf" ...) piped into oracle.cli("liftover", "--bed", W, "-") piped into oracle.cli("stats", "--paf", "-"); never the code under
test.  The exit status is 101 if either of the first two commands panics.  Every route prints the same bytes: the whole-file text route
(a file, stdin) and the record route (RB_GENERAL_PATH=1)."""
import hashlib
import json
import os
import subprocess

import pytest

from golden.make_digests import tile_bed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
FLAGS = {"plain": None, "--stats": [], "--stats-qbed": ["--qbed"]}
HEADERS = {"--stats": b"#reference_name\t", "--stats-qbed": b"#query_name\t"}
# final records of the oracle's pipeline on asm_small.paf, and how many of them lie inside their window (`id:Z:` with nothing behind it)
COUNTS = {(100, "asm_small"): (806, 785), (7, "asm_small"): (2935, 2914), (0, "asm_small"): (15771, 15750), (1000, "asm_small"): (195, 177),
          (100, "tile"): (3833, 1878), (7, "tile"): (9208, 6547), (0, "tile"): (48320, 45551), (1000, "tile"): (1949, 334)}


def rb_run(*args, env=None, stdin=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    return subprocess.run([RB, *map(str, args)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=None if env is None else {**os.environ, **env})


_oracle_cache = {}
_last_runs = {}  # the three runs of the last check_all_routes (a test that also looks at stderr)


def pipeline(oracle, paf_path, n, bed, flag, pre=()):
    """(exit status, stdout) of the oracle's pipeline, and the stdout of its first two commands; every stage computed once per input"""
    k1 = (paf_path, n, pre)
    if k1 not in _oracle_cache:
        _oracle_cache[k1] = oracle.cli(*pre, "break-paf", "--max-size", n, paf_path)
    rc1, pieces = _oracle_cache[k1]
    k2 = k1 + (bed,)
    if k2 not in _oracle_cache:
        _oracle_cache[k2] = oracle.cli(*pre, "liftover", "--bed", bed, "-", stdin=pieces)
    rc2, lifted = _oracle_cache[k2]
    out = lifted
    if FLAGS[flag] is not None:
        rc3, out = oracle.cli("stats", "--paf", *FLAGS[flag], "-", stdin=lifted)
        assert rc3 == 0
    return (101 if rc1 or rc2 else 0), out, pieces, lifted


def chain_args(n, bed, flag):
    return ["liftover", "--bed", bed, "--break", n] + ([] if flag == "plain" else [flag])


def check_all_routes(oracle, paf_path, n, bed, flag, pre=()):
    rc, want, pieces, lifted = pipeline(oracle, paf_path, n, bed, flag, pre)
    a = [*pre, *chain_args(n, bed, flag)]
    runs = {"text route": rb_run(*a, paf_path), "record route": rb_run(*a, paf_path, env={"RB_GENERAL_PATH": "1"}), "stdin": rb_run(*a, stdin=open(paf_path, "rb").read())}
    for what, r in runs.items():
        assert r.returncode == rc, (what, a, r.stderr[-300:])
        assert r.stdout == want, (what, a, len(r.stdout), len(want))
    _last_runs.clear()
    _last_runs.update(runs)
    return rc, want, pieces, lifted


@pytest.fixture(scope="module")
def beds(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_beds")
    tile = str(d / "tile.bed")
    tile_bed(tile)
    recs = [l.split("\t") for l in open(f"{golden}/asm_small.paf")]
    whole = d / "whole.bed"  # a window [0, t_len) per target: every piece lies inside its window and keeps its own (empty) id
    whole.write_text("".join(f"{t}\t0\t{n}\n" for t, n in dict((f[5], f[6]) for f in recs).items()))
    return {"asm_small": f"{golden}/asm_small.bed", "tile": tile, "whole": str(whole)}


@pytest.mark.parametrize("flag", list(FLAGS))
@pytest.mark.parametrize("bed", ["asm_small", "tile", "whole"])
@pytest.mark.parametrize("n", [100, 7, 0])
def test_chain_on_asm_small(oracle, golden, beds, n, bed, flag):
    rc, want, pieces, lifted = check_all_routes(oracle, f"{golden}/asm_small.paf", n, beds[bed], flag)
    assert rc == 0
    if flag != "plain":
        assert want.startswith(HEADERS[flag]) and want.count(b"\n") == 1 + lifted.count(b"\n")
    if (n, bed) in COUNTS:  # both branches -- clipped at a window's edge, inside the window -- are well populated
        assert (lifted.count(b"\n"), lifted.count(b"\tid:Z:\tcg:Z:")) == COUNTS[(n, bed)]
    if bed == "whole":
        assert lifted.count(b"\n") == pieces.count(b"\n") == lifted.count(b"\tid:Z:\tcg:Z:")


def test_the_device_pipeline_is_what_runs(golden, beds):
    """a file and stdin take the whole-file text route (rb_host_break_liftover_text / _stats_text: no decline on minimap2-style input),
    RB_GENERAL_PATH=1 the record route (the host batch of the re-read pieces is packed)"""
    paf = f"{golden}/asm_small.paf"
    for flag, fn in (("plain", b"rb_host_break_liftover_text"), ("--stats", b"rb_host_break_liftover_stats_text")):
        a = chain_args(100, beds["tile"], flag)
        for r in (rb_run(*a, paf, env={"RB_TIMING": "1"}), rb_run(*a, env={"RB_TIMING": "1"}, stdin=open(paf, "rb").read())):
            assert r.returncode == 0 and fn in r.stderr and b"pack batch" not in r.stderr, r.stderr
            assert (b"assemble lines" in r.stderr) == (flag == "plain")
        r = rb_run(*a, paf, env={"RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
        assert r.returncode == 0 and fn not in r.stderr and b"pack batch" in r.stderr, r.stderr


def test_counts_at_1000(oracle, golden, beds):
    for bed in ("asm_small", "tile"):
        rc, want, pieces, lifted = pipeline(oracle, f"{golden}/asm_small.paf", 1000, beds[bed], "plain")
        assert (rc, lifted.count(b"\n"), lifted.count(b"\tid:Z:\tcg:Z:")) == (0, *COUNTS[(1000, bed)])
        r = rb_run(*chain_args(1000, beds[bed], "plain"), f"{golden}/asm_small.paf")
        assert (r.returncode, r.stdout) == (0, want)


def test_legacy_policy_and_short_flags(oracle, golden, beds):
    """--bsearch legacy applies to both stages; `lo`, -b"""
    paf = f"{golden}/asm_small.paf"
    for flag in FLAGS:
        check_all_routes(oracle, paf, 100, beds["tile"], flag, pre=("--bsearch", "legacy"))
    rc, want, _, _ = pipeline(oracle, paf, 7, beds["asm_small"], "--stats-qbed")
    r = rb_run("lo", "-b", beds["asm_small"], "--stats-qbed", "--break", "7", paf)
    assert (r.returncode, r.stdout) == (rc, want)


HAND = """Q1 100 0 21 + T 100 0 22 0 0 60 cg:Z:5M2I3M3D9=2X
Q2 100 5 17 - T 100 30 42 0 0 60 cg:Z:4=3M5=
Q3 100 0 9 + T 100 50 59 0 0 60 cg:Z:9=
Q4 200 10 55 + T2 300 100 170 0 0 60 cg:Z:10=30D10=5I10=5X5=
Q5 200 60 90 - T2 300 180 216 0 0 60 cg:Z:12=6D6=2X10=
Q6 100 0 0 + T3 100 0 10 0 0 60 cg:Z:10N
Q7 100 0 8 + T4 100 0 8 0 0 60 cg:Z:8=
Q8 100 20 29 + T3 100 20 29 0 0 60 cg:Z:4=1X4=
"""
HAND_BED = "T\t2\t20\nT\t31\t40\nT\t45\t70\nT2\t0\t110\nT2\t110\t140\nT2\t140\t300\nT2\t186\t192\nT3\t0\t100\nT4\t0\t100\nT9\t0\t5\n"


def test_hand_made_paf(oracle, tmp_path):
    """an M-cigar (the stats warning, once); a `-` strand record; records whose long indel sits at a window's edge (Q4: the 30D is
    [110, 140) and a window is exactly that; Q5: the 6D is [192, 198), a window ends where it begins); several contigs; and contig order:
    Q6 (10N, on T3) turns into no piece at all -- every piece of it is None in the oracle's break-paf --, so among the PIECES T4 appears
    before T3 while among the records T3 comes first: the second command prints Q7 before Q8, a liftover of the input would not"""
    paf, bed = tmp_path / "hand.paf", tmp_path / "hand.bed"
    paf.write_text(HAND.replace(" ", "\t"))
    bed.write_text(HAND_BED)
    rc, _, pieces, _ = pipeline(oracle, str(paf), 2, str(bed), "plain")
    assert rc == 0 and b"Q6" not in pieces and pieces.index(b"Q7") < pieces.index(b"Q8")
    direct = oracle.cli("liftover", "--bed", bed, paf)[1]
    assert direct.index(b"Q8") < direct.index(b"Q7"), "among the records T3 comes first"
    for n in (2, 30):
        for flag in FLAGS:
            rc, want, pieces, lifted = check_all_routes(oracle, str(paf), n, str(bed), flag)
            assert rc == 0 and lifted.count(b"\n") >= 8
            if n == 2:
                assert lifted.index(b"Q7") < lifted.index(b"Q8"), "contigs in order of first appearance among the pieces"
            for what, r in _last_runs.items():
                assert r.stderr.count(b"cigar string contains 'M'") == (0 if flag == "plain" else 1), (what, flag, r.stderr)


PANICS = {
    # target span 6 != 5 reference bases: the first command's check_integrity().unwrap() (paf.rs:70): nothing reaches the second
    "integrity": ("Q 10 0 5 + T 10 0 5 0 0 60 cg:Z:5=\nQ 10 0 5 + T 10 0 6 0 0 60 cg:Z:5=\n", "break-paf"),
    # the second record's break_paf_on_indels does not find a piece's edge among its aligned positions: RB_ST_PANIC_NOTFOUND (liftover.rs:31) in
    # the first command, after it has printed the first record's pieces
    "notfound": ("Q 100 0 20 + T 100 0 26 0 0 60 cg:Z:10=6D10=\nQ 100 0 15 + T 100 0 10 0 0 60 cg:Z:5S10=\n", "break-paf"),
    # the second record is all indel: aligned_pairs panics (paf.rs:757) in the first command after it has printed the first record's pieces
    "part-way": ("Q 100 0 20 + T 100 0 26 0 0 60 cg:Z:10=6D10=\nQ 100 0 5 + T 100 50 50 0 0 60 cg:Z:5I\nQ 100 0 9 + T 100 60 69 0 0 60 cg:Z:9=\n", "break-paf"),
}


@pytest.mark.parametrize("case", list(PANICS))
def test_where_a_command_panics(oracle, tmp_path, case):
    """stdout and the exit status are the oracle pipeline's (what the second command makes of the pieces the first printed before it
    panicked is still printed); stderr is what the plain command that panicked says.  All three panic in the FIRST command: no input was
    found on which the oracle's break-paf succeeds and its liftover of the pieces panics (S, H, P, N ops inside a piece, a window edge
    inside each of them: the second command clips them all) -- a piece starts and ends on a match op and its edges are aligned positions"""
    bed = tmp_path / "r.bed"
    bed.write_text("T\t0\t5\nT\t8\t30\n")
    paf = tmp_path / f"{case}.paf"
    paf.write_text(PANICS[case][0].replace(" ", "\t"))
    for env in (None, {"RB_GENERAL_PATH": "1"}):
        said = rb_run(PANICS[case][1], "--max-size", 3, paf, env=env)
        assert said.returncode == 101 and b"panicked" in said.stderr
        for flag in FLAGS:
            rc, want, pieces, lifted = pipeline(oracle, str(paf), 3, str(bed), flag)
            assert rc == 101
            if case == "integrity":
                assert lifted == b""
            else:
                assert pieces.count(b"\n") == 2 and lifted.count(b"\n") == 3
            r = rb_run(*chain_args(3, bed, flag), paf, env=env)
            assert (r.returncode, r.stdout) == (101, want), (case, flag, env, r.stdout, r.stderr)
            assert r.stderr.endswith(said.stderr[said.stderr.index(b"thread 'main' panicked"):]), (case, flag, env, r.stderr, said.stderr)


def test_refused_combinations(golden):
    paf, bed = f"{golden}/asm_small.paf", f"{golden}/asm_small.bed"
    for a in (["liftover", "--bed", bed, "--break", "100", "--qbed", paf], ["liftover", "--bed", bed, "--break", "100", "--largest", paf],
              ["--gpus", "2", "liftover", "--bed", bed, "--break", "100", paf], ["break-paf", "--break", "100", paf],
              ["stats", "--paf", "--break", "100", paf], ["liftover", "-l", "-b", bed, "--break", "7", "--stats", paf]):
        r = rb_run(*a)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.count(b"\n") == 1, (a, r.stderr)
        assert b"--break" in r.stderr or b"--stats" in r.stderr, (a, r.stderr)


def test_without_the_flag_nothing_changes(golden, beds):
    """the plain commands print the bytes they printed before the flag existed (digests recorded in tests/golden)"""
    dig = json.load(open(os.path.join(golden, "digests.json")))
    paf = f"{golden}/asm_small.paf"
    for key, a in (("liftover_asm_small_bed", ["liftover", "--bed", beds["asm_small"], paf]), ("liftover_tile_100kb", ["liftover", "--bed", beds["tile"], paf]),
                   ("break_paf_100_modern", ["break-paf", "--max-size", "100", paf]), ("break_paf_100_legacy", ["--bsearch", "legacy", "break-paf", "--max-size", "100", paf])):
        r = rb_run(*a)
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == dig[key]["md5"], key
