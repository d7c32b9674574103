"""`rb break-paf --max-size N [--orient] [--paired-len L --aln A --query Q] [--stats | --stats-qbed]` at the file level: stdout must be, byte
for byte, what the pipeline `rb break-paf --max-size N in.paf [| rb orient -] [| rb filter .. -] [| rb stats --paf [--qbed] -]` prints -- here
the ORACLE's pipeline, oracle.cli piped into oracle.cli; never the code under test.  The exit status is 101 if a command in front of stats
panics.  Every route prints the same bytes: the whole-file text route (a file, stdin) and the record route (RB_GENERAL_PATH=1)."""
import hashlib
import json
import os

import pytest

from test_gpu_cli_chain import FLAGS, HEADERS, PANICS, rb_run

pytestmark = pytest.mark.gpu
# pieces, flipped rows under orient, rows kept at --paired-len 1000000 of the oracle's pipeline on asm_small.paf, by --max-size
COUNTS = {100: (2447, 978, 1944), 1000: (553, 172, 525), 5000: (280, 144, 269), 0: (46935, 7576, 43915)}

_oracle_cache = {}
_last_runs = {}


def stages(what, filt):
    """what: "orient", "filter" or "both"; filt: dict of the filter's long flags -> (oracle stages, rb's flags)"""
    st, flags = [], []
    if what in ("orient", "both"):
        st.append(("orient",))
        flags.append("--orient")
    if what in ("filter", "both"):
        f = [x for k, v in filt.items() for x in (k, v)]
        st.append(("filter", *f))
        flags += f
    return st, flags


def pipeline(oracle, paf_path, n, what, filt, flag, pre=()):
    """(exit status, stdout) of the oracle's pipeline and the stdout of every stage in front of stats; every stage computed once per input"""
    key = (paf_path, n, pre)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.cli(*pre, "break-paf", "--max-size", n, paf_path)
    rc, out = _oracle_cache[key]
    outs = [out]
    for st in stages(what, filt)[0]:
        key = key + (tuple(map(str, st)),)
        if key not in _oracle_cache:
            _oracle_cache[key] = oracle.cli(*st, "-", stdin=out)
        rc2, out = _oracle_cache[key]
        rc = rc or rc2
        outs.append(out)
    if FLAGS[flag] is not None:
        rc3, stats = oracle.cli("stats", "--paf", *FLAGS[flag], "-", stdin=out)
        if rc3:
            # stats' own Paf::from_file panics on what reached it.  main.rs:51 prints the header before it reads anything; the oracle's CLI reads
            # first and so prints nothing at all.  What the pipeline prints then is what the plain `rb stats --paf -` (code the options do not
            # touch) prints on the same input: the header, and status 101
            r = rb_run("stats", "--paf", *FLAGS[flag], "-", stdin=out)
            assert (rc3, stats, r.returncode, r.stdout.count(b"\n")) == (101, b"", 101, 1) and r.stdout.startswith(HEADERS[flag])
            rc, stats = 101, r.stdout
        out = stats
    return (101 if rc else 0), out, outs


def rb_args(n, what, filt, flag, cmd="break-paf"):
    return [cmd, "--max-size", n, *stages(what, filt)[1]] + ([] if flag == "plain" else [flag])


def check_all_routes(oracle, paf_path, n, what, filt, flag, pre=(), cmd="break-paf"):
    rc, want, outs = pipeline(oracle, paf_path, n, what, filt, flag, pre)
    a = [*pre, *rb_args(n, what, filt, flag, cmd)]
    runs = {"text route": rb_run(*a, paf_path), "record route": rb_run(*a, paf_path, env={"RB_GENERAL_PATH": "1"}), "stdin": rb_run(*a, stdin=open(paf_path, "rb").read())}
    for how, r in runs.items():
        assert r.returncode == rc, (how, a, r.stderr[-300:])
        assert r.stdout == want, (how, a, len(r.stdout), len(want), r.stderr[-300:])
    _last_runs.clear()
    _last_runs.update(runs)
    return rc, want, outs


L0, L1M = {"--paired-len": 0}, {"--paired-len": 1000000}
ASM = [(100, w, f, flag) for flag in FLAGS for w, f in (("orient", {}), ("filter", L0), ("filter", L1M), ("both", L0), ("both", L1M))]
ASM += [(5000, "both", L1M, flag) for flag in FLAGS] + [(5000, "orient", {}, "plain"), (5000, "filter", L0, "--stats")]
ASM += [(0, "both", L1M, "--stats"), (0, "both", L1M, "plain")]


@pytest.mark.parametrize("n,what,filt,flag", ASM, ids=[f"{n}-{w}-{f.get('--paired-len', '')}-{flag}" for n, w, f, flag in ASM])
def test_pairs_on_asm_small(oracle, golden, n, what, filt, flag):
    rc, want, outs = check_all_routes(oracle, f"{golden}/asm_small.paf", n, what, filt, flag)
    assert rc == 0
    pieces, last = outs[0], outs[-1]
    assert pieces.count(b"\n") == COUNTS[n][0]
    if flag != "plain":
        assert want.startswith(HEADERS[flag]) and want.count(b"\n") == 1 + last.count(b"\n")
    # the population, from the oracle alone: 9 pairs, 5 of them flipped; L = 1000000 drops some pairs and keeps others, L = 0 drops nothing
    if what != "filter":
        names = [ln.split(b"\t")[0] for ln in outs[1].splitlines()]
        assert len(names) == COUNTS[n][0] and sum(x.endswith(b"-") for x in names) == COUNTS[n][1]
        pairs = {(t[5], t[0]) for t in (ln.split(b"\t") for ln in outs[1].splitlines())}
        assert len(pairs) == 9 and sum(q.endswith(b"-") for _, q in pairs) == 5
    if what != "orient":
        assert last.count(b"\n") == (COUNTS[n][2] if filt["--paired-len"] else COUNTS[n][0])
    assert last.count(b"\tid:Z:\tcg:Z:") == last.count(b"\n"), "every printed line has an empty id"


def test_counts_at_1000(oracle, golden):
    rc, want, outs = pipeline(oracle, f"{golden}/asm_small.paf", 1000, "both", L1M, "plain")
    names = [ln.split(b"\t")[0] for ln in outs[1].splitlines()]
    assert (rc, len(names), sum(x.endswith(b"-") for x in names), outs[2].count(b"\n")) == (0, *COUNTS[1000])
    r = rb_run(*rb_args(1000, "both", L1M, "plain"), f"{golden}/asm_small.paf")
    assert (r.returncode, r.stdout) == (0, want)


def test_the_device_pipeline_is_what_runs(golden):
    """a file and stdin take the whole-file text route (rb_host_break_pairs_text / _stats_text: no decline on minimap2-style input),
    RB_GENERAL_PATH=1 the record route (the host batch is packed); the pipelined chunk route is not taken"""
    paf = f"{golden}/asm_small.paf"
    for flag, fn in (("plain", b"rb_host_break_pairs_text"), ("--stats", b"rb_host_break_pairs_stats_text")):
        a = rb_args(100, "both", L1M, flag)
        for r in (rb_run(*a, paf, env={"RB_TIMING": "1"}), rb_run(*a, env={"RB_TIMING": "1"}, stdin=open(paf, "rb").read())):
            assert r.returncode == 0 and fn in r.stderr and b"pairs rows" in r.stderr and b"pack batch" not in r.stderr, r.stderr
            assert (b"assemble lines" in r.stderr) == (flag == "plain") and b"pipelined" not in r.stderr
        r = rb_run(*a, paf, env={"RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
        assert r.returncode == 0 and fn not in r.stderr and b"pairs rows" not in r.stderr and b"record route: pieces re-read" in r.stderr, r.stderr


def hand_paf():
    """dozens of pairs on four targets, one to three records each, both strands, D ops of 0, 3, 6 and 9 bases (--max-size 2 cuts them)"""
    lines = []
    for i in range(36):
        for j in range(1 + i % 3):
            a, d, b = 5 + i, (i % 4) * 3, 7
            cg = f"{a}={d}D{b}=" if d else f"{a + b}="
            q_st, t_st = 10 + 40 * j, 1000 * i + 100 * j
            lines.append(f"q{i} 500 {q_st} {q_st + a + b} {'+' if (i + j) % 3 else '-'} t{i % 4} 100000 {t_st} {t_st + a + d + b} 0 0 60 cg:Z:{cg}")
    lines += [
        # pieces on both strands whose sum is exactly 0: not flipped
        "QZ 200 0 20 + T 1000 0 20 0 0 60 cg:Z:20=", "QZ 200 30 50 - T 1000 30 50 0 0 60 cg:Z:20=",
        # the records say + (50 against 30 query bases); the 30I is cut out by break-paf and the pieces say - (10 + 10 against 30)
        "QF 200 0 50 + T 1000 100 120 0 0 60 cg:Z:10=30I10=", "QF 200 60 90 - T 1000 130 160 0 0 60 cg:Z:30=",
        # T1: QB's 20 bases go at --paired-len 100, QA's 1000 stay
        "QA 2000 0 1000 + T1 5000 0 1000 0 0 60 cg:Z:1000=", "QB 200 0 20 + T1 5000 2000 2020 0 0 60 cg:Z:20=",
        "QM 100 0 21 + T2 100 0 22 0 0 60 cg:Z:5M2I3M3D9=2X",   # an M-cigar
        "Q6 100 0 0 + T3 100 0 10 0 0 60 cg:Z:10N",             # leaves no piece
        # the strict edges of --aln 20 and --query 100
        "QE 100 0 20 + T4 1000 0 20 0 0 60 cg:Z:20=", "QE1 101 0 21 + T4 1000 30 51 0 0 60 cg:Z:21=",
    ]
    return "".join(ln.replace(" ", "\t") + "\n" for ln in lines)


HAND_FILTERS = [("orient", {}), ("filter", {"--paired-len": 100}), ("filter", {"--aln": 20}), ("filter", {"--query": 100}), ("filter", {}),
                ("both", {"--paired-len": 20, "--aln": 20, "--query": 100}), ("both", {"--paired-len": 100})]


@pytest.mark.parametrize("what,filt", HAND_FILTERS, ids=[w + "".join(f"{k}={v}" for k, v in f.items()) for w, f in HAND_FILTERS])
def test_hand_made_paf(oracle, tmp_path, what, filt):
    if what == "filter" and not filt:
        filt = {"--query": 0}  # (some filter flag has to be there for the stage to be there: its default)
    paf = tmp_path / "hand.paf"
    paf.write_text(hand_paf())
    for flag in FLAGS:
        rc, want, outs = check_all_routes(oracle, str(paf), 2, what, filt, flag)
        assert rc == 0
        pieces, last = outs[0], outs[-1]
        assert b"Q6" not in pieces and pieces.count(b"\n") > 100
        for how, r in _last_runs.items():
            assert r.stderr.count(b"cigar string contains 'M'") == (1 if flag != "plain" and b"QM" in last else 0), (how, flag, r.stderr)
    names = {ln.split(b"\t")[0] for ln in last.splitlines()}
    if what != "filter":
        o = {ln.split(b"\t")[0] for ln in outs[1].splitlines()}
        assert b"QZ+" in o and b"QZ-" not in o, "a sum of exactly 0 is not flipped"
        assert b"QF-" in o and b"QF+" not in o, "the pieces decide, not the records"
        assert b"QF+\t" in oracle.cli("orient", str(paf))[1], "the records alone say +"
        assert len(o) > 36 and 5 < sum(x.endswith(b"-") for x in o) < len(o) - 5
    sfx = b"+" if what == "both" else b""
    if filt.get("--paired-len") == 100:
        assert b"QA" + sfx in names and b"QB" + sfx not in names and b"T1" in {ln.split(b"\t")[5] for ln in last.splitlines()}
    if "--aln" in filt or "--query" in filt and filt["--query"]:
        assert b"QE1" + sfx in names and b"QE" + sfx not in names and b"QE" in pieces
    if filt == {"--query": 0}:
        assert last == pieces, "no record here has q_len 0: the filter's defaults keep everything"


@pytest.mark.parametrize("case", list(PANICS))
def test_where_the_first_command_panics(oracle, tmp_path, case):
    """stdout and the exit status are the oracle pipeline's (what the later commands make of the pieces the first printed before it panicked
    is still printed); stderr ends as the plain break-paf ends"""
    paf = tmp_path / f"{case}.paf"
    paf.write_text(PANICS[case][0].replace(" ", "\t"))
    for env in (None, {"RB_GENERAL_PATH": "1"}):
        said = rb_run("break-paf", "--max-size", 3, paf, env=env)
        assert said.returncode == 101 and b"panicked" in said.stderr
        for what, filt in (("orient", {}), ("both", {"--paired-len": 5})):
            for flag in FLAGS:
                rc, want, outs = pipeline(oracle, str(paf), 3, what, filt, flag)
                assert rc == 101
                assert outs[0].count(b"\n") == (0 if case == "integrity" else 2)
                r = rb_run(*rb_args(3, what, filt, flag), paf, env=env)
                assert (r.returncode, r.stdout) == (101, want), (case, what, flag, env, r.stdout, r.stderr)
                assert r.stderr.endswith(said.stderr[said.stderr.index(b"thread 'main' panicked"):]), (case, flag, env, r.stderr, said.stderr)


def test_a_flipped_record_that_ends_behind_its_query_length(oracle, tmp_path):
    """q_len < q_en under a flipped pair: the oracle's orient prints the wrapped start as a u64, and every command behind it panics on that
    record when it reads it (q_en < q_st).  The bytes are whatever the oracle pipeline prints, on every route -- with the one proviso of
    pipeline(): a stats stage that panics itself has printed its header"""
    paf = tmp_path / "wrap.paf"
    paf.write_text("QW 10 0 20 - T 100 0 20 0 0 60 cg:Z:20=\nQW 10 2 6 + T 100 30 34 0 0 60 cg:Z:4=\nQK 50 0 9 - T 100 50 59 0 0 60 cg:Z:9=\n".replace(" ", "\t"))
    for what, filt in (("orient", {}), ("both", {"--paired-len": 5})):
        for flag in FLAGS:
            rc, want, outs = check_all_routes(oracle, str(paf), 100, what, filt, flag)
            assert rc == (0 if (what, flag) == ("orient", "plain") else 101)
            assert b"QW-\t10\t18446744073709551606\t10\t+" in outs[1], "the wrapped start, as a u64"
            if what == "both":
                assert outs[2] == b"" and want == (b"" if flag == "plain" else want.splitlines(True)[0]), "the filter panics; stats prints its header over no input"


def test_refused_combinations(golden):
    paf, bed = f"{golden}/asm_small.paf", f"{golden}/asm_small.bed"
    for a in (["orient", "--orient", paf], ["liftover", "--bed", bed, "--orient", paf], ["stats", "--paf", "--orient", paf], ["trim-paf", "--orient", paf],
              ["liftover", "--bed", bed, "--paired-len", "5", paf], ["trim-paf", "--aln", "5", paf], ["invert", "--query", "5", paf],
              ["orient", "--paired-len", "5", paf], ["stats", "--paf", "--aln", "5", paf],
              ["break-paf", "--orient", "--scaffold", paf], ["break-paf", "--paired-len", "5", "--insert", "10", paf], ["break-paf", "--scaffold", paf],
              ["--gpus", "2", "break-paf", "--orient", paf], ["--gpus", "2", "break-paf", "--paired-len", "5", "--stats", paf], ["--gpus", "2", "bp", "--aln", "5", paf]):
        r = rb_run(*a)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.count(b"\n") == 1, (a, r.stderr)


def test_legacy_policy_and_aliases(oracle, golden):
    paf = f"{golden}/asm_small.paf"
    for flag in FLAGS:
        check_all_routes(oracle, paf, 100, "both", L1M, flag, pre=("--bsearch", "legacy"))
    legacy = pipeline(oracle, paf, 100, "both", L1M, "plain", pre=("--bsearch", "legacy"))[1]
    assert legacy != pipeline(oracle, paf, 100, "both", L1M, "plain")[1], "the two policies differ on this file"
    for cmd in ("bp", "breakpaf"):
        check_all_routes(oracle, paf, 5000, "both", L1M, "--stats", cmd=cmd)
    rc, want, _ = pipeline(oracle, paf, 5000, "orient", {}, "plain")
    r = rb_run("bp", "-m", "5000", "--orient", paf)
    assert (r.returncode, r.stdout) == (rc, want)


def test_without_the_options_nothing_changes(oracle, golden):
    """the plain commands print the bytes they printed before the options existed: digests recorded in tests/golden where there is one, the
    oracle's bytes otherwise"""
    dig = json.load(open(os.path.join(golden, "digests.json")))
    paf, bed = f"{golden}/asm_small.paf", f"{golden}/asm_small.bed"
    for key, a in (("liftover_asm_small_bed", ["liftover", "--bed", bed, paf]), ("break_paf_100_modern", ["break-paf", "--max-size", "100", paf]),
                   ("break_paf_100_legacy", ["--bsearch", "legacy", "break-paf", "--max-size", "100", paf])):
        r = rb_run(*a)
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == dig[key]["md5"], key
    for a in (["orient", paf], ["orient", "--scaffold", "--insert", "500", paf], ["filter", "--paired-len", "1000000", paf], ["filter", "-p", "1000000", "-a", "5000", "-q", "100", paf],
              ["break-paf", "--max-size", "100", "--stats", paf]):
        r, (rc, want) = rb_run(*a), (oracle.cli(*a) if "--stats" not in a else (0, oracle.cli("stats", "--paf", "-", stdin=oracle.cli(*a[:3], paf)[1])[1]))
        assert (r.returncode, r.stdout) == (rc, want), a
