"""liftover --qbed on the device text route: RB_LIFT_QBED on rb_host_liftover_text / rb_host_liftover_largest_text against the oracle
(reduce on the batch as read; swap, normalize and liftover on the exchanged columns), and `rb liftover --qbed [--largest]` against the
oracle CLI, byte for byte, with the lap line of the text route as the witness.  What the inputs hold: tests/test_qbed_inputs.py."""
import os
import random
import subprocess

import numpy as np
import pytest

import largest_util as lu
import qbed_util as qu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
ROUTE = b"liftover --qbed (text to text)"
ROUTE_LARGEST = b"liftover --qbed --largest (text to text)"


# ---------------------------------------------------------------------------------------------- the wrappers
@pytest.fixture(scope="module")
def batch():
    return qu.qbed_batch()


@pytest.fixture(scope="module")
def refs(oracle, batch):
    return {p: qu.qbed_reference(oracle, batch, p) for p in (oracle.MODERN, oracle.LEGACY)}


def check_rows(got, ref):
    rows, orows = got["rows"], ref["rows"]
    assert len(rows) == len(orows)
    for k in ("rec", "win", "status"):
        assert np.array_equal(rows[k].astype(np.int64), orows[k].astype(np.int64)), k
    ok = orows["status"] == 0
    for k in ("t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len"):
        assert np.array_equal(rows[k][ok].astype(np.uint64), orows[k][ok].astype(np.uint64)), k
    assert np.array_equal((rows["flags"] & 1)[ok], (orows["flags"] & 1)[ok].astype(rows["flags"].dtype))
    assert got["text"] == ref["text"]


@pytest.mark.parametrize("policy", [0, 1])
def test_wrapper_equals_the_oracle(engine, batch, refs, policy):
    ref = refs[policy]
    got = qu.host_liftover_text(engine, batch, policy | qu.LIFT_QBED)
    assert got["rc"] == 0 and not got["cig_status"].any()
    check_rows(got, ref)
    # reduce rows: the records AS READ
    assert np.array_equal(got["red"]["status"], ref["red"]["status"])
    good = ref["red"]["status"] == 0
    for k in ("t_bases", "q_bases", "nmatch", "aln_len", "equal", "diff", "ins", "del", "matches", "ins_events", "del_events"):
        assert np.array_equal(got["red"][k][good], ref["red"][k][good]), k
    for k in ("both spans off", "target span off"):  # RB_ST_PANIC_INTEGRITY_T: the original record's check (the swapped record with only its
        assert int(got["red"]["status"][batch["special"][k]]) == 18  # target span off would say _Q)
    # norm rows: the swapped records
    assert np.array_equal(got["norm"]["status"], ref["norm"]["status"])
    good = ref["norm"]["status"] == 0
    for k in ("t_st", "t_en", "q_st", "q_en", "first_op", "n_ops", "lead_ops", "trail_ops", "nmatch", "aln_len"):
        assert np.array_equal(got["norm"][k][good], ref["norm"][k][good]), k
    stripped = (ref["norm"]["lead_ops"] + ref["norm"]["trail_ops"]) > 0
    assert np.array_equal((got["norm"]["flags"][good] & qu.F_STRIPPED) != 0, stripped[good])


def test_the_flag_does_something(engine, batch, refs):
    plain = qu.host_liftover_text(engine, batch, 0)
    assert plain["rc"] == 0
    ref = refs[0]["rows"]
    assert len(plain["rows"]) != len(ref) or not np.array_equal(plain["rows"]["t_st"].astype(np.uint64), ref["t_st"].astype(np.uint64))


def test_break_text_refuses_the_flag(engine, batch):
    r = qu.host_break_text(engine, batch, qu.LIFT_QBED)
    assert r["rc"] == qu.E_INVALID and "RB_LIFT_QBED" in r["error"]
    assert qu.host_break_text(engine, batch, 0)["rc"] == 0


def test_largest_wrapper_equals_the_reference_over_the_oracles_rows(engine, oracle, batch, refs):
    n_win = len(batch["w_st"])
    ids = [f"id{i % 7}" for i in range(n_win)]  # several windows share an id
    win_key, inside_key, n_keys = lu.intern_ids(ids)
    # as it stands the batch has a stripped record inside a window: declined, nothing selected
    r = qu.host_liftover_largest_text(engine, batch, qu.LIFT_QBED, win_key, n_keys, inside_key)
    assert (r["rc"], r["declined"], len(r["rows"])) == (0, 1, 0)
    keep = qu.windows_without_stripped_inside(batch, refs[0])
    e = qu.with_windows(batch, keep)
    ref = qu.qbed_reference(oracle, e)
    wk = win_key[keep]
    want_sel, want_bad = lu.largest_ref(ref["rows"], wk, np.full(len(e["strand"]), inside_key, np.uint32), n_keys)
    assert want_bad == 0 and len(want_sel) >= 5
    r = qu.host_liftover_largest_text(engine, e, qu.LIFT_QBED, wk, n_keys, inside_key)
    assert (r["rc"], r["declined"]) == (0, 0)
    sel = want_sel.astype(np.int64)
    check_rows(r, dict(rows=ref["rows"][sel], text=[ref["text"][k] for k in sel]))
    assert np.array_equal(r["red"]["status"], ref["red"]["status"]) and np.array_equal(r["norm"]["status"], ref["norm"]["status"])


# ---------------------------------------------------------------------------------------------- the front end
def rb_run(*args, env=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    return subprocess.run([RB, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, **(env or {})})


SMALL_PAF = ("q1\t100\t10\t30\t+\tt1\t200\t50\t72\t20\t22\t60\tcg:Z:10=2D10=\n"
             "q1\t100\t40\t50\t-\tt1\t200\t100\t113\t10\t13\t60\tcg:Z:10=3D\n"
             "q1\t100\t60\t76\t-\tt2\t200\t0\t13\t12\t15\t60\tcg:Z:5=3I4=1X3=\n"
             "q2\t100\t0\t10\t+\tt1\t200\t0\t13\t10\t13\t60\tcg:Z:10=3D\n")
SMALL_BED = "q1\t35\t60\tw_in\nq1\t12\t25\tw_a\nq1\t62\t70\tw_b\nq1\t65\t68\tw_indel\nq2\t0\t10\tw_edge\nq2\t5\t20\tw_tail\n"
FIFTH = "q2\t100\t20\t33\t+\tt1\t200\t20\t30\t10\t13\t60\tcg:Z:3I10=\n"  # swaps to a leading 3D: the reference panics at paf.rs:782


@pytest.fixture(scope="module")
def files(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("qbed")
    recs = [ln.split("\t") for ln in open(f"{golden}/asm_small.paf")]
    (d / "q.bed").write_text("".join(f"{f[0]}\t{int(f[2]) + 100}\t{min(int(f[3]), int(f[2]) + 30000)}\n" for f in recs[::5]))
    lines = open(f"{golden}/asm_small.paf").readlines()
    random.Random(7).shuffle(lines)
    (d / "shuffled.paf").write_text("".join(lines))
    (d / "small.paf").write_text(SMALL_PAF)
    (d / "small.bed").write_text(SMALL_BED)
    (d / "small5.paf").write_text(SMALL_PAF + FIFTH)
    return dict(fixture=(f"{golden}/asm_small.paf", str(d / "q.bed")), shuffled=(str(d / "shuffled.paf"), str(d / "q.bed")),
                small=(str(d / "small.paf"), str(d / "small.bed")), small5=(str(d / "small5.paf"), str(d / "small.bed")))


def check_cli(oracle, a, witness, expect_witness=True):
    orc, want = oracle.cli(*a)
    assert orc == 0
    r = rb_run(*a, env={"RB_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == want
    assert (witness in r.stderr) == expect_witness, r.stderr[-2000:]
    g = rb_run(*a, env={"RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
    assert g.returncode == 0 and g.stdout == r.stdout and witness not in g.stderr
    return want


@pytest.mark.parametrize("which", ["fixture", "shuffled", "small"])
def test_cli_qbed_text_route_equals_the_oracle(oracle, files, which):
    paf, bed = files[which]
    want = check_cli(oracle, ["liftover", "--qbed", "--bed", bed, paf], ROUTE)
    if which == "small":
        lines = want.split(b"\n")
        assert len(lines) == 7 and lines[1] == b"t1\t200\t100\t110\t-\tq1\t100\t40\t50\t10\t10\t60\tid:Z:_TO.3I.\tcg:Z:10="
    else:
        assert want.count(b"\n") == 126 and want.count(b"\t-\t") == 121
    if which == "fixture":
        assert len(want) > 1000


@pytest.mark.parametrize("which", ["fixture", "shuffled", "small"])
def test_cli_qbed_largest_text_route_equals_the_oracle(oracle, files, which):
    paf, bed = files[which]
    # the small file has a stripped record inside a window: the wrapper declines, the record route prints the oracle's bytes
    want = check_cli(oracle, ["liftover", "--qbed", "--largest", "--bed", bed, paf], ROUTE_LARGEST, expect_witness=which != "small")
    assert want.count(b"\n") == (6 if which == "small" else 50)
    if which == "fixture":
        assert len(want) > 1000


def test_cli_qbed_legacy_policy(oracle, files):
    paf, bed = files["fixture"]
    check_cli(oracle, ["--bsearch", "legacy", "liftover", "--qbed", "--bed", bed, paf], ROUTE)


def test_cli_qbed_a_swapped_leading_deletion_panics(oracle, files):
    paf, bed = files["small5"]
    a = ["liftover", "--qbed", "--bed", bed, paf]
    orc, want = oracle.cli(*a)
    assert (orc, want) == (101, b"")
    r = rb_run(*a, env={"RB_TIMING": "1"})
    assert (r.returncode, r.stdout) == (101, b"")
