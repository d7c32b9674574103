"""What the inputs of tests/test_gpu_swap_inplace.py and tests/test_gpu_qbed_text.py hold, proven with the oracle alone: a GPU test that
compares against the oracle on inputs without the hard cases would pass vacuously."""
import numpy as np
import pytest

import qbed_util as qu
from rbtest_util import CONT


@pytest.fixture(scope="module")
def recs():
    return qu.swap_records()


def test_swap_batch_has_every_length_on_both_strands(recs):
    for s in "+-":
        have = {len(w) for what, w, st in recs if st == ord(s) and what.startswith("plain")}
        assert have >= {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000, 4097}, s
        assert have >= {511, 512, 513, 1023, 1024, 1025}, s  # where rb_k_swap_inplace stops taking turns


def test_swap_batch_has_every_pair_placement_on_both_strands(recs):
    for s in "+-":
        by = {what[:-2]: w for what, w, st in recs if st == ord(s) and not what.startswith("plain")}
        assert set(by) == set(qu.PAIR_CASES)
        at = {k: np.nonzero((w & 15) == CONT)[0].tolist() for k, w in by.items()}   # where the continuation words lie
        n = {k: len(w) for k, w in by.items()}
        assert at["words 0-1"] == [1] and at["words n-2..n-1"] == [n["words n-2..n-1"] - 1]
        assert at["straddles 63|64"] == [64]
        k = "straddles the mirror of 63|64"
        assert [n[k] - 1 - p for p in at[k]] == [63]                       # reversed, the continuation word lands on 63 and its owner on 64
        assert at["middle, odd n, below"] == [4] and at["middle, odd n, above"] == [5] and n["middle, odd n, below"] == 9   # word 4 is the centre
        assert at["middle, even n"] == [5] and n["middle, even n"] == 10   # words 4 | 5 are the two centre words
        assert at["two pairs back to back"] == [4, 6]
        assert n["one pair is the record"] == 2 and at["one pair is the record"] == [1]
        for k, (a, b) in (("beside I and D", (1, 2)), ("beside D and I", (2, 1))):
            w, p = by[k], at[k][0]
            assert (int(w[p - 2]) & 15, int(w[p + 1]) & 15) == (a, b)
        for w in by.values():                                              # every continuation word has an owner in front of it
            c = np.nonzero((w & 15) == CONT)[0]
            assert (c > 0).all() and ((w[c - 1] & 15) != CONT).all()


def test_swap_batches_are_packed_between_guards(oracle):
    bs = qu.swap_batches()
    assert [len(s) for _, _, _, s in bs[1:]] == [1, 3, 4, 5] and len(bs[0][3]) == len(qu.swap_records())
    assert {int(off[0]) % 4 for _, _, off, _ in bs} == {0, 1, 2, 3}        # the first record at every phase of 16 bytes
    for what, arr, off, strand in bs:
        g = int(off[0])
        assert (arr[:g] == qu.GUARD).all() and (arr[int(off[-1]):] == qu.GUARD).all() and len(arr) > int(off[-1])
        assert not (arr[g:int(off[-1])] == qu.GUARD).any()
        want = qu.oracle_swap_whole(oracle, arr, off, strand)
        assert (want[:g] == qu.GUARD).all() and (want[int(off[-1]):] == qu.GUARD).all()
        assert not np.array_equal(want, arr)
        again = qu.oracle_swap_whole(oracle, want, off, strand)            # the swap is an involution
        assert np.array_equal(again, arr), what
    # on '-' the oracle keeps an owner in front of its continuation word
    what, arr, off, strand = bs[0]
    want = qu.oracle_swap_whole(oracle, arr, off, strand)
    c = np.nonzero((want & 15) == CONT)[0]
    assert len(c) > 40 and ((want[c - 1] & 15) != CONT).all()


@pytest.fixture(scope="module")
def qbed(oracle):
    d = qu.qbed_batch()
    return d, qu.qbed_reference(oracle, d)


def test_qbed_batch_shape(qbed):
    d, _ = qbed
    n = len(d["strand"])
    n_ops = np.diff(d["op_off"].astype(np.int64))
    assert 35 <= n <= 45 and 25 <= len(d["w_st"]) <= 40
    assert (n_ops > 2048).sum() == 2 and n_ops.min() == 1 and ((n_ops > 100) & (n_ops <= 300)).any()
    assert {chr(s) for s in d["strand"]} == {"+", "-"}
    assert d["q_names"][:6] == ["qA", "qB", "qC", "qA", "qB", "qC"] and set(d["contig"].tolist()) == {0, 1, 2}
    assert (d["w_contig"] == 3).sum() == 2                                 # windows on a name no record has


def test_qbed_batch_yields_every_kind_of_row(qbed, oracle):
    d, ref = qbed
    rows, norm = ref["rows"], ref["norm"]
    n_ops = np.diff(d["op_off"].astype(np.int64))
    ok = rows["status"] == oracle.OK
    inside = ok & ((rows["flags"] & 1) != 0)
    stripped = (norm["lead_ops"] + norm["trail_ops"]) > 0
    assert inside.any()
    assert (inside & stripped[rows["rec"]]).any()                          # its id gets a _TO.<lead>.<trail> suffix
    assert (rows["status"] == oracle.NONE_INDEL).any()
    assert (ok & (n_ops[rows["rec"]] > 2048)).any() and (ok & (n_ops[rows["rec"]] <= 2048)).any()
    for s in "+-":
        assert (ok & (d["strand"][rows["rec"]] == ord(s)) & ~inside).any(), s
    assert ok.sum() * 2 >= len(rows) and len(rows) >= 30
    assert (rows["status"] < oracle.PANIC_NOTFOUND).all()                  # (no row makes the reference panic)
    # windows cut records: rows whose text is not the whole swapped CIGAR
    assert sum(1 for h, t in zip(rows, ref["text"]) if int(h["status"]) == 0 and not (int(h["flags"]) & 1)) >= 10


def test_qbed_batch_one_record_fails_both_integrity_checks(qbed, oracle):
    d, ref = qbed
    r = d["special"]["both spans off"]
    r1 = d["special"]["target span off"]
    bad = np.nonzero(ref["red"]["status"] != oracle.OK)[0]
    assert bad.tolist() == [r, r1] and int(ref["red"]["status"][r]) == oracle.PANIC_INTEGRITY_T
    assert int(ref["norm"]["status"][r]) >= oracle.PANIC_NOTFOUND and int(ref["norm"]["status"][r1]) >= oracle.PANIC_NOTFOUND
    # a scan of the SWAPPED records is not Paf::from_file's check_integrity: where one span is off it names the other check, and the
    # I / D counters of every record with an indel change places -- why the wrapper scans the records as read first
    sw = oracle.reduce(oracle.Batch(ref["swapped"], d["op_off"], d["q_st"], d["q_en"], d["t_st"], d["t_en"], d["strand"]))
    assert int(ref["red"]["status"][r1]) == oracle.PANIC_INTEGRITY_T and int(sw["status"][r1]) == oracle.PANIC_INTEGRITY_Q
    assert int(sw["status"][r]) == oracle.PANIC_INTEGRITY_T   # both spans off: the target check comes first either way
    assert not np.array_equal(sw["ins"], ref["red"]["ins"]) and np.array_equal(sw["ins"], ref["red"]["del"])


def test_qbed_flag_changes_the_answer(qbed, oracle):
    d, ref = qbed
    plain = oracle.Batch(d["ops"], d["op_off"], d["t_st"], d["t_en"], d["q_st"], d["q_en"], d["strand"], d["contig"])
    rows, _ = oracle.liftover(plain, d["w_contig"], d["w_st"], d["w_en"])
    assert len(rows) != len(ref["rows"]) or not np.array_equal(rows["t_st"], ref["rows"]["t_st"])


def test_without_stripped_inside_is_what_the_largest_wrapper_takes(qbed, oracle):
    d, ref = qbed
    keep = qu.windows_without_stripped_inside(d, ref)
    assert 0 < (~keep).sum() < len(keep) // 2
    e = qu.with_windows(d, keep)
    r2 = qu.qbed_reference(oracle, e)
    stripped = (r2["norm"]["lead_ops"] + r2["norm"]["trail_ops"]) > 0
    ok_inside = (r2["rows"]["status"] == 0) & ((r2["rows"]["flags"] & 1) != 0)
    assert not (ok_inside & stripped[r2["rows"]["rec"]]).any() and ok_inside.any()
    assert (r2["rows"]["status"] == 0).sum() >= 15
