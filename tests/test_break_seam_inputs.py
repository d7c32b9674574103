"""What the inputs of tests/test_gpu_break_seams.py hold (tests/break_seam_util.py), proved on the CPU: the records are regular and pass the
oracle's normalisation, their long indels lie on the seams the families name -- counted as the stream kernel counts and as
rb_k_break_pieces counts --, the piece counts and the cuts at the pass boundaries are the ones named, the tile batches fit one tile, and the
restated cut rule gives the oracle's number of rows per record on every family.  Counts only: the oracle's row coordinates are those of the
clip, which moves on to the next match op."""
import numpy as np
import pytest

import break_seam_util as u
from rbtest_util import batch_args


def _oracle_counts(oracle, b, max_size):
    rows, _ = oracle.break_paf(oracle.Batch(*batch_args(b), b["contig"]), max_size)
    assert (rows["status"] == 0).all()
    return np.bincount(rows["rec"].astype(np.int64), minlength=len(b["t_st"]))


def _status(oracle, b):
    return oracle.normalize(oracle.Batch(*batch_args(b), b["contig"]))["status"]


def _counts_agree(oracle, b, sizes=u.MAX_SIZES, ok=None):
    recs = u.records(b)
    for ms in sizes:
        got = _oracle_counts(oracle, b, ms)
        mine = np.array([u.n_pieces(c, ms) for c in recs])
        if ok is not None:
            assert (got[~ok] == 0).all()
            got, mine = got[ok], mine[ok]
        assert np.array_equal(got, mine), (ms, got[:8], mine[:8])


def test_planted_makes_what_it_says():
    for n, head, longs in ((60, 0, [1, 30, 58]), (61, 5, [6, 40, 41, 64]), (5400, 31, [32, 5120, 5121, 5400])):
        c = u.planted(n, head, longs)
        code, ln = c & 15, c >> 4
        assert len(c) == n and u.is_regular(c)
        at = np.array(sorted(longs)) - head
        assert (ln[at] == u.BIG).all() and np.isin(code[at], (u.I, u.D)).all()
        rest = np.ones(n, bool)
        rest[at] = False
        indel = np.isin(code, (u.I, u.D, u.X))
        assert (ln[rest & indel] <= 3).all() and (ln[rest & ~indel] <= 9).all() and (code[rest & ~indel] == u.EQ).all()
        assert int(np.where(code == u.I, 0, ln).sum()) < 100_000
        with pytest.raises(AssertionError):
            u.planted(n, head, [head])  # the first op is a match op


@pytest.mark.parametrize("variant", u.VARIANTS)
def test_family_a_cuts_every_seam_class_on_the_stated_side(oracle, variant):
    b, idx = u.family_a(variant)
    assert sorted(int(b["op_off"][r]) % 32 for r in idx) == u.HEADS
    assert all(u.is_regular(c) for c in u.records(b)) and (_status(oracle, b) == 0).all()
    want = {"before": (True, False), "behind": (False, True), "both": (True, True)}[variant]
    for classes, unit in ((u.STREAM_CLASSES, 32), (u.PIECES_CLASSES, 4)):
        before, behind = set(), set()
        for r in idx:
            x, y = u.seam_sides(u.records(b, [r])[0], int(b["op_off"][r]) % unit, classes)
            before |= x
            behind |= y
        if want[0]:
            assert before >= set(classes), (variant, unit, before)
        if want[1]:
            assert behind >= set(classes), (variant, unit, behind)
    # the long records are the stream kernel's, and two of them reach a second segment from every head class
    n = np.diff(b["op_off"].astype(np.int64))[idx]
    assert (n > 2048).all() and (n > u.SEGMENT + 256).sum() >= 5
    pieces = _oracle_counts(oracle, b, 100)[idx]
    assert 9 <= pieces.min() and pieces.max() <= 13
    assert (_oracle_counts(oracle, b, u.BIG) == 1).all()          # the comparison is strict
    assert _oracle_counts(oracle, b, 0)[idx].min() > 60 * 10      # a cut at every indel: tens of passes
    _counts_agree(oracle, b)


def test_family_a_both_opens_no_empty_piece(oracle):
    one, _ = u.family_a("behind")
    two, idx = u.family_a("both")
    assert np.array_equal(_oracle_counts(oracle, one, 100)[idx], _oracle_counts(oracle, two, 100)[idx])


def test_family_b_piece_counts_and_pass_boundaries(oracle):
    fam = u.family_b()
    assert len(fam) == 11
    b = u.make_batch([c for c, _, _ in fam.values()])
    assert (b["op_off"] % 32 == 0).all() and (np.diff(b["op_off"].astype(np.int64)) > 2048).all()
    assert (_status(oracle, b) == 0).all()
    got = _oracle_counts(oracle, b, u.BIG - 1)
    for r, (name, (c, pieces, closing)) in enumerate(fam.items()):
        assert u.is_regular(c) and got[r] == pieces, (name, got[r], pieces)
        cut, last = u.cuts(c, u.BIG - 1)
        assert last and len(cut) == pieces - 1
        if closing is not None:
            assert cut[u.PASS - 1] == closing, (name, cut[u.PASS - 1])
        if name.startswith("cut32"):
            # the dense tail: pieces 32 .. 64 are closed behind the 32nd cut, 37 ops apart, so pass 3 resumes in the segment pass 2 resumed in
            tail = np.array(cut[u.PASS:2 * u.PASS + 1])
            assert len(tail) == 33 and tail[0] > closing and (np.diff(tail) == 37).all()
            assert tail[-1] // u.SEGMENT == tail[0] // u.SEGMENT
    assert fam["cut32_early"][2] < 2 * u.STEP and fam["cut32_seg1_middle"][2] // u.SEGMENT == 1 and len(fam["cut32_seg1_middle"][0]) > 2 * u.SEGMENT
    c = fam["cut32_run_5119_5120"][0]
    assert (c[5119] >> 4) == u.BIG == (c[5120] >> 4) and {int(c[5119]) & 15, int(c[5120]) & 15} == {u.I, u.D}
    c = fam["last_piece_one_op"][0]
    assert (c[-2] >> 4) == u.BIG and (int(c[-1]) & 15) == u.EQ
    _counts_agree(oracle, b, (100, u.BIG - 1, u.BIG))
    for tiny_at in (31, 63, 33):
        t = u.make_batch([u.tiny_record(tiny_at)])
        assert _oracle_counts(oracle, t, 100)[0] == 71 == u.n_pieces(u.tiny_record(tiny_at), 100)


def test_family_c_has_records_the_oracle_keeps_and_records_it_drops(oracle):
    b, ends = u.family_c()
    ok = _status(oracle, b) == 0
    assert 8 <= ok.sum() < len(ok)
    kept = [e for e, k in zip(ends, ok) if k]
    assert any(e[0] for e in kept) and any(e[1] == 2 for e in kept) and any(e == (0, 0) for e in kept)
    for c, (lead, trail) in zip(u.records(b), ends):
        assert u.is_regular(c, ends=False) and u.is_regular(c[lead:len(c) - trail])
    long_ = np.diff(b["op_off"].astype(np.int64)) > 2048
    assert (ok & long_).sum() >= 4 and (ok & ~long_).sum() >= 2
    _counts_agree(oracle, b, (100, u.BIG, 0), ok=ok)


def test_family_d_piece_counts_around_the_collect_cap(oracle):
    for n_cut in u.CAP_CUTS:
        c = u.cap_record(n_cut)
        assert u.is_regular(c) and len(c) == 2 * n_cut + 1
        b = u.make_batch([c])
        assert _status(oracle, b)[0] == 0 and _oracle_counts(oracle, b, 100)[0] == n_cut + 1
    assert [n + 1 for n in u.CAP_CUTS] == [u.CAP - 1, u.CAP, u.CAP + 1]
    b, want = u.family_d_batch()
    assert len(want) == 70 and sorted(want)[-3:] == [u.CAP - 1, u.CAP, u.CAP + 1] and {0, 1} < {w - 1 for w in want}
    assert (_status(oracle, b) == 0).all() and _oracle_counts(oracle, b, 100).tolist() == want
    _counts_agree(oracle, b, (100, u.BIG))


@pytest.mark.parametrize("pieces", [u.TILE_HITS - 1, u.TILE_HITS, u.TILE_HITS + 1])
def test_family_e_batches_fit_one_tile(oracle, pieces):
    assert (u.TILE_REC, u.TILE_OPS, u.TILE_HITS) == (32, 4064, 64)
    b = u.family_e(pieces)
    n = np.diff(b["op_off"].astype(np.int64))
    assert 16 <= len(n) <= u.TILE_REC and int(n.sum()) <= u.TILE_OPS and n.min() >= 40 and n.max() <= 120
    assert set((b["op_off"][:-1] % 8).tolist()) == set(range(8))
    assert all(u.is_regular(c) for c in u.records(b)) and (_status(oracle, b) == 0).all()
    assert int(_oracle_counts(oracle, b, 100).sum()) == pieces
    second = sum(int(c[1] >> 4) == u.BIG for c in u.records(b))
    last_but_one = sum(int(c[-2] >> 4) == u.BIG for c in u.records(b))
    assert second >= 8 and last_but_one >= 8
    _counts_agree(oracle, b, (100, u.BIG))


def test_family_f_stays_ok_and_keeps_its_pieces(oracle):
    b, idx = u.family_a("behind", soft=True)
    assert all((int(c[0]) & 15) == u.S and not u.is_regular(c) and u.is_regular(c[1:]) for c in u.records(b, idx))
    assert sorted(int(b["op_off"][r]) % 32 for r in idx) == u.HEADS
    assert (_status(oracle, b) == 0).all()
    for r in idx:  # the long indels lie where seam_longs puts them, counted from g0 with the clip in front
        c, head = u.records(b, [r])[0], int(b["op_off"][r]) % 32
        assert (np.flatnonzero((c >> 4) == u.BIG) + head).tolist() == u.seam_longs("behind", head + 1, len(c) - 1)
    assert (_oracle_counts(oracle, b, u.BIG) == 1).all() and _oracle_counts(oracle, b, 100)[idx].min() >= 9
    _counts_agree(oracle, b)
