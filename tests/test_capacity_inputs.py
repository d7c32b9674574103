"""The inputs of tests/test_gpu_capacity.py hold what those tests lean on -- shown with the oracle alone, no GPU: how many rows and how
many clipped ops each input has (what a call with fewer cannot fit), that the windows are deep enough for clips to lose their slot,
that a record has more pieces than the collect pass of two-walk break-paf keeps, that the lopsided batch is lopsided, and that the
rows a short one-walk call asks for reach, within the host wrapper's six attempts, a size at which no scratch-row cursor can run out."""
import numpy as np
import pytest

import capacity_util as cu


# (input, legacy policy, max_size) -> (N rows, ops of all clips): the oracle's, pinned so that a change of a generator shows here first
TRUTHS = [("L-regular", False, None), ("L-regular", True, None), ("L-sparse", False, None), ("L-irregular", False, None), ("L-irregular", True, None),
          ("L-few", False, None), ("B-regular", False, 0), ("B-regular", False, 100), ("B-regular", True, 100), ("B-lopsided", False, 100),
          ("B-irregular", False, 0), ("B-irregular", False, 100)]


@pytest.mark.parametrize("name,legacy,max_size", TRUTHS)
def test_rows_and_clipped_ops_of_every_input(oracle, name, legacy, max_size):
    inp, t = cu.get_input(oracle, name), cu.truth(oracle, name, legacy, max_size)
    print(f"{name} legacy={legacy} max_size={max_size}: n_rec {inp.n_rec} n_ops {inp.n_ops} arenas {inp.n_arena} N {t.N} clip ops {t.clip_ops} (padded {t.clip_ops_padded})")
    assert inp.n_arena == {"L-few": 1, "B-lopsided": 4}.get(name, 2)
    # rows_cap in {1, N // 2, N - 1} are three different short capacities, and N rows are more than one pass of a record and one block hold
    assert t.N > 1024 and len({1, t.N // 2, t.N - 1}) == 3
    # out_cap = n_arena * 1024 - 4 (no slot fits, arenas of 1020 ops) is short whatever the code does: the clips alone are more ops
    assert t.clip_ops > inp.n_arena * 1024
    assert t.clip_ops_padded >= t.clip_ops
    # every record of the irregular mixes passes remove_trailing_indels + check_integrity, or is one the record scan gives no rows (UNFUSED)
    ok = cu._ok(oracle, inp.b)
    if name not in cu.UNFUSED:
        assert ok.all()
    else:
        assert not ok.all() and ok.sum() > 0.8 * inp.n_rec  # (break_frac: headers that disagree with the CIGAR)
    assert (np.bincount(t.rows["rec"].astype(np.int64), minlength=inp.n_rec)[~ok] == 0).all()


def test_l_regular_windows_are_deeper_than_the_slots(oracle):
    inp = cu.get_input(oracle, "L-regular")
    wc, st, en = inp.windows
    assert (np.diff(st.astype(np.int64)) == 40).all() and ((en - st) == 200).all()
    depth = [(int(((st <= p) & (en > p)).sum())) for p in range(200, int(st[-1]), 97)]
    assert min(depth) == 5 and max(depth) == 5  # > 4: more than RB_MS = 2 slots, more than rb_plan_out_capacity's four copies
    # and records see them: some record has more hits than one streaming pass resolves (32), most have more than two
    t = cu.truth(oracle, "L-regular")
    per_rec = np.bincount(t.rows["rec"].astype(np.int64), minlength=inp.n_rec)
    assert per_rec.max() > 32 and np.median(per_rec) > 2
    # the tile kernel and the per-record kernel both get records: short ones (8 .. 2048 ops) that lie side by side, and long ones
    n_ops = np.diff(inp.b["op_off"].astype(np.int64))
    assert (n_ops >= 200).sum() >= 30 and (n_ops < 40).sum() >= 500


def test_l_sparse_shares_the_batch(oracle):
    a, b = cu.get_input(oracle, "L-regular"), cu.get_input(oracle, "L-sparse")
    assert np.array_equal(a.b["ops"], b.b["ops"]) and np.array_equal(a.b["t_st"], b.b["t_st"]) and len(b.windows[1]) == 60


def test_irregular_inputs_are_irregular(oracle):
    for name, lo, hi in (("L-irregular", 0.15, 0.30), ("B-irregular", 0.02, 0.05)):
        inp = cu.get_input(oracle, name)
        frac = inp.odd.mean()
        assert lo < frac <= hi, (name, frac)
        t = cu.truth(oracle, name, False, 100 if name[0] == "B" else None)
        assert np.isin(t.rows["rec"], np.flatnonzero(inp.odd)).sum() > 20, name  # rows the generic kernel has to make


def test_l_few_overflows_the_host_wrapper_s_first_guess(oracle):
    inp, t = cu.get_input(oracle, "L-few"), cu.truth(oracle, "L-few")
    assert inp.n_rec == 40 and t.N > 16 * inp.n_rec + len(inp.windows[1]) + 1024  # lift_sized (capi.hip): rows_cap of the first attempt
    assert np.bincount(t.rows["rec"].astype(np.int64)).max() > 64                    # several passes per record


def test_b_regular_has_a_record_beyond_the_collect_pass(oracle):
    for name in ("B-regular", "B-irregular"):
        inp = cu.get_input(oracle, name)
        for max_size in inp.max_sizes:
            t = cu.truth(oracle, name, False, max_size)
            per_rec = np.bincount(t.rows["rec"].astype(np.int64), minlength=inp.n_rec)
            assert per_rec[300] == 601 and per_rec[300] > cu.RB_BP_CAP  # the `redo_only` second walk of the two-walk route


def test_b_lopsided_is_lopsided_and_its_retries_converge(oracle):
    inp, t = cu.get_input(oracle, "B-lopsided"), cu.truth(oracle, "B-lopsided", False, 100)
    per_rec = np.bincount(t.rows["rec"].astype(np.int64), minlength=inp.n_rec)
    heavy = np.arange(0, 24 * 44, 44)
    assert inp.n_rec == 1100 and inp.n_arena == 4 and (heavy % 2 == 0).all() and (heavy % 4 == 0).all()
    assert (per_rec[heavy] == 301).all() and (np.delete(per_rec, heavy) == 1).all()
    assert t.N == 24 * 301 + 1076
    # every record is short (at most 2048 ops: none is scheduled longest-first), so record r runs at schedule slot r
    assert np.diff(inp.b["op_off"].astype(np.int64)).max() == 601
    # with rows_cap = N a cursor's share is N / 4 rows; the heavy records alone ask more than that of any ONE or TWO cursors, and
    # whichever way records or tiles map to cursors, 24 x 301 pieces on four cursors put at least six heavy records on one
    share = t.N // inp.n_arena
    assert 24 * 301 // 2 > share
    # the growth rule of rb_k_finish reaches N * n_arena -- each cursor's share is then N, no cursor can run out -- in five steps: a
    # short first call and five more are the six attempts lift_sized allows
    assert cu.growth_steps(t.N, t.N * inp.n_arena) <= 5
    for name in ("B-regular", "B-irregular"):  # the others: two arenas
        i2 = cu.get_input(oracle, name)
        for max_size in i2.max_sizes:
            n = cu.truth(oracle, name, False, max_size).N
            assert cu.growth_steps(n, n * i2.n_arena) <= 5


def test_text_items(oracle):
    cigs, parsed, printed = cu.text_items(oracle)
    assert len(cigs) == 200 and [p.decode() for p in printed] == cigs
    total, nbytes = sum(len(p) for p in parsed), sum(len(p) for p in printed)
    assert total > 4096 and nbytes > 2 * total  # (an op is at least two characters)
    assert max(len(p) for p in parsed) > 256 and min(len(p) for p in parsed) == 0  # several steps of the format kernel; an empty CIGAR
    assert len({0, total // 2, total - 1, total}) == 4 and len({0, nbytes // 2, nbytes - 1, nbytes}) == 4
