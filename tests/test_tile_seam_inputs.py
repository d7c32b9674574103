"""What the inputs of tests/test_gpu_tile_seams.py hold, proven on the CPU: tests/tile_seam_util.py builds them, rb_plan_tiles_host cuts them,
the per-base oracle counts their hits.  No device."""
import numpy as np
import pytest

import break_seam_util as bs
import tile_seam_util as u
from rbtest_util import batch_args


def one_tile_each(b, where, op_off=None):
    """the plan puts exactly the claimed records into exactly one tile each, and nothing else into any tile"""
    tiles = u.plan_tiles(b["op_off"] if op_off is None else op_off)
    assert [(f, c) for f, c, tiny in tiles] == list(where) and not any(t for _, _, t in tiles)


def norm_of(oracle, b):
    return oracle.normalize(oracle.Batch(*batch_args(b), b["contig"]))


def good_records_are_regular(oracle, b, but=()):
    norm = norm_of(oracle, b)
    for r, c in enumerate(u.records(b)):
        if r not in but:
            assert bs.is_regular(c) and norm["status"][r] == 0 and norm["lead_ops"][r] == 0 and norm["trail_ops"][r] == 0, r
            k, ln = c & 15, c >> 4
            assert 1 <= int(ln.min()) and (int(ln.max()) <= 30 or int(ln.max()) == bs.BIG)
            indel = np.flatnonzero((k == u.I) | (k == u.D))
            assert np.isin(k[indel - 1], (u.M, u.EQ, u.X)).all() and np.isin(k[indel + 1], (u.M, u.EQ, u.X)).all()
    assert (np.diff(b["t_st"].astype(np.int64)) > 0).all() and (b["t_st"][1:] >= b["t_en"][:-1] + np.uint64(u.ROOM - 1)).all()
    assert set(b["strand"][:2].tolist()) == {ord("+"), ord("-")} and (b["strand"][2:] == b["strand"][:-2]).all()


def lift_rows(oracle, b, w):
    return oracle.liftover(oracle.Batch(*batch_args(b), b["contig"]), *w)[0]


def hits_of(oracle, b, w):
    return u.hits_per_record(lift_rows(oracle, b, w), len(b["t_st"]), norm_of(oracle, b)["status"])


def ok_clip_per_record(oracle, b, w, recs):
    rows = lift_rows(oracle, b, w)
    ok = np.bincount(rows["rec"][rows["status"] == 0].astype(np.int64), minlength=len(b["t_st"]))
    assert (ok[list(recs)] >= 1).all()


def pieces_of(b, where, max_size):
    cigs = u.records(b)
    return [sum(bs.n_pieces(cigs[r], max_size) for r in range(f, f + c)) for f, c in where]


def test_the_model_on_plain_tiles():
    no = [False] * 32
    assert u.handed_back(32, no, [2] * 32) == 0 and u.handed_back(32, no, [2] * 31 + [3]) == 1
    assert u.handed_back(3, [False] * 3, [65, 0, 0]) == 3 and u.handed_back(3, [False] * 3, [64, 1, 0]) == 2
    bad = lambda *k: [j in k for j in range(32)]  # noqa: E731
    assert u.handed_back(32, bad(0), [1] * 32) == 1 and u.handed_back(32, bad(31), [1] * 32) == 1 and u.handed_back(32, bad(0, 31), [1] * 32) == 2
    assert u.handed_back(32, bad(15), [1] * 32) == 16 and u.handed_back(32, bad(16), [1] * 32) == 16 and u.handed_back(32, bad(15, 16), [1] * 32) == 17
    assert u.handed_back(32, bad(10, 21), [1] * 32) == 22 and u.handed_back(32, bad(*range(1, 32, 2)), [1] * 32) == 31
    assert u.handed_back(32, [True] * 32, [1] * 32) == 32
    assert u.handed_back(32, bad(25), [3] * 32) == 11 and u.handed_back(32, bad(5), [3] * 32) == 11 + 6
    assert u.handed_back(4, [False] * 4, [1] * 4, gaps=[9999, 1024, 0, 7]) == 0 and u.handed_back(4, [False] * 4, [1] * 4, gaps=[0, 1025, 0, 7]) == 4
    assert u.handed_back(4, [True, False, False, False], [1] * 4, gaps=[0, 1025, 0, 7]) == 1   # (the gap in front of the run's first record is nobody's)
    assert u.handed_back(4, [False] * 4, pieces=[16] * 4) == 0 and u.handed_back(4, [False] * 4, pieces=[16, 16, 16, 17]) == 4


# ---- A
@pytest.fixture(scope="module")
def fam_a():
    return [u.family_a(k) for k in range(len(u.A_HEADS))]


def test_a_geometry(fam_a, oracle):
    rel7, ends, steps, on_step = set(), set(), set(), set()
    for k, (b, where, claims) in enumerate(fam_a):
        one_tile_each(b, where)
        good_records_are_regular(oracle, b)
        n = np.diff(b["op_off"].astype(np.int64))
        for (first, cnt), (head, total) in zip(where, claims):
            g = u.geometry(b, first, cnt)
            assert g["head"] == head == u.A_HEADS[k] and g["n_tile"] == total - head and g["n_steps"] == -(-total // u.STEP) and g["gend3"] == total & 3
            assert n[first - 1] > u.SHORT_MAX and (first + cnt == len(n) or n[first + cnt] > u.SHORT_MAX)
            rel7 |= g["rel7"]
            on_step |= g["rel_step"] & {0, u.STEP - 1}
            steps.add(g["n_steps"])
            if total == 511:
                assert (n[first:first + 20] == 8).all() and g["rel7"] == {head & 7}
        assert where[-1][0] + where[-1][1] == len(n)           # the batch ends with a tile
        ends.add(u.geometry(b, *where[-1])["gend3"])
    assert rel7 == set(range(8)) and ends == {0, 1, 2, 3} and on_step == {0, u.STEP - 1} and steps == {1, 2, 3, 4, 8}
    assert [c for _, _, cl in fam_a for c in cl if c[1] >= u.TILE_OPS] == [(0, 4064), (31, 4095)]


def test_a_hits_and_pieces(fam_a, oracle):
    for b, where, _ in fam_a:
        w = u.windows_in_turn(b, where)
        h = hits_of(oracle, b, w)
        per_tile = [int(h[f:f + c].sum()) for f, c in where]
        assert max(per_tile) <= u.RBT_HITS and min(per_tile) >= 3 and int(h.sum()) >= len(w[1]) - len(where)
        assert u.expected_back(oracle, b, lift_rows(oracle, b, w)) == 0
        ok_clip_per_record(oracle, b, w, [r for f, c in where for r in range(f, f + c)])
        p = pieces_of(b, where, u.BREAK_A)
        assert max(p) <= u.RBT_HITS and all(x > c for x, (f, c) in zip(p, where))     # every tile is cut somewhere
        assert u.expected_back(oracle, b, max_size=u.BREAK_A) == 0


def test_a_window_kinds():
    b, where, _ = u.family_a(1)
    first = where[3][0] + 1
    t0, t1 = int(b["t_st"][first]), int(b["t_en"][first])
    assert u.window(b, first, 0) == (t0, t0 + 1) and u.window(b, first, 1) == (t1 - 1, t1) and u.window(b, first, 5)[1] == t1
    assert u.window(b, first, 6)[0] == int(b["t_st"][first + 1]) and u.window(b, first, 7) == (t0 - 1, t1 + 1)
    c = u.records(b, [first])[0]
    s4, e4 = u.window(b, first, 4)
    p = t0 + int(c[0] >> 4) + (int(c[1] >> 4) if int(c[1] & 15) != u.I else 0)
    assert p < s4 < e4 < p + int(c[2] >> 4)
    assert t0 < u.window(b, first, 2)[0] < t0 + int(c[0] >> 4) and t1 - int(c[-1] >> 4) <= u.window(b, first, 3)[0] < t1


# ---- B
@pytest.mark.parametrize("name", list(u.B_CASES))
def test_b_hit_counts(oracle, name):
    b, where = u.b_batch()
    one_tile_each(b, where)
    good_records_are_regular(oracle, b)
    first, cnt = where[0]
    assert cnt == u.B_REC and u.geometry(b, first, cnt)["head"] == u.B_HEAD
    w = u.b_windows(b, where, name)
    h = hits_of(oracle, b, w)
    counts = u.B_CASES[name][0]
    assert h[first:first + cnt].tolist() == counts and int(h.sum()) == sum(counts)
    assert (sum(counts) > u.RBT_HITS) == (name in u.B_OVERFLOW)
    back = u.expected_back(oracle, b, lift_rows(oracle, b, w))
    want = {"sum65": 1, "hit64_ends_record15": 8, "hit64_inside_record15": 9, "first_record_64": 23, "first_record_65": 24}
    assert back == want.get(name, 0)
    ok_clip_per_record(oracle, b, w, [first + j for j, k in enumerate(counts) if k and j < u.B_REC - back])


# ---- C
@pytest.mark.parametrize("name", list(u.C_CASES))
def test_c_bad_records(oracle, name):
    lanes, kind, per = u.C_CASES[name]
    b, where, w = u.c_case(name)
    one_tile_each(b, where)
    first, cnt = where[0]
    assert cnt == u.C_REC == 32 and u.geometry(b, first, cnt)["head"] == u.C_HEAD
    good_records_are_regular(oracle, b, but=[first + j for j in lanes])
    bad = u.bad_records(oracle, b)
    assert np.flatnonzero(bad).tolist() == [first + j for j in lanes]
    norm = norm_of(oracle, b)
    for j in lanes:
        c = u.records(b, [first + j])[0]
        if kind == "split":
            assert not bs.is_regular(c) and norm["status"][first + j] == 0 and norm["lead_ops"][first + j] == 0
        elif kind == "lead_ins":
            assert norm["lead_ops"][first + j] == 1 and norm["status"][first + j] == 0 and bs.is_regular(c[1:])
        else:
            assert bs.is_regular(c) and norm["status"][first + j] != 0
    h = hits_of(oracle, b, w)[first:first + cnt]
    assert h.tolist() == [0 if (kind == "t_en" and j in lanes) else per for j in range(cnt)]
    back = u.expected_back(oracle, b, lift_rows(oracle, b, w))
    want = {"lane0": 1, "lane31": 1, "lanes0_31": 2, "lane15": 16, "lane16": 16, "lanes15_16": 17, "three_runs_of_ten": 22, "odd_lanes": 31,
            "all_split": 32, "all_lead_ins": 32, "all_t_en": 32, "hit_cut_then_bad_behind_it": 11, "hit_cut_and_run_cut": 17}
    assert back == want[name]
    assert u.expected_back(oracle, b, max_size=50) == u.handed_back(cnt, bad[first:first + cnt], pieces=[1] * cnt)
    if back < cnt:
        ok_clip_per_record(oracle, b, w, np.flatnonzero(~bad[first:first + cnt]) + first)


# ---- D
def check_starts(oracle, s):
    b, twin = s["b"], s["twin"]
    first, cnt = s["first"], s["cnt"]
    one_tile_each(b, [(first, cnt)])
    good_records_are_regular(oracle, twin)
    old0, old1 = b["op_off"][:-1].astype(np.int64), b["op_off"][1:].astype(np.int64)
    st, n = s["starts"][:-1].astype(np.int64), s["n_ops"]
    assert (st >= old0).all() and (st + n <= old1).all() and (np.diff(st) > 0).all()         # every record inside its own old extent, in order
    assert np.array_equal(u.gap_list(s)[2:], s["gaps"][2:]) and u.gap_list(s)[1] == st[1] - old0[1]
    mine = np.zeros(len(b["ops"]), bool)
    for r in range(len(st)):
        mine[st[r]:st[r] + n[r]] = True
    assert np.array_equal(b["ops"][mine], twin["ops"]) and np.array_equal(np.diff(twin["op_off"].astype(np.int64)), n)
    assert np.isin(b["ops"][~mine], (u.G_ONES, u.G_EQ)).all() and int(mine.sum()) == len(twin["ops"])
    for k in ("t_st", "t_en", "q_st", "q_en", "strand"):
        assert np.array_equal(b[k], twin[k])
    return u.geometry(b, first, cnt, starts=st, n_ops=n), u.geometry(b, first, cnt)


def test_d_kept_gaps_and_geometry(oracle):
    seen, ends, g_start, g_end = set(), set(), set(), set()
    for name in u.D_CASES:
        s = u.d_case(name)
        new, old = check_starts(oracle, s)
        gaps = s["gaps"][2:].tolist()
        seen |= set(gaps)
        ends.add(new["gend3"])
        st, n = s["starts"][:-1].astype(np.int64), s["n_ops"]
        g0 = int(st[1]) & ~31
        for r in range(2, len(st)):
            if st[r] > st[r - 1] + n[r - 1]:
                g_start.add(int(st[r - 1] + n[r - 1] - g0) & 7), g_end.add(int(st[r] - 1 - g0) & 7)
        w = u.windows_in_turn(s["twin"], [(s["first"], s["cnt"])])
        rows = lift_rows(oracle, s["twin"], w)
        back = u.expected_back(oracle, s["twin"], rows, gaps=s["gaps"], op_off=s["b"]["op_off"])
        assert back == u.D_BACK.get(name, 0), name
        assert int(u.hits_per_record(rows, len(st), np.zeros(len(st)))[1:].sum()) <= u.RBT_HITS
        for ms, two in ((u.BREAK_A, False), (u.BREAK_A, True)):
            assert u.expected_back(oracle, s["twin"], max_size=ms, gaps=s["gaps"], op_off=s["b"]["op_off"], two_walk=two) == back
        assert sum(bs.n_pieces(c, u.BREAK_A) for c in u.records(s["twin"])[1:]) <= u.RBT_HITS
        ok_clip_per_record(oracle, s["twin"], w, [r for r in range(1, len(st)) if n[r] >= u.MIN_OPS])
        if name.startswith("front_"):
            front = u.D_CASES[name]["front"]
            assert old["head"] == 20 and new["head"] == (20 + front) % 32 != old["head"]
        if name == "tail_cut":
            assert new["n_steps"] < old["n_steps"]
        if name == "gap_holds_a_step":
            assert st[1] + n[1] - g0 <= u.STEP and st[2] - g0 >= 2 * u.STEP
    assert set(u.KEPT_GAPS) <= seen and u.RBT_GAP_MAX + 1 in seen and ends == {0, 1, 2, 3}
    assert g_start == set(range(8)) and g_end == set(range(8))
    s = u.d_case("shrunk_to_8")
    assert sorted(s["n_ops"][1:].tolist())[:3] == [8, 8, 8]
    s = u.d_case("shrunk_to_7")
    assert np.flatnonzero(s["n_ops"] < u.MIN_OPS).tolist() == [5, 9]


# ---- E
@pytest.mark.parametrize("max_size", u.E_SIZES)
def test_e_pieces(oracle, max_size):
    b, where = u.e_dense()
    one_tile_each(b, where)
    good_records_are_regular(oracle, b)
    g = u.geometry(b, *where[0])
    assert g["head"] == 15 and g["n_tile"] == 1010 and u.STEP - 1 in g["rel_step"]
    cut = max_size < bs.BIG
    assert pieces_of(b, where, max_size) == [where[0][1] * (3 if cut else 1)] and where[0][1] * 3 <= u.RBT_HITS
    s = u.e_starts()
    check_starts(oracle, s)
    assert s["gaps"][2:].tolist() == [1, 8, 65, 513, u.RBT_GAP_MAX]
    assert sum(bs.n_pieces(c, max_size) for c in u.records(s["twin"])[1:]) == s["cnt"] * (3 if cut else 1)
    for r, c in enumerate(u.records(s["twin"])[1:] + u.records(b, range(where[0][0], sum(where[0])))):
        big = np.flatnonzero((c >> 4) == bs.BIG).tolist()
        assert big == [1, len(c) - 2] and set((c[big] & 15).tolist()) <= {u.I, u.D}
    for two in (False, True):
        assert u.expected_back(oracle, b, max_size=max_size, two_walk=two) == 0
        assert u.expected_back(oracle, s["twin"], max_size=max_size, gaps=s["gaps"], op_off=s["b"]["op_off"], two_walk=two) == 0


# ---- the input of tests/test_gpu_tile.py::test_a_tile_is_cut_around_a_record_it_cannot_take
def test_the_model_on_the_cut_test_of_test_gpu_tile(oracle):
    bad = [5, 41, 42, 90]
    b = u.cut_test_input(bad)
    assert np.flatnonzero(u.bad_records(oracle, b)).tolist() == bad
    st = np.arange(0, 300_000, 49_999, dtype=np.uint64)   # (test_gpu_tile.sliding(span=300_000, step=49_999, width=12_000))
    w = (np.zeros(len(st), np.uint32), st, st + np.uint64(12_000))
    back = u.expected_back(oracle, b, lift_rows(oracle, b, w))
    assert len(bad) <= back < 96 // 2      # the range that test asserted before it asserted this count
    assert len(bad) <= u.expected_back(oracle, b, max_size=50) < 96 // 2
