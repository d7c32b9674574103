"""What the inputs of tests/test_gpu_magnitude.py hold, and that their references are right (CPU only).

clip_regular / break_regular (tests/magnitude_util.py) are the reference for regular records of 2^31 .. 2^32 - 1 units, which the
per-base oracle cannot expand.  They are pinned twice: against the per-base oracle on small regular records with windows on every kind of
boundary, both strands and both binary-search policies; and against the op-space CPU baseline (oracle/rb_opspace.c) on the big inputs
themselves -- both are exact by construction, so a difference there is a finding in rb_opspace.c.  The rest asserts the sizes the big
inputs are built for: sR, sQ, U, the lane sums the stream kernel sees, regularity, which records share a tile."""
import numpy as np
import pytest

import magnitude_util as mu
from rbtest_util import batch_args, random_batch, random_windows
from test_plan_tiles import cut


def _same_rows(got, want, what, flags=True):
    (rows, ops), (orows, oops) = got, want
    assert len(rows) == len(orows), (what, len(rows), len(orows))
    for k in ("rec", "win", "status"):
        assert np.array_equal(rows[k], orows[k]), (what, k)
    ok = orows["status"] == 0
    for k in ("t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_n") + (("flags",) if flags else ()):
        bad = np.nonzero(ok & (rows[k] != orows[k]))[0]
        assert len(bad) == 0, (what, k, bad[:5], rows[k][bad[:5]], orows[k][bad[:5]], orows["rec"][bad[:5]], orows["win"][bad[:5]])
    for g, o in zip(rows[ok], orows[ok]):
        assert np.array_equal(ops[int(g["out_off"]):int(g["out_off"]) + int(g["out_n"])], oops[int(o["out_off"]):int(o["out_off"]) + int(o["out_n"])]), \
            (what, int(o["rec"]), int(o["win"]))
    return int(ok.sum()), int((~ok).sum())


def _obatch(oracle, b):
    return oracle.Batch(*batch_args(b), b["contig"])


def test_shift_moves_coordinates_and_nothing_else():
    rng = np.random.default_rng(1)
    b = random_batch(rng, 300, "regular")
    w = random_windows(rng, b, 120)
    for Kt, Kq in mu.SHIFTS:
        sb, sw = mu.shift(b, w, Kt, Kq)
        for k, K in (("t_st", Kt), ("t_en", Kt), ("q_st", Kq), ("q_en", Kq)):
            assert sb[k].dtype == np.uint64 and [int(x) for x in sb[k]] == [int(x) + K for x in b[k]]
        assert [int(x) for x in sw[1]] == [int(x) + Kt for x in w[1]] and [int(x) for x in sw[2]] == [int(x) + Kt for x in w[2]]
        assert sb["ops"] is b["ops"] and sb["op_off"] is b["op_off"] and sw[0] is w[0]
        assert max(int(sb["t_en"].max()), int(sb["q_en"].max()), int(sw[2].max())) < 2**63
    # the first pair puts a start below 2^32 and an end above it, in records and in windows
    sb, sw = mu.shift(b, w, *mu.SHIFTS[0])
    assert ((sb["t_st"] < 2**32) & (sb["t_en"] > 2**32)).any() and ((sb["q_st"] < 2**32) & (sb["q_en"] > 2**32)).any()
    assert ((sw[1] < 2**32) & (sw[2] > 2**32)).any()


@pytest.mark.parametrize("policy", [mu.MODERN, mu.LEGACY])
def test_clip_regular_equals_the_per_base_oracle(oracle, policy):
    """every record on a contig of its own under twelve windows of its own, the ends drawn from its op boundaries"""
    rng = np.random.default_rng(40 + policy)
    recs = mu.small_regular(rng, 260)
    b = mu.batch_of(recs, contig=range(len(recs)))
    wc, ws, we = [], [], []
    kinds = dict(i_dup=0, in_d=0, at_start=0, at_last=0, around=0)
    for r, (ops, t_st, _, _) in enumerate(recs):
        sR = mu.sums(ops)[0]
        Rb = np.cumsum([0] + [ln if c in mu.REF else 0 for ln, c in ops])
        for s, e in mu.edge_windows(rng, ops, t_st, 12):
            wc.append(r); ws.append(s); we.append(e)
            for k, (ln, c) in enumerate(ops):  # what the window's ends fall on
                kinds["i_dup"] += c == mu.I and (s - t_st == Rb[k] - 1 or e - 1 - t_st == Rb[k] - 1)
                kinds["in_d"] += c in (mu.D, mu.N) and (Rb[k] <= s - t_st < Rb[k] + ln or Rb[k] <= e - 1 - t_st < Rb[k] + ln)
            kinds["at_start"] += s == t_st
            kinds["at_last"] += e == t_st + sR
            kinds["around"] += s < t_st and e > t_st + sR
    w = (np.array(wc, np.uint32), np.array(ws, np.uint64), np.array(we, np.uint64))
    assert min(kinds.values()) > 50, kinds
    n_ok, n_none = _same_rows(mu.liftover_regular(b, w, policy), oracle.liftover(_obatch(oracle, b), *w, policy=policy), f"policy {policy}")
    assert n_ok + n_none >= 2000 and n_none > 20, (n_ok, n_none)
    # a plain call agrees with the batch form
    ops, t_st, q_st, strand = recs[3]
    c = mu.clip_regular(mu.cigar_string(ops), t_st, q_st, strand, t_st, t_st + mu.sums(ops)[0], policy)
    assert c["status"] == 0 and not c["inside"] and c["ops"] == ops and c["t_st"] == t_st


def test_the_two_policies_differ_on_these_windows(oracle):
    """(otherwise the pin above would say nothing about the binary search: a window that ends on the base in front of an insertion finds
    the base or the insertion, by the generation of the standard library)"""
    rng = np.random.default_rng(40)
    recs = mu.small_regular(rng, 260)
    b = mu.batch_of(recs, contig=range(len(recs)))
    w = [(r, s, e) for r, (ops, t_st, _, _) in enumerate(recs) for s, e in mu.edge_windows(rng, ops, t_st, 12)]
    w = (np.array([x[0] for x in w], np.uint32), np.array([x[1] for x in w], np.uint64), np.array([x[2] for x in w], np.uint64))
    a, l = mu.liftover_regular(b, w, mu.MODERN)[0], mu.liftover_regular(b, w, mu.LEGACY)[0]
    assert len(a) == len(l) and ((a["status"] != l["status"]) | (a["q_st"] != l["q_st"]) | (a["q_en"] != l["q_en"])).sum() > 5


@pytest.mark.parametrize("policy", [mu.MODERN, mu.LEGACY])
@pytest.mark.parametrize("max_size", [0, 2, 10])
def test_break_regular_equals_the_per_base_oracle(oracle, policy, max_size):
    rng = np.random.default_rng(900 + max_size)
    b = mu.batch_of(mu.small_regular(rng, 300, max_ops=24))
    n_ok, n_none = _same_rows(mu.break_paf_regular(b, max_size, policy), oracle.break_paf(_obatch(oracle, b), max_size, policy=policy),
                              f"break {max_size} policy {policy}", flags=False)
    assert n_ok > (600 if max_size < 10 else 300)


# ------------------------------------------------------------------ the big inputs
def _spans_batch(t_st, with_overflow=False):
    recs = []
    for i, U in enumerate(mu.SPAN_SIZES + ((2**32,) if with_overflow else ())):
        ops = mu.spans_record(U)
        recs.append((ops, t_st, 77 + i, "+-"[i % 2]))
        recs.append((ops, t_st, 77 + i, "-+"[i % 2]))
    return mu.batch_of(recs, contig=[i // 2 for i in range(len(recs))])


def spans_case(t_st):
    """(batch of the five sizes on both strands, each size on a contig of its own; its windows)"""
    b = _spans_batch(t_st)
    wc, ws, we = [], [], []
    for i, U in enumerate(mu.SPAN_SIZES):
        c, s, e = mu.span_windows(mu.spans_record(U), t_st)
        wc.append(c + np.uint32(i)); ws.append(s); we.append(e)
    return b, (np.concatenate(wc), np.concatenate(ws), np.concatenate(we))


@pytest.mark.parametrize("t_st", [1000, 2**32 - 5])
def test_span_records_hold_what_they_are_built_for(oracle, t_st):
    b, w = spans_case(t_st)
    for i, U in enumerate(mu.SPAN_SIZES):
        ops = mu.as_ops(b["ops"][int(b["op_off"][2 * i]):int(b["op_off"][2 * i + 1])])
        sR, sQ, u = mu.sums(ops)
        assert u == U and mu.is_regular(ops) and 15 <= len(ops) <= 40 and max(ln for ln, _ in ops) < 2**28
        assert {mu.I, mu.D, mu.N} <= {c for _, c in ops}
        assert int(b["t_en"][2 * i]) - t_st == sR and int(b["q_en"][2 * i]) - int(b["q_st"][2 * i]) == sQ
        assert chr(b["strand"][2 * i]) != chr(b["strand"][2 * i + 1])
        # the fused scan's lane guard: a lane's eight ops reach 2^25, so the fused scan hands these records back (route not asserted there)
        assert max(mu.lane_sums(b, 2 * i)) >= 2**25
    sR = [int(b["t_en"][2 * i]) - t_st for i in range(len(mu.SPAN_SIZES))]
    assert sR[0] < 2**31 and max(sR) > 2**31 + 1  # reference offsets on both sides of 2^31 ...
    offs = {int(s) - t_st for s, e in zip(w[1], w[2]) if int(e) - int(s) == 1}
    assert {0, 2**31 - 1, 2**31, 2**31 + 1} <= offs and any(x - 1 in offs for x in sR)  # ... and windows one base wide on them
    # the record of 2^32 units is one unit past what a regular record may hold
    assert mu.sums(mu.spans_record(2**32))[2] == 2**32 and mu.is_regular(mu.spans_record(2**32))
    # the run-length reference against the op-space baseline: rows, clips, order
    got, want = mu.liftover_regular(b, w), oracle.liftover_opspace(_obatch(oracle, b), *w, n_threads=4)
    assert want is not None
    n_ok, n_none = _same_rows(got, want, f"spans at {t_st}")
    assert n_ok > 150 and n_none >= 10, (n_ok, n_none)
    for max_size in (100, 2**27):
        got, want = mu.break_paf_regular(b, max_size), oracle.break_opspace(_obatch(oracle, b), max_size, n_threads=4)
        assert want is not None
        assert _same_rows(got, want, f"spans at {t_st}, break {max_size}", flags=False)[0] >= (20 if max_size == 100 else 10)


def lane_case():
    """64-op records whose ops 8 .. 15 (one lane) or 4 .. 11 (two lanes) sum to 2^25 - 1, 2^25, 2^25 + 1; both strands"""
    recs = []
    for first in (8, 4):
        for j, total in enumerate(mu.LANE_SUMS):
            recs.append((mu.lane_record(total, first), 1000 + 13 * j, 400 + j, "+-"[(j + first // 4) % 2]))
    b = mu.batch_of(recs)
    sR = int((b["t_en"] - b["t_st"]).max())
    st = sorted({0, 1, 200, 2**24, 2**25 - 40, 2**25 - 1, 2**25, 2**25 + 1, 2**25 + 300, sR - 50})
    w = (np.zeros(len(st), np.uint32), np.array(st, np.uint64) + np.uint64(1000), np.array(st, np.uint64) + np.uint64(1000 + 2000))
    return b, w


def test_lane_records_hold_what_they_are_built_for(oracle):
    b, w = lane_case()
    assert (b["op_off"] % np.uint64(32) == 0).all()  # every record starts a lane: lane = op index // 8
    for r in range(6):
        ops = mu.as_ops(b["ops"][64 * r:64 * r + 64])
        ls = mu.lane_sums(b, r)
        assert mu.is_regular(ops) and len(ls) == 8
        if r < 3:
            assert ls[1] == mu.LANE_SUMS[r] and max(ls[:1] + ls[2:]) < 2**12
        else:  # the same eight ops across two lanes: neither reaches the guard
            assert ls[0] + ls[1] > mu.LANE_SUMS[r - 3] and max(ls) < 2**25 and min(ls[0], ls[1]) > 2**23
    n_ok, _ = _same_rows(mu.liftover_regular(b, w), oracle.liftover_opspace(_obatch(oracle, b), *w, n_threads=4), "lane records")
    assert n_ok >= 25
    assert _same_rows(mu.break_paf_regular(b, 0), oracle.break_opspace(_obatch(oracle, b), 0, n_threads=4), "lane records, break", flags=False)[0] == 30  # (four indels a record: five pieces)


S = mu.TILE_SMALL
# name -> (the tile's records, whether the tile kernel keeps the tile).  The guards are reached twice: in records of several hundred ops whose
# lanes stay below 2^25, so that the guard under test alone decides (the route is asserted), and in records of a dozen ops, whose lanes
# reach 2^25 and which the tile kernel therefore hands back on either side of the guard (results only).
TILE_CASES = {
    "sR below": (lambda: [S, S, mu.tile_long_sR(2**31 - 1)], True),
    "sR at": (lambda: [S, S, mu.tile_long_sR(2**31)], False),
    "sQ below": (lambda: [S, S, mu.tile_long_sQ(2**31 - 1)], True),
    "sQ at": (lambda: [S, S, mu.tile_long_sQ(2**31)], False),
    "tot below": (lambda: mu.tile_long_total(2**32 - 1), True),
    "tot at": (lambda: mu.tile_long_total(2**32), False),
    "sR below, few ops": (lambda: [S, S, mu.tile_record_sR(2**31 - 1)], False),
    "sR at, few ops": (lambda: [S, S, mu.tile_record_sR(2**31)], False),
    "sQ below, few ops": (lambda: [S, S, mu.tile_record_sQ(2**31 - 1)], False),
    "sQ at, few ops": (lambda: [S, S, mu.tile_record_sQ(2**31)], False),
    "tot below, few ops": (lambda: mu.tile_total_records(2**32 - 1), False),
    "tot at, few ops": (lambda: mu.tile_total_records(2**32), False),
}


def tile_case(name):
    """(batch, window lists on its last record, whether the tile kernel keeps the tile)"""
    make, kept = TILE_CASES[name]
    b = mu.tile_batch(make())
    return b, mu.last_record_windows(b), kept


@pytest.mark.parametrize("name", list(TILE_CASES))
def test_tile_records_hold_what_they_are_built_for(oracle, name):
    b, wl, kept = tile_case(name)
    below, few = name.split()[1].startswith("below"), name.endswith("few ops")
    assert kept == (below and not few) and (mu.max_lane_sum(b) >= 2**25) == few
    n = len(b["t_st"])
    sR, sQ = [int(x) for x in b["t_en"] - b["t_st"]], [int(x) for x in b["q_en"] - b["q_st"]]
    n_ops = np.diff(b["op_off"].astype(np.int64))
    # one tile holds them all (rb_plan_tiles_host: consecutive records of 8 and more ops)
    sched, tiles, n_long, _ = cut(n_ops.astype(np.uint64))
    assert tiles.tolist() == [[0, n, 0]] and n_long == 0 and (n_ops >= 8).all()
    for r in range(n):
        assert mu.is_regular(mu.as_ops(b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])]))
    tot = sum(sR) + sum(sQ)
    kind = name.split()[0]
    if kind == "sR":  # (the tile's total stays below its own guard: the record's span decides)
        assert sR[-1] == (2**31 - 1 if below else 2**31) and max(sQ) < 1000 and max(sR[:-1]) < 100 and tot < 2**32
    elif kind == "sQ":
        assert sQ[-1] == (2**31 - 1 if below else 2**31) and max(sR) < 1000 and max(sQ[:-1]) < 100 and tot < 2**32
    else:
        assert tot == (2**32 - 1 if below else 2**32) and max(sR + sQ) < 2**31
        assert 2**31 - 10_000 < sum(sR[:-1]) < 2**31 and sum(sR) > 2**31 + 2**29  # the last record starts near 2^31 of the tile's reference total
    for i, w in enumerate(wl):
        assert (np.diff(w[1].astype(np.int64)) >= 0).all() and (np.diff(w[2].astype(np.int64)) >= 0).all()  # sorted, ends too
        assert (w[2] > b["t_st"][-1]).all() and (w[1] >= b["t_en"][-2]).all()                              # on the last record only
        n_ok, n_none = _same_rows(mu.liftover_regular(b, w), oracle.liftover_opspace(_obatch(oracle, b), *w, n_threads=2), f"{name}, windows {i}")
        assert n_ok + n_none == len(w[1]) and n_ok >= (len(w[1]) * 2 + 2) // 3  # (a window inside a long D or N holds no match base)
    for max_size in (100, 2**27):
        assert _same_rows(mu.break_paf_regular(b, max_size), oracle.break_opspace(_obatch(oracle, b), max_size, n_threads=2), f"{name}, break {max_size}",
                          flags=False)[0] >= n


def test_guard_pairs_hold_what_they_are_built_for():
    for total in (511, 512, 513):
        b, left, right = mu.guard_pairs(total)
        for l, r in zip(left, right):
            ql, qr = int(b["q_en"][l] - b["q_st"][l]), int(b["q_en"][r] - b["q_st"][r])
            ov = int(b["q_en"][l]) - int(b["q_st"][r])
            assert ql + qr == total and 0 < ov < min(ql, qr) and int(b["q_st"][l]) < int(b["q_st"][r])
            assert (2**20 * (ql + qr) >= 2**29) == (total >= 512) and 2**20 * ov < 2**31
        assert len({(chr(b["strand"][l]), chr(b["strand"][r])) for l, r in zip(left, right)}) == 4
    b, left, right = mu.wide_pair()
    ov = int(b["q_en"][0]) - int(b["q_st"][1])
    assert ov == 1500 and 2**30 < 2**20 * ov < 2**31


def test_the_oracle_takes_the_trim_file_at_every_shift(oracle):
    """the file of tests/test_gpu_magnitude.py's resident trim-paf: the reference cuts every group (exit 0) wherever the file lies, and what
    it prints moves with the file"""
    text = mu.trim_groups_text(7)
    assert text.count("\n") == 2000
    for pre in ([], ["--bsearch", "legacy"]):
        rc, base = oracle.cli(*pre, "trim-paf", "-", stdin=text.encode())
        assert rc == 0 and base.count(b"\n") == 2000
        for Kt, Kq in mu.SHIFTS:
            rc, out = oracle.cli(*pre, "trim-paf", "-", stdin=mu.shift_paf_text(text, Kt, Kq).encode())
            assert rc == 0 and out.decode() == mu.shift_paf_text(base.decode(), Kt, Kq)
