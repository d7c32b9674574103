"""The inputs of tests/test_gpu_scan_rows.py hold what they are meant to hold, and the flag reference says what the header says.

No GPU: the routing rule and the geometry of the row form (include/rustybam_amd.h, rb_ctx_scan_route) are
recomputed here from the generated arrays, so a change to the generator that loses a case fails this file, and the plain-numpy
reference of rb_reduce_row.flags / rb_norm_row.flags (tests/scan_util.py) is pinned on hand-written records."""
import numpy as np
import pytest

import scan_util as su
from rbtest_util import CONT, batch_args, pack


@pytest.fixture(scope="module")
def gen():
    return su.batches(0)


def _n(b):
    return np.diff(b["op_off"].astype(np.int64))


def _rec(b, r):
    return b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])]


def _where(b, **kv):
    return [r for r, t in enumerate(b["tags"]) if all(t.get(k) == v for k, v in kv.items())]


# ------------------------------------------------------------------------------------------------ the flag reference
REG, STR, HASM = su.F_REGULAR, su.F_STRIPPED, su.F_HAS_M
HAND = [  # (cigar words, reduce flags, norm flags where the norm row is OK)
    ("5=1X3=", REG, REG),
    ("4M2I3M", REG | HASM, REG | HASM),
    ("2I5=3D", REG, REG | STR),                                    # regular as loaded, stripped, the kept range is 5=
    ("2I3N5=", REG, STR),                                          # the kept range begins on N: not for the streaming kernels
    ("5=2N3=", REG, REG),
    ("5=3=", 0, 0),                                                # equal neighbours
    ("5=0X3=", 0, 0),                                              # a zero length
    ("3S5=", 0, 0), ("5=2H", 0, 0), ("5=1P3=", 0, 0),
    ("0M5=", 0, 0),                                                # an M of no bases: bamstats.rs:145 asks matches > 0
    ("5=300000000X2=", 0, 0),                                      # a continuation word
    ("4294967290=5X", 0, 0),                                       # (one long op: a continuation word again)
    ("268435455=268435455X" * 8 + "15=", REG, REG),                # 2^32 - 1 units in single words ...
    ("268435455=268435455X" * 8 + "16=", 0, 0),                    # ... and 2^32
    ("2I3D", REG, None), ("", REG, None),                          # no norm row to speak of (paf.rs:757, :663)
]


def test_flag_reference_on_hand_written_records():
    assert pack("4294967290=5X").tolist() == [((4294967290 & 0x0FFFFFFF) << 4) | 7, (15 << 4) | CONT, (5 << 4) | 8]
    for text, red, norm in HAND:
        got = su.flags_of(pack(text))
        assert got[0] == red and (norm is None or got[1] == norm), (text[:40], got, (red, norm))
    # raw words no text can spell: codes above 8, a continuation word in front
    w = pack("5=1X3=")
    for code in su.UNKNOWN_CODES:
        v = w.copy()
        v[1] = (1 << 4) | code
        assert su.flags_of(v) == (0, 0) and su.sums(v) == dict(R=8, Q=8, M=8, U=9, m_len=0)
    v = np.concatenate([[(3 << 4) | CONT], w]).astype(np.uint32)
    assert su.flags_of(v) == (0, 0) and su.sums(v)["U"] == 12 and su.sums(v)["R"] == 9
    v = np.concatenate([pack("2M"), [(9 << 4) | CONT], pack("1X")]).astype(np.uint32)
    assert su.sums(v) == dict(R=(9 << 28) + 3, Q=(9 << 28) + 3, M=(9 << 28) + 3, U=(9 << 28) + 3, m_len=(9 << 28) + 2)
    assert su.flags_of(v) == (HASM, HASM) and su.end_runs(np.concatenate([pack("2D"), [(1 << 4) | CONT], pack("1X1I")])) == (2, 1)


def test_batch_reference_equals_the_per_record_one(gen, oracle):
    """flags_ref (vectorised) = flags_of record by record, and the generator's own sums and end runs are the oracle's"""
    for name, b in gen.items():
        red, norm = su.flags_ref(b)
        s = su.batch_sums(b["ops"], b["op_off"])
        ob = oracle.Batch(*batch_args(b), b["contig"])
        ored, onorm = oracle.reduce(ob), oracle.normalize(ob)
        for k, f in (("R", "t_bases"), ("Q", "q_bases")):
            assert np.array_equal(s[k].astype(np.uint64), ored[f]), (name, k)
        assert np.array_equal((s["U"] & 0xFFFFFFFF).astype(np.uint32), ored["aln_len"]), name
        live = onorm["status"] != oracle.PANIC_EMPTY_CIGAR
        assert np.array_equal(s["lead"][live], onorm["lead_ops"][live]) and np.array_equal(s["trail"][live], onorm["trail_ops"][live]), name
        assert np.array_equal(ored["status"] == oracle.PANIC_OVERFLOW, s["U"] > su.U32_MAX), name
        for r in range(len(red)):
            w = _rec(b, r)
            one = su.flags_of(w)
            assert red[r] == one[0], (name, r)
            if onorm["status"][r] == 0:
                assert norm[r] == one[1], (name, r)
            assert su.sums(w)["U"] == s["U"][r] and su.end_runs(w) == (s["lead"][r], s["trail"][r]) or len(w) == 0, (name, r)


# ------------------------------------------------------------------------------------------------ the geometry
def test_every_batch_takes_the_route_it_is_for(gen):
    wave = {"route_63_records", "route_mean_1537"}
    assert tuple(gen) == su.BATCH_NAMES and set(su.WAVE_BATCHES) == wave
    for name, b in gen.items():
        took, listed = su.route(b["op_off"])
        assert (took + listed == 0) == (name in wave), name
    n = _n(gen["route_63_records"])
    assert len(n) == 63 and len(_n(gen["route_64_records"])) == 64 and n.sum() // 63 <= su.ROWS_MEAN_MAX
    for name, total, q in (("route_mean_1536", 1536 * 64, 1536), ("route_mean_1536_63", 1536 * 64 + 63, 1536), ("route_mean_1537", 1537 * 64, 1537)):
        n = _n(gen[name])
        assert len(n) == 64 and n.sum() == total and total // 64 == q and n.max() <= su.ROW_MAX_OPS and n.min() >= su.ROW_MIN_OPS
    assert su.route(gen["route_mean_1536_63"]["op_off"]) == (64, 0)


@pytest.mark.parametrize("mode", ["regular", "wild"])
def test_boundary_lengths_at_every_phase(gen, mode):
    b = gen["lengths_" + mode]
    n, off = _n(b), b["op_off"].astype(np.int64)
    want = {0, 1, 2, 3, 4, 5, 15, 16, 17} | {c + d for c in (64, 128, 256, 1024, 2048) for d in range(-4, 5)}
    seen = {(int(n[r]), int(off[r]) % 4) for r in range(len(n))}
    for length in want:
        for phase in range(4):
            assert (length, phase) in seen, (length, phase)
    assert ((n > 5900) & (n < 6100)).sum() == 1
    took, listed = su.route(b["op_off"])
    assert listed == 4 * (4 + 4) + 1 and took > 0                 # lengths 0..3 and 2049..2052 at four phases, the long one
    # the head decides whether n + head crosses a multiple of 64: both happen for the lengths around a step's end
    steps = {(int(n[r]), (int(n[r]) + int(off[r]) % 4 + 63) // 64) for r in range(len(n))}
    for length in (62, 63, 64, 126, 254, 255, 256, 1022, 2046):
        assert len({s for (m, s) in steps if m == length}) == 2, length
    if mode == "regular":
        red, _ = su.flags_ref(b)
        assert (red & REG).all()


def test_wavefronts_of_mixed_fate(gen):
    b = gen["fate"]
    n = _n(b)
    assert len(n) % 4 == 1 and len(n) % 16 not in (0,) and len(n) >= su.ROWS_MIN_REC          # the last wavefront has one live row
    quads = {tuple(int(x) for x in n[r:r + 4]) for r in range(0, len(n) - 3, 4)}
    assert (2048, 4, 3, 2049) in quads
    taken = lambda q: sum(su.ROW_MIN_OPS <= x <= su.ROW_MAX_OPS for x in q)  # noqa: E731
    assert {taken(q) for q in quads} >= {0, 1, 2, 4}
    assert su.route(b["op_off"])[1] == int(((n < 4) | (n > 2048)).sum()) >= 10


def test_one_defect_records(gen):
    seen_unknown, seen_cont = set(), set()
    for name, n_words in (("defects_5", 5), ("defects_300", 300), ("defects_2048", 2048)):
        b = gen[name]
        n, off = _n(b), b["op_off"].astype(np.int64)
        red, norm = su.flags_ref(b)
        got = set()
        for r in _where(b, kind="clean"):
            assert n[r] == n_words and su.defects(_rec(b, r)) == [] and int(red[r]) & ~HASM == REG and int(norm[r]) & ~HASM == REG
        for r in _where(b, kind="defect"):
            t, w = b["tags"][r], _rec(b, r)
            d = su.defects(w)
            assert len(w) == n_words and len(d) == 1, (name, r, d)
            head = int(off[r]) % 4
            assert head == t["head"] and not (red[r] & REG) and not (norm[r] & REG)
            at, what = d[0]
            if what == "same" and t["at"] == 0:
                at = 0                                             # (an equal pair is reported at its second word)
            assert at == t["at"] and what == t["what"], (name, r, d, t)
            got.add((head, at, what))
            if what == "unknown":
                seen_unknown.add(int(w[at]) & 15)
            if what == "cont":
                seen_cont.add((int(w[at]) >> 4, at == 0))
            # everything but the defect is the clean record
            clean = su.base3_words(n_words)
            assert (w != clean).sum() == 1
        for head in range(4):
            want = {0, n_words - 1} | ({su.STEP - head} if n_words > 64 else set())
            if name != "defects_2048":
                want = {i for i in (0, 3, 4, 63 - head, 64 - head, 255, 256, n_words - 2, n_words - 1) if 0 <= i < n_words}
            for at in want:
                for what in su.DEFECTS:
                    assert (head, at, what) in got, (name, head, at, what)
        assert su.route(b["op_off"])[0] >= len(got)                # the row form takes them all
    assert seen_unknown == {9, 10, 11, 12, 13, 15}
    assert {v for v, _ in seen_cont} >= {1, 8, 9, 15} and {f for _, f in seen_cont} == {True, False}


def test_clean_records_between_hostile_neighbours(gen):
    b = gen["hostile"]
    off = b["op_off"].astype(np.int64)
    red, norm = su.flags_ref(b)
    seen = set()
    for r in _where(b, kind="hostile_mid"):
        t, w, before, after = b["tags"][r], _rec(b, r), _rec(b, r - 1), _rec(b, r + 1)
        assert b["tags"][r - 1]["kind"] == "hostile_before" and b["tags"][r + 1]["kind"] == "hostile_after"
        head, tail = int(off[r]) % 4, int(off[r + 1]) % 4
        assert head != 0 and tail != 0                            # shares its first and its last 16-byte group
        assert min(len(before), len(after)) >= 4 and int(red[r]) & ~HASM == REG and int(norm[r]) & ~HASM == REG
        pb, na = int(before[-1]), int(after[0])
        if t["what"] == "same":
            assert pb & 15 == int(w[0]) & 15 and na & 15 == int(w[-1]) & 15 and red[r - 1] & REG and red[r + 1] & REG
        elif t["what"] == "zero":
            assert pb >> 4 == 0 and na >> 4 == 0
        else:
            assert pb & 15 not in su.REGULAR_CODES and na & 15 not in su.REGULAR_CODES
        seen.add((head, tail, t["what"]))
    assert {h for h, _, _ in seen} == {1, 2, 3} and {t for _, t, _ in seen} == {1, 2, 3} and {w for _, _, w in seen} == set(su.HOSTILE)
    assert su.route(b["op_off"])[1] == 0


def test_magnitudes(gen, oracle):
    b = gen["magnitude"]
    n, off = _n(b), b["op_off"].astype(np.int64)
    s = su.batch_sums(b["ops"], b["op_off"])
    ob = oracle.Batch(*batch_args(b), b["contig"])
    ored, onorm = oracle.reduce(ob), oracle.normalize(ob)
    one = lambda kind: _where(b, kind=kind)[0]  # noqa: E731
    r = one("overflow_2048")
    assert n[r] == 2048 and s["U"][r] == 2048 * ((1 << 28) - 1) and ored["status"][r] == oracle.PANIC_OVERFLOW
    w = _rec(b, r).astype(np.int64)
    assert ((w & 15) == np.array([7, 8] * 1024)).all() and (w[::2] >> 4).sum() >> 38 == 0 and (w[::2] >> 4).sum() >> 37 == 1
    assert ored["t_bases"][r] == s["U"][r]
    assert s["U"][one("total_u32_max")] == 2**32 - 1 and ored["status"][one("total_u32_max")] == 0
    assert s["U"][one("total_2_32")] == 2**32 and ored["status"][one("total_2_32")] == oracle.PANIC_OVERFLOW
    r = one("events_all_indel")
    assert n[r] == 2048 and ored["ins_events"][r] == 1024 and ored["del_events"][r] == 1024 and onorm["status"][r] == oracle.PANIC_ALL_INDEL
    r = one("events_1023")
    assert n[r] == 2048 and ored["ins_events"][r] == 1023 and onorm["status"][r] == 0
    heads = set()
    for r in _where(b, kind="cont_boundaries"):
        head, w = int(off[r]) % 4, _rec(b, r)
        at = {int(i) for i in np.flatnonzero((w & 15) == CONT)}
        assert {(i + head) % 4 for i in at} >= {0} and {4 - head if head else 4, 64 - head, 128 - head, 256 - head} <= at
        assert max(int(x) >> 4 for x in w[sorted(at)]) >= 8 and ored["status"][r] == 0 and s["U"][r] > 2**31
        heads.add(head)
    assert heads == {0, 1, 2, 3}
    assert ored["status"][one("cont_3e9")] == 0 and n[one("cont_3e9")] >= 4
    st = {b["tags"][r]["how"]: (int(ored["status"][r]), int(onorm["status"][r])) for r in _where(b, kind="broken")}
    assert st == {"t_en+1": (18, 18), "q_en+2": (19, 19), "t_inverted": (18, 18), "q_inverted": (19, 19)}
    for r in _where(b, kind="all_indel"):
        assert n[r] >= 4 and onorm["status"][r] == oracle.PANIC_ALL_INDEL
    quirks = _where(b, kind="quirk")
    assert all(n[r] >= 4 for r in quirks) and {chr(b["strand"][r]) for r in quirks} == {"+", "-"}
    assert {b["tags"][r]["text"] for r in quirks} >= {"2D1I5=3X4=", "5=1X3=2D1I2D"}
    assert len({int(onorm["status"][r]) for r in quirks}) >= 2    # the quirks of paf.rs:673, :690-701 break some of them, not all
    took, listed = su.route(b["op_off"])
    assert took >= len(n) - 5 and took + listed == len(n)


def test_the_whole_set_stays_small(gen):
    assert sum(int(b["op_off"][-1]) for b in gen.values()) < 3_000_000
