"""CPU twin of tests/test_gpu_text_seams.py: the inputs of tests/text_seam_util.py are what they claim to be.  The plain-Python reference
equals the oracle (rbo_parse_cigar, rbo_cigar_to_string) on every string and item the GPU file uses; every case lies where its name says
by the position model; every grid is complete; and no valid string of the families that assert "status 0, never 3" holds a run of ten
digits."""
import numpy as np
import pytest

import text_seam_util as tu
from test_gpu_text import oracle_format, oracle_parse

DIGITS = b"0123456789"


# ------------------------------------------------------------------------------------------------ the reference is the oracle's
@pytest.mark.parametrize("name", list(tu.PARSE_LAYOUTS))
def test_parse_reference_equals_the_oracle(oracle, name):
    for c in tu.layout(name).cases:
        want, got = oracle_parse(oracle, c.s), tu.ref_parse(c.s)[0]
        assert (want is None) == (got is None), (c.name, c.s[:40])
        if want is not None:
            assert np.array_equal(tu.ref_words(got), want), (c.name, c.s[:40])


@pytest.mark.parametrize("name", list(tu.FORMAT_SETS))
def test_format_reference_equals_the_oracle(oracle, name):
    F = tu.format_set(name)
    for i in range(F.n):
        seg = F.words(i).copy()
        fl, ll = F.clip(i)
        if len(seg) == 1 and fl and ll:
            seg[0] = ((fl + ll - (int(seg[0]) >> 4)) << 4) | (int(seg[0]) & 15)
        else:
            if len(seg) and fl:
                seg[0] = (fl << 4) | (int(seg[0]) & 15)
            if len(seg) and ll:
                seg[-1] = (ll << 4) | (int(seg[-1]) & 15)
        assert tu.ref_format(F.words(i), fl, ll) == oracle_format(oracle, seg), (name, i)


def test_runs_and_statuses_of_the_reference():
    assert tu.ref_parse(b"12=0003X7") == (None, [2, 4, 1])
    assert tu.ref_parse(b"") == ([], [])
    assert tu.ref_parse(b"0000000012=3X") == ([(12, 7), (3, 8)], [10, 1])
    assert tu.want_status(b"268435455M") == {0} and tu.want_status(b"268435456M") == {2} and tu.want_status(b"1Q") == {1, 3}
    assert tu.want_status(b"0000000012=") == {0, 3} and tu.want_status(b"4294967295=") == {3} and tu.want_status(b"4294967296=") == {1, 3}
    assert tu.place(35, 32) == (0, 0, 0) and tu.place(35, 32 + 1023) == (63, 0, 15) and tu.place(35, 32 + 1024 + 17) == (1, 1, 1)


@pytest.mark.parametrize("name", ["phases", "splits", "full-steps"] + [f"count-{n}" for n in tu.N_REC])
def test_never_three_holds_of_the_reference_alone(name):
    """every string of these families is valid but the one-byte strings of the phase grid, and none has a run of ten digits"""
    for c in tu.layout(name).cases:
        ops, runs = tu.ref_parse(c.s)
        assert max(runs, default=0) <= 9, c.name
        if name == "phases" and len(c.s) == 1:
            assert ops is None
        else:
            assert ops is not None and tu.want_status(c.s) == {0}, c.name


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("name", list(tu.PARSE_LAYOUTS))
def test_layouts_are_what_the_contract_asks(name):
    """strings in increasing order with a gap between them, the buffer ends at the next multiple of 16 behind the last string; the four
    fillings differ in the gaps only"""
    Lo = tu.layout(name)
    assert Lo.size % 16 == 0 and 0 <= Lo.size - Lo.cases[-1].b1 < 16 or Lo.size == 16
    bufs = [Lo.buffer(f) for f in tu.FILLS]
    inside = np.zeros(Lo.size, bool)
    prev = 0
    for c in Lo.cases:
        assert c.b0 >= prev + (tu.MIN_GAP if prev else 0)
        inside[c.b0:c.b1] = True
        prev = c.b1
        for b in bufs:
            assert b[c.b0:c.b1] == c.s
    a = [np.frombuffer(b, np.uint8) for b in bufs]
    assert (a[0][~inside] == ord("9")).all() and (a[1][~inside] == ord("M")).all() and (a[3][~inside] == 0xFF).all()
    for c in Lo.cases:
        assert bufs[2][c.b0 - 5:c.b0] == b"cg:Z:" and bufs[2][c.b1:c.b1 + 1] in (b"\t", b"")
    raw, off = Lo.back_to_back()
    assert len(raw) % 16 == 0 and len(raw) - int(off[-1]) < 16 and len(off) == len(Lo.cases) + 1
    for i, c in enumerate(Lo.cases):
        assert raw[int(off[i]):int(off[i + 1])] == c.s


def test_phase_grid_is_complete_and_hostile():
    Lo = tu.layout("phases")
    want = {(ph, n) for ph in range(16) for n in list(range(41)) + [1024 * k - ph + d for k in (1, 2) for d in (-1, 0, 1)]}
    assert {c.tag for c in Lo.cases} == want and len(Lo.cases) == len(want)
    nine, letter = Lo.buffer("nine"), Lo.buffer("letter")
    front, behind_digit, behind_letter, end_phase = [0] * 16, [0] * 16, [0] * 16, set()
    for c in Lo.cases:
        assert c.b0 & 15 == c.tag[0] and len(c.s) == c.tag[1]
        front[c.b0 & 15] += nine[c.b0 - 1:c.b0] in (b"9",)
        behind_digit[c.b1 & 15] += c.b1 < Lo.size and nine[c.b1:c.b1 + 1] == b"9"
        behind_letter[c.b1 & 15] += c.b1 < Lo.size and letter[c.b1:c.b1 + 1] == b"M"
        end_phase.add((c.b0 & 15, c.b1 & 15))
        if len(c.s) > 1:
            assert c.s[0] in DIGITS and c.s[-1] in tu.OPCH    # a digit in front joins the first number, a digit behind starts a new one
    assert min(front) >= 47 and min(behind_digit) >= 40 and min(behind_letter) >= 40
    assert end_phase == {(a, b) for a in range(16) for b in range(16)}
    # the ends on and next to a step boundary; a string wholly inside one chunk with bytes masked on both sides
    for ph in range(16):
        ends = {tu.place(c.b0, c.b1 - 1)[:2] + (tu.place(c.b0, c.b1 - 1)[2],) for c in Lo.cases if c.tag[0] == ph and c.tag[1] > 1000}
        assert {(63, 0, 14), (63, 0, 15), (0, 1, 0), (63, 1, 14), (63, 1, 15), (0, 2, 0)} <= ends
    assert any(0 < (c.b0 & 15) and len(c.s) > 0 and (c.b0 & 15) + len(c.s) < 16 for c in Lo.cases)


@pytest.mark.parametrize("name,values", [("splits", tu.SPLIT_VALUES), ("splits-2^28", ["268435456"])])
def test_every_split_of_every_number_is_there(name, values):
    Lo = tu.layout(name)
    want = {(v, k, b, ph) for v in values for k in range(1, len(v) + 1) for b in tu.SPLIT_BOUNDS for ph in tu.SPLIT_PHASES}
    assert {c.tag[:4] for c in Lo.cases} == want and len(Lo.cases) == len(want)
    assert {len(v.lstrip("0")) for v in values} >= ({9} if name != "splits" else set(range(1, 10)))
    for c in Lo.cases:
        v, k, bound, ph, at, B = c.tag
        assert c.b0 & 15 == ph and c.s[at:at + len(v)] == v.encode() and c.s[at + len(v)] in tu.OPCH
        assert at == 0 or c.s[at - 1] in tu.OPCH
        # the filler in front: one-digit ops (one op of two digits where the number starts on an odd byte)
        ops = tu.ref_parse(c.s[:at])[0]
        assert ops is not None and sum(ln > 9 for ln, _ in ops) <= 1
        last_before, first_after = tu.place(c.b0, c.b0 + at + k - 1), tu.place(c.b0, c.b0 + at + k)
        step = {"lane": 0, "step1": 1, "step2": 2}[bound]
        assert first_after[1:] == (step, 0) and last_before[2] == 15
        if bound == "lane":
            assert last_before[1] == 0 and first_after[0] == last_before[0] + 1 and B % 1024
        else:
            assert last_before[:2] == (63, step - 1) and first_after[0] == 0
        assert tu.place(c.b0, c.b0 + at)[2] == 16 - k           # k digits in front of the boundary, the rest (or the op character) behind
        if name == "splits":
            assert tu.want_status(c.s) == {0}
        else:
            assert tu.want_status(c.s) == {2}


def test_full_steps_fill_every_lane():
    Lo = tu.layout("full-steps")
    assert {c.tag for c in Lo.cases} == {(ph, n) for ph in (0, 1, 8, 15) for n in tu.FULL_N}
    seen = set()
    for c in Lo.cases:
        per = tu.ops_per_step(c)
        assert sum(per) == c.tag[1] == len(tu.ref_parse(c.s)[0])
        seen |= {(c.b0 & 1, k) for k in per}
        # an op is two bytes: a step of 1 KiB holds 512 at most, the 513th is the first of the next step
        assert max(per) <= 512
        if c.tag == (0, 1537):
            assert per == [512, 512, 512, 1]
        if c.tag == (1, 1537):
            assert per == [511, 512, 512, 2]                    # the op character in the other byte of its pair
        if c.tag == (0, 513):
            assert per == [512, 1]
        if c.tag == (0, 511):
            assert per == [511]
    assert {(0, 511), (0, 512), (1, 511), (1, 512), (0, 1), (1, 2)} <= seen


def test_all_byte_values_on_both_bytes_of_a_pair():
    Lo = tu.layout("bytes")
    assert {c.tag[:3] for c in Lo.cases} == {(b, t, par) for b in range(256) for t in range(4) for par in (0, 1)} and len(Lo.cases) == 2048
    accepted = set()
    for c in Lo.cases:
        b, t, par, pos = c.tag
        assert c.s[pos] == b and (c.b0 + pos) & 1 == par and len(c.s) == (2, 3, 4, 6)[t]
        if tu.ref_parse(c.s)[0] is not None:
            accepted.add((b, t))
    # the byte is an op character where one belongs and a digit where one belongs
    assert accepted == {(b, 0) for b in tu.OPCH} | {(b, 1) for b in DIGITS} | {(b, 2) for b in DIGITS} | {(b, 3) for b in tu.OPCH} | {(b, 3) for b in DIGITS}
    assert {c.b0 & 15 for c in Lo.cases} == set(range(16))


def test_status_cases_lie_where_their_names_say():
    Lo = tu.layout("status")
    by = {c.name: c for c in Lo.cases if c.name != "good"}
    for i, c in enumerate(Lo.cases):                                # a good record on both sides of every case
        assert (c.name == "good") == (i % 2 == 0) and (c.name != "good" or tu.want_status(c.s) == {0})
    assert Lo.cases[-1].name == "good"

    def at(name, k):
        c = by[name]
        return tu.place(c.b0, c.b0 + k)

    for name, step in (("MM-lane", 0), ("MM-lane-ph15", 0), ("MM-step", 1)):
        k = by[name].s.index(b"MM")
        assert at(name, k)[2] == 15 and at(name, k + 1)[1:] == (step, 0) and at(name, k)[1] == max(step - 1, 0)
    assert at("M-byte0", 0) == (0, 0, 0) and at("M-byte15", 0) == (0, 0, 15)
    for name, step in (("tail-digits", 0), ("tail-digits-step", 1)):
        c = by[name]
        k = len(c.s) - 3
        assert c.s[k - 2:] == b"12345" and at(name, k - 1)[2] == 15 and at(name, k)[1:] == (step, 0) and tu.ref_parse(c.s)[0] is None
    for name, c in by.items():
        if not name.startswith("run"):
            continue
        nd, where = int(name[3:].split("-")[0]), name.split("-")[2]
        ops, runs = tu.ref_parse(c.s)
        assert ops is not None and max(runs) == nd
        k = max(i for i in range(len(c.s)) if c.s[i:i + nd].isdigit())  # where the run starts
        a, b = at(name, k), at(name, k + nd - 1)
        assert {"inside": a[:2] == b[:2], "lanes": a[1] == b[1] and b[0] == a[0] + 1, "step": (a[1], b[1]) == (0, 1), "step2": (a[1], b[1]) == (1, 2)}[where], name
        assert tu.want_status(c.s) == ({0} if nd == 9 else {0, 3})
    assert {c.pin for c in by.values()} == {None, 1, 2, 3}
    for name in ("bad+long", "bad+long-lanes"):
        assert tu.ref_parse(by[name].s) == (None, tu.ref_parse(by[name].s)[1]) and max(tu.ref_parse(by[name].s)[1]) == 9 and b"268435456" in by[name].s
    for name in ("long", "long-last", "long-u32max-9digits"):
        assert tu.want_status(by[name].s) == {2}
    for name in ("ten+bad", "ten+bad-lanes", "ten+long", "ten+long+bad", "ten-u32", "ten-past-u32"):
        assert max(tu.ref_parse(by[name].s)[1]) >= 10 and 3 in tu.want_status(by[name].s)


def test_record_counts():
    for n in tu.N_REC:
        Lo = tu.layout(f"count-{n}")
        assert len(Lo.cases) == n and {len(tu.ref_parse(c.s)[0]) for c in Lo.cases} <= {1, 2, 3}
    assert set(tu.N_REC) == {1, 3, 4, 5, 2047, 2048, 2049, 4097}


# ------------------------------------------------------------------------------------------------ format
def test_format_phase_grid_is_complete_with_every_store_shape():
    F = tu.format_set("phase-x-bytes")
    off, text = F.expected()
    got, shapes = set(), set()
    for i in range(F.n):
        n_ops, nb = int(F.count[i]), int(off[i + 1] - off[i])
        assert 1 <= n_ops <= 12 and all(1 <= (int(w) >> 4) <= 9999 for w in F.words(i))
        if F.tags[i] is None:
            continue
        ph, want = F.tags[i]
        assert (int(off[i]) & 15, nb) == (ph, want)
        got.add((ph, nb))
        shapes.add(tu.store_shape(ph, nb))
    assert got == {(ph, nb) for ph in range(16) for nb in range(2, 49)}
    assert {s for s, _ in shapes} == {"bytes", "head", "tail", "both", "whole"} and ("whole", 1) in shapes
    assert {("head", 1), ("tail", 1), ("both", 1), ("both", 2), ("whole", 3)} <= shapes
    assert tu.store_shape(0, 16) == ("whole", 1) and tu.store_shape(1, 30) == ("bytes", 0) and tu.store_shape(15, 2) == ("bytes", 0)


def test_format_seam_items_and_their_steps():
    F = tu.format_set("255-seam")
    assert F.tags == [(n, m) for n in tu.F2_COUNTS for m in tu.F2_MODES]
    assert [tu.format_steps(n) for n in (255, 256, 257, 512)] == [[(0, 255)], [(0, 256)], [(0, 255), (255, 2)], [(0, 255), (255, 255), (510, 2)]]
    last_words, off = set(), F.expected()[0]
    for i, (n, mode) in enumerate(F.tags):
        fl, ll = F.clip(i)
        assert (fl != 0, ll != 0) == {"first": (1, 0), "last": (0, 1), "both": (1, 1), "neither": (0, 0)}[mode]
        steps = tu.format_steps(n)
        assert sum(k for _, k in steps) == n
        last_words.add(steps[-1][1])                              # the step in which last_len applies: the last one; it prints this many words
        # where every step starts in the text: consecutive steps at different phases
        w = F.words(i)
        phases = [(int(off[i]) + len(tu.ref_format(w[:i0], fl, 0))) & 15 for i0, _ in steps]
        assert all(a != b for a, b in zip(phases, phases[1:])), (n, mode, phases)
        # first_len and last_len change the number of digits of their op
        assert all(1 <= (int(x) >> 4) <= 998 for x in w) and (not fl or fl > 999) and (not ll or ll > 9999)
    assert last_words == {1, 2, 4, 5, 254, 255, 256} and {len(tu.format_steps(n)) for n in tu.F2_COUNTS} == {1, 2, 3}


def test_two_arrays_differ_everywhere():
    F = tu.format_set("two-arrays")
    assert len(F.ops) == len(F.alt) and ((F.ops >> 4) != (F.alt >> 4)).all() and ((F.ops & 15) != (F.alt & 15)).all()
    assert {tuple(F.tags[4 * b:4 * b + 4]) for b in range(F.n // 4)} == {tuple((p >> j) & 1 for j in range(4)) for p in range(16)}
    for i in range(F.n):
        assert (int(F.first[i]) >> 63) == F.tags[i] and tu.ref_format(F.words(i)) != tu.ref_format(F.other_words(i))
    assert max(F.count) > 256 and min(F.count) == 1


def test_continuation_pairs_sit_at_the_seams():
    F = tu.format_set("continuation")
    assert len(F.ops) == len(F.alt)
    pairs = set()
    for i, (n, at, v, use_alt) in enumerate(F.tags):
        w = F.words(i)
        assert len(w) == n and (int(F.first[i]) >> 63) == use_alt and not ((F.other_words(i) & 15) == tu.CONT).any()
        if at is None:                                            # the continuation word behind the item is not the item's
            f = int(F.first[i]) & ((1 << 63) - 1)
            src = F.alt if use_alt else F.ops
            assert int(src[f + n]) & 15 == tu.CONT and not ((w & 15) == tu.CONT).any()
            assert tu.ref_format(w).endswith(b"%d%c" % (int(w[-1]) >> 4, tu.OPCH[int(w[-1]) & 15]))
            pairs.add((n, None, 0, use_alt))
            continue
        assert list(np.flatnonzero((w & 15) == tu.CONT)) == [at + 1] and str(v).encode() in tu.ref_format(w)
        assert (int(w[at]) >> 4) + ((int(w[at + 1]) >> 4) << 28) == v
        pairs.add((n, at, v, use_alt))
    assert pairs == set(F.tags)
    where = {(n, at) for n, at, _, _ in F.tags if at is not None}
    assert {(300, 3), (300, 254), (300, 255), (300, 256)} <= where and (2, 0) in where and any(at == n - 2 and n > 2 for n, at in where)
    assert {v for _, at, v, _ in F.tags if at is not None} == {1 << 28, 999999999, 1000000000, 4294967295}
    assert {n for n, at, _, _ in F.tags if at is None} >= {1, 4, 255, 256}


def test_every_digit_pattern_is_there():
    F = tu.format_set("digits")
    lens = np.concatenate([F.words(i) for i in range(F.n - 1)]) >> 4
    have = set(lens.tolist())
    assert set(range(1, 100000)) <= have and len(F.ops) == sum(F.count)
    assert all(k * 10000 in have and min(k * 10000 + 9999, (1 << 28) - 1) in have for k in range(1, 26844))
    assert {int(x) // 10000 for x in have} == set(range(26844)) and max(have) == (1 << 28) - 1
    tens = F.words(F.n - 1)
    assert len(tens) == 40 and [(int(a) >> 4) + ((int(b) >> 4) << 28) for a, b in zip(tens[::2], tens[1::2])] == list(tu.TEN_DIGITS)
    assert all(10 ** 9 <= t < 1 << 32 for t in tu.TEN_DIGITS) and len(set(tu.TEN_DIGITS)) == 20
    assert tu.ref_format(tens) == b"".join(b"%d%c" % (t, tu.OPCH[i % 9]) for i, t in enumerate(tu.TEN_DIGITS))
