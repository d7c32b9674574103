"""The cases of tests/test_gpu_big_offsets.py hold what they claim (no GPU): every placement puts 2^32 where its class says, from the
payload's own offsets; placing a payload is a bijection for the models; a decoy answers differently for every item that can tell; the
periodic output cases have the period, the size and the byte at 2^32 they are meant to have."""
import numpy as np
import pytest

import rustybam_amd
import bam_rec_util as B
import big_offset_util as G
import nftext_util as nu
import text_seam_util as tu

B32 = G.B32


@pytest.fixture(scope="module")
def shapes():
    return dict(md=rustybam_amd.md_shape(), bam=rustybam_amd.bam_shape())


ALL = [(k, pid) for k in ("parse", "md", "bam") for pid in G.IDS[k]]


@pytest.mark.parametrize("kind,pid", ALL, ids=[f"{k}-{p}" for k, p in ALL])
def test_placement_puts_2_to_the_32_where_it_says(shapes, kind, pid):
    pl = G.placement(kind, pid, shapes)
    p, K, P = pl.p, pl.K, len(pl.p.data)
    assert 0 <= K and K + P + 64 <= G.BUF_BYTES                     # the payload, and the group behind it, inside the buffer
    if K >= B32:
        assert K - B32 + len(p.decoy().data) + P + 64 <= K          # the decoy well in front of the payload
    lo, hi = (None, None) if pl.lo is None else (K + pl.lo, K + pl.hi)
    if pl.cls == "a":
        assert lo < B32 < hi
        if kind == "parse":
            assert tu.place(pl.lo, pl.hi - 1)[1] == 0              # one step: the string ends inside its first KiB
        elif kind == "md":
            assert hi - lo <= shapes["md"][1]
        elif pid == "a-fixed":
            assert hi - lo == 32 and lo == K + int(p.off[pl.item])
        elif pid.startswith("a-aux"):
            an, R = pl.anatomy, int(p.off[pl.item])
            assert an["aux"][1] - an["aux"][0] <= shapes["bam"][1] and hi - lo == 8
            head = bytes(p.data[pl.lo:pl.hi])
            assert head[:4] == b"YIBI" and int.from_bytes(head[4:], "little") == 3
            assert {"a-aux-tag": B32 - lo == 1, "a-aux-type": B32 - lo == 2, "a-aux-count": 4 < B32 - lo < 8}[pid]
        elif pid == "a-z-value":
            m = B.model(p.data, p.off, p.rec_len)
            assert m["has_md"][pl.item] and (int(m["md_off"][pl.item]), int(m["md_end"][pl.item])) == (pl.lo, pl.hi) and hi - lo == 255
            assert pl.anatomy["aux"][1] - pl.anatomy["aux"][0] <= shapes["bam"][1]
        else:
            assert pid == "a-cigar" and (hi - lo) // 4 == 65 <= shapes["bam"][4] and (B32 - lo) % 4 == 2
    elif pl.cls == "b":
        assert lo < B32 < hi
        first_end, last_start = K + pl.steps[0], K + pl.steps[1]
        assert first_end <= B32 < last_start                          # beyond the first step, in front of the last
        if kind == "parse":
            steps = tu.place(pl.lo, pl.hi - 1)[1] + 1
            assert steps >= 3 and 0 < tu.place(pl.lo, pl.x)[1] < steps - 1 and tu.place(pl.lo, pl.x)[1] == tu.place(pl.lo, pl.x - 1)[1]
        elif kind == "md":
            assert hi - lo > shapes["md"][1]
        elif pid == "b-aux-wave":
            assert hi - lo > shapes["bam"][1] and (pl.lo, pl.hi) == tuple(int(p.off[pl.item]) + v for v in pl.anatomy["aux"])
        else:
            m = B.model(p.data, p.off, p.rec_len)
            assert int(m["op_off"][pl.item + 1] - m["op_off"][pl.item]) == 70000 == (hi - lo) // 4 > shapes["bam"][4]
            assert B.source_of(p.data, p.off, p.rec_len, m)[pl.item] == pl.lo
    elif pl.cls == "c":
        assert lo == B32 and hi > lo and (lo, hi) == (K + int(p.off[pl.item]), K + int(p.end[pl.item]))
    elif pl.cls == "d":
        assert hi == B32 and pl.item == p.n - 1 and K + int(p.end.max()) == B32 and hi > lo
    elif pl.cls[0] == "e":
        assert K == G.K_ABOVE[int(pl.cls[1])] and K >= B32
    else:
        assert pl.cls == "f" and K == B32 - P // 2
        below, above = (p.end + np.uint64(K) <= B32), (p.off + np.uint64(K) >= B32)
        assert K < B32 < K + P and (p.n < 3 or (below.any() and above.any()))   # (one string alone: the buffer around it spans 2^32)
        if p.n >= 8:                                                    # the four records of one wavefront on both sides
            i = int(np.nonzero(~below)[0][0])                           # the first item that reaches 2^32 or lies behind it
            quad = slice(i - i % 4, i - i % 4 + 4)
            across = ~below[quad] & ~above[quad]
            assert (below[quad].any() or across.any()) and (above[quad].any() or across.any()) or i % 4 == 0
            if i % 4 == 0 and not across.any():                          # (2^32 between two wavefronts: the one behind starts on it)
                assert int(p.off[i]) + K >= B32
    assert sorted(G.K_ABOVE) == [B32, B32 + 1, B32 + (1 << 20) + 7]


def test_every_class_is_there_for_every_entry_point():
    for kind in ("parse", "md", "bam"):
        classes = {c for _, _, c in G.PLACEMENTS[kind]}
        assert classes == {"a", "b", "c", "d", "e0", "e1", "e2", "f"}, kind
    assert {x[0] for x in G.BAM_PLACEMENTS if x[2] == "a"} == {"a-fixed", "a-aux-tag", "a-aux-type", "a-aux-count", "a-z-value", "a-cigar"}
    assert {x[0] for x in G.BAM_PLACEMENTS if x[2] == "b"} == {"b-aux-wave", "b-cg-70000"}
    assert {x[1] for x in G.PARSE_PLACEMENTS if x[2] == "f"} == set(tu.PARSE_LAYOUTS)
    assert {x[1] for x in G.BAM_PLACEMENTS if x[2] == "f"} == {"gather", "aux", "cg", "status", "fields", "mixed"}


PAYLOADS = sorted({(k, x[1]) for k in ("parse", "md", "bam") for x in G.PLACEMENTS[k]})


def _same(a, b):
    if isinstance(a, dict):
        return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
    return a == b


@pytest.mark.parametrize("kind,name", PAYLOADS, ids=[f"{k}-{n}" for k, n in PAYLOADS])
def test_placing_is_a_bijection_and_the_decoy_differs(shapes, kind, name):
    """the model of the payload's bytes at K = 4096 + 7 of a bytes object, asked at the moved offsets, is the moved model; and with its
    offsets applied to the decoy every item answers differently, those apart whose answer is a refusal or that read nothing"""
    p = G.payload(kind, name, shapes)
    K = G.K_SMALL
    placed = bytes([G.FILL]) * K + p.data + bytes([G.FILL]) * 64
    want, got = G.model(p, K), G.model(p, K, data=placed)
    if kind == "parse":
        assert got["refs"] == want["refs"] and all(w <= g for w, g in zip(want["allowed"], got["allowed"]))
    else:
        assert _same(want, got)
    if kind == "bam":                                                   # only offsets INTO the buffer move
        m0 = G.model(p, 0)
        has = m0["has_md"] != 0
        assert (has.any() or name == "gather") and np.array_equal(want["md_off"][has], m0["md_off"][has] + np.uint64(K)) and not want["md_off"][~has].any()
        for k in ("tid", "pos", "flag", "l_seq", "has_md", "status", "op_off", "ops"):
            assert np.array_equal(want[k], m0[k]), k
    d = p.decoy()
    assert d.n == p.n and sorted(d.labels) == sorted(p.labels)
    if p.n > 1:
        assert d.labels == p.labels[G.DECOY_ROT.get((kind, name), 1):] + p.labels[:G.DECOY_ROT.get((kind, name), 1)] and d.data != p.data
        assert p.same_as_decoy() == []
        tell = [not e for e in G.cannot_tell(p)]
        assert sum(tell) >= 1 and (kind != "md" or sum(tell) >= p.n - 5)


def test_the_mixed_deal_is_the_gpu_file_s(shapes):
    import test_gpu_bam_records as T
    f = getattr(T.mixed, "__wrapped__", None) or getattr(T.mixed, "__pytest_wrapped__", None)
    f = getattr(f, "obj", f)
    assert f is not None, "this pytest does not show the function inside a fixture"
    assert [lb for lb, _ in f(shapes["bam"])] == [lb for lb, _ in G.mixed_cases(shapes["bam"])]


# ------------------------------------------------------------------------------------------------ the periodic output cases
CASES = {"nf-full": G.nucfreq_full, "nf-small": G.nucfreq_small, "format": G.format_case}


@pytest.mark.parametrize("name", sorted(CASES))
def test_periodic_case_passes_2_to_the_32_inside_an_item(name):
    o = CASES[name](False)
    P = len(o.period)
    assert P == sum(o.cyc_len) and not o.tail
    assert o.total() == o.reps * P >= B32 + G.PAST and (o.reps - 1) * P < B32 + G.PAST + 1   # no more repeats than it takes
    assert o.total() + 80 <= G.BUF_BYTES
    assert B32 % P != 0                                                  # not at a period boundary
    i, a, b = o.item_at(B32)
    assert a < B32 < b                                                   # strictly inside an item / a segment
    lens = o.item_len()
    assert sum(int(x) for x in o.cyc_len) * o.reps == int(o.text_off()[-1]) == o.total() and len(lens) == o.n_items()
    assert [int(x) for x in o.text_off()[:o.m + 1]] == [sum(o.cyc_len[:k]) for k in range(o.m + 1)]
    assert int(o.text_off()[i]) == (i // o.m) * P + sum(o.cyc_len[:i % o.m])   # Python integers against the uint64 cumulative sum
    if name == "format":
        assert i % o.m == o.long_index and o.cycle[o.long_index][1] == G.LONG_WORDS and b - a > 8 * 10**6
        assert 0 < B32 % P - sum(o.cyc_len[:o.long_index]) < o.cyc_len[o.long_index]
    else:
        starts = set(o.one_truth[4])
        assert B32 % P not in starts                                      # strictly inside a line


@pytest.mark.parametrize("name", sorted(CASES))
def test_trimmed_case_ends_on_2_to_the_32(name):
    o = CASES[name](True)
    assert o.total() == B32 == int(o.text_off()[-1]) and len(o.tail) >= 1
    assert sum(int(x) for x in o.cyc_len) * o.reps + sum(int(x) for x in o.tail_len) == B32
    assert len(o.tail_text) == sum(o.tail_len) and o.tail_len[-1] > 0  # the last item is not empty: it ends on 2^32
    assert o.text(B32 - 64, B32) == (o.period + o.tail_text)[-64:]
    assert o.text(o.reps * len(o.period) - 5, o.reps * len(o.period) + 5) == o.period[-5:] + (o.tail_text + o.period)[:5]


def test_nucfreq_cycle_holds_what_it_says():
    S, W, pre_max, suf_max = rustybam_amd.nucfreq_text_shape()
    o = G.nucfreq_full(False)
    case = o.one
    assert sorted(case.seg_n.tolist()) == sorted(G.NF_N) and o.m == 8
    assert (max(len(x) for x in case.pre), max(len(x) for x in case.suf)) == (255, 255) == (pre_max, suf_max)
    assert (0, 1) in {(len(a), len(b)) for a, b in zip(case.pre, case.suf)} and (255, 255) in {(len(a), len(b)) for a, b in zip(case.pre, case.suf)}
    text, off, first, lines, starts = o.one_truth
    covered_somewhere, uncovered_somewhere, ten = False, False, False
    for s in range(o.m):
        rows = case.counts[int(case.seg_cnt[s]):int(case.seg_cnt[s]) + int(case.seg_n[s])]
        cov = (rows[:, 0] & nu.COVERED) != 0
        covered_somewhere |= bool(cov.any())
        uncovered_somewhere |= bool((~cov).any())
        vals = rows[cov].astype(np.uint64)
        vals[:, 0] &= nu.COVERED - 1
        ten |= bool((vals >= 10**9).any())
        assert int(lines[s]) == int(cov.sum())
    assert covered_somewhere and uncovered_somewhere and ten
    assert b"\t4294967295\t" in text and b"\t0\t" in text              # a ten-digit count in print; p + 1 wraps to 0 behind the last position
    assert len(set(case.seg_cnt.tolist())) == 8 and int((case.seg_cnt + case.seg_n).max()) <= len(case.counts)
    sm = G.nucfreq_small(False)
    assert all(int(n) > W for n in sm.one.seg_n) and sm.one.seg_n[0] == 4096 and len(sm.table) < 4200
    ln = np.diff(np.array(sm.one_truth[4] + [len(sm.period)]))
    assert 17 < ln.mean() <= 22 and ln.max() == 22
    n_pos = int(sm.one.seg_n.astype(np.int64).sum()) * sm.reps
    assert 1.5e8 < n_pos < 3e8 and 6e5 < n_pos / 256 < 1.2e6             # about 2 10^8 positions, 8 10^5 runs


def test_format_cycle_holds_what_it_says():
    o = G.format_case(False)
    n_small = tu.format_seam_items().n + tu.format_cont_items().n + tu.format_phase_items().n
    assert o.m == n_small + 1 and o.n_items() < 10**6
    a = G.format_arrays(o)
    assert len(a.first) == o.n_items() and (a.first >> np.uint64(63)).any() and a.fl.any() and a.ll.any()
    # every item of the cycle prints what the reference prints from the joined arrays
    for j in list(range(0, o.m, 97)) + [o.long_index]:
        f, c, fl, ll, t = o.cycle[j]
        src = o.alt if f >> 63 else o.ops
        f &= (1 << 63) - 1
        if c < 5000:
            assert tu.ref_format(src[f:f + c], fl, ll) == t
    assert o.period[:len(o.cycle[0][4])] == o.cycle[0][4]
    w = o.ops[o.long_first:o.long_first + G.LONG_WORDS]
    assert (w & 15 == tu.CONT).sum() == 3 and int(G._format_len_of_words(w).sum()) == o.cyc_len[o.long_index]


def test_transfer_windows():
    w = G.xfer_windows()
    assert w[0] == (0, G.MIB) and w[-1][1] == G.XFER_BYTES and w[-1][0] <= G.XFER_BYTES - 4096
    assert any(a <= B32 - G.MIB and b >= B32 + G.MIB for a, b in w)
    for c in (B32 - G.RING_CHUNK, B32, B32 + G.RING_CHUNK):
        assert any(a <= c - 65536 and c + 65536 <= b for a, b in w), c
    assert all(b0 < a1 for (_, b0), (a1, _) in zip(w, w[1:])) and sum(b - a for a, b in w) < 8 * G.MIB
    x = G.xfer_pattern(B32 - 4096, B32 + 4096)
    assert x.all() and not np.array_equal(x[:4096], x[4096:]) and len(set(x.tolist())) > 100
    assert G.DOWN == (B32 - 32 * G.MIB, B32 + 32 * G.MIB) and G.XFER_BYTES == B32 + 64 * G.MIB
