"""rb_dev_nucfreq_text: a plain-Python model of both line formats and of the three segment arrays, and the hand-made cases the GPU
tests run (tests/test_gpu_nucfreq_text.py) -- tests/test_nucfreq_text_inputs.py checks, without a GPU, that the model prints what the
oracle prints and that the cases contain what the GPU file says they do."""
import itertools
from types import SimpleNamespace

import numpy as np

COVERED = 0x80000000
FULL, SMALL = 0, 1
NONE = (1 << 64) - 1  # seg_first of a segment with no covered position
HEADER_FULL = b"#chr\tstart\tend\tA\tC\tG\tT\tregion_id\n"  # nucfreq.rs:127-131
MED = 1000000   # main.rs:101: a print piece
FETCH = 10000   # main.rs:100-110: a fetch


def dec(v):
    """decimal digits of v >= 0, by hand (the inputs test holds it against str())"""
    v = int(v)
    assert v >= 0
    out = bytearray()
    while True:
        out.append(48 + v % 10)
        v //= 10
        if v == 0:
            break
    return bytes(reversed(out))


def full_line(prefix, p, a, c, g, t, suffix):
    """impl Display for Nucfreq (nucfreq.rs:17-33) between the caller's prefix and suffix; the end column is a u32"""
    return b"".join((prefix, dec(p), b"\t", dec((p + 1) & 0xFFFFFFFF), b"\t", dec(a), b"\t", dec(c), b"\t", dec(g), b"\t", dec(t), suffix))


def small_line(a, c, g, t):
    """nucfreq.rs:148-150: the largest and the second largest of the four"""
    m = sorted((int(a), int(c), int(g), int(t)))
    return dec(m[3]) + b"\t" + dec(m[2]) + b"\n"


def model(case):
    """-> (text, seg_text_off [n_seg + 1], seg_first [n_seg], seg_lines [n_seg], line_starts) of a case"""
    cnt = case.counts
    parts, off, first, lines, starts = [], [0], [], [], []
    at = 0
    for s in range(len(case.seg_n)):
        f, n_lines = NONE, 0
        c0, p0 = int(case.seg_cnt[s]), int(case.seg_pos[s])
        for k in np.nonzero(cnt[c0:c0 + int(case.seg_n[s]), 0] & COVERED)[0].tolist():
            a, c, g, t = (int(x) for x in cnt[c0 + k])
            a &= COVERED - 1
            if f == NONE:
                f = p0 + k
            n_lines += 1
            ln = small_line(a, c, g, t) if case.mode == SMALL else full_line(case.pre[s], p0 + k, a, c, g, t, case.suf[s])
            starts.append(at)
            parts.append(ln)
            at += len(ln)
        off.append(at)
        first.append(f)
        lines.append(n_lines)
    return b"".join(parts), np.array(off, np.uint64), np.array(first, np.uint64), np.array(lines, np.uint64), starts


def pack_strings(case):
    """the prefixes and suffixes of a case as rb_dev_nucfreq_text takes them: (strings, pre_off, pre_len, suf_off, suf_len)"""
    blob, po, pl, so, sl = bytearray(b"?"), [], [], [], []  # (a byte in front: offset 0 is nobody's)
    for a, b in zip(case.pre, case.suf):
        po.append(len(blob)), pl.append(len(a))
        blob += a
        so.append(len(blob)), sl.append(len(b))
        blob += b
    u = lambda x: np.array(x, np.uint32)  # noqa: E731
    return bytes(blob), u(po), u(pl), u(so), u(sl)


def make_case(name, mode, counts, segs):
    """segs: (cnt, pos, n, prefix, suffix) each"""
    counts = np.ascontiguousarray(np.array(counts, np.uint64).reshape(-1, 4).astype(np.uint32))
    c = SimpleNamespace(name=name, mode=mode, counts=counts,
                        seg_cnt=np.array([s[0] for s in segs], np.uint64), seg_pos=np.array([s[1] for s in segs], np.uint64),
                        seg_n=np.array([s[2] for s in segs], np.uint32), pre=[bytes(s[3]) for s in segs], suf=[bytes(s[4]) for s in segs])
    for s in range(len(segs)):
        assert int(c.seg_cnt[s]) + int(c.seg_n[s]) <= len(counts) and int(c.seg_pos[s]) + int(c.seg_n[s]) <= 1 << 32
    return c


# ---- the cases ----
A_SEAMS = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
           999999999, 1000000000, (1 << 31) - 1]
CGT_SEAMS = A_SEAMS + [1 << 31, (1 << 32) - 1]
POS_SEAMS = [10 ** k - 1 for k in range(1, 10)] + [(1 << 31) - 1, (1 << 32) - 2]  # a segment of two positions starts at each


def _rng(seed):
    return np.random.default_rng(seed)


def _covered_counts(rng, n, hi=40):
    c = rng.integers(0, hi, (n, 4)).astype(np.uint64)
    c[:, 0] |= COVERED
    return c


def digit_seams(mode):
    """every digit count of every field: each seam value in each of A, C, G, T, and positions either side of every power of ten, of
    2^31 and the last two positions there are (the very last prints 0 for p + 1)"""
    rows = []
    for f in range(4):
        for v in (A_SEAMS if f == 0 else CGT_SEAMS):
            r = [COVERED | 7, 7, 7, 7]
            r[f] = v | (COVERED if f == 0 else 0)
            rows.append(r)
    n_val = len(rows)
    segs = [(0, 0, n_val, b"c\t", b"\tid\n")]
    rng = _rng(11)
    for p in POS_SEAMS:
        at = len(rows)
        rows += _covered_counts(rng, 2).tolist()
        segs.append((at, p, 2, b"chrP\t", b"\tx\n"))
    return make_case("digit_seams", mode, rows, segs)


FIX_LENS = [0, 1, 15, 16, 17, 255]


def phases(mode):
    """prefix and suffix lengths 0, 1, 15, 16, 17, 255 in every combination, 70 lines a segment (more than one step; with 255 + 255 more
    than one stage of the print kernel), counts of 1 - 3 digits so that line starts fall on every byte phase"""
    rng = _rng(12)
    rows, segs = [], []
    for pl, sl in itertools.product(FIX_LENS, FIX_LENS):
        at = len(rows)
        rows += _covered_counts(rng, 70, 300).tolist()
        pre = bytes(65 + (i + pl) % 26 for i in range(pl))
        suf = bytes(97 + (i + sl) % 26 for i in range(sl))
        segs.append((at, 995 + 13 * len(segs), 70, pre, suf))
    return make_case("phases", mode, rows, segs)


def run_length_list(S, W):
    R = W // 4  # (a wavefront's run)
    return sorted({0, 1, S - 1, S, S + 1, R - 1, R, R + 1, W - 1, W, W + 1, 2 * W + 1})


def run_lengths(mode, S, W):
    """segments of 0, 1, S - 1, S, S + 1, W - 1, W, W + 1, 2 W + 1 positions (and either side of a wavefront's run), all covered"""
    rng = _rng(13)
    rows, segs = [], []
    for n in run_length_list(S, W):
        at = len(rows)
        rows += _covered_counts(rng, n).tolist()
        segs.append((at, 99990 - n // 2, n, b"chr7\t", b"\trl\n"))
    return make_case("run_lengths", mode, rows, segs)


def coverage(mode, S, W):
    """uncovered runs that span a whole step and a whole workgroup (and more); a covered position only at the first / only at the
    last index; nothing covered"""
    rng = _rng(14)
    rows, segs = [], []

    def seg(n, covered_idx):
        at = len(rows)
        c = rng.integers(1, 40, (n, 4)).astype(np.uint64)  # (counts stay: an uncovered position with counts must still print nothing)
        m = np.zeros(n, bool)
        m[covered_idx] = True
        c[m, 0] |= COVERED
        rows.extend(c.tolist())
        segs.append((at, 5000 + 7 * len(segs), n, b"chrC\t", b"\tcov\n"))
    n = 4 * W + 5
    k = np.arange(n)
    seg(n, k[(k < S - 3) | ((k >= 3 * S) & (k < W - 1)) | (k >= 3 * W + 3)])  # holes: two steps and more, two workgroups and more
    seg(n, [0])
    seg(n, [n - 1])
    seg(n, [])
    seg(W, [])
    seg(1, [])
    seg(n, k[k % 3 == 0])
    return make_case("coverage", mode, rows, segs)


def many_short(mode):
    """3000 segments of 1 - 5 positions behind each other: seams between segments at every phase"""
    rng = _rng(15)
    rows, segs = [], []
    for i in range(3000):
        n = int(rng.integers(1, 6))
        at = len(rows)
        c = _covered_counts(rng, n, 1200)
        if i % 7 == 3:
            c[int(rng.integers(0, n)), 0] &= COVERED - 1
        rows += c.tolist()
        segs.append((at, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), n, b"s%d\t" % (i % 13), b"\t%d\n" % (i % 101)))
    return make_case("many_short", mode, rows, segs)


def overlapping(mode):
    """segments that share counts: nested, shifted and identical ranges, each with a position and strings of its own"""
    rng = _rng(16)
    rows = _covered_counts(rng, 700).tolist()
    for i in range(0, 700, 9):
        rows[i][0] &= COVERED - 1
    segs = [(0, 0, 700, b"a\t", b"\t1\n"), (100, 100, 300, b"bb\t", b"\t22\n"), (100, 100, 300, b"bb\t", b"\t22\n"), (250, 77, 450, b"ccc\t", b"\t\n"),
            (699, 1, 1, b"d\t", b"\tz\n"), (0, 123456, 700, b"a\t", b"\t1\n")]
    return make_case("overlapping", mode, rows, segs)


def shuffled_layout(mode):
    """seg_cnt not in segment order: the segments' counts lie in the array in another order than the segments print"""
    rng = _rng(17)
    ns = [300, 1, 65, 257, 0, 64, 1030]
    order = [3, 6, 0, 5, 1, 4, 2]
    at, cnt_of, rows = 0, {}, []
    for s in order:
        cnt_of[s] = at
        rows += _covered_counts(rng, ns[s], 70000).tolist()
        at += ns[s]
    segs = [(cnt_of[s], 1000 * s, ns[s], b"q%d\t" % s, b"\tw\n") for s in range(len(ns))]
    return make_case("shuffled_layout", mode, rows, segs)


def small_orders():
    """--small: all 24 orders of four distinct counts, ties for the first and the second place, all four equal; the covered bit of the
    A word must not count as part of A (A = 0 beside it, and A the largest beside it)"""
    rows = [list(p) for p in itertools.permutations([3, 45, 678, 9012])]
    rows += [[5, 5, 1, 0], [1, 5, 5, 0], [0, 1, 5, 5], [5, 0, 1, 5], [9, 4, 4, 1], [1, 4, 9, 4], [4, 1, 4, 9], [7, 7, 7, 7], [0, 0, 0, 0],
             [0, 3, 2, 1], [100, 3, 2, 1], [(1 << 31) - 1, (1 << 32) - 1, 1 << 31, 0], [0, 1 << 31, 0, 0]]
    for r in rows:
        r[0] |= COVERED
    rows.append([5, 6, 7, 8])  # (not covered)
    return make_case("small_orders", SMALL, rows, [(0, 10, len(rows), b"", b"")])


CASE_NAMES = ["small_orders"] + [f"{n}-{m}" for m in ("full", "small")
                                  for n in ("digit_seams", "phases", "run_lengths", "coverage", "many_short", "overlapping", "shuffled_layout")]


def get_case(name, S, W):
    if name == "small_orders":
        return small_orders()
    kind, m = name.split("-")
    mode = FULL if m == "full" else SMALL
    f = globals()[kind]
    return f(mode, S, W) if kind in ("run_lengths", "coverage") else f(mode)


# ---- the regions of `rb nucfreq` as the front end cuts them (main.rs:82-121) ----
def oracle_text(pyoracle, reads, ref_names, ref_lens, regions, small):
    """(bytes `rb nucfreq` prints for regions = [(name, st, en, id)], lines compared, longest region) -- pyoracle.nucfreq per fetch of
    10 kb, the model's lines per print piece of 1 Mbp, the header lines in between"""
    out, n_lines, longest = [], 0, 0
    for name, st, en, rid in regions:
        tid = ref_names.index(name)
        longest = max(longest, en - st)
        for m0 in range(st, en, MED):
            m1 = min(m0 + MED, en)
            pos, cnt = [], []
            for f0 in range(m0, m1, FETCH):
                rc, p, c = pyoracle.nucfreq(*reads, tid, f0, min(f0 + FETCH, m1))
                assert rc == 0
                pos.append(p), cnt.append(c)
            pos, cnt = np.concatenate(pos), np.concatenate(cnt)
            keep = pos < ref_lens[tid]
            pos, cnt = pos[keep], cnt[keep]
            # the piece as a segment of rb_dev_nucfreq_text: every position of it, the covered ones marked
            n = m1 - m0
            rows = np.zeros((n, 4), np.uint64)
            rows[pos.astype(np.int64) - m0] = cnt
            rows[pos.astype(np.int64) - m0, 0] |= COVERED
            case = make_case("piece", SMALL if small else FULL, rows, [(0, m0, n, name.encode() + b"\t", b"\t" + rid.encode() + b"\n")])
            text, _, first, lines, _ = model(case)
            if small:
                if int(first[0]) != NONE:
                    out.append(b"#" + name.encode() + b"\t" + dec(first[0]) + b"\t" + rid.encode() + b"\n")
            else:
                out.append(HEADER_FULL)
            out.append(text)
            n_lines += int(lines[0])
    return b"".join(out), n_lines, longest
