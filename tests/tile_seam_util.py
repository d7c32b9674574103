"""Inputs of the tile kernel's seam tests (tests/test_tile_seam_inputs.py, tests/test_gpu_tile_seams.py) and a plain restatement of what
rb_tile_body (rustybam_amd/csrc/k_tile.hip) decides before and behind its stream: which records of a tile it keeps and how many it hands
to the per-record kernel.  None of it is taken from the kernel but its constants, which are read from the defines.

A tile under test is ISOLATED: rb_cut_tiles is greedy and a record above RB_SHORT_MAX_DEFAULT ops closes a tile, so a separator of more
than that many ops lies in front of every tile (its length sets head = first op of the tile & 31) and behind it, or the batch ends there.

Records are regular (= X M I D, no two neighbours of one type, a match-type op at both ends): even op indices carry = or M (4 .. 30 bases),
odd ones X (1 .. 30) or I / D (1 .. 5), so every indel lies between two match-type ops and no boundary is the generic kernel's; at most
one op of a record is a "long" indel of 6 .. 30 bases, which break-paf --max-size 5 cuts at.  Strands alternate, targets increase with
ROOM bases between two records."""
import ctypes as C
import os
import re

import numpy as np

import break_seam_util as bs
from rbtest_util import OPC, sums

EQ, X, I, D, M = OPC["="], OPC["X"], OPC["I"], OPC["D"], OPC["M"]
ROOM = 1000                 # reference bases between two records
G_ONES, G_EQ = 0xFFFFFFFF, 0xFFFFFFF7   # what lies outside the records of a starts-form batch: all ones, and a = of the largest length
BREAK_A = 5                 # --max-size of family A: cuts at the long indel of a record and nowhere else


def _define(name, path):
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustybam_amd", "csrc", path)) as f:
        return int(re.search(r"^#define\s+%s\s+(\d+)" % name, f.read(), re.M).group(1))


RBT_OPS, RBT_REC, RBT_HITS, RBT_GAP_MAX = (_define(k, "k_tile.hip") for k in ("RBT_OPS", "RBT_REC", "RBT_HITS", "RBT_GAP_MAX"))
RB_MS = _define("RB_MS", "rb_lift.h")
SHORT_MAX = _define("RB_SHORT_MAX_DEFAULT", "capi.hip")
STEP = 512                  # ops a step of the stream covers: 64 lanes of 8
TILE_OPS = RBT_OPS - 32     # ops of a tile's records at most (rb_tile_max_ops)
MIN_OPS = 8                 # ops of a record the tile kernel takes at least


# ------------------------------------------------------------------------------------------------ the model
def handed_back(n, bad, hits=None, gaps=None, pieces=None):
    """One tile of n records -> how many of them rb_tile_body hands to the per-record kernel.
    hits[j]   liftover form (BED windows, or break-paf in two walks, whose windows are the pieces): hits of record j; None: break form
    bad[j]    the set-up cannot take record j (bad_records)
    gaps[j]   RB_LIFT_OP_STARTS: ops between record j - 1 and record j (gaps[0] is not looked at); None: a dense batch
    pieces[j] break form (one walk): pieces of record j"""
    lo, hi, back = 0, n, 0
    if hits is not None and int(np.sum(hits)) > RBT_HITS:   # 1. the hits fill the lanes: the leading records whose hits fit stay
        m = int((np.cumsum(hits) <= RBT_HITS).sum())
        if m == 0:
            return n
        back, hi = n - m, m
    if any(bad[lo:hi]):                                     # 2. the longest run of records the set-up can take, the first one on ties
        best_s = best_n = 0
        prev = lo
        for j in list(np.flatnonzero(np.asarray(bad[lo:hi], bool)) + lo) + [hi]:
            if j - prev > best_n:
                best_s, best_n = prev, j - prev
            prev = j + 1
        if best_n == 0:
            return n
        back += (hi - lo) - best_n
        lo, hi = best_s, best_s + best_n
    if gaps is not None and any(int(g) > RBT_GAP_MAX for g in gaps[lo + 1:hi]):   # 3. what is left goes back as a whole
        return back + hi - lo
    if pieces is not None and int(np.sum(pieces[lo:hi])) > RBT_HITS:
        return back + hi - lo
    return back


def plan_tiles(op_off):
    """rb_plan_tiles_host -> [(first record, records, pass-through)]"""
    from rustybam_amd import capi
    L = capi.lib()
    L.rb_plan_tiles_host.restype = C.c_int64
    off = np.ascontiguousarray(op_off, dtype=np.uint64)
    n = len(off) - 1
    sched, tiles, n_long = np.zeros(max(n, 1), np.uint32), np.zeros(3 * max(n, 1), np.uint32), C.c_uint64(0)
    nt = L.rb_plan_tiles_host(C.c_uint64(n), off.ctypes.data_as(C.c_void_p), C.c_uint64(0), sched.ctypes.data_as(C.c_void_p),
                              tiles.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.byref(n_long))
    assert nt >= 0
    return [(int(f) & 0x7FFFFFFF, int(c), bool(int(f) >> 31)) for f, c, _ in tiles[:3 * nt].reshape(-1, 3)]


def records(b, idx=None):
    off = b["op_off"].astype(np.int64)
    return [b["ops"][off[r]:off[r + 1]] for r in (range(len(off) - 1) if idx is None else idx)]


def bad_records(oracle, b):
    """the records the tile kernel's set-up cannot take: irregular, end indels stripped, norm status not OK, fewer than MIN_OPS ops"""
    norm = oracle.normalize(oracle.Batch(*[b[k] for k in ("ops", "op_off", "t_st", "t_en", "q_st", "q_en", "strand")], b["contig"]))
    reg = np.array([len(c) > 0 and bs.is_regular(c) for c in records(b)])
    return (~reg) | (norm["status"] != 0) | (norm["lead_ops"] != 0) | (norm["trail_ops"] != 0) | (np.diff(b["op_off"].astype(np.int64)) < MIN_OPS)


def hits_per_record(orows, n_rec, status):
    """the oracle's rows per record; a record the reference panics on has no job to count hits for"""
    h = np.bincount(orows["rec"].astype(np.int64), minlength=n_rec)
    return np.where(status == 0, h, 0)


def expected_back(oracle, b, orows=None, max_size=None, gaps=None, op_off=None, two_walk=False):
    """the whole batch: the model's count over the tiles rb_plan_tiles_host cuts from op_off (default: the batch's own); liftover over
    the windows that gave `orows`, or break-paf at max_size (two_walk: its pieces are the windows of the liftover form)"""
    n_rec = len(b["t_st"])
    bad = bad_records(oracle, b)
    status = oracle.normalize(oracle.Batch(*[b[k] for k in ("ops", "op_off", "t_st", "t_en", "q_st", "q_en", "strand")], b["contig"]))["status"]
    hits = pieces = None
    if max_size is None:
        hits = hits_per_record(orows, n_rec, status)
    else:
        p = np.array([bs.n_pieces(c, max_size) if s == 0 else 0 for c, s in zip(records(b), status)])
        hits, pieces = (p, None) if two_walk else (None, p)
    total = 0
    for first, cnt, tiny in plan_tiles(b["op_off"] if op_off is None else op_off):
        s = slice(first, first + cnt)
        total += cnt if tiny else handed_back(cnt, bad[s], None if hits is None else hits[s], None if gaps is None else gaps[s],
                                              None if pieces is None else pieces[s])
    return total


# ------------------------------------------------------------------------------------------------ records and batches
def record(n, seed, long_at=None):
    """a regular record of exactly n ops; long_at: the odd op index that carries the long indel"""
    i = np.arange(n)
    h = i * 7 + seed * 13 + (i * i) % 11
    k = (i // 2 + seed) % 3
    code = np.where(i % 2 == 0, np.where(k == 0, M, EQ), np.choose(k, [X, I, D]))
    ln = np.where(i % 2 == 0, 4 + h % 27, np.where(code == X, 1 + h % 30, 1 + h % 5))
    if n % 2 == 0:
        code[-1], ln[-1] = X, 1 + h[-1] % 30
    if long_at is not None:
        assert long_at % 2 == 1 and 0 < long_at < n - 1, (n, long_at)
        code[long_at], ln[long_at] = (I, D)[seed % 2], 6 + h[long_at] % 25
    c = ((ln << 4) | code).astype(np.uint32)
    assert bs.is_regular(c) and int(ln.max()) <= 30
    return c


def long_spot(n, seed):
    """second op, last op but one (the odd index next to it), or the middle, in turn"""
    return (1, (n - 2) - ((n - 2) % 2 == 0), (n // 2) | 1)[seed % 3] if n >= 4 else None


def make_batch(cigs):
    n = len(cigs)
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    RQ = [sums(c) for c in cigs]
    R, Q = np.array([x[0] for x in RQ], np.uint64), np.array([x[1] for x in RQ], np.uint64)
    t_st = np.uint64(1000) + np.concatenate([[0], np.cumsum(R + np.uint64(ROOM))[:-1]]).astype(np.uint64)
    q_st = np.arange(n, dtype=np.uint64) * np.uint64(7)
    strand = np.where(np.arange(n) % 2 == 0, ord("+"), ord("-")).astype(np.uint8)
    return dict(ops=np.concatenate(cigs).astype(np.uint32), op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=q_st, q_en=q_st + Q, strand=strand,
                contig=np.zeros(n, np.uint32))


def rebuild(b, cigs_of):
    """the batch with the CIGARs of the records in cigs_of {record: cigar} replaced, headers recomputed"""
    cigs = records(b)
    for r, c in cigs_of.items():
        cigs[r] = np.asarray(c, np.uint32)
    return make_batch(cigs)


def separator(at, head):
    """a record above SHORT_MAX ops, so long that the record behind it starts `head` ops behind a multiple of 32 when this one starts at op `at`"""
    return SHORT_MAX + 1 + (head - at - SHORT_MAX - 1) % 32


def layout(tiles, tail=True, longs=True):
    """tiles = [(head, [ops of record 0, 1, ..])] -> (batch, [(first record, records) per tile]): a separator in front of every tile and,
    tail, one behind the last"""
    cigs, where, at = [], [], 0
    for head, lens in tiles:
        s = separator(at, head)
        cigs.append(record(s, len(cigs)))
        at += s
        assert at % 32 == head and all(MIN_OPS <= n <= SHORT_MAX for n in lens) and sum(lens) <= TILE_OPS and len(lens) <= RBT_REC, (head, lens)
        where.append((len(cigs), len(lens)))
        for n in lens:
            cigs.append(record(n, len(cigs), long_spot(n, len(cigs)) if longs else None))
            at += n
    if tail:
        cigs.append(record(separator(at, 0), len(cigs)))
    return make_batch(cigs), where


def fill(prefix, total, cap=2000):
    """prefix + records of up to cap ops, total ops together"""
    out, rem = list(prefix), total - sum(prefix)
    assert rem >= MIN_OPS, (prefix, total)
    while rem:
        n = rem if rem <= cap else (cap if rem - cap >= MIN_OPS else rem - MIN_OPS)
        out.append(n)
        rem -= n
    return out


def geometry(b, first, cnt, starts=None, n_ops=None):
    """of the tile of records [first, first + cnt): head, n_tile, n_steps, gend & 3, the set of rel0 & 7 and rel0 % STEP of its records'
    starts (counted from g0 = the first op's 32-op line); starts / n_ops: the records' extents when they are not the batch's offsets"""
    st = np.asarray(b["op_off"][:-1] if starts is None else starts, np.int64)[first:first + cnt]
    n = np.diff(b["op_off"].astype(np.int64))[first:first + cnt] if n_ops is None else np.asarray(n_ops, np.int64)[first:first + cnt]
    g_first, gend = int(st[0]), int(st[-1] + n[-1])
    g0 = g_first & ~31
    rel0 = st - g0
    return dict(head=g_first - g0, n_tile=gend - g_first, n_steps=(gend - g0 + STEP - 1) // STEP, gend3=gend & 3, rel7=set((rel0 & 7).tolist()),
                rel_step=set((rel0[1:] % STEP).tolist()))


# ------------------------------------------------------------------------------------------------ windows
N_KINDS = 8


def window(b, r, kind):
    """window `kind` of record r: 0 its first base, 1 its last base, 2 one base inside its first op, 3 one base inside its last op, 4 inside
    one op (its third), 5 ends exactly at its t_en, 6 starts at the NEXT record's t_st (and hits that one), 7 holds the whole record"""
    t0, t1 = int(b["t_st"][r]), int(b["t_en"][r])
    o = int(b["op_off"][r])
    c = b["ops"][o:o + 3].astype(np.int64)
    l0, l2 = int(c[0] >> 4), int(c[2] >> 4)
    llast = int(b["ops"][int(b["op_off"][r + 1]) - 1]) >> 4
    if kind == 0:
        return t0, t0 + 1
    if kind == 1:
        return t1 - 1, t1
    if kind == 2:
        return t0 + l0 // 2, t0 + l0 // 2 + 1
    if kind == 3:
        return t1 - 1 - llast // 2, t1 - llast // 2
    if kind == 4:
        p = t0 + sums(c[:2])[0]
        return p + 1, p + l2 - 1
    if kind == 5:
        return t1 - 3, t1
    if kind == 6:
        nxt = int(b["t_st"][r + 1]) if r + 1 < len(b["t_st"]) else t1
        return nxt, nxt + 2
    return t0 - 1, t1 + 1


def windows_in_turn(b, where, per=2):
    """`per` windows for every record of the tiles in `where`, the kinds taken in turn along each tile; sorted, st and en both ascending"""
    w = []
    for first, cnt in where:
        for k in range(cnt):
            w += [window(b, first + k, (per * k + j) % N_KINDS) for j in range(per)]
    return as_windows(w)


def as_windows(w, sort=True):
    w = sorted(w) if sort else list(w)
    st, en = np.array([x[0] for x in w], np.uint64), np.array([x[1] for x in w], np.uint64)
    assert (np.diff(st.astype(np.int64)) >= 0).all() and (np.diff(en.astype(np.int64)) >= 0).all(), "the window list must stay monotone"
    return np.zeros(len(w), np.uint32), st, en


# ------------------------------------------------------------------------------------------------ A: stream geometry
A_HEADS = (0, 1, 15, 16, 31)
A_TOTALS = (511, 512, 513, 1024, 1025, 1536, 1537)   # head + n_tile
A_FULL = {0: TILE_OPS, 31: TILE_OPS + 31}            # eight steps; the most a plan makes
A_END = 200                                          # head + n_tile of the tile that ends batch k is A_END + k: gend & 3 takes every value


def a_lengths(head, total):
    """the records of family A's tile with head + n_tile = total"""
    n = total - head
    if total == 511:
        return fill([8] * 20, n)                               # records of 8 ops back to back: every chunk holds a record start
    if total == 512:
        return fill(list(range(9, 25)), n)
    if total == 513:
        return fill(list(range(25, 32)), n)
    if total == 1024:
        return fill([STEP - head] + [8] * 10, n)               # a record starts on op 0 of step 1
    if total == 1025:
        return fill([STEP - 1 - head] + list(range(9, 16)), n)  # ... on op 511 of step 0
    if total == 1536:
        return fill([2 * STEP - head] + list(range(11, 18)), n)  # ... on op 0 of step 2 (ring slot 0 again)
    if total == 1537:
        return fill([2 * STEP - 1 - head] + [8] * 5, n)
    if total >= TILE_OPS:
        return fill([2000] + [8] * 16 + list(range(9, 16)), n)
    return fill(list(range(8, 16)), n)                         # the end tiles


def family_a(k):
    """batch k of family A: the tiles of head A_HEADS[k], one per total, and an end tile with no separator behind it
    -> (batch, [(first, cnt)], [claimed (head, total)])"""
    head = A_HEADS[k]
    totals = list(A_TOTALS) + ([A_FULL[head]] if head in A_FULL else []) + [A_END + k]
    b, where = layout([(head, a_lengths(head, t)) for t in totals], tail=False)
    return b, where, [(head, t) for t in totals]


# ------------------------------------------------------------------------------------------------ B: hits fill the lanes
B_REC, B_HEAD = 24, 7
_three = lambda n3, n_rec=B_REC: [3] * n3 + [2] * (n_rec - n3)  # noqa: E731
# name -> (hits per record, arrangement of a record's windows)
B_CASES = {
    "sum63": (_three(15), "disjoint"),
    "sum64": (_three(16), "disjoint"),
    "sum65": (_three(17), "disjoint"),
    "hit64_ends_record15": ([4] * 16 + [2] * 8, "disjoint"),
    "hit64_inside_record15": ([4] * 15 + [6] + [2] * 8, "disjoint"),
    "first_record_64": ([RBT_HITS] + [1] * 23, "disjoint"),
    "first_record_65": ([RBT_HITS + 1] + [1] * 23, "disjoint"),
    "one_record_has_hits": ([0] * 7 + [5] + [0] * 16, "disjoint"),
    "no_hits": ([0] * B_REC, "disjoint"),
    "classes_nested": ([3, 4, 5, 0] * 5 + [0] * 4, "nested"),
    "classes_identical": ([3, 4, 5, 0] * 5 + [0] * 4, "identical"),
    "classes_disjoint": ([3, 4, 5, 0] * 5 + [0] * 4, "disjoint"),
}
B_OVERFLOW = ("sum65", "hit64_ends_record15", "hit64_inside_record15", "first_record_64", "first_record_65")


def b_batch():
    return layout([(B_HEAD, [76 + r for r in range(B_REC)])])


def b_windows(b, where, name):
    counts, how = B_CASES[name]
    first, cnt = where[0]
    w = []
    for j, k in enumerate(counts):
        t0, t1 = int(b["t_st"][first + j]), int(b["t_en"][first + j])
        assert t1 - t0 >= 3 * k + 8
        for i in range(k):
            w.append({"disjoint": (t0 + 3 * i, t0 + 3 * i + 2), "identical": (t0 + 5, t1 - 5), "nested": (t0 + 2 * i, t1 - 3)}[how])
    if not w:
        w = [(int(b["t_en"][-1]) + 10, int(b["t_en"][-1]) + 20)]   # (a window list is never empty: this one lies behind every record)
    return as_windows(w)


# ------------------------------------------------------------------------------------------------ C: the run cut
C_REC, C_HEAD = RBT_REC, 21
KINDS = ("split", "lead_ins", "t_en")
# name -> (bad lanes, kind of badness, windows per record)
C_CASES = {
    "lane0": ([0], "split", 1), "lane31": ([31], "lead_ins", 1), "lanes0_31": ([0, 31], "t_en", 1),
    "lane15": ([15], "lead_ins", 1), "lane16": ([16], "t_en", 1), "lanes15_16": ([15, 16], "split", 1),
    "three_runs_of_ten": ([10, 21], "t_en", 1), "odd_lanes": (list(range(1, 32, 2)), "split", 1),
    "all_split": (list(range(32)), "split", 1), "all_lead_ins": (list(range(32)), "lead_ins", 1), "all_t_en": (list(range(32)), "t_en", 1),
    "hit_cut_then_bad_behind_it": ([25], "split", 3), "hit_cut_and_run_cut": ([5], "split", 3),
}


def c_case(name):
    """-> (batch, [(first, cnt)], windows): one tile of 32 records of 36 .. 44 ops with the bad records of the case"""
    lanes, kind, per = C_CASES[name]
    b, where = layout([(C_HEAD, [36 + r % 9 for r in range(C_REC)])])
    first = where[0][0]
    new = {}
    for j in lanes:
        c = records(b, [first + j])[0]
        if kind == "split":      # op 4 in two ops of its type: the same bases, irregular
            w = int(c[4])
            new[first + j] = np.concatenate([c[:4], [(((w >> 4) - 1) << 4) | (w & 15), (1 << 4) | (w & 15)], c[5:]])
        elif kind == "lead_ins":  # remove_trailing_indels strips it: the record no longer lies where its offsets say
            new[first + j] = np.concatenate([[(2 << 4) | I], c])
    b = rebuild(b, new)
    if kind == "t_en":           # check_integrity fails: the record has a status, not a job
        b["t_en"][[first + j for j in lanes]] += np.uint64(1)
    w = []
    for j in range(C_REC):
        t0 = int(b["t_st"][first + j])
        w += [(t0 + 9 + 30 * i, t0 + 9 + 30 * i + 12) for i in range(per)]
    return b, where, as_windows(w)


# ------------------------------------------------------------------------------------------------ D: RB_LIFT_OP_STARTS
def starts_batch(head, lens, gaps, front=0, tail=5, lead=None, make=None):
    """A batch in starts form, made by hand.  The tile's records have lens[r] ops; gaps[r] ops lie between record r - 1 and r (gaps[0] is not
    used), `front` ops in front of record 0 inside its old extent and `tail` ops behind the last one.  The OLD dense batch, which defines
    the plan, is a separator (the old tile starts `head` ops behind a multiple of 32) and the old records: record r's old extent reaches
    from lead[r] ops in front of it (default: none, half, all of the gap in turn) to where record r + 1's begins.
    -> dict: ops (garbage outside the records), op_off (old), starts [n_rec + 1], n_ops [n_rec], twin (the dense batch of the records as
    they are now), first / cnt (the tile), gaps [n_rec] (0 in front of the tile's first record)"""
    n = len(lens)
    gaps = [0] + list(gaps[1:]) if len(gaps) == n else [0] + list(gaps)
    assert len(gaps) == n
    if lead is None:
        lead = [0] + [(0, gaps[r] // 2, gaps[r])[r % 3] for r in range(1, n)]
    lead = [front] + list(lead[1:])
    sep = separator(0, head)
    make = make or (lambda n_ops, idx: record(n_ops, idx, long_spot(n_ops, idx)))
    cigs = [record(sep, 0)] + [make(lens[r], r + 1) for r in range(n)]
    twin = make_batch(cigs)
    new_start, at = [], sep + front
    for r in range(n):
        at += gaps[r]
        new_start.append(at)
        at += lens[r]
    old_start = [new_start[r] - lead[r] for r in range(n)]
    total = at + tail
    old_off = np.array([0] + old_start + [total], np.uint64)
    assert old_start[0] == sep
    ops = np.where(np.arange(total) % 2 == 0, G_ONES, G_EQ).astype(np.uint32)
    ops[:sep] = cigs[0]
    for r in range(n):
        ops[new_start[r]:new_start[r] + lens[r]] = cigs[r + 1]
    b = dict(twin)
    b.update(ops=ops, op_off=old_off)
    return dict(b=b, twin=twin, starts=np.array([0] + new_start + [total], np.uint64), n_ops=np.array([sep] + list(lens), np.int64),
                first=1, cnt=n, gaps=np.array([0] + gaps, np.int64))


KEPT_GAPS = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, RBT_GAP_MAX - 1, RBT_GAP_MAX)
# name -> arguments of starts_batch
D_CASES = {
    "gaps_small": dict(head=3, lens=[24 + r for r in range(9)], gaps=[0, 0, 1, 7, 8, 9, 63, 64, 65], tail=5),
    "gaps_step": dict(head=30, lens=[40, 9, 33, 64], gaps=[0, 511, 512, 513], tail=6),
    "gaps_max": dict(head=12, lens=[100, 8, 57], gaps=[0, RBT_GAP_MAX - 1, RBT_GAP_MAX], tail=7),
    "gap_above_max": dict(head=12, lens=[100, 8, 57, 30], gaps=[0, 5, RBT_GAP_MAX + 1, 2], tail=4),
    # gaps of 9 .. 23 ops between records of 16: their first and last ops take every position of a chunk
    "chunk_positions": dict(head=5, lens=[16] * 16, gaps=[0] + [9 + r for r in range(15)], tail=9),
    # record 0 ends on op 500 of step 0, record 1 starts in step 2: the gap holds all of step 1
    "gap_holds_a_step": dict(head=0, lens=[500, 60, 31], gaps=[0, 2 * STEP - 500 + 17, 3], tail=8),
    "front_1": dict(head=20, lens=[50, 20, 30], gaps=[0, 4, 11], front=1, tail=0),
    "front_16": dict(head=20, lens=[50, 20, 30], gaps=[0, 4, 11], front=16, tail=1),    # (the first op moves to the next 32-op line)
    "front_31": dict(head=20, lens=[50, 20, 30], gaps=[0, 4, 11], front=31, tail=2),
    "tail_cut": dict(head=9, lens=[50, 20, 30], gaps=[0, 0, 0], tail=700),
    "shrunk_to_8": dict(head=17, lens=[40, 8, 8, 40, 8], gaps=[0, 30, 3, 12, 100], tail=3),
    "shrunk_to_7": dict(head=17, lens=[40, 8, 41, 42, 7, 43, 44, 45, 7, 46], gaps=[0, 30, 3, 12, 100, 1, 2, 3, 4, 5], tail=3),
}
D_BACK = {"gap_above_max": 4, "shrunk_to_7": 10 - 4}   # the tile's records; all but the longest run, [0, 4)


def d_case(name):
    return starts_batch(**D_CASES[name])


def gap_list(s):
    """the gaps of a starts-form batch, from its start table and extents"""
    st, n = s["starts"][:-1].astype(np.int64), s["n_ops"]
    return np.concatenate([[0], st[1:] - (st[:-1] + n[:-1])])


# ------------------------------------------------------------------------------------------------ E: break form across seams and gaps
def e_record(n_ops, idx):
    """bs.planted: a long indel as the second op and as the last op but one"""
    return bs.planted(n_ops, 0, [1, n_ops - 2], seed=900 + idx)


E_SIZES = (100, bs.BIG - 1, bs.BIG, bs.BIG + 1)   # --max-size below the planted length (twice), at it, above it


def e_dense():
    """family A's geometry head 15, total 1025 (a record starts on op 511 of step 0), 21 records of three pieces each"""
    lens = fill([STEP - 1 - 15] + list(range(9, 16)) + [8] * 12, 1025 - 15)
    assert len(lens) == 21
    cigs, at = [], 0
    s = separator(0, 15)
    cigs.append(record(s, 0))
    for k, n in enumerate(lens):
        cigs.append(e_record(n, k))
    cigs.append(record(separator(s + sum(lens), 0), 99))
    return make_batch(cigs), [(1, len(lens))]


def e_starts():
    """gaps of 1, 8, 65, 513 and 1024 ops between planted records: the long indels lie on either side of every gap"""
    return starts_batch(head=6, lens=[30, 9, 70, 8, 41, 25], gaps=[0, 1, 8, 65, 513, RBT_GAP_MAX], tail=11, make=e_record)


# ------------------------------------------------------------------------------------------------ the input of tests/test_gpu_tile.py
def cut_test_input(bad=(5, 41, 42, 90), n_rec=96, seed=0xC07, lo=100, hi=160, span=150_000):
    """test_a_tile_is_cut_around_a_record_it_cannot_take's batch, made on the host alone (the GPU test makes it with the engine's record scan
    and checks that both are the same): the library's synthetic records, op 3 (or the next op of two bases and more) of every bad record split
    in two ops of its type"""
    from rustybam_amd import capi
    n = capi.synth_n_ops(seed, 0, n_rec, lo, hi)
    off = np.zeros(n_rec + 1, np.uint64)
    off[1:] = np.cumsum(n)
    ops = capi.synth_fill_ops_host(seed, 0, off)
    RQ = [sums(ops[int(off[r]):int(off[r + 1])]) for r in range(n_rec)]
    strand = np.where(np.arange(n_rec) % 3 == 0, ord("-"), ord("+")).astype(np.uint8)
    rng = np.random.default_rng(seed & 0xFFFF)
    t_st = rng.integers(0, span, n_rec).astype(np.uint64)
    q_st = rng.integers(0, 100_000, n_rec).astype(np.uint64)
    b = dict(ops=ops, op_off=off, t_st=t_st, t_en=t_st + np.array([x[0] for x in RQ], np.uint64), q_st=q_st,
             q_en=q_st + np.array([x[1] for x in RQ], np.uint64), strand=strand, contig=np.zeros(n_rec, np.uint32))
    return split_ops(b, bad)


def split_ops(b, bad):
    off = b["op_off"].astype(np.int64)
    new_ops, new_off = [], [0]
    for r in range(len(off) - 1):
        seg = b["ops"][int(off[r]):int(off[r + 1])].tolist()
        if r in bad:
            k = next(i for i in range(3, len(seg)) if (seg[i] >> 4) >= 2)
            w = seg[k]
            seg[k:k + 1] = [((w >> 4) - 1) << 4 | (w & 15), 1 << 4 | (w & 15)]
        new_ops += seg
        new_off.append(len(new_ops))
    b2 = dict(b)
    b2["ops"] = np.array(new_ops, np.uint32)
    b2["op_off"] = np.array(new_off, np.uint64)
    return b2
