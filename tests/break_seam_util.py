"""Inputs of the break-paf seam tests (tests/test_break_seam_inputs.py, tests/test_gpu_break_seams.py) and a plain restatement of the cut
rule (liftover.rs:182-226), none of it taken from the kernels.

The cut detection exists three times: rb_k_break_pieces (k_misc.hip: 8 ops a lane and 512 a step, counted from the record's 16-byte
group; at most CAP pieces of a record collected in LDS), the BRK build of rb_stream_record (rb_stream.h: the flat step of 512 ops counted
from the record's 128-byte line, segments of 5120 ops, 32 pieces a pass) and the BRK build of the tile kernel (k_tile.hip: up to TILE_REC
records and TILE_HITS pieces a tile).  planted() puts long indels on chosen ops of a regular record; the families lay them on those seams.

Assumption of family E, held by the `phase` asserts of the GPU test: rb_plan_create puts consecutive records of 8 .. 2048 ops into one tile
while they are at most rb_tile_max_records() = RBT_REC and rb_tile_max_ops() = RBT_OPS - 32 ops together.  The constants are read from
k_tile.hip's defines, not through the GPU library.
"""
import os
import re

import numpy as np

from rbtest_util import OPC, sums
from test_gpu_stream_flat import HEADS, LENGTHS, T_GAP, _place

EQ, X, I, D, S, M = OPC["="], OPC["X"], OPC["I"], OPC["D"], OPC["S"], OPC["M"]
BIG = 150                    # length of a planted indel; every other I / D has at most 3 bases
MAX_SIZES = (100, BIG - 1, BIG, 0)
STEP, SEGMENT, PASS = 512, 5120, 32   # ops a step, ops a segment, pieces a pass of the stream kernel
CAP = 512                    # RB_BP_CAP: pieces of a record the collect pass of rb_k_break_pieces keeps
STREAM_CLASSES = (4, 8, 16, 256, 512, 5120)   # 4-op group, capture pair, granule, half step, step, segment
PIECES_CLASSES = (8, 512)                      # a lane's ops and a step of rb_k_break_pieces
# seam starts counted from the stream kernel's g0; the + 4 entries are seams of rb_k_break_pieces for the heads that are no multiple of 4 .. 8
SEAMS = [4, 8, 12, 16, 256, 260, 512, 516, 768, 5120, 5124, 5376]
VARIANTS = ("before", "behind", "both")


def _define(name, text):
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M).group(1))


with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustybam_amd", "csrc", "k_tile.hip")) as _f:
    _t = _f.read()
TILE_REC, TILE_OPS, TILE_HITS = _define("RBT_REC", _t), _define("RBT_OPS", _t) - 32, _define("RBT_HITS", _t)
del _f, _t


# ------------------------------------------------------------------------------------------------ the cut rule, restated
def cuts(cig, max_size):
    """-> (op index of the cut that closes piece j, for every piece a cut closes; is there a last piece behind the last cut).
    One walk with pre / R: an I / D longer than max_size closes the piece [pre, R) if R > pre and moves pre behind itself; what lies
    behind the last long indel is a piece if Rtot > pre."""
    pre = R = 0
    closing = []
    for k, w in enumerate(np.asarray(cig).tolist()):
        c, ln = w & 15, w >> 4
        ref = ln if c in (M, D, EQ, X, OPC["N"]) else 0
        if c in (I, D) and ln > max_size:
            if R > pre:
                closing.append(k)
            pre = R + ref
        R += ref
    return closing, R > pre


def n_pieces(cig, max_size):
    closing, last = cuts(cig, max_size)
    return len(closing) + int(last)


def is_regular(cig, ends=True):
    c, ln = np.asarray(cig) & 15, np.asarray(cig) >> 4
    ok = bool((ln > 0).all() and (c[1:] != c[:-1]).all() and np.isin(c, (M, I, D, OPC["N"], EQ, X)).all())
    return ok and (not ends or (int(c[0]) in (M, EQ, X) and int(c[-1]) in (M, EQ, X)))


# ------------------------------------------------------------------------------------------------ the generator
def planted(n_ops, head, longs, big=BIG, max_size=3, seed=None):
    """a regular record of exactly n_ops ops: the op at index g - head is an I or D (in turn) of `big` bases for every g in longs, every
    other op is = (3 .. 9 bases) or an X / I / D of 1 .. min(3, max_size) bases; no two neighbours of one type, match ops at both ends"""
    at = sorted({int(g) - head for g in longs})
    assert all(0 < k < n_ops - 1 for k in at), (n_ops, head, at[:3], at[-3:])
    assert max_size >= 1
    rng = np.random.default_rng(7919 * n_ops + head if seed is None else seed)
    is_long = np.zeros(n_ops + 1, bool)
    is_long[at] = True
    small = rng.integers(0, 3, n_ops)
    s_len = rng.integers(1, min(3, max_size) + 1, n_ops)
    e_len = rng.integers(3, 10, n_ops)
    ops, prev, turn = [], -1, 0
    for i in range(n_ops):
        if is_long[i]:
            c, ln = (I, D)[turn % 2], big
            turn += 1
        elif prev == EQ:
            # (match-type where a long indel or the record's end follows: the planted indels keep their turn, the ends are match ops)
            c = X if (i == n_ops - 1 or is_long[i + 1]) else (X, I, D)[small[i]]
            ln = int(s_len[i])
        else:
            c, ln = EQ, int(e_len[i])
        assert c != prev
        ops.append((ln << 4) | c)
        prev = c
    return np.array(ops, np.uint32)


def make_batch(cigs, strands="+-"):
    """records T_GAP apart on one contig, the strands in turn"""
    n = len(cigs)
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    t_st = 1000 + T_GAP * np.arange(n, dtype=np.uint64)
    RQ = [sums(c) for c in cigs]
    R, Q = np.array([x[0] for x in RQ], np.uint64), np.array([x[1] for x in RQ], np.uint64)
    q_st = np.arange(n, dtype=np.uint64) * 7
    strand = np.array([ord(strands[i % len(strands)]) for i in range(n)], np.uint8)
    return dict(ops=np.concatenate(cigs), op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=q_st, q_en=q_st + Q, strand=strand, contig=np.zeros(n, np.uint32))


def records(b, idx=None):
    off = b["op_off"].astype(np.int64)
    return [b["ops"][off[r]:off[r + 1]] for r in (range(len(off) - 1) if idx is None else idx)]


# ------------------------------------------------------------------------------------------------ A / F: seams of the layouts
def seam_longs(variant, head, n_ops):
    """ops (counted from g0) that carry a long indel: the last op before each seam, the first behind it, or both"""
    gs = set()
    for g in SEAMS:
        gs |= {"before": {g - 1}, "behind": {g}, "both": {g - 1, g}}[variant]
    return sorted(g for g in gs if 0 < g - head < n_ops - 1)


def family_a(variant, soft=False):
    """-> (batch, indices of the placed records): the records of tests/test_gpu_stream_flat.py with long indels at the seams; soft (family
    F): a 5S in front of every placed record, which makes it irregular and leaves its pieces as they are"""
    placed = []
    for n, h in zip(LENGTHS, HEADS):
        if soft:
            c = np.concatenate([np.array([(5 << 4) | S], np.uint32), planted(n - 1, h + 1, seam_longs(variant, h + 1, n - 1))])
        else:
            c = planted(n, h, seam_longs(variant, h, n))
        placed.append((c, h))
    b, idx = _place(placed)
    if soft:  # (_place counts every op but I on the reference: clipped bases are query bases alone)
        b["t_en"][idx] -= np.uint64(5)
    return b, idx


def seam_sides(cig, unit_head, classes, max_size=BIG - 1):
    """which seam classes a long indel of `cig` touches: -> (classes with one on the last op before a seam, classes with one on the first
    op behind it).  Ops are counted from `unit_head` ops in front of the record (the stream kernel: op_off % 32, rb_k_break_pieces:
    op_off % 4); a seam's class is the largest of `classes` that divides it."""
    c, ln = np.asarray(cig) & 15, np.asarray(cig) >> 4
    k = np.flatnonzero(((c == I) | (c == D)) & (ln > max_size)) + unit_head

    def cls(g):
        return {max(x for x in classes if s % x == 0) for s in g.tolist() if any(s % x == 0 for x in classes)}
    return cls(k + 1), cls(k)


# ------------------------------------------------------------------------------------------------ B: pass boundaries of the stream kernel
def _spread(n, lo, hi):
    p = np.linspace(lo, hi, n).astype(int).tolist()
    assert len(set(p)) == n and min(np.diff(p), default=9) > 2
    return p


def _tail(at):
    return [at + 37 * (j + 1) for j in range(40)]


def tiny_record(tiny_at):
    """tests/test_gpu_break_onewalk.py::test_many_pieces_in_several_passes: 70 long deletions, piece `tiny_at` is one M op of one base"""
    cig = []
    for k in range(70):
        cig += [((1 if k == tiny_at else 300 + k) << 4) | M] + ([(2 << 4) | I, (250 << 4) | M] if k != tiny_at else []) + [(500 << 4) | D]
    cig.append((40 << 4) | M)
    return np.array(cig, np.uint32)


def family_b():
    """-> {name: (record, pieces at BIG - 1, op of the cut that closes piece 31 or None)}; every record a multiple of 32 ops long, so that in a
    batch of them every record starts a line and op k of the record is op k from g0"""
    seg0 = _spread(31, 100, 4900)
    out = {}
    for name, c32, n in (("cut32_at_5119", [5119], 6656), ("cut32_at_5120", [5120], 6656), ("cut32_run_5119_5120", [5119, 5120], 6656),
                         ("cut32_seg1_middle", [7700], 10752)):
        out[name] = (planted(n, 0, seg0 + c32 + _tail(c32[-1])), 73, c32[0])
    out["cut32_early"] = (planted(5632, 0, [20 + 19 * i for i in range(31)] + [610] + _tail(610)), 73, 610)
    for k in (32, 33, 64, 65, 97):
        p = _spread(k - 1, 50, 5550)
        out[f"pieces_{k}"] = (planted(5632, 0, p), k, p[31] if k > 32 else None)
    out["last_piece_one_op"] = (planted(5632, 0, [700, 2600, 5121, 5400, 5630]), 6, None)
    return out


# ------------------------------------------------------------------------------------------------ C: record ends
def family_c():
    """-> (batch, per record: (lead, trail) op counts of the indel runs around the regular body).  Long and short indel runs in front of and
    behind bodies of 5300, 2101 and 77 ops that also have a long indel on their second op and their last op but one."""
    w = lambda ln, c: (ln << 4) | c  # noqa: E731
    runs = [(), (w(BIG, I),), (w(BIG, D),), (w(BIG, I), w(BIG, D)), (w(2, D), w(BIG, I)), (w(3, I),)]
    cigs, ends = [], []
    for i, lead in enumerate(runs):
        for j, trail in enumerate(runs):
            if (i + j) % 2 and i and j:
                continue
            n = (5300, 2101, 77)[(i + 2 * j) % 3]
            body = planted(n, 0, [1, n // 3, n // 3 + 1, n - 2], seed=100 * i + j)
            cigs.append(np.concatenate([np.array(lead, np.uint32), body, np.array(trail, np.uint32)]).astype(np.uint32))
            ends.append((len(lead), len(trail)))
    return make_batch(cigs), ends


# ------------------------------------------------------------------------------------------------ D: the collect cap
def cap_record(n_cut):
    ops = []
    for k in range(n_cut):
        ops += [(3 << 4) | EQ, (BIG << 4) | (I, D)[k % 2]]
    return np.array(ops + [(3 << 4) | EQ], np.uint32)


CAP_CUTS = (CAP - 2, CAP - 1, CAP)


def family_d_batch():
    """70 records: the three cap records at 11, 12 (neighbours) and 40, the others of 40 .. 250 ops with no cut or one"""
    cigs, want = [], []
    at = {11: CAP_CUTS[2], 12: CAP_CUTS[0], 40: CAP_CUTS[1]}
    for r in range(70):
        if r in at:
            cigs.append(cap_record(at[r])), want.append(at[r] + 1)
        else:
            n = 40 + 3 * r
            cigs.append(planted(n, 0, [n // 2] if r % 2 else [])), want.append(1 + r % 2)
    return make_batch(cigs), want


# ------------------------------------------------------------------------------------------------ E: tiles
TILE_LENGTHS = [41, 43, 58, 77, 120, 40, 95, 66, 51, 84, 49, 110, 63, 72, 45, 101, 57, 88, 42, 69, 93, 54, 47, 118]


def family_e(pieces):
    """24 records of 40 .. 120 ops, one tile, with `pieces` pieces together: every record has one or two long indels, on its second op, its
    last op but one or its middle, in turn"""
    n_rec = len(TILE_LENGTHS)
    total = pieces - n_rec
    assert n_rec <= total <= 3 * n_rec
    cigs = []
    for r, n in enumerate(TILE_LENGTHS):
        k = total // n_rec + (1 if r < total % n_rec else 0)
        spots = [1, n - 2, n // 2]
        cigs.append(planted(n, 0, [spots[(r + j) % 3] for j in range(k)], seed=500 + r))
    return make_batch(cigs)
