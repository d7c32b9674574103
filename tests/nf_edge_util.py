"""Inputs of the nucfreq edge suite (test_nucfreq_edge_inputs.py proves on the CPU what they hold, test_gpu_nucfreq_edges.py runs them):
what lies AROUND a tile of rb_dev_nucfreq -- the list walkers' second tile, the prefix maximum's top level, regions that select nothing,
coordinates where 32 bits run out, the limits of the depth cap's bookkeeping, the resident entry's memory contract.

The expectation for counts and coverage is always the oracle (oracle.nucfreq, one call per region = per fetch, cached per distinct
region).  plan_tiles() below restates rb_k_nf_read_spans / rb_k_nf_plan_tiles in numpy; it only proves which build a tile takes and which
reads are in its range, never what a count should be."""
import functools
import heapq

import numpy as np

from nf_util import REF_OPS, Reads, oracle_region, random_reads

M, I, D, N, S = 0, 1, 2, 3, 4
TILE = 4096          # NF_TILE
SCAN_BLOCK = 2048    # NF_SCAN_PER_BLOCK: reads per block of the prefix maximum; its top level takes 64 blocks a turn
DEPTH_CAP = 8000     # RB_NF_DEPTH_CAP
LIVE_MAX = 15360     # NFA_LIVE: buffered reads rb_k_nf_admit can hold
PIECE = 10000        # the reference fetches 10 kb at a time: one device region = one fetch
COVERED = 0x80000000
RD_OK, RD_FILTERED, RD_BAD_CIGAR = 0, 1, 2
P31, P32 = 1 << 31, 1 << 32


def cig(*x):
    return [(l << 4) | o for l, o in x]


def pieces(regions, piece=PIECE):
    """regions of any length -> the pieces of at most 10000 positions the reference fetches"""
    out = []
    for t, st, en in regions:
        if en <= st:
            out.append((t, st, en))
        for s0 in range(st, en, piece):
            out.append((t, s0, min(s0 + piece, en)))
    return out


# ---- numpy restatement of the set-up kernels (CPU test only) -------------------------------------------------------------------
def read_spans(rd):
    """rb_k_nf_read_spans: -> (status [n], end [n] u64: pos + reference span, clamped to 2^32 - 1; 0 for reads that are not OK)"""
    if rd.n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    off = rd.op_off.astype(np.int64) - int(rd.op_off[0])
    code, ln = (rd.ops & 15).astype(np.int64), (rd.ops >> 4).astype(np.int64)
    isref = np.isin(code, sorted(REF_OPS))

    def per_read(v):
        c = np.concatenate([[0], np.cumsum(v)])
        return c[off[1:]] - c[off[:-1]]
    n_ops = off[1:] - off[:-1]
    span = per_read(np.where(isref, ln, 0))
    bad = (n_ops == 0) | (per_read(isref) == 0) | (per_read(isref & (ln == 0)) > 0) | (per_read(code > 8) > 0)
    if len(code):
        bad |= (n_ops == 1) & ~np.isin(code[np.minimum(off[:-1], len(code) - 1)], [0, 7, 8])
    bad |= (rd.pos < 0) | (rd.pos > P31 - 1) | (span > P31 - 1)
    filtered = (rd.tid < 0) | ((rd.flag & 0x704) != 0)
    status = np.where(filtered, RD_FILTERED, np.where(bad, RD_BAD_CIGAR, RD_OK))
    end = np.where(status == RD_OK, np.minimum(rd.pos + span, P32 - 1), 0).astype(np.uint64)
    return status, end


def plan_tiles(rd, regions):
    """rb_k_nf_tile_count / rb_k_nf_plan_tiles: -> int64 [n_tiles, 5] of (region, st, en, lo, hi): reads [lo, hi) are in the tile's range.
    lo = the first read whose prefix maximum of (tid << 32 | end) exceeds (tid, st); hi = the first read with (tid, pos) >= (tid, en)"""
    status, end = read_spans(rd)
    tid64 = rd.tid.astype(np.uint32).astype(np.uint64) << np.uint64(32)
    pmax = np.maximum.accumulate(np.where(status == RD_OK, tid64 | end, np.uint64(0)).astype(np.uint64)) if rd.n else np.zeros(0, np.uint64)
    poskey = tid64 | (rd.pos.astype(np.uint64) & np.uint64(0xFFFFFFFF))
    assert (poskey[1:] >= poskey[:-1]).all(), "the reads are not in file order"
    out = []
    for r, (t, st, en) in enumerate(regions):
        for s0 in range(st, en, TILE):
            s1 = min(s0 + TILE, en)
            lo = hi = 0
            if t >= 0 and s0 <= 0xFFFFFFFE and rd.n:
                k_st, k_en = np.uint64((t << 32) | s0), np.uint64((t << 32) | min(s1, 0xFFFFFFFF))
                lo = int(np.searchsorted(pmax, k_st, side="right"))
                hi = max(lo, int(np.searchsorted(poskey, k_en, side="left")))
            out.append((r, s0, s1, lo, hi))
    return np.array(out, np.int64).reshape(-1, 5)


def prefix_max(rd, carry=True):
    """the prefix maximum of (tid << 32 | end) as the three launches compute it: per block of 2048, the blocks' maxima 64 at a time.
    carry=False: what it would be if a turn of the top level started from nothing (to show that an input needs the carry)"""
    status, end = read_spans(rd)
    key = np.where(status == RD_OK, (rd.tid.astype(np.uint32).astype(np.uint64) << np.uint64(32)) | end, np.uint64(0)).astype(np.uint64)
    nb = scan_blocks(rd)
    pad = np.zeros(nb * SCAN_BLOCK, np.uint64)
    pad[:rd.n] = key
    inner = np.maximum.accumulate(pad.reshape(nb, SCAN_BLOCK), axis=1)
    before = np.zeros(nb, np.uint64)
    for b in range(1, nb):
        before[b] = 0 if (not carry and b % 64 == 0) else max(before[b - 1], inner[b - 1, -1])
    return np.maximum(inner, before[:, None]).reshape(-1)[:rd.n]


def first_above(pm, k):
    """the binary search of rb_k_nf_plan_tiles, probe for probe: the first index whose prefix maximum exceeds k (if pm is monotone)"""
    a, b = 0, len(pm)
    while a < b:
        mid = (a + b) >> 1
        if int(pm[mid]) > k:
            b = mid
        else:
            a = mid + 1
    return a


def tile_kinds(plan):
    """nf_tile_kind: 1 = byte counters + byte differences (launched over all tiles), 2 = byte counters + 16-bit differences (the list of
    rb_k_nf_tiles<true, false>), 0 = 16-bit counters (the list of rb_k_nf_tiles<false, false>)"""
    n = plan[:, 4] - plan[:, 3]
    return np.where(n <= 127, 1, np.where(n <= 255, 2, 0))


def scan_blocks(rd):
    return (rd.n + SCAN_BLOCK - 1) // SCAN_BLOCK


def most_buffered(rd, tid, st, en):
    """the header's rule for one fetch: the first read of a start position always enters, a later one unless 8000 are buffered (admitted
    before it, ending at or behind the position).  -> (the most reads buffered at once, how many were dropped)"""
    status, end = read_spans(rd)
    live, cur, most, dropped = [], None, 0, 0
    for i in np.flatnonzero((status == RD_OK) & (rd.tid == tid) & (rd.pos < en) & (end.astype(np.int64) > st)).tolist():
        p = int(rd.pos[i])
        if p != cur:
            cur, first = p, True
            while live and live[0] < p:
                heapq.heappop(live)
        if first or len(live) < DEPTH_CAP:
            heapq.heappush(live, int(end[i]))
        else:
            dropped += 1
        first = False
        most = max(most, len(live))
    return most, dropped


# ---- the expectation: the oracle, per region, cached -------------------------------------------------------------------------------
def expected(oracle, rd, regions, cache=None):
    """-> (covered [n_positions] bool, counts [n_positions, 4] u64) of the regions laid end to end, as the device lays them"""
    cache = {} if cache is None else cache
    cov, cnt = [np.zeros(0, bool)], [np.zeros((0, 4), np.uint64)]
    for t, st, en in regions:
        assert en - st <= PIECE, "one device region = one fetch of the reference"
        if (t, st, en) not in cache:
            cache[(t, st, en)] = oracle_region(oracle, rd, t, st, en)
        cov.append(cache[(t, st, en)][0]), cnt.append(cache[(t, st, en)][1])
    return np.concatenate(cov), np.concatenate(cnt)


def compare(counts, regions, cov, cnt, what=""):
    """device counts [n_positions, 4] u32 against expected(): bit-exact, coverage bit included; names the first region that differs"""
    assert counts.shape == (len(cov), 4), (what, counts.shape, len(cov))
    g = counts.astype(np.uint64)
    gcov = (g[:, 0] & COVERED) != 0
    g[:, 0] &= COVERED - 1
    wrong = (gcov != cov) | (g != cnt).any(axis=1)
    if wrong.any():
        k, o = int(np.flatnonzero(wrong)[0]), 0
        for r, (t, st, en) in enumerate(regions):
            if k < o + (en - st):
                raise AssertionError(f"{what}: region {r} ({t}, {st}, {en}) position {st + k - o}: device {g[k].tolist()} covered {bool(gcov[k])}, "
                                     f"oracle {cnt[k].tolist()} covered {bool(cov[k])}; {int(wrong.sum())} positions differ")
            o += en - st


# ---- case 1: the list walkers past their first tile ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walker_reads():
    """three piles of three-op reads (aM 2D bM) with starts uniform over 1500 positions: contig 0 deep enough for the 16-bit build (and
    the lane-per-read route), contig 1 for the middle build, contig 2 for the byte build"""
    rng = np.random.default_rng(1001)
    tid, pos, cigs, seqs = [], [], [], []
    for t, n in ((0, 2600), (1, 880), (2, 150)):
        for p in np.sort(rng.integers(0, 1500, n)).tolist():
            a, b = int(rng.integers(30, 201)), int(rng.integers(30, 201))
            tid.append(t), pos.append(p), cigs.append(cig((a, M), (2, D), (b, M))), seqs.append(rng.choice([1, 2, 4, 8, 15], size=a + b).tolist())
    return Reads(tid, pos, [0] * len(tid), cigs, seqs)


def walker_regions(n_per_list=1100):
    """n_per_list small regions on contig 0 and on contig 1 and about 100 on contig 2, drawn with repeats from a pool of 70 and shuffled;
    three regions of two and three tiles and a few empty ones among them"""
    rng = np.random.default_rng(1002)
    pool = sorted({(int(rng.integers(300, 1201)), int(rng.integers(1, 41))) for _ in range(80)})[:70]
    regions = []
    for t, n in ((0, n_per_list), (1, n_per_list), (2, 100)):
        for k in rng.integers(0, len(pool), n).tolist():
            regions.append((t, pool[k][0], pool[k][0] + pool[k][1]))
    regions += [(0, 100, 9100), (1, 0, 5000), (2, 500, 7500), (0, 700, 700), (1, 0, 0), (2, 1499, 1499), (1, 900, 900)]
    return [regions[k] for k in rng.permutation(len(regions)).tolist()]


# ---- case 2: the prefix maximum across its top level ----------------------------------------------------------------------------------
TOP_HEAD, TOP_TAIL = 6, 5          # reads in front of the tiny ones (five of one base, the long one), reads on contig 1 behind them
TOP_CASES = {                      # name -> (tiny reads, index of a second long read or None)
    "64_blocks": (64 * SCAN_BLOCK - TOP_HEAD - TOP_TAIL, None),   # the last size the top level takes in one turn
    "131072_tiny": (131072, None),                                # 65 blocks: block 64 holds six tiny reads
    "131073_tiny": (131073, None),
    "72_blocks": (72 * SCAN_BLOCK - TOP_HEAD - TOP_TAIL - 1, 70 * SCAN_BLOCK + 100),
    # the search for a tile's first read probes the middle of the file first, then the middle of a half: only with the second long read
    # behind the file's middle and in front of block 64, and a probe at or behind block 64, does a lost carry send the search the wrong way
    "88_blocks": (88 * SCAN_BLOCK - TOP_HEAD - TOP_TAIL - 1, 50 * SCAN_BLOCK + 100),
}


@functools.lru_cache(maxsize=2)
def top_input(name):
    """-> (Reads, regions, facts).  Five one-base reads, at index 5 the long read 5M <2n + 100>N 7M, n tiny reads (1M, two positions
    apart), a handful of reads on contig 1; optionally a second long read of the same shape further down"""
    n, second = TOP_CASES[name]
    rng = np.random.default_rng(2000 + n)
    long_cig, long_span = cig((5, M), (2 * n + 100, N), (7, M)), 5 + 2 * n + 100 + 7
    tid, pos, cigs, seqs = [0] * 5, [0, 1, 2, 3, 4], [cig((1, M))] * 5, [[1], [2], [4], [8], [1]]
    tid.append(0), pos.append(5), cigs.append(long_cig), seqs.append(rng.choice([1, 2, 4, 8], size=12).tolist())
    base = rng.choice([1, 2, 4, 8], size=n).tolist()
    long_at = [5]
    for k in range(n):
        if second is not None and len(tid) == second:
            long_at.append(len(tid))
            tid.append(0), pos.append(10 + 2 * k), cigs.append(long_cig), seqs.append(rng.choice([1, 2, 4, 8], size=12).tolist())
        tid.append(0), pos.append(10 + 2 * k), cigs.append(cig((1, M))), seqs.append([base[k]])
    n0 = len(tid)
    for k in range(TOP_TAIL):
        tid.append(1), pos.append(3 + 4 * k), cigs.append(cig((20, M))), seqs.append(rng.choice([1, 2, 4, 8], size=20).tolist())
    rd = Reads(tid, pos, [0] * len(tid), cigs, seqs)
    regions, tails = [], []
    for i in long_at:       # around a long read's last seven bases: beyond every tiny read
        e = pos[i] + long_span
        tails.append((i, len(regions), e))
        regions.append((0, e - 12, e + 5))
    last = [(0, pos[n0 - 10], pos[n0 - 1] + 3)]                      # inside the tiny reads of the last block
    seams = [b * SCAN_BLOCK for b in (63, 64, 70) if b * SCAN_BLOCK + 4 < n0]
    regions += last + [(0, pos[b - 4], pos[b + 4] + 1) for b in seams] + [(1, 0, 60)]
    return rd, regions, dict(n0=n0, long_at=long_at, tails=tails, seams=seams, n_tiny=n)


# ---- case 3: nothing selected ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nothing_input():
    """reads on contigs 0 and 2 (none on 1, none above 2), unplaced records at the end; more than 300 regions most of which select nothing"""
    rng = np.random.default_rng(3003)
    tid, pos, flag, cigs, seqs = [], [], [], [], []
    for t in (0, 2):
        for p in np.sort(rng.integers(0, 3000, 40)).tolist():
            a, b = int(rng.integers(30, 201)), int(rng.integers(30, 201))
            tid.append(t), pos.append(p), flag.append(0), cigs.append(cig((a, M), (3, D), (b, M))), seqs.append(rng.choice([1, 2, 4, 8], size=a + b).tolist())
    for fl, c, s in ((4, [], []), (4, [], [1, 2, 4]), (0, cig((10, M)), [1] * 10)):   # unplaced: tid -1, with and without a cigar
        tid.append(-1), pos.append(-1), flag.append(fl), cigs.append(c), seqs.append(s)
    rd = Reads(tid, pos, flag, cigs, seqs)
    last0, last2 = 3000 + 403, 3000 + 403      # no read reaches this far (pos < 3000, span <= 403)
    ordinary = [(0, 500, 700), (2, 100, 4300), (0, 2990, 3500), (2, 0, 1)]
    nothing = [(1, 100, 130), (1, 0, 4097), (5, 0, 50), (1000, 7, 9), (-1, 0, 40), (-1, 5, 6), (0, last0, last0 + 30), (2, 10 ** 6, 10 ** 6 + 7),
               (0, 50000, 50001), (2, P31, P31 + 3)]
    one = [(0, 600, 601), (2, 1500, 1501), (0, last0 - 1, last0), (0, 0, 1)]
    empty = [(0, 10, 10), (1, 0, 0), (-1, 0, 0), (7, 99, 99), (2, 10 ** 6, 10 ** 6), (0, 0, 0), (0, P32 + 5, P32 + 5)]

    def run(k, at):
        return [empty[(at + j) % len(empty)] for j in range(k)]
    regions = run(20, 0) + ordinary[:1] + run(2, 3) + ordinary[1:2] + run(1, 5) + ordinary[2:]          # the front
    k = 0
    while len(regions) < 150:
        regions += [nothing[k % len(nothing)], one[k % len(one)], nothing[(k + 3) % len(nothing)]]
        regions += ordinary[k % len(ordinary):k % len(ordinary) + 1] if k % 4 == 0 else []
        k += 1
    regions += run(1, 1) + ordinary[:1] + run(2, 2) + ordinary[3:] + run(20, 4) + ordinary[1:2]          # the middle
    while len(regions) < 300:
        regions += [one[k % len(one)], nothing[k % len(nothing)], nothing[(k + 5) % len(nothing)]]
        k += 1
    regions += ordinary[2:3] + run(1, 6) + ordinary[:1] + run(2, 0) + one[:1] + run(20, 2)                # the very end
    return rd, regions, dict(nothing=nothing, empty=empty, one=one, n_unplaced=3)


# ---- case 4: high coordinates --------------------------------------------------------------------------------------------------------
GIANT_N = (1 << 28) - 1


def giant_cigar(span):
    """3M, N ops of at most 2^28 - 1 each, 100M: a reference span of `span`"""
    n, ops = span - 103, [(3, M)]
    while n > 0:
        ops.append((min(n, GIANT_N), N))
        n -= min(n, GIANT_N)
    return cig(*(ops + [(100, M)]))


def giant_contribution(pos, span, seq, st, en):
    """what the read 3M <..>N 100M at pos adds to the pileup of [st, en), by hand (as test_long_ops.py does for its giant record): covered
    over its whole span, its bases where the two M ops lie.  -> (covered [en - st] bool, counts [en - st, 4] u64)"""
    cov, cnt = np.zeros(en - st, bool), np.zeros((en - st, 4), np.uint64)
    a, b = max(st, pos), min(en, pos + span)
    if a < b:
        cov[a - st:b - st] = True
    col = {1: 0, 2: 1, 4: 2, 8: 3}
    for q, x in [(k, pos + k) for k in range(3)] + [(3 + k, pos + span - 100 + k) for k in range(100)]:
        if st <= x < en and seq[q] in col:
            cnt[x - st, col[seq[q]]] += 1
    return cov, cnt


@functools.lru_cache(maxsize=None)
def high_input():
    """-> (Reads, regions, facts).  (a) about 40 reads with indels that start in [2^31 - 400, 2^31 - 1] and end past 2^31; (b) the giant read:
    pos 2^31 - 1, span 2^31 - 1, end 2^32 - 2; (c) two reads the device declines: a span of 2^31, and pos = 2^31"""
    rng = np.random.default_rng(4004)
    recs = []
    for p in sorted(rng.integers(P31 - 400, P31 - 1, 39).tolist()) + [P31 - 1]:
        c = []
        for _ in range(int(rng.integers(3, 9))):
            c += [(int(rng.integers(40, 160)), M), [(int(rng.integers(1, 9)), I), (int(rng.integers(1, 9)), D), (int(rng.integers(1, 300)), N)][int(rng.integers(0, 3))]]
        c.append((int(rng.integers(400, 500)), M))
        q = sum(l for l, o in c if o in (M, I))
        recs.append((p, cig(*c), rng.choice([1, 2, 4, 8, 15], size=q).tolist()))
    n_a = len(recs)
    giant_seq = rng.choice([1, 2, 4, 8], size=103).tolist()
    decl_seq = rng.choice([1, 2, 4, 8], size=103).tolist()
    recs.append((P31 - 1, giant_cigar(P31 - 1), giant_seq))                 # (b) index n_a: behind every other read of its start position
    recs.append((P31 - 350, giant_cigar(P31), decl_seq))                      # (c) a span of 2^31
    recs.sort(key=lambda r: r[0])                                             # (stable: the declined read goes in among (a))
    recs.append((P31, cig((50, M)), rng.choice([1, 2, 4, 8], size=50).tolist()))   # (c) pos = 2^31
    rd = Reads([0] * len(recs), [r[0] for r in recs], [0] * len(recs), [r[1] for r in recs], [r[2] for r in recs])
    giant = max(i for i, r in enumerate(recs) if r[2] is giant_seq)
    declined = sorted([i for i, r in enumerate(recs) if r[2] is decl_seq] + [len(recs) - 1])
    end = P32 - 2
    regions = [(0, P31 - 500, P31 + 300), (0, P31 - 1, P31), (0, P31, P31 + 1), (0, P31 - 4097, P31 + 4097),    # straddling 2^31
               (0, P31 + 300, P31 + 1500), (0, P31 - 350, P31 - 340),
               (0, end - 150, end + 40), (0, end - 100, end), (0, end - 1, end), (0, end, end + 10),              # the giant read's last hundred bases
               (0, P31 + (1 << 30), P31 + (1 << 30) + 50),                                                         # deep inside its N ops
               (0, end - 4096 - 50, end - 30), (0, P32 - 60, P32 + 30)]
    return rd, regions, dict(n_a=n_a, giant=giant, declined=declined, giant_seq=giant_seq, giant_pos=P31 - 1, giant_span=P31 - 1)


def without(rd, drop):
    """the same reads without those at the indices of drop (for the oracle: reads the device declines, the read worked out by hand)"""
    keep = [i for i in range(rd.n) if i not in set(drop)]
    cigs = [rd.ops[int(rd.op_off[i]):int(rd.op_off[i + 1])].tolist() for i in keep]
    seqs = []
    for i in keep:
        b = rd.seq[int(rd.seq_off[i]):int(rd.seq_off[i]) + (int(rd.l_seq[i]) + 1) // 2]
        seqs.append(np.stack([b >> 4, b & 15], axis=1).reshape(-1)[:int(rd.l_seq[i])].tolist())
    return Reads(rd.tid[keep], rd.pos[keep], rd.flag[keep], cigs, seqs)


def high_expected(oracle, cache=None):
    """the oracle on the reads of (a) + the giant read's contribution by hand (pileups add up below the cap); the declined reads add nothing"""
    rd, regions, f = high_input()
    cov, cnt = expected(oracle, without(rd, [f["giant"]] + f["declined"]), regions, cache)
    cov, cnt, o = cov.copy(), cnt.copy(), 0
    for t, st, en in regions:
        gc, gn = giant_contribution(f["giant_pos"], f["giant_span"], f["giant_seq"], st, en)
        cov[o:o + en - st] |= gc
        cnt[o:o + en - st] += gn
        o += en - st
    return cov, cnt


# ---- case 5: the depth cap's bookkeeping at its limits ----------------------------------------------------------------------------------
CAP_REGION = (0, 0, 9000)


@functools.lru_cache(maxsize=None)
def cap_input(n_starts=7360, n_filtered=0):
    """reads 1M <7600>N 1M: 8000 on position 0, one on each of the positions 1 .. n_starts, a second one (dropped) on every tenth; optionally
    reads of flag 0x400 mixed into position 0 in front of the 8000th passing read"""
    rng = np.random.default_rng(5005)
    c = cig((1, M), (7600, N), (1, M))
    pos = [0] * DEPTH_CAP
    flag = [0] * DEPTH_CAP
    for k in sorted(rng.integers(0, 7000, n_filtered).tolist(), reverse=True):
        pos.insert(k, 0), flag.insert(k, 0x400)
    for p in range(1, n_starts + 1):
        pos += [p] * (2 if p % 10 == 0 else 1)
    flag += [0] * (len(pos) - len(flag))
    seqs = rng.choice([1, 2, 4, 8], size=(len(pos), 2)).tolist()
    return Reads([0] * len(pos), pos, flag, [c] * len(pos), seqs)


@functools.lru_cache(maxsize=None)
def pool_reads():
    """the 8100 reads on one start position of test_gpu_nucfreq.py::test_depth_cap_one_start_position"""
    n = 8100
    seqs = np.random.default_rng(3).choice([1, 2, 4, 8], size=(n, 4)).tolist()
    return Reads([0] * n, [5] * n, [0] * n, [cig((4, M))] * n, seqs)


# ---- case 6: the resident entry's contract ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contract_input():
    """the reads and regions of test_gpu_nucfreq.py::test_random_reads_all_op_types (seed 0), the regions in the reference's 10 kb pieces"""
    rng = np.random.default_rng(77)
    rd = random_reads(rng, 300, n_contig=3, span=30000, long_frac=0.1)
    regions = []
    for _ in range(6):
        t = int(rng.integers(0, 3))
        st = int(rng.integers(0, 35000))
        regions.append((t, st, st + int(rng.integers(1, 20000))))
    regions += [(0, 4095, 4097), (1, 0, 4096), (2, 8192, 8193), (0, 60000, 60010)]
    return rd, pieces(regions)


# ---- the resident-buffer harness ------------------------------------------------------------------------------------------------------
SENT, SENT_BYTE = 4096, 0xA5


class DevBuf:
    """`nbytes` of payload in a device tensor that goes on for SENT bytes of sentinel: what is written behind the payload shows"""

    def __init__(self, torch, dev, nbytes, host=None, fill=0):
        self.n = int(nbytes)
        h = np.full(self.n + SENT, SENT_BYTE, np.uint8)
        h[:self.n] = fill if host is None else np.frombuffer(host.tobytes(), np.uint8)
        self.host = h
        self.t = torch.from_numpy(h.copy()).to(dev)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def sentinel_ok(self, h=None):
        return bool(((self.get() if h is None else h)[self.n:] == SENT_BYTE).all())

    def unchanged(self):
        return bool(np.array_equal(self.get(), self.host))


class Resident:
    """reads and regions resident in HBM, every array exactly as long as the header says (seq: 32 readable bytes behind the last read, here
    0xEE), a sentinel behind each.  run() allocates counts / read_status / counters / workspace afresh, prefilled with a byte"""

    def __init__(self, ctx, rd, regions):
        self.torch, self.eng, self.dev = ctx
        self.rd, self.rg = rd, np.array(regions, np.int64).reshape(-1, 3)
        self.out_off = np.concatenate([[0], np.cumsum(self.rg[:, 2] - self.rg[:, 1])]).astype(np.uint64)
        self.n_pos, self.n_rg = int(self.out_off[-1]), len(self.rg)
        o0 = int(rd.op_off[0]) if rd.n else 0
        seq_end = int((rd.seq_off + (rd.l_seq.astype(np.uint64) + np.uint64(1)) // np.uint64(2)).max()) if rd.n else 0
        seq = np.concatenate([rd.seq[:seq_end], np.full(32 + (-seq_end) % 4, 0xEE, np.uint8)])
        arrays = dict(ops=rd.ops[o0:int(rd.op_off[-1])] if rd.n else np.zeros(0, np.uint32), op_off=rd.op_off - np.uint64(o0), seq=seq,
                      seq_off=rd.seq_off, l_seq=rd.l_seq, tid=rd.tid, pos=rd.pos, flag=rd.flag,
                      rg_tid=self.rg[:, 0].astype(np.int32), rg_st=self.rg[:, 1].astype(np.uint64), rg_en=self.rg[:, 2].astype(np.uint64),
                      out_off=self.out_off)
        self.inp = {k: DevBuf(self.torch, self.dev, np.ascontiguousarray(v).nbytes, np.ascontiguousarray(v)) for k, v in arrays.items()}
        self.ws_bytes = self.eng.nucfreq_workspace_bytes(rd.n, self.n_rg, self.n_pos)
        self.out = None

    def run(self, prefill=0xEE, ws_short=0, ws_shift=0):
        """one rb_dev_nucfreq call -> (counts [n_positions, 4] u32, read_status [n_reads] u32, counters dict); the four sentinels are checked"""
        T, dev, i = self.torch, self.dev, self.inp
        self.out = dict(counts=DevBuf(T, dev, 16 * self.n_pos, fill=prefill), status=DevBuf(T, dev, 4 * self.rd.n, fill=prefill),
                        counters=DevBuf(T, dev, 48, fill=prefill), ws=DevBuf(T, dev, self.ws_bytes, fill=prefill))
        o = self.out
        T.cuda.synchronize()
        self.eng.dev_nucfreq(self.rd.n, i["ops"].ptr, i["op_off"].ptr, i["seq"].ptr, i["seq_off"].ptr, i["l_seq"].ptr, i["tid"].ptr, i["pos"].ptr,
                             i["flag"].ptr, self.n_rg, i["rg_tid"].ptr, i["rg_st"].ptr, i["rg_en"].ptr, i["out_off"].ptr, self.n_pos,
                             o["counts"].ptr, o["status"].ptr, o["counters"].ptr, o["ws"].ptr + ws_shift, self.ws_bytes - ws_short)
        T.cuda.synchronize()
        h = self.last = {k: b.get() for k, b in o.items()}
        for k, b in o.items():
            assert b.sentinel_ok(h[k]), f"rb_dev_nucfreq wrote behind {k}"
        c = h["counters"][:48].view(np.uint64)
        ctr = dict(max_depth=int(c[0]), n_covered=int(c[1]), n_bad=int(c[2]), unsorted=int(c[3]), n_dropped=int(c[4]), cap_overflow=int(c[5]))
        return h["counts"][:16 * self.n_pos].view(np.uint32).reshape(-1, 4).copy(), h["status"][:4 * self.rd.n].view(np.uint32).copy(), ctr

    def outputs_untouched(self):
        """after a refused call: counts, read_status, counters and the workspace still hold what run() put there"""
        self.torch.cuda.synchronize()
        return all(b.unchanged() for b in self.out.values())

    def inputs_unchanged(self):
        return all(b.unchanged() for b in self.inp.values())
