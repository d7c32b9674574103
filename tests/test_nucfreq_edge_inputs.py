"""What the inputs of test_gpu_nucfreq_edges.py hold, proved on the CPU (no GPU): which build of the tile kernel every tile takes and how
long the two tile lists get, how many blocks the prefix maximum has and where the long reads sit, which regions select nothing, the spans
and ends around 2^31 and 2^32, how many reads the depth cap's replay has to buffer.  plan_tiles() is a numpy restatement of the set-up
kernels and is used for nothing else; what a position counts is the oracle's business."""
import numpy as np
import pytest

import nf_edge_util as nu
from nf_edge_util import P31, P32


def test_walker_lists_are_longer_than_any_grid(oracle):
    rd = nu.walker_reads()
    regions = nu.walker_regions()
    assert all(en - st <= nu.PIECE for _t, st, en in regions)
    plan = nu.plan_tiles(rd, regions)
    kind, n_in = nu.tile_kinds(plan), plan[:, 4] - plan[:, 3]
    tid = np.array([regions[r][0] for r in plan[:, 0]])
    # the 16-bit build's list and the middle build's: each longer than three workgroups on each of 256 compute units would take in one go
    assert (kind == 0).sum() >= 1100 and (kind == 2).sum() >= 1100 and (kind == 1).sum() >= 100
    assert (n_in[kind == 0] > 512).sum() >= 1100, "the 16-bit build's tiles are past the lane-per-read threshold"
    small = np.array([regions[r][2] - regions[r][1] <= 40 for r in plan[:, 0]])
    assert set(kind[small & (tid == 0)]) == {0} and set(kind[small & (tid == 1)]) == {2} and set(kind[small & (tid == 2)]) == {1}
    assert 500 < n_in[small & (tid == 0)].min() and n_in[small & (tid == 0)].max() < 800
    assert 128 <= n_in[small & (tid == 1)].min() and n_in[small & (tid == 1)].max() <= 255
    assert n_in[small & (tid == 2)].max() <= 127
    # regions of two and three tiles; their far tiles hold no read
    per_region = np.bincount(plan[:, 0], minlength=len(regions))
    assert sorted(per_region[per_region > 1].tolist()) == [2, 2, 3] and (per_region == 0).sum() == 4
    assert (n_in == 0).sum() >= 3
    # the two lists grow towards each other in one array of max_tiles + 2 words: they fit, and lie interleaved in tile order
    n_pos = sum(en - st for _t, st, en in regions)
    assert (kind != 1).sum() <= n_pos // nu.TILE + len(regions)
    assert len(set(np.flatnonzero(np.diff(kind)).tolist())) > 500
    # the pool is small: the oracle answers 2300 regions with about 200 fetches
    assert len(set(regions)) < 230
    cache = {}
    cov, cnt = nu.expected(oracle, rd, regions, cache)
    assert len(cov) == n_pos and len(cache) == len(set(regions))
    assert cnt.sum(axis=1).max() > 255 and n_pos // 2 < cov.sum() < n_pos


@pytest.mark.parametrize("name", list(nu.TOP_CASES))
def test_prefix_maximum_top_level(oracle, name):
    rd, regions, f = nu.top_input(name)
    want_blocks = {"64_blocks": 64, "131072_tiny": 65, "131073_tiny": 65, "72_blocks": 72, "88_blocks": 88}[name]
    assert nu.scan_blocks(rd) == want_blocks
    assert f["n_tiny"] == {"64_blocks": 131061, "131072_tiny": 131072, "131073_tiny": 131073, "72_blocks": 147444, "88_blocks": 180212}[name]
    assert f["long_at"][0] == 5 and f["long_at"][0] < nu.SCAN_BLOCK
    if want_blocks > 65:
        assert f["long_at"][1] // nu.SCAN_BLOCK == (70 if name == "72_blocks" else 50) and f["seams"] == [63 * 2048, 64 * 2048, 70 * 2048]
    elif want_blocks == 65:
        assert f["seams"] == [63 * 2048, 64 * 2048] and f["n0"] > 64 * 2048 + 4   # tiny reads of contig 0 in block 64: they need the carry
    else:
        assert f["seams"] == [63 * 2048] and rd.n == 64 * 2048
    status, end = nu.read_spans(rd)
    assert (status == nu.RD_OK).all()
    plan = nu.plan_tiles(rd, regions)
    assert len(plan) == len(regions)
    lo, hi = plan[:, 3], plan[:, 4]
    # every region of contig 0 in front of the first long read's end needs that read: its tiles' range starts at index 5, whatever block
    # the tiny reads around it are in; behind that end the range starts at the second long read; contig 1 starts behind all of contig 0
    e0 = int(end[5])
    for r, (t, st, en) in enumerate(regions):
        if t == 0 and st < e0:
            assert lo[r] == 5, (r, lo[r])
        elif t == 0:
            assert lo[r] == f["long_at"][1]
        else:
            assert lo[r] == f["n0"] and hi[r] == rd.n
    # what the carry of the top level is worth: without it the prefix maximum of the contig-0 reads in blocks 64 .. falls short (64 blocks:
    # one turn, nothing to carry).  The search probes the file's middle first, so only the 88-block input, whose second long read sits
    # behind the middle and in front of block 64, sends a search the wrong way when the carry is lost: a tile would start behind that read
    pm, pm_lost = nu.prefix_max(rd), nu.prefix_max(rd, carry=False)
    assert np.array_equal(pm, np.maximum.accumulate(pm)) and int(pm[5]) == e0
    need = np.flatnonzero(pm != pm_lost)
    if want_blocks == 64:
        assert need.size == 0
    else:
        assert need.size >= 6 and need.min() == 64 * nu.SCAN_BLOCK and (rd.tid[need] == 0).all()
    if name == "88_blocks":
        i2, r2, e2 = f["tails"][1]
        assert rd.n // 2 < i2 < 64 * nu.SCAN_BLOCK and lo[r2] == i2 == nu.first_above(pm, regions[r2][1]) < nu.first_above(pm_lost, regions[r2][1])
    last = len(f["long_at"])
    assert hi[last] == f["n0"] and hi[last] - 1 >= (want_blocks - 1) * nu.SCAN_BLOCK - nu.TOP_TAIL   # the last block's tiny reads
    # the far regions are covered by exactly the long read: its last seven bases count one each, the N op in front of them counts nothing
    for i, r, e in f["tails"]:
        cov, cnt = nu.expected(oracle, rd, [regions[r]])
        under_next = i != f["long_at"][-1]       # (the first long read's end lies under the second one's N op: covered, nothing counted)
        assert cov.tolist() == [True] * 12 + [under_next] * 5
        assert cnt.sum(axis=1).tolist() == [0] * 5 + [1] * 7 + [0] * 5
        assert int(end[i]) == e and int(rd.pos[:f["n0"]].max()) + 1 < e - 7
    # contig 1's low region does not see contig 0's long reads
    cov, cnt = nu.expected(oracle, rd, [regions[-1]])
    assert regions[-1] == (1, 0, 60) and cnt.sum(axis=1).max() <= 5 and cov.tolist() == [False] * 3 + [True] * 36 + [False] * 21


def test_regions_that_select_nothing(oracle):
    rd, regions, f = nu.nothing_input()
    assert len(regions) >= 300
    status, end = nu.read_spans(rd)
    assert (status[-f["n_unplaced"]:] == nu.RD_FILTERED).all() and (rd.tid[-f["n_unplaced"]:] == -1).all() and (status[:-f["n_unplaced"]] == nu.RD_OK).all()
    assert set(rd.tid.tolist()) == {0, 2, -1}
    e = np.array([en <= st for _t, st, en in regions])
    runs, k = [], 0
    while k < len(e):           # runs of consecutive empty regions: (first, length)
        if e[k]:
            j = k
            while j < len(e) and e[j]:
                j += 1
            runs.append((k, j - k))
            k = j
        else:
            k += 1
    assert runs[0] == (0, 20) and runs[-1] == (len(regions) - 20, 20)
    assert sorted(l for _k, l in runs) == [1, 1, 1, 2, 2, 2, 20, 20, 20]
    assert [l for k, l in runs if 100 < k < 250] == [1, 2, 20]
    tids = {t for t, _s, _e in regions}
    assert {-1, 0, 1, 2, 5, 1000} <= tids
    cache = {}
    cov, cnt = nu.expected(oracle, rd, regions, cache)
    for rg in f["nothing"] + f["empty"]:
        assert rg in regions and (rg[2] == rg[1] or not cache[rg][0].any())
    assert sum(regions.count(rg) for rg in f["one"]) > 50 and any(cache[rg][0].any() for rg in f["one"]) and not all(cache[rg][0].any() for rg in f["one"])
    assert 0 < cov.sum() < len(cov) and cnt.sum() > 0
    plan = nu.plan_tiles(rd, regions)
    assert (plan[:, 3] == plan[:, 4]).sum() > 100 and len(plan) > 256


def test_high_coordinates(oracle):
    rd, regions, f = nu.high_input()
    status, end = nu.read_spans(rd)
    span = [sum(int(w) >> 4 for w in rd.ops[int(rd.op_off[i]):int(rd.op_off[i + 1])] if (int(w) & 15) in (0, 2, 3, 7, 8)) for i in range(rd.n)]   # Python ints
    pos = [int(p) for p in rd.pos]
    g = f["giant"]
    assert pos[g] == P31 - 1 and span[g] == P31 - 1 and pos[g] + span[g] == P32 - 2 and int(end[g]) == P32 - 2 and status[g] == nu.RD_OK
    assert max(int(w) >> 4 for w in rd.ops[int(rd.op_off[g]):int(rd.op_off[g + 1])]) == (1 << 28) - 1 and int(rd.op_off[g + 1] - rd.op_off[g]) == 10
    d0, d1 = f["declined"]
    assert span[d0] == P31 and pos[d0] == P31 - 350 and pos[d1] == P31 and span[d1] == 50 and d1 == rd.n - 1
    assert [i for i in range(rd.n) if status[i] != nu.RD_OK] == [d0, d1] and status[d0] == status[d1] == nu.RD_BAD_CIGAR and end[d0] == end[d1] == 0
    a = [i for i in range(rd.n) if i not in (g, d0, d1)]
    assert len(a) == f["n_a"] == 40 and all(P31 - 400 <= pos[i] <= P31 - 1 and pos[i] + span[i] > P31 and int(end[i]) == pos[i] + span[i] for i in a)
    assert sum(pos[i] == P31 - 1 for i in a) == 1 and pos == sorted(pos)
    assert any(st < P31 < en for _t, st, en in regions) and any(st < P32 < en for _t, st, en in regions) and all(en - st <= nu.PIECE for _t, st, en in regions)
    # every region's tile range holds the reads that reach it; the giant read is in the range of every tile between its start and its end
    plan = nu.plan_tiles(rd, regions)
    for r, s0, s1, lo, hi in plan.tolist():
        reach = [i for i in range(rd.n) if status[i] == nu.RD_OK and pos[i] < s1 and pos[i] + span[i] > s0]
        assert all(lo <= i < hi for i in reach), (r, s0, s1)
        assert (g in reach) == (s1 > P31 - 1 and s0 < P32 - 2)
    # the hand-worked contribution of a read 3M <..>N 100M is the oracle's pileup of it: the same shape at a span the oracle can walk
    small = nu.Reads([0], [1000], [0], [nu.giant_cigar(5000)], [f["giant_seq"]])
    for st, en in ((900, 1100), (1000, 1003), (5800, 6100), (5999, 6000), (6000, 6010), (3000, 3050)):
        cov, cnt = nu.expected(oracle, small, [(0, st, en)])
        hc, hn = nu.giant_contribution(1000, 5000, f["giant_seq"], st, en)
        assert np.array_equal(cov, hc) and np.array_equal(cnt, hn)
    # the expectation: (a) reaches past 2^31, the giant read's last hundred bases are there, the declined reads' bases are not
    cov, cnt = nu.high_expected(oracle)
    o = {rg: sum(e - s for _t, s, e in regions[:k]) for k, rg in enumerate(regions)}
    k = o[(0, P32 - 2 - 100, P32 - 2)]
    assert cov[k:k + 100].all() and cnt[k:k + 100].sum(axis=1).tolist() == [1] * 100
    k = o[(0, P32 - 2, P32 - 2 + 10)]
    assert not cov[k:k + 10].any()
    k = o[(0, P31 + (1 << 30), P31 + (1 << 30) + 50)]
    assert cov[k:k + 50].all() and cnt[k:k + 50].sum() == 0
    k = o[(0, P31 + 300, P31 + 1500)]
    assert cnt[k:k + 1200].sum() > 0
    last_a = max(pos[i] + span[i] for i in a)
    assert last_a < P31 + 4097 and cnt[o[(0, P31 - 4097, P31 + 4097)] + (last_a - (P31 - 4097)):o[(0, P31 - 4097, P31 + 4097)] + 8194].sum() == 0
    # regions lie on the declined reads' bases (all of them A, C, G or T: counted, they would show)
    assert (0, pos[d0], pos[d0] + 10) in regions and any(st <= pos[d1] and pos[d1] + 50 <= en for _t, st, en in regions)


def test_depth_cap_limits(oracle):
    exact, over, filt = nu.cap_input(), nu.cap_input(n_starts=7361), nu.cap_input(n_filtered=300)
    assert exact.n == 8000 + 7360 + 736 and over.n == exact.n + 1 and filt.n == exact.n + 300
    assert nu.most_buffered(exact, *nu.CAP_REGION) == (nu.LIVE_MAX, 736)
    assert nu.most_buffered(over, *nu.CAP_REGION) == (nu.LIVE_MAX + 1, 736)
    assert nu.most_buffered(filt, *nu.CAP_REGION) == (nu.LIVE_MAX, 736)
    f = np.flatnonzero(filt.flag == 0x400)
    passing_before = np.cumsum(filt.flag == 0)[f]
    assert len(f) == 300 and (filt.pos[f] == 0).all() and passing_before.max() < 8000 and f.max() > 6000
    # the oracle's answer does not depend on how many reads the device can buffer: 8000 bases on position 0, one on each first read's
    # position, none from a second read of a position; everything up to the first N op's end is covered
    for rd in (exact, filt):
        cov, cnt = nu.expected(oracle, rd, [nu.CAP_REGION])
        assert cnt.sum(axis=1)[:7361].tolist() == [8000] + [1] * 7360 and cov[:7602].all()
        assert cnt[7601:9000].sum(axis=1).tolist() == [8000] + [1] * 1398 and cov.all()
    # the drop pool: 64 regions of 127 words fit the pool of n_reads + 1024 words, 200 do not
    pool = nu.pool_reads()
    words = (pool.n + 63) // 64
    assert 64 * words <= pool.n + 1024 < 200 * words
    assert nu.most_buffered(pool, 0, 0, 100) == (8000, 100)
    cov, cnt = nu.expected(oracle, pool, [(0, 0, 100)])
    assert cnt.sum(axis=1)[5:9].tolist() == [8000] * 4


def test_contract_input(oracle):
    rd, regions = nu.contract_input()
    assert rd.n == 300 and set(rd.tid.tolist()) == {0, 1, 2} and all(0 <= en - st <= nu.PIECE for _t, st, en in regions)
    status, end = nu.read_spans(rd)
    assert {nu.RD_OK, nu.RD_FILTERED} == set(status.tolist())
    kinds = set(nu.tile_kinds(nu.plan_tiles(rd, regions)).tolist())
    assert kinds == {1}
    assert int(rd.seq_off[0]) == 0 and len(rd.ops) == int(rd.op_off[-1])
