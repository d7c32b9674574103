"""The stream clip kernel resolves a window boundary from what the step captured when it streamed the boundary's chunk (rb_stream.h: the
capture table) and falls back to its checkpoints and the record for the boundaries no step captured.  Records of more than 2048 ops (the
stream kernel takes them, not the tile kernel), windows placed on the edges of a lane's chunk (8 ops), of a step (512 ops), of a segment
(5120 ops) and of the record, inside I / D / N ops and inside one op; rows, clipped CIGARs and normalised rows against the per-base oracle."""
import numpy as np
import pytest

import rustybam_amd
from rbtest_util import OPC, batch_args, compare_hits

pytestmark = pytest.mark.gpu

EQ, X, I, D, N = OPC["="], OPC["X"], OPC["I"], OPC["D"], OPC["N"]


def _cigar(n_ops, lead=()):
    """n_ops regular ops behind `lead`: match ops at even places (= of 3 .. 9, every 7th of 60 bases), between them X 1, I 2, D 3, N 5 in turn; no two
    neighbours of one type, a match op at both ends"""
    ops = [(ln << 4) | c for ln, c in lead]
    mid = ((1, X), (2, I), (3, D), (5, N))
    for k in range(n_ops):
        if k % 2 == 0:
            ops.append(((60 if (k // 2) % 7 == 3 else 3 + (k // 2) % 7) << 4) | EQ)
        else:
            ln, c = mid[(k // 2) % 4]
            ops.append((ln << 4) | c)
    if n_ops % 2 == 0:
        ops.append((4 << 4) | EQ)
    return np.array(ops, np.uint32)


def _ref_prefix(ops):
    rl = np.where((ops & 15) == I, 0, ops >> 4).astype(np.int64)
    return np.concatenate([[0], np.cumsum(rl)])


def _batch(cigars, t0=1000):
    n = len(cigars)
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigars])
    ops = np.concatenate(cigars)
    t_st = np.full(n, t0, np.uint64)
    q_st = np.arange(n, dtype=np.uint64) * 7
    R = np.array([int(np.where((c & 15) == I, 0, c >> 4).sum()) for c in cigars], np.uint64)
    Q = np.array([int(np.where(((c & 15) == D) | ((c & 15) == N), 0, c >> 4).sum()) for c in cigars], np.uint64)
    strand = np.where(np.arange(n) % 2 == 0, ord("+"), ord("-")).astype(np.uint8)  # both strands
    return dict(ops=ops, op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=q_st, q_en=q_st + Q, strand=strand, contig=np.zeros(n, np.uint32))


def _edge_windows(cig, t0, delta, kept_from=0):
    """sorted windows that do not overlap, whose edges lie `delta` bases off the first base of the ops named below (indices among the kept ops)"""
    P = _ref_prefix(cig[kept_from:])
    n = len(cig) - kept_from
    marks = [0, 7, 8, 9, 16, 511, 512, 513, 1023, 1024, 5119, 5120, 5121, n - 9, n - 8, n - 1]
    marks += [k for k in (1, 3, 5, 7, 517, 519, 5117) if k < n]  # X, I, D, N ops and their neighbours
    marks += list(range(100, n - 20, 450))  # enough windows for a second pass over the record
    pos = sorted({int(P[k]) + delta for k in marks if 0 <= k < n} | {int(P[k]) + 1 for k in (5, 7, 13) if k < n})  # inside a D / N op
    pos = [x for x in pos if x >= -3]
    pos.append(int(P[-1]) + 5)  # behind the record's end
    st = np.array(pos[:-1], np.int64) + t0
    en = np.array(pos[1:], np.int64) + t0
    k60 = next(k for k in range(600, n) if (int(cig[kept_from + k]) >> 4) == 60)  # a window wholly inside one op: its own list entry, in order
    extra_st, extra_en = int(P[k60]) + 10 + t0, int(P[k60]) + 20 + t0
    keep = (en > st) & ~((st < extra_en) & (en > extra_st))
    st, en = np.append(st[keep], extra_st), np.append(en[keep], extra_en)
    o = np.argsort(st, kind="stable")
    return st[o].astype(np.uint64), en[o].astype(np.uint64)


def _run(engine, oracle, b, w, policy, what, fused, max_fallback=None):
    pol = policy | (rustybam_amd.LIFT_FUSED_SCAN if fused else 0)
    rows, ops, norm, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=pol)
    ob = oracle.Batch(*batch_args(b), b["contig"])
    orows, oops = oracle.liftover(ob, *w, policy=policy)
    onorm = oracle.normalize(ob)
    for k in ("status", "t_st", "t_en", "q_st", "q_en", "first_op", "n_ops", "nmatch", "aln_len"):
        assert np.array_equal(norm[k].astype(np.int64), onorm[k].astype(np.int64)), f"{what}: norm.{k}"
    if fused:  # (rows of records the reference panics on only carry the status, as in tests/test_gpu_parity.py)
        keep = (norm["status"] == 0)[rows["rec"]] if len(rows) else np.zeros(0, bool)
        assert (rows["status"][~keep] != 0).all(), f"{what}: fused rows of panicking records must carry a status"
        rows = rows[keep]
    compare_hits(rows, ops, orows, oops, what)
    if max_fallback is not None:
        # what the fallback may take of a sorted list: lane 0 of the step a later pass resumes at has no op in
        # front of its chunk, so per record and resumed pass the boundaries of ONE chunk at most -- with windows that do not overlap
        # and lie more than 8 ops apart, one window's two
        fb, cap = _fallback_count(engine, b, w, pol)
        print(f"{what}: fallback {fb}, capture table {cap}")
        assert cap > 0 and fb <= max_fallback, (what, fb, cap)
    return rows, cnt


def _fallback_count(engine, b, w, policy):
    """boundaries the diagnostics build resolved from (checkpoints and record, capture table)"""
    rows, ops, norm, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=policy | (1024 << 8))
    return int(cnt["phase"][0]), int(cnt["phase"][1])


@pytest.fixture(scope="module")
def long_batch():
    return _batch([_cigar(6001), _cigar(5300), _cigar(2100), _cigar(7001)])


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("policy", [rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY])
def test_boundaries_on_chunk_step_segment_and_record_edges(engine, oracle, long_batch, delta, fused, policy):
    b = long_batch
    ws, we = _edge_windows(b["ops"][: int(b["op_off"][1])], 1000, delta)
    assert len(ws) > 32  # two passes over the first record
    w = (np.zeros(len(ws), np.uint32), ws, we)
    passes = -(-len(ws) // 32)
    rows, cnt = _run(engine, oracle, b, w, policy, f"edges delta={delta} fused={fused} policy={policy}", fused, max_fallback=2 * 4 * (passes - 1))
    assert len(rows) > 4 * 20 and (rows["status"] == 0).sum() > 60
    assert cnt["n_generic"] == 0 or policy == rustybam_amd.BSEARCH_LEGACY


def test_sorted_windows_resolve_from_the_capture_table(engine, long_batch):
    """Sorted windows, one pass: nothing is to be resolved on the fallback path (counters of the diagnostics build, debug bit 1024).
    Among the windows are clips that end on the last base of a step: their end offset is the first one of the next step, whose first
    chunk captures it after the slot's cursor has moved on."""
    b = long_batch
    ws, we = _edge_windows(b["ops"][: int(b["op_off"][1])], 1000, 0)
    ws, we = ws[:30], we[:30]  # one pass: a later pass resumes inside the record, and what lies in front of its first step is the fallback's
    w = (np.zeros(len(ws), np.uint32), ws, we)
    fb, cap = _fallback_count(engine, b, w, rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN)
    assert cap > 0 and fb == 0, (fb, cap)


@pytest.mark.parametrize("fused", [False, True])
def test_stripped_head_record_of_2055_ops(engine, oracle, fused):
    """leading indels are stripped: first_op is 3, no multiple of 8, and the aligned head of the stream holds ops that are not the record's"""
    lead = ((2, I), (3, D), (1, I))
    cigs = [_cigar(2055, lead), _cigar(2049, lead[:1]), _cigar(2060, lead[:2])]
    b = _batch(cigs)
    b["t_en"] = b["t_en"].copy()
    ws, we = _edge_windows(cigs[0], 1000 + 3, 0, kept_from=3)
    w = (np.zeros(len(ws), np.uint32), ws, we)
    _run(engine, oracle, b, w, rustybam_amd.BSEARCH_MODERN, f"stripped head fused={fused}", fused, max_fallback=2 * 3 * (-(-len(ws) // 32) - 1))


@pytest.mark.parametrize("fused", [False, True])
def test_more_boundaries_in_a_step_than_the_table_holds(engine, oracle, long_batch, fused):
    """80 windows of 3 bases inside the first 512 ops: 160 boundaries in one step, five passes"""
    b = long_batch
    st = 1000 + 5 + 11 * np.arange(80, dtype=np.uint64)
    w = (np.zeros(80, np.uint32), st, st + 3)
    rows, cnt = _run(engine, oracle, b, w, rustybam_amd.BSEARCH_MODERN, f"dense fused={fused}", fused, max_fallback=0)
    assert len(rows) == 4 * 80


@pytest.mark.parametrize("fused", [False, True])
def test_unsorted_window_list_takes_the_fallback(engine, oracle, long_batch, fused):
    b = long_batch
    ws, we = _edge_windows(b["ops"][: int(b["op_off"][1])], 1000, 0)
    o = np.random.default_rng(7).permutation(len(ws))
    w = (np.zeros(len(ws), np.uint32), ws[o], we[o])
    _run(engine, oracle, b, w, rustybam_amd.BSEARCH_MODERN, f"unsorted fused={fused}", fused)
    fb, cap = _fallback_count(engine, b, w, rustybam_amd.BSEARCH_MODERN)
    assert fb > 0 and cap == 0, (fb, cap)


def test_records_a_tile_hands_back_reach_the_list_kernel(engine, oracle):
    """the list form of the kernel (k_liftover_list.hip), by the route tests/test_gpu_tile.py uses: with the line between short and long
    records moved up, records of 2100 - 2200 ops are tiled, and a tile with a record whose end indels were stripped is handed back record
    by record"""
    import os
    lead = ((2, I), (3, D))
    cigs = [_cigar(2101), _cigar(2150, lead), _cigar(2199), _cigar(2120)]
    b = _batch(cigs)
    ws, we = _edge_windows(cigs[0], 1000, 0)
    w = (np.zeros(len(ws), np.uint32), ws, we)
    old = os.environ.get("RB_SHORT_MAX")
    os.environ["RB_SHORT_MAX"] = "2300"
    try:
        for fused in (False, True):
            rows, cnt = _run(engine, oracle, b, w, rustybam_amd.BSEARCH_MODERN, f"list form fused={fused}", fused)
            assert int(cnt["phase"][3]) > 0 and int(cnt["phase"][4]) > 0, (fused, cnt["phase"])
    finally:
        if old is None:
            os.environ.pop("RB_SHORT_MAX", None)
        else:
            os.environ["RB_SHORT_MAX"] = old
