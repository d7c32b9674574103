"""The stream clip kernel at the seams of a step's layout (rb_stream.h).  A step is 512 ops counted from g0, the first op of the 128-byte
line in which the record starts: a lane's 4-op groups, the 8 ops of a capture entry, the 16 ops of a store granule, the two halves of a step
(256 ops), the step and the segment (5120 ops).  Windows are placed on those seams for records that start at several offsets inside their
first line, record ends are placed against the halves, the fused verification is broken across the seams, and narrow clips crowd the
half-step seam.  Everything is compared with the per-base oracle and integer-exact: rows, clipped CIGARs and normalised rows."""
import os

import numpy as np
import pytest

import rustybam_amd
from rbtest_util import OPC, batch_args, compare_hits
from test_gpu_stream_capture import _cigar, _fallback_count, _ref_prefix, _run
from test_gpu_tile import synth_batch, tile_env

pytestmark = pytest.mark.gpu

EQ, X, I, D, N, S = OPC["="], OPC["X"], OPC["I"], OPC["D"], OPC["N"], OPC["S"]
MODERN, LEGACY, FUSED = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY, rustybam_amd.LIFT_FUSED_SCAN
T_GAP = 200_000  # reference distance between two records of a batch: each record has the windows laid over it to itself

# ops (counted from g0) whose first base a window edge is laid at: a 4-op group, the capture pair, the granule, the half-step (in the
# first and the second step), the step, the segment and the half-step behind it
SEAMS = [3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 256, 257, 767, 768, 769, 511, 512, 513, 5119, 5120, 5121, 5375, 5376, 5377]


def _cig(n_ops):
    """a regular record of exactly n_ops ops (_cigar makes odd counts; an X in front makes the even ones)"""
    c = _cigar(n_ops) if n_ops % 2 else _cigar(n_ops - 1, lead=((2, X),))
    assert len(c) == n_ops
    return c


def _place(cigars_and_heads):
    """[(cigar, head)] -> batch in which record 2 i + 1 is cigar i starting `head` ops behind a multiple of 32 (the length of the short record in
    front of it, record 2 i, sets that), every record T_GAP apart on the reference; -> (batch, indices of the placed records)"""
    cigs, idx, at = [], [], 0
    for c, head in cigars_and_heads:
        f = (head - at - 9) % 32 + 9  # 9 .. 40 ops
        cigs.append(_cig(f))
        at += f
        assert at % 32 == head
        idx.append(len(cigs))
        cigs.append(c)
        at += len(c)
    n = len(cigs)
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    t_st = 1000 + T_GAP * np.arange(n, dtype=np.uint64)
    R = np.array([int(np.where((c & 15) == I, 0, c >> 4).sum()) for c in cigs], np.uint64)
    Q = np.array([int(np.where(((c & 15) == D) | ((c & 15) == N), 0, c >> 4).sum()) for c in cigs], np.uint64)
    strand = np.where(np.arange(n) % 4 < 2, ord("+"), ord("-")).astype(np.uint8)  # both strands among the placed records
    b = dict(ops=np.concatenate(cigs), op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=np.arange(n, dtype=np.uint64) * 7, q_en=np.arange(n, dtype=np.uint64) * 7 + Q,
             strand=strand, contig=np.zeros(n, np.uint32))
    return b, idx


def _seam_windows(cig, t0, head, delta, marks, fill=True, limit=None):
    """sorted windows that do not overlap, over one record: edges `delta` bases off the first base of the ops `marks` (counted from g0)"""
    P = _ref_prefix(cig)
    n = len(cig)
    ks = [m - head for m in marks]
    if fill:
        ks += list(range(100, n - 20, 450))  # enough windows for a second pass
    pos = sorted({int(P[k]) + delta for k in ks if 0 < k < n} | {int(P[-1]) + 5})
    if limit is not None:
        pos = pos[:limit + 1]
    st, en = np.array(pos[:-1], np.int64) + t0, np.array(pos[1:], np.int64) + t0
    return st, en


def _windows(b, idx, per_record):
    """the window list of a batch: per_record(cigar, t0, head) for every placed record, in reference order"""
    st, en = [], []
    for r in idx:
        c = b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])]
        s, e = per_record(c, int(b["t_st"][r]), int(b["op_off"][r]) % 32)
        st.append(s), en.append(e)
    st, en = np.concatenate(st).astype(np.uint64), np.concatenate(en).astype(np.uint64)
    assert (st[1:] >= en[:-1]).all() and (en > st).all()
    return np.zeros(len(st), np.uint32), st, en


HEADS = [0, 1, 3, 4, 5, 28, 31]
LENGTHS = [6001, 5500, 7001, 2100, 5400, 6200, 5801]


@pytest.fixture(scope="module")
def seam_batch():
    return _place([(_cig(n), h) for n, h in zip(LENGTHS, HEADS)])


# ---- 1. seams of the layout


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_window_edges_on_group_pair_granule_half_step_and_segment(engine, oracle, seam_batch, delta, fused, policy):
    b, idx = seam_batch
    assert sorted(int(b["op_off"][r]) % 32 for r in idx) == HEADS
    w = _windows(b, idx, lambda c, t0, head: _seam_windows(c, t0, head, delta, SEAMS))
    hits = [int(((w[2] > b["t_st"][r]) & (w[1] < b["t_en"][r])).sum()) for r in idx]
    passes = max(-(-h // 32) for h in hits)
    assert passes == 2 and min(hits) > 12
    rows, cnt = _run(engine, oracle, b, w, policy, f"seams delta={delta} fused={fused} policy={policy}", fused, max_fallback=2 * len(idx) * (passes - 1))
    assert len(rows) > len(idx) * 12 and (rows["status"] == 0).sum() > 0.8 * len(rows)
    assert cnt["n_generic"] == 0 or policy == LEGACY


def test_one_pass_over_the_seams_resolves_from_the_capture_table(engine, seam_batch):
    b, idx = seam_batch
    w = _windows(b, idx, lambda c, t0, head: _seam_windows(c, t0, head, 0, SEAMS, fill=False, limit=30))
    fb, cap = _fallback_count(engine, b, w, MODERN | FUSED)
    assert cap > 0 and fb == 0, (fb, cap)


# ---- 2. record ends against the halves of a step


@pytest.mark.parametrize("fused", [False, True])
def test_record_ends_against_the_halves(engine, oracle, fused):
    """consecutive long records: the last op of each lies, counted from g0, at 255, 256, 257, 511, 512 or 513 mod 512, the next record starts
    behind it in the same line; windows over the ends and over the middle of every record, so that every op of it is in a clip"""
    cigs, at = [], 0
    for last in (255, 256, 257, 511, 512, 513, 256, 512):
        head = at % 32
        n = 2048 + (last + 1 - head) % 512
        n += 512 if n < 2100 else 0
        assert (head + n - 1) % 512 == last % 512
        cigs.append(_cig(n))
        at += n
    n = len(cigs)
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    t_st = 1000 + T_GAP * np.arange(n, dtype=np.uint64)
    R = np.array([int(np.where((c & 15) == I, 0, c >> 4).sum()) for c in cigs], np.uint64)
    Q = np.array([int(np.where(((c & 15) == D) | ((c & 15) == N), 0, c >> 4).sum()) for c in cigs], np.uint64)
    b = dict(ops=np.concatenate(cigs), op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=t_st * 0 + 11, q_en=11 + Q,
             strand=np.where(np.arange(n) % 2 == 0, ord("+"), ord("-")).astype(np.uint8), contig=np.zeros(n, np.uint32))

    def ends(c, t0, head):
        P, m = _ref_prefix(c), len(c)
        pos = [-5, int(P[20]), int(P[40]), int(P[m - 40]), int(P[m - 20]), int(P[m - 2]), int(P[-1]) + 5]
        return np.array(pos[:-1], np.int64) + t0, np.array(pos[1:], np.int64) + t0

    w = _windows(b, range(n), ends)
    rows, cnt = _run(engine, oracle, b, w, MODERN, f"record ends fused={fused}", fused)
    assert len(rows) == 6 * n and (rows["status"] == 0).sum() >= 5 * n and cnt["n_generic"] == 0


# ---- 3. the fused verification across the seams


def _broken(kind, seam, head):
    """a regular record of 2301 ops, broken between the ops `seam` and `seam` + 1 (counted from g0)"""
    c = _cig(2301).copy()
    k = seam + 1 - head  # the record's op behind the seam
    assert k >= 1
    if kind == "pair":  # two adjacent ops of one type, one on each side of the seam
        c[k] = (c[k] & ~np.uint32(15)) | (c[k - 1] & 15)
    elif kind == "zero":
        c[k] = c[k] & 15
    elif kind == "soft":
        c[k] = (c[k] & ~np.uint32(15)) | S
    return c


@pytest.mark.parametrize("kind", ["pair", "zero", "soft"])
def test_verification_across_the_seams(engine, oracle, kind):
    seams = [3, 255, 511]
    heads = [0, 1, 3]
    b, idx = _place([(_broken(kind, s, h), h) for s, h in zip(seams, heads)])
    w = _windows(b, idx, lambda c, t0, head: _seam_windows(c, t0, head, 0, [3, 4, 5, 255, 256, 257, 511, 512, 513], fill=False))
    _run(engine, oracle, b, w, MODERN, f"broken ({kind})", True)
    ob = oracle.Batch(*batch_args(b), b["contig"])
    onorm = oracle.normalize(ob)
    # (the break is seen at all: the oracle does not call these records regular)
    rows, ops, norm, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=MODERN | FUSED)
    assert np.array_equal(norm["status"], onorm["status"])
    assert int(cnt["n_generic"]) > 0 or (norm["status"][idx] != 0).all(), (kind, cnt["n_generic"], norm["status"][idx])


def test_unbroken_twins_stay_on_the_fast_path(engine, oracle):
    b, idx = _place([(_cig(2301), h) for h in (0, 1, 3)])
    w = _windows(b, idx, lambda c, t0, head: _seam_windows(c, t0, head, 0, [3, 4, 5, 255, 256, 257, 511, 512, 513], fill=False))
    rows, cnt = _run(engine, oracle, b, w, MODERN, "unbroken twins", True)
    assert len(rows) > 3 * 6 and cnt["n_generic"] == 0


# ---- 4. narrow clips at the half-step seam


@pytest.mark.parametrize("slots", [None, "1"])
@pytest.mark.parametrize("fused", [False, True])
def test_narrow_clips_on_both_sides_of_the_half_step(engine, oracle, fused, slots):
    """80 windows of 1 - 3 ops around op 768 (counted from g0: op 256 of step 1): consecutive clips of a slot share a granule or lie in
    neighbouring ones, so some go to their slot and some to the copy list; with one slot (RB_DEBUG_SLOTS=1) more of them are copied"""
    b, idx = _place([(_cig(2501), h) for h in (0, 5, 31)])
    rng = np.random.default_rng(41)
    steps = rng.integers(1, 4, 80)

    def narrow(c, t0, head):
        P = _ref_prefix(c)
        k = 768 - head - int(steps[:40].sum()) + np.concatenate([[0], np.cumsum(steps)])
        assert k[0] > 512 - head and k[40] == 768 - head and k[-1] < 1024 - head
        pos = sorted({int(P[x]) for x in k})
        return np.array(pos[:-1], np.int64) + t0, np.array(pos[1:], np.int64) + t0

    w = _windows(b, idx, narrow)
    assert len(w[1]) >= 3 * 60
    old = os.environ.get("RB_DEBUG_SLOTS")
    if slots is not None:
        os.environ["RB_DEBUG_SLOTS"] = slots
    try:
        rows, cnt = _run(engine, oracle, b, w, MODERN, f"narrow fused={fused} slots={slots}", fused)
    finally:
        if old is None:
            os.environ.pop("RB_DEBUG_SLOTS", None)
        else:
            os.environ["RB_DEBUG_SLOTS"] = old
    assert len(rows) == len(w[1]) and (rows["status"] == 0).sum() > 3 * 40


# ---- 5. short records on the per-record kernel


@pytest.mark.parametrize("policy", [FUSED, 0])
def test_short_records_on_the_per_record_kernel(engine, oracle, policy):
    """tiles off: 2000 records of 8 - 300 ops, each a wave of the stream kernel whose one step holds the record's head, its end and ops of
    both neighbours"""
    b = synth_batch(engine, 0xF1A7, 2000, 8, 300, span=300_000)
    assert set(int(x) % 32 for x in b["op_off"][:-1]) == set(range(32))
    span = int(b["t_en"].max())
    st = np.arange(0, span, 4_139, dtype=np.uint64)
    w = (np.zeros(len(st), np.uint32), st, np.minimum(st + np.uint64(5_000), np.uint64(span)))
    ob = oracle.Batch(*batch_args(b), b["contig"])
    orows, oops = oracle.liftover(ob, *w, policy=policy & 1)
    with tile_env(False):
        rows, ops, norm, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=policy)
    assert int(cnt["phase"][3]) == 0  # no tiles were made
    keep = (norm["status"] == 0)[rows["rec"]]
    assert keep.sum() > 2000
    compare_hits(rows[keep], ops, orows, oops, f"short records, tiles off, policy={policy}")
