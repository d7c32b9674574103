"""The generic wave clip kernel (rb_k_liftover_generic_wave with rb_k_generic_checkpoints and rb_k_generic_jobs, k_liftover.hip) on inputs
placed on its geometry: a checkpoint every 64 kept ops, the jumps of pass 1 and pass 2 with the second attempt, cp_search beyond its first
64 checkpoints, equal ranges that straddle a checkpoint, runs carried from step to step in pass 3, the checkpoint kernel's load groups,
rb_defer_record on a window list that is not sorted, and the unsorted-tpos_aln detection on records with checkpoints.
tests/generic_util.py builds the inputs, tests/test_generic_inputs.py proves on the CPU what they hold.  Every comparison is against the
per-base oracle, bit-exact, no row left out, and every test asserts its route: the rows the generic kernel must have written carry
RB_HIT_GENERIC and the call's n_generic counts them.

One-line mutations of k_liftover.hip this file was run against (each as a library variant, the whole file once):
  * `if (!jumped || b_set) break;` -> `break;` (no second attempt in pass 2): 17 of the 71 tests fail -- the windows that are no edges, the
    long record, the unsorted list, the descriptor modes and the run without checkpoints;
  * `(ptype == opc && (lane == 0 || i > ia))` dropped from `odd` (the fast step of pass 3 no longer sees equal neighbours): all 71 fail;
  * `if (t_st == 0)` -> `if (false)` in front of the first-ops loop (no look at the record's first ops when a hit starts at a checkpoint):
    16 fail, all of the legacy policy -- the edges at t_st = 0 and the windows that are no edges (the record that opens with 400S);
  * `gcp[mid].y <= target` -> `<` in last_le, `k2 > k1 + 1u` -> `k2 > k1`, and `m != ~0ull` -> `true` in cp_search: none fails, and no
    input can make one, because none of the three changes a row.  A checkpoint is a place to START a walk from: every checkpoint at or in
    front of the one the search should find is as good (the walk is longer, the sums the same), and each of the three can only move the
    answer towards the record's start.  `<` picks the checkpoint in front when one stands exactly at the target; cp_search cut off after
    its first ballot answers 63 instead of 64 .. 67, and pass 2 jumps there or not at all; `k2 == k1 + 1` makes c_end1 the end of the
    walk's first step, where `c_end1 > c0 + 64` is false, so no jump is taken.  They cost steps, which no counter of the library shows.
"""
import os

import numpy as np
import pytest

import generic_util as gu
import rustybam_amd
from rbtest_util import batch_args, compare_hits

pytestmark = pytest.mark.gpu

MODERN, LEGACY, FUSED = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY, rustybam_amd.LIFT_FUSED_SCAN
GENERIC = rustybam_amd.HIT_GENERIC
NORM_KEYS = ("status", "t_st", "t_en", "q_st", "q_en", "first_op", "n_ops", "nmatch", "aln_len")
ROW_KEYS = ("rec", "win", "status", "flags", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_n")   # (not out_off: the arenas fill in any order)


class Data:
    """batches, model records and window lists per (t_st, strand); the oracle's rows computed once per (list, policy) and left unchanged"""

    def __init__(self, oracle):
        self.oracle, self.b, self.recs, self.norm, self._w, self._rows = oracle, {}, {}, {}, {}, {}
        for t0 in (1000, 0):
            for strand in "+-":
                b = gu.batch(t0, strand)
                self.b[t0, strand] = b
                self.norm[t0, strand], self.recs[t0, strand] = gu.model_records(oracle, b)
                assert (self.norm[t0, strand]["status"] == 0).all()

    def windows(self, t0, tag):
        """the lists depend on the normalised coordinates alone, which are the same on both strands"""
        if (t0, tag) not in self._w:
            recs = self.recs[t0, "+"]
            if tag.startswith("edge"):
                w = gu.edge_windows(recs, int(tag[4:]))
            elif tag == "special":
                w = gu.special_windows(recs)
            elif tag == "long":
                w = gu.long_windows(next(r for r in recs if r.name == "long"))
            else:
                w = gu.unsorted_windows(recs)
            self._w[t0, tag] = w
        return self._w[t0, tag]

    def rows(self, t0, strand, tag, policy):
        key = (t0, strand, tag, policy)
        if key not in self._rows:
            b = self.b[t0, strand]
            self._rows[key] = self.oracle.liftover(self.oracle.Batch(*batch_args(b), b["contig"]), *self.windows(t0, tag), policy=policy)
        return self._rows[key]


@pytest.fixture(scope="module")
def data(oracle):
    return Data(oracle)


def _check_route(rows, cnt, recs, w, what):
    """every row of an irregular record is the generic kernel's; of the regular copy, the rows of the windows that start or end more than
    RB_WALK_MAX ops deep in its D / I run; and n_generic counts exactly the rows that carry the flag"""
    irregular = np.array([r.irregular for r in recs])
    gen = (rows["flags"] & GENERIC) != 0
    bad = np.flatnonzero(irregular[rows["rec"]] & ~gen)
    assert len(bad) == 0, f"{what}: rows of irregular records without RB_HIT_GENERIC: {rows[bad[:4]]}"
    reg = next(r for r in recs if r.name == "struct_regular")
    deep = gu.deep_windows(reg, w)
    mine = (rows["rec"] == reg.r) & np.isin(rows["win"], deep)
    assert mine.sum() == len(set(deep)) and gen[mine].all(), f"{what}: deep windows of the regular copy: {rows[mine & ~gen][:4]}"
    assert int(cnt["n_generic"]) == int(gen.sum()), (what, int(cnt["n_generic"]), int(gen.sum()))
    return int(gen.sum())


def _lift(engine, data, t0, strand, tag, policy, fused, deep=True):
    b, recs, w = data.b[t0, strand], data.recs[t0, strand], data.windows(t0, tag)
    what = f"t_st={t0} strand={strand} {tag} policy={policy} fused={fused}"
    rows, ops, norm, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=policy | (FUSED if fused else 0))
    onorm = data.norm[t0, strand]
    for k in NORM_KEYS:
        assert np.array_equal(norm[k].astype(np.int64), onorm[k].astype(np.int64)), f"{what}: norm.{k}"
    orows, oops = data.rows(t0, strand, tag, policy)
    compare_hits(rows, ops, orows, oops, what)
    n_gen = _check_route(rows, cnt, recs, w if deep else (w[0][:0], w[1][:0], w[2][:0]), what)
    return rows, ops, n_gen


# ------------------------------------------------------------------------------------------------ 1, 2: edges
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_edges_at_checkpoints_steps_and_structures(engine, data, delta, strand, policy, fused):
    """windows whose edges lie delta bases off the first base of the marked ops: 0, 1, both sides of every structure of the structured
    record, the multiples of 64 and 256 with their neighbours, n - 2, n - 1 of records of 63 .. 257, 455 and 4300 ops"""
    rows, ops, n_gen = _lift(engine, data, 1000, strand, f"edge{delta}", policy, fused)
    assert len(rows) > 500 and (rows["status"] == 0).sum() > 0.6 * len(rows) and n_gen > 0.8 * len(rows)


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_long_one_base_inside_and_straddling_windows(engine, data, strand, policy, fused):
    """the windows that are no edges: into, out of and inside the run of 150 D / I ops (pass 2's jump and second attempt, 'none'), from op 2
    into the run of 130 X ops, over the zero lengths and the merge across checkpoint 64, onto the base in front of the I op at 256, one
    base, inside one op, the record's span (not 'inside') and a window around the record (RB_HIT_INSIDE)"""
    for t0 in (1000, 0):
        rows, ops, n_gen = _lift(engine, data, t0, strand, "special", policy, fused)
        assert (rows["status"] == 1).sum() >= 5
        if t0:                                                      # (at t_st = 0 no window starts in front of a record)
            assert (rows["flags"] & 1).sum() >= len(data.recs[t0, strand])


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_edges_at_t_st_zero(engine, data, delta, strand, policy, fused):
    """the same at t_st = 0, with the records whose first unit consumes no reference: S, H, 70 zero-length ops and then S, and 400S --
    units at position -1, a tpos_aln that is not sorted, the serial replay of the probe sequence; detected from the record's first ops when
    the hit starts at a checkpoint behind them"""
    rows, ops, n_gen = _lift(engine, data, 0, strand, f"edge{delta}", policy, fused)
    recs = data.recs[0, strand]
    wrapped = np.array([r.wrapped for r in recs])[rows["rec"]]
    assert wrapped.sum() > 200 and (rows["status"][wrapped] == 0).sum() > 100
    r400 = next(r.r for r in recs if r.name == "lead_400S")
    assert (rows["status"][rows["rec"] == r400] == 16).sum() >= 5      # (what a search that took the array for sorted would have found)


# ------------------------------------------------------------------------------------------------ 3: the long record
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_long_record_beyond_64_checkpoints(engine, data, policy):
    """4300 ops, 68 checkpoints: windows whose last base lies just behind checkpoints 63 .. 66 (cp_search's second ballot)"""
    for strand in "+-":
        for fused in (False, True):
            rows, ops, n_gen = _lift(engine, data, 1000, strand, "long", policy, fused, deep=False)
            long_r = next(r.r for r in data.recs[1000, strand] if r.name == "long")
            mine = rows[rows["rec"] == long_r]
            assert len(mine) == len(data.windows(1000, "long")[1]) and (mine["status"] == 0).all()


# ------------------------------------------------------------------------------------------------ 4: a list that is not sorted
@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("fused", [False, True])
def test_unsorted_list_of_more_than_200_windows(engine, data, strand, fused):
    """rb_defer_record enumerates the windows of a list that is not sorted 64 to a ballot and carries its count from ballot to ballot"""
    for t0, policy in ((1000, MODERN), (1000, LEGACY), (0, MODERN)):
        w = data.windows(t0, "unsorted")
        assert len(w[1]) >= 200
        rows, ops, n_gen = _lift(engine, data, t0, strand, "unsorted", policy, fused)
        per_rec = np.bincount(rows["rec"], minlength=len(data.recs[t0, strand]))
        assert (per_rec > 64).all(), per_rec


# ------------------------------------------------------------------------------------------------ 5: descriptors, early exit
@pytest.mark.parametrize("strand", ["+", "-"])
def test_descriptor_and_early_exit_modes(engine, data, strand):
    """RB_LIFT_DESCRIPTORS and RB_LIFT_EARLY_EXIT: the rows and clips of the default mode; a generic row carries no descriptor"""
    from test_gpu_parity import _rebuild_from_descriptor
    b = data.b[1000, strand]
    for tag in ("edge0", "special"):
        w = data.windows(1000, tag)
        base_rows, base_ops, n_gen = _lift(engine, data, 1000, strand, tag, MODERN, False)
        for pol in (rustybam_amd.LIFT_EARLY_EXIT, rustybam_amd.LIFT_DESCRIPTORS, rustybam_amd.LIFT_DESCRIPTORS | rustybam_amd.LIFT_EARLY_EXIT):
            rows, ops, _, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=pol)
            assert len(rows) == len(base_rows)
            for k in ROW_KEYS:
                if k != "flags":
                    assert np.array_equal(rows[k], base_rows[k]), (tag, pol, k)
            gen = (rows["flags"] & GENERIC) != 0
            assert np.array_equal(gen, (base_rows["flags"] & GENERIC) != 0) and int(cnt["n_generic"]) == n_gen
            assert not (rows["flags"][gen] & rustybam_amd.HIT_DESCRIPTOR).any(), (tag, pol)
            n_desc = 0
            for g, o in zip(rows, base_rows):
                if int(o["status"]) != 0:
                    continue
                want = base_ops[int(o["out_off"]):int(o["out_off"]) + int(o["out_n"])]
                if int(g["flags"]) & rustybam_amd.HIT_DESCRIPTOR:
                    got = _rebuild_from_descriptor(b, g, ops[int(g["out_off"]):int(g["out_off"]) + 4])
                    n_desc += 1
                else:
                    got = ops[int(g["out_off"]):int(g["out_off"]) + int(g["out_n"])]
                assert np.array_equal(got, want), (tag, pol, int(g["rec"]), int(g["win"]))
            if pol & rustybam_amd.LIFT_DESCRIPTORS:
                assert n_desc > 0                                   # (rows of the regular copy that stayed on the fast path)


# ------------------------------------------------------------------------------------------------ 6: break-paf
@pytest.mark.parametrize("max_size", [0, 2, 100])
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_break_paf_pieces_through_the_generic_kernel(engine, oracle, data, policy, max_size):
    """the pieces of the irregular records are the generic kernel's in both forms of break-paf (one walk: the records it declines)"""
    for strand in "+-":
        b, recs = data.b[1000, strand], data.recs[1000, strand]
        orows, oops = oracle.break_paf(oracle.Batch(*batch_args(b), b["contig"]), max_size, policy=policy)
        irregular = np.array([r.irregular for r in recs])
        for walks, extra in ((1, rustybam_amd.BREAK_ONE_WALK), (2, 0), (1, rustybam_amd.BREAK_ONE_WALK | FUSED), (2, FUSED)):
            what = f"break max={max_size} policy={policy} strand={strand} walks={walks} fused={bool(extra & FUSED)}"
            rows, ops, norm, cnt = engine.break_paf(*batch_args(b), max_size, policy=policy | extra)
            assert (norm["status"] == 0).all(), what
            compare_hits(rows, ops, orows, oops, what)
            gen = (rows["flags"] & GENERIC) != 0
            assert gen[irregular[rows["rec"]]].all() and int(cnt["n_generic"]) >= int(irregular[rows["rec"]].sum()), what
        if max_size < 100:
            assert len(orows) > 20 * len(recs)


# ------------------------------------------------------------------------------------------------ 7: checkpoints off
_CHILD = r'''
import pickle, sys
sys.path.insert(0, %r)
import torch  # noqa: F401 (HIP runtime load order, see conftest)
import rustybam_amd
calls = pickle.load(open(sys.argv[1], "rb"))
eng = rustybam_amd.Engine(0)
out = []
for b, w, pol in calls:
    rows, ops, norm, cnt = eng.liftover(b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"], b["contig"], *w, policy=pol)
    out.append((rows, ops, int(cnt["n_generic"])))
eng.close()
pickle.dump(out, open(sys.argv[2], "wb"))
'''


def test_same_rows_and_clips_without_checkpoints(engine, data):
    """RB_DEBUG_NO_GEN_CP=1 (read once per process: a fresh child) makes every walk start at the record's first op: the calls of the edges
    test (modern policy) and the long record's windows give the same rows and the same clips, byte for byte"""
    import pickle
    import subprocess
    import sys
    import tempfile
    calls, mine = [], []
    for tag in ("edge-1", "edge0", "edge1", "long"):
        for strand in "+-":
            for fused in (False, True):
                b = {k: v for k, v in data.b[1000, strand].items() if k != "names"}
                calls.append((b, data.windows(1000, tag), MODERN | (FUSED if fused else 0)))
                mine.append(_lift(engine, data, 1000, strand, tag, MODERN, fused, deep=tag != "long"))
    with tempfile.TemporaryDirectory() as d:
        pickle.dump(calls, open(os.path.join(d, "in.pkl"), "wb"))
        env = dict(os.environ, RB_DEBUG_NO_GEN_CP="1")
        code = _CHILD % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, "-c", code, os.path.join(d, "in.pkl"), os.path.join(d, "out.pkl")], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        theirs = pickle.load(open(os.path.join(d, "out.pkl"), "rb"))
    assert len(theirs) == len(mine)
    for k, ((rows, ops, n_gen), (crows, cops, cn_gen)) in enumerate(zip(mine, theirs)):
        assert len(rows) == len(crows) and n_gen == cn_gen, k
        for f in ROW_KEYS:
            assert rows[f].tobytes() == crows[f].tobytes(), (k, f)
        for g, c in zip(rows, crows):
            if int(g["status"]) == 0:
                a = ops[int(g["out_off"]):int(g["out_off"]) + int(g["out_n"])]
                z = cops[int(c["out_off"]):int(c["out_off"]) + int(c["out_n"])]
                assert a.tobytes() == z.tobytes(), (k, int(g["rec"]), int(g["win"]))
