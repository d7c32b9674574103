"""The trim-paf pair kernels (k_trim4.hip, k_trim.hip, rb_pair.h) on inputs planted at the thresholds of rb_dev_overlap_split's cascade
(tests/trim_seam_util.py; what each input holds is proved on the CPU by tests/test_trim_seam_inputs.py): bit-exact against the oracle under
both binary-search policies, then the route the row's diagnostic word reports against the restatement of the cascade's sizes."""
import functools

import numpy as np
import pytest

import rustybam_amd
import trim_seam_util as u
from test_gpu_trim import _compare

pytestmark = pytest.mark.gpu

POLICIES = [rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY]


@functools.lru_cache(maxsize=None)
def _want(name, scores, policy):
    """the oracle's rows and clips of a case, computed once per process and left unchanged"""
    from oracle import pyoracle
    args, left, right = u.case(name).args()
    return pyoracle.overlap_split(pyoracle.Batch(*args), left, right, scores, policy)


def _routes(rows):
    return np.where(rows["_row"] == 1, "row", np.where(rows["_pad"] == 1, "wave", "serial"))


def _check_routes(c, rows, orows, legacy, what):
    if c.route_open is not None:
        return
    got = _routes(rows)
    want = c.routes(legacy)
    bad = [(i, c.notes[i], got[i], want[i][0]) for i in range(len(rows)) if orows["status"][i] == 0 and got[i] != want[i][0]]
    assert not bad, f"{what}: route differs from the restatement (pair, note, diagnostic, expected): {bad[:6]}"
    assert ((rows["_row"] == 0) | (rows["_pad"] == 1)).all()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(u.CASES))
def test_planted_case_equals_the_oracle_and_takes_the_expected_route(engine, oracle, name, policy):
    c = u.case(name)
    args, left, right = c.args()
    for scores in c.scores:
        what = f"{name} policy={policy} scores={scores}"
        rows, out = engine.overlap_split(*args, left, right, scores, policy)
        orows, oout = _want(name, scores, policy)
        if c.status is not None:
            assert (orows["status"] == c.status).all(), what
        _compare(rows, out, orows, oout, what)
        _check_routes(c, rows, orows, policy == rustybam_amd.BSEARCH_LEGACY, what)


def test_status_cases_report_the_oracle_s_status(engine, oracle):
    """item 12 by name: touching and inner pairs are cut, apart and same-start pairs carry the reference's panics -- under both policies, on
    records of 193 and 1025 ops (the comparison itself is test_planted_case's)"""
    c = u.case("statuses")
    args, left, right = c.args()
    for policy in POLICIES:
        rows, _ = engine.overlap_split(*args, left, right, (1, 1, 1), policy)
        assert rows["status"].tolist() == [u.STATUS_OF[n.split()[0]] for n in c.notes]
        assert (rows["_pad"][rows["status"] != 0] == 0).all()      # a panic is the serial kernel's to report


def _in_place(engine, c, scores, policy):
    """rb_dev_overlap_split with RB_TRIM_IN_PLACE on a device copy of the case's batch, set up as trim_driver.ResidentTrim does: the ops with
    room behind them, the norm rows from rb_dev_scan_records, pair_out_off behind the ops.  -> (rows, the ops array afterwards)"""
    import torch
    from rustybam_amd import capi
    dev = torch.device("cuda", 0)
    (ops, op_off, t_st, t_en, q_st, q_en, strand), left, right = c.args()
    n, n_ops, k = len(op_off) - 1, int(op_off[-1]), len(left)
    cursor = (n_ops + 31) // 32 * 32
    lens = np.diff(op_off.astype(np.int64))
    need = lens[left.astype(np.int64)] + lens[right.astype(np.int64)]
    poff = cursor + np.concatenate([[0], np.cumsum(need)[:-1]])
    d_ops = torch.zeros(cursor + int(need.sum()) + 64, dtype=torch.int32, device=dev)
    d_ops[:n_ops] = torch.from_numpy(ops.view(np.int32)).to(dev)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)  # noqa: E731
    d_off, d_c = i64(op_off), [i64(x) for x in (t_st, t_en, q_st, q_en)]
    d_strand = torch.from_numpy(np.ascontiguousarray(strand)).to(dev)
    d_contig = torch.zeros(n, dtype=torch.int32, device=dev)
    d_norm = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_l, d_r = torch.from_numpy(left.view(np.int32)).to(dev), torch.from_numpy(right.view(np.int32)).to(dev)
    d_po = torch.from_numpy(poff.astype(np.int64)).to(dev)
    d_rows = torch.zeros(k * 128, dtype=torch.uint8, device=dev)
    view = engine.batch_view(n, n_ops, d_ops.data_ptr(), d_off.data_ptr(), *[x.data_ptr() for x in d_c], d_strand.data_ptr(), d_contig.data_ptr())
    torch.cuda.synchronize()
    engine.dev_scan_records(view, 0, d_norm.data_ptr())
    engine.dev_overlap_split(view, d_norm.data_ptr(), k, d_l.data_ptr(), d_r.data_ptr(), d_po.data_ptr(), scores, policy | capi.TRIM_IN_PLACE,
                             d_rows.data_ptr(), d_ops.data_ptr())
    engine.sync()
    return d_rows.cpu().numpy().view(capi.PAIR_DT).copy(), d_ops.cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", [n for n in u.CASES if u.case(n).in_place])
def test_in_place_equals_copy(engine, name, policy):
    """items 1, 4, 6 and 9 again with the records cut where they lie: the same rows as the copying call apart from out_off, which lies inside
    the record's own extent; the clip read from the array is the copied clip; no word of the array but the two end words of each clip changed"""
    c = u.case(name)
    (ops, op_off, *_), left, right = c.args()
    for scores in c.scores:
        what = f"{name} in place policy={policy} scores={scores}"
        rows, out = engine.overlap_split(*c.args()[0], left, right, scores, policy)
        irows, arr = _in_place(engine, c, scores, policy)
        assert (rows["status"] == 0).all() and (rows["_pad"] == 1).all(), what
        for k in rows.dtype.names:
            if k != "out_off":
                assert np.array_equal(rows[k], irows[k]), f"{what}: {k} differs at pairs {np.flatnonzero((rows[k] != irows[k]).reshape(len(rows), -1).any(axis=1))[:5]}"
        ends = []
        for i in range(len(rows)):
            for s, rec in ((0, int(left[i])), (1, int(right[i]))):
                at, cnt = int(irows["out_off"][i][s]), int(irows["out_n"][i][s])
                assert int(op_off[rec]) <= at and cnt >= 1 and at + cnt <= int(op_off[rec + 1]), f"{what}: pair {i} side {s}: clip [{at}, {at + cnt}) outside its record"
                o = int(rows["out_off"][i][s])
                assert np.array_equal(arr[at:at + cnt], out[o:o + cnt]), f"{what}: pair {i} side {s}: the clip in the array is not the copied clip"
                ends += [at, at + cnt - 1]
        same = arr[:len(ops)] == ops
        same[ends] = True
        assert same.all(), f"{what}: words {np.flatnonzero(~same)[:8]} changed and are no clip's end"
        assert (arr[len(ops):] == 0).all(), what


@pytest.mark.parametrize("policy,scores", [(rustybam_amd.BSEARCH_MODERN, (1, 1, 1)), (rustybam_amd.BSEARCH_LEGACY, (2, 3, 5))])
def test_the_pending_list_walker_s_second_round(engine, oracle, policy, scores):
    """12288 pairs the 64-op row form lists and the 128-op one takes, and among them 64 whose overlap spans 6200 .. 7000 ops: only the slab
    attempt can hold those, and its 48 workgroups read 64 list entries each per round, so an entry at 3072 or behind is read in the second
    round of rb_tw_walk_next.  The list's order is decided by atomics, so that the second round is reached rests on a probability and not on
    a construction: the list has 12352 entries, a slab pair lies among the first 3072 with a probability of at most 1/4, and all 64 of them
    with one of (1/4)^64 or so.  Every pair equals the oracle; the 64 are cut by a wave kernel."""
    args, left, right, is_slab, _, _ = u.walker_batch()
    assert len(left) >= 12288 + 64 > u.SLABS * u.WALK
    rows, out = engine.overlap_split(*args, left, right, scores, policy)
    orows, oout = oracle.overlap_split(oracle.Batch(*args), left, right, scores, policy)
    assert (orows["status"] == 0).all()
    _compare(rows, out, orows, oout, f"walker policy={policy}")
    assert ((rows["_pad"][is_slab] == 1) & (rows["_row"][is_slab] == 0)).all(), np.flatnonzero(is_slab & ((rows["_pad"] != 1) | (rows["_row"] != 0)))[:8]
    assert (rows["_row"][~is_slab] == 1).all()
