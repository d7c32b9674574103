"""The inputs of tests/test_gpu_generic_wave.py hold what they are meant to hold.

No GPU: the records are normalised by the per-base oracle, the numpy model of tests/generic_util.py says which checkpoints, jumps, second
attempts and kinds of step every (record, window) pair leads the generic wave kernel through, and the counts are asserted -- so a change
of a constant (RB_GCP, the step of 64 ops) or of a builder that loses a case fails this file instead of leaving the GPU file blind.  The
model itself is held against the oracle: status, row and clipped ops of every pair, modern policy."""
import numpy as np
import pytest

import generic_util as gu
from rbtest_util import batch_args, unpack

MODERN, LEGACY = 0, 1


@pytest.fixture(scope="module")
def inputs(oracle):
    """per t_st: batch ('+' strand), norm rows, model records, window lists"""
    out = {}
    for t0 in (1000, 0):
        b = gu.batch(t0, "+")
        norm, recs = gu.model_records(oracle, b)
        out[t0] = dict(b=b, norm=norm, recs=recs, by_name={r.name: r for r in recs})
    return out


def _orows(oracle, b, w, policy=MODERN):
    rows, ops = oracle.liftover(oracle.Batch(*batch_args(b), b["contig"]), *w, policy=policy)
    return rows, ops


@pytest.mark.parametrize("t0", [1000, 0])
def test_records_hold_what_they_state(inputs, t0):
    x = inputs[t0]
    b, norm, by = x["b"], x["norm"], x["by_name"]
    assert (norm["status"] == 0).all(), norm["status"]                 # no record the reference panics on
    assert [by[f"len{n}"].n for n in gu.LENGTHS] == list(gu.LENGTHS)
    assert by["long"].n == gu.N_LONG and by["long"].ncp > 64 + 2       # cp_search takes a second ballot
    for name, rec in by.items():
        if name != "struct_regular" and name != "lead_2H" and name != "lead_zeros_4S":
            pair = np.flatnonzero((rec.code[1:] == rec.code[:-1]) & (rec.code[1:] == gu.EQ))
            assert len(pair) >= 1, name                                # irregular by adjacent = ops
        assert rec.irregular == (name != "struct_regular"), name
    assert [len(np.flatnonzero(by[f"len{n}"].code[1:] == by[f"len{n}"].code[:-1])) for n in gu.LENGTHS] == [1] * len(gu.LENGTHS)
    # the stripped record: three leading indels gone, and the checkpoints addressed by a start that is no multiple of 64
    s = by["stripped"]
    assert int(norm["first_op"][s.r]) == 3 and s.n == 130 and s.t_st == t0
    assert s.ops_off % gu.GCP != 0 and any(r.ops_off % gu.GCP for r in by.values() if r.has_cp and r is not s)
    # the structured record, op by op
    for name in ("struct", "struct_regular"):
        r = by[name]
        assert r.n == gu.N_STRUCT and int(norm["first_op"][r.r]) == 0
        assert np.isin(r.code[gu.DI_RUN[0]:gu.DI_RUN[1] + 1], (gu.I, gu.D)).all() and r.ism[gu.DI_RUN[0] - 1] and r.ism[gu.DI_RUN[1] + 1]
        assert not (r.code[gu.DI_RUN[0] + 1:gu.DI_RUN[1] + 1] == r.code[gu.DI_RUN[0]:gu.DI_RUN[1]]).any()
        assert r.code[gu.AT_256] == gu.I and r.len[gu.AT_256] > 0 and r.ism[gu.AT_256 - 1]
    r = by["struct"]
    assert (r.code[gu.EQ_RUN[0]:gu.EQ_RUN[1] + 1] == gu.EQ).all() and r.code[gu.EQ_RUN[0] - 1] != gu.EQ and r.code[gu.EQ_RUN[1] + 1] != gu.EQ
    assert (r.len[gu.EQ_RUN[0]:gu.EQ_RUN[1] + 1] > 0).all() and gu.EQ_RUN[0] < 64 <= gu.EQ_RUN[1]
    assert unpack(r.words[gu.ZEROS[0]:gu.ZEROS[1] + 1].astype(np.uint32)) == "5=0=6=0I2I7="
    assert r.len[gu.ZERO_AT] == 0 and gu.ZERO_AT % gu.GCP == 0 and gu.AT_256 % 256 == 0
    xr = slice(gu.X_RUN[0], gu.X_RUN[1] + 1)
    assert (r.code[xr] == gu.X).all() and (r.len[xr] == 1).all() and gu.X_RUN[1] - gu.X_RUN[0] + 1 == 130
    assert gu.X_RUN[0] <= 384 and 447 < gu.X_RUN[1]                    # the step 384 .. 447 lies inside the run
    assert r.code[gu.X_RUN[0] - 2] != gu.X and r.code[gu.X_RUN[1] + 1] != gu.X
    g = by["struct_regular"]
    assert not g.irregular and (g.len > 0).all()
    if t0 == 0:
        assert by["lead_3S"].words[0] == gu.op(3, gu.S) and by["lead_2H"].words[0] == gu.op(2, gu.H)
        z = by["lead_zeros_4S"]
        assert (z.len[:70] == 0).all() and z.words[70] == gu.op(4, gu.S) and not np.isin(z.code[:70], (gu.I, gu.D)).any()
        for name in ("lead_3S", "lead_2H", "lead_zeros_4S", "lead_400S"):
            assert by[name].wrapped and by[name].has_cp and by[name].t_st == 0 and int(norm["first_op"][by[name].r]) == 0, name
        assert 3 * 400 > by["lead_400S"].N > 2 * 400
        assert sum(r.wrapped for r in by.values()) == 4
    else:
        assert not any(r.wrapped for r in by.values())


def _count(dec, pred):
    return sum(1 for d in dec.values() if pred(d))


def test_model_finds_every_branch(inputs):
    """the counts the issue asks for, over the windows of the t_st = 1000 batch (the GPU file runs these very lists)"""
    x = inputs[1000]
    recs, by = x["recs"], x["by_name"]
    irr = [r for r in recs if r.irregular]
    dec = {}
    for tag, w in [(f"edge{d}", gu.edge_windows(recs, d)) for d in (-1, 0, 1)] + [("special", gu.special_windows(recs))]:
        for k, v in gu.decisions(irr, w).items():
            dec[(tag,) + k] = v
    long_rec = by["long"]
    dl = gu.decisions([long_rec], gu.long_windows(long_rec))
    counts = dict(
        pairs=len(dec),
        jump1=_count(dec, lambda d: d["jump1"]),
        jump2=_count(dec, lambda d: d["jump2"]),
        second=_count(dec, lambda d: d["second"]),
        straddle=_count(dec, lambda d: d["straddle"]),
        both_steps=_count(dec, lambda d: "fast" in d["steps"] and "general" in d["steps"]),
        carried=_count(dec, lambda d: d["carried"]),
        no_start=_count(dec, lambda d: d["no_start"]),
        k1_nonzero=_count(dec, lambda d: d["k1"] > 0),
        k3_ge_64=_count(dl, lambda d: d["k3"] >= 64),
        long_jump2=_count(dl, lambda d: d["jump2"]),
        long_k1_ge_32=_count(dl, lambda d: d["k1"] >= 32),
    )
    print("generic inputs, model counts:", counts)
    for k, v in counts.items():
        assert v >= 5, (k, counts)
    # an equal range straddles a checkpoint at the I op of index 256 (the last reference base in front of it is op 255's)
    s = by["struct"]
    d = s.decide(s.P(gu.AT_256) - 1, s.P(gu.AT_256) + 2)
    assert d["straddle"] and d["k1"] == gu.AT_256 // gu.GCP - 1 and d["equal"][1] - d["equal"][0] == int(s.len[gu.AT_256])
    # and the second attempt is what a window that ends deep in the D / I run needs
    d = s.decide(s.P(2), s.P(gu.DI_RUN[0] + 120) + 1)
    assert d["jump2"] and d["second"] and d["status"] == 0 and d["ib"] == gu.DI_RUN[0] - 1


@pytest.mark.parametrize("t0", [1000, 0])
def test_model_against_the_oracle(oracle, inputs, t0):
    """status, row and clipped ops of every pair the model decides (every record whose tpos_aln is sorted), modern policy"""
    x = inputs[t0]
    b, recs = x["b"], x["recs"]
    lists = [gu.edge_windows(recs, d) for d in (-1, 0, 1)] + [gu.special_windows(recs), gu.long_windows(x["by_name"]["long"])]
    n_checked = 0
    for w in lists:
        rows, ops = _orows(oracle, b, w)
        dec = gu.decisions(recs, w)
        assert len(rows) == len(dec)
        for row in rows:
            d = dec[(int(row["rec"]), int(row["win"]))]
            if d["wrapped"]:
                continue
            what = (b["names"][int(row["rec"])], int(w[1][row["win"]]), int(w[2][row["win"]]))
            assert int(row["status"]) == d["status"], (what, int(row["status"]), d["status"])
            if d["status"] != 0:
                continue
            assert bool(row["flags"] & 1) == d["inside"], what
            got = ops[int(row["out_off"]):int(row["out_off"]) + int(row["out_n"])]
            assert np.array_equal(got.astype(np.int64), d["clip"]), (what, unpack(got[:8]), unpack(d["clip"][:8].astype(np.uint32)))
            if not d["inside"]:
                for k, v in d["row"].items():
                    assert int(row[k]) == v, (what, k, int(row[k]), v)
            n_checked += 1
    assert n_checked > 1000


@pytest.mark.parametrize("t0", [1000, 0])
def test_oracle_rows_of_the_lists(oracle, inputs, t0):
    """with the oracle alone: most rows are clips, some are 'none', and the two policies differ (the equal range matters)"""
    x = inputs[t0]
    b, recs = x["b"], x["recs"]
    n_diff = 0
    for tag, w in [(f"edge{d}", gu.edge_windows(recs, d)) for d in (-1, 0, 1)] + [("special", gu.special_windows(recs)),
                                                                                  ("unsorted", gu.unsorted_windows(recs))]:
        per = {}
        for pol in (MODERN, LEGACY):
            rows, ops = _orows(oracle, b, w, pol)
            ok, none = int((rows["status"] == 0).sum()), int((rows["status"] == 1).sum())
            print(f"t_st={t0} {tag} policy={pol}: {len(w[1])} windows, {len(rows)} rows, {ok} clips, {none} none, "
                  f"{int((rows['status'] == 16).sum())} not found")
            assert ok >= 0.6 * len(rows) and none >= 5, (tag, pol, len(rows), ok, none)
            per[pol] = (rows, ops)
        (ra, oa), (rb, ob) = per[MODERN], per[LEGACY]
        assert len(ra) == len(rb)
        differs = np.zeros(len(ra), bool)
        for k in ("status", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_n"):
            differs |= ra[k] != rb[k]
        n_diff += len(np.unique(ra["win"][differs])) if tag != "unsorted" else 0
    print(f"t_st={t0}: windows whose modern and legacy rows differ: {n_diff}")
    assert n_diff >= 3
    if t0 == 0:
        # the record with 400 units at position -1: the probe sequence runs into them, and rows come out that a sorted array would not give
        r = x["by_name"]["lead_400S"].r
        rows, _ = _orows(oracle, b, gu.edge_windows(recs, 0))
        mine = rows[rows["rec"] == r]
        assert (mine["status"] == 16).sum() >= 5 and (mine["status"] == 0).sum() >= 5, np.bincount(mine["status"])


def test_unsorted_list_is_unsorted_and_long(inputs):
    recs = inputs[1000]["recs"]
    wc, st, en = gu.unsorted_windows(recs)
    assert len(st) >= 200 and (np.diff(st.astype(np.int64)) < 0).sum() > 50 and len(np.unique(wc)) == 1
    # every record meets more than 64 of them: rb_defer_record carries its count over ballot steps
    for r in recs:
        assert int(((r.t_en > st.astype(np.int64)) & (r.t_st < en.astype(np.int64))).sum()) > 64, r.name
    wc, st, en = gu.edge_windows(recs, 0)
    assert (np.diff(st.astype(np.int64)) > 0).all() and (np.diff(en.astype(np.int64)) > 0).all()   # sorted: the monotone route


def test_regular_copy_windows_deep_in_the_run(inputs):
    """the regular copy reaches the generic kernel through RB_WALK_MAX alone: windows that start or end more than 24 ops deep"""
    g = inputs[1000]["by_name"]["struct_regular"]
    w = gu.special_windows(inputs[1000]["recs"])
    deep = gu.deep_windows(g, w)
    assert len(deep) >= 8
