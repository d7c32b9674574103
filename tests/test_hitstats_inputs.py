"""What the inputs of tests/test_gpu_hitstats.py hold, proved on the CPU (tests/hitstats_util.py builds them; the oracle gives the
references).  A GPU test that passes on inputs that lack a case proves nothing about that case: each case is asserted here."""
import numpy as np

import hitstats_util as hu
import rustybam_amd

DESC, INSIDE = rustybam_amd.HIT_DESCRIPTOR, rustybam_amd.HIT_INSIDE


def test_kernel_shape_constants():
    row_step, wave_step, row_max = hu.kernel_shape()
    assert row_step == 16 * 4 and wave_step == 64 * 4  # (four ops per lane and load)
    assert row_max % wave_step == 0 and row_max >= 2 * wave_step


def test_hand_made_rows_hold_every_case(oracle):
    H = hu.hand_made()
    rows, out, kind = H.rows, H.out_ops, np.array(H.kind)
    row_step, wave_step, row_max = hu.kernel_shape()
    ok = rows["status"] == 0
    plain = ok & ((rows["flags"] & DESC) == 0)
    desc = ok & ((rows["flags"] & DESC) != 0)
    n = np.array([len(c) if c is not None else 0 for c in H.clips])
    # every clip is where its row says, and the expansion the reference uses finds it
    for k in np.nonzero(ok)[0]:
        assert np.array_equal(hu.expand(rows[k], out, H.ops, H.op_off), H.clips[k])
    # plain clips: every length at every word offset mod 4
    want_len = set(hu.short_lengths())
    assert {1, 2, 3} <= want_len and all(m * s + d in want_len for s in (row_step, wave_step) for m in (1, 2) for d in (-1, 0, 1))
    for ln in want_len:
        assert {int(o) % 4 for o in rows["out_off"][plain & (n == ln) & (kind == "short")]} == {0, 1, 2, 3}, ln
    # the wavefront form: one op past the row form's limit, its own step edges, 70,000 ops; plain and through a descriptor
    long_n = set(n[plain & (n > row_max)])
    assert row_max + 1 in long_n and 70_000 in long_n
    assert any(v % wave_step == 0 for v in long_n) and any(v % wave_step == 1 for v in long_n) and any(v % wave_step == wave_step - 1 for v in long_n)
    assert (desc & (n > row_max) & ((rows["flags"] & INSIDE) != 0)).any() and (desc & (n > row_max) & ((rows["flags"] & INSIDE) == 0)).any()
    # a wavefront's four rows: short beside long, OK beside not-OK, plain beside descriptor
    quads = [slice(q, q + 4) for q in range(0, len(rows) - 3, 4)]
    assert any((n[q][ok[q]] > row_max).any() and (n[q][ok[q]] <= row_max).any() for q in quads)
    assert sum(ok[q].any() and (~ok[q]).any() for q in quads) >= 5
    assert sum(plain[q].any() and desc[q].any() for q in quads) >= 5
    # descriptors: one-op clips with both, one and no end length, multi-op clips likewise, INSIDE rows whose d[2], d[3] are garbage
    out4 = np.concatenate([out, np.zeros(4, np.uint32)])
    d = np.array([[int(x) for x in out4[int(o):int(o) + 4]] for o in rows["out_off"]])
    one, multi, ins = desc & (d[:, 1] == 1) & ((rows["flags"] & INSIDE) == 0), desc & (d[:, 1] > 1) & ((rows["flags"] & INSIDE) == 0), desc & ((rows["flags"] & INSIDE) != 0)
    for sel in (one, multi):
        assert {(bool(a), bool(b)) for a, b in d[sel][:, 2:4]} == {(True, True), (True, False), (False, True), (False, False)}
    assert ins.sum() >= 3 and (d[ins][:, 2] > 1 << 27).all()
    for k in np.nonzero(ins)[0]:  # INSIDE: the record's own ops, lengths untouched
        st = int(H.op_off[rows["rec"][k]]) + d[k, 0]
        assert np.array_equal(H.clips[k], H.ops[st:st + d[k, 1]])
    k = int(np.nonzero(kind == "desc-one-both")[0][0])
    assert int(H.clips[k][0]) >> 4 == 100 + 120 - 150
    assert {int(o) % 4 for o in rows["out_off"][desc]} == {0, 1, 2, 3}  # descriptors at every word offset
    starts = {(int(H.op_off[rows["rec"][k]]) + d[k, 0]) % 4 for k in np.nonzero(desc)[0]}
    assert starts == {0, 1, 2, 3}  # and their ops in the batch too
    # op codes: all nine inside clips, M among them; continuation words
    codes = np.concatenate([c & 15 for c in H.clips if c is not None])
    assert set(range(9)) <= set(codes.tolist()) and 14 in codes
    want = hu.oracle_stats(oracle, rows, H.clips)
    assert (want["flags"][ok] & hu.F_HAS_M).any() and not (want["flags"][ok] & hu.F_HAS_M).all()
    assert (want["matches"] > 0).any() and ((want["diff"] > want["matches"]) & (want["matches"] > 0)).any()
    k = int(np.nonzero(kind == "cont-I")[0][0])
    assert want["ins_events"][k] == 1 and want["ins"][k] >= 1 << 28
    assert (want["equal"][kind == "cont-EQ"] >= 3_000_000_000).all() and (kind == "cont-EQ").sum() == 2
    k = int(np.nonzero(kind == "X-only")[0][0])
    assert want["equal"][k] == 0 and all(want[f][k] == 0.0 for f in hu.RATIOS)
    # no ratio is NaN: a clip starts on a match op, so equal + diff > 0 (the NaN case cannot arise from a clip)
    assert not any(np.isnan(want[f]).any() for f in hu.RATIOS)
    assert all((int(c[0]) & 15) in (0, 7, 8) for c in H.clips if c is not None)
    # wrong spans
    assert set(want["status"][np.char.startswith(kind, "wrong")]) == {hu.ST_T, hu.ST_Q}
    assert (want["status"][ok & ~np.char.startswith(kind, "wrong")] == 0).all()
    # rows that are not OK: all zero but the status
    assert (~ok).sum() >= 8 and len(set(rows["status"][~ok])) >= 6
    z = want[~ok].copy()
    z["status"] = 0
    assert z.tobytes() == bytes(z.nbytes)
    # out_ops ends with the last clip, rounded up to four words; a clip's neighbours in its granules are not zero
    ends = [int(h["out_off"]) + (4 if h["flags"] & DESC else int(h["out_n"])) for h in rows[ok]]
    assert len(out) == (max(ends) + 3) // 4 * 4 and max(ends) % 4 != 0
    assert (out == hu.GARBAGE).sum() >= 40
    # the references are not all alike
    assert len({tuple(x) for x in want[["equal", "diff", "ins", "del"]][ok].tolist()}) >= 20


def test_real_input_holds_every_kind_of_row(oracle):
    inp = hu.real_input(oracle)
    n_ops = np.diff(inp.b["op_off"])
    assert len(n_ops) == 96 and inp.odd.sum() >= 8 and n_ops[~inp.odd].min() >= 150 and n_ops.max() <= 6000
    assert {int(s) for s in inp.b["strand"]} == {ord("+"), ord("-")}
    _, row_step_w, row_max = hu.kernel_shape()
    for legacy in (False, True):
        t = hu.real_truth(oracle, legacy)
        r = t.rows
        ok = r["status"] == 0
        assert (ok & ((r["flags"] & 1) != 0)).sum() >= 96  # INSIDE rows: the window that contains every record
        assert (~ok).sum() >= 3                              # rows the reference drops
        assert inp.odd[r["rec"][ok]].sum() >= 10             # rows of irregular records: the generic kernel's
        assert (~inp.odd[r["rec"][ok]]).sum() >= 1000        # rows of regular records: descriptor-eligible
        assert (r["out_n"][ok] > row_max).any() and (r["out_n"][ok] < 64).any()  # both forms of the kernel
        assert len({tuple(x) for x in t.stats[["equal", "diff", "ins", "del"]][ok].tolist()}) >= 200
        assert (t.stats["status"][ok] == 0).all()
    for max_size in (0, 100):
        t = hu.real_truth(oracle, False, max_size)
        ok = t.rows["status"] == 0
        assert ok.sum() >= 300 and (t.stats["status"][ok] == 0).all()
    assert len(hu.real_truth(oracle, False, 0).rows) > 10 * len(hu.real_truth(oracle, False, 100).rows)
