"""What the inputs of tests/test_gpu_rows_to_batch.py hold, and that the numpy model of rb_dev_rows_to_batch (tests/rows_batch_util.py) is the
contract: proved on the CPU, against the oracle's break_paf where ops are concerned.

The thresholds the lengths are built around are IMPORTED from the library (rb_rows_to_batch_shape), not mirrored."""
import numpy as np

import rows_batch_util as ru
import rustybam_amd
from rbtest_util import unpack

DESC, INSIDE = rustybam_amd.HIT_DESCRIPTOR, rustybam_amd.HIT_INSIDE


def test_shape_is_the_kernels():
    """the constants come out of the library, and are the ones k_rows_batch.hip defines"""
    import os
    import re
    txt = open(os.path.join(ru.ROOT, "rustybam_amd", "csrc", "k_rows_batch.hip")).read()
    want = tuple(int(re.search(rf"#define {k} (\d+)u", txt).group(1)) for k in ("RB_RTB_ROW_STEP", "RB_RTB_ROW_MAX", "RB_RTB_WAVE_STEP"))
    assert ru.kernel_shape() == want
    row_step, row_max, wave_step = want
    assert row_step == 64 and wave_step == 256, "a step is one 16-byte group per lane: 16 and 64 lanes"
    assert row_max % wave_step == 0 and row_max > 2 * row_step


def test_hand_made_rows_hold_what_they_claim():
    H = ru.hand_made()
    rows, kind = H.rows, H.kind
    ok = rows["status"] == 0
    n = np.where(ok, np.where(rows["flags"] & DESC, [int(H.out_ops[int(o) + 1]) if f & DESC else 0 for o, f in zip(rows["out_off"], rows["flags"])], rows["out_n"]), 0)
    row_step, row_max, wave_step = ru.kernel_shape()
    # one-op pieces, a one-op descriptor clip with both lengths replaced, INSIDE rows, both forms
    assert (n[ok] == 1).sum() >= 4
    k = kind.index("desc-one-both")
    d = H.out_ops[int(rows["out_off"][k]):][:4]
    assert rows["flags"][k] == DESC and d[1] == 1 and d[2] and d[3]
    assert ((rows["flags"][ok] & INSIDE) != 0).sum() >= 4
    assert ((rows["flags"][ok] & DESC) != 0).any() and ((rows["flags"][ok] & DESC) == 0).any()
    # rows the reference dropped between OK rows, and none it panicked on (those are declining()'s)
    bad = np.nonzero(~ok)[0]
    assert set(rows["status"][bad]) == {1, 2, 3, 4, 5}
    assert all(0 < b < len(rows) - 1 and ok[:b].any() and ok[b + 1:].any() for b in bad)
    assert not H.model.declined
    # plain clips 0, 1, 2 and 3 words past a 16-byte boundary; descriptor clips too
    plain = ok & ((rows["flags"] & DESC) == 0)
    assert set(rows["out_off"][plain] % 4) == {0, 1, 2, 3}
    assert {h for h, f in zip(H.src_head, rows["flags"]) if h is not None and f & DESC} == {0, 1, 2, 3}
    # every threshold: T - 1, T, T + 1, as a plain clip and (up to the row limit) as a descriptor clip
    T = [row_step, 2 * row_step, wave_step, row_max, (row_max // wave_step + 1) * wave_step, (row_max // wave_step + 2) * wave_step]
    for t in T:
        for dlt in (-1, 0, 1):
            assert (n[plain] == t + dlt).any(), f"no plain clip of {t + dlt} ops"
            if t <= row_max and t + dlt <= row_max:
                assert (n[ok & ~plain] == t + dlt).any(), f"no descriptor clip of {t + dlt} ops"
    # the short clips at every pair of (source, destination) word offsets: the shift between the two is what the copy kernel turns on
    dst = np.zeros(len(rows), np.int64)
    dst[ok] = H.model.op_off[:-1].astype(np.int64)
    for t in (1, 2, 3, 4, 5, row_step - 1, row_step, row_step + 1, 2 * row_step - 1, 2 * row_step, 2 * row_step + 1):
        sel = np.nonzero(plain & (n == t) & np.array([k_.startswith("plain") for k_ in kind]))[0]
        pairs = {(H.src_head[i], int(dst[i]) % 4) for i in sel}
        assert len(pairs) == 16, f"{t}-op clips: (source, destination) offsets {sorted(pairs)}"
    # the wavefront form: every shift 0 .. 3 among the long clips
    long_ = np.nonzero(ok & (n > row_max))[0]
    assert {(int(dst[i]) - H.src_head[i]) % 4 for i in long_} == {0, 1, 2, 3}
    assert n.max() >= 80_000
    # long and short, OK and not OK share a wavefront's four rows somewhere
    groups = [slice(i, i + 4) for i in range(0, len(rows) - 3, 4)]
    assert any((n[g] > row_max).any() and ((n[g] <= row_max) & ok[g]).any() and (~ok[g]).any() for g in groups)
    # continuation words inside a plain clip
    assert any(((H.out_ops[int(o):int(o) + int(c)] & 15) == 14).any() for o, c in zip(rows["out_off"][plain], rows["out_n"][plain]))
    # out_ops ends with the last clip rounded up to four words
    end = max(int(o) + (4 if f & DESC else int(c)) for o, c, f in zip(rows["out_off"][ok], rows["out_n"][ok], rows["flags"][ok]))
    assert len(H.out_ops) == (end + 3) // 4 * 4


def test_model_is_the_contract_on_the_hand_made_rows():
    """a second, slower statement of the rules, piece by piece"""
    H = ru.hand_made()
    m, p = H.model, 0
    for k, h in enumerate(H.rows):
        if h["status"] != 0:
            continue
        got = m.ops[int(m.op_off[p]):int(m.op_off[p + 1])]
        off = int(h["out_off"])
        if h["flags"] & DESC:
            first, count, d2, d3 = (int(x) for x in H.out_ops[off:off + 4])
            src = H.ops[int(H.op_off[h["rec"]]) + first:][:count].copy()
            assert len(got) == count
            if not h["flags"] & INSIDE:
                if count == 1 and d2 and d3:
                    src[0] = ((d2 + d3 - (int(src[0]) >> 4)) << 4) | (int(src[0]) & 15)
                else:
                    if d2:
                        src[0] = (d2 << 4) | (int(src[0]) & 15)
                    if d3:
                        src[-1] = (d3 << 4) | (int(src[-1]) & 15)
            assert np.array_equal(got, src), (k, H.kind[k])
        else:
            assert np.array_equal(got, H.out_ops[off:off + int(h["out_n"])]), (k, H.kind[k])
        assert (m.t_st[p], m.t_en[p], m.q_st[p], m.q_en[p]) == (h["t_st"], h["t_en"], h["q_st"], h["q_en"])
        assert m.parent[p] == h["rec"] and m.strand[p] == H.strand[h["rec"]] and m.contig[p] == H.contig[h["rec"]]
        p += 1
    assert p == m.n_pieces and m.op_off[p] == m.n_ops == len(m.ops)
    assert len(set(H.strand)) == 2 and len(set(H.contig)) > 2, "strand and contig must tell the parents apart"


def test_declining_sets():
    sets = ru.declining()
    assert [m.declined for _, _, _, m in sets] == [w[:3] != "ok:" for w, _, _, _ in sets]
    assert sum(m.declined for _, _, _, m in sets) >= 5 and sum(not m.declined for _, _, _, m in sets) >= 4
    for what, rows, out, m in sets:
        assert (rows["status"][[0, 2]] == 0).all(), what
        assert m.n_pieces == int((rows["status"] == 0).sum())


def test_model_on_the_oracles_break_paf(oracle):
    """asm_small.paf through the oracle's break_paf: the model of its rows is the pieces `rb break-paf` prints, op for op, and read back as
    a batch every piece passes the oracle's integrity check and normalises to itself (what the second command of the pipeline sees)"""
    b = ru.asm_small()
    ob = oracle.Batch(b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"], b["contig"])
    for max_size in (100, 7):
        rows, ops = oracle.break_paf(ob, max_size)
        hit = rustybam_amd.capi.hit_rows_from(rows)
        m = ru.model(hit, ops, b["ops"], b["op_off"], b["strand"], b["contig"])
        ok = np.nonzero(rows["status"] == 0)[0]
        assert m.n_pieces == len(ok) > len(b["strand"]) and not m.declined
        for p in (0, 1, len(ok) // 2, len(ok) - 1):
            h = rows[ok[p]]
            assert unpack(m.ops[int(m.op_off[p]):int(m.op_off[p + 1])]) == unpack(ops[int(h["out_off"]):int(h["out_off"]) + int(h["out_n"])])
        assert np.array_equal(m.ops, np.concatenate([ops[int(h["out_off"]):int(h["out_off"]) + int(h["out_n"])] for h in rows[ok]]))
        pb = oracle.Batch(m.ops, m.op_off, m.t_st, m.t_en, m.q_st, m.q_en, m.strand, m.contig)
        red, norm = oracle.reduce(pb), oracle.normalize(pb)
        assert (red["status"] == 0).all() and (norm["status"] == 0).all()
        assert (norm["first_op"] == 0).all() and np.array_equal(norm["n_ops"], np.diff(m.op_off).astype(np.uint32))
        assert (norm["lead_ops"] == 0).all() and (norm["trail_ops"] == 0).all(), "a piece starts and ends on a match op: nothing is stripped"
        assert (np.diff(m.op_off) == 1).any(), "one-op pieces"
        # a piece's parent is the record it was cut from: same strand, pieces in record order then piece order
        assert np.array_equal(m.parent, rows["rec"][ok]) and (np.diff(m.parent.astype(np.int64)) >= 0).all()


def test_starts_form_keeps_every_record():
    b = ru.asm_small()
    ops2, starts = ru.starts_form(b, np.random.default_rng(5))
    lens = np.diff(b["op_off"]).astype(np.int64)
    assert not np.array_equal(np.argsort(starts[:-1]), np.arange(len(lens))), "the starts must be shuffled"
    for r in (0, 1, len(lens) // 2, len(lens) - 1):
        assert np.array_equal(ops2[int(starts[r]):int(starts[r]) + int(lens[r])], b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])])
    assert len(ops2) > len(b["ops"])
