"""The inputs of tests/test_gpu_largest.py hold what they are meant to hold, and its reference says what the reference program says.

No GPU.  (a) largest_ref (tests/largest_util.py, written from main.rs:200-208) over the oracle's liftover rows reproduces the oracle CLI's
`liftover --largest`, line for line, with window ids that are all different and with ids that repeat.  (b) The fabricated row sets
contain every case rb_dev_largest can get wrong, counted here from the arrays, so a change to a builder that loses one fails this file."""
import os

import numpy as np
import pytest

import largest_util as lu
from golden.make_digests import tile_bed
from rbtest_util import read_bed, read_paf
from rustybam_amd.capi import HIT_INSIDE


@pytest.mark.parametrize("bed_kind", ["tiles", "repeated_ids"])
def test_largest_ref_reproduces_the_oracle_cli(oracle, golden, tmp_path, bed_kind):
    paf = os.path.join(golden, "asm_small.paf")
    bed = str(tmp_path / "w.bed")
    (tile_bed if bed_kind == "tiles" else lu.repeated_id_bed)(bed)
    R = read_paf(paf)
    wc, ws, we, ids = read_bed(bed, R.contig_names)
    rows, _ = oracle.liftover(oracle.Batch(*R.arrays(), R.contig), wc, ws, we)
    win_key, inside_key, n_keys = lu.intern_ids(ids)
    if bed_kind == "repeated_ids":
        assert n_keys == 6 and len(ids) > 100
    sel, n_bad = lu.largest_ref(rows, win_key, np.full(R.n, inside_key, np.uint32), n_keys)
    assert n_bad == 0
    rc, out = oracle.cli("liftover", "--largest", "--bed", bed, paf)
    assert rc == 0
    lines = out.decode().splitlines()
    assert len(lines) == len(sel) > (100 if bed_kind == "tiles" else 4)
    for ln, k in zip(lines, sel):
        h, t = rows[int(k)], ln.split("\t")
        want_id = "" if int(h["flags"]) & HIT_INSIDE else ids[int(h["win"])]
        got = (t[0], int(t[2]), int(t[3]), t[5], int(t[7]), int(t[8]), [x for x in t[12:] if x.startswith("id:Z:")][0][5:])
        r = int(h["rec"])
        assert got == (R.q_name[r], int(h["q_st"]), int(h["q_en"]), R.t_name[r], int(h["t_st"]), int(h["t_en"]), want_id), (ln[:120], int(k))


def test_known_answer_of_the_property_set():
    s = lu.properties()
    sel, n_bad = lu.largest_ref(s["rows"], s["win_key"], s["rec_key"], s["n_keys"])
    assert sel.tolist() == [4, 8, 0, 14, 17, 20] and n_bad == 3   # keys 0, 1, 3, 4, 5, 6; keys 2 and 7 have no winner
    # without rec_key every INSIDE row is a bad key
    sel2, n_bad2 = lu.largest_ref(s["rows"], s["win_key"], None, s["n_keys"])
    assert n_bad2 == 2 + 5 and sel2.tolist() == [4, 8, 0, 17, 20]


def _per_key(s):
    rows = s["rows"]
    key, span, ok = lu.row_keys(rows, s["win_key"], s["rec_key"]), lu.spans(rows), rows["status"] == 0
    return rows, key, span, ok


def test_property_set_contains_every_case():
    s = lu.properties()
    rows, key, span, ok = _per_key(s)
    n_keys = s["n_keys"]
    tied = no_ok = top_not_ok = only_zero = 0
    for q in range(n_keys):
        m = key == q
        if not m.any():
            continue
        if not (m & ok).any():
            no_ok += 1
            continue
        top = span[m & ok].max()
        tied += int((span[m & ok] == top).sum() >= 3)
        top_not_ok += int(span[m & ~ok].max(initial=0) > top)
        only_zero += int((m & ok).sum() == 1 and top == 0)
    assert (tied, no_ok, top_not_ok, only_zero) == (1, 1, 2, 1)                # (key 1, and key 3 whose row of span 8 is not OK)
    assert ok[0] and span[0] == 0 and (key[ok] == key[0]).sum() == 1          # ... and that one is row 0
    inside = (rows["flags"] & HIT_INSIDE) != 0
    assert (inside & ok).sum() == 5
    assert (key[inside] != s["win_key"][rows["win"][inside]]).all()            # their window's key is another one
    assert (span[ok] >= 1 << 32).sum() >= 3
    lo = {}
    for q, v in zip(key[ok & (key < n_keys)], span[ok & (key < n_keys)]):
        lo.setdefault((int(q), int(v) & 0xFFFFFFFF), set()).add(int(v) >> 32)
    assert sum(len(v) >= 2 for v in lo.values()) >= 1                          # equal low halves, different high halves, on one key
    assert (ok & (key >= n_keys)).sum() == 3 and (~ok & (key >= n_keys)).sum() == 1
    assert not (key == 7).any() and not (key == 2)[ok].any()                    # gaps for the compaction


def test_shapes_of_the_other_sets():
    for n in (0, 1, 63, 64, 65, 257):
        s = lu.one_key(n)
        assert len(s["rows"]) == n and len(set(lu.spans(s["rows"]).tolist())) <= 1
        assert lu.largest_ref(s["rows"], s["win_key"], s["rec_key"], 1)[0].tolist() == ([n - 1] if n else [])
    s = lu.contended()
    rows, key, span, ok = _per_key(s)
    assert len(rows) == 20_000 and s["n_keys"] == 1 and (span == span.max()).sum() > 100
    s = lu.sparse()
    rows, key, span, ok = _per_key(s)
    assert s["n_keys"] == 70_001 and len(rows) == 5_000
    present = np.unique(key)
    assert len(present) < 5_000 and {0, 70_000} <= set(present.tolist())
    assert all(b in present and b - 1 in present for b in range(2048, 70_001, 2048))   # both sides of every block boundary of the scan
    s = lu.skewed(11)
    rows, key, span, ok = _per_key(s)
    assert len(rows) == 50_000
    hot = np.bincount(key[key < s["n_keys"]]).max()
    assert 0.4 * len(rows) < hot < 0.7 * len(rows)
    assert 0.08 < (~ok).mean() < 0.12 and 0.08 < ((rows["flags"] & HIT_INSIDE) != 0).mean() < 0.12
    assert (ok & (key >= s["n_keys"])).sum() > 10 and (span >= 1 << 32).sum() > 1000
