"""The contract of the text entry points (rb_host_*_text) at the front they share: what each one writes, and what it leaves alone, on
an empty file, on a file with a CIGAR that does not parse, on a small good file (against the oracle), and when it refuses its arguments.
Every caller-owned output is filled with a sentinel before the call (tests/qbed_util.py: _text_call), so "untouched" is observable."""
import numpy as np
import pytest

import largest_util as lu
import pairs_util as pu
import qbed_util as qu
from rustybam_amd import capi

pytestmark = pytest.mark.gpu

NAMES = list(qu.TEXT_ENTRY_POINTS)
FORM = {k: v[0] for k, v in qu.TEXT_ENTRY_POINTS.items()}
END = {k: v[2] for k, v in qu.TEXT_ENTRY_POINTS.items()}
BREAK_LIFTOVER = ("rb_host_break_liftover_text", "rb_host_break_liftover_stats_text")
MAX_SIZE = 10
WINDOWS = [(0, 105, 112), (1, 25, 40)]  # one cuts record 0 of GOOD, one contains its record 2
WIN_KEY, INSIDE_KEY, N_KEYS = lu.intern_ids(["a", "b"])

EMPTY = qu.text_batch([], [], [], "", [], WINDOWS)
BAD = qu.text_batch(["4=", "5M3", "2=1X2="], [100, 400, 30], [5, 50, 7], "+-+", [0, 0, 1], WINDOWS)
# record 1 is cut at its 20D by break-paf; on '-' and longer than record 0, it turns the pair (key 0) they share around under --orient
GOOD = qu.text_batch(["10=2X8=", "16=20D6=2I4=", "2=1X2="], [100, 400, 30], [5, 50, 7], "+-+", [0, 0, 1], WINDOWS)


def pairs_of(d, mode=pu.ORIENT):
    n = len(d["strand"])
    return dict(rec_key=[0, 0, 1][:n], rec_q_len=[1000] * n, n_keys=2 if n else 0, mode=mode)


def call(engine, name, d, **kw):
    return qu.text_entry(engine, name, d, max_size=MAX_SIZE, largest=(WIN_KEY, N_KEYS, INSIDE_KEY), pairs=kw.pop("pairs", pairs_of(d)), **kw)


def outs_of(name):
    """the out-pointers entry point `name` has"""
    return {"text": ("rows", "row_text_off", "row_text"), "stats": ("rows", "stats"), "scan": ()}[FORM[name]]


# ---------------------------------------------------------------------------------------------- (a) an empty file
@pytest.mark.parametrize("name", NAMES)
def test_an_empty_file(engine, name):
    r = call(engine, name, EMPTY)
    assert r["rc"] == 0
    if FORM[name] == "scan":
        return
    assert r["n_rows"] == 0
    for k in outs_of(name):
        assert r["ptr"][k] == ("set" if k == "row_text_off" else "null"), k
    if FORM[name] == "text":
        assert r["off"].tolist() == [0, 0]
    assert not r["counters"].view(np.uint8).any()
    if END[name]:
        assert r["declined"] == 0
    if END[name] == "pieces":
        assert r["row_piece"] is None


# ---------------------------------------------------------------------------------------------- (b) a CIGAR that does not parse
@pytest.mark.parametrize("name", NAMES)
def test_a_cigar_that_does_not_parse(engine, name):
    r = call(engine, name, BAD)
    assert r["rc"] == 0
    st = r["cig_status"].tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] not in (0, qu.SENTINEL)
    assert qu.untouched(r["red"]) and qu.untouched(r["norm"])
    if FORM[name] == "scan":
        return
    assert r["n_rows"] == 0
    for k in outs_of(name):
        assert r["ptr"][k] == "null", k  # (*row_text_off too: unlike the empty file, nothing is allocated)
    # the counters: the pipeline's pair clears them before it parses, the others leave them alone when they stop here
    if name in BREAK_LIFTOVER:
        assert not r["counters"].view(np.uint8).any()
    else:
        assert qu.untouched(r["counters"])
    if END[name]:
        assert r["declined"] == 0
    if END[name] == "pairs":
        assert not r["key_flip"].any()
    if END[name] == "pieces":
        assert r["row_piece"] is None


# ---------------------------------------------------------------------------------------------- (c) three good records, against the oracle
@pytest.fixture(scope="module")
def want(oracle):
    """what the plain form of every route must give on GOOD: name -> dict(rows, text), all from the oracle and the numpy references"""
    d = GOOD
    b = oracle.Batch(d["ops"], d["op_off"], d["t_st"], d["t_en"], d["q_st"], d["q_en"], d["strand"], d["contig"])
    rows, out = oracle.liftover(b, d["w_contig"], d["w_st"], d["w_en"])
    lift = dict(rows=rows, text=qu.rows_text(rows, out))
    sel, bad = lu.largest_ref(rows, WIN_KEY, np.full(3, INSIDE_KEY, np.uint32), N_KEYS)
    assert bad == 0 and len(sel) == 2
    sel = sel.astype(np.int64)
    brows, bout = oracle.break_paf(b, MAX_SIZE)
    brk = dict(rows=brows, text=qu.rows_text(brows, bout))
    assert len(brows) == 4 and (brows["status"] == 0).all()
    p = pairs_of(d)
    m = pu.model(pu.case("good", capi.hit_rows_from(brows), p["rec_key"], p["rec_q_len"], d["strand"], p["n_keys"], mode=p["mode"]))
    assert m.key_flip.tolist() == [1, 0] and int(m.info["declined"]) == 0 and m.keep.all()
    pairs = dict(rows=m.rows_out, text=brk["text"], key_flip=m.key_flip)
    # the pieces as the second command reads them: every row of break-paf one record, its strand and contig its parent's
    parent = brows["rec"].astype(np.int64)
    clips = [bout[int(h["out_off"]):int(h["out_off"]) + int(h["out_n"])] for h in brows]
    p_off = np.zeros(len(brows) + 1, np.uint64)
    p_off[1:] = np.cumsum([len(c) for c in clips])
    pb = oracle.Batch(np.concatenate(clips).astype(np.uint32), p_off, brows["t_st"].astype(np.uint64), brows["t_en"].astype(np.uint64),
                      brows["q_st"].astype(np.uint64), brows["q_en"].astype(np.uint64), d["strand"][parent], d["contig"][parent])
    prows, pout = oracle.liftover(pb, d["w_contig"], d["w_st"], d["w_en"])
    assert len(prows) == 2
    piece = prows["rec"].astype(np.uint32)
    text = qu.rows_text(prows, pout)
    prows = prows.copy()
    prows["rec"] = parent[piece]
    return {"rb_host_liftover_text": lift, "rb_host_liftover_largest_text": dict(rows=rows[sel], text=[lift["text"][k] for k in sel]),
            "rb_host_break_text": brk, "rb_host_break_pairs_text": pairs,
            "rb_host_break_liftover_text": dict(rows=prows, text=text, row_piece=piece),
            "scan": dict(red=oracle.reduce(b), norm=oracle.normalize(b))}


@pytest.fixture(scope="module")
def got(engine):
    return {name: call(engine, name, GOOD) for name in NAMES}


def check_rows(g, w):
    rows, orows = g["rows"], w["rows"]
    assert len(rows) == len(orows) and g["n_rows"] == len(orows)
    for k in ("rec", "win", "status"):
        assert np.array_equal(rows[k].astype(np.int64), orows[k].astype(np.int64)), k
    ok = orows["status"] == 0
    for k in ("t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len"):
        assert np.array_equal(rows[k][ok].astype(np.uint64), orows[k][ok].astype(np.uint64)), k
    assert np.array_equal((rows["flags"] & 1)[ok], (orows["flags"] & 1)[ok].astype(rows["flags"].dtype))
    assert g["text"] == w["text"]


@pytest.mark.parametrize("name", [n for n in NAMES if FORM[n] == "text"])
def test_the_plain_forms_equal_the_oracle(got, want, name):
    g, w = got[name], want[name]
    assert g["rc"] == 0 and not g["cig_status"].any()
    if END[name]:
        assert g["declined"] == 0
    check_rows(g, w)
    assert len(g["rows"]) > 0
    if END[name] == "pairs":
        assert np.array_equal(g["key_flip"], w["key_flip"])
    if END[name] == "pieces":
        assert np.array_equal(g["row_piece"], w["row_piece"])
    for k in ("status", "t_bases", "q_bases", "nmatch", "aln_len"):
        assert np.array_equal(g["red"][k], want["scan"]["red"][k]), k
    for k in ("status", "t_st", "t_en", "q_st", "q_en", "first_op", "n_ops"):
        assert np.array_equal(g["norm"][k], want["scan"]["norm"][k]), k


@pytest.mark.parametrize("name", [n for n in NAMES if FORM[n] == "stats"])
def test_the_stats_forms_give_the_rows_of_the_plain_forms(got, name):
    g, plain = got[name], got[name.replace("_stats_text", "_text")]
    assert g["rc"] == 0 and plain["rc"] == 0
    assert g["rows"].tobytes() == plain["rows"].tobytes() and len(g["rows"]) > 0
    assert len(g["stats"]) == len(g["rows"]) == g["n_rows"] and g["ptr"]["stats"] == "set"
    assert (g["stats"]["status"] == 0).all()
    for k in ("key_flip", "row_piece", "declined"):
        if k in plain:
            assert np.array_equal(g[k], plain[k]), k


def test_scan_text_gives_the_rows_of_liftover_text(got):
    s, l = got["rb_host_scan_text"], got["rb_host_liftover_text"]
    assert s["rc"] == 0 and not s["cig_status"].any()
    assert s["red"].tobytes() == l["red"].tobytes() and s["norm"].tobytes() == l["norm"].tobytes()
    assert not qu.untouched(s["red"]) and not qu.untouched(s["norm"])


# ---------------------------------------------------------------------------------------------- (d) the refusals
def assert_refused(r):
    """RB_E_INVALID, and every output as the caller left it"""
    assert r["rc"] == qu.E_INVALID
    assert qu.untouched(r["cig_status"]) and qu.untouched(r["red"]) and qu.untouched(r["norm"]) and qu.untouched(r["counters"])
    assert r["n_rows"] == qu.UNTOUCHED
    assert all(v in ("untouched",) for v in r["ptr"].values()), r["ptr"]
    assert r.get("declined", qu.INT_UNTOUCHED) == qu.INT_UNTOUCHED
    assert "key_flip" not in r or qu.untouched(r["key_flip"])
    assert r.get("row_piece", "untouched") == "untouched"


@pytest.mark.parametrize("name", [n for n in NAMES if FORM[n] == "stats"])
def test_a_stats_form_without_stats_is_refused(engine, name):
    assert_refused(call(engine, name, GOOD, null=("stats",)))


@pytest.mark.parametrize("name", ["rb_host_break_text", "rb_host_break_liftover_text"])
def test_break_routes_refuse_qbed(engine, name):
    r = call(engine, name, GOOD, policy=qu.LIFT_QBED)
    assert_refused(r)
    assert "RB_LIFT_QBED" in r["error"]


def test_largest_refuses_keys_outside_the_key_space(engine):
    name = "rb_host_liftover_largest_text"
    assert_refused(qu.text_entry(engine, name, GOOD, largest=(np.array([0, N_KEYS], np.uint32), N_KEYS, INSIDE_KEY)))
    assert_refused(qu.text_entry(engine, name, GOOD, largest=(WIN_KEY, N_KEYS, N_KEYS)))


def test_pairs_refuses_an_unknown_mode_bit(engine):
    assert_refused(call(engine, "rb_host_break_pairs_text", GOOD, pairs=pairs_of(GOOD, mode=pu.ORIENT | 4)))


def test_liftover_text_without_rows_is_refused(engine):
    r = call(engine, "rb_host_liftover_text", GOOD, null=("rows",))
    assert r["ptr"]["rows"] == "untouched"  # (the caller's variable: it was not passed)
    assert_refused(r)
