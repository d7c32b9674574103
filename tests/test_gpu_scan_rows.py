"""The row form of the record scan (rb_k_scan_rows, k_records.hip: a row of 16 lanes per short record, four records to a wavefront)
against the per-base oracle and the plain flag reference of tests/scan_util.py, on inputs placed on its geometry
(tests/test_scan_inputs.py proves what they hold).  Bit-exact throughout.  Every test asserts, through rb_ctx_scan_route, which kernel
scanned what: a test that relied on the routing constants alone would go blind when they move.

One-line mutations of rb_k_scan_rows this file was run against (each as a library variant): `n <= RB_SQ_MAX` -> `<`, `n >= 4u` -> `>= 5u`,
carry_w not updated between steps, the continuation branch's `len & 15u` -> `& 7u`, the high 20-bit piece dropped from sum40 and
`any_edge` -> `st == 0` fail 6 to 16 of the 21 tests each.  Removing the edge mask on `mylast` fails none, and no input can make it:
a lane's last word lies outside its record only in the row's last step (its index is >= n only when the step's 64 words reach past
n + head), where no later lane's in-record word and no later step reads it -- the mask is redundant beside the per-word `ok` test."""
import os

import numpy as np
import pytest

import rustybam_amd
import scan_util as su
from rbtest_util import CONT, batch_args, read_paf

pytestmark = pytest.mark.gpu

REG = su.F_REGULAR


@pytest.fixture(scope="module")
def gen():
    return su.batches(0)


def _where(b, **kv):
    return [r for r, t in enumerate(b["tags"]) if all(t.get(k) == v for k, v in kv.items())]


@pytest.mark.parametrize("name", su.BATCH_NAMES)
def test_generated_batch(engine, oracle, gen, name):
    """every field of both rows against the oracle, the flags of every row against the reference, the route asserted"""
    b = gen[name]
    red, norm = su.check_scan(engine, oracle, b, name, "wave" if name in su.WAVE_BATCHES else "rows")
    if name == "hostile":                                          # the neighbours' adjoining words leak into nothing
        mid = _where(b, kind="hostile_mid")
        assert (red["flags"][mid] & REG).all() and (norm["flags"][mid] & REG).all() and (red["status"][mid] == 0).all()
    if name.startswith("defects"):
        clean, bad = _where(b, kind="clean"), _where(b, kind="defect")
        assert (norm["flags"][clean] & REG).all() and not (red["flags"][bad] & REG).any() and not (norm["flags"][bad] & REG).any()
    if name == "magnitude":
        r = _where(b, kind="overflow_2048")[0]
        assert red["status"][r] == 22 and int(red["t_bases"][r]) == int(red["q_bases"][r]) == 2048 * ((1 << 28) - 1)
        assert red["status"][_where(b, kind="total_u32_max")[0]] == 0 and red["aln_len"][_where(b, kind="total_u32_max")[0]] == 0xFFFFFFFF
        assert red["status"][_where(b, kind="total_2_32")[0]] == 22
        r = _where(b, kind="events_all_indel")[0]
        assert (red["ins_events"][r], red["del_events"][r], norm["status"][r]) == (1024, 1024, 20)


@pytest.mark.parametrize("name", ["lengths_wild", "defects_300", "hostile", "magnitude"])
def test_same_rows_from_both_kernels(engine, gen, name):
    """the same records three ways: one batch (row form), chunks of at most 63 records (wave-per-record kernel), and with one very long
    record appended so that the batch mean passes 1536 ops (wave-per-record kernel): all rows identical, byte for byte"""
    b = gen[name]
    n = len(b["op_off"]) - 1
    red, norm = engine.scan_records(*batch_args(b))
    took, listed = engine.scan_route()
    assert (took, listed) == su.route(b["op_off"]) and took > 0 and took + listed == n
    parts = []
    for lo in range(0, n, su.ROWS_MIN_REC - 1):
        sub = su.subset(b, np.arange(lo, min(lo + su.ROWS_MIN_REC - 1, n)))
        parts.append(engine.scan_records(*batch_args(sub)))
        assert engine.scan_route() == (0, 0)
    red_c, norm_c = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    longer = su.with_long_record(np.random.default_rng(5), b)
    assert su.route(longer["op_off"]) == (0, 0) and int(longer["op_off"][-1]) // (n + 1) == su.ROWS_MEAN_MAX + 1
    red_l, norm_l = engine.scan_records(*batch_args(longer))
    assert engine.scan_route() == (0, 0)
    for what, r2, n2 in (("chunks", red_c, norm_c), ("long record appended", red_l[:n], norm_l[:n])):
        for rows, other, kind in ((red, r2, "reduce"), (norm, n2, "norm")):
            a, o = rows.view(np.uint8).reshape(n, -1), other.view(np.uint8).reshape(n, -1)
            bad = np.flatnonzero((a != o).any(axis=1))
            assert len(bad) == 0, f"{name}, {what}: {kind} rows differ at records {bad[:8]}: {rows[bad[:2]]} vs {other[bad[:2]]}"


def test_fixture_through_the_row_form(engine, oracle, golden):
    """the fixture's 208 records of 4 - 2048 ops (the whole fixture has a mean of 3118 ops and takes the wave-per-record kernel)"""
    r = read_paf(os.path.join(golden, "asm_small.paf"))
    full = dict(ops=r.ops, op_off=r.op_off, t_st=r.t_st, t_en=r.t_en, q_st=r.q_st, q_en=r.q_en, strand=r.strand, contig=r.contig)
    n = np.diff(r.op_off.astype(np.int64))
    assert su.route(r.op_off) == (0, 0)
    idx = np.flatnonzero((n >= su.ROW_MIN_OPS) & (n <= su.ROW_MAX_OPS))
    assert len(idx) == 208
    b = su.subset(full, idx)
    red, norm = su.check_scan(engine, oracle, b, "fixture, short records", "rows")
    assert engine.scan_route() == (208, 0)
    assert (red["status"] == 0).all() and (norm["flags"] & REG).all() and (red["flags"] & REG).all()   # minimap2 cigars are all "regular"


def test_long_ops_through_the_row_form(engine, oracle):
    """the records of tests/test_long_ops.py (lengths of 2^28 and more: continuation words) seven times over, so that the batch has 64
    records and more and the continuation branch of the row form runs"""
    from test_long_ops import CASES, _batch
    _, one, _ = _batch()
    b = su.concat([one] * 7)
    n = np.diff(b["op_off"].astype(np.int64))
    has_cont = np.array([((b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])] & 15) == CONT).any() for r in range(len(n))])
    assert (has_cont & (n >= su.ROW_MIN_OPS) & (n <= su.ROW_MAX_OPS)).sum() >= 7 * 6
    red, norm = su.check_scan(engine, oracle, b, "long ops x 7", "rows")
    assert engine.scan_route()[0] == int(((n >= su.ROW_MIN_OPS) & (n <= su.ROW_MAX_OPS)).sum())
    names = [ln.split()[0] for ln in CASES]
    regular = ((norm["flags"] & REG) != 0).reshape(7, len(CASES))
    assert regular[:, names.index("qH")].all() and regular[:, names.index("qG")].all() and not regular[:, names.index("qA")].any() \
        and not regular[:, names.index("qE")].any()


def test_scan_list_grows_and_nothing_leaks_into_the_next_call(oracle):
    """one context: 64 records, then 50,000, then 64 -- the context's list of the records the row form leaves to the wave-per-record
    kernel grows with the largest batch seen, and its count starts at zero in every call (a stale one would list records twice or drop
    them) -- then a second engine in the same process, and the first one again"""
    rng = np.random.default_rng(64_50_000)
    eng = rustybam_amd.Engine(0)
    eng2 = None
    try:
        listed = []
        for n_rec in (64, 50_000, 64):
            b = su.random_short_batch(rng, n_rec)
            su.check_scan(eng, oracle, b, f"one context, {n_rec} records", "rows")
            listed.append(eng.scan_route()[1])
        assert listed[1] > 1000 and listed[1] > 10 * max(listed[0], listed[2])
        eng2 = rustybam_amd.Engine(0)
        b = su.random_short_batch(rng, 300)
        su.check_scan(eng2, oracle, b, "second engine", "rows")
        assert eng.scan_route() == (64 - listed[2], listed[2])     # (the first context still answers for its own last call)
        su.check_scan(eng, oracle, su.random_short_batch(rng, 2000), "first engine again", "rows")
    finally:
        eng.close()
        if eng2 is not None:
            eng2.close()


def test_one_pointer_calls_and_null_strand(engine, gen):
    """rb_dev_scan_records with the reduce pointer alone, the norm pointer alone and a null `strand` (= all '+'), on a row-form batch:
    the rows of the two-pointer call, and the buffer that was not passed stays untouched"""
    import torch
    from devutil import DevBatch
    b = su.concat([gen["magnitude"], gen["fate"]])               # (sums of every size, stripped ends, and records the row form lists)
    b["strand"] = np.full(len(b["strand"]), ord("+"), np.uint8)
    dev = torch.device("cuda:0")
    db = DevBatch(torch, engine, dev, b)
    n = db.n_rec
    no_strand = engine.batch_view(n, db.n_ops, db.d_ops.data_ptr(), db.d_off.data_ptr(), *[x.data_ptr() for x in db.d_c], 0, db.d_contig.data_ptr())

    def run(view, want_red, want_norm):
        d_red = torch.full((n * 72,), 0xEE, dtype=torch.uint8, device=dev)
        d_norm = torch.full((n * 64,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        engine.dev_scan_records(view, d_red.data_ptr() if want_red else 0, d_norm.data_ptr() if want_norm else 0)
        route = engine.scan_route()                                # (waits for the context's stream)
        assert route == su.route(b["op_off"]) and route[0] > 0 and route[1] > 0
        torch.cuda.synchronize()
        return d_red.cpu().numpy(), d_norm.cpu().numpy()
    red, norm = run(db.view, True, True)
    assert (red.view(rustybam_amd.REDUCE_DT)["status"] < 23).all() and (norm.view(rustybam_amd.NORM_DT)["status"] < 23).all()   # (rows were written)
    r1, n1 = run(db.view, True, False)
    assert np.array_equal(r1, red) and (n1 == 0xEE).all()
    r2, n2 = run(db.view, False, True)
    assert np.array_equal(n2, norm) and (r2 == 0xEE).all()
    r3, n3 = run(no_strand, True, True)
    assert np.array_equal(r3, red) and np.array_equal(n3, norm)

