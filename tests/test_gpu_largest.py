"""liftover --largest on the device: rb_dev_largest against the plain reference of tests/largest_util.py (held to the oracle CLI by
tests/test_largest_inputs.py, which also counts the cases the fabricated rows hold), and the `rb` front end's text route against the
oracle CLI, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import largest_util as lu
import rustybam_amd
from devutil import DevBatch
from golden.make_digests import tile_bed
from rbtest_util import batch_args, random_batch, random_windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
ROUTE = b"liftover --largest (text to text)"


def check(engine, s, what):
    want_sel, want_bad = lu.largest_ref(s["rows"], s["win_key"], s["rec_key"], s["n_keys"])
    sel, n_bad = engine.largest(s["rows"], s["win_key"], s["rec_key"], s["n_keys"])
    assert sel.dtype == np.uint64 and len(sel) == len(want_sel), (what, len(sel), len(want_sel))
    assert np.array_equal(sel, want_sel), (what, np.nonzero(sel != want_sel)[0][:5])
    assert n_bad == want_bad, what
    return sel


# ---------------------------------------------------------------------------------------------- the ABI on fabricated rows
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_one_key_equal_spans_the_last_row_wins(engine, n):
    sel = check(engine, lu.one_key(n), f"one key, {n} rows")
    assert sel.tolist() == ([n - 1] if n else [])


def test_one_key_contended(engine):
    check(engine, lu.contended(), "20,000 rows on one key")


def test_many_keys_few_rows(engine):
    s = lu.sparse()
    sel = check(engine, s, "70,001 keys")
    k = lu.row_keys(s["rows"], s["win_key"], s["rec_key"])[sel.astype(np.int64)]
    assert (np.diff(k) > 0).all()  # ascending key order, one row per key


def test_no_keys(engine):
    s = lu.one_key(65)
    s["n_keys"] = 0
    sel, n_bad = engine.largest(s["rows"], s["win_key"], s["rec_key"], 0)
    assert len(sel) == 0 and n_bad == 65  # every OK row has a key outside an empty key space


def test_property_set(engine):
    s = lu.properties()
    assert check(engine, s, "properties").tolist() == [4, 8, 0, 14, 17, 20]
    s["rec_key"] = None  # NULL: an INSIDE row is a bad key
    check(engine, s, "properties without rec_key")


@pytest.mark.parametrize("seed", [11, 12])
def test_random_skewed(engine, seed):
    check(engine, lu.skewed(seed), f"skewed {seed}")


class Dev:
    """a row set in device memory (torch tensors), with outputs and scratch sized for it or for `like`"""

    def __init__(self, torch, eng, s, n_keys_cap=None):
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        self.torch, self.eng, self.s = torch, eng, s
        self.rows, self.wk, self.rk = up(s["rows"]), up(s["win_key"].astype(np.uint32)), up(s["rec_key"].astype(np.uint32))
        cap = n_keys_cap or s["n_keys"]
        self.sel = torch.full((cap * 8 + 8,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = torch.full((16,), 0xEE, dtype=torch.uint8, device=dev)
        self.scr = torch.full((eng.largest_scratch_bytes(cap),), 0xEE, dtype=torch.uint8, device=dev)  # (the call zeroes it itself)

    def run(self, sel=None, out=None, scr=None):
        sel, out, scr = sel if sel is not None else self.sel, out if out is not None else self.out, scr if scr is not None else self.scr
        s = self.s
        self.torch.cuda.synchronize()
        self.eng.dev_largest(self.rows.data_ptr(), len(s["rows"]), self.wk.data_ptr(), self.rk.data_ptr(), s["n_keys"], sel.data_ptr(), out.data_ptr(),
                             scr.data_ptr())
        self.eng.sync()
        o = out.cpu().numpy().view(np.uint64)
        return sel.cpu().numpy().view(np.uint64)[:int(o[0])].copy(), int(o[1]), sel.cpu().numpy().tobytes() + out.cpu().numpy().tobytes()


def test_stale_scratch_and_determinism(engine):
    import torch
    a, b = lu.skewed(21, n=30_000), lu.skewed(22, n=9_000, n_keys=300)
    A, B = Dev(torch, engine, a), Dev(torch, engine, b, n_keys_cap=a["n_keys"])
    for s, (sel, n_bad, _) in ((a, A.run()), (b, B.run(A.sel, A.out, A.scr)), (a, A.run())):  # one scratch, one sel, three calls
        want_sel, want_bad = lu.largest_ref(s["rows"], s["win_key"], s["rec_key"], s["n_keys"])
        assert np.array_equal(sel, want_sel) and n_bad == want_bad
    assert A.run()[2] == A.run()[2]  # the same call twice: the same bytes, sel's unused tail included


def test_rows_of_liftover_as_they_lie_on_the_device(oracle):
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    try:
        rng = np.random.default_rng(4242)
        b = random_batch(rng, 300, "mixed", n_contig=2)
        w = random_windows(rng, b, 40, True)
        ids = [f"id{int(i)}" for i in rng.integers(0, 12, 40)]  # 40 windows, at most 12 ids
        win_key, inside_key, n_keys = lu.intern_ids(ids)
        assert n_keys < 14 and len(set(ids)) < 40
        rec_key = np.full(300, inside_key, np.uint32)
        orows, _ = oracle.liftover(oracle.Batch(*batch_args(b), b["contig"]), *w)
        want_sel, want_bad = lu.largest_ref(orows, win_key, rec_key, n_keys)
        assert len(want_sel) > 5 and want_bad == 0
        # (mixed: some records make the reference panic; the stand-alone scan drops them before the hit count, as the oracle does)
        D = DevBatch(torch, eng, dev, b)
        rows, out, cnt = D.run(w, policy=rustybam_amd.BSEARCH_MODERN)
        assert rows.shape[0] == len(orows)
        up = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)  # noqa: E731
        d_wk, d_rk = up(win_key), up(rec_key)
        d_sel = torch.zeros(n_keys, dtype=torch.int64, device=dev)
        d_out = torch.zeros(2, dtype=torch.int64, device=dev)
        d_scr = torch.empty(eng.largest_scratch_bytes(n_keys), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.dev_largest(rows.data_ptr(), rows.shape[0], d_wk.data_ptr(), d_rk.data_ptr(), n_keys, d_sel.data_ptr(), d_out.data_ptr(), d_scr.data_ptr())
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        assert (int(o[0]), int(o[1])) == (len(want_sel), 0)
        assert np.array_equal(d_sel.cpu().numpy()[:int(o[0])].view(np.uint64), want_sel)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- the front end
def rb_run(*args, env=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    return subprocess.run([RB, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def beds(tmp_path_factory):
    d = tmp_path_factory.mktemp("largest")
    tiles, rep = str(d / "tiles.bed"), str(d / "rep.bed")
    tile_bed(tiles)
    lu.repeated_id_bed(rep)
    return {"tiles": tiles, "repeated_ids": rep}


@pytest.mark.parametrize("bed_kind", ["tiles", "repeated_ids"])
def test_cli_text_route_equals_the_oracle(oracle, golden, beds, bed_kind):
    a = ["liftover", "--largest", "--bed", beds[bed_kind], f"{golden}/asm_small.paf"]
    orc, want = oracle.cli(*a)
    assert orc == 0 and want.count(b"\n") > 4
    r = rb_run(*a, env={"RB_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == want
    assert ROUTE in r.stderr, r.stderr[-2000:]  # the records were selected on the device
    g = rb_run(*a, env={"RB_TIMING": "1", "RB_GENERAL_PATH": "1"})
    assert g.returncode == 0 and g.stdout == want and ROUTE not in g.stderr


def test_cli_legacy_policy(oracle, golden, beds):
    a = ["--bsearch", "legacy", "liftover", "--largest", "--bed", beds["tiles"], f"{golden}/asm_small.paf"]
    orc, want = oracle.cli(*a)
    r = rb_run(*a, env={"RB_TIMING": "1"})
    assert (orc, r.returncode) == (0, 0) and r.stdout == want and ROUTE in r.stderr


def test_cli_declines_a_stripped_record_inside_a_window(oracle, tmp_path):
    paf, bed = tmp_path / "s.paf", tmp_path / "s.bed"
    paf.write_text("q1\t100\t0\t12\t+\tchrT\t1000\t100\t110\t10\t12\t60\tcg:Z:2I10=\n"       # leading 2I: stripped, its id becomes _TO.2I.
                   "q2\t100\t0\t50\t+\tchrT\t1000\t180\t230\t50\t50\t60\tcg:Z:50=\n"          # cut by both windows
                   "q3\t100\t0\t30\t+\tchrT\t1000\t300\t330\t29\t30\t60\tcg:Z:20=1X9=\n")     # inside the second window, not stripped
    bed.write_text("chrT\t50\t200\tidA\nchrT\t190\t400\tidB\n")
    a = ["liftover", "--largest", "--bed", bed, paf]
    orc, want = oracle.cli(*a)
    assert orc == 0 and b"id:Z:_TO.2I." in want and want.count(b"\n") == 4  # ids "", _TO.2I., idA, idB
    r = rb_run(*a, env={"RB_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == want
    assert ROUTE not in r.stderr  # declined: the record route printed it
