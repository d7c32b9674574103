"""rb_dev_pairs_rows (k_pairs.hip) against its numpy model (tests/pairs_util.py), byte for byte: rows_out, key_flip, info.
tests/test_pairs_inputs.py proves on the CPU what the inputs hold, that the model says what the oracle's `break-paf | orient | filter` says,
and that the library's host mirror agrees with it.

Memory: every output lies in a buffer that goes on behind the capacity the call is told, filled with a sentinel; so does the scratch."""
from types import SimpleNamespace

import numpy as np
import pytest

import pairs_util as pu
import rustybam_amd
from devutil import DevBatch

pytestmark = pytest.mark.gpu
SENT = 0xEE
TAIL = 64  # elements of sentinel behind every capacity


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


class Resident:
    """a case's inputs in HBM"""

    def __init__(self, ctx, c):
        torch, eng, dev = ctx
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, dt), dtype=dt).view(np.uint8)).to(dev)  # noqa: E731
        self.c = c
        self.d_rows, self.d_key = up(c.rows, rustybam_amd.HIT_DT), up(c.rec_key, np.uint32)
        self.d_qlen, self.d_strand = up(c.rec_q_len, np.uint64), up(c.strand, np.uint8)

    def unchanged(self):
        c = self.c
        return all(len(a) == 0 or d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
                   for d, a in ((self.d_rows, c.rows), (self.d_key, c.rec_key), (self.d_qlen, c.rec_q_len), (self.d_strand, c.strand)))


def call(ctx, R, rows_cap, mode=None, rows_ptr=None, n_rows=None, dirty=SENT):
    """ONE rb_dev_pairs_rows call that is told rows_cap, on buffers TAIL elements longer and full of 0xEE (the scratch: full of `dirty`):
    -> the outputs as the call left them, and `tails`: nothing at or behind a capacity, the info block or the scratch was written"""
    torch, eng, dev = ctx
    c = R.c
    n_rows = len(c.rows) if n_rows is None else n_rows
    d_out = torch.full(((rows_cap + TAIL) * 64,), SENT, dtype=torch.uint8, device=dev)
    d_flip = torch.full((c.n_keys + TAIL,), SENT, dtype=torch.uint8, device=dev)
    d_info = torch.full((64 + 256,), SENT, dtype=torch.uint8, device=dev)
    scr_bytes = eng.pairs_scratch_bytes(c.n_keys, n_rows)
    d_scr = torch.full((scr_bytes + 4096,), dirty, dtype=torch.uint8, device=dev)
    d_scr[scr_bytes:] = SENT
    torch.cuda.synchronize()
    eng.dev_pairs_rows(R.d_rows.data_ptr() if rows_ptr is None else rows_ptr, n_rows, R.d_key.data_ptr(), R.d_qlen.data_ptr(), R.d_strand.data_ptr(),
                       len(c.rec_key), c.n_keys, c.mode if mode is None else mode, c.L, c.A, c.Q, d_out.data_ptr(), rows_cap, d_flip.data_ptr(),
                       d_info.data_ptr(), d_scr.data_ptr())
    torch.cuda.synchronize()
    out, flip, info = d_out.cpu().numpy(), d_flip.cpu().numpy(), d_info.cpu().numpy()
    tails = dict(rows_out=bool((out[rows_cap * 64:] == SENT).all()), key_flip=bool((flip[c.n_keys:] == SENT).all()), info=bool((info[64:] == SENT).all()),
                 scratch=bool((d_scr[scr_bytes:] == SENT).all().item()))
    return SimpleNamespace(raw_out=out, d_out=d_out, rows_out=out[:rows_cap * 64].view(rustybam_amd.HIT_DT), key_flip=flip[:c.n_keys],
                           info=info[:64].view(rustybam_amd.PAIRS_INFO_DT)[0].copy(), tails=tails)


def check(r, m, what, rows_cap=None):
    assert all(r.tails.values()), f"{what}: written behind a capacity: {[k for k, v in r.tails.items() if not v]}"
    want = pu.model_info(m, rows_cap)
    print(f"{what}: info {r.info}, model {want}")
    assert r.info.tobytes() == want.tobytes(), f"{what}: info {r.info} != {want}"
    assert r.key_flip.tobytes() == m.key_flip.tobytes(), f"{what}: key_flip {r.key_flip.tolist()} != {m.key_flip.tolist()}"
    if rows_cap is None:  # a call that fitted: every kept row, and nothing behind them
        n = len(m.rows_out)
        bad = np.nonzero(r.rows_out[:n] != m.rows_out)[0]
        assert len(bad) == 0, f"{what}: rows_out differs first at {bad[0]}: {r.rows_out[bad[0]]} != {m.rows_out[bad[0]]}"
        assert (r.raw_out[n * 64:] == SENT).all(), f"{what}: a row was written behind rows_out[n_kept]"


def run_case(ctx, c, mode=None):
    R = Resident(ctx, c)
    m = pu.model(c, mode)
    r = call(ctx, R, len(m.rows_out), mode)
    check(r, m, c.name if mode is None else f"{c.name}, mode {mode}")
    assert R.unchanged(), f"{c.name}: the call wrote to its inputs"
    return R, m, r


@pytest.mark.parametrize("n", pu.row_counts())
def test_row_counts(ctx, n):
    run_case(ctx, pu.random_case(n, 100 + n))


def test_no_rows_and_no_keys(ctx):
    """n_rows == 0 needs no rows and no rows_out; n_keys == 0 no key_flip -- every OK row then declines for its key and nothing is kept"""
    torch, eng, dev = ctx
    d_info = torch.full((64,), SENT, dtype=torch.uint8, device=dev)
    d_flip = torch.full((16,), SENT, dtype=torch.uint8, device=dev)
    d_scr = torch.zeros(eng.pairs_scratch_bytes(3, 0), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_pairs_rows(0, 0, 0, 0, 0, 0, 3, pu.ORIENT | pu.FILTER, 0, 0, 0, 0, 0, d_flip.data_ptr(), d_info.data_ptr(), d_scr.data_ptr())
    torch.cuda.synchronize()
    assert (d_info.cpu().numpy() == 0).all() and d_flip.cpu().numpy().tolist() == [0] * 3 + [SENT] * 13
    c = pu.random_case(300, 5)
    c.n_keys = 0
    R, m, r = run_case(ctx, c)
    assert int(r.info["n_kept"]) == 0 and r.info["declined"] == pu.DECL_KEY


_runs = pu.key_run_cases()


@pytest.mark.parametrize("c", _runs, ids=[c.name for c in _runs])
def test_key_runs(ctx, c):
    run_case(ctx, c)


_edges = pu.threshold_cases() + pu.wide_cases()


@pytest.mark.parametrize("c", _edges, ids=[c.name for c in _edges])
def test_thresholds_and_64_bit_sums(ctx, c):
    run_case(ctx, c)


_modes = pu.mode_cases()


@pytest.mark.parametrize("c", _modes, ids=[c.name for c in _modes])
def test_each_mode_bit(ctx, c):
    R, m, r = run_case(ctx, c)
    ok = int((c.rows["status"] == 0).sum())
    if c.mode == pu.ORIENT:
        assert int(r.info["n_kept"]) == ok and r.info["n_flipped_rows"] > 0
    if c.mode == pu.FILTER:
        assert r.info["n_flipped_rows"] == 0 and not r.key_flip.any() and 0 < r.info["n_kept"] < ok
    if c.mode == 0:
        assert r.rows_out[:ok].tobytes() == c.rows[c.rows["status"] == 0].tobytes()


_declines = pu.decline_cases()


@pytest.mark.parametrize("c", _declines, ids=[c.name for c in _declines])
def test_declines(ctx, c):
    R, m, r = run_case(ctx, c)
    assert int(r.info["declined"]) == c.expect["declined"]


def test_bad_arguments(ctx):
    """a misaligned rows pointer and an unknown mode bit are refused before anything is enqueued"""
    torch, eng, dev = ctx
    R = Resident(ctx, pu.random_case(100, 1))
    with pytest.raises(rustybam_amd.RbError):
        call(ctx, R, 100, rows_ptr=R.d_rows.data_ptr() + 8, n_rows=50)
    with pytest.raises(rustybam_amd.RbError):
        call(ctx, R, 100, mode=4)


@pytest.mark.parametrize("n", [700, 2500])
def test_capacity(ctx, n):
    """rows_cap of n_kept - 1, 1 and 0: RB_OK, overflow, n_kept exact, nothing behind rows_out[rows_cap]; then exactly n_kept fits"""
    c = pu.random_case(n, 31)
    R, m = Resident(ctx, c), pu.model(c)
    n_kept = len(m.rows_out)
    assert n_kept > 100
    for cap in (n_kept - 1, 1, 0):
        r = call(ctx, R, cap)
        check(r, m, f"rows_cap {cap}", cap)
        assert r.info["overflow"] != 0 and int(r.info["n_kept"]) == n_kept
        check(call(ctx, R, int(r.info["n_kept"])), m, "the retry with the reported count")
    r = call(ctx, R, n_kept + 10)  # (more room than needed: the same rows, the rest untouched)
    check(r, m, "rows_cap n_kept + 10")
    assert R.unchanged()


def test_repeatability(ctx):
    """two calls write the same bytes; a scratch full of ones or of 0xEE gives what a zeroed scratch gives"""
    c = pu.random_case(5000, 17, n_keys=3)
    R, m = Resident(ctx, c), pu.model(c)
    n = len(m.rows_out)
    first = call(ctx, R, n, dirty=0)
    check(first, m, "fresh scratch")
    for dirty in (0, 0xFF, SENT):
        r = call(ctx, R, n, dirty=dirty)
        assert r.raw_out.tobytes() == first.raw_out.tobytes() and r.key_flip.tobytes() == first.key_flip.tobytes() and r.info.tobytes() == first.info.tobytes()


def test_host_array_form(ctx):
    torch, eng, dev = ctx
    c = pu.random_case(1000, 3)
    m = pu.model(c)
    rows_out, key_flip, info = eng.pairs_rows(c.rows, c.rec_key, c.rec_q_len, c.strand, c.n_keys, c.mode, c.L, c.A, c.Q)
    assert rows_out.tobytes() == m.rows_out.tobytes() and key_flip.tobytes() == m.key_flip.tobytes() and info.tobytes() == m.info.tobytes()


@pytest.mark.parametrize("descriptors", [False, True], ids=["ops", "descriptors"])
def test_into_the_tail(ctx, descriptors):
    """the rows of rb_dev_break on asm_small.paf: rows_out fed to rb_dev_stats_rows with the same batch and out_ops gives the stats of the
    same rows picked by hand from a call on all rows -- out_off and flags came through"""
    torch, eng, dev = ctx
    b, rec_key, q_len, n_keys = pu.asm_small()
    D = DevBatch(torch, eng, dev, b)
    policy = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | (rustybam_amd.LIFT_DESCRIPTORS if descriptors else 0)
    rows, out, cnt = D.run(None, policy, max_size=100, rows_cap=4096)
    h, _ = D.host_rows(rows, out)
    assert len(h) == 2447 and (h["status"] == 0).all()
    c = pu.case("asm_small", h.copy(), rec_key, q_len, b["strand"], n_keys, L=1_000_000)
    m = pu.model(c)
    assert (int(m.info["n_kept"]), int(m.key_flip.sum())) == (1944, 5) and 0 < m.info["n_flipped_rows"] < 1944
    R = Resident(ctx, c)
    r = call(ctx, R, 1944, rows_ptr=rows.data_ptr())
    check(r, m, "the rows of break-paf --max-size 100")
    d_all = torch.zeros(len(h) * 72, dtype=torch.uint8, device=dev)
    d_kept = torch.zeros(1944 * 72, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_stats_rows(D.view, rows.data_ptr(), len(h), out.data_ptr(), d_all.data_ptr())
    eng.dev_stats_rows(D.view, r.d_out.data_ptr(), 1944, out.data_ptr(), d_kept.data_ptr())
    torch.cuda.synchronize()
    st_all = d_all.cpu().numpy().view(rustybam_amd.REDUCE_DT)
    st_kept = d_kept.cpu().numpy().view(rustybam_amd.REDUCE_DT)
    # a flipped row's q_st / q_en changed, its clip did not: every stats field is the clip's
    assert st_kept.tobytes() == st_all[m.keep].tobytes() and (st_kept["status"] == 0).all()
