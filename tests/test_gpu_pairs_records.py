"""rb_dev_pairs_records (k_pairs.hip) against its numpy model (tests/pairs_rec_util.py), byte for byte: kept, the two coordinate columns,
key_flip, key_order, info.  tests/test_pairs_rec_inputs.py proves on the CPU what the inputs hold, that the model says what the oracle's
`orient`, `orient --scaffold` and `filter` say, and that the library's host mirror agrees with it.

Memory: every output lies in a buffer that goes on behind the capacity the call is told, filled with a sentinel; so does the scratch."""
from types import SimpleNamespace

import numpy as np
import pytest

import pairs_rec_util as pr
import rustybam_amd

pytestmark = pytest.mark.gpu
SENT = 0xEE
TAIL = 64  # elements of sentinel behind every capacity
DTYPES = (np.uint64, np.uint64, np.uint64, np.uint64, np.uint8, np.uint32, np.uint64)  # of pr.columns


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


class Resident:
    """a case's columns in HBM"""

    def __init__(self, ctx, c):
        torch, eng, dev = ctx
        self.c = c
        self.d = [torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, dt), dtype=dt).view(np.uint8)).to(dev) for a, dt in zip(pr.columns(c), DTYPES)]

    def ptrs(self):
        return [d.data_ptr() for d in self.d]

    def unchanged(self):
        return all(len(a) == 0 or d.cpu().numpy().tobytes() == np.ascontiguousarray(a, dtype=dt).tobytes() for d, a, dt in zip(self.d, pr.columns(self.c), DTYPES))


def call(ctx, R, kept_cap, mode=None, dirty=SENT, columns=True, order=True, ptrs=None, n_rec=None, scratch_off=0):
    """ONE rb_dev_pairs_records call that is told kept_cap, on buffers TAIL elements longer and full of 0xEE (the scratch: full of `dirty`)
    -> rc, the outputs as the call left them, and `tails`: nothing at or behind a capacity, the info block or the scratch was written"""
    torch, eng, dev = ctx
    c = R.c
    n = len(c.t_st) if n_rec is None else n_rec
    full = lambda k: torch.full((k,), SENT, dtype=torch.uint8, device=dev)  # noqa: E731
    d_kept, d_qs, d_qe = full((kept_cap + TAIL) * 4), full((n + TAIL) * 8), full((n + TAIL) * 8)
    d_flip, d_ord, d_info = full(c.n_keys + TAIL), full((c.n_keys + TAIL) * 8), full(64 + 256)
    scr_bytes = eng.pairs_records_scratch_bytes(c.n_keys, n)
    d_scr = torch.full((scr_bytes + 4096,), dirty, dtype=torch.uint8, device=dev)
    d_scr[scr_bytes:] = SENT
    torch.cuda.synchronize()
    rc = eng.dev_pairs_records(*(R.ptrs() if ptrs is None else ptrs), n, c.n_keys, c.mode if mode is None else mode, c.L, c.A, c.Q,
                               d_kept.data_ptr() if kept_cap else 0, kept_cap, d_qs.data_ptr() if columns else 0, d_qe.data_ptr() if columns else 0,
                               d_flip.data_ptr(), d_ord.data_ptr() if order else 0, d_info.data_ptr(), d_scr.data_ptr() + scratch_off)
    torch.cuda.synchronize()
    kept, qs, qe, flip, ord_, info = (d.cpu().numpy() for d in (d_kept, d_qs, d_qe, d_flip, d_ord, d_info))
    tails = dict(kept=bool((kept[kept_cap * 4:] == SENT).all()), q_st=bool((qs[n * 8:] == SENT).all()), q_en=bool((qe[n * 8:] == SENT).all()),
                 key_flip=bool((flip[c.n_keys:] == SENT).all()), key_order=bool((ord_[c.n_keys * 8:] == SENT).all()), info=bool((info[64:] == SENT).all()),
                 scratch=bool((d_scr[scr_bytes:] == SENT).all().item()))
    raw = b"".join(x.tobytes() for x in (kept, qs, qe, flip, ord_, info))
    return SimpleNamespace(rc=rc, raw=raw, raw_kept=kept, kept=kept[:kept_cap * 4].view(np.uint32), q_st=qs[:n * 8].view(np.uint64), q_en=qe[:n * 8].view(np.uint64),
                           key_flip=flip[:c.n_keys], key_order=ord_[:c.n_keys * 8].view(np.uint64), info=info[:64].view(rustybam_amd.PAIRS_INFO_DT)[0].copy(),
                           tails=tails, untouched=lambda a: bool((a == SENT).all()))


def check(r, m, what, kept_cap=None, columns=True, order=True):
    assert r.rc == 0, f"{what}: rc {r.rc}"
    assert all(r.tails.values()), f"{what}: written behind a capacity: {[k for k, v in r.tails.items() if not v]}"
    want = pr.model_info(m, kept_cap)
    print(f"{what}: info {r.info}, model {want}")
    assert r.info.tobytes() == want.tobytes(), f"{what}: info {r.info} != {want}"
    assert r.key_flip.tobytes() == m.key_flip.tobytes(), f"{what}: key_flip {r.key_flip.tolist()} != {m.key_flip.tolist()}"
    if order:
        assert r.key_order.tobytes() == m.key_order.tobytes(), f"{what}: key_order {r.key_order.tolist()[:8]} != {m.key_order.tolist()[:8]}"
    else:
        assert (r.key_order.view(np.uint8) == SENT).all(), f"{what}: key_order was NULL"
    for k in ("q_st", "q_en"):
        got = getattr(r, k)
        if columns:
            bad = np.nonzero(got != getattr(m, k))[0]
            assert len(bad) == 0, f"{what}: {k} differs first at {bad[0]}: {got[bad[0]]} != {getattr(m, k)[bad[0]]}"
        else:
            assert (got.view(np.uint8) == SENT).all()
    n = len(m.kept) if kept_cap is None else min(len(m.kept), kept_cap)
    bad = np.nonzero(r.kept[:n] != m.kept[:n])[0]
    assert len(bad) == 0, f"{what}: kept differs first at {bad[0]}: {r.kept[bad[0]]} != {m.kept[bad[0]]}"
    assert (r.raw_kept[n * 4:] == SENT).all(), f"{what}: an index was written behind kept[n_kept]"


def run_case(ctx, c, mode=None):
    R = Resident(ctx, c)
    m = pr.model(c, mode)
    r = call(ctx, R, len(m.kept), mode)
    check(r, m, c.name if mode is None else f"{c.name}, mode {mode}")
    assert R.unchanged(), f"{c.name}: the call wrote to its inputs"
    return R, m, r


@pytest.mark.parametrize("n", pr.record_counts())
def test_record_counts(ctx, n):
    run_case(ctx, pr.random_case(n, 100 + n))


def test_no_records_and_no_keys(ctx):
    """n_rec == 0 needs no columns and no kept; n_keys == 0 no key arrays -- every record then declines for its key and nothing is kept"""
    torch, eng, dev = ctx
    d_info = torch.full((64,), SENT, dtype=torch.uint8, device=dev)
    d_flip = torch.full((16,), SENT, dtype=torch.uint8, device=dev)
    d_ord = torch.full((16 * 8,), SENT, dtype=torch.uint8, device=dev)
    d_scr = torch.zeros(eng.pairs_records_scratch_bytes(3, 0), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert eng.dev_pairs_records(0, 0, 0, 0, 0, 0, 0, 0, 3, pr.ORIENT | pr.FILTER, 0, 0, 0, 0, 0, 0, 0, d_flip.data_ptr(), d_ord.data_ptr(), d_info.data_ptr(),
                                 d_scr.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (d_info.cpu().numpy() == 0).all() and d_flip.cpu().numpy().tolist() == [0] * 3 + [SENT] * 13
    assert d_ord.cpu().numpy().tolist() == [0] * 24 + [SENT] * 104
    c = pr.random_case(300, 5)
    c.n_keys = 0
    R, m, r = run_case(ctx, c)
    assert int(r.info["n_kept"]) == 0 and r.info["declined"] == pr.DECL_KEY and r.q_st.tobytes() == c.q_st.tobytes()


_layouts = pr.layout_cases()


@pytest.mark.parametrize("c", _layouts, ids=[c.name for c in _layouts])
def test_key_layouts(ctx, c):
    run_case(ctx, c)


_edges = pr.threshold_cases() + pr.wide_cases() + pr.decline_cases()


@pytest.mark.parametrize("c", _edges, ids=[c.name for c in _edges])
def test_thresholds_wide_sums_and_declines(ctx, c):
    R, m, r = run_case(ctx, c)
    if "declined" in c.expect:
        assert int(r.info["declined"]) == c.expect["declined"]
    if "kept" in c.expect:
        assert int(r.info["n_kept"]) == c.expect["kept"]
    if "key_flip" in c.expect:
        assert r.key_flip.tolist() == c.expect["key_flip"]


_modes = pr.mode_cases()


@pytest.mark.parametrize("c", _modes, ids=[c.name for c in _modes])
def test_each_mode(ctx, c):
    R, m, r = run_case(ctx, c)
    n = len(c.t_st)
    if c.mode == 0:
        assert r.kept.tolist() == list(range(n)) and not r.key_flip.any() and not r.key_order.any() and r.q_st.tobytes() == c.q_st.tobytes()
    if c.mode == pr.ORIENT:
        assert int(r.info["n_kept"]) == n and r.info["n_flipped_rows"] > 0 and r.key_order.all()
    if c.mode == pr.FILTER:
        assert r.info["n_flipped_rows"] == 0 and not r.key_flip.any() and not r.key_order.any() and 0 < r.info["n_kept"] < n


def test_optional_outputs(ctx):
    """q_st_out / q_en_out both NULL, key_order NULL: the rest comes out the same and nothing is written where they would have been"""
    c = pr.random_case(700, 41)
    R, m = Resident(ctx, c), pr.model(c)
    check(call(ctx, R, len(m.kept), columns=False), m, "no coordinate columns", columns=False)
    check(call(ctx, R, len(m.kept), order=False), m, "no key_order", order=False)


def test_refused_arguments(ctx):
    """an unknown mode bit, a misaligned pointer, one coordinate column without the other, 2^32 records: RB_E_INVALID, nothing enqueued or written"""
    torch, eng, dev = ctx
    c = pr.random_case(100, 1)
    R = Resident(ctx, c)
    p = R.ptrs()

    def refused(r):
        assert r.rc == -1 and r.untouched(np.frombuffer(r.raw, np.uint8)), "RB_E_INVALID, and no output byte was written"
    refused(call(ctx, R, 100, mode=4))
    refused(call(ctx, R, 100, mode=pr.ORIENT | 8))
    for i in (0, 3, 6):  # t_st, q_en, rec_q_len: 8-byte columns off by 4
        refused(call(ctx, R, 100, ptrs=p[:i] + [p[i] + 4] + p[i + 1:], n_rec=50))
    refused(call(ctx, R, 100, ptrs=p[:5] + [p[5] + 2] + p[6:], n_rec=50))  # rec_key off by 2
    refused(call(ctx, R, 100, scratch_off=8))
    torch.cuda.synchronize()
    full = torch.full((4096,), SENT, dtype=torch.uint8, device=dev)
    for n_rec in (1 << 32, 1 << 40):  # (told, not allocated: the call must refuse before it looks at anything)
        assert eng.dev_pairs_records(*p, n_rec, c.n_keys, c.mode, 0, 0, 0, 0, 0, 0, 0, full.data_ptr(), 0, full.data_ptr(), full.data_ptr()) == -1
    torch.cuda.synchronize()
    assert (full.cpu().numpy() == SENT).all()
    rc = eng.dev_pairs_records(*p, 100, c.n_keys, c.mode, 0, 0, 0, 0, 0, full.data_ptr(), 0, full.data_ptr(), 0, full.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and (full.cpu().numpy() == SENT).all(), "q_st_out without q_en_out"
    assert eng.dev_pairs_records(*p, 100, c.n_keys, c.mode, 0, 0, 0, 0, 5, 0, 0, full.data_ptr(), 0, full.data_ptr(), full.data_ptr()) == -1, "kept_cap without kept"
    check(call(ctx, R, 100), pr.model(c), "the context still works")


@pytest.mark.parametrize("n", [700, 2500])
def test_capacity(ctx, n):
    """kept_cap of n_kept - 1, 1 and 0 (kept == NULL): RB_OK, overflow, n_kept exact, nothing behind kept[kept_cap]; then exactly n_kept fits"""
    c = pr.random_case(n, 31)
    R, m = Resident(ctx, c), pr.model(c)
    n_kept = len(m.kept)
    assert n_kept > 100
    for cap in (n_kept - 1, 1, 0):
        r = call(ctx, R, cap)
        check(r, m, f"kept_cap {cap}", cap)
        assert r.info["overflow"] != 0 and int(r.info["n_kept"]) == n_kept
        check(call(ctx, R, int(r.info["n_kept"])), m, "the retry with the reported count")
    check(call(ctx, R, n_kept + 10), m, "kept_cap n_kept + 10")
    assert R.unchanged()


def test_repeatability(ctx):
    """two calls write the same bytes; a scratch full of ones or of 0xEE gives what a zeroed scratch gives"""
    c = pr.random_case(4000, 17, n_keys=3)
    R, m = Resident(ctx, c), pr.model(c)
    first = call(ctx, R, len(m.kept), dirty=0)
    check(first, m, "fresh scratch")
    for dirty in (0, 0xFF, SENT):
        assert call(ctx, R, len(m.kept), dirty=dirty).raw == first.raw


def test_host_array_form(ctx):
    torch, eng, dev = ctx
    c = pr.random_case(1000, 3)
    m = pr.model(c)
    got = eng.pairs_records(*pr.columns(c), c.n_keys, c.mode, c.L, c.A, c.Q)
    for k in ("kept", "q_st", "q_en", "key_flip", "key_order", "info"):
        assert got[k].tobytes() == getattr(m, k).tobytes(), k


def test_rows_call_still_agrees(ctx):
    """the run-summing loop is shared with rb_dev_pairs_rows: one hit row per record with the record's coordinates gives the same keys flipped and the
    same records kept (tests/test_gpu_pairs_rows.py holds that call to its own model)"""
    torch, eng, dev = ctx
    c = pr.laid_runs_case()
    m = pr.model(c)
    rows = np.zeros(len(c.t_st), rustybam_amd.HIT_DT)
    rows["rec"] = np.arange(len(rows))
    for k in ("t_st", "t_en", "q_st", "q_en"):
        rows[k] = getattr(c, k)
    rows_out, key_flip, info = eng.pairs_rows(rows, c.rec_key, c.rec_q_len, c.strand, c.n_keys, c.mode, c.L, c.A, c.Q)
    assert key_flip.tobytes() == m.key_flip.tobytes() and rows_out["rec"].tolist() == m.kept.tolist() and info.tobytes() == m.info.tobytes()
    assert rows_out["q_st"].tobytes() == m.q_st[m.kept].tobytes()
