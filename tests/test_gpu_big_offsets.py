"""Byte offsets at and behind 2^32: rb_dev_parse_cigars, rb_dev_parse_md and rb_dev_bam_records reading their input there,
rb_dev_format_cigars and rb_dev_nucfreq_text printing more than 4 GiB in one call, and one rb_dev_upload / rb_dev_download of more than
4 GiB.  Cases and models are tests/big_offset_util.py's (tests/test_big_offset_inputs.py proves on the CPU that every case holds what it
claims); everything is compared bit for bit with the plain-Python models of the unplaced, small inputs -- never with another kernel call.

One buffer of 2^32 + 16 MiB bytes from torch spans offset 0 to beyond 2^32: an offset that lost its high half still lands inside the
allocation, on a decoy, and gives a wrong answer -- not a fault.

Mutants that these tests catch with wrong answers and no fault (one offset cut to 32 bits each): R in rb_k_bam_peek -- 33 of the 34
bam_records cases; the load address la in rb_md_walk -- 7 of the 8 parse_md cases; out in rb_k_nft -- the nucfreq text and capacity cases.
On one MI355X every test here takes less than a second."""
import ctypes as C

import numpy as np
import pytest

import rustybam_amd
import bam_rec_util as B
import big_offset_util as G
import nftext_util as nu
import sam_util as U
import text_seam_util as tu

pytestmark = pytest.mark.gpu
B32, MIB = G.B32, G.MIB
GUARD = 8
SLICE = 64 * MIB
A5 = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
p = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


@pytest.fixture(scope="module")
def shapes():
    return dict(md=rustybam_amd.md_shape(), bam=rustybam_amd.bam_shape())


@pytest.fixture(scope="module")
def big(ctx):
    """the buffer: [0] is the tensor.  Freed when the module is done"""
    torch, eng, dev = ctx
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 6 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free: the buffer of 2^32 + 16 MiB bytes wants 6 GiB")
    holder = [torch.empty(G.BUF_BYTES, dtype=torch.uint8, device=dev)]
    assert holder[0].data_ptr() % 16 == 0
    yield holder
    torch.cuda.synchronize()
    del holder[0]
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ helpers
def _dev(ctx, a):
    torch, _, dev = ctx
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a.copy()).to(dev)


def _a5(ctx, n, dt):
    """n entries of dt, every byte 0xA5, on the device (as bytes)"""
    torch, _, dev = ctx
    return torch.full((max(n, 1) * np.dtype(dt).itemsize,), 0xA5, dtype=torch.uint8, device=dev)


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _put(ctx, buf, at, data):
    torch = ctx[0]
    if len(data):
        buf[at:at + len(data)].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))


def place(ctx, big, pl):
    """0xEE everywhere, the decoy at K - 2^32 where there is room for one, the payload at K"""
    buf = big[0]
    buf.fill_(G.FILL)
    if pl.K >= B32:
        _put(ctx, buf, pl.K - B32, pl.p.decoy().data)
    _put(ctx, buf, pl.K, pl.p.data)
    return buf


def _sentinels(arr, n, what):
    assert (arr[n:].view(f"u{arr.itemsize}") == A5[arr.itemsize]).all(), f"{what}: written behind its {n} entries"


# ------------------------------------------------------------------------------------------------ 1. inputs behind 2^32
def _parse_once(ctx, buf, d_off, d_end, n, cap):
    torch, eng, dev = ctx
    d_ops, d_opoff, d_st = _a5(ctx, cap + GUARD, np.uint32), _a5(ctx, n + 1 + GUARD, np.uint64), _a5(ctx, n + GUARD, np.uint8)
    d_scr = torch.zeros(eng.text_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = eng.L.rb_dev_parse_cigars(eng.ctx, p(buf.data_ptr()), p(d_off.data_ptr()), p(d_end.data_ptr()), C.c_uint64(n), p(d_opoff.data_ptr()),
                                   p(d_ops.data_ptr()), C.c_uint64(cap + GUARD), p(d_st.data_ptr()), p(d_scr.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0
    return _host(d_opoff, np.uint64), _host(d_ops, np.uint32), _host(d_st, np.uint8)


@pytest.mark.parametrize("pid", G.IDS["parse"])
def test_parse_cigars_reads_behind_2_to_the_32(ctx, shapes, big, pid):
    """the seam layouts of test_gpu_text_seams.py (text_off + text_end, PAF bytes between the strings) with 2^32 inside a string of one
    step, inside a middle step of a long one, on a first byte, behind the last byte, in front of the whole layout and in its middle:
    status in the reference's set, the count exact, the ops the reference's, op_off exact; a second call writes the same bytes"""
    pl = G.placement("parse", pid, shapes)
    pay, K, n = pl.p, pl.K, pl.p.n
    buf = place(ctx, big, pl)
    d_off, d_end = _dev(ctx, pay.off + np.uint64(K)), _dev(ctx, pay.end + np.uint64(K))
    got = _parse_once(ctx, buf, d_off, d_end, n, len(pay.data) // 2)
    again = _parse_once(ctx, buf, d_off, d_end, n, len(pay.data) // 2)
    for x, y in zip(got, again):
        assert x.tobytes() == y.tobytes()
    op_off, ops, status = got
    want = G.model(pay, K)
    _sentinels(op_off, n + 1, "op_off"), _sentinels(status, n, "status")
    assert int(op_off[0]) == 0 and (np.diff(op_off[:n + 1].astype(np.int64)) >= 0).all()
    total = int(op_off[n])
    _sentinels(ops, total, "ops")
    for i, (ref, allowed) in enumerate(zip(want["refs"], want["allowed"])):
        st, a, b = int(status[i]), int(op_off[i]), int(op_off[i + 1])
        assert st in allowed, (pid, pay.labels[i], st, sorted(allowed))
        if ref is not None and max(ln for ln, _ in ref + [(0, 0)]) < 1 << tu.LEN_BITS:
            assert b - a == len(ref), (pid, pay.labels[i])
        if st == 0:
            assert np.array_equal(ops[a:b], tu.ref_words(ref)), (pid, pay.labels[i])


@pytest.mark.parametrize("pid", G.IDS["md"])
def test_parse_md_reads_behind_2_to_the_32(ctx, shapes, big, pid):
    """every MD seam case of sam_util.md_cases with 2^32 inside a string of the row form, inside a middle step of the wavefront form, on
    a first byte, behind the last byte, in front of all strings and in their middle: the four counts and the status of md_model"""
    torch, eng, dev = ctx
    pl = G.placement("md", pid, shapes)
    pay, K, n = pl.p, pl.K, pl.p.n
    buf = place(ctx, big, pl)
    d_off, d_end = _dev(ctx, pay.off + np.uint64(K)), _dev(ctx, pay.end + np.uint64(K))
    want = G.model(pay, K)
    runs = []
    for _ in range(2):
        d_out, d_st = _a5(ctx, 4 * (n + GUARD), np.uint32), _a5(ctx, n + GUARD, np.uint8)
        torch.cuda.synchronize()
        eng.dev_parse_md(buf.data_ptr(), d_off.data_ptr(), d_end.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        runs.append((_host(d_out, np.uint32).reshape(-1, 4), _host(d_st, np.uint8)))
    out, status = runs[0]
    assert out.tobytes() == runs[1][0].tobytes() and status.tobytes() == runs[1][1].tobytes()
    bad = [pay.labels[i] for i in range(n) if (tuple(int(x) for x in out[i]), int(status[i])) != want[i]]
    assert not bad, f"{pid}: {len(bad)} strings differ, first {bad[:8]}; e.g. got {out[pay.labels.index(bad[0])]}, want {want[pay.labels.index(bad[0])]}"
    assert (out[n:] == 0xA5A5A5A5).all() and (status[n:] == 0xA5).all(), "written behind the n results"


BAM_NAMES = ("tid", "pos", "flag", "l_seq", "has_md", "md_off", "md_end", "op_off", "ops", "status")
BAM_DT = dict(tid=np.int32, pos=np.int64, flag=np.uint32, l_seq=np.uint32, has_md=np.uint8, md_off=np.uint64, md_end=np.uint64, op_off=np.uint64,
              ops=np.uint32, status=np.uint8)


def _bam_once(ctx, buf, d_off, d_len, n, cap):
    """-> (dict of host arrays with their 0xA5 guards, dict of the device tensors)"""
    torch, eng, dev = ctx
    d = {k: _a5(ctx, (cap if k == "ops" else n + (k == "op_off")) + GUARD, BAM_DT[k]) for k in BAM_NAMES}
    d_scr = torch.zeros(max(eng.bam_scratch_bytes(n), 256), dtype=torch.uint8, device=dev)
    assert d["ops"].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    eng.dev_bam_records(buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, *[d[k].data_ptr() for k in BAM_NAMES[:9]], cap, d["status"].data_ptr(),
                        d_scr.data_ptr())
    torch.cuda.synchronize()
    return {k: _host(d[k], BAM_DT[k]) for k in BAM_NAMES}, d


def _bam_check(got, want, labels, cap):
    """tests/test_gpu_bam_records.py's check: every column and op_off equal, 0xA5 behind every array and behind ops[total]"""
    n = len(labels)
    for k in B.COLS + ("op_off",):
        m = n + (k == "op_off")
        bad = np.nonzero(got[k][:m] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} records differ, first {[(labels[min(i, n - 1)], int(got[k][i]), int(want[k][i])) for i in bad[:4]]}"
        _sentinels(got[k], m, k)
    total = int(want["op_off"][n])
    assert total <= cap
    bad = np.nonzero(got["ops"][:total] != want["ops"][:total])[0]
    if len(bad):
        r = int(np.searchsorted(want["op_off"], bad[0], side="right")) - 1
        raise AssertionError(f"ops: {len(bad)} words differ, first at {bad[0]} = word {int(bad[0] - want['op_off'][r])} of {labels[r]}: "
                             f"{got['ops'][bad[0]]:#x} for {want['ops'][bad[0]]:#x}")
    _sentinels(got["ops"], total, "ops")


@pytest.mark.parametrize("pid", G.IDS["bam"])
def test_bam_records_reads_behind_2_to_the_32(ctx, shapes, big, pid):
    """the case groups of test_gpu_bam_records.py and its mixed deal with 2^32 inside the 32 fixed bytes, inside an aux head, inside a Z
    value under search, inside a CIGAR of the row form, inside a middle step of a long aux area and of the 70000-op CG tag, on a record's
    first byte, behind the last record, in front of the whole stream and in its middle: every column, op_off and ops of the model, md_off
    and md_end moved by K"""
    pl = G.placement("bam", pid, shapes)
    pay, K, n = pl.p, pl.K, pl.p.n
    buf = place(ctx, big, pl)
    d_off, d_len = _dev(ctx, pay.off + np.uint64(K)), _dev(ctx, pay.rec_len)
    cap = len(pay.data) // 4
    want = G.model(pay, K)
    got, _ = _bam_once(ctx, buf, d_off, d_len, n, cap)
    _bam_check(got, want, pay.labels, cap)
    again, _ = _bam_once(ctx, buf, d_off, d_len, n, cap)
    for k in BAM_NAMES:
        assert again[k].tobytes() == got[k].tobytes(), k
    if pl.cls in "abd":
        assert int(want["status"][pl.item]) == B.BAM_OK


def test_bam_columns_across_2_to_the_32_to_rows_equal_the_span_model(ctx, big):
    """the composition of test_gpu_bam_records.py at K = 2^32 - P // 2: the columns as they lie on the device go into
    rb_dev_scan_records, rb_dev_parse_md (text = the buffer) and rb_dev_aln_stats"""
    torch, eng, dev = ctx
    pay = G.composition_payload()
    n, P = pay.n, len(pay.data)
    K = B32 - P // 2
    assert (pay.end + np.uint64(K) <= B32).sum() >= 30 and (pay.off + np.uint64(K) >= B32).sum() > 100   # (and one large record across)
    buf = big[0]
    buf.fill_(G.FILL)
    _put(ctx, buf, K, pay.data)
    want = G.model(pay, K)
    as_read = B.records_of(pay.data, pay.off, pay.rec_len, G.model(pay, 0), pay.refs)
    cap = P // 4
    got, d = _bam_once(ctx, buf, _dev(ctx, pay.off + np.uint64(K)), _dev(ctx, pay.rec_len), n, cap)
    _bam_check(got, want, pay.labels, cap)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    strand = torch.full((n,), ord("+"), dtype=torch.uint8, device=dev)
    red = torch.zeros(n * rustybam_amd.REDUCE_DT.itemsize, dtype=torch.uint8, device=dev)
    d_md, d_mst, d_rows = _a5(ctx, 4 * (n + GUARD), np.uint32), _a5(ctx, n + GUARD, np.uint8), _a5(ctx, (n + GUARD) * 80, np.uint8)
    view = eng.batch_view(n, int(want["op_off"][-1]), d["ops"].data_ptr(), d["op_off"].data_ptr(), zero.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                          zero.data_ptr(), strand.data_ptr(), 0)
    torch.cuda.synchronize()
    eng.dev_scan_records(view, red.data_ptr(), 0)
    eng.dev_parse_md(buf.data_ptr(), d["md_off"].data_ptr(), d["md_end"].data_ptr(), n, d_md.data_ptr(), d_mst.data_ptr())
    eng.dev_aln_stats(view, red.data_ptr(), d["pos"].data_ptr(), d["flag"].data_ptr(), d["l_seq"].data_ptr(), d_md.data_ptr(), d_mst.data_ptr(),
                      d["has_md"].data_ptr(), d_rows.data_ptr())
    torch.cuda.synchronize()
    rows, md4, mst = _host(d_rows, rustybam_amd.ALN_DT), _host(d_md, np.uint32).reshape(-1, 4), _host(d_mst, np.uint8)
    assert (rows[n:].view(np.uint8) == 0xA5).all() and (md4[n:] == 0xA5A5A5A5).all() and (mst[n:] == 0xA5).all()
    bad = [r["name"] for r, g in zip(as_read, rows) if not r["flag"] & 4 and g.tobytes() != U.span_model(r).tobytes()]
    assert not bad, f"{len(bad)} rows differ from the span model, first {bad[:6]}"
    for r, g4, gs in zip(as_read, md4, mst):
        if not r["flag"] & 4 and r["md"] is not None:
            assert (tuple(int(x) for x in g4), int(gs)) == U.md_model(r["md"]), r["name"]
    assert sum(1 for r, g in zip(as_read, rows) if not r["flag"] & 4 and g["status"] == 0) > 400


# ------------------------------------------------------------------------------------------------ 2. outputs behind 2^32
def _text_is(ctx, buf, o, lo, hi, or_untouched=False):
    """bytes [lo, hi) of the buffer against the case's text, ON THE DEVICE in slices of whole periods of at most 64 MiB (the period is
    uploaded once); or_untouched: a byte may also still be 0xEE"""
    torch, eng, dev = ctx
    if hi <= lo:
        return True
    P = len(o.period)
    d_period = torch.from_numpy(np.frombuffer(o.period, np.uint8).copy()).to(dev)
    ok = torch.ones((), dtype=torch.bool, device=dev)

    def eq(got, want):
        e = got == want
        return (e | (got == G.FILL)).all() if or_untouched else e.all()
    body = min(hi, o.reps * P)
    a = lo
    if a % P and a < body:                                               # up to the next period start
        b = min(body, a - a % P + P)
        ok &= eq(buf[a:b], d_period[a % P:a % P + (b - a)])
        a = b
    per = max(1, SLICE // P)
    while a + P <= body:
        k = min(per, (body - a) // P)
        ok &= eq(buf[a:a + k * P].view(k, P), d_period)
        a += k * P
    if a < hi:                                                           # the last, partial period and the tail
        assert hi - a <= SLICE
        ok &= eq(buf[a:hi], torch.from_numpy(np.frombuffer(o.text(a, hi), np.uint8).copy()).to(dev))
    return bool(ok.item())


def _untouched(buf, a, b):
    """bytes [a, b) still hold the fill (in slices: no temporary of the buffer's size)"""
    ok = True
    for g in range(a, b, 4 * SLICE):
        ok = ok and bool((buf[g:min(b, g + 4 * SLICE)] == G.FILL).all().item())
    return ok


def _windows(buf, o, total):
    """the first MiB, the two MiB around 2^32, the last MiB and the 80 bytes behind the end, on the host against the model"""
    for a, b in ((0, MIB), (B32 - MIB, min(B32 + MIB, total)), (total - MIB, total)):
        got, want = buf[a:b].cpu().numpy().tobytes(), o.text(a, b)
        if got != want:
            k = next(i for i in range(b - a) if got[i] != want[i])
            raise AssertionError(f"text differs at byte {a + k} = 2^32 {a + k - B32:+d}: got {got[max(0, k - 40):k + 40]!r}, want {want[max(0, k - 40):k + 40]!r}")
    assert buf[total:total + 80].cpu().numpy().tobytes() == bytes([G.FILL]) * 80, "bytes behind the text were written"


def _capacity(ctx, buf, o, off, cap):
    """the truncation contract on a buffer that held 0xEE: nothing at or behind text[cap]; every item that ends at or in front of the last
    16-byte boundary <= cap whole; below the cap a byte is untouched or the right one"""
    total = o.total()
    assert cap < total
    assert _untouched(buf, cap, G.BUF_BYTES), f"a byte at or behind text[{cap}] was written"
    ends = off[1:]
    whole_end = int(ends[ends <= np.uint64(cap & ~15)].max())
    assert whole_end > B32 - 16 * MIB
    assert _text_is(ctx, buf, o, 0, whole_end), "an item that ends in front of the cap is not whole"
    assert _text_is(ctx, buf, o, whole_end, cap, or_untouched=True), "a wrong byte below the cap"


def _nf_call(ctx, big, o, cap=None, text_null=False):
    torch, eng, dev = ctx
    buf = big[0]
    a = G.nf_arrays(o)
    n = len(a.seg_n)
    d_counts = _dev(ctx, np.concatenate([o.one.counts.reshape(-1), np.zeros(16, np.uint32)]))
    d_strings = _dev(ctx, np.frombuffer(a.strings, np.uint8))
    d_off, d_first, d_lines = _a5(ctx, n + 1 + GUARD, np.uint64), _a5(ctx, n + GUARD, np.uint64), _a5(ctx, n + GUARD, np.uint64)
    scr_bytes = eng.nucfreq_text_scratch_bytes(n, int(a.seg_n.astype(np.uint64).sum()))
    d_scr = torch.full((scr_bytes + 512,), 0xEE, dtype=torch.uint8, device=dev)
    scr = (d_scr.data_ptr() + 255) & ~255
    buf.fill_(G.FILL)
    torch.cuda.synchronize()
    small = o.mode == nu.SMALL
    rc = eng.dev_nucfreq_text(d_counts.data_ptr(), a.seg_cnt, a.seg_pos, a.seg_n, d_strings.data_ptr(), a.pre_off, a.pre_len, a.suf_off, a.suf_len, o.mode,
                              d_off.data_ptr(), d_first.data_ptr(), d_lines.data_ptr(), 0 if text_null else buf.data_ptr(),
                              o.total() if cap is None else cap, scr, check=False)
    torch.cuda.synchronize()
    assert rc == 0 and (small or len(a.strings) > 510)
    off, first, lines = _host(d_off, np.uint64), _host(d_first, np.uint64), _host(d_lines, np.uint64)
    want = o.text_off()
    assert np.array_equal(off[:n + 1], want), f"seg_text_off: first difference at segment {int(np.nonzero(off[:n + 1] != want)[0][0])}"
    assert np.array_equal(first[:n], a.first) and np.array_equal(lines[:n], a.lines)
    _sentinels(off, n + 1, "seg_text_off"), _sentinels(first, n, "seg_first"), _sentinels(lines, n, "seg_lines")
    assert set(bytes(d_scr.cpu().numpy()[scr - d_scr.data_ptr() + scr_bytes:])) <= {0xEE}, "bytes behind the scratch were written"
    return want


def _fmt_call(ctx, big, o, cap=None, text_null=False):
    torch, eng, dev = ctx
    buf = big[0]
    a = G.format_arrays(o)
    n = len(a.first)
    pad = np.zeros(16, np.uint32)
    d_ops, d_alt = _dev(ctx, np.concatenate([o.ops, pad])), _dev(ctx, np.concatenate([o.alt, pad]))
    d_first, d_count, d_fl, d_ll = _dev(ctx, a.first), _dev(ctx, a.count), _dev(ctx, a.fl), _dev(ctx, a.ll)
    d_toff = _a5(ctx, n + 1 + GUARD, np.uint64)
    d_scr = torch.zeros(eng.text_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev)
    buf.fill_(G.FILL)
    torch.cuda.synchronize()
    rc = eng.L.rb_dev_format_cigars(eng.ctx, p(d_ops.data_ptr()), p(d_alt.data_ptr()), C.c_uint64(n), p(d_first.data_ptr()), p(d_count.data_ptr()),
                                    p(d_fl.data_ptr()), p(d_ll.data_ptr()), p(d_toff.data_ptr()), p(0 if text_null else buf.data_ptr()),
                                    C.c_uint64(o.total() if cap is None else cap), p(d_scr.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0
    toff = _host(d_toff, np.uint64)
    want = o.text_off()
    assert np.array_equal(toff[:n + 1], want), f"text_off: first difference at item {int(np.nonzero(toff[:n + 1] != want)[0][0])}"
    _sentinels(toff, n + 1, "text_off")
    return want


OUT = {"nf-full": (G.nucfreq_full, _nf_call), "nf-small": (G.nucfreq_small, _nf_call), "format": (G.format_case, _fmt_call)}


@pytest.mark.parametrize("name", sorted(OUT))
@pytest.mark.parametrize("trimmed", [False, True], ids=["past", "ends-on-2^32"])
def test_text_of_more_than_4_gib(ctx, big, name, trimmed):
    """one call prints past 2^32 (2^32 inside a line / inside the long item), or up to byte 2^32 exactly: the offsets are the 64-bit
    cumulative sums of the model's lengths, the whole text is the model's period repeated, the bytes behind it are untouched"""
    make, call = OUT[name]
    o = make(trimmed)
    total = o.total()
    assert total == B32 if trimmed else total >= B32 + G.PAST
    call(ctx, big, o)
    buf = big[0]
    _windows(buf, o, total)
    assert _text_is(ctx, buf, o, 0, total), "the text differs from the model's somewhere outside the windows"
    assert _untouched(buf, total, G.BUF_BYTES), "bytes behind the text were written"


@pytest.mark.parametrize("name", sorted(OUT))
@pytest.mark.parametrize("cap", G.CAPS, ids=["2^32-1", "2^32", "2^32+1", "2^32+15"])
def test_text_capacity_at_2_to_the_32(ctx, big, name, cap):
    """text_cap on, next to and 15 behind 2^32: RB_OK, the offsets exact, and the truncation contract of the call"""
    make, call = OUT[name]
    o = make(False)
    off = call(ctx, big, o, cap=cap)
    _capacity(ctx, big[0], o, off, cap)


@pytest.mark.parametrize("name", sorted(OUT))
def test_text_sizes_only(ctx, big, name):
    """text == NULL: the same offsets (the scan's carry across 2^32 with no text at all), and no byte of the buffer written"""
    make, call = OUT[name]
    call(ctx, big, make(False), text_null=True)
    assert _untouched(big[0], 0, G.BUF_BYTES)


# ------------------------------------------------------------------------------------------------ 3. one transfer of more than 4 GiB
def _host_free_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def test_one_upload_and_one_download_across_2_to_the_32(ctx):
    """2^32 + 64 MiB in one rb_dev_upload through the staging ring: the patterned windows arrive where they belong (the first MiB, both
    sides of every chunk boundary near 2^32, the last 4 KiB), everything else is zero; one rb_dev_download of 64 MiB across 2^32"""
    torch, eng, dev = ctx
    if _host_free_bytes() < 12 << 30:
        pytest.skip(f"{_host_free_bytes() >> 20} MiB of host memory available: the source of 2^32 + 64 MiB bytes wants 12 GiB")
    if torch.cuda.mem_get_info(dev)[0] < G.XFER_BYTES + (1 << 30):
        pytest.skip("not enough device memory for 2^32 + 64 MiB bytes beside the module's buffer")
    src = np.zeros(G.XFER_BYTES, np.uint8)
    wins = G.xfer_windows()
    for a, b in wins:
        src[a:b] = G.xfer_pattern(a, b)
    d = torch.empty(G.XFER_BYTES, dtype=torch.uint8, device=dev)
    try:
        d.fill_(G.FILL)
        torch.cuda.synchronize()
        assert eng.L.rb_dev_upload(eng.ctx, p(d.data_ptr()), src.ctypes.data_as(p), C.c_size_t(G.XFER_BYTES)) == 0
        eng.sync()
        torch.cuda.synchronize()
        at = 0
        for a, b in wins + [(G.XFER_BYTES, G.XFER_BYTES)]:
            for g in range(at, a, 4 * SLICE):                            # between the windows: zero
                assert int(d[g:min(a, g + 4 * SLICE)].sum(dtype=torch.int64).item()) == 0, f"a byte in [{g}, {min(a, g + 4 * SLICE)}) is not zero"
            if b > a:
                small = torch.from_numpy(G.xfer_pattern(a, b)).to(dev)
                assert torch.equal(d[a:b], small), f"the window [{a}, {b}) = 2^32 {a - B32:+d} .. differs"
            at = b
        lo, hi = G.DOWN
        back = np.full(hi - lo, 0x55, np.uint8)
        assert eng.L.rb_dev_download(eng.ctx, back.ctypes.data_as(p), p(d.data_ptr() + lo), C.c_size_t(hi - lo)) == 0
        assert np.array_equal(back, src[lo:hi])
    finally:
        torch.cuda.synchronize()
        del d
        torch.cuda.empty_cache()
