"""rb_k_parse_cigars / rb_k_format_cigars (rustybam_amd/csrc/k_text.hip) at their lane, step and store seams, through rb_dev_parse_cigars
and rb_dev_format_cigars on device buffers.  Inputs, the plain-Python reference and the position model are tests/text_seam_util.py's;
tests/test_text_seam_inputs.py proves on the CPU that the reference is the oracle's on every string and item used here, that every case
lies where its name says and that every grid is complete.  Nothing here is compared with another kernel, and no record or item is left
out of a comparison.

Parse: strings at chosen offsets of one buffer (text_off + text_end) that ends at the next multiple of 16 behind the last string, with
hostile bytes between them, and the same strings back to back (text_end = NULL).  op_off, ops and status have 0xEE sentinels behind them;
a second call must write the same bytes.  Format: the WHOLE 0xEE-filled text buffer is compared with the reference's concatenation.

One-line mutants of k_text.hip and the tests that fail on them: lane 0 not taking carry_nd -- the phase grid, the splits, 2^28, full steps,
status; `tnd >= 9u` -- the phase grid, the splits, 2^28, status; fixed_first left out of mx -- 2^28, status; first_valid one byte short --
every parse test; ops_alt ignored -- two arrays, continuation words; last_len at the last word of a STEP -- the 255-word seam."""
import ctypes as C

import numpy as np
import pytest

import rustybam_amd
import text_seam_util as tu

pytestmark = pytest.mark.gpu
SLACK = 64
EE32, EE64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
p = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


def _dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a.copy()).to(dev)


# ------------------------------------------------------------------------------------------------ parse
def _parse_once(ctx, d_text, d_off, d_end, n, cap):
    torch, eng, dev = ctx
    d_ops = torch.full((cap + SLACK,), -0x11111112, dtype=torch.int32, device=dev)
    d_opoff = torch.full((n + 1 + SLACK,), -0x1111111111111112, dtype=torch.int64, device=dev)
    d_st = torch.full((n + SLACK,), 0xEE, dtype=torch.uint8, device=dev)
    d_scr = torch.zeros(eng.text_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = eng.L.rb_dev_parse_cigars(eng.ctx, p(d_text.data_ptr()), p(d_off.data_ptr()), p(d_end.data_ptr() if d_end is not None else 0), C.c_uint64(n),
                                   p(d_opoff.data_ptr()), p(d_ops.data_ptr()), C.c_uint64(cap + SLACK), p(d_st.data_ptr()), p(d_scr.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0
    return d_opoff.cpu().numpy().view(np.uint64), d_ops.cpu().numpy().view(np.uint32), d_st.cpu().numpy()


def parse(ctx, buf, off, end):
    """two calls on fresh sentinel buffers -> (op_off, ops, status), sentinels included"""
    torch, eng, dev = ctx
    assert len(buf) % 16 == 0
    d_text = _dev(torch, dev, np.frombuffer(buf, np.uint8))
    assert d_text.data_ptr() % 16 == 0 and d_text.numel() == len(buf)
    n = len(end) if end is not None else len(off) - 1
    d_off, d_end = _dev(torch, dev, off), (_dev(torch, dev, end) if end is not None else None)
    a = _parse_once(ctx, d_text, d_off, d_end, n, len(buf) // 2)
    b = _parse_once(ctx, d_text, d_off, d_end, n, len(buf) // 2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    return a


def check_parse(Lo, got, what):
    """every record against the reference: status in its set; status 0: its ops; op_off monotonic and exact for every valid record"""
    op_off, ops, status = got
    n = len(Lo.cases)
    refs, allowed = Lo.expected()
    assert (op_off[n + 1:] == EE64).all() and (status[n:] == 0xEE).all(), what
    assert int(op_off[0]) == 0 and (np.diff(op_off[:n + 1].astype(np.int64)) >= 0).all(), what
    total = int(op_off[n])
    assert (ops[total:] == EE32).all(), what
    for i, c in enumerate(Lo.cases):
        st, a, b = int(status[i]), int(op_off[i]), int(op_off[i + 1])
        assert st in allowed[i], (what, c.name, st, sorted(allowed[i]))
        if refs[i] is not None and max(ln for ln, _ in refs[i] + [(0, 0)]) < 1 << tu.LEN_BITS:
            assert b - a == len(refs[i]), (what, c.name)     # (the count is exact whatever the status)
        if st == 0:
            assert np.array_equal(ops[a:b], tu.ref_words(refs[i])), (what, c.name)


def run_layout(ctx, name, fills=("paf",)):
    Lo = tu.layout(name)
    first = None
    for f in fills:
        got = parse(ctx, Lo.buffer(f), Lo.off, Lo.end)
        check_parse(Lo, got, f"{name} fill={f}")
        if first is None:
            first = got
        else:                                                     # nothing outside a string decides anything
            for x, y in zip(first, got):
                assert np.array_equal(x, y), (name, f)
    raw, off = Lo.back_to_back()
    check_parse(Lo, parse(ctx, raw, off, None), f"{name} back to back")
    return first


def test_parse_start_phase_x_end_phase_with_hostile_gaps(ctx):
    """every start phase x lengths 0 .. 40 and ends on and next to the two step boundaries; digits, op characters, `cg:Z:` ... tab and
    0xFF between the strings give the same op_off, ops and status, the reference's"""
    op_off, ops, status = run_layout(ctx, "phases", tu.FILLS)
    Lo = tu.layout("phases")
    for i, c in enumerate(Lo.cases):
        assert int(status[i]) == (0 if len(c.s) != 1 else 1), c.name


def test_parse_every_split_of_every_number(ctx):
    """k digits of a d-digit number in front of a lane boundary, the first and the second step boundary, d - k behind it: status 0
    exactly (no string has a run of ten digits) and the reference's ops"""
    op_off, ops, status = run_layout(ctx, "splits", ("nine", "paf"))
    assert not status[:len(tu.layout("splits").cases)].any()


def test_parse_two_to_the_28_at_every_split(ctx):
    """the value put together from two lanes, or from the carry of the step before, reaches the check for lengths the packed form
    cannot hold"""
    op_off, ops, status = run_layout(ctx, "splits-2^28", ("nine", "paf"))
    assert (status[:len(tu.layout("splits-2^28").cases)] == 2).all()


def test_parse_full_steps(ctx):
    """eight ops in every lane, 512 in the stage of a step, the record ending one op short of, on and one op behind a step seam"""
    op_off, ops, status = run_layout(ctx, "full-steps", ("letter", "paf"))
    assert not status[:len(tu.layout("full-steps").cases)].any()


def test_parse_all_256_byte_values(ctx):
    """every byte value where a digit and where an op character belongs, on the even and the odd byte of a pair: status 0 with the
    reference's ops exactly where the reference accepts, 1 or 3 otherwise"""
    op_off, ops, status = run_layout(ctx, "bytes", ("paf", "nine"))
    Lo = tu.layout("bytes")
    refs, _ = Lo.expected()
    for i, c in enumerate(Lo.cases):
        assert (int(status[i]) == 0) == (refs[i] is not None) and int(status[i]) in (0, 1, 3), (c.name, int(status[i]))


def test_parse_status_at_the_seams(ctx):
    """what is wrong with a string found across a lane and a step boundary, runs of 9 / 10 / 16 digits inside a chunk, across two and
    across a step, the precedence of the statuses; the good neighbours of every bad record keep status 0 and their ops"""
    op_off, ops, status = run_layout(ctx, "status", tu.FILLS)
    Lo = tu.layout("status")
    for i, c in enumerate(Lo.cases):
        if c.name == "good":
            assert int(status[i]) == 0
        elif c.name.startswith("run9-"):
            assert int(status[i]) == 0, c.name
        elif c.name.startswith("run"):
            assert int(status[i]) in (0, 3), c.name


@pytest.mark.parametrize("n_rec", tu.N_REC)
def test_parse_record_count_seams(ctx, n_rec):
    """four records a block, 2048 records a block of the scan: op_off exact up to op_off[n_rec]"""
    name = f"count-{n_rec}"
    Lo = tu.layout(name)
    op_off, ops, status = run_layout(ctx, name)
    refs, _ = Lo.expected()
    want = np.zeros(n_rec + 1, np.uint64)
    want[1:] = np.cumsum([len(r) for r in refs])
    assert np.array_equal(op_off[:n_rec + 1], want) and not status[:n_rec].any()
    assert np.array_equal(ops[:int(want[-1])], np.concatenate([tu.ref_words(r) for r in refs]))


# ------------------------------------------------------------------------------------------------ format
def run_format(ctx, name):
    torch, eng, dev = ctx
    F = tu.format_set(name)
    want_off, want = F.expected()
    nbytes = len(want)
    size = ((nbytes + 15) & ~15) + SLACK
    d_text = torch.full((size,), 0xEE, dtype=torch.uint8, device=dev)
    assert d_text.data_ptr() % 16 == 0
    d_toff = torch.full((F.n + 1 + SLACK,), -0x1111111111111112, dtype=torch.int64, device=dev)
    d_ops, d_alt = _dev(torch, dev, F.ops), (_dev(torch, dev, F.alt) if F.alt is not None else None)
    d_first, d_count = _dev(torch, dev, F.first), _dev(torch, dev, F.count)
    d_fl, d_ll = (_dev(torch, dev, F.fl) if F.fl is not None else None), (_dev(torch, dev, F.ll) if F.ll is not None else None)
    d_scr = torch.zeros(eng.text_scratch_bytes(F.n) + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: p(t.data_ptr() if t is not None else 0)
    rc = eng.L.rb_dev_format_cigars(eng.ctx, ptr(d_ops), ptr(d_alt), C.c_uint64(F.n), ptr(d_first), ptr(d_count), ptr(d_fl), ptr(d_ll), ptr(d_toff),
                                    ptr(d_text), C.c_uint64(size), ptr(d_scr))
    torch.cuda.synchronize()
    assert rc == 0
    toff = d_toff.cpu().numpy().view(np.uint64)
    assert np.array_equal(toff[:F.n + 1], want_off) and (toff[F.n + 1:] == EE64).all(), name
    got = d_text.cpu().numpy().tobytes()
    if got != want + b"\xEE" * (size - nbytes):                   # the whole buffer; which item, for the message
        for i in range(F.n):
            a, b = int(want_off[i]), int(want_off[i + 1])
            assert got[a:b] == want[a:b], (name, i, None if F.tags is None else F.tags[i], got[a:b][:80], want[a:b][:80])
        assert got[nbytes:] == b"\xEE" * (size - nbytes), (name, "behind text_off[n_items]")
    return F


def test_format_output_phase_x_step_bytes(ctx):
    """items of 2 .. 48 bytes at every output phase: the byte loop, whole 16-byte groups with a head, a tail, both and neither; a store
    outside an item's bytes shows in its neighbour or in the sentinel"""
    run_format(ctx, "phase-x-bytes")


def test_format_255_word_seam_with_first_and_last_len(ctx):
    """items whose last step prints 1, 2, 255 and 256 words, with first_len, last_len, both and neither"""
    run_format(ctx, "255-seam")


def test_format_two_source_arrays(ctx):
    """ops and ops_alt hold different words at every index; the four items of a block take every pattern of the two"""
    run_format(ctx, "two-arrays")


def test_format_continuation_words_through_both_arrays(ctx):
    """an op and its continuation word around the 255-word seam, as the last two words and as the whole of an item, in ops and in
    ops_alt; a continuation word behind an item's last op is not the item's"""
    run_format(ctx, "continuation")


def test_format_every_digit_pattern(ctx):
    """every length 1 .. 99999, every value of the digits above the low four with 0000 and 9999 below, twenty ten-digit lengths"""
    run_format(ctx, "digits")
