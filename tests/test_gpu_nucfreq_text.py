"""rb_dev_nucfreq_text on hand-made counts (no pileup) against the plain-Python model of tests/nftext_util.py: the three segment
arrays and the WHOLE text buffer, the bytes behind its end included.  tests/test_nucfreq_text_inputs.py holds the model to the oracle
and checks that the cases contain what their names say."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import rustybam_amd
import nftext_util as nu

pytestmark = pytest.mark.gpu

SLACK = 80  # sentinel bytes kept behind the text a call is told it has
RB_E_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


@pytest.fixture(scope="module")
def shape():
    S, W, pre_max, suf_max = rustybam_amd.nucfreq_text_shape()
    assert S == 64 and W % S == 0 and pre_max == 255 and suf_max == 255
    return S, W


_cache = {}


def case_and_truth(name, S, W):
    """(case, model outputs): computed once, shared by the tests, never changed"""
    if name not in _cache:
        c = nu.get_case(name, S, W)
        c.name = name
        _cache[name] = (c, nu.model(c))
    return _cache[name]


def run(ctx, case, cap="exact", text_null=False, junk=0xEE, seg_arrays=None, mode=None, total=None):
    """one rb_dev_nucfreq_text call on buffers that hold `junk` everywhere; returns rc, the three arrays and the whole text buffer"""
    torch, eng, dev = ctx
    n_seg = len(case.seg_n)
    strings, po, pl, so, sl = nu.pack_strings(case)
    if total is None:
        total = len(_cache[case.name][1][0])
    cap = total if cap == "exact" else int(cap)
    d_counts = torch.from_numpy(np.concatenate([case.counts.reshape(-1), np.zeros(16, np.uint32)]).view(np.int32)).to(dev)
    d_strings = torch.from_numpy(np.frombuffer(strings, np.uint8).copy()).to(dev)
    d_off = torch.full(((n_seg + 1) * 8,), junk, dtype=torch.uint8, device=dev)
    d_first = torch.full((max(n_seg, 1) * 8,), junk, dtype=torch.uint8, device=dev)
    d_lines = torch.full((max(n_seg, 1) * 8,), junk, dtype=torch.uint8, device=dev)
    d_text = torch.full((max(total, cap) + SLACK,), junk, dtype=torch.uint8, device=dev)
    scr_bytes = eng.nucfreq_text_scratch_bytes(n_seg, int(case.seg_n.sum()))
    d_scr = torch.full((scr_bytes + 512,), junk, dtype=torch.uint8, device=dev)
    scr = (d_scr.data_ptr() + 255) & ~255
    assert d_counts.data_ptr() % 16 == 0 and d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    a = dict(seg_cnt=case.seg_cnt, seg_pos=case.seg_pos, seg_n=case.seg_n, pre_off=po, pre_len=pl, suf_off=so, suf_len=sl)
    a.update(seg_arrays or {})
    rc = eng.dev_nucfreq_text(d_counts.data_ptr(), a["seg_cnt"], a["seg_pos"], a["seg_n"], d_strings.data_ptr(), a["pre_off"], a["pre_len"], a["suf_off"],
                              a["suf_len"], case.mode if mode is None else mode, d_off.data_ptr(), d_first.data_ptr(), d_lines.data_ptr(),
                              0 if text_null else d_text.data_ptr(), cap, scr, check=False)
    torch.cuda.synchronize()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    return SimpleNamespace(rc=rc, off=u64(d_off), first=u64(d_first)[:n_seg], lines=u64(d_lines)[:n_seg], text=d_text.cpu().numpy().tobytes(),
                           scratch_tail=bytes(d_scr.cpu().numpy()[scr - d_scr.data_ptr() + scr_bytes:]), cap=cap, total=total, junk=junk)


def check_arrays(o, truth, what):
    text, off, first, lines, _ = truth
    assert o.rc == 0, what
    assert np.array_equal(o.off, off), f"{what}: seg_text_off"
    assert np.array_equal(o.first, first), f"{what}: seg_first"
    assert np.array_equal(o.lines, lines), f"{what}: seg_lines"
    assert set(o.scratch_tail) <= {o.junk}, f"{what}: bytes behind the scratch were written"


@pytest.mark.parametrize("name", nu.CASE_NAMES)
def test_case_equals_model(ctx, shape, name):
    """digit seams, output phases, run lengths, coverage patterns, many short segments, overlapping segments, a seg_cnt layout out of
    order and the --small orders: all three arrays, and the text buffer byte for byte up to and behind its end"""
    case, truth = case_and_truth(name, *shape)
    o = run(ctx, case)
    check_arrays(o, truth, name)
    text = truth[0]
    got = o.text
    if got[:len(text)] != text:
        k = next(i for i in range(len(text)) if got[i] != text[i])
        raise AssertionError(f"{name}: text differs at byte {k} of {len(text)}: got {got[max(0, k - 40):k + 40]!r}, want {text[max(0, k - 40):k + 40]!r}")
    assert got[len(text):] == bytes([o.junk]) * SLACK, f"{name}: bytes behind the text were written"


@pytest.mark.parametrize("name", ["many_short-full", "run_lengths-small", "phases-full"])
@pytest.mark.parametrize("cap_of", ["0", "1", "15", "16", "half", "exact-1", "exact"])
def test_capacity(ctx, shape, name, cap_of):
    """whatever text_cap is: RB_OK, the arrays exact, nothing at or behind text[text_cap], every segment that ends at or in front of the
    last 16-byte boundary <= text_cap whole, and below the cap a byte is either untouched or the right one"""
    case, truth = case_and_truth(name, *shape)
    text, off = truth[0], truth[1]
    total = len(text)
    cap = {"0": 0, "1": 1, "15": 15, "16": 16, "half": total // 2 + 3, "exact-1": total - 1, "exact": total}[cap_of]
    o = run(ctx, case, cap=cap)
    check_arrays(o, truth, f"{name} cap {cap}")
    got = o.text
    assert got[cap:] == bytes([o.junk]) * (len(got) - cap), f"{name}: a byte at or behind text[{cap}] was written"
    lim = cap & ~15
    whole = [s for s in range(len(case.seg_n)) if int(off[s + 1]) <= lim]
    for s in whole:
        a, b = int(off[s]), int(off[s + 1])
        assert got[a:b] == text[a:b], (name, cap, s)
    if cap_of == "half":
        assert 0 < len(whole) < len(case.seg_n)
    g, w = np.frombuffer(got[:cap], np.uint8), np.frombuffer(text[:cap], np.uint8)
    assert ((g == w) | (g == o.junk)).all()
    if cap == total:
        assert got[:total] == text


@pytest.mark.parametrize("name", ["coverage-full", "many_short-small"])
def test_sizes_only(ctx, shape, name):
    """text == NULL: the arrays, and no text"""
    case, truth = case_and_truth(name, *shape)
    o = run(ctx, case, text_null=True)
    check_arrays(o, truth, name)
    assert set(o.text) <= {o.junk}


@pytest.mark.parametrize("name", ["phases-full", "many_short-full", "coverage-small"])
def test_repeatable_whatever_the_buffers_held(ctx, shape, name):
    """two calls give the same bytes, whatever outputs and scratch held before (0xEE, then 0x00, then 0xFF)"""
    case, truth = case_and_truth(name, *shape)
    text = truth[0]
    for junk in (0xEE, 0x00, 0xFF):
        o = run(ctx, case, junk=junk)
        check_arrays(o, truth, f"{name} junk {junk:#x}")
        assert o.text[:len(text)] == text and o.text[len(text):] == bytes([junk]) * SLACK


def test_empty_calls(ctx):
    """n_seg == 0, and segments of no positions only"""
    none = nu.make_case("none", nu.FULL, np.zeros((0, 4)), [])
    o = run(ctx, none, total=0)
    assert o.rc == 0 and int(o.off[0]) == 0 and set(o.text) == {0xEE}
    empties = nu.make_case("empties", nu.FULL, np.zeros((4, 4)), [(0, 5, 0, b"a\t", b"\n"), (3, 1 << 32, 0, b"b\t", b"\n")])
    o = run(ctx, empties, total=0)
    assert o.rc == 0 and not o.off.any() and not o.lines.any() and (o.first == nu.NONE).all() and set(o.text) == {0xEE}


def test_refusals(ctx, shape):
    """RB_E_INVALID: a segment that reaches behind 2^32, a prefix or a suffix of more than 255 bytes, a mode that is neither, a NULL
    pointer that is needed, a misaligned buffer -- and nothing is written"""
    torch, eng, dev = ctx
    case, truth = case_and_truth("overlapping-full", *shape)
    _, po, pl, so, sl = nu.pack_strings(case)

    def refused(**kw):
        o = run(ctx, case, **kw)
        assert o.rc == RB_E_INVALID, kw
        assert set(o.text) == {0xEE} and set(o.off.tobytes()) == {0xEE} and set(o.lines.tobytes()) == {0xEE}
    pos = case.seg_pos.copy()
    pos[2] = (1 << 32) - int(case.seg_n[2]) + 1
    refused(seg_arrays=dict(seg_pos=pos))
    pos[2] = (1 << 32) + 1
    refused(seg_arrays=dict(seg_pos=pos))
    long_pre, long_suf = pl.copy(), sl.copy()
    long_pre[1], long_suf[4] = 256, 256
    refused(seg_arrays=dict(pre_len=long_pre))
    refused(seg_arrays=dict(suf_len=long_suf))
    refused(mode=2)
    refused(mode=-1)
    for k in ("seg_cnt", "seg_pos", "pre_off", "pre_len", "suf_off", "suf_len"):
        refused(seg_arrays={k: None})
    # NULL outputs, NULL scratch, NULL counts, misaligned text: straight through the C ABI
    n = len(case.seg_n)
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    base = (d.data_ptr() + 255) & ~255
    p, u64p, u32p = C.c_void_p, lambda a: a.ctypes.data_as(C.c_void_p), lambda a: a.ctypes.data_as(C.c_void_p)
    torch.cuda.synchronize()

    def call(counts=base, off=base + 4096, first=base + 8192, lines=base + 12288, text=base + 16384, scratch=base + 32768, mode=nu.FULL):
        return eng.L.rb_dev_nucfreq_text(eng.ctx, p(counts), C.c_uint64(n), u64p(case.seg_cnt), u64p(case.seg_pos), u32p(case.seg_n), p(base + 20000),
                                         u32p(po), u32p(pl), u32p(so), u32p(sl), C.c_int(mode), p(off), p(first), p(lines), p(text), C.c_uint64(0), p(scratch))
    assert call(text=0) == 0  # (the call as such is fine: sizes only)
    for kw in (dict(counts=0), dict(off=0), dict(first=0), dict(lines=0), dict(scratch=0), dict(text=base + 16384 + 8), dict(counts=base + 4),
               dict(scratch=base + 32768 + 64)):
        assert call(**kw) == RB_E_INVALID, kw
    torch.cuda.synchronize()
    # --small looks at no string: strings and their arrays may be NULL
    sm, sm_truth = case_and_truth("overlapping-small", *shape)
    o = run(ctx, sm, seg_arrays=dict(pre_off=None, pre_len=None, suf_off=None, suf_len=None))
    check_arrays(o, sm_truth, "small without strings")
    assert o.text[:len(sm_truth[0])] == sm_truth[0]


def test_host_form_on_a_bam(ctx, golden):
    """rb_host_nucfreq_text on the reads of a golden BAM: the slabs' text is the model's on the counts rb_host_nucfreq gives"""
    import nf_util
    torch, eng, dev = ctx
    names, _, rd = nf_util.read_bam(f"{golden}/asm_small.bam")
    tid = names.index("chr22")
    regions = [(tid, 10024000, 10027000), (tid, 10025500, 10026100)]
    rt, st, en = [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions]
    counts, _, ctr = eng.nucfreq(*rd.args(), rt, st, en)
    segs = [(0, 10024000, 1000, b"chr22\t", b"\tr0\n"), (1000, 10025000, 2000, b"chr22\t", b"\tr0\n"), (3000, 10025500, 600, b"chr22\t", b"\tr1\n")]
    for mode in (nu.FULL, nu.SMALL):
        case = nu.make_case("bam", mode, counts, segs)
        strings, po, pl, so, sl = nu.pack_strings(case)
        slabs, _, ctr2 = eng.nucfreq_text(*rd.args(), rt, st, en, case.seg_cnt, case.seg_pos, case.seg_n, strings, po, pl, so, sl, mode)
        text, off, first, lines, _ = nu.model(case)
        assert ctr2 == ctr and int(lines.sum()) > 500 and int(first[0]) > 10024000
        assert [s[0] for s in slabs] == [0] and np.array_equal(slabs[0][1], off) and np.array_equal(slabs[0][2], first)
        assert slabs[0][3] == text


@pytest.mark.parametrize("slab_of", ["half", "below-longest", "one"])
def test_host_form_in_several_slabs(ctx, golden, slab_of):
    """RB_DEBUG_NFT_SLAB lowers the 1 GiB a slab holds.  Half the text: runs of several whole segments; one byte less than the longest
    segment: that segment alone in a slab of its own size; one byte: every segment alone.  The slabs come in segment order and are cut
    where the rule says (whole segments while they fit, one at least), their offsets rebased, the strings those of the right
    segments, the text the model's"""
    import os
    import nf_util
    torch, eng, dev = ctx
    names, _, rd = nf_util.read_bam(f"{golden}/asm_small.bam")
    tid = names.index("chr22")
    rt, st, en = [tid, tid], [10024000, 10025500], [10027000, 10026100]
    counts, _, _ = eng.nucfreq(*rd.args(), rt, st, en)
    segs = [(0, 10024000, 1000, b"chr22\t", b"\tr0\n"), (1000, 10025000, 0, b"x\t", b"\tempty\n"), (1000, 10025000, 1200, b"chr22\t", b"\tr0\n"),
            (2200, 10026200, 800, b"chr22\t", b"\tsecond\n"), (3000, 10025500, 600, b"c\t", b"\tr1\n"), (3100, 10025600, 37, b"c\t", b"\tr2\n")]
    for mode in (nu.FULL, nu.SMALL):
        case = nu.make_case("bam", mode, counts, segs)
        strings, po, pl, so, sl = nu.pack_strings(case)
        text, off, first, lines, _ = nu.model(case)
        off = off.astype(np.int64)
        longest = int(np.diff(off).max())
        slab = {"half": len(text) // 2, "below-longest": longest - 1, "one": 1}[slab_of]
        want, s0 = [], 0
        while s0 < len(segs):
            s1 = s0 + 1
            while s1 < len(segs) and off[s1 + 1] - off[s0] <= slab:
                s1 += 1
            want.append((s0, s1))
            s0 = s1
        os.environ["RB_DEBUG_NFT_SLAB"] = str(slab)
        try:
            slabs, _, _ = eng.nucfreq_text(*rd.args(), rt, st, en, case.seg_cnt, case.seg_pos, case.seg_n, strings, po, pl, so, sl, mode)
        finally:
            del os.environ["RB_DEBUG_NFT_SLAB"]
        assert [(s[0], s[0] + len(s[2])) for s in slabs] == want
        for s0, rel, fst, txt in slabs:
            k = len(fst)
            assert np.array_equal(rel.astype(np.int64), off[s0:s0 + k + 1] - off[s0])
            assert np.array_equal(fst, first[s0:s0 + k]) and txt == text[int(off[s0]):int(off[s0 + k])]
        if slab_of == "half":
            assert len(want) >= 2 and any(b - a > 1 for a, b in want)
        elif slab_of == "below-longest":
            assert any(len(s[3]) == longest > slab and len(s[2]) == 1 for s in slabs)
        else:
            assert len(want) == len(segs)
