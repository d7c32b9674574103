"""The capacity contract of rb_dev_liftover / rb_dev_break (include/rustybam_amd.h): `rows [rows_cap]`, `out_ops [out_cap]`, and "on
capacity overflow counters->overflow != 0 and counters say what is needed; the caller enlarges and calls again" -- what the host wrapper
(lift_sized, capi.hip) and every sizing loop of the tests lean on -- and the same for the caps of the text kernels.

A short capacity is only DECLARED: every buffer handed to a short call is as large as the generous call of the same input used, plus
slack, all of it holding a sentinel (DevBatch.run_once).  A store past a declared capacity lands in memory the test owns and shows as
a broken sentinel.  The inputs are tests/capacity_util.py's; tests/test_capacity_inputs.py proves on the CPU what is assumed of them
here (N = the true number of rows, the ops of all clips, which short capacities are short whatever the code does)."""
import ctypes as C
import os

import numpy as np
import pytest

import capacity_util as cu
import rustybam_amd
from devutil import DevBatch
from rbtest_util import batch_args, compare_hits

pytestmark = pytest.mark.gpu
RB_E_CAPACITY = -4


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


# (input, legacy binary-search policy, --max-size, one-walk route); the legacy policy on the inputs where it can matter most
CASES = [(name, legacy, None, False) for name, legacy in (("L-regular", False), ("L-regular", True), ("L-sparse", False), ("L-irregular", False),
                                                          ("L-irregular", True), ("L-few", False))]
CASES += [("B-regular", False, ms, ow) for ms in (0, 100) for ow in (False, True)] + [("B-regular", True, 100, ow) for ow in (False, True)]
CASES += [("B-lopsided", False, 100, ow) for ow in (False, True)] + [("B-irregular", False, ms, ow) for ms in (0, 100) for ow in (False, True)]
IDS = [f"{n}{'-legacy' if lg else ''}{'' if ms is None else f'-max{ms}'}{'-onewalk' if ow else ('' if ms is None else '-twowalks')}" for n, lg, ms, ow in CASES]
case_param = pytest.mark.parametrize("case", CASES, ids=IDS)

_batches, _cases, _generous = {}, {}, {}


class Case:
    """one (input, policy, route): the resident batch, the oracle's truth, and the generous call every short call is sized after"""

    def __init__(self, ctx, oracle, case):
        torch, eng, dev = ctx
        self.torch, self.key = torch, case
        self.name, self.legacy, self.max_size, self.one_walk = case
        self.inp = cu.get_input(oracle, self.name)
        self.t = cu.truth(oracle, self.name, self.legacy, self.max_size)
        if self.name not in _batches:
            _batches[self.name] = DevBatch(torch, eng, dev, self.inp.b)
        self.D = _batches[self.name]
        self.policy = cu.policy_of(self.name, self.legacy, self.one_walk)
        self.is_break = self.max_size is not None
        plan = eng.plan_create(self.D.op_off_host, self.D.contig_host, *(self.inp.windows if self.inp.windows is not None else (None, None, None)))
        try:
            self.plan_out = eng.plan_out_capacity(plan, self.is_break)
        finally:
            eng.plan_destroy(plan)
        self.stride = cu.slot_stride(self.inp.n_ops, self.inp.n_rec)
        # the slots a call with room has (lift_common: two for break-paf, as deep as the windows overlap, at most two, for liftover)
        self.want = (self.plan_out - self.inp.n_ops // 16 - 32 * self.inp.n_rec - (1 << 20)) // self.stride
        assert 1 <= self.want <= 2 and self.want * self.stride + self.inp.n_ops // 16 + 32 * self.inp.n_rec + (1 << 20) == self.plan_out
        self.rows_g, self.out_g = cu.generous(self.inp, self.t, self.plan_out)
        self.alloc_rows, self.alloc_out = self.rows_g + 1, self.out_g + 64

    def call(self, rows_cap, out_cap, policy=None, alloc_out=None):
        """one call; RB_OK and the three guards are asserted for every call made here"""
        o = self.D.run_once(self.inp.windows, self.policy if policy is None else policy, self.max_size, rows_cap, out_cap,
                            alloc_rows=max(self.alloc_rows, rows_cap + 1), alloc_out=max(alloc_out or 0, self.alloc_out, out_cap + 64))
        assert o.rc == 0, (o.rc, self.D.eng.L.rb_ctx_last_error(self.D.eng.ctx))
        self.guards(o)
        assert o.cnt["redo_two_walk"] == 0
        return o

    def guards(self, o):
        assert o.rows_tail_ok, f"{self.key}: a row was written at or behind rows[rows_cap = {o.rows_cap}]"
        assert o.out_tail_ok, f"{self.key}: an op was written at or behind out_ops[out_cap = {o.out_cap}]"
        assert o.ws_tail_ok, f"{self.key}: bytes behind the workspace of rows_cap = {o.rows_cap} were written"

    def rows_of(self, o):
        n = int(o.cnt["n_hits"])
        return o.rows[:n * 64].view(self.torch.int32).view(n, 16)

    def equals_oracle(self, o, what, exact=False):
        """a call without overflow holds the oracle's rows and clips: row count and digest; exact: field by field, for the message"""
        assert o.cnt["overflow"] == 0 and o.cnt["brk_scratch_short"] == 0, (self.key, what)
        assert int(o.cnt["n_hits"]) == self.t.N, (self.key, what, int(o.cnt["n_hits"]), self.t.N)
        rows = self.rows_of(o)
        if exact:
            compare_hits(*self.D.host_rows(rows, o.out), self.t.rows, self.t.ops, f"{self.key} {what}")
        assert self.D.digest(rows, o.out) == self.t.digest(), (self.key, what)

    def generous(self):
        """(a) the call with room for everything, made once per case"""
        if self.key not in _generous:
            o = self.call(self.rows_g, self.out_g)
            self.equals_oracle(o, "generous call", exact=True)
            used, needed = int(o.cnt["out_ops_used"]), int(o.cnt["out_ops_needed"])
            print(f"{self.key}: N {self.t.N} out_ops_used {used} out_ops_needed {needed} rows_cap {self.rows_g} out_cap {self.out_g}")
            assert used <= self.out_g and used >= self.want * self.stride  # (the arenas begin behind the slots)
            _generous[self.key] = dict(used=used, needed=needed)
        return _generous[self.key]

    def converge(self, o, what):
        """(e) from a short call: call again with EXACTLY what the counters report, no margin, while the call overflows.  One further call
        for liftover and two-walk break-paf; one-walk break-paf whose scratch-row cursor ran short (brk_scratch_short) may take six calls
        in all, the host wrapper's limit (tests/test_capacity_inputs.py: the growth rule gets there whatever the schedule)."""
        calls, scratch_short = 1, False
        while o.cnt["overflow"]:
            scratch_short |= bool(o.cnt["brk_scratch_short"])
            assert self.one_walk or not scratch_short
            assert calls < (6 if scratch_short else 2), (self.key, what, calls, int(o.cnt["n_hits"]), int(o.cnt["out_ops_needed"]), o.rows_cap, o.out_cap)
            o = self.call(max(o.rows_cap, int(o.cnt["n_hits"])), max(o.out_cap, int(o.cnt["out_ops_needed"])))
            calls += 1
        self.equals_oracle(o, f"{what}, call {calls}")
        return calls


def get_case(ctx, oracle, case):
    if case not in _cases:
        _cases[case] = Case(ctx, oracle, case)
    _cases[case].generous()
    return _cases[case]


@case_param
def test_generous_call(ctx, oracle, case):
    """(a) overflow == 0, n_hits == N, rows and clips equal the oracle's"""
    c = get_case(ctx, oracle, case)
    g = c.generous()
    # a call gets the slots it wants only from want * slot_stride + 1024 * n_arena ops on (lift_common): "what makes the job fit" is never less
    assert g["needed"] >= c.want * c.stride + 1024 * c.inp.n_arena


@case_param
@pytest.mark.parametrize("which", ["one", "half", "all-but-one"])
def test_rows_too_few(ctx, oracle, case, which):
    """(b) + (e): RB_OK, overflow, nothing written past what was declared, n_hits tells the truth, and a call with what it reports fits"""
    c = get_case(ctx, oracle, case)
    rows_cap = {"one": 1, "half": c.t.N // 2, "all-but-one": c.t.N - 1}[which]
    o = c.call(rows_cap, c.out_g)
    assert o.cnt["overflow"] != 0
    if not c.one_walk:
        assert int(o.cnt["n_hits"]) == c.t.N and o.cnt["brk_scratch_short"] == 0  # the scan total: it does not depend on the capacity
    else:
        assert int(o.cnt["n_hits"]) >= c.t.N
        if o.cnt["brk_scratch_short"]:
            assert int(o.cnt["n_hits"]) > rows_cap
    c.converge(o, f"rows_cap {rows_cap}")


@case_param
def test_rows_exact(ctx, oracle, case):
    """(c) rows_cap == N is enough -- except for one-walk break-paf, whose scratch rows are shared out among cursors: it may say
    brk_scratch_short instead, and on the lopsided batch it must"""
    c = get_case(ctx, oracle, case)
    o = c.call(c.t.N, c.out_g)
    if c.one_walk and (o.cnt["brk_scratch_short"] or c.name == "B-lopsided"):
        assert o.cnt["brk_scratch_short"] != 0 and o.cnt["overflow"] != 0
        assert int(o.cnt["n_hits"]) > c.t.N
        assert c.converge(o, "rows_cap N") <= 6
    else:
        c.equals_oracle(o, "rows_cap N")


@case_param
def test_ops_too_few(ctx, oracle, case):
    """(d) + (e): out_cap too small with rows to spare.  A capacity below the ops of all clips MUST overflow (no two clips share a word);
    above that, whether a call is short depends on how many slots fit -- a value that turns out not to be short is noted and must
    then give the oracle's result."""
    c = get_case(ctx, oracle, case)
    g = c.generous()
    caps = {"no slot, arenas of 1020": c.inp.n_arena * 1024 - 4,
            "a slot less than the generous call": (c.want - 1) * c.stride,  # (one slot_stride short of its arena_origin)
            "half of what the generous call used": (g["used"] // 2) & ~3}
    short = []
    for what, cap in caps.items():
        if cap == 0:
            print(f"{c.key}: '{what}' would be out_cap = 0 (one slot wanted): not exercised")
            continue
        o = c.call(c.rows_g, cap)
        if c.t.clip_ops > cap:
            assert o.cnt["overflow"] != 0, (c.key, what, cap)
        if not o.cnt["overflow"]:
            print(f"{c.key}: out_cap {cap} ({what}) is not short: the clips fit with fewer slots")
            c.equals_oracle(o, what)
            continue
        short.append(what)
        assert int(o.cnt["n_hits"]) == c.t.N and o.cnt["brk_scratch_short"] == 0  # (rows to spare)
        assert int(o.cnt["out_ops_needed"]) > cap, (c.key, what, cap, int(o.cnt["out_ops_needed"]))
        assert c.converge(o, f"out_cap {cap} ({what})") == 2
    assert "no slot, arenas of 1020" in short


@pytest.mark.parametrize("name", ["L-regular", "L-irregular"])
def test_descriptor_mode(ctx, oracle, name):
    """(f) RB_LIFT_DESCRIPTORS keeps 4 words per row in front of the arenas: an out_cap below 4 * rows_cap + 1024 is refused before
    anything is written; at that size short rows behave as in copied-ops mode"""
    c = get_case(ctx, oracle, (name, False, None, False))
    pol = c.policy | rustybam_amd.LIFT_DESCRIPTORS
    out_g = 4 * c.rows_g + 1024 + c.inp.n_arena * (c.t.clip_ops_padded + 1024)  # (the generic kernel's rows still carry real ops)
    o = c.call(c.rows_g, out_g, policy=pol, alloc_out=out_g + 64)
    c.equals_oracle(o, "descriptors, generous")  # (rb_dev_digest_rows expands a descriptor through the batch)
    r = c.D.host_rows(c.rows_of(o), o.out)[0]
    n_desc = int(((r["flags"] & rustybam_amd.HIT_DESCRIPTOR) != 0).sum())
    assert n_desc == int((c.t.rows["status"] == 0).sum()) if name == "L-regular" else n_desc > 0
    # refused: no byte of rows, out or the counters changes
    c.D.d_cnt.fill_(0xAB)
    o = c.D.run_once(c.inp.windows, pol, None, c.rows_g, 4 * c.rows_g + 1020, alloc_rows=c.alloc_rows, alloc_out=out_g + 64)
    assert o.rc == RB_E_CAPACITY
    assert b"4 * rows_cap + 1024" in c.D.eng.L.rb_ctx_last_error(c.D.eng.ctx)
    assert o.cnt.tobytes() == b"\xAB" * 64
    assert bool((o.rows == 0xEE).all().item()) and bool((o.out == -0x11111112).all().item()) and o.ws_tail_ok
    c.D.d_cnt.zero_()
    for rows_cap in (1, c.t.N // 2, c.t.N - 1):
        o = c.call(rows_cap, 4 * rows_cap + 1024, policy=pol, alloc_out=out_g + 64)
        assert o.cnt["overflow"] != 0 and int(o.cnt["n_hits"]) == c.t.N


def test_slots_forced_off(ctx, oracle):
    """(g) RB_DEBUG_SLOTS=0 (read by the library per call): every clip goes through rb_k_copy_clips into the arenas, short and sized"""
    c = get_case(ctx, oracle, ("L-regular", False, None, False))
    cap = (c.t.clip_ops // 2) & ~3  # short whatever the code does: the clips alone are twice that
    os.environ["RB_DEBUG_SLOTS"] = "0"
    try:
        o = c.call(c.rows_g, cap)
        assert o.cnt["overflow"] != 0 and int(o.cnt["n_hits"]) == c.t.N and int(o.cnt["out_ops_needed"]) > cap
        assert c.converge(o, "no slots") == 2
        o = c.call(c.rows_g, c.out_g)
        c.equals_oracle(o, "no slots, generous")
    finally:
        del os.environ["RB_DEBUG_SLOTS"]


def test_host_wrapper_converges(engine, oracle):
    """(h) rb_host_liftover sizes its outputs itself (lift_sized): on L-few its first guess of 16 * n_rec + n_win + 1024 rows is too small
    (tests/test_capacity_inputs.py), so the first attempt overflows and the result comes from a retry"""
    inp, t = cu.get_input(oracle, "L-few"), cu.truth(oracle, "L-few")
    rows, ops, norm, cnt = engine.liftover(*batch_args(inp.b), inp.b["contig"], *inp.windows)
    assert cnt["overflow"] == 0 and int(cnt["n_hits"]) == t.N
    compare_hits(rows, ops, t.rows, t.ops, "L-few through rb_host_liftover")
    rows, ops, norm, cnt = engine.liftover(*batch_args(inp.b), inp.b["contig"], *inp.windows, policy=rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN)
    compare_hits(rows, ops, t.rows, t.ops, "L-few through rb_host_liftover, fused scan")


# ---- the text kernels: ops_cap of rb_dev_parse_cigars, text_cap of rb_dev_format_cigars ----
@pytest.fixture(scope="module")
def text(ctx, oracle):
    torch, eng, dev = ctx
    cigs, parsed, printed = cu.text_items(oracle)
    n = len(cigs)
    raw = b"".join(c.encode() for c in cigs)
    t_off = np.zeros(n + 1, np.int64)
    t_off[1:] = np.cumsum([len(c) for c in cigs])
    op_off = np.zeros(n + 1, np.int64)
    op_off[1:] = np.cumsum([len(p) for p in parsed])
    ops = np.concatenate(parsed).astype(np.uint32)
    from types import SimpleNamespace
    return SimpleNamespace(n=n, raw=raw, t_off=t_off, op_off=op_off, ops=ops, printed=b"".join(printed), total=int(op_off[-1]), nbytes=int(t_off[-1]),
                           d_text=torch.from_numpy(np.frombuffer(raw + b"\0" * 32, np.uint8).copy()).to(dev), d_toff=torch.from_numpy(t_off).to(dev),
                           d_ops=torch.from_numpy(np.concatenate([ops, np.zeros(64, np.uint32)]).view(np.int32)).to(dev),
                           d_first=torch.from_numpy(op_off[:-1].copy()).to(dev), d_count=torch.from_numpy(np.diff(op_off).astype(np.int32)).to(dev),
                           d_scr=torch.zeros(eng.text_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("cap_of", ["0", "half", "total-1", "total"])
def test_parse_ops_cap(ctx, text, cap_of):
    """op_off is exact whatever the cap (the caller sees op_off[n_rec] > ops_cap), the ops below the cap are the oracle's, nothing at or
    behind the cap is written"""
    torch, eng, dev = ctx
    T = text
    cap = {"0": 0, "half": T.total // 2, "total-1": T.total - 1, "total": T.total}[cap_of]
    d_ops = torch.full((T.total + 64,), -0x11111112, dtype=torch.int32, device=dev)
    d_off = torch.full((T.n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((T.n,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = C.c_void_p
    rc = eng.L.rb_dev_parse_cigars(eng.ctx, p(T.d_text.data_ptr()), p(T.d_toff.data_ptr()), p(0), C.c_uint64(T.n), p(d_off.data_ptr()), p(d_ops.data_ptr()),
                                   C.c_uint64(cap), p(d_st.data_ptr()), p(T.d_scr.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(d_off.cpu().numpy(), T.op_off)
    assert not d_st.cpu().numpy().any()
    got = d_ops.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:min(cap, T.total)], T.ops[:min(cap, T.total)])
    assert (got[cap:] == 0xEEEEEEEE).all()


@pytest.mark.parametrize("cap_of", ["0", "half", "bytes-1", "bytes"])
def test_format_text_cap(ctx, text, cap_of):
    """text_off is exact whatever the cap (the caller sees text_off[n_items] > text_cap), nothing at or behind the cap is written, and
    an item that ends at or in front of the last 16-byte boundary below the cap is printed whole (the kernel stores a step of an item
    -- up to 255 ops -- if the step ends at or in front of the cap: every step of such an item does)"""
    torch, eng, dev = ctx
    T = text
    cap = {"0": 0, "half": T.nbytes // 2, "bytes-1": T.nbytes - 1, "bytes": T.nbytes}[cap_of]
    d_text = torch.full((T.nbytes + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert d_text.data_ptr() % 16 == 0
    d_off = torch.full((T.n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    p = C.c_void_p
    rc = eng.L.rb_dev_format_cigars(eng.ctx, p(T.d_ops.data_ptr()), p(0), C.c_uint64(T.n), p(T.d_first.data_ptr()), p(T.d_count.data_ptr()), p(0), p(0),
                                    p(d_off.data_ptr()), p(d_text.data_ptr()), C.c_uint64(cap), p(T.d_scr.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(d_off.cpu().numpy(), T.t_off)
    got = d_text.cpu().numpy().tobytes()
    assert got[cap:] == b"\xEE" * (T.nbytes + 64 - cap)
    whole = [i for i in range(T.n) if int(T.t_off[i + 1]) <= (cap & ~15)]
    for i in whole:
        a, b = int(T.t_off[i]), int(T.t_off[i + 1])
        assert got[a:b] == T.printed[a:b], (cap, i)
    if cap_of == "half":
        assert 0 < len(whole) < T.n
    # below the cap a byte is either untouched or the right one
    g, w = np.frombuffer(got[:cap], np.uint8), np.frombuffer(T.printed[:cap], np.uint8)
    assert ((g == w) | (g == 0xEE)).all()
    if cap == T.nbytes:
        assert got[:T.nbytes] == T.printed
