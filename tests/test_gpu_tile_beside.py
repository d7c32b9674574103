"""rb_dev_liftover with the tile kernel BESIDE the per-record kernel (rustybam_amd/csrc/capi.hip, lift_common: the context's side stream,
forked and joined with two events) against the same call on one stream (RB_TILE_BESIDE=0, read per call) and against the per-base oracle.

The batches alternate short records (600 .. 2000 ops, the tile kernel's) with long ones (2100 .. 6000 ops, the per-record kernel's), and no
record but the first starts on a multiple of 32 ops: every long record shares its first and its last 128-byte line of input with a short
neighbour, and the two kernels, which now run at the same time, write rows, slot lines, list entries and arena cursors side by side.  The
windows slide along every record at a step scaled to its length, so that a record has 3 .. 8 hits; they are sorted and overlap two deep.

What two calls must agree in: every row byte for byte, but for out_off of a clip that lies in the arenas (the order in which waves take
arena room is not fixed, with one stream or with two), and every clip by content."""
import ctypes as C
import os

import numpy as np
import pytest

import rustybam_amd
import tile_seam_util as u
from devutil import DevBatch
from rbtest_util import batch_args, compare_hits
from test_gpu_tile_seams import descriptors_to_ops

pytestmark = pytest.mark.gpu

MODERN, LEGACY, FUSED, DESC = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY, rustybam_amd.LIFT_FUSED_SCAN, rustybam_amd.LIFT_DESCRIPTORS
HIT_DT = rustybam_amd.HIT_DT


class env:
    """environment variables the library reads per call, for the calls made inside the block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ------------------------------------------------------------------------------------------------ inputs
def lengths(kinds, seed):
    """ops per record: 's' 600 .. 2000, 'l' 2100 .. 6000, 't' 600 .. 700 (several of them make one tile); no record but the first starts on
    a multiple of 32 ops"""
    rng = np.random.default_rng(seed)
    out, at = [], 0
    for k in kinds:
        lo, hi = {"s": (600, 2000), "l": (2100, 6000), "t": (600, 700)}[k]
        n = int(rng.integers(lo, hi + 1))
        if (at + n) % 32 == 0:
            n += 1 if n < hi else -1
        out.append(n)
        at += n
    assert all(x % 32 for x in np.cumsum(out)[:-1])
    return out


def batch_of(kinds, seed, irregular=()):
    lens = lengths(kinds, seed)
    b = u.make_batch([u.record(n, seed + r) for r, n in enumerate(lens)])
    if irregular:  # op 4 in two ops of its type: the same bases, and a record neither clip kernel takes
        new = {}
        for r in irregular:
            c = u.records(b, [r])[0]
            w = int(c[4])
            new[r] = np.concatenate([c[:4], [(((w >> 4) - 1) << 4) | (w & 15), (1 << 4) | (w & 15)], c[5:]]).astype(np.uint32)
        b = u.rebuild(b, new)
        assert all(x % 32 for x in b["op_off"][1:-1].astype(np.int64))
    return b


def windows_of(b):
    """3 .. 8 windows along every record, neighbours overlapping: sorted, two deep, none reaches another record (u.ROOM bases lie between two)"""
    w = []
    for r in range(len(b["t_st"])):
        t0, t1 = int(b["t_st"][r]), int(b["t_en"][r])
        k = 3 + r % 6
        step = (t1 - t0) // k
        a = min(step // 4, u.ROOM // 4)
        w += [(t0 + i * step - a, t0 + (i + 1) * step + a) for i in range(k)]
    return u.as_windows(w)


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


class Case:
    """a batch, its windows, the oracle's answer (made once) and the batch resident on the device"""

    def __init__(self, ctx, oracle, b):
        torch, eng, dev = ctx
        self.b, self.w = b, windows_of(b)
        self.ob = oracle.Batch(*batch_args(b), b["contig"])
        self.want = {p: oracle.liftover(self.ob, *self.w, policy=p) for p in (0, 1)}
        hits = np.bincount(self.want[0][0]["rec"].astype(np.int64), minlength=len(b["t_st"]))
        assert hits.min() >= 3 and hits.max() <= 8, (hits.min(), hits.max())
        self.d = DevBatch(torch, eng, dev, b)
        self.rows_cap = int(hits.sum()) + 64
        n_rec, n_ops = self.d.n_rec, self.d.n_ops
        self.slot_stride = ((n_ops + 31) & ~31) + 32 * n_rec + 64   # capi.hip, slot_stride_of

    def arena_origin(self, policy, slots=None):
        """the first op of out_ops behind the slots: the windows overlap two deep, so the call makes min(2, RB_MS) slots (RB_DEBUG_SLOTS: fewer)"""
        n = min(2, u.RB_MS) if slots is None else min(int(slots), 2, u.RB_MS)
        return 4 * self.rows_cap if policy & DESC else n * self.slot_stride

    def run(self, policy, beside, slots=None):
        """one sized call -> (rows HIT_DT, out ops, counters)"""
        with env(RB_TILE_BESIDE=None if beside else 0, RB_DEBUG_SLOTS=slots):
            rows, out, cnt = self.d.run(self.w, policy=policy, rows_cap=self.rows_cap)
        assert cnt["overflow"] == 0
        r, o = self.d.host_rows(rows, out)
        return r.copy(), o.copy(), cnt

    def check_oracle(self, res, policy, what):
        r, o, _ = res
        if policy & DESC:
            r, o = descriptors_to_ops(self.b, r, o)
        compare_hits(r, o, *self.want[policy & 1], what)


def same_call(a, b, origin, what):
    """rows equal byte for byte except out_off of clips in the arenas (at or behind `origin`); every clip equal by content"""
    (ra, oa), (rb, ob) = a[:2], b[:2]
    assert len(ra) == len(rb), f"{what}: {len(ra)} rows and {len(rb)}"
    ok = ra["status"] == 0
    desc = (ra["flags"] & rustybam_amd.HIT_DESCRIPTOR) != 0
    in_arena = ok & ~desc & (ra["out_off"] >= origin)
    assert np.array_equal(in_arena, (rb["status"] == 0) & ((rb["flags"] & rustybam_amd.HIT_DESCRIPTOR) == 0) & (rb["out_off"] >= origin)), f"{what}: not the same clips lie in the arenas"
    fa, fb = ra.copy(), rb.copy()
    fa["out_off"][in_arena] = 0
    fb["out_off"][in_arena] = 0
    bad = np.flatnonzero((fa.view(np.uint8).reshape(-1, 64) != fb.view(np.uint8).reshape(-1, 64)).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:5]} differ: {ra[bad[:3]]} and {rb[bad[:3]]}"
    words = np.where(desc, 4, ra["out_n"]).astype(np.int64)
    for i in np.flatnonzero(ok):
        x, y = int(ra["out_off"][i]), int(rb["out_off"][i])
        assert np.array_equal(oa[x:x + words[i]], ob[y:y + words[i]]), f"{what}: the clip of row {i} (rec {ra['rec'][i]} win {ra['win'][i]}) differs"


# ------------------------------------------------------------------------------------------------ 1. equal results
@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    return Case(ctx, oracle, batch_of("sl" * 100, 11))


@pytest.mark.parametrize("policy,slots", [(MODERN, None), (FUSED, None), (FUSED | DESC, None), (MODERN | DESC, None), (FUSED | LEGACY, None), (LEGACY, None),
                                          (FUSED, 0), (MODERN, 0)])
def test_beside_equals_one_stream_equals_oracle(mixed, policy, slots):
    what = f"policy {policy:#x} slots {slots}"
    one = mixed.run(policy, False, slots)
    two = mixed.run(policy, True, slots)
    n_tiles = len(u.plan_tiles(mixed.b["op_off"]))
    assert n_tiles > 0 and int(two[2]["phase"][3]) == n_tiles and int(one[2]["phase"][3]) == n_tiles, f"{what}: tiles"
    mixed.check_oracle(one, policy, what + " (one stream)")
    mixed.check_oracle(two, policy, what + " (beside)")
    origin = mixed.arena_origin(policy, slots)
    same_call(one, two, origin, what)
    for k in ("n_hits", "n_generic", "out_ops_needed"):
        assert int(one[2][k]) == int(two[2][k]), f"{what}: counters.{k}"


# ------------------------------------------------------------------------------------------------ 2. both lists fed at once
@pytest.mark.parametrize("policy", [MODERN, FUSED])
def test_both_kernels_feed_the_lists(ctx, oracle, policy):
    """a tile of four short records whose second one is irregular (the tile keeps its longest run and hands the others to the list kernel,
    on the side stream) and an irregular long record (its hits take the generic route from the per-record kernel)"""
    kinds = "sl" * 8 + "tttt" + "ls" * 8
    c = Case(ctx, oracle, batch_of(kinds, 23, irregular=(17, 20)))
    assert kinds[17] == "t" and kinds[20] == "l"
    tiles = u.plan_tiles(c.b["op_off"])
    assert (16, 4, False) in tiles, tiles
    one, two = c.run(policy, False), c.run(policy, True)
    what = f"both lists, policy {policy:#x}"
    c.check_oracle(one, policy, what + " (one stream)")
    c.check_oracle(two, policy, what + " (beside)")
    same_call(one, two, c.arena_origin(policy), what)
    got = [(int(x[2]["n_generic"]), int(x[2]["phase"][3]), int(x[2]["phase"][4])) for x in (one, two)]
    print(f"{what}: (n_generic, tiles, handed back) one stream {got[0]}, beside {got[1]}")
    assert got[0] == got[1], what
    back = u.expected_back(oracle, c.b, c.want[0][0])
    assert back == 2 and got[1][1] == len(tiles), what
    if policy & FUSED:  # (the irregular record shows while the tile streams, not in its set-up: tile_seam_util's model is of the set-up)
        assert got[1][2] >= back, f"{what}: {got[1][2]} records handed back"
    else:
        assert got[1][2] == back, f"{what}: the tile keeps records 18 and 19 and hands 16 and 17 back"
    generic = set(two[0]["rec"][(two[0]["flags"] & rustybam_amd.HIT_GENERIC) != 0].tolist())
    assert got[1][0] > 0 and {17, 20} <= generic, f"{what}: hits of both irregular records take the generic route (records {sorted(generic)})"


# ------------------------------------------------------------------------------------------------ raw calls: no sizing loop, no host sync inside
class Raw:
    """the buffers of rb_dev_liftover calls on one engine: plan, workspace, rows, out; call() enqueues and does not wait"""

    def __init__(self, torch, eng, dev, case, policy, d=None):
        self.torch, self.eng, self.case, self.policy = torch, eng, case, policy
        self.d = d or case.d
        self.plan = eng.plan_create(self.d.op_off_host, self.d.contig_host, *case.w)
        self.rows_cap, self.out_cap = case.rows_cap, eng.plan_out_capacity(self.plan, False)
        self.ws = torch.zeros(eng.plan_workspace_bytes(self.plan, self.rows_cap), dtype=torch.uint8, device=dev)
        self.rows = torch.full((self.rows_cap * 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = torch.full((self.out_cap,), -0x11111112, dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(64, dtype=torch.uint8, device=dev)
        if not policy & FUSED:
            eng.dev_scan_records(self.d.view, 0, self.d.d_norm.data_ptr())
        torch.cuda.synchronize()

    def call(self):
        cp, d = C.c_void_p, self.d
        return int(self.eng.L.rb_dev_liftover(self.eng.ctx, self.plan, C.byref(d.view), cp(d.d_norm.data_ptr()), C.c_int(self.policy), cp(self.ws.data_ptr()),
                                              cp(self.rows.data_ptr()), C.c_uint64(self.rows_cap), cp(self.out.data_ptr()), C.c_uint64(self.out_cap), cp(self.cnt.data_ptr())))

    def result(self, rows=None, out=None):
        """after a synchronisation: (rows HIT_DT, out ops, counters)"""
        cnt = self.cnt.cpu().numpy().view(rustybam_amd.COUNTERS_DT)[0].copy()
        assert cnt["overflow"] == 0
        n = int(cnt["n_hits"])
        r = (self.rows if rows is None else rows)[:n * 64].cpu().numpy().view(HIT_DT).copy()
        return r, (self.out if out is None else out).cpu().numpy().view(np.uint32).copy(), cnt

    def close(self):
        self.eng.plan_destroy(self.plan)


@pytest.fixture(scope="module")
def small(ctx, oracle):
    return Case(ctx, oracle, batch_of("sl" * 30, 37))


@pytest.mark.parametrize("policy", [MODERN, FUSED])
def test_ten_calls_without_a_host_sync(ctx, small, policy):
    """the next call's fills and set-up kernels may not overtake the side stream's work of the call before: one wait at the end, on the
    context's stream alone (rb_ctx_sync)"""
    torch, eng, dev = ctx
    x = Raw(torch, eng, dev, small, policy)
    try:
        assert x.call() == 0
        eng.sync()
        first = x.result()
        small.check_oracle(first, policy, "one call")
        assert [x.call() for _ in range(10)] == [0] * 10
        eng.sync()
        same_call(first, x.result(), small.arena_origin(policy), f"ten calls back to back, policy {policy:#x}")
    finally:
        eng.sync()
        x.close()


def test_the_callers_stream_sees_a_finished_call(ctx, small):
    """copies enqueued on the caller's stream right behind the call, no host sync in between: the stream has waited for the side stream"""
    torch, eng, dev = ctx
    x = Raw(torch, eng, dev, small, FUSED)
    try:
        assert torch.cuda.current_stream().cuda_stream == eng.L.rb_ctx_stream(eng.ctx), "torch's current stream is the engine's"
        assert x.call() == 0
        rows_then = x.rows.clone()
        slot_then = x.out[:small.slot_stride].clone()
        torch.cuda.synchronize()
        r, o, cnt = x.result()
        small.check_oracle((r, o, cnt), FUSED, "synchronised read")
        in_slot0 = (r["status"] == 0) & (r["out_off"] < small.slot_stride)
        used = int((r["out_off"][in_slot0] + r["out_n"][in_slot0]).max())
        assert in_slot0.any() and used > 0
        assert np.array_equal(rows_then.cpu().numpy(), x.rows.cpu().numpy()), "rows copied on the caller's stream behind the call"
        assert np.array_equal(slot_then[:used].cpu().numpy(), x.out[:used].cpu().numpy()), "the first slot's used range copied on the caller's stream behind the call"
        short = np.diff(small.b["op_off"].astype(np.int64))[r["rec"][in_slot0]] <= u.SHORT_MAX
        assert short.any() and not short.all(), "the first slot holds clips of short and of long records"
    finally:
        eng.sync()
        x.close()


# ------------------------------------------------------------------------------------------------ 5. nothing to overlap
@pytest.mark.parametrize("kinds", ["s" * 40, "l" * 40])
def test_nothing_to_overlap(ctx, oracle, kinds):
    """only short records (stream_end == 0) or only long ones (no tiles): the call is the one-stream call either way"""
    c = Case(ctx, oracle, batch_of(kinds, 41))
    for policy in (MODERN, FUSED):
        one, two = c.run(policy, False), c.run(policy, True)
        what = f"all '{kinds[0]}', policy {policy:#x}"
        c.check_oracle(two, policy, what)
        same_call(one, two, c.arena_origin(policy), what)
        assert int(one[2]["phase"][3]) == int(two[2]["phase"][3]) and (int(two[2]["phase"][3]) > 0) == (kinds[0] == "s"), what


# ------------------------------------------------------------------------------------------------ 6. lifetime
def test_fifty_engines_one_call_each(ctx, small):
    torch, _, dev = ctx
    first = None
    for i in range(50):
        eng = rustybam_amd.Engine(0)   # (a stream of its own, and its side stream)
        x = Raw(torch, eng, dev, small, FUSED)
        try:
            assert x.call() == 0, f"engine {i}: {eng.L.rb_ctx_last_error(eng.ctx).decode()}"
            eng.sync()
            res = x.result()
        finally:
            x.close()
            eng.close()
        if first is None:
            first = res
            small.check_oracle(first, FUSED, "engine 0")
        else:
            same_call(first, res, small.arena_origin(FUSED), f"engine {i}")


def test_two_engines_on_two_streams_interleaved(ctx, small):
    torch, _, dev = ctx
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    engs = [rustybam_amd.Engine(0, s.cuda_stream) for s in streams]
    xs = [Raw(torch, e, dev, small, FUSED, d=DevBatch(torch, e, dev, small.b)) for e in engs]
    try:
        rcs = [x.call() for _ in range(4) for x in xs]   # a b a b ..: no wait in between
        assert rcs == [0] * 8
        for e in engs:
            e.sync()
        res = [x.result() for x in xs]
        small.check_oracle(res[0], FUSED, "engine a")
        small.check_oracle(res[1], FUSED, "engine b")
        same_call(res[0], res[1], small.arena_origin(FUSED), "two engines")
    finally:
        for x, e in zip(xs, engs):
            e.sync()
            x.close()
            e.close()
