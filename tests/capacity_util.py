"""Inputs of the capacity tests (tests/test_gpu_capacity.py) and what the oracle says about them (tests/test_capacity_inputs.py proves, on
the CPU, the properties the GPU tests lean on).

The contract under test is include/rustybam_amd.h's: rb_dev_liftover / rb_dev_break write at most rows_cap rows and out_cap ops, say so in
counters->overflow when that is not enough, and report in n_hits / out_ops_needed what is.  Every input is small -- one call plus its
retries -- and chosen for the place in the code where its rows or clips go when room is short:

  L-regular    600 regular records, a tenth of them long (two arenas; the tile kernel and the per-record kernel both run), windows 5 deep:
               three clips in five lose their slot and go through rb_k_copy_clips into the arenas
  L-sparse     the same records under 60 random windows, some of them thousands of bases wide: few rows, large clips, most in their slots
  L-irregular  30 % of the records from the modes wild / mixed / spliced: the generic kernel's arena writes
  L-few        40 long records under a window every 37 bases: one arena, many rows and several passes per record
  B-regular    break-paf, 600 records, one of them with 601 pieces (more than RB_BP_CAP: the two-walk route's second walk takes it)
  B-lopsided   break-paf, 1100 short records (four arenas) of which 24 -- every 44th, so all on schedule slots = 0 mod 4 -- have 301
               pieces each and the others one: in the one-walk route nearly all scratch rows are asked of ONE cursor
  B-irregular  B-regular with 5 % irregular records: the declined list of the one-walk route

Records the reference panics on are kept out of the irregular mixes (their rows differ by route: with the fused scan they carry the
status, the oracle has none).  B-regular and B-irregular hold records whose header disagrees with their CIGAR (break_frac): those have
no rows when the record scan has run first, which is how these two are run (no RB_LIFT_FUSED_SCAN); every other input is run fused."""
from types import SimpleNamespace

import numpy as np

import rustybam_amd
from rbtest_util import batch_args, digest_rows, random_batch, random_windows, sums

RB_BP_CAP = 512      # k_misc.hip: pieces of one record the collect pass of two-walk break-paf keeps
RB_MAX_ARENA = 256   # capi.hip
UNFUSED = ("B-regular", "B-irregular")
KEYS = ("t_st", "t_en", "q_st", "q_en", "strand", "contig")


def n_arena(n_rec):
    """pick_arenas (capi.hip): arenas of out_ops, cursors of the scratch rows"""
    return int(min(max(n_rec // 256, 1), RB_MAX_ARENA))


def slot_stride(n_ops, n_rec):
    """slot_stride_of (capi.hip): ops of one positional slot"""
    return ((n_ops + 31) & ~31) + 32 * n_rec + 64


def grow(have):
    """rb_k_finish: the rows a call whose scratch-row cursor ran short asks for"""
    return have + have // 4 + 1024


def growth_steps(start, target, limit=64):
    """applications of grow() that take `start` to at least `target`"""
    k = 0
    while start < target and k < limit:
        start, k = grow(start), k + 1
    return k


def from_cigars(cigs, m):
    b = {k: np.asarray(m[k]) for k in KEYS}
    b["op_off"] = np.zeros(len(cigs) + 1, np.uint64)
    b["op_off"][1:] = np.cumsum([len(c) for c in cigs])
    b["ops"] = np.concatenate(cigs).astype(np.uint32) if cigs else np.zeros(0, np.uint32)
    return b


def cigars_of(b):
    return [b["ops"][int(b["op_off"][i]):int(b["op_off"][i + 1])] for i in range(len(b["op_off"]) - 1)]


def mix(parts, choice):
    """record i from parts[choice[i]] (batches of one size), the way tests/test_gpu_break_onewalk.py mixes irregular records in"""
    cigs = [cigars_of(p) for p in parts]
    m = {k: np.array([parts[c][k][i] for i, c in enumerate(choice)], dtype=parts[0][k].dtype) for k in KEYS}
    return from_cigars([cigs[c][i] for i, c in enumerate(choice)], m)


def _ok(oracle, b):
    return oracle.normalize(oracle.Batch(*batch_args(b), b["contig"]))["status"] == 0


def _irregular_mix(oracle, rng, base, frac, **kw):
    """`frac` of the records of `base` replaced by records of the modes wild / mixed / spliced (a third each), except where the reference
    would panic on the replacement"""
    n = len(base["op_off"]) - 1
    odd = [random_batch(rng, n, mode, n_contig=1, **kw) for mode in ("wild", "mixed", "spliced")]
    u = rng.random(n)
    choice = np.where(u < frac, 1 + np.minimum((u * 3 / frac).astype(np.int64), 2), 0)
    for k, o in enumerate(odd):
        choice[(choice == k + 1) & ~_ok(oracle, o)] = 0
    return mix([base] + odd, choice), choice != 0


def _deep_windows(b):
    st = np.arange(0, int(b["t_en"].max()), 40, dtype=np.uint64)
    return np.zeros(len(st), np.uint32), st, st + np.uint64(200)  # five windows over every base


def _many_pieces(n_cut, del_len=500):
    """a regular record of n_cut long deletions: n_cut + 1 pieces for every max_size below del_len"""
    cig = []
    for k in range(n_cut):
        cig += [((3 + k % 7) << 4) | 7, (del_len << 4) | 2]
    cig.append((5 << 4) | 7)
    return np.array(cig, np.uint32)


def _replace(b, idx, cig, t_st=100, q_st=7):
    cigs = cigars_of(b)
    m = {k: b[k].copy() for k in KEYS}
    for i in idx:
        cigs[i] = cig
        R, Q = sums(cig)
        m["t_st"][i], m["t_en"][i], m["q_st"][i], m["q_en"][i] = t_st, t_st + R, q_st, q_st + Q
    return from_cigars(cigs, m)


_inputs = {}


def get_input(oracle, name):
    """-> SimpleNamespace(b = the batch, windows = (w_contig, w_st, w_en) or None, max_sizes = break-paf's --max-size values, odd = which
    records are irregular or None)"""
    if name in _inputs:
        return _inputs[name]
    windows, max_sizes, odd = None, (), None
    if name in ("L-regular", "L-sparse"):
        b = random_batch(np.random.default_rng(7101), 600, "regular", n_contig=1, long_frac=0.1)
        windows = _deep_windows(b) if name == "L-regular" else random_windows(np.random.default_rng(7102), b, 60)
    elif name == "L-irregular":
        rng = np.random.default_rng(7103)
        b, odd = _irregular_mix(oracle, rng, random_batch(rng, 600, "regular", n_contig=1, long_frac=0.1), 0.3, long_frac=0.1)
        windows = _deep_windows(b)
    elif name == "L-few":
        b = random_batch(np.random.default_rng(11), 40, "regular", n_contig=1, long_frac=1.0)
        st = np.arange(0, int(b["t_en"].max()), 37, dtype=np.uint64)
        windows = (np.zeros(len(st), np.uint32), st, st + np.uint64(50))
    elif name in ("B-regular", "B-irregular"):
        rng = np.random.default_rng(7104)
        b = random_batch(rng, 600, "regular", n_contig=1, long_frac=0.1, break_frac=0.1)
        if name == "B-irregular":
            b, odd = _irregular_mix(oracle, rng, b, 0.05, long_frac=0.1, break_frac=0.1)
        b = _replace(b, [300], _many_pieces(600))
        if odd is not None:
            odd[300] = False
        max_sizes = (0, 100)
    elif name == "B-lopsided":
        b = random_batch(np.random.default_rng(7105), 1100, "regular", n_contig=1, long_frac=0.0)
        ops = b["ops"].copy()
        long_indel = ((ops & 15) == 1) | ((ops & 15) == 2)
        long_indel &= (ops >> 4) > 100
        ops[long_indel] = (9 << 4) | (ops[long_indel] & 15)  # nobody else has an indel longer than --max-size
        b["ops"] = ops
        cigs = cigars_of(b)
        for i, c in enumerate(cigs):
            R, Q = sums(c)
            b["t_en"][i], b["q_en"][i] = b["t_st"][i] + np.uint64(R), b["q_st"][i] + np.uint64(Q)
        b = _replace(b, list(range(0, 24 * 44, 44)), _many_pieces(300, del_len=300))
        max_sizes = (100,)
    else:
        raise KeyError(name)
    _inputs[name] = SimpleNamespace(name=name, b=b, windows=windows, max_sizes=max_sizes, odd=odd, n_rec=len(b["op_off"]) - 1, n_ops=int(b["op_off"][-1]),
                                    n_arena=n_arena(len(b["op_off"]) - 1))
    return _inputs[name]


_truth = {}


def truth(oracle, name, legacy=False, max_size=None):
    """The oracle's rows and clips of an input, computed once: rows, ops, N = the rows, clip_ops = the ops of all clips (a call cannot fit
    into fewer: no two clips share a word of out_ops), clip_ops_padded = the same with every clip rounded up to a multiple of 4 (what the
    clips would take if all of them went to one arena), digest() = rb_dev_digest_rows' value for these rows (computed on first use)."""
    key = (name, bool(legacy), max_size)
    if key in _truth:
        return _truth[key]
    inp = get_input(oracle, name)
    ob = oracle.Batch(*batch_args(inp.b), inp.b["contig"])
    pol = oracle.LEGACY if legacy else oracle.MODERN
    rows, ops = oracle.liftover(ob, *inp.windows, policy=pol) if inp.windows is not None else oracle.break_paf(ob, max_size, policy=pol)
    ok = rows["status"] == 0
    t = SimpleNamespace(rows=rows, ops=ops, N=len(rows), clip_ops=int(rows["out_n"][ok].astype(np.int64).sum()),
                        clip_ops_padded=int(((rows["out_n"][ok].astype(np.int64) + 3) & ~3).sum()), _digest=None)

    def digest():
        if t._digest is None:
            t._digest = digest_rows(rows, ops)
        return t._digest
    t.digest = digest
    _truth[key] = t
    return t


def policy_of(name, legacy=False, one_walk=False):
    p = rustybam_amd.BSEARCH_LEGACY if legacy else rustybam_amd.BSEARCH_MODERN
    if name not in UNFUSED:
        p |= rustybam_amd.LIFT_FUSED_SCAN
    if one_walk:
        p |= rustybam_amd.BREAK_ONE_WALK
    return p


def generous(inp, t, plan_out_capacity):
    """(rows_cap, out_cap) with which one call fits whatever the schedule: every scratch-row cursor of one-walk break-paf can hold all
    rows, every arena all clips, behind the slots rb_plan_out_capacity counts"""
    return t.N * inp.n_arena + 1024, (plan_out_capacity + inp.n_arena * (t.clip_ops_padded + 1024) + 3) & ~3


# ---- the text kernels ----
def text_items(oracle, n=200, seed=0x7E57):
    """n random CIGAR strings (tests/test_gpu_text.py's generator) with the oracle's parse of each and the oracle's print of that"""
    from test_gpu_text import oracle_format, oracle_parse, rand_cigar
    rng = np.random.default_rng(seed)
    cigs = [rand_cigar(rng, int(k), big=True) for k in rng.integers(0, 40, n - 4)] + [rand_cigar(rng, k) for k in (255, 256, 257, 700)]
    parsed = [oracle_parse(oracle, c) for c in cigs]
    assert all(p is not None for p in parsed)
    printed = [oracle_format(oracle, p) for p in parsed]
    return cigs, parsed, printed
